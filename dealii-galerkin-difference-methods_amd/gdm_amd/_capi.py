"""ctypes binding of libgdm_hip.so (include/gdm_hip.h).

The product path: every device computation goes through these entry points.
There is no CPU fallback -- if the library or a GPU is missing, operator
construction raises GdmError.
"""
import ctypes
import importlib.util
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("GDM_HIP_LIB") or os.path.join(PKG_ROOT, "lib", "libgdm_hip.so")
HEADER = os.path.join(os.path.dirname(PKG_ROOT), "include", "gdm_hip.h")

GDM_OK = 0
GDM_OP_MASS, GDM_OP_ADVECTION, GDM_OP_WAVE, GDM_OP_CONVECTIVE, GDM_OP_ELASTICITY = 0, 1, 2, 3, 4


class GdmError(RuntimeError):
    pass


class MeshDesc(ctypes.Structure):
    _fields_ = [
        ("dim", ctypes.c_int32),
        ("fe_degree", ctypes.c_int32),
        ("n_subdivisions", ctypes.c_int32 * 3),
        ("lo", ctypes.c_double * 3),
        ("hi", ctypes.c_double * 3),
        ("n_ranks", ctypes.c_int32),
        ("rank", ctypes.c_int32),
        ("periodic", ctypes.c_int32),
    ]


class Halo(ctypes.Structure):
    _fields_ = [
        ("rank_below", ctypes.c_int32),
        ("rank_above", ctypes.c_int32),
        ("owned_offset", ctypes.c_int64),
        ("send_below_offset", ctypes.c_int64),
        ("send_below_count", ctypes.c_int64),
        ("recv_below_offset", ctypes.c_int64),
        ("recv_below_count", ctypes.c_int64),
        ("send_above_offset", ctypes.c_int64),
        ("send_above_count", ctypes.c_int64),
        ("recv_above_offset", ctypes.c_int64),
        ("recv_above_count", ctypes.c_int64),
        ("dealii_ghost_planes_below", ctypes.c_int32),
        ("dealii_ghost_planes_above", ctypes.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Layout(ctypes.Structure):
    _fields_ = [
        ("n_dofs_global", ctypes.c_int64),
        ("plane_size", ctypes.c_int64),
        ("n_planes_global", ctypes.c_int32),
        ("owned_plane_begin", ctypes.c_int32),
        ("owned_plane_end", ctypes.c_int32),
        ("ghost_planes_below", ctypes.c_int32),
        ("ghost_planes_above", ctypes.c_int32),
        ("cell_plane_begin", ctypes.c_int32),
        ("cell_plane_end", ctypes.c_int32),
        ("halo_depth", ctypes.c_int32),
        ("n_owned", ctypes.c_int64),
        ("n_local", ctypes.c_int64),
        ("n_bc_points", ctypes.c_int64),
        ("n_bc_points_ref", ctypes.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FieldTerm(ctypes.Structure):
    """gdm_field_term: one term s_t f_0(x_0) f_1(x_1) f_2(x_2) of a velocity component"""
    _fields_ = [
        ("component", ctypes.c_int32),
        ("factor", ctypes.c_void_p * 3),
    ]


class CoefTerm(ctypes.Structure):
    """gdm_coef_term: one term k_0(x_0) k_1(x_1) k_2(x_2) of a coefficient"""
    _fields_ = [("factor", ctypes.c_void_p * 3)]


class MassPathPass(ctypes.Structure):
    _fields_ = [("axis", ctypes.c_int), ("v3", ctypes.c_int), ("segments", ctypes.c_int), ("in_place", ctypes.c_int)]


class MassPath(ctypes.Structure):
    """gdm_mass_path: what the last line passes of the mass inverse launched"""
    _fields_ = [("n_passes", ctypes.c_int), ("rk_mode", ctypes.c_int), ("passes", MassPathPass * 3)]


FIELD_MAX_TERMS = 8
COEF_MAX_TERMS = 4

_lib = None


def torch_hip_runtime():
    """Path of the HIP runtime torch ships (None when torch is absent).

    libgdm_hip.so NEEDs `libamdhip64.so.7` (RUNPATH /opt/rocm/lib) while
    libtorch_hip NEEDs torch's own copy, whose soname is the same
    `libamdhip64.so.7`.  Loaded first, the engine would map /opt/rocm's
    runtime and a later `import torch` a second one (plus a second
    libhsa-runtime64): two HIP runtimes in one process.  Preloading torch's
    copy makes the dynamic linker satisfy the engine's NEEDED entry by soname
    and torch's by file identity, so every Python process maps exactly one.
    """
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return None
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    return path if os.path.exists(path) else None


def load():
    """Load libgdm_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GdmError("libgdm_hip.so not built (%s); run __graft_entry__.build()" % LIB_PATH)
    rt = torch_hip_runtime()
    if rt is not None:
        ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
    L = ctypes.CDLL(LIB_PATH)
    P, i32, i64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    sig = {
        "gdm_last_error": [ctypes.c_char_p, ctypes.c_size_t],
        "gdm_abi_version": [],
        "gdm_get_device_count": [ctypes.POINTER(ctypes.c_int)],
        "gdm_op_create": [ctypes.POINTER(MeshDesc), i32, P, i32, i32, ctypes.POINTER(P)],
        "gdm_op_destroy": [P],
        "gdm_op_layout": [P, ctypes.POINTER(Layout)],
        "gdm_halo_plan": [ctypes.POINTER(MeshDesc), ctypes.POINTER(Halo)],
        "gdm_mass_diagonal": [P, P],
        "gdm_memcpy_d2d": [P, P, P, ctypes.c_size_t],
        "gdm_vec_pointwise_mult": [P, i64, P, P, P],
        "gdm_op_set_stream": [P, P],
        "gdm_op_use_own_stream": [P],
        "gdm_op_get_stream": [P, P],
        "gdm_apply": [P, P, P, P],
        "gdm_add_boundary_data": [P, P, P],
        "gdm_apply_planes": [P, P, P, i32, i32],
        "gdm_apply_planes2": [P, P, P, i32, i32, i32, i32],
        "gdm_field_points": [ctypes.POINTER(MeshDesc), i32, P],
        "gdm_field_matrix_1d": [ctypes.POINTER(MeshDesc), i32, i32, P, P],
        "gdm_field_tile": [i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                           ctypes.POINTER(ctypes.c_int)],
        "gdm_op_set_advection_field": [P, i32, P],
        "gdm_op_set_field_scale": [P, P],
        "gdm_coef_matrix_1d": [ctypes.POINTER(MeshDesc), d, i32, i32, P, P],
        "gdm_coef_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                          ctypes.POINTER(ctypes.c_int)],
        "gdm_op_set_coefficient": [P, i32, P],
        "gdm_coef_solve": [P, d, d, P, P, d, d, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(d)],
        "gdm_op_set_coefficient_grid": [P, P, P],
        "gdm_coef_grid_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                               ctypes.POINTER(ctypes.c_int)],
        "gdm_coef_grid_tables_1d": [ctypes.POINTER(MeshDesc), i32, P, P, P],
        "gdm_density_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                             ctypes.POINTER(ctypes.c_int)],
        "gdm_density_cholesky_1d": [ctypes.POINTER(MeshDesc), i32, P, P, P],
        "gdm_op_set_density": [P, i32, P],
        "gdm_density_apply": [P, P, P],
        "gdm_density_apply_add": [P, P, d, P, P],
        "gdm_density_solve": [P, P, P, d, d, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(d)],
        "gdm_op_set_density_grid": [P, P],
        "gdm_density_grid_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_int)],
        "gdm_density_diag": [P, P],
        "gdm_op_set_density_grid_z_chunk": [P, i32],
        "gdm_mass_apply": [P, P, P],
        "gdm_mass_solve": [P, P, P],
        "gdm_mass_solve_rk": [P, P, d, P, P, d, P, P],
        "gdm_op_set_mass_seg_waves": [P, i32],
        "gdm_op_mass_path": [P, ctypes.POINTER(MassPath)],
        "gdm_mass_solve_periodic": [P, P, P],
        "gdm_mass_solve_periodic_rk": [P, P, d, P, P, d, P, P],
        "gdm_mass_periodic_tables": [ctypes.POINTER(MeshDesc), i32, P, P, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)],
        "gdm_mass_cholesky_1d": [ctypes.POINTER(MeshDesc), i32, i32, P, P],
        "gdm_constraints_distribute": [P, P],
        "gdm_mass_solve_cg": [P, P, P, d, d, i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(d)],
        "gdm_mass_solve_lines": [P, i32, P, i64, i64, i64, i64, i64],
        "gdm_vec_axpby": [P, i64, d, P, d, P],
        "gdm_vec_dot": [P, i64, P, P, ctypes.POINTER(d)],
        "gdm_vec_rk_update": [P, i64, d, P, P, P, d, P, P],
        "gdm_eval_boundary": [P, i32, P, i32, d, i32, P],
        "gdm_apply_bc_fn": [P, P, P, i32, P, i32, d, d, d],
        "gdm_add_boundary_fn": [P, P, i32, P, i32, d, d, d],
        "gdm_error_norms": [P, P, i32, P, i32, d, P, P],
        "gdm_add_load_fn": [P, i32, P, i32, d, i32, d, P],
        "gdm_add_load": [P, P, d, P],
        "gdm_add_dirichlet_data": [P, P, P],
        "gdm_load_vector_1d": [ctypes.POINTER(MeshDesc), i32, P, P],
        "gdm_load_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                          ctypes.POINTER(ctypes.c_int)],
        "gdm_eval_grid": [P, P, P, P],
        "gdm_add_load_grad": [P, P, d, P],
        "gdm_eval_trace": [P, P, P, P],
        "gdm_eval_grid_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                               ctypes.POINTER(ctypes.c_int)],
        "gdm_fastdiag_tables": [ctypes.POINTER(MeshDesc), d, i32, P, P],
        "gdm_system_solve_setup": [P],
        "gdm_system_solve": [P, d, d, P, P],
        "gdm_fastdiag_transform": [P, i32, i32, P, P],
        "gdm_elasticity_tile": [i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                ctypes.POINTER(ctypes.c_int)],
        "gdm_elasticity_tables_1d": [ctypes.POINTER(MeshDesc), i32, P, P, P],
        "gdm_elasticity_diagonal": [P, P],
        "gdm_elasticity_precond_setup": [P],
        "gdm_elasticity_precond": [P, P, P],
        "gdm_elasticity_solve": [P, P, P, i32, d, d, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(d)],
        "gdm_vec_interleave": [P, i32, i32, P, P],
        "gdm_error_norms_grid": [P, P, P, P, P],
        "gdm_mass_spike_eps": [P, P],
        "gdm_mass_solve_slab": [P, P, P],
        "gdm_mass_solve_interface": [P, P],
        "gdm_mass_solve_interface_ghosts": [P, P],
        "gdm_mass_solve_interface_rk": [P, P, d, P, P, d, P, P],
        "gdm_mass_solve_interface_round": [P, P, i32],
        "gdm_mass_spike_rounds": [P, ctypes.POINTER(ctypes.c_int)],
        "gdm_synchronize": [P],
        "gdm_malloc": [P, ctypes.c_size_t, ctypes.POINTER(P)],
        "gdm_free": [P, P],
        "gdm_memcpy_h2d": [P, P, P, ctypes.c_size_t],
        "gdm_memcpy_d2h": [P, P, P, ctypes.c_size_t],
        "gdm_bc_points": [P, P],
        "gdm_bc_reference_order": [P, P],
        "gdm_time_op": [P, i32, P, P, P, i32, ctypes.POINTER(d)],
        "gdm_csr_create": [i32, i64, i64, i64, P, P, P, i32, ctypes.POINTER(P)],
        "gdm_csr_destroy": [P],
        "gdm_csr_info": [P, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)],
        "gdm_csr_set_stream": [P, P],
        "gdm_csr_set_lanes": [P, i32],
        "gdm_csr_kernel": [P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
        "gdm_csr_download": [P, P, P, P],
        "gdm_csr_vmult": [P, P, P],
        "gdm_csr_cg": [P, P, P, i32, i32, d, d, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(d)],
        "gdm_csr_read_triplets": [i32, ctypes.c_char_p, i32, ctypes.POINTER(P)],
        "gdm_csr_write_triplets": [P, ctypes.c_char_p, i32],
        "gdm_csr_time_vmult": [P, P, P, i32, ctypes.POINTER(d)],
        "gdm_cut_poisson_create": [i32, i32, d, d, P, d, i32, d, d, ctypes.POINTER(P)],
        "gdm_cut_poisson_info": [P, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64),
                                 ctypes.POINTER(i64)],
        "gdm_cut_poisson_matrix": [P, i32, ctypes.POINTER(P)],
        "gdm_cut_poisson_csr": [P, P, P, P],
        "gdm_cut_poisson_rhs": [P, P],
        "gdm_cut_poisson_solve": [P, P, d, d, i32, P, ctypes.POINTER(i32), ctypes.POINTER(d)],
        "gdm_cut_poisson_l2_error": [P, P, ctypes.POINTER(d)],
        "gdm_cut_poisson_destroy": [P],
        "gdm_cut_advection_create": [i32, i32, d, d, P, P, d, d, i32, ctypes.POINTER(P)],
        "gdm_cut_advection_info": [P, ctypes.POINTER(i64), ctypes.POINTER(i64), P, ctypes.POINTER(i64)],
        "gdm_cut_advection_bc_points": [P, P],
        "gdm_cut_advection_op": [P, ctypes.POINTER(P)],
        "gdm_cut_advection_compute_rhs": [P, P, P, P],
        "gdm_cut_advection_mass_solve": [P, P, P],
        "gdm_cut_advection_create2": [i32, i32, d, d, P, P, d, d, i32, i32, i32, ctypes.POINTER(P)],
        "gdm_cut_advection_couple": [P, P, P],
        "gdm_cut_advection_destroy": [P],
        "gdm_cut_wave_create": [i32, i32, i32, d, d, i32, P, i32, i32, d, d, d, i32, ctypes.POINTER(P)],
        "gdm_cut_wave_info": [P, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), P],
        "gdm_cut_wave_points": [P, P, P, P, P],
        "gdm_cut_wave_op": [P, ctypes.POINTER(P)],
        "gdm_cut_wave_compute_rhs": [P, P, P, P, P],
        "gdm_cut_wave_couple": [P, P, P],
        "gdm_cut_wave_mass_apply": [P, P, P],
        "gdm_cut_wave_mass_solve": [P, P, P],
        "gdm_cut_wave_system_solve": [P, d, P, P],
        "gdm_cut_wave_stiffness_solve": [P, P, P],
        "gdm_cut_wave_eval": [P, P, P],
        "gdm_cut_wave_destroy": [P],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    _lib = L
    return L


def last_error():
    buf = ctypes.create_string_buffer(1024)
    load().gdm_last_error(buf, 1024)
    return buf.value.decode(errors="replace")


def check(rc, what=""):
    if rc != GDM_OK:
        raise GdmError("%s failed (%d): %s" % (what, rc, last_error()))
    return rc


def declared_symbols():
    """Every function the public header declares (for the export test)."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(gdm_\w+)\s*\(", txt, flags=re.M)))


def device_count():
    n = ctypes.c_int(0)
    rc = load().gdm_get_device_count(ctypes.byref(n))
    return n.value if rc == GDM_OK else 0


def mesh_desc(dim, fe_degree, n_subdivisions, lo=0.0, hi=1.0, n_ranks=1, rank=0, periodic=0):
    m = MeshDesc()
    m.dim, m.fe_degree = dim, fe_degree
    ns = list(n_subdivisions) if hasattr(n_subdivisions, "__len__") else [n_subdivisions] * dim
    for d in range(3):
        m.n_subdivisions[d] = int(ns[d]) if d < dim else 1
        m.lo[d] = float(lo) if d < dim else 0.0
        m.hi[d] = float(hi) if d < dim else 1.0
    m.n_ranks, m.rank, m.periodic = n_ranks, rank, periodic
    return m


def field_points(mesh, axis):
    """The n_sub (p+1) + 2 abscissae at which a field factor along `axis` is
    sampled: lo, the Gauss points cell by cell, hi (pure host, no GPU)."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("field_points: axis outside [0, dim)")
    x = np.zeros(mesh.n_subdivisions[axis] * (mesh.fe_degree + 1) + 2)
    check(load().gdm_field_points(ctypes.byref(mesh), int(axis), x.ctypes.data_as(ctypes.c_void_p)),
          "gdm_field_points")
    return x


def field_matrix_1d(mesh, axis, which, f=None):
    """Band [n_sub + 1][2p+1] of M[f] (which = 0) or C[f] (which = 1) along
    `axis`; f sampled at field_points (None: f = 1).  Pure host, no GPU."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("field_matrix_1d: axis outside [0, dim)")
    n = mesh.n_subdivisions[axis]
    fp = None
    if f is not None:
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.size != n * (mesh.fe_degree + 1) + 2:
            raise GdmError("field_matrix_1d: f has %d samples, field_points has %d"
                           % (f.size, n * (mesh.fe_degree + 1) + 2))
        fp = f.ctypes.data_as(ctypes.c_void_p)
    band = np.zeros((n + 1, 2 * mesh.fe_degree + 1))
    check(load().gdm_field_matrix_1d(ctypes.byref(mesh), int(axis), int(which), fp,
                                     band.ctypes.data_as(ctypes.c_void_p)), "gdm_field_matrix_1d")
    return band


def field_tile(fe_degree):
    """(tile_x, tile_y, z_chunk) of the separable field's volume kernel, kernel axes"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_field_tile(int(fe_degree), *[ctypes.byref(v) for v in t]), "gdm_field_tile")
    return tuple(v.value for v in t)


def coef_matrix_1d(mesh, nitsche, axis, which, f=None):
    """Band [n_sub + 1][2p+1] of M[f] (which = 0) or B[f] (which = 1) of the wave
    operator with a coefficient factor f along `axis` (gdm_coef_matrix_1d); f
    sampled at field_points (None: f = 1).  Pure host, no GPU."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("coef_matrix_1d: axis outside [0, dim)")
    n = mesh.n_subdivisions[axis]
    fp = None
    if f is not None:
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.size != n * (mesh.fe_degree + 1) + 2:
            raise GdmError("coef_matrix_1d: f has %d samples, field_points has %d"
                           % (f.size, n * (mesh.fe_degree + 1) + 2))
        fp = f.ctypes.data_as(ctypes.c_void_p)
    band = np.zeros((n + 1, 2 * mesh.fe_degree + 1))
    check(load().gdm_coef_matrix_1d(ctypes.byref(mesh), float(nitsche), int(axis), int(which), fp,
                                    band.ctypes.data_as(ctypes.c_void_p)), "gdm_coef_matrix_1d")
    return band


def coef_tile(fe_degree, dim):
    """(tile_x, tile_y, z_chunk) of the coefficient kernel, kernel axes"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_coef_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]), "gdm_coef_tile")
    return tuple(v.value for v in t)


def coef_grid_tile(fe_degree, dim):
    """(tile_x, tile_y, z_chunk) of the grid coefficient kernel, kernel axes (gdm_coef_grid_tile)"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_coef_grid_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]), "gdm_coef_grid_tile")
    return tuple(v.value for v in t)


def coef_grid_tables_1d(mesh, axis):
    """(val[Q][p+1], der[Q][p+1], first[Q]) of the grid coefficient kernel along
    `axis`, Q = n_sub (p+1): basis values, physical derivatives and the first
    node of the cell's DoF box per Gauss point (gdm_coef_grid_tables_1d).  Pure
    host, no GPU."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("coef_grid_tables_1d: axis outside [0, dim)")
    n1 = mesh.fe_degree + 1
    Q = mesh.n_subdivisions[axis] * n1
    val, der, first = np.zeros((Q, n1)), np.zeros((Q, n1)), np.zeros(Q, dtype=np.int32)
    check(load().gdm_coef_grid_tables_1d(ctypes.byref(mesh), int(axis), val.ctypes.data_as(ctypes.c_void_p),
                                         der.ctypes.data_as(ctypes.c_void_p),
                                         first.ctypes.data_as(ctypes.c_void_p)), "gdm_coef_grid_tables_1d")
    return val, der, first


def density_tile(fe_degree, dim):
    """(tile_x, tile_y, z_chunk) of the density kernel, kernel axes (gdm_density_tile)"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_density_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]), "gdm_density_tile")
    return tuple(v.value for v in t)


def density_grid_tile(fe_degree, dim):
    """(tile_x, tile_y, z_chunk) of the grid density kernel, kernel axes (gdm_density_grid_tile)"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_density_grid_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]),
          "gdm_density_grid_tile")
    return tuple(v.value for v in t)


def density_cholesky_1d(mesh, axis, f=None):
    """(lrow [N, p+1], invd [N]): the banded Cholesky rows of the weighted 1D
    mass matrix M[f] along `axis`; f sampled at field_points (None: f = 1).
    Pure host, no GPU (gdm_density_cholesky_1d)."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("density_cholesky_1d: axis outside [0, dim)")
    n, p = mesh.n_subdivisions[axis], mesh.fe_degree
    fp = None
    if f is not None:
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.size != n * (p + 1) + 2:
            raise GdmError("density_cholesky_1d: f has %d samples, field_points has %d" % (f.size, n * (p + 1) + 2))
        fp = f.ctypes.data_as(ctypes.c_void_p)
    lrow, invd = np.zeros((n + 1, p + 1)), np.zeros(n + 1)
    check(load().gdm_density_cholesky_1d(ctypes.byref(mesh), int(axis), fp, lrow.ctypes.data_as(ctypes.c_void_p),
                                         invd.ctypes.data_as(ctypes.c_void_p)), "gdm_density_cholesky_1d")
    return lrow, invd


def load_vector_1d(mesh, axis, f=None):
    """The 1D load vector b[i] = sum_q w_q h phi_i(x_q) f(x_q) along `axis`
    (n_sub + 1 entries); f sampled at field_points (None: f = 1; the two end
    values are not read).  Pure host, no GPU (gdm_load_vector_1d)."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("load_vector_1d: axis outside [0, dim)")
    n = mesh.n_subdivisions[axis]
    fp = None
    if f is not None:
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.size != n * (mesh.fe_degree + 1) + 2:
            raise GdmError("load_vector_1d: f has %d samples, field_points has %d"
                           % (f.size, n * (mesh.fe_degree + 1) + 2))
        fp = f.ctypes.data_as(ctypes.c_void_p)
    b = np.zeros(n + 1)
    check(load().gdm_load_vector_1d(ctypes.byref(mesh), int(axis), fp, b.ctypes.data_as(ctypes.c_void_p)),
          "gdm_load_vector_1d")
    return b


def fastdiag_tables(mesh, nitsche, axis):
    """(S, lambda) of the fast diagonalisation along `axis`: the generalised
    eigenpairs A S = M S diag(lambda), S^T M S = I, of the wave operator's 1D
    factor A = L + box Nitsche terms; S [N, N] (column j = eigenvector j),
    lambda ascending.  Pure host, no GPU (gdm_fastdiag_tables)."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("fastdiag_tables: axis outside [0, dim)")
    n = mesh.n_subdivisions[axis] + 1
    S, lam = np.zeros((n, n)), np.zeros(n)
    check(load().gdm_fastdiag_tables(ctypes.byref(mesh), float(nitsche), int(axis), S.ctypes.data_as(ctypes.c_void_p),
                                     lam.ctypes.data_as(ctypes.c_void_p)), "gdm_fastdiag_tables")
    return S, lam


def elasticity_tile(fe_degree, dim=3):
    """(tile_x, tile_y, z_chunk) of the elasticity kernel, kernel axes (gdm_elasticity_tile)"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_elasticity_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]), "gdm_elasticity_tile")
    return tuple(v.value for v in t)


def elasticity_tables_1d(mesh, axis):
    """(bands [4, N, 2p+1], S [N, N], lambda [N]) of direction `axis`: the
    Dirichlet-reduced M, C, C^T, L and the embedded interior eigenpairs of
    (L, M).  Pure host, no GPU (gdm_elasticity_tables_1d)."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("elasticity_tables_1d: axis outside [0, dim)")
    n = mesh.n_subdivisions[axis] + 1
    bands, S, lam = np.zeros((4, n, 2 * mesh.fe_degree + 1)), np.zeros((n, n)), np.zeros(n)
    check(load().gdm_elasticity_tables_1d(ctypes.byref(mesh), int(axis), bands.ctypes.data_as(ctypes.c_void_p),
                                          S.ctypes.data_as(ctypes.c_void_p), lam.ctypes.data_as(ctypes.c_void_p)),
          "gdm_elasticity_tables_1d")
    return bands, S, lam


def load_tile(fe_degree, dim=3):
    """(tile_x, tile_y, z_chunk) of the general load kernel, kernel axes (gdm_load_tile)"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_load_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]), "gdm_load_tile")
    return tuple(v.value for v in t)


def eval_grid_tile(fe_degree, dim=3):
    """(cells_x, cells_y, cells_z) of one work item of the grid evaluation kernel, kernel axes
    (gdm_eval_grid_tile)"""
    t = [ctypes.c_int(0) for _ in range(3)]
    check(load().gdm_eval_grid_tile(int(fe_degree), int(dim), *[ctypes.byref(v) for v in t]), "gdm_eval_grid_tile")
    return tuple(v.value for v in t)


def mass_periodic_tables(mesh, axis):
    """Host tables of the periodic mass inverse along `axis` (pure host, no
    GPU): (T [N-1, 2], m [p], rows_lo, rows_hi), gdm_mass_periodic_tables."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("mass_periodic_tables: axis outside [0, dim)")
    n, p = mesh.n_subdivisions[axis], mesh.fe_degree
    T, m = np.zeros((n, 2)), np.zeros(p)
    lo, hi = ctypes.c_int(0), ctypes.c_int(0)
    check(load().gdm_mass_periodic_tables(ctypes.byref(mesh), int(axis), T.ctypes.data_as(ctypes.c_void_p),
                                          m.ctypes.data_as(ctypes.c_void_p), ctypes.byref(lo), ctypes.byref(hi)),
          "gdm_mass_periodic_tables")
    return T, m, lo.value, hi.value


def mass_cholesky_1d(mesh, axis, periodic=False):
    """(lrow [N, p+1], invd [N]): the banded Cholesky rows of the 1D mass
    matrix along `axis`, or (periodic) of blockdiag(M[0:N-1, 0:N-1], 1) (pure
    host, no GPU; gdm_mass_cholesky_1d)."""
    import numpy as np

    if not 0 <= axis < mesh.dim:
        raise GdmError("mass_cholesky_1d: axis outside [0, dim)")
    N, p = mesh.n_subdivisions[axis] + 1, mesh.fe_degree
    lrow, invd = np.zeros((N, p + 1)), np.zeros(N)
    check(load().gdm_mass_cholesky_1d(ctypes.byref(mesh), int(axis), int(bool(periodic)),
                                      lrow.ctypes.data_as(ctypes.c_void_p), invd.ctypes.data_as(ctypes.c_void_p)),
          "gdm_mass_cholesky_1d")
    return lrow, invd


def mass_spike_rounds(dim, fe_degree, n_subdivisions, n_ranks, lo=0.0, hi=1.0):
    """Refinement rounds (extra p-plane exchanges) the distributed mass
    inverse needs for this partition; -1: refused (pure host, no GPU)."""
    r = ctypes.c_int(0)
    m = mesh_desc(dim, fe_degree, n_subdivisions, lo, hi, n_ranks)
    check(load().gdm_mass_spike_rounds(ctypes.byref(m), ctypes.byref(r)), "gdm_mass_spike_rounds")
    return r.value


def mesh_spike_rounds(m):
    """mass_spike_rounds for an existing gdm_mesh_desc (an operator's .mesh)."""
    r = ctypes.c_int(0)
    check(load().gdm_mass_spike_rounds(ctypes.byref(m), ctypes.byref(r)), "gdm_mass_spike_rounds")
    return r.value


def mass_spike_eps(dim, fe_degree, n_subdivisions, n_ranks, lo=0.0, hi=1.0):
    """Largest coupling the distributed mass inverse's truncated interface
    systems drop (pure host, no GPU); the solve needs <= 1e-15."""
    e = ctypes.c_double(0.0)
    m = mesh_desc(dim, fe_degree, n_subdivisions, lo, hi, n_ranks)
    check(load().gdm_mass_spike_eps(ctypes.byref(m), ctypes.byref(e)), "gdm_mass_spike_eps")
    return e.value

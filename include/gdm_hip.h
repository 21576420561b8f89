/*
 * gdm_hip.h -- C ABI of libgdm_hip.so, the MI355X (gfx950) operator engine for
 * the Galerkin-difference-method (GDM) hot path of
 * peterrum/dealii-galerkin-difference-methods.
 *
 * The reference has no formal FFI: its drop-in surface is the operator classes
 * the RK drivers call plus deal.II's MatrixType concept (vmult).  Each entry
 * point below replaces one of those reference interfaces (paths relative to
 * the reference root):
 *
 *   gdm_op_create        GDM::System<dim>(comm, p, n_comp, ghost) +
 *                        subdivided_hyper_cube + categorize
 *                        (include/gdm/system.h:355-424) and
 *                        Discretization::reinit
 *                        (applications/advection/include/gdm/advection/
 *                        discretization.h:27-89) and
 *                        StiffnessMatrixOperator::reinit (advection/stiffness.h:23-38,
 *                        wave/stiffness.h:23-31) / MassMatrixOperator::reinit
 *                        (advection/mass.h:25-28)
 *   gdm_op_layout        System::locally_owned_dofs / locally_active_dofs and the
 *                        Partitioner (system.h:634-688, 720-757;
 *                        advection/discretization.h:85-88), plus
 *                        StiffnessMatrixOperator::initialize_dof_vector's block(0)
 *                        size (advection/stiffness.h:162-179)
 *   gdm_apply            StiffnessMatrixOperator::compute_rhs (advection:
 *                        advection/stiffness.h:196-606; wave:
 *                        wave/stiffness.h:409-420 -> :42-407), volume + box-face
 *                        terms of the uncut path
 *   gdm_mass_apply       TrilinosWrappers::SparseMatrix::vmult on the matrix of
 *                        MassMatrixOperator::get_sparse_matrix (advection/mass.h:30-36)
 *   gdm_mass_solve       *Problem::solve(mass_matrix, result, rhs)
 *                        (advection/problem.h:236-267, wave/problem.h:471-502):
 *                        the CG + ILU/AMG solve is replaced by the exact
 *                        Kronecker inverse of the uncut mass matrix
 *   gdm_vec_axpby/dot    the vector updates of TimeStepping::ExplicitRungeKutta
 *                        (advection/problem.h:91-94) / SolverCG inner products
 *   gdm_bc_points        StiffnessMatrixOperator::collect_boundary_points
 *                        (advection/stiffness.h:40-160): coordinates of the
 *                        boundary quadrature points (device order)
 *   gdm_bc_reference_order  permutation between the reference's block(0)
 *                        order (cell, face, q) and the device order
 *
 * Conventions: plain pointers and sizes only; every function returns GDM_OK (0)
 * or a negative error code, never throws across the ABI; the message of the
 * last error on the calling thread is available from gdm_last_error.  Vector
 * arguments are DEVICE pointers (hipMalloc'ed or torch CUDA tensors) unless
 * the name says _host.  Calls are ordered on the operator's stream; results
 * that reach host memory are synchronous on return.
 */
#ifndef GDM_HIP_H
#define GDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDM_HIP_ABI_VERSION 19

enum gdm_status {
  GDM_OK = 0,
  GDM_ERR_ARG = -1,         /* invalid argument (AssertThrow in the reference) */
  GDM_ERR_HIP = -2,         /* HIP runtime error */
  GDM_ERR_UNSUPPORTED = -3, /* ExcNotImplemented in the reference */
  GDM_ERR_NOMEM = -4,
  GDM_ERR_STATE = -5
};

/* operator kinds */
enum gdm_op_kind {
  GDM_OP_MASS = 0,       /* (v, u)                                  mass.h:144-156   */
  GDM_OP_ADVECTION = 1,  /* (a u, grad v) - <(a.n) u_up, v>_box     stiffness.h:345-532 */
  GDM_OP_WAVE = 2,       /* -(grad v, grad u) [+ Nitsche on the box] wave/stiffness.h:151-330 */
  GDM_OP_CONVECTIVE = 3, /* -(a . grad u, v)  prototypes/advection_01_gdm.cc:164-206 */
  GDM_OP_ELASTICITY = 4  /* 2 mu (eps(u), eps(v)) + lambda (div u, div v), zero boundary
                            constraints            tests/elasticity_01_gdm.cc:143-184 */
};

typedef struct gdm_op gdm_op;

typedef struct {
  int32_t dim;               /* 1, 2 or 3                                   */
  int32_t fe_degree;         /* odd, 1..9 (fe.h:321-323)                     */
  int32_t n_subdivisions[3]; /* cells per direction                          */
  double lo[3], hi[3];       /* box (subdivided_hyper_cube/_rectangle)       */
  int32_t n_ranks, rank;     /* slab partition along the last coordinate     */
  int32_t periodic;          /* bit d: periodic constraints in direction d
                                (System::make_periodicity_constraints, system.h:427-463:
                                vertex N_d - 1 := vertex 0; gdm_apply / gdm_mass_apply
                                distribute the input and condense the result, the
                                constrained rows are zero; single rank; not with the
                                advection face terms or box Nitsche) */
} gdm_mesh_desc;

/* Local vector layout of one rank.  Device vectors are stored
 * [ghost planes below | owned planes | ghost planes above], each plane
 * lexicographic (x fastest), i.e. the reference's global DoF order
 * (system.h:238-244) restricted to a plane range. */
typedef struct {
  int64_t n_dofs_global;
  int64_t plane_size;             /* DoFs per vertex plane of the last coordinate */
  int32_t n_planes_global;
  int32_t owned_plane_begin;      /* global vertex planes [begin, end) owned   */
  int32_t owned_plane_end;
  int32_t ghost_planes_below;     /* halo depth actually present (<= p)         */
  int32_t ghost_planes_above;
  int32_t cell_plane_begin;       /* owned cell planes (system.h:747-757)       */
  int32_t cell_plane_end;
  int32_t halo_depth;             /* = fe_degree                                */
  int64_t n_owned;                /* owned DoFs                                 */
  int64_t n_local;                /* owned + ghost DoFs                         */
  int64_t n_bc_points;            /* device block(0) size: boundary points of the owned
                                     cells plus, on a multi-rank mesh, those of the
                                     neighbour cells whose DoF boxes reach owned DoFs
                                     (owner-computes replaces compress(add)) */
  int64_t n_bc_points_ref;        /* the reference's block(0) size: points of the owned
                                     cells only (stiffness.h:40-160)                  */
} gdm_layout;

/* Ghost-plane exchange of one rank: owner-computes needs the
 * p vertex planes next to the slab from each z-neighbour (the reference's
 * update_ghost_values + compress(add), advection/stiffness.h:343, 605).  All
 * ranges are in elements of the rank's engine-local vector (gdm_layout);
 * every range is contiguous.  The caller moves them with its own
 * communicator (MPI_Isend/Irecv on device pointers with a GPU-aware MPI,
 * ncclSend/ncclRecv, or torch.distributed, gdm_amd/distributed.py):
 *   send [send_below_offset, + send_below_count) to rank_below, which
 *   receives it into its [recv_above_offset, + recv_above_count), and the
 *   mirror image towards rank_above.
 * deal.II's LinearAlgebra::distributed::Vector stores [owned | ghosts sorted]
 * with the reference's ghost layer (one ghost cell layer: dealii_ghost_planes_
 * below / _above planes, system.h:657-688, 767-771) -- fewer than the p planes
 * owner-computes reads -- so the engine vector is a separate buffer: its owned
 * block starts at owned_offset and equals deal.II's owned block element for
 * element (the reference's global lexicographic order). */
typedef struct {
  int32_t rank_below, rank_above; /* -1: none */
  int64_t owned_offset;           /* = ghost_planes_below * plane_size */
  int64_t send_below_offset, send_below_count;
  int64_t recv_below_offset, recv_below_count;
  int64_t send_above_offset, send_above_count;
  int64_t recv_above_offset, recv_above_count;
  int32_t dealii_ghost_planes_below, dealii_ghost_planes_above;
} gdm_halo;

/* params (n_params):
 *   GDM_OP_MASS        : none
 *   GDM_OP_ADVECTION   : a_x, a_y, a_z               (constant field, see below)
 *   GDM_OP_CONVECTIVE  : a_x, a_y, a_z
 *   GDM_OP_ELASTICITY  : mu, lambda                  (mu > 0, lambda >= 0; see "Linear
 *                                                     elasticity" below)
 *   The reference evaluates advection->value(x_q, d) at every quadrature point
 *   (advection/stiffness.h:395-406, 443, 510).  The params give a CONSTANT
 *   field, which is what every reference preset uses (ConstantFunction,
 *   advection-app.cc:131-139).  A spatially varying field is expressible when
 *   every component is a short sum of products of one-variable functions,
 *   a_d(x, t) = sum_t s_t(t) f_t0(x_0) f_t1(x_1) f_t2(x_2) (solid-body rotation,
 *   shear flows, the deformational swirl): gdm_op_set_advection_field below
 *   replaces a[] by such a sum and the result equals the reference's cell loop
 *   up to summation order.  A general Function<dim> without that structure is
 *   still not expressible: a caller with one must keep the reference's cell
 *   loop (the engine cannot detect it, it only sees what it is given).
 *   GDM_OP_WAVE        : [nitsche_parameter]         (> 0 enables box Nitsche,
 *                        function_domain_dbc; absent / <= 0 = natural BC) */
int gdm_last_error(char *buf, size_t len);
int gdm_abi_version(void);
int gdm_get_device_count(int *n);

int gdm_op_create(const gdm_mesh_desc *mesh, int kind, const double *params, int n_params, int device,
                  gdm_op **out);
int gdm_op_destroy(gdm_op *op);
/* the exchange plan of mesh->rank (pure host function: no device, no op) */
int gdm_halo_plan(const gdm_mesh_desc *mesh, gdm_halo *out);
int gdm_op_layout(const gdm_op *op, gdm_layout *out);
/* launch on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream;
 * NULL is the HIP null stream); gdm_op_use_own_stream restores the operator's
 * private non-blocking stream.  An operator's calls must stay ordered (one
 * stream at a time, or the caller orders the streams): they share the
 * operator's face scratch and the stencil's tail-work counter.  Each call is
 * self-contained otherwise, so it may be captured in a hipGraph and replayed. */
int gdm_op_set_stream(gdm_op *op, void *hip_stream);
int gdm_op_use_own_stream(gdm_op *op);
/* the hipStream_t the operator launches on now (set or own): a communicator
 * orders a device-side ghost exchange after the operator's work on it and
 * makes later work wait for the exchange (RcclRank's split-phase
 * update_ghost_values, advection/stiffness.h:343) -- ABI v10 */
int gdm_op_get_stream(const gdm_op *op, void **hip_stream);

/* dst_owned = K src_local (+ inflow boundary-data term when bc_values != NULL,
 * advection only: bc_values are the stage boundary values, device order, size
 * n_bc_points).  src_local has the full local layout (ghost planes filled). */
int gdm_apply(gdm_op *op, const double *src_local, double *dst_owned, const double *bc_values);
/* The volume part of gdm_apply for the owned output planes [plane_begin,
 * plane_end) of the last coordinate only (global plane indices; 3D).  Lets a
 * multi-rank caller compute the planes that need no ghost data while the
 * ghost-plane exchange is in flight, then the p planes next to each slab edge
 * (the overlap of update_ghost_values, advection/stiffness.h:343, with the cell
 * loop).  Boundary data: gdm_add_boundary_data afterwards. */
int gdm_apply_planes(gdm_op *op, const double *src_local, double *dst_owned, int plane_begin, int plane_end);
/* gdm_apply_planes of two plane ranges [b0, e0) and [b1, e1) in ONE launch
 * (ABI 13): the p planes next to both slab edges after the exchange, so the
 * thin edge ranges share the GPU instead of running one after the other.  The
 * same bits as two gdm_apply_planes calls.  Both ranges are clipped to the
 * owned planes first; an empty (or wholly unowned) range is allowed. */
int gdm_apply_planes2(gdm_op *op, const double *src_local, double *dst_owned, int b0, int e0, int b1, int e1);
/* dst_owned += inflow boundary-data term only (the bc part of gdm_apply,
 * advection/stiffness.h:520-529 with a.n < 0); no-op for other kinds */
int gdm_add_boundary_data(gdm_op *op, const double *bc_values, double *dst_owned);
/* ------------------------------------------------------------------------
 * Separable advection field (ABI 16): a_d(x, t) = sum over the terms t with
 * component d of s_t(t) f_t0(x_0) f_t1(x_1) f_t2(x_2) on a GDM_OP_ADVECTION
 * operator -- advection->value(x_q, d) after advection->set_time(t)
 * (advection/stiffness.h:339, 395-406, 443, 510) for fields of that form.
 * Tensor Gauss quadrature of (a u, grad v) factorises exactly: each term is
 * A_x (x) A_y (x) A_z with the banded 1D matrices C[f] (along the term's
 * component: sum_q w_q f(x_q) phi_i'(x_q) phi_j(x_q)) and M[f] (elsewhere:
 * sum_q w_q f(x_q) phi_i(x_q) phi_j(x_q)); the box-face term takes a.n at
 * every face quadrature point from the same samples.
 *
 *   gdm_field_points     pure host (no device, no op): the n_sub (p+1) + 2
 *                        abscissae along `axis` at which a factor is sampled:
 *                        lo, the Gauss points cell by cell, hi (the two end
 *                        values give the normal flux on the box faces)
 *   gdm_field_matrix_1d  pure host: the band [n_sub + 1][2p+1] (entry [i][k] =
 *                        A(i, i - p + k)) of M[f] (which = 0) or C[f] (which =
 *                        1) the engine uses along `axis`; f sampled at
 *                        gdm_field_points (NULL: f = 1)
 *   gdm_op_set_advection_field
 *                        builds and uploads every table and scratch buffer of
 *                        the field and replaces the constant a[] of
 *                        gdm_op_create; calling it again replaces the field
 *                        (it waits for the operator's stream first);
 *                        n_terms = 0 restores the constant field and its code
 *                        path, bit for bit.  factor[d] are HOST arrays sampled
 *                        at gdm_field_points(d) (NULL = 1; entries d >= dim are
 *                        ignored); at most GDM_FIELD_MAX_TERMS terms; terms that
 *                        pass the same array (pointer identity) share its
 *                        tables and sweeps.  The arrays are copied.
 *   gdm_op_set_field_scale
 *                        the time factors s_t (default 1): host values, not
 *                        baked into the tables; every apply enqueued after the
 *                        call uses them (an RK driver calls it per stage), a
 *                        captured graph keeps the values of its capture.
 * With a field gdm_apply (with and without bc_values), gdm_add_boundary_data,
 * gdm_apply_bc_fn, gdm_add_boundary_fn and gdm_time_op work as before; the mass
 * entry points do not depend on a.  GDM_ERR_UNSUPPORTED: n_ranks > 1, a
 * non-advection operator, the inner operator of a gdm_cut_advection handle,
 * and gdm_apply_planes / gdm_apply_planes2 while a field is set.  GDM_ERR_ARG:
 * n_terms outside [0, GDM_FIELD_MAX_TERMS], component outside [0, dim).
 * gdm_field_tile: the (x, y) tile and the z chunk of the field's volume kernel
 * in kernel axes (pure host; for tests and sizing).
 * ---------------------------------------------------------------------- */
#define GDM_FIELD_MAX_TERMS 8
typedef struct {
  int32_t component;       /* the velocity component this term belongs to */
  const double *factor[3]; /* host arrays at gdm_field_points; NULL = 1     */
} gdm_field_term;
int gdm_field_points(const gdm_mesh_desc *mesh, int axis, double *x_host);
int gdm_field_matrix_1d(const gdm_mesh_desc *mesh, int axis, int which, const double *f, double *band_host);
int gdm_field_tile(int fe_degree, int *tile_x, int *tile_y, int *z_chunk);
int gdm_op_set_advection_field(gdm_op *op, int n_terms, const gdm_field_term *terms);
int gdm_op_set_field_scale(gdm_op *op, const double *s);
/* ------------------------------------------------------------------------
 * Separable coefficient of the wave / heat / Poisson operator: kappa(x) = sum
 * over the terms t of k_t0(x_0) k_t1(x_1) k_t2(x_2) > 0 on a GDM_OP_WAVE
 * operator (dim 1-3, with or without Nitsche terms) -- compute_rhs of
 * wave/stiffness.h:151-330 with every JxW(q) of the operator part (:171-181)
 * and of the box-face part (:296-310) multiplied by kappa at the quadrature
 * point:
 *   K[kappa] u = -(kappa grad v, grad u)
 *                - sum_faces (-<kappa dv/dn, u> - <kappa v, du/dn> + gamma/h_min <kappa v, u>),
 * data term <gamma/h_min v - dv/dn, kappa g_D> (:312-327).  The source term
 * and the mass matrix do not change.  Tensor Gauss quadrature factorises this
 * exactly: per term t and direction d the Kronecker term B_d[k_td] (x)
 * (M_e[k_te], e != d) with M[f]_ij = sum_q w_q f(x_q) phi_i phi_j and B[f] =
 * -L[f] - (f(lo) Nitsche end block of row 0 + f(hi) end block of row N - 1),
 * L[f]_ij = sum_q w_q f(x_q) phi_i' phi_j'.  One kernel launch per apply
 * (csrc/gdm_vardiff.hip), no face kernel, bitwise repeatable.
 *
 *   gdm_coef_matrix_1d   pure host: the band [n_sub + 1][2p+1] of M[f] (which =
 *                        0) or B[f] (which = 1) the engine uses along `axis`
 *                        for the Nitsche parameter `nitsche` (gamma; h_min is
 *                        the mesh's); f sampled at gdm_field_points (NULL: f =
 *                        1, the band of the constant operator)
 *   gdm_coef_tile        pure host: the (x, y) tile and the z chunk of the
 *                        kernel in kernel axes (for tests and sizing)
 *   gdm_op_set_coefficient
 *                        builds and uploads every table and all scratch and
 *                        copies the factor arrays; calling it again replaces
 *                        the coefficient (it waits for the operator's stream
 *                        first); n_terms = 0 restores the constant operator
 *                        and its code path, bit for bit.  factor[d] are HOST
 *                        arrays sampled at gdm_field_points(d) (NULL = 1;
 *                        entries d >= dim are ignored); at most
 *                        GDM_COEF_MAX_TERMS terms; terms that pass the same
 *                        array (pointer identity) share its tables.
 *   gdm_coef_solve       x = (alpha M - tau K[kappa])^-1 rhs by CG with
 *                        ReductionControl(max_it, abs_tol, rel_tol), x the
 *                        initial guess, preconditioned by the fast
 *                        diagonalisation of the constant operator with the
 *                        domain mean of kappa, (alpha M - tau mean(kappa)
 *                        K_0)^-1 (gdm_system_solve's passes; needs
 *                        gdm_system_solve_setup).  Poisson: alpha = 0, tau = 1,
 *                        nitsche > 0; heat-implicit: alpha = 1, tau = dt.
 *                        *its_host = last_step, *res_host = the last residual
 *                        norm (either may be NULL).  GDM_ERR_STATE: max_it
 *                        reached, breakdown (p^T A p <= 0: kappa is not
 *                        positive), no coefficient set, or before
 *                        gdm_system_solve_setup.  rhs != x.
 * While a coefficient is set gdm_apply computes K[kappa] src (bc_values must
 * be NULL), gdm_time_op works, gdm_add_dirichlet_data uses kappa g (kappa at
 * the boundary points follows from the samples: Gauss entries in the
 * tangential directions, the lo / hi entry in the normal one; g_bc is not
 * modified), gdm_add_load* and the mass entry points are unchanged,
 * gdm_system_solve returns GDM_ERR_STATE (the direct solve is the
 * constant-coefficient one: use gdm_coef_solve) and gdm_system_solve_setup
 * stays legal.  GDM_ERR_UNSUPPORTED: another operator kind, n_ranks > 1, a
 * periodic mesh, the inner operator of a cut handle, and gdm_apply_planes /
 * gdm_apply_planes2 while a coefficient is set.  GDM_ERR_ARG: n_terms outside
 * [0, GDM_COEF_MAX_TERMS], a non-finite sample, and for n_terms = 1 a factor
 * that vanishes or changes sign.  For sums the caller guarantees kappa > 0.
 * Separable sums only here: a general coefficient, sampled on the tensor
 * Gauss grid, is set by gdm_op_set_coefficient_grid below.  The density (a
 * weighted mass) is set by gdm_op_set_density below.
 * ---------------------------------------------------------------------- */
#define GDM_COEF_MAX_TERMS 4
typedef struct {
  const double *factor[3]; /* host arrays at gdm_field_points; NULL = 1 */
} gdm_coef_term;
int gdm_coef_matrix_1d(const gdm_mesh_desc *mesh, double nitsche, int axis, int which, const double *f,
                       double *band_host);
int gdm_coef_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk);
int gdm_op_set_coefficient(gdm_op *op, int n_terms, const gdm_coef_term *terms);
int gdm_coef_solve(gdm_op *op, double alpha, double tau, const double *rhs, double *x, double rel_tol,
                   double abs_tol, int max_it, int *its_host, double *res_host);

/* ------------------------------------------------------------------------
 * General coefficient of the wave / heat / Poisson operator: kappa > 0 given
 * pointwise on the tensor Gauss grid, the same K[kappa] and data term as above
 * with kappa evaluated at every quadrature point (csrc/gdm_coefgrid.hip: one
 * volume launch per apply and, with nitsche > 0, two small launches per box
 * face; gather form, bitwise repeatable, nothing allocated per apply, a first
 * apply can be captured in a hipGraph).
 *
 *   gdm_op_set_coefficient_grid
 *       kq   DEVICE array in gdm_add_load's fq layout, kq[(qz Q_y + qy) Q_x +
 *            qx], Q_d = n_sub_d (p+1), x fastest; the abscissae are entries
 *            1..Q_d of gdm_field_points.
 *       kbc  DEVICE array of kappa at the n_bc_points boundary points in device
 *            block(0) order (gdm_bc_points; the order of g_bc of
 *            gdm_add_dirichlet_data).  Required when the operator was created
 *            with nitsche > 0, ignored (may be NULL) otherwise.
 *       Both arrays are BORROWED, not copied: they must outlive the coefficient,
 *       and the caller may overwrite the values in place between applies (a
 *       time- or solution-dependent kappa); the next gdm_apply sees them.  The
 *       call allocates all scratch, waits for the operator's stream and runs one
 *       device reduction over kq (and kbc): GDM_ERR_ARG for a sample that is not
 *       finite or not positive (the coefficient then stays as it was), and the
 *       Gauss-weighted domain mean of kappa is stored for gdm_coef_solve's
 *       preconditioner.  Calling it again with the same pointers refreshes that
 *       mean.  kq == NULL removes the coefficient and restores the constant
 *       operator bit for bit.  A grid coefficient replaces a separable one and
 *       the other way round.
 *   gdm_coef_grid_tile
 *       pure host: the kernel's node tile and z chunk in kernel axes.  A 3D mesh
 *       maps (x, y, z) to the kernel axes (x, y, z); a 2D mesh maps (x, y) to
 *       (x, y) with a trivial z axis; a 1D mesh maps x to the kernel's z axis
 *       with trivial x and y axes.
 *   gdm_coef_grid_tables_1d
 *       pure host: for each of the n_sub (p+1) Gauss points along `axis` the
 *       p+1 basis values val[q (p+1) + i], the p+1 physical derivatives
 *       der[q (p+1) + i] (divided by h) and first[q], the first node of the
 *       cell's DoF box -- the tables the kernel uses.
 * While a grid coefficient is set everything stated above for a separable
 * coefficient holds: gdm_apply computes K[kappa] src (bc_values must be NULL),
 * gdm_time_op(which = 0) times it, gdm_add_dirichlet_data uses kbc . g without
 * modifying g_bc, gdm_coef_solve solves (alpha M - tau K[kappa]) -- (alpha
 * M[rho] - tau K[kappa]) with a separable density set -- preconditioned at the
 * mean of kappa, gdm_system_solve returns GDM_ERR_STATE, gdm_add_load* and the
 * mass entry points are unchanged.  GDM_ERR_UNSUPPORTED: another operator
 * kind, n_ranks > 1, a periodic mesh, the inner operator of a cut handle, and
 * gdm_apply_planes / gdm_apply_planes2 while the coefficient is set.  For a
 * kappa that is a separable sum gdm_op_set_coefficient is the faster path.
 * ---------------------------------------------------------------------- */
int gdm_op_set_coefficient_grid(gdm_op *op, const double *kq, const double *kbc);
int gdm_coef_grid_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk);
int gdm_coef_grid_tables_1d(const gdm_mesh_desc *mesh, int axis, double *val_host, double *der_host,
                            int32_t *first_host);

/* ------------------------------------------------------------------------
 * Separable density of the wave / heat operator: rho(x) = sum over the terms t
 * of r_t0(x_0) r_t1(x_1) r_t2(x_2) > 0 on a GDM_OP_WAVE operator, for
 *   rho u_tt = div(kappa grad u) + f    and    rho c u_t = div(kappa grad u) + f.
 * The weighted mass is M[rho]_ij = sum_q w_q rho(x_q) phi_i phi_j: the cell loop
 * of wave/mass.h:47-249 with every JxW(q) multiplied by rho at the quadrature
 * point.  Tensor Gauss quadrature factorises it exactly, M[rho] = sum_t
 * (x)_d M_d[r_td] with the bands of gdm_coef_matrix_1d(which = 0).  The terms
 * are gdm_coef_term: HOST arrays sampled at gdm_field_points(d) (NULL = 1;
 * entries d >= dim are ignored), at most GDM_COEF_MAX_TERMS terms, terms that
 * pass the same array (pointer identity) share its tables.
 *
 *   gdm_density_tile     pure host: the (x, y) tile and the z chunk of the
 *                        kernel (csrc/gdm_varmass.hip) in kernel axes
 *   gdm_density_cholesky_1d
 *                        pure host: the row-form banded Cholesky factor of
 *                        M_axis[f] in the layout of gdm_mass_cholesky_1d
 *                        (lrow [N][p+1], invd [N]); GDM_ERR_ARG when M[f] is not
 *                        positive definite
 *   gdm_op_set_density   builds and uploads every table and all scratch and
 *                        copies what it needs of the factor arrays; calling it
 *                        again replaces the density (it waits for the
 *                        operator's stream first); n_terms = 0 removes it.
 *   gdm_density_apply    dst = M[rho] src, one kernel launch, bitwise
 *                        repeatable (src != dst)
 *   gdm_density_apply_add
 *                        dst = M[rho] src + c * add in the same launch (add !=
 *                        dst; add may be NULL: the plain apply)
 *   gdm_density_solve    x = M[rho]^-1 rhs.  One term: exact and direct,
 *                        (x)_d M_d[r_d]^-1 by two-sweep line solves with the
 *                        weighted Cholesky factors; *its_host = 0, the
 *                        tolerances are not read, x = rhs is allowed.  A sum:
 *                        CG with ReductionControl(max_it, abs_tol, rel_tol), x
 *                        the initial guess (rhs != x), preconditioned by
 *                        W^-1/2 M^-1 W^-1/2 with W = diag(M[rho]) / diag(M) and
 *                        the exact passes of gdm_mass_solve.  *its_host =
 *                        last_step, *res_host = the last residual norm (either
 *                        may be NULL).  GDM_ERR_STATE: no density set, max_it
 *                        reached, breakdown (p^T M[rho] p <= 0: rho is not
 *                        positive).
 * With a density set gdm_coef_solve solves (alpha M[rho] - tau K[kappa]) x =
 * rhs, with or without a coefficient (none: K[kappa] = K_0), preconditioned by
 * the fast diagonalisation of (alpha mean(rho) M - tau mean(kappa) K_0); the
 * means are Gauss-weighted.  gdm_time_op(which = 3) times gdm_density_apply.
 * Nothing else changes: gdm_apply, gdm_mass_apply, gdm_mass_solve* and
 * gdm_system_solve keep computing with the unweighted M (it is also part of the
 * preconditioners), bit for bit.  GDM_ERR_UNSUPPORTED: another operator kind,
 * n_ranks > 1, a periodic mesh, the inner operator of a cut handle.
 * GDM_ERR_ARG: n_terms outside [0, GDM_COEF_MAX_TERMS], a non-finite sample,
 * and for n_terms = 1 a factor that vanishes or changes sign (or a negative
 * product).  For sums the caller guarantees rho > 0.  Not covered: a density
 * on periodic, multi-rank or cut meshes, a time-dependent density, and an RK
 * update fused into the weighted solve.
 * ---------------------------------------------------------------------- */
int gdm_density_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk);
int gdm_density_cholesky_1d(const gdm_mesh_desc *mesh, int axis, const double *f, double *lrow_host,
                            double *invd_host);
int gdm_op_set_density(gdm_op *op, int n_terms, const gdm_coef_term *terms);
int gdm_density_apply(gdm_op *op, const double *src, double *dst);
int gdm_density_apply_add(gdm_op *op, const double *src, double c, const double *add, double *dst);
int gdm_density_solve(gdm_op *op, const double *rhs, double *x, double rel_tol, double abs_tol, int max_it,
                      int *its_host, double *res_host);

/* ------------------------------------------------------------------------
 * General density on the Gauss grid: rho given by its samples on the tensor
 * Gauss grid of the mesh, for a density that is no short separable sum (a
 * model read from a file, a curved inclusion, a random field, rho(u)
 * re-evaluated every step).  M[rho] u = (B_z (x) B_y (x) B_x)^T diag(w rho)
 * (B_z (x) B_y (x) B_x) u with the value tables of gdm_coef_grid_tables_1d:
 * one launch of csrc/gdm_massgrid.hip, gather form, bitwise repeatable,
 * nothing allocated per apply.
 *
 *   gdm_op_set_density_grid
 *       rq is a DEVICE array in gdm_add_load's layout rq[(qz Q_y + qy) Q_x + qx]
 *       (the grid of kq), BORROWED, not copied: it must outlive the density, and
 *       the caller may overwrite it in place; the next gdm_density_apply sees
 *       the new values.  The call waits for the operator's stream, allocates all
 *       scratch, runs one device reduction (a sample that is not finite or not
 *       positive: GDM_ERR_ARG, the operator stays as it was), forms the
 *       Gauss-weighted mean of rho (fixed-order partials summed on the host) and
 *       W^-1/2 with W = diag(M[rho]) / diag(M) on the device.  Calling it again
 *       with the same pointer refreshes the mean and W and keeps the tables and
 *       the scratch (one reduction and the diagonal launch, nothing allocated).
 *       After an in-place overwrite WITHOUT this call the apply is current, and
 *       gdm_density_solve forms W again from the samples it finds (one launch of
 *       the kernel's diagonal mode per solve), but the mean in gdm_coef_solve's
 *       preconditioner is the old rho's: still SPD, so that CG converges, only
 *       more slowly.
 *       rq = NULL removes the density.  A grid density replaces a separable one
 *       and the other way round.
 *   gdm_density_grid_tile
 *       pure host: the (x, y) tile and the largest z chunk of the kernel,
 *       kernel axes (2D: z trivial; 1D: the mesh's x is the kernel's z).  A
 *       mesh with fewer than two workgroups per CU runs with a half or a
 *       quarter of the z chunk; the bits do not depend on it.
 *   gdm_op_set_density_grid_z_chunk
 *       steers the launch like gdm_op_set_mass_seg_waves and changes no bit of a
 *       result: z_chunk in [1, the chunk of gdm_density_grid_tile] node planes
 *       per workgroup, -1 restores the automatic choice; GDM_ERR_ARG otherwise,
 *       GDM_ERR_STATE without a grid density.  A new set call (not a refresh)
 *       chooses automatically again.
 *   gdm_density_diag
 *       dst_owned = diag(M[rho]) of the density that is set: on the grid
 *       sum_q w_q rho_q prod_d B_d[q_d, i_d]^2 by the kernel's diagonal mode,
 *       for a separable density sum_t prod_d diag(M_d[r_td]).  GDM_ERR_STATE
 *       without a density.
 * With a grid density set gdm_density_apply[_add] launch the grid kernel,
 * gdm_time_op(which = 3) times it, gdm_density_solve is always the CG described
 * above (rhs != x; preconditioner W^-1/2 M^-1 W^-1/2; the same GDM_ERR_STATE
 * returns) and gdm_coef_solve solves (alpha M[rho] - tau K[kappa]) x = rhs for
 * kappa absent, separable or on the grid, preconditioned at (mean(rho),
 * mean(kappa)).  Nothing else changes; without a grid density every launch is
 * the one it was.  GDM_ERR_UNSUPPORTED as for gdm_op_set_density: another
 * operator kind, n_ranks > 1, a periodic mesh, the inner operator of a cut
 * handle.  For a rho that is a separable sum gdm_op_set_density is the faster
 * path.
 * ---------------------------------------------------------------------- */
int gdm_op_set_density_grid(gdm_op *op, const double *rq);
int gdm_density_grid_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk);
int gdm_op_set_density_grid_z_chunk(gdm_op *op, int z_chunk);
int gdm_density_diag(gdm_op *op, double *dst_owned);

/* dst_owned = M src_local */
int gdm_mass_apply(gdm_op *op, const double *src_local, double *dst_owned);
/* x_owned = M^-1 rhs_owned (exact Kronecker inverse; single rank; not with
 * periodic constraints: gdm_mass_solve_periodic) */
int gdm_mass_solve(gdm_op *op, const double *rhs_owned, double *x_owned);
/* gdm_mass_solve_rk: k = M^-1 rhs, then gdm_vec_rk_update's acc_out = acc_in +
 * beta k and, when Y != NULL, Y = y + alpha k -- one RK stage's solve and
 * update (advection/problem.h:62-94 + the solve of :236-267) with the update
 * fused into the last line-solve pass, so k never reaches HBM.  rhs_owned is
 * overwritten (scratch).  Aliasing (GDM_ERR_ARG otherwise): rhs_owned overlaps
 * none of acc_in / acc_out / y / Y; acc_out and Y are distinct; a written
 * vector (acc_out, Y) may equal a read one (acc_in, y) but not partially
 * overlap it.  Same bits as gdm_mass_solve(rhs, rhs) + gdm_vec_rk_update.
 * Single rank, non-periodic (periodic: gdm_mass_solve_periodic_rk). */
int gdm_mass_solve_rk(gdm_op *op, double *rhs_owned, double beta, const double *acc_in, double *acc_out,
                      double alpha, const double *y, double *Y);

/* Dispatch control for tests and A/B runs (ABI 19).  Which kernels a mass
 * inverse or an SpMV launches depends on sizes that small tests do not reach;
 * these entry points steer that choice and report it.  None of them changes a
 * result's bits beyond what the steered kernels are specified to give, and
 * none changes the default dispatch.
 *   gdm_op_set_mass_seg_waves   the line passes of the mass inverse (gdm_mass_solve,
 *                        _rk, _periodic*, _slab) split the lines of a pass with
 *                        fewer than `waves` waves of 64 lines into segments;
 *                        waves in [0, default] (0: never segment; the default
 *                        is one wave per SIMD of the chip, 1024), -1 restores
 *                        the default; GDM_ERR_ARG otherwise.
 *   gdm_op_mass_path     what the last line passes of this operator launched:
 *                        per pass the kernel axis (0 = x, contiguous lines; 1,
 *                        2 = y, z, strided lines; the one direction of a 1D
 *                        mesh is kernel axis 2), v3 (single sweep) or v2 (two
 *                        sweeps), the segments per line (1 = whole lines) and
 *                        whether it ran in place;
 *                        rk_mode = 0 when no RK update was fused into the last
 *                        pass, else the fused kernel's variant: 1 = acc only,
 *                        2 = acc and Y, 3 = acc and Y with acc_in == y.  A fused
 *                        pass reports in_place = 0 (its result is not stored).
 *                        n_passes = 0 before the first solve.
 *   gdm_csr_set_lanes    K in {2, 4, 8, 16, 32, 64}: gdm_csr_vmult / gdm_csr_cg
 *                        run the K-lanes-per-row kernel; K = 0: the row-block
 *                        kernel (the default).  GDM_ERR_ARG otherwise.
 *   gdm_csr_kernel       mode 1 / lanes 0: row-block kernel; mode 0 / lanes K. */
typedef struct {
  int n_passes; /* 0..3, in launch order */
  int rk_mode;
  struct {
    int axis;     /* kernel axis of the pass: 0 = x, 1 = y, 2 = z */
    int v3;       /* 1: single-sweep kernel, 0: two-sweep kernel */
    int segments; /* segments per line; 1 = whole lines */
    int in_place; /* the pass read and wrote the same buffer */
  } pass[3];
} gdm_mass_path;
int gdm_op_set_mass_seg_waves(gdm_op *op, int waves);
int gdm_op_mass_path(const gdm_op *op, gdm_mass_path *out);

/* Exact mass inverse with periodicity constraints (ABI 17; replaces the
 * SolverCG + PreconditionJacobi of prototypes/advection_01_gdm.cc:208-217 by a
 * direct solve): x_owned = distribute((P^T M P)^-1 rhs_owned), the condensed
 * mass of System::make_periodicity_constraints (system.h:427-463).  Along a
 * periodic direction the condensed 1D matrix on the N - 1 free vertices is
 *   M_per = A + U S U^T,  A = M[0:N-1, 0:N-1],  U = [e_0, m],  m = M[0:N-1, N-1],
 *   S = [[M[N-1,N-1], 1], [1, 0]],
 * and M_per^-1 b = g - T (U^T g) with g = A^-1 b, T = Z (S^-1 + U^T Z)^-1,
 * Z = A^-1 U (Woodbury, nothing truncated).  The line passes of gdm_mass_solve
 * run with the tables of blockdiag(A, 1) in the periodic directions; one
 * rank-2 correction per periodic direction follows and writes x[N-1] = x[0]
 * (bit for bit).  The rhs entries on constrained DoFs are ignored (any finite
 * value; a condensed rhs has them zero).  x_owned may equal rhs_owned.
 * Without periodic constraints: gdm_mass_solve, same bits.  Single rank. */
int gdm_mass_solve_periodic(gdm_op *op, const double *rhs_owned, double *x_owned);
/* gdm_mass_solve_rk with periodicity constraints (ABI 17; one RK stage of
 * advection_01_gdm.cc:208-217 + :252-268 without the SolverCG): the last
 * correction writes acc_out = acc_in + beta k and, when Y != NULL, Y = y +
 * alpha k instead of k.  rhs_owned is overwritten (scratch).  Aliasing rules
 * of gdm_mass_solve_rk.  Same bits as gdm_mass_solve_periodic(rhs, rhs) +
 * gdm_vec_rk_update; without periodic constraints gdm_mass_solve_rk. */
int gdm_mass_solve_periodic_rk(gdm_op *op, double *rhs_owned, double beta, const double *acc_in, double *acc_out,
                               double alpha, const double *y, double *Y);
/* The host tables of gdm_mass_solve_periodic along `axis` (pure host, no
 * device; the direct replacement of the SolverCG of advection_01_gdm.cc:
 * 208-217): T_host [N-1][2], m_host [p] = M[N-1-p+j, N-1], and the rows the
 * correction touches, [0, rows_lo) and [N-1-rows_hi, N-1): a row k is skipped
 * only if max(|T[k][0]|, |T[k][1]| max|m|) <= 1e-18.  N = n_subdivisions + 1. */
int gdm_mass_periodic_tables(const gdm_mesh_desc *mesh, int axis, double *T_host, double *m_host, int *rows_lo,
                             int *rows_hi);
/* Row-form banded Cholesky factor of the 1D mass matrix along `axis` (pure
 * host): lrow_host [N][p+1], lrow[i][k] = L(i, i - p + k); invd_host [N] =
 * 1 / L(i, i).  periodic != 0: of blockdiag(M[0:N-1, 0:N-1], 1), the matrix the
 * line passes of gdm_mass_solve_periodic factor -- its rows equal M's except
 * the last one (0, ..., 0, 1). */
int gdm_mass_cholesky_1d(const gdm_mesh_desc *mesh, int axis, int periodic, double *lrow_host, double *invd_host);

/* Distributed exact mass inverse (n_ranks > 1; replaces the CG + ILU/AMG
 * solve of advection/problem.h:236-267 / wave/problem.h:457-502 across MPI
 * ranks).  M^-1 = M_q^-1 (x) ... (x) M_0^-1; the in-slab directions are
 * solved locally; the partitioned direction q = dim - 1 by a truncated SPIKE
 * scheme: each slab solves with its own diagonal block A_r of M_q, the ranks
 * exchange p planes with each slab neighbour (exactly the ghost planes of the
 * stencil's update_ghost_values), and a 2p x 2p interface system per slab
 * boundary (the same for every line) corrects the slab:
 *   gdm_mass_solve_slab(op, rhs_owned, x_owned)   x = (A_r^-1 (x) M_y^-1 (x) M_x^-1) rhs
 *   <copy x_owned into the owned part of a local vector; ghost exchange>
 *   for round in [0, rounds):                        (thin slabs only)
 *     gdm_mass_solve_interface_round(op, x_local, round); <ghost exchange>
 *   gdm_mass_solve_interface(op, x_local)          owned part of x_local = M^-1 rhs
 * The truncated interface systems drop the far-spike couplings (entries
 * <= gdm_mass_spike_eps, pure host; decays geometrically with the slab
 * thickness).  When that exceeds 1e-15 (slabs thinner than ~48 planes at p = 5,
 * e.g. C4 at 8 ranks: 32 planes, p = 7, eps 2e-8) gdm_mass_spike_rounds
 * (pure host) returns the number m of refinement rounds: each evaluates the
 * dropped couplings at the current interface values, moves them into the
 * slab's edge planes (the right-hand sides of the next interface systems) and
 * needs one more ghost exchange of the same p planes; the error after m rounds
 * is ~eps^(m+1).  rounds = -1: refused (GDM_ERR_UNSUPPORTED from the slab
 * solve; a slab with fewer than 2p planes or eps too large).  n_ranks == 1:
 * the slab solve is gdm_mass_solve and the interface call a no-op. */
int gdm_mass_spike_eps(const gdm_mesh_desc *mesh, double *eps_host);
int gdm_mass_spike_rounds(const gdm_mesh_desc *mesh, int *rounds);
int gdm_mass_solve_slab(gdm_op *op, const double *rhs_owned, double *x_owned);
int gdm_mass_solve_interface_round(gdm_op *op, double *x_local, int round);
int gdm_mass_solve_interface(gdm_op *op, double *x_local);
/* gdm_mass_solve_interface, and the ghost planes of x_local are overwritten
 * with the interface solution -- the lower neighbour's last p planes and the
 * upper neighbour's first p planes of M^-1 rhs, which each interface system
 * yields on both ranks of the pair (ABI 14).  x_local is then a valid local
 * vector of M^-1 rhs (ghosts equal to the neighbours' owned values to the
 * truncation tolerance, <= 1e-15 relative): an RK stage that updates its
 * local vectors over the ghost planes too (k, acc, y, Y in local layout)
 * needs no update_ghost_values before the next stage's stencil
 * (advection/stiffness.h:343) -- one exchange per stage, the SPIKE one. */
int gdm_mass_solve_interface_ghosts(gdm_op *op, double *x_local);
/* The interface step of the one-exchange stage fused with its RK update
 * (ABI 15): k = M^-1 rhs on every plane of the local layout (the owned planes
 * corrected as gdm_mass_solve_interface does, the ghost planes the interface
 * solution as gdm_mass_solve_interface_ghosts writes them) goes straight into
 * acc_out = acc_in + beta k and, when Y != NULL, Y = y + alpha k -- local
 * vectors (n_local entries), the arithmetic and the bits of
 * gdm_mass_solve_interface_ghosts + gdm_vec_rk_update over n_local; k is not
 * stored (x_local, holding the slab solve and the exchanged planes, is only
 * read).  acc_out may equal acc_in (not partially overlap it), y may equal
 * acc_in; x_local must not overlap an output.  Multi-rank only. */
int gdm_mass_solve_interface_rk(gdm_op *op, const double *x_local, double beta, const double *acc_in, double *acc_out,
                                double alpha, const double *y, double *Y);

/* x_owned = M^-1 rhs_owned by SolverCG on the matrix-free mass operator with
 * ReductionControl(max_it, abs_tol, rel_tol) semantics, the solve of
 * prototypes/advection_01_gdm.cc:208-217 (PreconditionJacobi, rel 1e-8) and of
 * *Problem::solve (advection/problem.h:251-261); precond 0 = identity,
 * 1 = Jacobi (diagonal of the condensed mass).  x_owned is the initial guess
 * (the reference starts from zero); *its_host = SolverControl::last_step();
 * GDM_ERR_STATE when max_it is reached.  A residual norm that is not finite (a
 * NaN in rhs_owned or x_owned) and a breakdown (p^T A p <= 0) return
 * GDM_ERR_STATE at once, with the iteration count reached, instead of running
 * to max_it.  Works with periodic constraints (the condensed operator:
 * constrained rows zero).  Single rank. */
int gdm_mass_solve_cg(gdm_op *op, const double *rhs_owned, double *x_owned, double rel_tol, double abs_tol,
                      int max_it, int precond, int *its_host, double *res_host);

/* diag_owned (device) = the diagonal of the (condensed) mass matrix on the
 * owned DoFs: the PreconditionJacobi of prototypes/advection_01_gdm.cc:211
 * and the diagonal a distributed CG preconditions with (constrained rows 1). */
int gdm_mass_diagonal(gdm_op *op, double *diag_owned);
/* y = w .* x elementwise (a diagonal preconditioner application).  y may equal
 * x ("x *= w") or w; partial overlap is not allowed. */
int gdm_vec_pointwise_mult(gdm_op *op, int64_t n, const double *w, const double *x, double *y);
/* device-to-device copy on the operator's stream */
int gdm_memcpy_d2d(gdm_op *op, void *dst, const void *src, size_t bytes);

/* AffineConstraints::distribute of the periodicity constraints
 * (advection_01_gdm.cc:158, 268): v[last vertex of d] = v[first] for every
 * periodic direction d; no-op without periodic constraints. */
int gdm_constraints_distribute(gdm_op *op, double *v_owned);

/* In-place banded-Cholesky solve with the 1D mass matrix of reference
 * direction `axis` (0 = x, 1 = y, 2 = z) along n_lines lines of full length
 * N[axis]: line l starts at v + (l / A) * B + (l % A) * C and its entries are
 * `stride` apart.  The building block of the distributed mass inverse (the
 * slab-local directions are solved in place, the partitioned one after a
 * transpose; gdm_amd/distributed.py), replacing the CG of
 * advection/problem.h:236-267 on a multi-rank mesh. */
int gdm_mass_solve_lines(gdm_op *op, int axis, double *v, int64_t n_lines, int64_t stride, int64_t A, int64_t B,
                         int64_t C);

/* gdm_vec_axpby: y = a x + b y, one fma(a, x_i, b * y_i) per entry.  An operand
 * whose factor is zero is not read: b == 0 gives y = a x whatever y held
 * (uninitialised memory, NaN, Inf), a == 0 gives y = b y without touching x,
 * a == b == 0 gives y = +0 ("v = 0" on a fresh allocation).  For finite
 * operands this differs from the fma form only in the sign of a zero result.
 * x may equal y (y = (a + b) y in the arithmetic above); partial overlap is
 * not allowed.  No alignment requirement: vectors that both start on a 16-byte
 * boundary are moved in pairs, others entry by entry, with the same bits.
 * gdm_vec_dot: *result_host = x . y (x may equal y); two calls on the same
 * data return the same bits. */
int gdm_vec_axpby(gdm_op *op, int64_t n, double a, const double *x, double b, double *y);
int gdm_vec_dot(gdm_op *op, int64_t n, const double *x, const double *y, double *result_host);
int gdm_synchronize(gdm_op *op);

/* ------------------------------------------------------------------------
 * Device-resident explicit Runge-Kutta: replaces the per-stage
 * BlockVector allocation and vector updates of TimeStepping::
 * ExplicitRungeKutta (advection/problem.h:62-94, wave/problem.h:296-338) and
 * the host evaluation of block(0) in initialize_time_step / compute_rhs
 * (advection/stiffness.h:181-194, 286-289).
 *
 *   gdm_vec_rk_update   acc_out = acc_in + beta k and, when Y != NULL,
 *                       Y = y + alpha k, in one pass (low-storage form of a
 *                       Butcher table with one nonzero a_ij per stage, e.g.
 *                       RK_CLASSIC_FOURTH_ORDER).  One fma per output.  As
 *                       for gdm_mass_solve_rk, a written vector (acc_out,
 *                       Y) may equal a read one (acc_in, y) -- the first
 *                       stage in place is acc_out == acc_in == y -- and
 *                       acc_out and Y are distinct; k overlaps no output.
 *                       Vectors that are not all 16-byte aligned take an
 *                       entry-by-entry kernel with the same bits.
 *   gdm_eval_boundary   bc_values (device order, n_bc_points) = g(t)
 *                       (derivative 0) or dg/dt(t) (derivative 1) at the
 *                       boundary points for a built-in function:
 *     GDM_FN_CONSTANT      params: c
 *     GDM_FN_CONE          params: r0, center[dim] -- max(0, r0 - |x - c|)
 *                          (the advection app's ExactSolution,
 *                          applications/advection/advection-app.cc:51-79;
 *                          dg/dt = 0, its ExactSolutionDerivative)
 *     GDM_FN_SINE_PRODUCT  params: a[3], k[3], phi[3] --
 *                          prod_d sin(2 pi k_d (x_d - a_d t) + phi_d)
 *                          (a solution transported with velocity a)
 * ---------------------------------------------------------------------- */
enum gdm_fn_kind { GDM_FN_CONSTANT = 0, GDM_FN_CONE = 1, GDM_FN_SINE_PRODUCT = 2 };
int gdm_vec_rk_update(gdm_op *op, int64_t n, double beta, const double *k, const double *acc_in, double *acc_out,
                      double alpha, const double *y, double *Y);
int gdm_eval_boundary(gdm_op *op, int fn_kind, const double *params, int n_params, double t, int derivative,
                      double *bc_values);
/* gdm_apply_bc_fn: gdm_apply (stencil + inflow boundary term) with the stage
 * boundary values computed by the engine (into its own scratch, inflow faces
 * only, one launch before the stencil) instead of read from a caller's
 * bc_values vector: BC = g(t_g) + alpha dg/dt(t_k) (alpha = 0: g(t_g)), the
 * same bits as gdm_eval_boundary(g, t_g) / (dg/dt, t_k) followed by
 * gdm_vec_rk_update's Y = y + alpha k.  This is block(0) of the reference's
 * RK stages (advection/problem.h:62-94 with initialize_time_step,
 * stiffness.h:181-194, and the dg/dt stage block, stiffness.h:286-289) for
 * the classic RK4 tableau, where stage s >= 1 reads y0 + h a_{s,s-1} k_{s-1}:
 * the block(0) vectors and their stage updates disappear (block(0) after a
 * step is never read: initialize_time_step overwrites it, problem.h:88-90).
 * Advection operators; fn_kind / params as gdm_eval_boundary. */
int gdm_apply_bc_fn(gdm_op *op, const double *src_local, double *dst_owned, int fn_kind, const double *params,
                    int n_params, double t_g, double alpha, double t_k);
/* gdm_add_boundary_fn: gdm_add_boundary_data with the stage boundary values
 * of gdm_apply_bc_fn (the inflow term alone, after gdm_apply_planes) */
int gdm_add_boundary_fn(gdm_op *op, double *dst_owned, int fn_kind, const double *params, int n_params, double t_g,
                        double alpha, double t_k);

/* ----------------------------------------------------------------------
 * Postprocess on the device
 *   gdm_error_norms     the volume error norms of the reference's
 *                       postprocess (applications/advection/include/gdm/
 *                       advection/problem.h:269-425, the uncut mesh has no
 *                       immersed surface, so its *_face norms are 0):
 *                       norms_host = {Linf, L1, L2} of u - f(t) over
 *                       QGauss(p+1) on this rank's locally owned cells, f a
 *                       built-in function (gdm_fn_kind, same params as
 *                       gdm_eval_boundary).  u_local: engine-local vector
 *                       (ghost planes filled).  The caller reduces across
 *                       ranks as the reference does: Linf max, L1 sum,
 *                       L2 = sqrt(sum L2^2) (problem.h:410-425).
 *                       cell_errors (device, optional, n_owned_cells =
 *                       product of the owned cell counts, lexicographic
 *                       x fastest) = integrate_difference's per-cell L2
 *                       errors (include/gdm/vector_tools.h:25-86).
 * ---------------------------------------------------------------------- */
int gdm_error_norms(gdm_op *op, const double *u_local, int fn_kind, const double *params, int n_params, double t,
                    double *cell_errors, double *norms_host);

/* ------------------------------------------------------------------------
 * Forcing and Dirichlet data of the uncut wave / heat operator (ABI 18): the
 * two data terms of StiffnessMatrixOperator::compute_rhs(dst, src,
 * compute_impl_part, time) (applications/wave/include/gdm/wave/stiffness.h:
 * 409-420, body :151-330) next to the operator part gdm_apply computes:
 *   the source term (v, f(., t)) over QGauss(p+1)                 (:196-200)
 *   the Nitsche data <gamma_D / h v - dv/dn, g_D(., t)> on the box (:320-326)
 * Every call ADDS into dst_owned, as compute_rhs accumulates.  Single rank,
 * non-periodic, any operator kind (the load is the right-hand side of an L2
 * projection or a Poisson problem as well: tests/mass_01_gdm.cc,
 * tests/poisson_01_gdm.cc).
 *
 *   gdm_add_load_fn      dst += scale (v, f), f a built-in gdm_fn_kind at time t
 *                        (derivative 0) or its d/dt (derivative 1); kinds,
 *                        params and formulas as gdm_eval_boundary.
 *                        GDM_FN_CONSTANT and GDM_FN_SINE_PRODUCT are products
 *                        of one-variable functions, for which tensor Gauss
 *                        quadrature factorises exactly: (v, f) = b_z (x) b_y (x)
 *                        b_x with the 1D load vectors b_d[i] = sum_q w_q h
 *                        phi_i(x_q) f_d(x_q) (gdm_load_vector_1d); one term for
 *                        the value, dim terms for d/dt (sum_e P_e cos_e prod_{d
 *                        != e} sin_d, P_e = -2 pi k_e a_e).  The call reads and
 *                        writes dst once.  GDM_FN_CONE is evaluated pointwise
 *                        by the general kernel of gdm_add_load (d/dt = 0).
 *                        scale == 0, and a derivative that is identically
 *                        zero, launch nothing.
 *   gdm_add_load         dst += scale (v, f) with f given by the caller as a
 *                        DEVICE array on the tensor Gauss grid:
 *                        fq[(qz Q_y + qy) Q_x + qx], Q_d = n_sub_d (p+1),
 *                        q_d = cell_d (p+1) + point, x fastest, Q_d = 1 for
 *                        d >= dim; the abscissae along d are entries 1 .. Q_d
 *                        of gdm_field_points(mesh, d).  The array holds
 *                        8 (p+1)^dim bytes per cell, about as much per DoF
 *                        (1.7 KB at p = 5, 4 KB at p = 7 in 3D): the form for
 *                        moderate meshes and for data no built-in function
 *                        describes.  No intermediate grid is stored.
 *   gdm_add_dirichlet_data
 *                        dst += sum over the box faces of <gamma / h_min v -
 *                        dv/dn, g>, gamma the operator's Nitsche parameter,
 *                        h_min = min_d h_d (the cell's minimum vertex
 *                        distance, as in the operator part).  g_bc: device
 *                        array of n_bc_points values in the device block(0)
 *                        order (gdm_bc_points, gdm_bc_reference_order;
 *                        gdm_eval_boundary fills it for a built-in g).
 *                        GDM_OP_WAVE operators created with nitsche > 0 only
 *                        (GDM_ERR_UNSUPPORTED otherwise).
 *   gdm_load_vector_1d   pure host: b_host [n_sub + 1] = the 1D load vector
 *                        along `axis` for f sampled at the Gauss entries of
 *                        gdm_field_points (f has its n_sub (p+1) + 2 entries,
 *                        the two end values are not read; NULL: f = 1)
 *   gdm_load_tile        pure host: the (x, y) node tile and the z chunk of
 *                        node planes of the general load kernel, kernel axes
 *                        (3D: x, y, z; 2D: x, y, -; 1D: -, -, x)
 * GDM_ERR_UNSUPPORTED: n_ranks > 1, a periodic mesh, the inner operator of a
 * cut handle.  GDM_ERR_ARG: NULL vectors, derivative outside {0, 1}, the
 * parameter checks of gdm_eval_boundary.  All tables and scratch are built by
 * gdm_op_create; no call allocates, so a first call may be captured in a
 * hipGraph (t and scale are launch arguments, frozen at capture).  Gather
 * form throughout: the bits of a result do not depend on the launch.
 * ---------------------------------------------------------------------- */
int gdm_add_load_fn(gdm_op *op, int fn_kind, const double *params, int n_params, double t, int derivative,
                    double scale, double *dst_owned);
int gdm_add_load(gdm_op *op, const double *fq, double scale, double *dst_owned);
int gdm_add_dirichlet_data(gdm_op *op, const double *g_bc, double *dst_owned);
int gdm_load_vector_1d(const gdm_mesh_desc *mesh, int axis, const double *f, double *b_host);
int gdm_load_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk);

/* ------------------------------------------------------------------------
 * Grid evaluation: u and grad u on the tensor Gauss grid, the flux load and
 * the wall trace -- with gdm_add_load the three legs of a matrix-free
 * "evaluate, pointwise work, integrate" cycle, so that a quasi-linear problem
 * -div F(x, u, grad u) = f(x, u) is grid evaluation, pointwise work on the
 * grid arrays and grid integration (gdm_amd.QuasilinearHeatProblem).
 * Q_d = n_sub_d (p+1), Q = prod Q_d; grid arrays in gdm_add_load's fq layout
 * (x fastest); vector-valued grid arrays component-major, gq[e Q + q] with e
 * the reference direction.
 *   gdm_eval_grid        uq[Q] = u and gq[dim Q] = the physical gradient of u
 *                        at the Gauss points: FEValues::get_function_values
 *                        and get_function_gradients of every cell at once
 *                        (wave/stiffness.h:151-203, advection/problem.h:
 *                        330-425).  Either output may be NULL (it then costs
 *                        nothing); both NULL is GDM_ERR_ARG.  The outputs must
 *                        not overlap u_local (GDM_ERR_ARG).  One launch.
 *   gdm_add_load_grad    dst += scale sum_e (d_e v, F_e) over QGauss(p+1),
 *                        Fq[dim Q] as gq: the cell loop's
 *                        fe_values.shape_grad(i, q) * F(q) * JxW(q)
 *                        (wave/stiffness.h:171-181 with F in place of grad u),
 *                        the transpose of the gradient evaluation with the
 *                        Gauss weights.  One launch, dst is read and written
 *                        once; scale == 0 launches nothing.
 *   gdm_eval_trace       u_bc / dn_bc [n_bc_points] = the wall trace and the
 *                        outward normal derivative of u at the boundary points
 *                        in the device block(0) order (gdm_bc_points, g_bc,
 *                        kbc): FEFaceValues::get_function_values and
 *                        get_function_gradients . normal_vector of the box
 *                        faces (wave/stiffness.h:296-310).  Either output may
 *                        be NULL, not both; a no-op with n_bc_points == 0.
 *   gdm_eval_grid_tile   pure host: the block of cells that one work item of
 *                        the evaluation kernel owns, kernel axes (3D: x, y, z;
 *                        2D: x, y, -; 1D: -, -, x)
 * Every operator kind; on an elasticity operator a call takes one component
 * (pass the component's block of the component-major vector).
 * GDM_ERR_UNSUPPORTED: n_ranks > 1, a periodic mesh, the inner operator of a
 * cut handle.  All tables are built by gdm_op_create; no call allocates or
 * synchronises, so a first call may be captured in a hipGraph.  Every output
 * value is formed by one thread in a fixed order and stored once: the bits do
 * not depend on the launch, the stream or a graph replay.
 * ---------------------------------------------------------------------- */
int gdm_eval_grid(gdm_op *op, const double *u_local, double *uq, double *gq);
int gdm_add_load_grad(gdm_op *op, const double *Fq, double scale, double *dst_owned);
int gdm_eval_trace(gdm_op *op, const double *u_local, double *u_bc, double *dn_bc);
int gdm_eval_grid_tile(int fe_degree, int dim, int *cx, int *cy, int *cz);

/* ------------------------------------------------------------------------
 * Direct solve with the uncut wave / heat operator by fast diagonalisation
 * (added within ABI 18: new entry points only, backward compatible, the
 * version number is unchanged).  The linear solves of the "poisson" and
 * "heat-impl" simulation types (applications/wave/include/gdm/wave/problem.h:
 * 46-71, 210-279), where the reference runs CG + AMG on the assembled matrix.
 * On an uncut box the stiffness matrix is S = -K = sum_d M (x) .. A_d .. (x) M
 * with the symmetric 1D factors A_d = -B_d (the -L_d + box Nitsche band of
 * gdm_apply).  With the generalised eigenpairs A_d S_d = M_d S_d Lambda_d,
 * S_d^T M_d S_d = I:
 *   (alpha M + tau S)^-1 = (S_z (x) S_y (x) S_x)
 *                          diag(1 / (alpha + tau (lambda_z + lambda_y + lambda_x)))
 *                          (S_z (x) S_y (x) S_x)^T
 * -- 2 dim dense N_d x N_d contractions over the vector on the FP64 matrix
 * pipe (csrc/gdm_fastdiag.hip), the diagonal scaling in the epilogue of the
 * last forward pass.  Exact up to round-off ~ 1e-17 cond.
 *
 *   gdm_fastdiag_tables  pure host: S_host (row-major N x N, column j =
 *                        eigenvector j) and lambda_host (N, ascending) of
 *                        direction `axis`, N = n_subdivisions[axis] + 1;
 *                        nitsche = the operator's Nitsche parameter (h_min is
 *                        taken over the mesh's directions).  Each eigenvector's
 *                        entry of largest magnitude is positive; two calls give
 *                        the same bits.
 *   gdm_system_solve_setup  builds and uploads the tables of every direction
 *                        and two scratch vectors; idempotent.  The only call
 *                        of the group that allocates or synchronises.
 *   gdm_system_solve     x = (alpha M - tau K)^-1 rhs, K = gdm_apply of this op
 *                        (K = -S of the reference): heat-impl alpha = 1, tau =
 *                        dt (problem.h:217-226, 263-269; a changed last step
 *                        needs no new setup); poisson alpha = 0, tau = 1
 *                        (problem.h:46-67).  x_owned may equal rhs_owned; rhs
 *                        is otherwise not modified.  No allocation, no host
 *                        synchronisation: the call may be captured in a
 *                        hipGraph (alpha, tau frozen at capture).  Bitwise
 *                        repeatable.  Calls on one op share its scratch: order
 *                        them on one stream.
 *   gdm_fastdiag_transform  one pass, for tests and tools: dst = T src along
 *                        `axis` (reference direction), T = S (transpose 0) or
 *                        S^T (1); src and dst distinct.
 * GDM_ERR_UNSUPPORTED: a kind other than GDM_OP_WAVE, n_ranks > 1, a periodic
 * mesh, the inner operator of a cut handle.  GDM_ERR_STATE: solve / transform
 * before setup.  GDM_ERR_ARG: NULL pointers, non-finite alpha or tau, axis
 * outside [0, dim), and a singular or indefinite system: the interval [alpha +
 * tau sum_d lambda_d,min, alpha + tau sum_d lambda_d,max] contains 0 or its end
 * nearer to 0 is below 1e-12 of the other in magnitude (pure Neumann Poisson:
 * nitsche = 0 with alpha = 0; a Nitsche penalty too small for the degree, e.g.
 * gamma = 4 from p = 5 on).
 * ---------------------------------------------------------------------- */
int gdm_fastdiag_tables(const gdm_mesh_desc *mesh, double nitsche, int axis, double *S_host, double *lambda_host);
int gdm_system_solve_setup(gdm_op *op);
int gdm_system_solve(gdm_op *op, double alpha, double tau, const double *rhs_owned, double *x_owned);
int gdm_fastdiag_transform(gdm_op *op, int axis, int transpose, const double *src_owned, double *dst_owned);

/* ------------------------------------------------------------------------
 * Linear elasticity on uncut boxes (added within ABI 18: new entry points and
 * one new operator kind only, the version number is unchanged).  The matrix of
 * tests/elasticity_01_gdm.cc:143-184,
 *   a(u, v) = 2 mu (eps(u), eps(v)) + lambda (div u, div v)
 * (the reference has mu = 1, lambda = 0), with the constraints of
 * System::make_zero_boundary_constraints (system.h:466-498): every component
 * of every vertex on a box face is constrained to zero.  The operator is
 * P A P + I - P, P the mask of the free DoFs; the constrained rows carry a unit
 * diagonal (deal.II puts another positive number there, which changes neither
 * the CG iterates nor the iteration count while the right-hand side is zero on
 * those rows).
 *
 * Vectors are component-major: u = [u_0 | u_1 | (u_2)], dim blocks of n_dofs
 * entries, each block a scalar vector in the operator's layout, so every scalar
 * entry point (gdm_mass_apply, gdm_add_load, gdm_error_norms_grid, ...) works on
 * one component through a pointer offset.  The reference numbers DoFs vertex *
 * n_components + component (system.h:242-244): gdm_vec_interleave converts.
 *
 *   gdm_op_create(GDM_OP_ELASTICITY, {mu, lambda})
 *                        dim 2 or 3, single rank, non-periodic
 *                        (GDM_ERR_UNSUPPORTED otherwise); mu > 0, lambda >= 0
 *                        (GDM_ERR_ARG).
 *   gdm_apply            dst = (P A P + I - P) src on vectors of dim * n_dofs
 *                        entries, one launch for all components
 *                        (csrc/gdm_elasticity.hip: SparseMatrix::vmult of
 *                        elasticity_01_gdm.cc:184).  bc_values must be NULL and
 *                        src != dst (GDM_ERR_ARG).  No allocation; bitwise
 *                        repeatable.
 *   gdm_elasticity_tile  pure host: the (x, y) node tile and the z chunk of
 *                        node planes of the kernel (z_chunk = 1 in 2D).
 *   gdm_elasticity_tables_1d
 *                        pure host: the tables of direction `axis`, N =
 *                        n_subdivisions[axis] + 1.  bands_host [4][N][2p+1]:
 *                        the Dirichlet-reduced M, C, C^T, L (C_ij = int phi_i'
 *                        phi_j), entry [f][i][k] = A_f(i, i - p + k), rows and
 *                        columns 0 and N - 1 zero.  S_host (row-major N x N),
 *                        lambda_host (N): the generalised eigenpairs of the
 *                        interior (N-2) x (N-2) pencil (L, M), S^T M S = I,
 *                        embedded with zero rows / columns 0 and N - 1 of S and
 *                        lambda = 1 there.  Any of the outputs may be NULL
 *                        (S_host and lambda_host together).
 *   gdm_elasticity_diagonal
 *                        diag (device, dim * n_dofs) = the diagonal of
 *                        P A P + I - P: PreconditionJacobi::initialize of
 *                        elasticity_01_gdm.cc:178-179.  Synchronises.
 *   gdm_elasticity_precond_setup
 *                        builds and uploads the tables of the block
 *                        preconditioner and two scratch vectors; idempotent.
 *                        The only call of the preconditioner that allocates or
 *                        synchronises.
 *   gdm_elasticity_precond
 *                        z = B^-1 r on the free DoFs, 0 on the constrained ones,
 *                        B = blockdiag_c(P A_cc P + I - P): by Korn's inequality
 *                        spectrally equivalent to the operator, inverted exactly
 *                        by fast diagonalisation, B_cc^-1 = (S (x) S (x) S)
 *                        diag(1 / sum_d w_cd lambda_d) (S (x) S (x) S)^T with w_cd
 *                        = 2 mu + lambda (d = c), mu otherwise (the passes of
 *                        gdm_system_solve).  r != z.  No allocation, no host
 *                        synchronisation: capturable in a hipGraph.
 *                        GDM_ERR_STATE before setup.
 *   gdm_elasticity_solve SolverCG with ReductionControl(max_it, abs_tol,
 *                        rel_tol) (elasticity_01_gdm.cc:181-184), conventions of
 *                        gdm_mass_solve_cg: x is the initial guess, *its_host =
 *                        last_step, *res_host = the final residual norm,
 *                        GDM_ERR_STATE when max_it is reached, and at once (with
 *                        the count reached) for a residual norm that is not
 *                        finite or a breakdown (p^T A p <= 0).  precond: 0 none,
 *                        1 Jacobi (the reference's), 2 the block fast
 *                        diagonalisation (GDM_ERR_STATE before
 *                        gdm_elasticity_precond_setup).  Entries of rhs on
 *                        constrained DoFs count as 0 and those of x are set to
 *                        0.  The iteration count of precond 2 does not grow
 *                        with the mesh (a dozen at lambda = 0, where Jacobi
 *                        needs hundreds); it grows with lambda / mu towards the
 *                        incompressible limit (69 at lambda = 50 mu, 2D p = 3,
 *                        n = 40).  Allocates work vectors on the first call.
 *   gdm_vec_interleave   to_reference 1: dst[v * n_components + c] = src[c *
 *                        n_dofs + v] (component-major -> the reference's
 *                        numbering); 0: the inverse.  src != dst.  Any kind.
 *   gdm_error_norms_grid gdm_error_norms with the exact solution given as a
 *                        DEVICE array on the tensor Gauss grid, in the layout
 *                        of gdm_add_load's fq (integrate_difference against a
 *                        function that is not built in, elasticity_01_gdm.cc:
 *                        186-198; one call per component, L2 = sqrt(sum_c
 *                        L2_c^2)).  On several ranks exact_q is the whole
 *                        mesh's grid on every rank, which reads the cells
 *                        it owns.  Any kind.
 * ---------------------------------------------------------------------- */
int gdm_elasticity_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk);
int gdm_elasticity_tables_1d(const gdm_mesh_desc *mesh, int axis, double *bands_host, double *S_host,
                             double *lambda_host);
int gdm_elasticity_diagonal(gdm_op *op, double *diag);
int gdm_elasticity_precond_setup(gdm_op *op);
int gdm_elasticity_precond(gdm_op *op, const double *r, double *z);
int gdm_elasticity_solve(gdm_op *op, const double *rhs, double *x, int precond, double rel_tol, double abs_tol,
                         int max_it, int *its_host, double *res_host);
int gdm_vec_interleave(gdm_op *op, int n_components, int to_reference, const double *src, double *dst);
int gdm_error_norms_grid(gdm_op *op, const double *u_local, const double *exact_q, double *cell_errors,
                         double *norms_host);

/* memory helpers for callers without their own device allocator */
int gdm_malloc(gdm_op *op, size_t bytes, void **ptr);
int gdm_free(gdm_op *op, void *ptr);
int gdm_memcpy_h2d(gdm_op *op, void *dst, const void *src_host, size_t bytes);
int gdm_memcpy_d2h(gdm_op *op, void *dst_host, const void *src, size_t bytes);

/* boundary points: coordinates of all n_bc_points device points (device
 * order; the caller evaluates its boundary data there, ghost-cell points
 * included) and ref_to_dev[i] = device index of the i-th point in the
 * reference's block(0) order (owned cells lexicographic, faces 0..2dim-1, q;
 * n_bc_points_ref entries). */
int gdm_bc_points(const gdm_op *op, double *xyz_host);
int gdm_bc_reference_order(const gdm_op *op, int64_t *ref_to_dev_host);

/* time n_iter back-to-back applications with HIP events on the operator's
 * stream; which: 0 = gdm_apply, 1 = gdm_mass_apply, 2 = gdm_mass_solve, 3 =
 * gdm_density_apply (bc_values unused).
 * avg_ms_host receives the mean time per application. */
int gdm_time_op(gdm_op *op, int which, const double *src, double *dst, const double *bc_values, int n_iter,
                double *avg_ms_host);

/* ------------------------------------------------------------------------
 * Assembled sparse matrices: the irregular-stencil CG of
 * the cut-cell Poisson prototype and the on-disk triplet format.
 *
 *   gdm_csr_create       dealii::SparseMatrix<double>::reinit(sparsity) + the
 *                        assembled values (prototypes/cut_poisson_01_gdm.cc:
 *                        148-163, 327-336; full structural stencil of
 *                        System::create_sparsity_pattern, system.h:586-599).
 *                        Arrays are copied into device memory owned by the
 *                        handle; row_ptr int64 (n_rows+1), cols uint32 (the
 *                        reference's unsigned int indices), vals fp64.
 *                        src_is_device: 1 = the three arrays are device
 *                        pointers, 0 = host pointers.
 *   gdm_csr_vmult        SparseMatrix::vmult(dst, src) -- the matvec SolverCG
 *                        calls (cut_poisson_01_gdm.cc:335)
 *   gdm_csr_cg           SolverCG<>(ReductionControl(max_it, abs_tol, rel_tol))
 *                        .solve(A, x, b, P) with P = PreconditionIdentity
 *                        (precond 0, cut_poisson_01_gdm.cc:332-335) or
 *                        PreconditionJacobi (precond 1, omega = 1); x is the
 *                        initial guess; *its_host = last_step, *res_host = final
 *                        residual norm; GDM_ERR_STATE when max_it is reached.
 *   gdm_csr_read_triplets / gdm_csr_write_triplets
 *                        the binary / text triplet files of write_matrix_to_file
 *                        (applications/wave/wave-ev.cc:93-127): per entry u32
 *                        row, u32 column, f64 value (binary) or "row col value"
 *                        lines (text), rows ascending, diagonal first in each
 *                        square-matrix row (deal.II SparsityPattern order).
 *                        Reading sums duplicate (row, col) entries.
 * ---------------------------------------------------------------------- */
typedef struct gdm_csr gdm_csr;

int gdm_csr_create(int device, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *row_ptr,
                   const uint32_t *cols, const double *vals, int src_is_device, gdm_csr **out);
int gdm_csr_destroy(gdm_csr *A);
int gdm_csr_info(const gdm_csr *A, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
int gdm_csr_set_stream(gdm_csr *A, void *hip_stream);
/* kernel choice of gdm_csr_vmult / gdm_csr_cg (ABI 19; "dispatch control" above) */
int gdm_csr_set_lanes(gdm_csr *A, int K);
int gdm_csr_kernel(const gdm_csr *A, int *mode, int *lanes);
/* host copies of the three arrays (caller-allocated, sizes from gdm_csr_info) */
int gdm_csr_download(const gdm_csr *A, int64_t *row_ptr_host, uint32_t *cols_host, double *vals_host);
/* dst = A src (device pointers, dst of n_rows, src of n_cols entries) */
int gdm_csr_vmult(gdm_csr *A, const double *src, double *dst);
int gdm_csr_cg(gdm_csr *A, const double *b, double *x, int precond, int max_it, double abs_tol, double rel_tol,
               int *its_host, double *res_host);
int gdm_csr_read_triplets(int device, const char *path, int binary, gdm_csr **out);
int gdm_csr_write_triplets(const gdm_csr *A, const char *path, int binary);
/* mean time of n_iter back-to-back gdm_csr_vmult calls (HIP events, ms) */
int gdm_csr_time_vmult(gdm_csr *A, const double *src, double *dst, int n_iter, double *avg_ms_host);

/* ------------------------------------------------------------------------
 * Cut-cell systems: the 2D cut Poisson problem of
 * prototypes/cut_poisson_01_gdm.cc:57-405 assembled on the host
 * (csrc/gdm_cut.cpp) and solved by the device SpMV + SolverCG above.
 *
 *   gdm_cut_poisson_create   the reference's test<2>(ghost_penalty) system:
 *                            GDM degree p, n_sub^2 cells on [lo, hi]^2,
 *                            level set = FE_Q(1) interpolant of
 *                            |x - center| - radius (SignedDistance::Sphere),
 *                            NonMatching::MeshClassifier, the deal.II
 *                            QuadratureGenerator (Saye) on each intersected
 *                            cell, (grad v, grad u)_inside + Nitsche
 *                            (gamma = 5 (p+1) p) + ghost penalty (0.5 * 0.5 h
 *                            [d_n v][d_n u]) if ghost_penalty, rhs
 *                            rhs_value v + Nitsche data bc_value, zero
 *                            diagonals -> 1 (:148-323).  2D only.
 *   gdm_cut_poisson_matrix   the system matrix as a device CSR (gdm_csr_*)
 *   gdm_cut_poisson_csr      host copy of the CSR arrays (caller-allocated,
 *                            sizes from gdm_cut_poisson_info; ascending
 *                            columns, the entries cell assembly touches plus
 *                            every diagonal)
 *   gdm_cut_poisson_rhs      the right-hand side (host copy, n_rows values)
 *   gdm_cut_poisson_solve    SolverCG<>(ReductionControl(max_it, abs_tol,
 *                            rel_tol)).solve(A, u, rhs, PreconditionIdentity())
 *                            from u = 0 on the device (:332-335); A from
 *                            gdm_cut_poisson_matrix; u_host receives the
 *                            solution; GDM_ERR_STATE when max_it is reached
 *   gdm_cut_poisson_l2_error L2 error over the inside quadrature against the
 *                            manufactured solution bc + rhs/4 (r^2 - |x-c|^2)
 *                            (:349-405); u_host in the global DoF order
 * ------------------------------------------------------------------------ */
typedef struct gdm_cut_system gdm_cut_system;
int gdm_cut_poisson_create(int p, int n_sub, double lo, double hi, const double *center /* [2] or NULL */,
                           double radius, int ghost_penalty, double rhs_value, double bc_value, gdm_cut_system **out);
int gdm_cut_poisson_info(const gdm_cut_system *S, int64_t *n_rows, int64_t *nnz, int64_t *n_inside_cells,
                         int64_t *n_intersected_cells);
int gdm_cut_poisson_matrix(const gdm_cut_system *S, int device, gdm_csr **A);
int gdm_cut_poisson_csr(const gdm_cut_system *S, int64_t *row_ptr_host, uint32_t *cols_host, double *vals_host);
int gdm_cut_poisson_rhs(const gdm_cut_system *S, double *rhs_host);
int gdm_cut_poisson_solve(const gdm_cut_system *S, gdm_csr *A, double rel_tol, double abs_tol, int max_it,
                          double *u_host, int *its_host, double *res_host);
int gdm_cut_poisson_l2_error(const gdm_cut_system *S, const double *u_host, double *err);
int gdm_cut_poisson_destroy(gdm_cut_system *S);

/* ------------------------------------------------------------------------
 * Cut-cell advection (applications/advection, non-composite,
 * alpha = 0, 2D): the device compute_rhs / mass solve of the reference's
 * advection application on a mesh cut by an FE_Q(1) level set.
 *
 *   compute_rhs   rhs = Z S u + C u + F bc  (advection/stiffness.h:196-606):
 *                 S = the uncut fused Kronecker stencil of the box (the
 *                 advection operator of gdm_op_create with the box outflow
 *                 traces, no inflow data), Z zeroes the rows of the DoFs in
 *                 the box of a cell that is not fully inside, C =
 *                 those rows of the cut operator in full (volume and
 *                 outflow box-face terms of the inside cells, their cut
 *                 versions on intersected cells, outflow part of the
 *                 cut-surface term (II) :420-471) plus the ghost penalty
 *                 -0.5 gamma_A h^2 [d_n v][d_n u] (IV) :534-598, F = the
 *                 inflow data of (II) and (III) :473-532 (one column per
 *                 stage boundary point); C and F assembled on the host
 *                 (csrc/gdm_cut_advection.cpp), device CSR products.
 *   mass_solve    x = M_cut^-1 rhs exactly: banded Cholesky of the cut mass
 *                 (v, u)_inside + 0.5 gamma_M h^3 [d_n v][d_n u], zero
 *                 diagonals -> 1 (advection/mass.h:47-243), factored on the
 *                 host, triangular solves on the device (the SolverDirect
 *                 branch of advection/problem.h:262-265).  Up to 2^22 DoFs.
 *   bc_points     the stage boundary points (x, y) in the reference's
 *                 point_counter order (stiffness.h:40-160: per cell in
 *                 lexicographic order, its cut-surface points, then the inside
 *                 parts of its box faces in face order); block(0) of the
 *                 reference's BlockVector = the caller's values at them.
 *   op            the inner gdm_op (its stream; vector ops such as
 *                 gdm_vec_rk_update on these vectors).
 * level_set: the (n_sub + 1)^2 vertex values of the level set (x fastest);
 * cells with all values < 0 are inside, all > 0 outside (MeshClassifier).
 * u, bc, rhs, x: device pointers (n_dofs / n_bc_points doubles).
 * ------------------------------------------------------------------------ */
typedef struct gdm_cut_advection gdm_cut_advection;
int gdm_cut_advection_create(int fe_degree, int n_subdivisions, double left, double right, const double *level_set,
                             const double *advection /* [2] */, double ghost_parameter_A, double ghost_parameter_M,
                             int device, gdm_cut_advection **out);
/* cells[3] = inside, intersected, outside */
int gdm_cut_advection_info(const gdm_cut_advection *c, int64_t *n_dofs, int64_t *n_bc_points, int64_t *cells,
                           int64_t *mass_bandwidth);
int gdm_cut_advection_bc_points(const gdm_cut_advection *c, double *xy_host /* [n_bc_points][2] */);
int gdm_cut_advection_op(gdm_cut_advection *c, gdm_op **op);
int gdm_cut_advection_compute_rhs(gdm_cut_advection *c, const double *u, const double *bc, double *rhs);
int gdm_cut_advection_mass_solve(gdm_cut_advection *c, const double *rhs, double *x);
int gdm_cut_advection_destroy(gdm_cut_advection *c);
/* Composite advection (advection-app.cc's preset: params.composite, problem.h
 * :103-181; ABI v10): one handle per field.  location GDM_CUT_INSIDE (phi < 0,
 * params.advection) or GDM_CUT_OUTSIDE (phi > 0, params.advection_1; the
 * region, its box-face parts, the surface normal (stiffness.h:437), the ghost
 * penalty and the mass of MassMatrixOperator(location) follow the sign).
 * flags GDM_CUT_ADV_COMPOSITE: the inflow value u+ of the cut-surface term (II)
 * is the partner field evaluated at the surface point (stiffness.h:448-453),
 * so the surface points are no stage boundary points (collect_boundary_points
 * :115) and gdm_cut_advection_couple adds that part: rhs += P u_partner
 * (u_partner: the other field's DoF vector, same numbering).  compute_rhs(u,
 * bc, rhs) + couple(u_partner, rhs) = the field's block of compute_rhs
 * (stiffness.h:196-214); the box-face inflow (III) still reads bc.
 * gdm_cut_advection_create = create2(..., GDM_CUT_INSIDE, 0, ...). */
#define GDM_CUT_ADV_COMPOSITE 1
int gdm_cut_advection_create2(int fe_degree, int n_subdivisions, double left, double right, const double *level_set,
                              const double *advection /* [2] */, double ghost_parameter_A, double ghost_parameter_M,
                              int location, int flags, int device, gdm_cut_advection **out);
int gdm_cut_advection_couple(gdm_cut_advection *c, const double *u_partner, double *rhs);

/* ------------------------------------------------------------------------
 * Cut-cell wave / heat / poisson (applications/wave, dim 1 and
 * 2: the "wave", "heat-rk", "heat-impl", "heat-composite", "wave-composite"
 * and "step85" presets of wave-app.cc): the device operators of
 * the reference's wave application on a GDM line / square cut by the FE_Q(k)
 * interpolant of a level set (WaveProblem<dim>, wave/problem.h).
 *
 *   compute_rhs   rhs = [u != NULL] (Z S u + C u) + Ff fq + Fg gs
 *                 (wave/stiffness.h:42-407): S = the uncut wave stencil
 *                 -(grad v, grad u) of the box (gdm_op kind wave), Z zeroes
 *                 the rows of the DoFs in the box of a cell that is not fully
 *                 inside, C = those rows of -(grad v, grad u)_inside in full
 *                 + the surface Nitsche terms (:205-259, gamma_D = nitsche) +
 *                 the ghost penalty -0.5 gamma_A h [d_n v][d_n u] on the faces
 *                 (:330-395); Ff fq = (v, f) with fq = f at the inside
 *                 quadrature points, Fg gs = the Nitsche data
 *                 (gamma_D / h v - d_n v, g) with gs = g at the surface points
 *                 (either may be NULL: zero data).  Host assembly
 *                 csrc/gdm_cut_wave.cpp, device CSR products.
 *   mass_apply    out = M u, M = (v, u)_inside + 0.5 gamma_M h^3 [d_n v][d_n u],
 *                 zero diagonals -> 1 (wave/mass.h:47-249); gamma_M < 0 (the
 *                 reference's "not set", e.g. step85): no mass matrix
 *   mass_solve    x = M^-1 rhs (banded Cholesky: host factor, device
 *                 triangular solves; wave/problem.h:457-502)
 *   system_solve  x = (M + dt K)^-1 rhs, K the assembled stiffness matrix
 *                 (stiffness.h:602-800: (grad v, grad u)_inside + surface
 *                 Nitsche + 0.5 gamma_A h^3 [d_n v][d_n u], zero diagonals ->
 *                 1; heat-impl); refactored when dt changes
 *   stiffness_solve  x = K^-1 rhs (the "poisson" simulation type, problem.h:46-71)
 *   eval          vals = u_h at the inside quadrature points (the
 *                 postprocess of problem.h:504-615 reduces them with the
 *                 exact solution and the weights from gdm_cut_wave_points)
 * ls_values: per cell (lexicographic, x fastest) the level set at its
 * (k + 1)^dim Gauss-Lobatto support points (x fastest): the FE_Q(k)
 * interpolant.  Cells are classified by the signs of its Bernstein
 * coefficients (NonMatching::MeshClassifier); intersected cells get deal.II's
 * QuadratureGenerator (Saye) on the cell polynomial.  DoFs: vertices,
 * lexicographic (x fastest).  Vectors: device pointers (n_dofs, n_quad,
 * n_surface doubles).
 *
 * Composite presets (heat-composite, wave-composite; dim 1 and 2): one handle per
 * field, location GDM_CUT_INSIDE (phi < 0) or GDM_CUT_OUTSIDE (phi > 0), each
 * with its region's quadrature, mass and ghost-penalty faces (an intersected
 * cell and a neighbour not of the other location); flags select the Nitsche
 * data: GDM_CUT_WAVE_INTERFACE_DATA (II, the surface points; the presets
 * without composite), GDM_CUT_WAVE_DOMAIN_DATA (IV, the domain boundary faces
 * in the region, stiffness.h:262-330) and GDM_CUT_WAVE_COUPLED (the interface
 * terms of compute_rhs(BlockVector), stiffness.h:420-575: the own field's
 * part in compute_rhs, the partner's added by gdm_cut_wave_couple(c,
 * u_partner, rhs)).  The data points of gdm_cut_wave_points (sx, sn) are, cell
 * by cell, the interface points followed by the Gauss points of the cell's
 * domain faces (QGauss(p + 1) per face in 2D, outward normal), as selected.
 * A domain boundary face the level set crosses is refused (2D).
 * ------------------------------------------------------------------------ */
typedef struct gdm_cut_wave gdm_cut_wave;
#define GDM_CUT_INSIDE (-1)
#define GDM_CUT_OUTSIDE 1
#define GDM_CUT_WAVE_INTERFACE_DATA 1
#define GDM_CUT_WAVE_DOMAIN_DATA 2
#define GDM_CUT_WAVE_COUPLED 4
int gdm_cut_wave_create(int dim, int fe_degree, int n_subdivisions, double left, double right, int ls_degree,
                        const double *ls_values, int location, int flags, double gamma_M, double gamma_A,
                        double nitsche, int device, gdm_cut_wave **out);
/* cells[3] = inside, intersected, outside */
int gdm_cut_wave_info(const gdm_cut_wave *c, int64_t *n_dofs, int64_t *n_quad, int64_t *n_surface, int64_t *cells);
/* host arrays: quadrature points [n_quad][dim] and JxW [n_quad], surface points and unit normals [n_surface][dim] */
int gdm_cut_wave_points(const gdm_cut_wave *c, double *qx, double *qw, double *sx, double *sn);
int gdm_cut_wave_op(gdm_cut_wave *c, gdm_op **op);
int gdm_cut_wave_compute_rhs(gdm_cut_wave *c, const double *u, const double *fq, const double *gs, double *rhs);
int gdm_cut_wave_couple(gdm_cut_wave *c, const double *u_other, double *rhs);
int gdm_cut_wave_mass_apply(gdm_cut_wave *c, const double *u, double *out);
int gdm_cut_wave_mass_solve(gdm_cut_wave *c, const double *rhs, double *x);
int gdm_cut_wave_system_solve(gdm_cut_wave *c, double dt, const double *rhs, double *x);
int gdm_cut_wave_stiffness_solve(gdm_cut_wave *c, const double *rhs, double *x);
int gdm_cut_wave_eval(gdm_cut_wave *c, const double *u, double *vals);
int gdm_cut_wave_destroy(gdm_cut_wave *c);

#ifdef __cplusplus
}
#endif

#endif /* GDM_HIP_H */

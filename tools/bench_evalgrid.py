#!/usr/bin/env python3
"""Time the grid evaluation (gdm_eval_grid, gdm_add_load_grad, gdm_eval_trace;
csrc/gdm_evalgrid.hip) and one stage of QuasilinearHeatProblem next to two
yardsticks measured in the same process.  One process.

Legs (3D, --degree, --n^3 DoFs):
  ms_values        eval_grid, values only
  ms_values_grad   eval_grid, values and gradients
  ms_flux          add_load_grad
  ms_load          add_load (the value integral), for scale
  ms_trace         eval_trace, both outputs
  ms_stage_eval / ms_stage_pointwise / ms_stage_apply
                   one QuasilinearHeatProblem stage at nitsche = 6 p^2, kappa
                   = 1 + u^2: eval_grid + eval_trace, the torch pointwise work
                   with the in-place copies, the grid-coefficient apply
  ms_copy          a plain device copy of --copy-mb megabytes; its rate (read
                   + write) is the streaming rate of the memory bound
Each leg settles (back-to-back launches for --settle-ms), warms up, then times
--steps launches between two events; the legs alternate --rounds times and the
smallest mean per leg is reported (the procedure of tools/bench_coefgrid.py).

Memory bound of a leg: its compulsory bytes (8 per DoF read or read + written,
8 per Gauss point and component written or read) at the copy's rate;
fraction_* = bound / measured.

SpMV yardstick (the elasticity benchmark's): the interpolation matrix (B_z (x)
B_y (x) B_x) assembled with scipy from gdm_coef_grid_tables_1d and applied with
gdm_csr_vmult, at the largest mesh with at most --spmv-nnz non-zeros; the
values-only evaluation is timed on that mesh too.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))


def interpolation_matrix(op):
    """(B_z (x) B_y (x) B_x) as scipy CSR, x fastest"""
    import numpy as np
    import scipy.sparse as sp

    n1 = op.p + 1
    E = None
    for d in range(op.dim):
        val, _, first = op.coef_grid_tables_1d(d)
        val, first = np.asarray(val).reshape(-1, n1), np.asarray(first).reshape(-1)
        rows = np.repeat(np.arange(val.shape[0]), n1)
        cols = (first[:, None] + np.arange(n1)[None, :]).reshape(-1)
        B = sp.csr_matrix((val.reshape(-1), (rows, cols)), shape=(val.shape[0], op.mesh.n_subdivisions[d] + 1))
        E = B if E is None else sp.kron(B, E, format="csr")
    return E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="DoFs per direction")
    ap.add_argument("--degree", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copy-mb", type=int, default=1024)
    ap.add_argument("--spmv-nnz", type=float, default=1.5e8, help="non-zeros of the SpMV yardstick (0: skip)")
    args = ap.parse_args()

    import torch

    import gdm_amd

    p, n = args.degree, args.n - 1
    nitsche = 6.0 * p * p
    op = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(nitsche,))
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    nq, nb = op.n_grid_points, op.n_bc_points
    uq = torch.empty(nq, dtype=torch.float64, device="cuda")
    gq = torch.empty(3 * nq, dtype=torch.float64, device="cuda")
    ub = torch.empty(nb, dtype=torch.float64, device="cuda")
    db = torch.empty(nb, dtype=torch.float64, device="cuda")
    dst = op.new_vector(local=False)
    ca = torch.zeros(args.copy_mb * (1 << 20) // 8, dtype=torch.float64, device="cuda")
    cb = torch.ones_like(ca)
    stream = torch.cuda.current_stream()

    def kappa(v):
        return 1.0 + v * v

    prob = gdm_amd.QuasilinearHeatProblem(op, kappa)
    prob.u.copy_(u)
    prob.rhs(0.0, prob.u, dst)  # sets the coefficient from the initial u

    def stage_pointwise():
        prob.kq.copy_(kappa(uq))
        prob.kbc.copy_(kappa(ub))

    def stage_eval():
        op.eval_grid(u, uq, False)
        op.eval_trace(u, ub, False)

    op.eval_grid(u, uq, gq)
    legs = {
        "ms_values": lambda: op.eval_grid(u, uq, False),
        "ms_values_grad": lambda: op.eval_grid(u, uq, gq),
        "ms_flux": lambda: op.add_load_grad(gq, dst),
        "ms_load": lambda: op.add_load(uq, dst),
        "ms_trace": lambda: op.eval_trace(u, ub, db),
        "ms_stage_eval": stage_eval,
        "ms_stage_pointwise": stage_pointwise,
        "ms_stage_apply": lambda: op.apply(u, dst),
        "ms_copy": lambda: ca.copy_(cb),
    }

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    runs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            runs[k].append(timed(fn, args.steps))
    out = {k: min(v) for k, v in runs.items()}
    dofs = op.n_owned
    rate = 2.0 * ca.numel() * 8 / (out["ms_copy"] * 1e-3)  # bytes / s, read + write
    bound = {
        "values": 8.0 * (dofs + nq),
        "values_grad": 8.0 * (dofs + 4 * nq),
        "flux": 8.0 * (2 * dofs + 3 * nq),
        "load": 8.0 * (2 * dofs + nq),
        "trace": 8.0 * 2 * nb,
    }
    for k, b in bound.items():
        out["bound_ms_" + k] = b / rate * 1e3
        out["fraction_" + k] = out["bound_ms_" + k] / out["ms_" + k]
    out.update({"dofs": dofs, "degree": p, "grid_points": nq, "bc_points": nb, "copy_tb_s": rate / 1e12,
                "ms_stage": out["ms_stage_eval"] + out["ms_stage_pointwise"] + out["ms_stage_apply"],
                "eval_over_apply": out["ms_stage_eval"] / out["ms_stage_apply"],
                "steps": args.steps, "rounds": args.rounds,
                "runs": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    del prob, op, u, uq, gq, ub, db, dst, ca, cb, legs
    torch.cuda.empty_cache()

    if args.spmv_nnz > 0:
        n1 = p + 1
        ns = p
        while ((ns + 1) * n1) ** 3 * n1 ** 3 <= args.spmv_nnz:
            ns += 1
        sop = gdm_amd.GdmOperator(3, p, ns, 0.0, 1.0, "wave")
        t0 = time.perf_counter()
        E = interpolation_matrix(sop)
        assemble_s = time.perf_counter() - t0
        M = gdm_amd.SparseMatrix.from_scipy(E)
        su = torch.rand(sop.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        s1 = torch.empty(sop.n_grid_points, dtype=torch.float64, device="cuda")
        s2 = torch.empty_like(s1)
        ms_csr, ms_ev = [], []
        for _ in range(args.rounds):
            ms_csr.append(timed(lambda: M.vmult(s2, su), args.steps))
            ms_ev.append(timed(lambda: sop.eval_grid(su, s1, False), args.steps))
        out.update({"spmv_n_sub": ns, "spmv_nnz": int(E.nnz), "spmv_assemble_s": round(assemble_s, 2),
                    "spmv_ms_csr": min(ms_csr), "spmv_ms_values": min(ms_ev),
                    "spmv_csr_over_values": min(ms_csr) / min(ms_ev),
                    "spmv_rel_diff": float((s1 - s2).norm() / s2.norm())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

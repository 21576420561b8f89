#!/usr/bin/env python3
"""Linear elasticity on uncut boxes (GDM_OP_ELASTICITY): the matrix-free apply
next to the assembled matrix through gdm_csr_vmult, and the CG solve with the
Jacobi and the block fast-diagonalisation preconditioner.

  python tools/bench_elasticity.py [--apply 2:5:511 3:3:47] [--apply-only 3:3:191 3:5:191]
                                   [--solve 3:3:64 2:3:512] [--iters 20]

Cases are DIM:P:N_SUB (cube of N_SUB cells per direction, mu = 1; lambda = 2.5
for the apply, 0 for the solve).  One JSON line per case.

apply:
  apply_ms        gdm_apply, mean of back-to-back calls between two device
                  events (at least --iters and at least ~0.1 s of them) after
                  >= 0.5 s of the same calls
  csr_ms          the yardstick: P A P + I - P assembled here with scipy from
                  the product's own host tables (gdm_elasticity_tables_1d) and
                  applied with gdm_csr_vmult, timed the same way in the same
                  process; nnz_per_row of it
  csr_over_apply  > 1: the matrix-free apply is faster
  gflops          the FMA count of the shipped kernel per vertex (x sweeps 4 (2p+1)
                  per source on the tile with its y halo, the y sweeps of the
                  factor pairs that occur, the z march 4 dim (2p+1)) times 2, over
                  apply_ms
  hbm_bytes_per_dof  16: every component read once and written once (the tile
                  halo re-reads are served by the caches and not counted)
  rel_diff        rel-L2 difference of the two results
solve (zero start, ReductionControl(1000, 1e-10, 1e-8), random right-hand side):
  per preconditioner iterations, wall time of the whole call (host clock around
  a call that ends synchronised) and the time per iteration.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))

TILE_Y = 8


def timed(torch, fn, iters):
    t0 = time.perf_counter()
    calls = 0
    while True:  # warm-up: code objects, the clock
        for _ in range(3):
            fn()
        calls += 3
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > 0.5:
            break
    # a timed window of at least ~0.1 s, whatever the size of one call
    iters = max(iters, int(0.1 * calls / (time.perf_counter() - t0)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def dense_band(B, p):
    import scipy.sparse

    n = B.shape[0]
    return scipy.sparse.diags([B[max(0, p - k):n - max(0, k - p), k] for k in range(2 * p + 1)],
                              [k - p for k in range(2 * p + 1)], shape=(n, n), format="csr")


def assemble(op, mu, lam):
    """P A P + I - P as a scipy CSR matrix from the product's host tables"""
    import scipy.sparse as sp

    dim, p = op.dim, op.p
    F = []
    for d in range(dim):
        bands = op.elasticity_tables_1d(d)[0]
        F.append([dense_band(bands[f], p) for f in range(4)])  # M, C, C^T, L
    N = [F[d][0].shape[0] for d in range(dim)]

    def kron(fs):  # x fastest = the last Kronecker factor
        out = sp.identity(1, format="csr")
        for d in reversed(range(dim)):
            out = sp.kron(out, F[d][fs[d]], format="csr")
        return out

    blocks = [[None] * dim for _ in range(dim)]
    for c in range(dim):
        for e in range(dim):
            if c == e:
                blocks[c][e] = sum((2 * mu + lam if d == c else mu) * kron([3 if a == d else 0 for a in range(dim)])
                                   for d in range(dim))
            else:
                blocks[c][e] = mu * kron([1 if a == e else (2 if a == c else 0) for a in range(dim)]) + \
                    lam * kron([1 if a == c else (2 if a == e else 0) for a in range(dim)])
    A = sp.bmat(blocks, format="csr")
    free = np.ones(N[::-1])
    for ax in range(dim):
        idx = [slice(None)] * dim
        for end in (0, -1):
            idx[ax] = end
            free[tuple(idx)] = 0.0
    A = A + sp.diags(1.0 - np.tile(free.reshape(-1), dim))
    A.sum_duplicates()
    return A.tocsr()


def fma_per_vertex(dim, p):
    W = 2 * p + 1
    pairs = {2: 4, 3: 7}[dim]  # (x, y) factor pairs per source component
    x = 4 * W * (TILE_Y + 2 * p) / TILE_Y
    z = 4 * dim * W if dim == 3 else 0
    return dim * (x + pairs * W) + z


def bench_apply(torch, gdm_amd, dim, p, n, iters, with_csr=True):
    mu, lam = 1.0, 2.5
    op = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "elasticity", params=(mu, lam))
    u = op.new_vector_field().uniform_(-1, 1)
    y, y2 = op.new_vector_field(), op.new_vector_field()
    res = {"kind": "apply", "dim": dim, "p": p, "n_sub": n, "n_dofs": int(u.numel())}
    res["apply_ms"] = timed(torch, lambda: op.apply(u, y), iters)
    res["gflops"] = 2.0 * fma_per_vertex(dim, p) * op.n_owned / res["apply_ms"] * 1e-6
    res["hbm_bytes_per_dof"] = 16
    res["gbytes_per_s"] = 16.0 * u.numel() / res["apply_ms"] * 1e-6
    if not with_csr:
        return res
    t0 = time.perf_counter()
    A = assemble(op, mu, lam)
    res["assemble_s"] = round(time.perf_counter() - t0, 2)
    res["nnz_per_row"] = A.nnz / A.shape[0]
    M = gdm_amd.SparseMatrix.from_scipy(A)
    res["csr_ms"] = timed(torch, lambda: M.vmult(y2, u), iters)
    res["csr_over_apply"] = res["csr_ms"] / res["apply_ms"]
    res["rel_diff"] = float((y - y2).norm() / y2.norm())
    return res


def bench_solve(torch, gdm_amd, dim, p, n):
    op = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "elasticity", params=(1.0, 0.0))
    b = op.new_vector_field().uniform_(-1, 1)
    res = {"kind": "solve", "dim": dim, "p": p, "n_sub": n, "n_dofs": int(b.numel())}
    t0 = time.perf_counter()
    op.elasticity_precond_setup()
    res["precond_setup_s"] = round(time.perf_counter() - t0, 3)
    for pc in ("jacobi", "fastdiag"):
        x = op.new_vector_field()
        try:  # warm-up: code objects, work vectors (stops at max_it by design)
            op.elasticity_solve(b, x, pc, max_it=5)
        except gdm_amd.GdmError:
            pass
        best = None
        for _ in range(3):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its, r = op.elasticity_solve(b, x, pc, 1e-8, 1e-10, 100000)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        res[pc] = {"iterations": its, "residual": r, "wall_ms": best * 1e3, "ms_per_iteration": best * 1e3 / max(its, 1)}
    res["jacobi_over_fastdiag_time"] = res["jacobi"]["wall_ms"] / res["fastdiag"]["wall_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--apply", nargs="*", default=["2:5:511", "3:3:47"])
    ap.add_argument("--apply-only", nargs="*", default=["3:3:191", "3:5:191"],
                    help="apply without the CSR yardstick (sizes whose matrix does not fit)")
    ap.add_argument("--solve", nargs="*", default=["3:3:64", "2:3:512"])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch

    import gdm_amd

    if not torch.cuda.is_available():
        raise SystemExit("bench_elasticity: no GPU visible (there is no CPU path)")
    for case in args.apply:
        dim, p, n = (int(v) for v in case.split(":"))
        print(json.dumps(bench_apply(torch, gdm_amd, dim, p, n, args.iters)), flush=True)
        torch.cuda.empty_cache()
    for case in args.apply_only:
        dim, p, n = (int(v) for v in case.split(":"))
        print(json.dumps(bench_apply(torch, gdm_amd, dim, p, n, args.iters, with_csr=False)), flush=True)
        torch.cuda.empty_cache()
    for case in args.solve:
        dim, p, n = (int(v) for v in case.split(":"))
        print(json.dumps(bench_solve(torch, gdm_amd, dim, p, n)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of the direct heat-implicit / Poisson solve (gdm_system_solve) on an
uncut cube, next to the same six contractions written in torch.

  python tools/bench_fastdiag.py [--n 128 256] [--p 5 7] [--iters 20]

Per (n, p) one JSON line:
  solve_ms        gdm_system_solve(1, dt), mean of --iters back-to-back calls
                  between two device events, after a warm-up of at least half a
                  second of the same calls (settled clock)
  tflops, share   12 N flops per DoF (six N x N contractions) over solve_ms,
                  and that rate over the 42.7 TF measured for
                  v_mfma_f64_16x16x4_f64 (tools/microbench/fp64_pipes.hip)
  torch_ms        the outside yardstick: S^T along x, y, z, the diagonal
                  scaling, S along z, y, x with torch.matmul on the same tables
                  and the same vector (x: rows times T^T; y: batched T times the
                  (Ny, Nx) planes; z: T times the (Nz, Ny Nx) matrix), timed the
                  same way
  solve_over_torch  the target is <= 1.25
  rel_diff        rel-L2 difference of the two results
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))

PIPE_TF = 42.7


def timed(torch, fn, iters):
    t0 = time.perf_counter()
    while True:  # warm-up: code objects, library heuristics, the clock
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > 0.5:
            break
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--p", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch

    import gdm_amd

    alpha, tau = 1.0, 1e-3
    for n in args.n:
        for p in args.p:
            op = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(15.0,))
            t0 = time.perf_counter()
            op.system_solve_setup()
            setup_s = time.perf_counter() - t0
            N = n + 1
            rhs = op.new_vector(False).uniform_(-1, 1)
            x = op.new_vector(False)
            S, lam = op.fastdiag_tables(0)  # a cube: one table for the three directions
            Sd, lamd = torch.from_numpy(S).cuda(), torch.from_numpy(lam).cuda()
            Std = Sd.t().contiguous()
            inv = 1.0 / (alpha + tau * (lamd[:, None, None] + lamd[None, :, None] + lamd[None, None, :]))

            def torch_solve():
                v = torch.matmul(rhs.view(N * N, N), Sd)          # x: rows times (S^T)^T
                v = torch.matmul(Std, v.view(N, N, N))            # y, batched over z
                v = torch.matmul(Std, v.view(N, N * N))           # z
                v = v.view(N, N, N) * inv
                v = torch.matmul(Sd, v.view(N, N * N))            # z
                v = torch.matmul(Sd, v.view(N, N, N))             # y
                return torch.matmul(v.view(N * N, N), Std)        # x

            res = {"n": n, "p": p, "n_dofs": op.n_owned, "setup_s": round(setup_s, 3)}
            res["solve_ms"] = timed(torch, lambda: op.system_solve(alpha, tau, rhs, x), args.iters)
            flops = 12.0 * N * op.n_owned
            res["tflops"] = flops / res["solve_ms"] * 1e-9
            res["share_of_fp64_mfma"] = res["tflops"] / PIPE_TF
            res["torch_ms"] = timed(torch, torch_solve, args.iters)
            res["solve_over_torch"] = res["solve_ms"] / res["torch_ms"]
            ref = torch_solve().reshape(-1)
            res["rel_diff"] = float((x - ref).norm() / ref.norm())
            print(json.dumps(res), flush=True)
            del op, rhs, x, Sd, Std, inv, ref
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

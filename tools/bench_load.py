#!/usr/bin/env python3
"""Timings of the forcing / Dirichlet-data entry points (gdm_add_load_fn,
gdm_add_load, gdm_add_dirichlet_data) on a wave operator with box Nitsche.

  python tools/bench_load.py [--n 256] [--p 5 7] [--iters 10] [--no-array]

Per degree it prints one JSON line with, in ms (median of --iters timed calls
after two warm-up calls, HIP events on the operator's stream):
  axpby          gdm_vec_axpby over n_owned (24 B/DoF), the yardstick of
  load_fn_sine   the rank-1 add_load_fn (16 B/DoF)
  error_norms    gdm_error_norms, the forward mirror of the general kernel
  load_cone      the general kernel evaluating the cone in place
  load_array     the general kernel reading fq (8 (p+1)^3 bytes per cell), with
                 the achieved bandwidth of that read alone
  dirichlet      add_dirichlet_data
  stage / stage_data   one WaveProblem RK4 step / 4 without and with sine
                 forcing and Dirichlet data
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))

SINE = [0.8, 0.0, 0.0, 1.0, 0.5, 0.75, 0.3, 0.5, 0.2]


def timed(torch, fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--p", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-array", action="store_true", help="skip add_load (its fq array: 8 (n (p+1))^3 bytes)")
    args = ap.parse_args()
    import torch

    import gdm_amd

    for p in args.p:
        n = args.n
        op = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(15.0,))
        dst, x = op.new_vector(False), op.new_vector(False)
        x.uniform_(-1, 1)
        g = torch.rand(op.n_bc_points, dtype=torch.float64, device="cuda")
        res = {"n": n, "p": p, "n_dofs": op.n_owned}
        res["axpby_ms"] = timed(torch, lambda: op.axpby(1.0, x, 1.0, dst), args.iters)
        res["load_fn_sine_ms"] = timed(torch, lambda: op.add_load_fn(2, SINE, 0.3, dst), args.iters)
        res["load_fn_sine_over_axpby"] = res["load_fn_sine_ms"] / res["axpby_ms"]
        res["error_norms_ms"] = timed(torch, lambda: op.error_norms(x, 2, SINE, 0.3), max(3, args.iters // 3))
        cone = [0.45, 0.5, 0.55, 0.6]
        res["load_cone_ms"] = timed(torch, lambda: op.add_load_fn(1, cone, 0.0, dst), max(3, args.iters // 3))
        res["load_cone_over_error_norms"] = res["load_cone_ms"] / res["error_norms_ms"]
        res["dirichlet_ms"] = timed(torch, lambda: op.add_dirichlet_data(g, dst), args.iters)
        if not args.no_array:
            nq = (n * (p + 1)) ** 3
            try:
                fq = torch.empty(nq, dtype=torch.float64, device="cuda").uniform_(-1, 1)
                res["load_array_ms"] = timed(torch, lambda: op.add_load(fq, dst), 3)
                res["load_array_over_error_norms"] = res["load_array_ms"] / res["error_norms_ms"]
                res["load_array_fq_GBps"] = 8.0 * nq / res["load_array_ms"] * 1e-6
                del fq
            except RuntimeError as e:  # the array does not fit: say so
                res["load_array_ms"] = None
                res["load_array_note"] = str(e).splitlines()[0][:120]
            torch.cuda.empty_cache()
        plain = gdm_amd.WaveProblem(op)
        data = gdm_amd.WaveProblem(op, forcing=(2, SINE, 30.0), dirichlet=(2, SINE))
        for prob in (plain, data):
            prob.u.uniform_(-1e-3, 1e-3)
        res["stage_ms"] = timed(torch, lambda: plain.step(0.0, 1e-6), 5) / 4
        res["stage_data_ms"] = timed(torch, lambda: data.step(0.0, 1e-6), 5) / 4
        res["stage_data_over_stage"] = res["stage_data_ms"] / res["stage_ms"]
        print(json.dumps(res), flush=True)
        del op, plain, data, dst, x, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

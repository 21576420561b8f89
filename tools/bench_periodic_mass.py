#!/usr/bin/env python3
"""Time the exact periodic mass inverse (gdm_mass_solve_periodic) next to the
Jacobi-CG it replaces and to the non-periodic exact inverse of the same mesh,
every direction periodic, on the stream the operators use.

  ms_direct       gdm_mass_solve_periodic (line passes + one correction per direction)
  ms_cg           gdm_mass_solve_cg(rel 1e-8, Jacobi) from a zero initial guess
                  (the solve of prototypes/advection_01_gdm.cc:208-217; its host
                  reads of the dot products are part of the solve)
  ms_nonperiodic  gdm_mass_solve on the same mesh without constraints

Each leg settles (back-to-back solves for --settle-ms, the clocks ramp over
the first launches of a fresh process), warms up, then times --steps solves
between two events; the three legs alternate --rounds times and the smallest
mean per leg is reported (runs: every round, the spread).  The budget of
ratio_direct_nonperiodic from the code is 1 + the touched share of the vector
summed over the directions (budget).  Prints one JSON line.

  tools/bench_periodic_mass.py --dim 1 --degree 3 --cells 1024      # C1
  tools/bench_periodic_mass.py --dim 3 --degree 5 --cells 255       # 256^3 DoFs
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--degree", type=int, default=5)
    ap.add_argument("--cells", type=int, default=255, help="cells per direction")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    import gdm_amd

    dim, p, n = args.dim, args.degree, args.cells
    per = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass", periodic=(1 << dim) - 1)
    plain = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass")
    gen = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.rand(per.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    rhs = per.new_vector(local=False)
    per.mass_apply(raw, rhs)  # a condensed right-hand side (constrained rows zero)
    x = per.new_vector(local=False)
    stream = torch.cuda.current_stream()
    its = []

    def direct():
        per.mass_solve_periodic(rhs, x)

    def cg():
        x.zero_()
        its.append(per.mass_solve_cg(rhs, x, rel_tol=1e-8, abs_tol=1e-10, max_it=1000, precond=1)[0])

    def nonperiodic():
        plain.mass_solve(rhs, x)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    legs = {"ms_direct": direct, "ms_cg": cg, "ms_nonperiodic": nonperiodic}
    runs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            runs[k].append(leg(fn))
    out = {k: min(v) for k, v in runs.items()}
    out["ratio_cg_direct"] = out["ms_cg"] / out["ms_direct"]
    out["ratio_direct_nonperiodic"] = out["ms_direct"] / out["ms_nonperiodic"]
    rows = []
    for d in range(dim):
        _, _, lo, hi = per.mass_periodic_tables(d)
        rows.append(lo + hi)
    out["budget"] = 1.0 + sum(r / (n + 1.0) for r in rows)
    out.update({"dim": dim, "degree": p, "cells": n, "dofs": (n + 1) ** dim, "rows_touched": rows,
                "cg_iterations": its[-1], "steps": args.steps, "rounds": args.rounds,
                "runs": {k: [round(v, 4) for v in vs] for k, vs in runs.items()}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

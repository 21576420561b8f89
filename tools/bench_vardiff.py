#!/usr/bin/env python3
"""Time the wave operator with a separable coefficient (gdm_op_set_coefficient)
next to the constant wave stencil and the separable advection field's kernel,
and the preconditioned CG on top of it (gdm_coef_solve).  One process.

Apply (3D, degree 5, 256^3 DoFs by default):
  ms_wave_const    the constant wave stencil (gdm_apply without a coefficient)
  ms_coef_t1/2/4   the coefficient apply with 1, 2 and 4 terms
  ms_field_const3  tools/bench_varfield.py's leg of the same name: a constant
                   advection field as 3 terms through the field kernel (the same
                   x and y sweeps as ms_coef_t1 with one z accumulation more)
Each leg settles (back-to-back applies for --settle-ms), warms up, then times
--steps applies between two events; the legs alternate --rounds times and the
smallest mean per leg is reported.

Solve (3D, degree 3, --solve-n cells per direction, Poisson, kappa = 1 + 9
b(x) b(y) b(z), rel_tol 1e-8): the iteration count, ms per iteration (the whole
solve over the count, host reductions included) and gdm_system_solve alone (the
preconditioner's cost).  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))


def bump(t):
    return math.exp(-((t - 0.5) / 0.2) ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="DoFs per direction of the apply legs")
    ap.add_argument("--degree", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solve-n", type=int, default=128, help="cells per direction of the solve (0: skip)")
    args = ap.parse_args()

    import torch

    import gdm_amd

    p, n = args.degree, args.n - 1
    nitsche = 6.0 * p * p
    terms = [[lambda x: 1 + 0.5 * math.sin(3 * x), math.exp, lambda z: 1 + z * z],
             [lambda x: 0.3 * (2 + x), lambda y: 1 + y, math.cos],
             [lambda x: 0.2 * math.cos(x), None, lambda z: 1 + z],
             [None, lambda y: 0.1 * (1 + y * y), None]]
    legs = {"ms_wave_const": gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(nitsche,))}
    for T in (1, 2, 4):
        op = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(nitsche,))
        op.set_coefficient(terms[:T])
        legs["ms_coef_t%d" % T] = op
    a = (1.0, 0.15, -0.05)
    field3 = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "advection", params=a)
    field3.set_advection_field([(d, [None, None, None]) for d in range(3)])
    field3.set_field_scale(a)
    legs["ms_field_const3"] = field3
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.rand(field3.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    bc = torch.rand(field3.n_bc_points, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    dst = field3.new_vector(local=False)
    stream = torch.cuda.current_stream()

    def timed(fn, steps):
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
        for _ in range(steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    runs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, op in legs.items():
            bcv = bc if k == "ms_field_const3" else None
            runs[k].append(timed(lambda op=op, bcv=bcv: op.apply(src, dst, bcv), args.steps))
    out = {k: min(v) for k, v in runs.items()}
    for T in (1, 2, 4):
        out["ratio_coef_t%d_vs_wave_const" % T] = out["ms_coef_t%d" % T] / out["ms_wave_const"]
    out["ratio_coef_t1_vs_field_const3"] = out["ms_coef_t1"] / out["ms_field_const3"]
    out.update({"dofs": args.n ** 3, "degree": p, "steps": args.steps, "rounds": args.rounds,
                "runs": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    legs.clear()
    del field3, op, src, dst, bc

    if args.solve_n > 0:
        ns = args.solve_n
        sop = gdm_amd.GdmOperator(3, 3, ns, 0.0, 1.0, "wave", params=(54.0,))
        sop.set_coefficient([[None, None, None], [lambda t: 9.0 * bump(t), bump, bump]])
        sop.system_solve_setup()
        rhs = torch.rand(sop.n_owned, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        x = sop.new_vector(local=False)
        its = 0
        solve_ms = []
        for _ in range(args.rounds):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its, _ = sop.coef_solve(0.0, 1.0, rhs, x, rel_tol=1e-8)
            torch.cuda.synchronize()
            solve_ms.append((time.perf_counter() - t0) * 1e3)
        sop.set_coefficient([])
        pre = min(timed(lambda: sop.system_solve(0.0, 1.0, rhs, x), args.steps) for _ in range(args.rounds))
        out.update({"solve_dofs": (ns + 1) ** 3, "solve_iterations": its, "solve_ms": min(solve_ms),
                    "solve_ms_per_iteration": min(solve_ms) / max(its, 1), "ms_system_solve": pre})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time compute_rhs with a separable advection field (gdm_op_set_advection_field)
next to the constant-field operator: 3D, p = 5, 256^3 DoFs, boundary data
included, on the stream the operators use.

  ms_const         the constant-field gdm_apply (the existing stencil path)
  ms_field_const3  the same constant field as 3 terms through the field kernel
  ms_rotation      rotation about an off-centre z axis plus a drift along it

Each leg settles (back-to-back applies for --settle-ms, the clocks ramp over
the first launches of a fresh process), warms up, then times --steps applies
between two events; the three legs alternate --rounds times and the smallest
mean per leg is reported.  Prints one JSON line.
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
    ap.add_argument("--n", type=int, default=256, help="DoFs per direction")
    ap.add_argument("--degree", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    import gdm_amd

    p, n = args.degree, args.n - 1
    a = (1.0, 0.15, -0.05)
    const = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "advection", params=a)
    field3 = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "advection", params=a)
    field3.set_advection_field([(d, [None, None, None]) for d in range(3)])
    field3.set_field_scale(a)
    rot = gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "advection", params=a)
    rot.set_advection_field([(0, [None, lambda y: -(y - 0.3), None]), (1, [lambda x: x - 0.25, None, None]),
                             (2, [None, None, lambda z: 0.35])])
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.rand(const.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    bc = torch.rand(const.n_bc_points, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    dst = const.new_vector(local=False)
    stream = torch.cuda.current_stream()

    def leg(op):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            for _ in range(10):
                op.apply(src, dst, bc)
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            op.apply(src, dst, bc)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            op.apply(src, dst, bc)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    legs = {"ms_const": const, "ms_field_const3": field3, "ms_rotation": rot}
    runs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, op in legs.items():
            runs[k].append(leg(op))
    out = {k: min(v) for k, v in runs.items()}
    out["ratio_field_const3"] = out["ms_field_const3"] / out["ms_const"]
    out["ratio_rotation"] = out["ms_rotation"] / out["ms_const"]
    out.update({"dofs": args.n ** 3, "degree": p, "steps": args.steps, "rounds": args.rounds,
                "runs": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

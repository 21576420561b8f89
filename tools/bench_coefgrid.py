#!/usr/bin/env python3
"""Time the wave operator with a general coefficient on the Gauss grid
(gdm_op_set_coefficient_grid, csrc/gdm_coefgrid.hip) next to the constant wave
stencil and the separable coefficient's kernel, remeasured in the same process,
and the preconditioned CG on top of it (gdm_coef_solve).  One process.

Apply (3D, --degree, --n^3 DoFs):
  ms_coef_grid     the grid coefficient apply (volume kernel + box faces)
  ms_wave_const    the constant wave stencil
  ms_coef_t1/t4    the separable coefficient apply with 1 and 4 terms
  ms_copy          a plain device copy of --copy-mb megabytes; its rate
                   (read + write) is the streaming rate of the memory bound
Each leg settles (back-to-back launches for --settle-ms), warms up, then times
--steps launches between two events; the legs alternate --rounds times and the
smallest mean per leg is reported (the procedure of tools/bench_vardiff.py).

Derived bounds for the grid apply, per DoF: memory = (8 (p+1)^3 bytes of kappa +
16 bytes of src and dst) / the copy's rate; compute = 2 (3 (p+1)^4 + 3 (p+1)^3 +
2 (p+1)^2) FMAs / (78.6 TF/s / 2), the FP64 vector peak.  fraction_of_bound =
the larger bound's time / ms_coef_grid.

Solve (3D, degree 3, --solve-n cells per direction, Poisson, the Lorentzian
kappa = 1 + 9 / (1 + 40 sum_d (x_d - 0.5 + 0.1 d)^2), rel_tol 1e-8): iterations,
total ms, ms per iteration.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-galerkin-difference-methods_amd"))

FP64_VECTOR_PEAK = 78.6e12  # flop/s


def grid_tensor(op, torch, fn):
    """fn(x, y, z) on the tensor Gauss grid, evaluated on the device, x fastest"""
    xq = [torch.from_numpy(q).cuda() for q in op.quadrature_points()]
    return fn(xq[0][None, None, :], xq[1][None, :, None], xq[2][:, None, None]).contiguous().reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="DoFs per direction of the apply legs")
    ap.add_argument("--degree", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copy-mb", type=int, default=1024)
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

    def wave():
        return gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(nitsche,))

    def kappa(x, y, z):
        return 2 + torch.sin(3 * x * y + 2 * z) + 0.5 * torch.cos(5 * (x - y * z))

    grid = wave()
    kq = grid_tensor(grid, torch, kappa)
    bp = torch.from_numpy(grid.bc_points()).cuda()
    kbc = kappa(bp[:, 0], bp[:, 1], bp[:, 2]).contiguous()
    grid.set_coefficient_grid(kq, kbc)
    legs = {"ms_coef_grid": grid, "ms_wave_const": wave()}
    for T in (1, 4):
        op = wave()
        op.set_coefficient(terms[:T])
        legs["ms_coef_t%d" % T] = op
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.rand(grid.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    dst = grid.new_vector(local=False)
    ca = torch.zeros(args.copy_mb * (1 << 20) // 8, dtype=torch.float64, device="cuda")
    cb = torch.ones_like(ca)
    stream = torch.cuda.current_stream()

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

    runs = {k: [] for k in list(legs) + ["ms_copy"]}
    for _ in range(args.rounds):
        for k, op in legs.items():
            runs[k].append(timed(lambda op=op: op.apply(src, dst), args.steps))
        runs["ms_copy"].append(timed(lambda: ca.copy_(cb), args.steps))
    out = {k: min(v) for k, v in runs.items()}
    dofs, n1 = args.n ** 3, p + 1
    copy_rate = 2.0 * ca.numel() * 8 / (out["ms_copy"] * 1e-3)
    bytes_per_dof = 8.0 * n1 ** 3 * (n / args.n) ** 3 + 16.0
    fma_per_dof = 2.0 * (3 * n1 ** 4 + 3 * n1 ** 3 + 2 * n1 ** 2)
    ms_mem = dofs * bytes_per_dof / copy_rate * 1e3
    ms_fma = dofs * fma_per_dof / (FP64_VECTOR_PEAK / 2) * 1e3
    out.update({"dofs": dofs, "degree": p, "kappa_gb": kq.numel() * 8 / 1e9, "copy_tb_s": copy_rate / 1e12,
                "bound_ms_memory": ms_mem, "bound_ms_fma": ms_fma,
                "fraction_of_bound": max(ms_mem, ms_fma) / out["ms_coef_grid"],
                "gdof_s_coef_grid": dofs / out["ms_coef_grid"] / 1e6,
                "ratio_grid_vs_wave_const": out["ms_coef_grid"] / out["ms_wave_const"],
                "ratio_grid_vs_coef_t4": out["ms_coef_grid"] / out["ms_coef_t4"],
                "steps": args.steps, "rounds": args.rounds,
                "runs": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    legs.clear()
    del grid, op, src, dst, kq, kbc, ca, cb
    torch.cuda.empty_cache()

    if args.solve_n > 0:
        ns = args.solve_n
        sop = gdm_amd.GdmOperator(3, 3, ns, 0.0, 1.0, "wave", params=(54.0,))

        def lorentz(x, y, z):
            return 1 + 9 / (1 + 40 * ((x - 0.5) ** 2 + (y - 0.4) ** 2 + (z - 0.3) ** 2))

        skq = grid_tensor(sop, torch, lorentz)
        sbp = torch.from_numpy(sop.bc_points()).cuda()
        sop.set_coefficient_grid(skq, lorentz(sbp[:, 0], sbp[:, 1], sbp[:, 2]).contiguous())
        sop.system_solve_setup()
        rhs = torch.rand(sop.n_owned, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        x = sop.new_vector(local=False)
        its, solve_ms = 0, []
        for _ in range(args.rounds):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its, _ = sop.coef_solve(0.0, 1.0, rhs, x, rel_tol=1e-8)
            torch.cuda.synchronize()
            solve_ms.append((time.perf_counter() - t0) * 1e3)
        out.update({"solve_dofs": (ns + 1) ** 3, "solve_iterations": its, "solve_ms": min(solve_ms),
                    "solve_ms_per_iteration": min(solve_ms) / max(its, 1)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

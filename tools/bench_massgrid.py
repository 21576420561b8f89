#!/usr/bin/env python3
"""Time the mass matrix weighted by a general density on the Gauss grid
(gdm_op_set_density_grid, csrc/gdm_massgrid.hip) next to the grid coefficient's
apply, the separable density's kernel and the unweighted mass stencil,
remeasured in the same process, and the preconditioned CG on top of it
(gdm_density_solve).  One process.

Apply (3D; --cases degree:n, n^3 DoFs each; default 5:128 and 3:256):
  ms_density_grid    the grid density apply (one launch)
  ms_coef_grid       the grid coefficient apply at the same size (volume kernel
                     + box faces): the same coefficient bytes, about three times
                     the contractions
  ms_density_t1/t4   the separable density apply with 1 and 4 terms
  ms_mass_apply      the unweighted mass stencil
  ms_copy            a plain device copy of --copy-mb megabytes; its rate
                     (read + write) is the streaming rate of the memory bound
Each leg settles (back-to-back launches for --settle-ms), warms up, then times
--steps launches between two events; the legs alternate --rounds times and the
smallest mean per leg is reported (the procedure of tools/bench_coefgrid.py).

Derived bounds for the grid density apply, per DoF: memory = (8 (p+1)^3 bytes of
rho per cell + 16 bytes of src and dst) / the copy's rate; compute = (2 (p+1)^4
+ 2 (p+1)^3 + 2 (p+1)^2) FMAs (the kernel's own count without halo work:
DESIGN.md "Grid density") x 2 flop / 78.6 TF/s, the FP64 vector peak.
fraction_of_bound = the larger bound's time / ms_density_grid.

Solve (3D, degree 3, --solve-n cells per direction, the ellipse density rho = 1 +
9 exp(-(|y|^2 + y_0 y_1) / 0.15^2), y = x - 1/2, rel_tol 1e-8 from a zero guess):
iterations, total ms (host reductions included), ms per iteration.  Prints one
JSON line.
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
    ap.add_argument("--cases", default="5:128,3:256", help="degree:DoFs per direction of the apply legs, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copy-mb", type=int, default=1024)
    ap.add_argument("--solve-n", type=int, default=128, help="cells per direction of the solve (0: skip)")
    args = ap.parse_args()

    import torch

    import gdm_amd

    terms = [[lambda x: 1 + 0.5 * math.sin(3 * x), math.exp, lambda z: 1 + z * z],
             [lambda x: 0.3 * (2 + x), lambda y: 1 + y, math.cos],
             [lambda x: 0.2 * math.cos(x), None, lambda z: 1 + z],
             [None, lambda y: 0.1 * (1 + y * y), None]]

    def osc(x, y, z):
        return 2 + torch.sin(3 * x * y + 2 * z) + 0.5 * torch.cos(5 * (x - y * z))

    def ellipse(x, y, z):
        a, b, c = x - 0.5, y - 0.5, z - 0.5
        return 1 + 9 * torch.exp(-(a * a + b * b + c * c + a * b) / 0.15 ** 2)

    gen = torch.Generator(device="cuda").manual_seed(1)
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

    cases = []
    for case in args.cases.split(","):
        p, nd = (int(v) for v in case.split(":"))
        n = nd - 1

        def wave():
            return gdm_amd.GdmOperator(3, p, n, 0.0, 1.0, "wave", params=(6.0 * p * p,))

        dgrid = wave()
        rq = grid_tensor(dgrid, torch, osc)
        dgrid.set_density_grid(rq)
        kgrid = wave()
        bp = torch.from_numpy(kgrid.bc_points()).cuda()
        kbc = osc(bp[:, 0], bp[:, 1], bp[:, 2]).contiguous()
        kgrid.set_coefficient_grid(rq, kbc)  # the same samples serve as kappa
        sep = {}
        for T in (1, 4):
            sep[T] = wave()
            sep[T].set_density(terms[:T])
        plain = wave()
        src = torch.rand(dgrid.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        dst = dgrid.new_vector(local=False)
        legs = {"ms_density_grid": lambda: dgrid.density_apply(src, dst),
                "ms_coef_grid": lambda: kgrid.apply(src, dst),
                "ms_density_t1": lambda: sep[1].density_apply(src, dst),
                "ms_density_t4": lambda: sep[4].density_apply(src, dst),
                "ms_mass_apply": lambda: plain.mass_apply(src, dst),
                "ms_copy": lambda: ca.copy_(cb)}
        runs = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                runs[k].append(timed(fn, args.steps))
        out = {k: min(v) for k, v in runs.items()}
        dofs, n1 = nd ** 3, p + 1
        copy_rate = 2.0 * ca.numel() * 8 / (out["ms_copy"] * 1e-3)
        bytes_per_dof = 8.0 * n1 ** 3 * (n / nd) ** 3 + 16.0
        fma_per_dof = 2.0 * n1 ** 4 + 2.0 * n1 ** 3 + 2.0 * n1 ** 2
        ms_mem = dofs * bytes_per_dof / copy_rate * 1e3
        ms_fma = dofs * fma_per_dof * 2.0 / FP64_VECTOR_PEAK * 1e3
        out.update({"dofs": dofs, "degree": p, "rho_gb": rq.numel() * 8 / 1e9, "copy_tb_s": copy_rate / 1e12,
                    "fma_per_dof": fma_per_dof, "bound_ms_memory": ms_mem, "bound_ms_fma": ms_fma,
                    "fraction_of_bound": max(ms_mem, ms_fma) / out["ms_density_grid"],
                    "gdof_s_density_grid": dofs / out["ms_density_grid"] / 1e6,
                    "ratio_density_grid_vs_coef_grid": out["ms_density_grid"] / out["ms_coef_grid"],
                    "ratio_density_grid_vs_density_t4": out["ms_density_grid"] / out["ms_density_t4"],
                    "ratio_density_grid_vs_mass_apply": out["ms_density_grid"] / out["ms_mass_apply"],
                    "steps": args.steps, "rounds": args.rounds,
                    "runs": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
        cases.append(out)
        legs.clear()
        del dgrid, kgrid, sep, plain, src, dst, rq, kbc, bp
        torch.cuda.empty_cache()

    result = {"cases": cases}
    if args.solve_n > 0:
        ns = args.solve_n
        sop = gdm_amd.GdmOperator(3, 3, ns, 0.0, 1.0, "wave", params=(54.0,))
        sop.set_density_grid(grid_tensor(sop, torch, ellipse))
        rhs = torch.rand(sop.n_owned, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        x = sop.new_vector(local=False)
        its, solve_ms = 0, []
        for _ in range(args.rounds):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its, _ = sop.density_solve(rhs, x, rel_tol=1e-8)
            torch.cuda.synchronize()
            solve_ms.append((time.perf_counter() - t0) * 1e3)
        result.update({"solve_dofs": (ns + 1) ** 3, "solve_iterations": its, "solve_ms": min(solve_ms),
                       "solve_ms_per_iteration": min(solve_ms) / max(its, 1)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()

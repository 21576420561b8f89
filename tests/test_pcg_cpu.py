"""The library's one CG (csrc/gdm_pcg.h) on the host: host/pcg_check.cc
instantiates the template on std::vector<double> with a dense matrix, under
AddressSanitizer and UBSan, and prints the iteration count, the residual
history and x.  The same systems restated here run through vardiff_ref.pcg,
the recurrence the GPU solves are tested against.

Both sides run the same recurrence in the same order in double precision; they
differ in the summation order inside dot (sequential there, numpy's pairwise /
BLAS here) and in the matrix-vector product's.  The residuals and x agree to
1e-12 relative to the scale of the vectors they are computed from: a residual
norm relative to the initial one, x relative to max |x|.  That is the scale of
the rounding errors: r -= step Ap rounds at eps |r_0| whatever is left of r, so
the last residuals of a run (1e-11 |r_0|, or 1e-17 |r_0| where CG terminates
after `order` steps, orders 2 and 7) are known to no more than that, and their
deviation relative to their own value measures rounding noise (order 33,
Jacobi: 4.6e-9 on the last residual, 9.5e-12 |r_0|; order 7: 0.5 on the last).
Measured at order 33, the larger of the identity and the Jacobi run: 1.3e-16
on the residual history and 6.7e-16 on x, factors 7000 and 1500 below 1e-12,
which therefore stands (the rule: kept if the measurement is at least 100
times below it).  The iteration counts are equal, which pins the last
residuals to the same side of the threshold.
"""
import os
import subprocess

import numpy as np
import pytest

import vardiff_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "dealii-galerkin-difference-methods_amd", "lib", "host", "pcg_check")
ORDERS = (1, 2, 7, 33)
REL_TOL = 1e-10
BOUND = 1e-12


def run(order, *args):
    out = subprocess.run([CHECK, str(order), "--rel-tol", repr(REL_TOL), *args], check=True, capture_output=True,
                         text=True, timeout=60)
    assert out.stderr == "", out.stderr  # a sanitizer report goes to stderr
    r = {}
    for line in out.stdout.splitlines():
        key, _, rest = line.partition(" ")
        r[key] = rest
    return {"status": r["status"], "its": int(r["its"]), "applies": int(r["applies"]), "res": float(r["res"]),
            "hist": np.array(r["hist"].split(), dtype=np.float64), "x": np.array(r["x"].split(), dtype=np.float64)}


def system(n):
    i = np.arange(n)
    A = 1.0 / (1 + np.abs(i[:, None] - i[None, :])) + np.diag(i + 1.0)
    b = 1.0 + (i % 3) / 2.0 - (i % 5) / 4.0
    return A, b


def deviation(got, ref):
    """(largest deviation of a residual of the history relative to the initial one, that of x relative to max |x|)"""
    hist = np.max(np.abs(got["hist"] - ref[2])) / ref[2][0]
    return hist, np.max(np.abs(got["x"] - ref[0])) / np.max(np.abs(ref[0]))


@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("n", ORDERS)
def test_matches_reference_recurrence(n, precond):
    A, b = system(n)
    inv = 1.0 / np.diag(A)
    ref = vardiff_ref.pcg(lambda v: A @ v, (lambda r: inv * r) if precond == "jacobi" else (lambda r: r.copy()), b,
                          rel_tol=REL_TOL)
    got = run(n, "--precond", precond)
    assert got["status"] == "converged"
    assert got["its"] == ref[1]
    assert len(got["hist"]) == len(ref[2]) == got["its"] + 1
    assert got["applies"] == got["its"] + 1
    assert got["res"] == got["hist"][-1]
    dh, dx = deviation(got, ref)
    print("order %d precond %s: its %d, deviation hist %.3e x %.3e" % (n, precond, got["its"], dh, dx))
    assert dh <= BOUND and dx <= BOUND


@pytest.mark.parametrize("n", ORDERS)
def test_exact_preconditioner_one_iteration(n):
    A, b = system(n)
    got = run(n, "--precond", "exact")
    assert got["status"] == "converged" and got["its"] == 1
    x = np.linalg.solve(A, b)
    assert np.max(np.abs(got["x"] - x)) <= BOUND * np.max(np.abs(x))


@pytest.mark.parametrize("n", ORDERS)
def test_converged_at_entry(n):
    got = run(n, "--mode", "entry")
    assert got["status"] == "converged" and got["its"] == 0
    assert got["applies"] == 1  # r = b - A x alone
    assert np.all(got["x"] == 0.0) and len(got["hist"]) == 1


@pytest.mark.parametrize("n", ORDERS)
def test_nan_rhs(n):
    got = run(n, "--mode", "nan")
    assert got["status"] == "non_finite" and got["its"] == 0
    assert got["applies"] == 1 and np.isnan(got["res"])


@pytest.mark.parametrize("n", ORDERS)
def test_indefinite_breakdown(n):
    got = run(n, "--mode", "indefinite")
    if n == 1:
        # diag(1, -1, 1, ...) of order 1 is (1): positive definite, nothing breaks down
        assert got["status"] == "converged" and got["its"] == 1
        return
    assert got["status"] == "breakdown" and got["its"] == 1
    assert np.all(got["x"] == 0.0)  # the step was not taken


@pytest.mark.parametrize("n,max_it", [(1, 0), (2, 0), (7, 0), (33, 0), (7, 2), (33, 2)])
def test_max_it(n, max_it):
    # orders 1 and 2 converge within 1 and 2 iterations: only max_it = 0 is too small there
    got = run(n, "--max-it", str(max_it))
    assert got["status"] == "max_it" and got["its"] == max_it
    assert got["applies"] == max_it + 1 and len(got["hist"]) == max_it + 1
    assert got["res"] == got["hist"][-1] > REL_TOL * got["hist"][0]

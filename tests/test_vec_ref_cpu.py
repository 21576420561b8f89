"""The references and bounds of tests/test_gpu_vec.py, checked without a GPU.

  * gdm_vec_dot: tests/vec_ref.py dot_emulate restates the kernels' summation
    order (per-lane chains of the grid-stride loop, wave and block trees, the
    final kernel) in numpy float64.  On the inputs of the device test it must
    stay inside dot_bound against math.fsum -- a bound that this order of
    summation could not meet would be too tight, and that shows here.
  * gdm_vec_axpby: the longdouble reference equals exact rational arithmetic
    (fractions.Fraction) to the precision of the longdouble format, and the
    elementwise bound 2 * 2^-53 (|a x| + |b y|) of the device test holds for
    fma(a, x, b * y) evaluated exactly and rounded as the kernel rounds.
"""
from fractions import Fraction

import numpy as np
import pytest

import vec_ref as V

DOT_LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 262144, 262145, 1000003]


@pytest.mark.parametrize("case", ["uniform", "same", "cancel"])
def test_dot_emulation_within_bound(case):
    for n in DOT_LENGTHS:
        x, y = V.dot_inputs(case, n)
        ref, sum_abs = V.dot_ref(x, y)
        got = V.dot_emulate(x, y)
        assert abs(got - ref) <= V.dot_bound(n, sum_abs), (case, n, got, ref)
        if case == "cancel" and n % 2 == 0:
            assert ref == 0.0 and sum_abs > 0.3 * n  # the relative form of the bound would be 0 here


def test_dot_emulation_is_the_plain_sum_where_it_is_exact():
    """small integers: every order of summation is exact, so the emulation's
    indexing (padding, lanes, blocks, partials) is checked exactly"""
    for n in (1, 255, 257, 262145, 1000003):
        x = np.arange(n) % 7 - 3.0
        y = np.arange(n) % 5 - 2.0
        assert V.dot_emulate(x, y) == float(np.sum(x.astype(np.int64) * y.astype(np.int64)))
    assert V.dot_emulate(np.zeros(0), np.zeros(0)) == 0.0


def test_dot_launch_shape():
    assert [V.dot_n_blocks(n) for n in (0, 1, 256, 257, 262144, 262145, 1000003)] == [1, 1, 1, 2, 1024, 1024, 1024]
    # the wrap lengths of test_gpu_vec.py: 262144 fills every lane once, the others take a second / fourth trip
    assert [-(-n // (256 * V.dot_n_blocks(n))) for n in (262144, 262145, 1000003)] == [1, 2, 4]


def _round_to_double(q):
    """a Fraction rounded to the nearest float64 (ties to even): float(Fraction) is correctly rounded"""
    return float(q)


@pytest.mark.parametrize("a,b", [(0.37, -1.25), (-0.6, 1.0), (0.5, 0.5), (0.0, 2.0), (1.0, 0.0)])
def test_axpby_reference_and_bound_vs_exact_rationals(a, b):
    rng = np.random.default_rng(5)
    x, y = rng.uniform(-1, 1, 200), rng.uniform(-1, 1, 200)
    y[:20] = -x[:20] * (a / b if b else 1.0)  # near-cancelling entries
    ref, mag = V.axpby_ref(a, x, b, y)
    eps_ld = float(np.finfo(np.longdouble).eps)
    for i in range(x.size):
        ax, by = Fraction(a) * Fraction(float(x[i])), Fraction(b) * Fraction(float(y[i]))
        exact = ax + by
        m = abs(ax) + abs(by)
        # three longdouble roundings (two products, one sum), each relative eps / 2 of a term bounded by m
        assert abs(Fraction(float(ref[i])) + Fraction(float(ref[i] - np.longdouble(float(ref[i])))) - exact) \
            <= 2 * Fraction(eps_ld) * m
        assert abs(Fraction(float(mag[i])) - m) <= Fraction(4 * V.U) * m
        # the kernel's arithmetic, exactly: t = round(b y), result = round(a x + t)
        t = Fraction(_round_to_double(by))
        got = Fraction(_round_to_double(ax + t))
        assert abs(got - exact) <= Fraction(2 * V.U) * m
        # and within the bound of the device test against the longdouble reference
        assert abs(np.longdouble(float(got)) - ref[i]) <= 2 * np.longdouble(V.U) * mag[i]

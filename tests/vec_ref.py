"""TEST INFRASTRUCTURE ONLY: plain references, inputs and error bounds of the
vector entry points (gdm_vec_axpby, gdm_vec_dot), shared by
tests/test_gpu_vec.py (device) and tests/test_vec_ref_cpu.py (which checks
these references and bounds themselves, without a GPU).

axpby: a x + b y evaluated in np.longdouble and rounded once.
dot:   math.fsum of the float64 products x_i * y_i.
"""
import math

import numpy as np

U = 2.0 ** -53  # unit roundoff of binary64
N_DOT_PARTIAL = 1024  # gdm_op::n_dot_partial (csrc/gdm_capi_internal.h): the cap of gdm_vec_dot's partial blocks
DOT_BLOCK = 256  # lanes per block of dot_partial_kernel / dot_final_kernel (csrc/gdm_vec.hip)


def axpby_ref(a, x, b, y):
    """(a x + b y, |a x| + |b y|), both in longdouble: the reference and the
    magnitude the bound of test_gpu_vec.py scales with"""
    ax = np.longdouble(a) * x.astype(np.longdouble)
    by = np.longdouble(b) * y.astype(np.longdouble)
    return ax + by, np.abs(ax) + np.abs(by)


def dot_inputs(case, n, seed=0):
    """(x, y) of one dot case; "same" returns the same array twice"""
    rng = np.random.default_rng(1000 + seed + n)
    x = rng.uniform(-1.0, 1.0, n)
    if case == "uniform":
        return x, rng.uniform(-1.0, 1.0, n)
    if case == "same":
        return x, x
    if case == "cancel":
        # pairs (v, -v) against a constant y: the terms cancel (an odd n leaves one term), so the sum is
        # ~ 0 while sum |x_i y_i| ~ n / 2 -- only a bound on the absolute error can hold here
        v = rng.uniform(0.5, 1.0, (n + 1) // 2)
        x = np.repeat(v, 2)[:n] * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        return x, np.full(n, 0.7)
    raise ValueError(case)


def dot_n_blocks(n):
    """gdm_vec_dot's launch: min(n_dot_partial, ceil(n / 256)) blocks, at least one"""
    return min(N_DOT_PARTIAL, max(1, -(-n // DOT_BLOCK)))


def dot_ref(x, y):
    """(fsum of the float64 products, sum |x_i y_i|)"""
    prod = x * y
    return math.fsum(prod), math.fsum(np.abs(prod))


def dot_bound(n, sum_abs):
    """|device - dot_ref| <= (ceil(n / (256 np)) + 32) 2^-53 sum |x_i y_i|, np = dot_n_blocks(n).

    Derivation (csrc/gdm_vec.hip).  dot_partial_kernel: lane l of block b
    folds its m = ceil(n / (256 np)) entries i = 256 b + l + 256 np j into
    s = fma(x_i, y_i, s): m roundings on the path of an entry (the product is
    not rounded).  wave_sum adds 6 levels, the four wave sums 3 more additions.
    dot_final_kernel: a lane adds at most ceil(1024 / 256) = 4 partials, then
    again 6 + 3.  An entry's product thus passes at most k = m + 22 rounded
    operations, so the computed sum is sum_i x_i y_i (1 + t_i) with |t_i| <=
    (1 + u)^k - 1 <= k u / (1 - k u) (Higham, Accuracy and Stability, Lemma
    3.1), u = 2^-53.  The reference rounds each product (u sum |x_i y_i|) and
    its exact sum once more (u |sum| <= u sum |x_i y_i|).  Together (k + 2) u /
    (1 - k u) <= (m + 32) u whenever k u <= 8 / (m + 32), i.e. for m below 2e8."""
    m = -(-n // (DOT_BLOCK * dot_n_blocks(n))) if n else 0
    return (m + 32) * U * sum_abs


def _fma(a, b, c):
    """fma(a, b, c) on float64 arrays through longdouble where it has a 64-bit
    significand (x86): the product keeps 11 more bits than float64, the sum is
    rounded to float64 at the end.  Elsewhere the product is rounded to
    float64 -- one more rounding per entry than the kernel, which the bound's
    slack of 8 covers."""
    if np.finfo(np.longdouble).nmant >= 63:
        return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(np.float64)
    return a * b + c


def _block_sum(s):
    """s: (blocks, 256) lane values -> (blocks,): wave_sum (lane l += lane l + o
    for o = 32 .. 1, lane 0 holds the wave's sum) and red[0] + red[1] + red[2] + red[3]"""
    w = s.reshape(s.shape[0], 4, 64).copy()
    o = 32
    while o > 0:
        w[:, :, :o] = w[:, :, :o] + w[:, :, o:2 * o]
        o //= 2
    r = w[:, :, 0]
    return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def dot_emulate(x, y):
    """gdm_vec_dot's summation order in numpy float64: per-lane fma chains over
    the grid-stride loop, wave and block trees, then dot_final_kernel's
    per-lane chains over the partials and the same trees"""
    n = x.size
    if n == 0:
        return 0.0
    nb = dot_n_blocks(n)
    lanes = nb * DOT_BLOCK
    m = -(-n // lanes)
    xp, yp = np.zeros(m * lanes), np.zeros(m * lanes)  # a lane past the end keeps s: fma(0, 0, s) = s
    xp[:n], yp[:n] = x, y
    xp, yp = xp.reshape(m, lanes), yp.reshape(m, lanes)
    s = np.zeros(lanes)
    for j in range(m):
        s = _fma(xp[j], yp[j], s)
    partial = _block_sum(s.reshape(nb, DOT_BLOCK))
    mf = -(-nb // DOT_BLOCK)
    pp = np.zeros(mf * DOT_BLOCK)
    pp[:nb] = partial
    pp = pp.reshape(mf, DOT_BLOCK)
    t = np.zeros(DOT_BLOCK)
    for j in range(mf):
        t = t + pp[j]
    return float(_block_sum(t.reshape(1, DOT_BLOCK))[0])

"""The near-hard probe's predicate (QEC_OPT_NEAR_PROBE; qec_near_probe) without a
GPU, against numpy float32: every pair of folds (t0, t1) it accepts has q = t1 / (t0 + t1) -- one float32 sum,
one correctly rounded float32 quotient, what the kernels' divisions return -- with bits(fma(-q, q, q)) <= T of
qec_near_hard_threshold, and its side is q >= 0.5; for every eps0 = 2^-8 .. 2^-20, on pairs around the boundary
ratio from the subnormals up to the 2^32-scaled folds, on zeros, NaNs, infinities and negative values (all
rejected) and on a million seeded random pairs."""
import ctypes
import functools

import numpy as np
import pytest

import qec_ldpc_amd as q

KS = list(range(8, 21))
TOP = 0x7F000000  # every accepted pattern lies below it (no NaN, no infinity, below 2^127)


def p_prime(p):
    return np.float32(2.0) / np.float32(3.0) * np.float32(p)


@functools.lru_cache(maxsize=None)
def compare_values():
    """T per k (eps0 = 2^-k) from qec_near_hard_threshold, over a grid of launches (p, R, L); a k no launch of the
    grid lands on takes the documented form, the bit pattern one below the float eps0 (1 - eps0)."""
    T = {}
    for R in (3, 4, 5):
        for L in (6, 10):
            for p in np.logspace(-5, np.log10(0.3), 400):
                eps, t = q.near_hard_threshold(p_prime(p), R, L)
                if eps:
                    k = int(round(-np.log2(eps)))
                    assert T.setdefault(k, t) == t
    for k in KS:
        e = 2.0 ** -k
        form = int(np.array([e * (1.0 - e)], np.float32).view(np.uint32)[0]) - 1
        assert T.setdefault(k, form) == form, k
    return T


def probe(b0, b1, k):
    """qec_near_probe on arrays of bit patterns -> (accepted, side)."""
    fn = q.lib().qec_near_probe
    with np.errstate(invalid="ignore"):  # signalling NaN patterns among the inputs
        t0 = b0.astype(np.uint32).view(np.float32).astype(np.float64).tolist()
        t1 = b1.astype(np.uint32).view(np.float32).astype(np.float64).tolist()
    side = ctypes.c_int(0)
    ref = ctypes.byref(side)
    eps = 2.0 ** -k
    ok, sd = np.empty(len(t0), bool), np.empty(len(t0), np.int8)
    for i, (a, b) in enumerate(zip(t0, t1)):
        ok[i] = fn(a, b, eps, ref)
        sd[i] = side.value
    return ok, sd


def check(b0, b1, k):
    """The issue's two properties on every accepted pair, and the predicate's own statement on all."""
    b0, b1 = np.asarray(b0, np.uint32), np.asarray(b1, np.uint32)
    ok, side = probe(b0, b1, k)
    K = (k + 1) << 23
    d = b1.astype(np.int64) - b0.astype(np.int64)
    stated = (np.maximum(b0, b1) < TOP) & (np.abs(d) >= K)
    assert np.array_equal(ok, stated), k
    t0, t1 = b0[ok].view(np.float32), b1[ok].view(np.float32)
    with np.errstate(all="ignore"):
        qq = t1 / (t0 + t1)  # float32 sum, float32 quotient (subnormals kept)
    f = (qq.astype(np.float64) - qq.astype(np.float64) ** 2).astype(np.float32)  # fma(-q, q, q)
    assert (f.view(np.uint32) <= np.uint32(compare_values()[k])).all(), k
    assert np.array_equal(qq >= np.float32(0.5), side[ok] == 1), k
    assert np.array_equal(side[ok] == 1, t1 > t0), k
    eps = np.float32(2.0 ** -k)
    assert ((qq <= eps) | (qq >= np.float32(1) - eps)).all(), k
    return ok, side


@pytest.mark.parametrize("k", KS)
def test_boundary_pairs(k):
    """Both patterns within +-4 of the boundary |b1 - b0| = K, the smaller fold from zero and the subnormals up to
    where the larger reaches the 2^32-scaled folds (2^33) and the top of the accepted range."""
    K = (k + 1) << 23
    lows = [0, 1, 2, 5, 1 << 22, (1 << 23) - 1]
    for e in list(range(1, 30, 3)) + list(range(30, 254 - (k + 1), 7)) + [127 - 32, 127 - 25 * 4, 127 + 33 - (k + 1),
                                                                         253 - (k + 1), 254 - (k + 1)]:
        if 1 <= e and e + k + 1 <= 254:
            lows += [(e << 23) + m for m in (0, 1, 0x2AAAAA, 0x400000, 0x7FFFFB, 0x7FFFFF)]
    lo = np.array(lows, np.int64)
    dl, dh = np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), indexing="ij")
    b_lo = (lo[:, None, None] + dl[None]).ravel()
    b_hi = (lo[:, None, None] + K + dh[None]).ravel()
    keep = (b_lo >= 0) & (b_hi < (1 << 31))
    b_lo, b_hi = b_lo[keep], b_hi[keep]
    ok0, s0 = check(b_hi, b_lo, k)  # t0 the larger: side 0
    ok1, s1 = check(b_lo, b_hi, k)  # t1 the larger: side 1
    assert ok0.any() and ok1.any() and (~ok0).any() and (~ok1).any()
    assert (s0[ok0] == 0).all() and (s1[ok1] == 1).all()
    # normal folds: the integer test is the ratio test max >= (2 / eps0) min, exactly
    n = (b_lo >= (1 << 23)) & (b_hi < TOP)
    ratio = b_hi[n].astype(np.uint32).view(np.float32).astype(np.float64) >= \
        2.0 ** (k + 1) * b_lo[n].astype(np.uint32).view(np.float32).astype(np.float64)
    assert np.array_equal(ok1[n], ratio)


def test_rejects_zeros_nans_infinities_negatives():
    f = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])
    good = [f(1.0), f(0.3), f(2.0 ** 32), f(2.0 ** -100), f(1e-40), 1]
    bad = [f(np.nan), 0x7FC00001, 0xFFC00000, 0x7F800001, f(np.inf), f(-np.inf), f(-0.0), f(-1.0), f(-1e-30), 0x80000001,
           f(2.0 ** 127), 0x7F7FFFFF]
    for k in KS:
        pairs = [(0, 0)] + [(b, g) for b in bad for g in good + [0]] + [(g, b) for b in bad for g in good + [0]] + \
                [(b, c) for b in bad for c in bad]
        b0, b1 = np.array(pairs, np.int64).T
        ok, _ = check(b0, b1, k)
        assert not ok.any(), k
        # a zero fold beside a positive one is a message of exactly 0 or 1: accepted from 2^(k - 125) on
        z = np.array([f(1.0), f(2.0 ** -60), (k + 1) << 23], np.int64)
        ok, side = check(np.concatenate([z, 0 * z]), np.concatenate([0 * z, z]), k)
        assert ok.all() and (side == np.array([0, 0, 0, 1, 1, 1])).all()
        ok, _ = check(np.array([((k + 1) << 23) - 1]), np.array([0]), k)
        assert not ok.any()
    for eps in (0.0, 2.0 ** -7, 2.0 ** -21, 3e-3, -2.0 ** -9, np.nan, np.inf):
        assert q.near_probe(1.0, 0.0, eps) == (False, 0) and q.near_probe(0.0, 1.0, eps)[0] is False


def test_random_pairs():
    """Some 10^6 seeded pairs over all eps0: raw 32-bit patterns (NaNs, negatives, infinities among them), and
    non-negative pairs whose exponent gap straddles the boundary."""
    rng = np.random.default_rng(20251)
    per = 1_000_000 // len(KS) // 2
    sides = np.zeros(2, np.int64)
    for k in KS:
        K = (k + 1) << 23
        raw0 = rng.integers(0, 1 << 32, per, dtype=np.int64)
        raw1 = rng.integers(0, 1 << 32, per, dtype=np.int64)
        lo = rng.integers(0, TOP - K - (4 << 23), per, dtype=np.int64)
        hi = np.minimum(lo + K + rng.integers(-(3 << 23), 4 << 23, per, dtype=np.int64), (1 << 31) - 1)
        hi = np.maximum(hi, 0)
        swap = rng.integers(0, 2, per).astype(bool)
        b0 = np.concatenate([raw0, np.where(swap, lo, hi)])
        b1 = np.concatenate([raw1, np.where(swap, hi, lo)])
        ok, side = check(b0, b1, k)
        sides += np.bincount(side[ok], minlength=2)
    assert (sides > 10_000).all(), sides  # it accepts, on both sides


def test_option_round_trip():
    from qec_ldpc_amd.codes import P61, code_path
    dec = q.DecoderCPU(q.Quantum_LDPC_Code.createFromFile(code_path(P61)))
    assert q.OPTIONS["near_probe"] == 25
    assert dec.get_option("near_probe") == 1
    dec.set_option("near_probe", 0)
    assert dec.get_option("near_probe") == 0
    dec.set_option("near_probe", 7)
    assert dec.get_option("near_probe") == 1

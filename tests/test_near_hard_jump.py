"""The near-hard jump (QEC_OPT_NEAR_HARD_JUMP) without a GPU: the
threshold function both engines take their eps0 and compare value T from, and the CPU engine with the
jump on and off against the oracle -- decisions, flags and iteration counts under the fixed and the
reference stop."""
import functools
import math

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import P7, P61, code_path
from qec_ldpc_amd.synthetic import depolarizing_errors

P_GRID = [1e-4, 3e-4, 1e-3, 2e-3, 5e-3, 0.01, 0.02, 0.03, 0.05, 0.075, 0.1, 0.15, 0.2, 0.25, 0.3]


def p_prime(p):
    """p' as the decoders form it: the float (2/3) p."""
    return np.float32(2.0) / np.float32(3.0) * np.float32(p)


def bound(pp, R, L, eps):
    """2 ((1 - p') / p') (delta / (1 - delta))^(R - 1) with delta = (L - 1) eps + 2^-20, in double."""
    pp = float(pp)
    d = (L - 1) * eps + 2.0 ** -20
    return 2.0 * (1.0 - pp) / pp * (d / (1.0 - d)) ** (R - 1)


@pytest.mark.parametrize("R", [3, 4, 5])
@pytest.mark.parametrize("L", [6, 10])
def test_threshold_properties(R, L):
    fired = 0
    for p in P_GRID:
        pp = p_prime(p)
        eps, T = q.near_hard_threshold(pp, R, L)
        if eps == 0.0:
            assert T == 0
            # no admissible power of two satisfies the inequality (a relative 1e-9 apart from the boundary)
            for k in range(8, 21):
                assert bound(pp, R, L, 2.0 ** -k) > 2.0 ** -k * (1 - 1e-9), (p, k)
            continue
        fired += 1
        k = -math.log2(eps)
        assert k == int(k) and 8 <= k <= 20, (p, eps)
        assert bound(pp, R, L, eps) <= eps, (p, eps)
        for k2 in range(8, int(k)):  # the largest such power of two
            assert bound(pp, R, L, 2.0 ** -k2) > 2.0 ** -k2 * (1 - 1e-9), (p, k2)
        t = float(np.array([T], np.uint32).view(np.float32)[0])
        assert 0.0 < t < eps * (1.0 - eps)
        # ... and only just: the next float up is eps (1 - eps) itself
        assert float(np.array([T + 1], np.uint32).view(np.float32)[0]) == eps * (1.0 - eps)
    assert fired >= 3
    for pp in (0.500001, 0.6, 0.75, 1.0, 1.5, 0.0, -0.1, float("nan")):
        assert q.near_hard_threshold(pp, R, L) == (0.0, 0)


def test_threshold_of_the_shipped_codes():
    """The thresholds DESIGN.md quotes for the headline point and P7's configs[1]."""
    assert q.near_hard_threshold(p_prime(0.01), 4, 10)[0] == 2.0 ** -9   # P61 X
    assert q.near_hard_threshold(p_prime(0.01), 5, 10)[0] == 2.0 ** -8   # P61 Z
    assert q.near_hard_threshold(p_prime(0.02), 3, 6)[0] == 2.0 ** -12   # P7, both sectors


def test_compare_value_separates(R=4, L=10):
    """bits(fma(-q, q, q)) <= T exactly excludes the floats of (eps0, 1 - eps0) around both ends."""
    eps, T = q.near_hard_threshold(p_prime(0.01), R, L)
    e32 = np.float32(eps)
    qs = np.array([0.0, np.nextafter(e32, np.float32(0)), e32, np.nextafter(e32, np.float32(1)), 0.25, 0.5, 0.75,
                   np.nextafter(np.float32(1) - e32, np.float32(0)), np.float32(1) - e32,
                   np.nextafter(np.float32(1) - e32, np.float32(1)), np.nextafter(np.float32(1), np.float32(0)), 1.0,
                   np.nan], np.float32)
    # fma(-q, q, q) = RN(q - q q): exact in double for float q, then one rounding
    f = (qs.astype(np.float64) - qs.astype(np.float64) ** 2).astype(np.float32)
    passes = f.view(np.uint32) <= np.uint32(T)
    for x, ok in zip(qs, passes):
        if ok:
            assert x <= e32 or x >= np.float32(1) - e32, x
        if not np.isnan(x) and (x < e32 or x > np.float32(1) - e32):
            assert ok, x  # strictly inside the eps0 bands passes (the ends themselves need not)


# ---- CPU engine: jump on = jump off = oracle ----------------------------------------------------------

KEYS = {"P7": P7, "P61": P61}


@functools.lru_cache(maxsize=None)
def setup(key):
    path = code_path(KEYS[key])
    code = q.Quantum_LDPC_Code.createFromFile(path)
    return code, q.DecoderCPU(code), OracleCode(path)


@functools.lru_cache(maxsize=None)
def syndromes(key, p):
    """256 depolarising syndromes, an all-zero one and a single-bit one."""
    code = setup(key)[0]
    x, z = depolarizing_errors(code.n, 20251, 256, p)
    sX = np.concatenate([code.syndrome(0, x), np.zeros((2, code.numEqsX), np.uint8)])
    sZ = np.concatenate([code.syndrome(1, z), np.zeros((2, code.numEqsZ), np.uint8)])
    sX[-1, 5] = 1
    sZ[-1, code.numEqsZ - 1] = 1
    return sX, sZ


@pytest.mark.parametrize("key", ["P7", "P61"])
@pytest.mark.parametrize("p", [0.001, 0.01, 0.05, 0.1])
@pytest.mark.parametrize("stop", ["fixed", "ref"])
def test_cpu_engine_jump_on_off_oracle(key, p, stop):
    code, dec, orc = setup(key)
    sX, sZ = syndromes(key, p)
    assert dec.get_option("near_hard") == 1 and dec.get_option("hard_paths") == 1
    for N in (2, 3, 4, 11, 12, 50):
        o = orc.decode_batch(sX, sZ, p, N, stop)
        on = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True)
        dec.set_option("near_hard", 0)
        try:
            off = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True)
        finally:
            dec.set_option("near_hard", 1)
        for name, a, b, c in zip(("eX", "eZ", "flags", "iters"), on[:4], off[:4], o[:4]):
            assert np.array_equal(a, c), (name, N, "jump on vs oracle")
            assert np.array_equal(b, c), (name, N, "jump off vs oracle")
        rec, its = dec.decode_batch_packed(sX, sZ, p, N, stop, want_iters=True)
        from qec_ldpc_amd.gather import pack_records
        assert np.array_equal(rec, pack_records(o[0], o[1], o[2])) and np.array_equal(its, o[3]), N


@pytest.mark.parametrize("key", ["P7", "P61"])
@pytest.mark.parametrize("stop", ["fixed", "ref"])
def test_cpu_engine_final_messages_keep_full_arithmetic(key, stop):
    """A call that requests the final messages never jumps: they equal the oracle's bit for bit."""
    code, dec, orc = setup(key)
    sX, sZ = syndromes(key, 0.01)
    sX, sZ = sX[-40:], sZ[-40:]
    for N in (4, 12):
        g = dec.decode_batch(sX, sZ, 0.01, N, stop, want_iters=True, want_q=True)
        o = orc.decode_batch(sX, sZ, 0.01, N, stop, want_q=True)
        for name, a, b in zip(("eX", "eZ", "flags", "iters"), g[:4], o[:4]):
            assert np.array_equal(a, b), (name, N)
        assert np.array_equal(g[4].view(np.uint32), o[4].view(np.uint32)), N


def test_option_round_trip():
    dec = setup("P7")[1]
    assert q.OPTIONS["near_hard"] == 15
    dec.set_option("near_hard", 0)
    assert dec.get_option("near_hard") == 0
    dec.set_option("near_hard", 7)
    assert dec.get_option("near_hard") == 1

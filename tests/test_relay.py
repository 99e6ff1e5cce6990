"""Relay-BP, set_relay(gammaX, gammaZ, solutions) under set_option("bp_method", 1): DESIGN.md section 2, "The relay
form", restated in numpy on the helpers of tests/test_minsum.py (float32 operations in the stated order, vectorised
over the batch with a per-row leg index) and held against the CPU engine; the anchors (one leg with gamma = 0 is plain
min-sum; a row that leg 0 solves; failure under L legs implies failure under leg 0); coverage of the cases a relay
has; the options and their refusals; the OSD stage behind the relay; the CLI; and the restated choice among the 36
RELAY kernels of bp_sparse.hip over the case table that tests/test_gpu_relay.py runs on the device.  The refusal of a
wave-circulant handle needs a device and is in tests/test_gpu_relay.py.

Every comparison is bit for bit (q_final as uint32 patterns); there is no tolerance, and every value is finite, which
is asserted.  The channel LLRs and, under priors, the integer weights are the library's.

Tables: L = 4 legs of q.relay_gammas (seed 1 for sector X, 2 for Z), cap 20 per leg, scale 160, decode p = 0.05
(test_minsum.MS_P), S = 1 and S = 3, on the 51 rows of test_sparse_shapes.inputs.
"""
import ctypes

import numpy as np
import pytest

import qec_ldpc_amd as q
from test_general_code import NS, STOPS, assert_same_decode, code_matrices, same_floats
from test_minsum import (CAP, F32, INSIDE, LLR_MAX, MS_P, MS_P_REF, PRIOR_NS, SMALL, U32, library_llr, minsum_cpu, osd_case,
                         routes, yard)
from test_priors import VECTORS, prior_vectors
from test_sparse_shapes import CASES, KERNELS, LDS_CASES, SHAPES, code_of, inputs, matrices, plan_of

LEGS = 4
SOLUTIONS = (1, 3)


# ---- the yardstick: "The relay form" of DESIGN.md section 2 in numpy ---------------------------------------------------
def relay_sector(H, s, llr, gam, S, wts, alpha_k, N, stop, D):
    """One sector of a batch; every row carries its own leg index and its own iteration count within the leg.
    llr: the channel LLR of every variable; gam [L, n] float32; wts [n] the integer weights.
    -> (e [B, n], syndrome failed [B], convergence failed [B], iterations [B], q [B, m, D],
        info = legs executed [B], leg of the first solution [B] or -1, leg of the winner [B] or -1)."""
    m, n = H.shape
    B = s.shape[0]
    L = gam.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]                                  # N(c), ascending
    edges = [[(int(c), int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]  # M(v)
    real = np.zeros((m, D), dtype=bool)
    for c in range(m):
        real[c, :len(nbr[c])] = True
    lam = np.asarray(llr, dtype=F32)
    gam = np.asarray(gam, dtype=F32)
    alpha = F32(alpha_k) / F32(256.0)
    connected = np.array([len(edges[v]) > 0 for v in range(n)])
    M0 = np.zeros((m, D), dtype=F32)                                               # the slots at the start of a leg
    for c in range(m):
        M0[c, :len(nbr[c])] = lam[nbr[c]]
    M = np.broadcast_to(M0, (B, m, D)).copy()
    mem = np.broadcast_to(lam, (B, n)).copy()                                      # leg 0: M_v = lambda_v
    d = np.broadcast_to(((lam < F32(0.0)) & connected).astype(np.uint8), (B, n)).copy()  # N = 0
    t = (s != 0).astype(U32)
    w32 = np.asarray(wts).astype(np.uint64)
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)
    leg = np.zeros(B, dtype=np.int64)
    k = np.zeros(B, dtype=np.int64)                                                # iterations executed in the leg
    sols = np.zeros(B, dtype=np.int64)
    wbest = np.zeros(B, dtype=np.uint64)
    best = np.zeros((B, n), dtype=np.uint8)
    first_leg = np.full(B, -1, dtype=np.int64)
    win_leg = np.full(B, -1, dtype=np.int64)

    def syndrome_fails(e):
        bad = np.zeros(B, dtype=bool)
        for c in range(m):
            bad |= (e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) != s[:, c]      # the entry's exact value
        return bad

    def inside_any(M):
        return ((np.abs(M) < INSIDE) & real[None]).any(axis=(1, 2))

    def check_update(M):
        R = np.zeros_like(M)
        for c in range(m):
            dc = len(nbr[c])
            bits = np.ascontiguousarray(M[:, c, :dc]).view(U32)
            a, g = bits & U32(0x7FFFFFFF), bits >> U32(31)
            others = ~np.eye(dc, dtype=bool)[None]
            mag = np.where(others, a[:, None, :], U32(0xFFFFFFFF)).min(axis=2)
            mag = np.minimum(mag, CAP)
            sign = np.bitwise_xor.reduce(np.where(others, g[:, None, :], U32(0)), axis=2) ^ t[:, c, None]
            out = (alpha * np.ascontiguousarray(mag).view(F32)).astype(F32)
            R[:, c, :dc] = (out.view(U32) | (sign << U32(31))).view(F32)
        return R

    def variable_update(R, last, g):
        """last [B]: the row is in iteration N - 1 of its leg; g [B, n]: the row's leg of the table."""
        new = np.zeros_like(R)
        dec = np.zeros((B, n), dtype=np.uint8)
        posts = mem.copy()
        for v in range(n):
            if not connected[v]:
                continue                                                           # decides 0, no memory, no weight
            t0 = F32(1.0) - g[:, v]
            t1 = t0 * lam[v]
            t2 = g[:, v] * mem[:, v]
            b = t1 + t2
            b = b + F32(0.0)                                                       # -0.0f becomes +0.0f
            rs = [R[:, c, kk] for c, kk in edges[v]]
            post = b
            for r in rs:
                post = post + r
            dec[:, v] = post < F32(0.0)
            posts[:, v] = post
            for j, (c, kk) in enumerate(edges[v]):
                x = b
                for i, r in enumerate(rs):
                    if i != j:
                        x = x + r
                new[:, c, kk] = np.where(last, post, x)
        return new, dec, posts

    with np.errstate(all="ignore"):
        while active.any():
            if N > 0:
                iters += active
                new, dec, posts = variable_update(check_update(M), k == N - 1, gam[leg])
                M = np.where(active[:, None, None], new, M)
                d = np.where(active[:, None], dec, d)
                mem = np.where(active[:, None], posts, mem)
                k += active
            end = active & (k == N)
            if N > 0 and stop == "ref":
                end |= active & ((k - 1) % 10 == 0) & ~inside_any(M)
            elif N > 0 and stop == "syndrome":
                end |= active & ~syndrome_fails(d)
            solved = end & ~syndrome_fails(d)
            W = (d.astype(np.uint64) * w32[None]).sum(axis=1) & np.uint64(0xFFFFFFFF)   # an unsigned 32-bit sum
            keep = solved & ((sols == 0) | (W < wbest))                            # ties keep the earlier leg
            best[keep] = d[keep]
            wbest[keep] = W[keep]
            win_leg[keep] = leg[keep]
            first_leg[solved & (sols == 0)] = leg[solved & (sols == 0)]
            sols += solved
            done = end & ((sols == S) | (leg == L - 1) | (N == 0))
            nxt = end & ~done
            active &= ~done
            leg[nxt] += 1
            k[nxt] = 0
            M[nxt] = M0
    e = np.where((sols > 0)[:, None], best, d)
    return e, sols == 0, inside_any(M), iters, M, (leg + 1, first_leg, win_leg)


def relay_yardstick(HX, HZ, sX, sZ, piX, piZ, gX, gZ, S, wX, wZ, alpha_k, N, stop):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D], (info X, info Z)); piX / piZ: n priors each, or a scalar
    p for both; wX / wZ: None (w_v = 1) or the integer weights.  The channel LLRs are the library's."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    n = HX.shape[1]
    if np.ndim(piX) == 0:
        lX = lZ = np.full(n, q.minsum_llr(F32(2.0) / F32(3.0) * F32(piX)), dtype=F32)
    else:
        lX, lZ = library_llr(piX), library_llr(piZ)
    one = np.ones(n, dtype=np.int32)
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fx, cx, ix, qx, infoX = relay_sector(HX, sX, lX, gX, S, one if wX is None else wX, alpha_k, N, stop, D)
    eZ, fz, cz, iz, qz, infoZ = relay_sector(HZ, sZ, lZ, gZ, S, one if wZ is None else wZ, alpha_k, N, stop, D)
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return (eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32),
            (infoX, infoZ))


def tables(n, legs=LEGS):
    """The two tables of the tests: the defaults of q.relay_gammas, seed 1 for sector X and 2 for Z."""
    return q.relay_gammas(n, legs, seed=1), q.relay_gammas(n, legs, seed=2)


_ryard = {}


def ryard(name, kind, stop, N, S, p=None, legs=LEGS):
    """The yardstick's relay decode of inputs(name), computed once and shared with tests/test_gpu_relay.py.
    kind: "scalar" (p, default MS_P[name]) or one of test_priors.VECTORS."""
    if kind == "scalar" and p is None:
        p = MS_P[name]
    key = (name, kind, stop, N, S, p, legs)
    if key not in _ryard:
        HX, HZ = matrices(name)
        n = HX.shape[1]
        gX, gZ = tables(n, legs)
        if kind == "scalar":
            pri, w = (p, p), (None, None)
        else:
            pri = prior_vectors(n, kind)
            dec = q.DecoderCPU(code_of(name, "general"))
            dec.set_priors(*pri)
            w = dec.osd_weights()
        _ryard[key] = relay_yardstick(HX, HZ, *inputs(name), pri[0], pri[1], gX, gZ, S, w[0], w[1], 160, N, stop)
    return _ryard[key]


def relay_cpu(code, S=1, priors=None, legs=LEGS, scale=160):
    dec = minsum_cpu(code, scale, priors)
    dec.set_relay(*tables(code.n, legs), solutions=S)
    return dec


# ---- the CPU engine against the yardstick -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("S", SOLUTIONS)
def test_cpu_engine_matches_the_yardstick(name, S):
    """Scalar p: every stop rule, every N, both routes of a regular code."""
    sX, sZ = inputs(name)
    decs = [relay_cpu(code_of(name, r), S) for r in routes(name)]
    for stop in STOPS:
        for N in NS:
            for p in (MS_P[name],) + ((MS_P_REF,) if stop == "ref" and N == 20 else ()):
                want = ryard(name, "scalar", stop, N, S, p)
                assert np.isfinite(want[4]).all()
                for r, dec in zip(routes(name), decs):
                    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                    assert_same_decode(got, want, "%s %s %s S=%d p=%g N=%d" % (name, r, stop, S, p, N))
                    assert dec.last_path() == {"minsum", "relay"}


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("kind", VECTORS)
def test_cpu_engine_matches_the_yardstick_under_priors(name, kind):
    """The prior vectors of test_priors; the special one holds 0, 1/2 and 1: a channel LLR of +0.0f (the -0.0f rule)
    and the largest and smallest integer weights."""
    HX, HZ = matrices(name)
    sX, sZ = inputs(name)
    pri = prior_vectors(HX.shape[1], kind)
    for S in SOLUTIONS:
        decs = [relay_cpu(code_of(name, r), S, pri) for r in routes(name)]
        for stop in STOPS:
            for N in PRIOR_NS:
                want = ryard(name, kind, stop, N, S)
                assert np.isfinite(want[4]).all()
                for r, dec in zip(routes(name), decs):
                    got = dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)  # p is not used
                    assert_same_decode(got, want, "%s %s %s %s S=%d N=%d" % (name, r, kind, stop, S, N))
    assert not same_floats(ryard(name, "scalar", "fixed", 11, 1)[4], ryard(name, kind, "fixed", 11, 1)[4])


def test_finiteness_and_the_bound():
    """|M| grows by at most 2 * 2^30 + (dv + 1) * 2^20 per iteration (|b| <= 2 * 2^30 + |M|, dv check messages of at
    most 2^20 each), so nothing overflows at any legal L * N; on the tables' runs every value is finite and within it."""
    for name in ("dense32", "tall", "hgp_ham"):
        dv = max(int(H.sum(axis=0).max()) for H in matrices(name))
        for kind in ("scalar", "special"):
            for N in (1, 11):
                qf = ryard(name, kind, "fixed", N, 1)[4]
                assert np.isfinite(qf).all()
                assert np.abs(qf).max() <= float(LLR_MAX) + LEGS * N * (2.0 * 2.0 ** 30 + (dv + 1) * 2.0 ** 20)


# ---- anchors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("hgp_ham", "tall", "r3-3-6-13"))
def test_one_leg_with_gamma_zero_is_plain_minsum(name):
    """L = 1 with every gamma = 0: b = lambda_v exactly, every output bit equals the min-sum call -- on the yardstick
    and on the CPU engine, with S = 1 and S = 3, scalar p and the special priors."""
    HX, HZ = matrices(name)
    n = HX.shape[1]
    sX, sZ = inputs(name)
    zero = np.zeros((1, n), dtype=F32)
    for kind in ("scalar", "special"):
        pri = None if kind == "scalar" else prior_vectors(n, kind)
        for S in SOLUTIONS:
            dec = minsum_cpu(code_of(name, "general"), 160, pri)
            dec.set_relay(zero, zero, solutions=S)
            w = (None, None) if pri is None else dec.osd_weights()
            for stop in STOPS:
                for N in PRIOR_NS:
                    want = yard(name, kind, stop, N)
                    p = MS_P[name]
                    ys = relay_yardstick(HX, HZ, sX, sZ, *((p, p) if pri is None else pri), zero, zero, S, w[0], w[1], 160, N, stop)
                    assert_same_decode(ys, want, "yardstick %s %s %s N=%d S=%d" % (name, kind, stop, N, S))
                    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                    assert_same_decode(got, want, "engine %s %s %s N=%d S=%d" % (name, kind, stop, N, S))
                    assert "relay" in dec.last_path()


@pytest.mark.parametrize("name", ("hgp_ham", "mid", "r3-3-6-13"))
def test_leg_zero_rows_and_failure_implies_leg_zero_failure(name):
    """S = 1: a row that leg 0 solves has the outputs of the L = 1 call with the same leg 0, sector by sector; and
    SYNDROME_FAIL under L legs implies SYNDROME_FAIL under leg 0 alone."""
    HX, HZ = matrices(name)
    n, mX = HX.shape[1], HX.shape[0]
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    for stop in STOPS:
        full = ryard(name, "scalar", stop, 20, 1)
        one = ryard(name, "scalar", stop, 20, 1, legs=1)
        for sec, bit in ((0, q.SYNDROME_FAIL_X), (1, q.SYNDROME_FAIL_Z)):
            solved0 = (one[2] & bit) == 0
            assert solved0.any()
            assert np.array_equal(full[sec][solved0], one[sec][solved0])
            assert np.array_equal(full[3][solved0, sec], one[3][solved0, sec])
            cbit = q.CONVERGENCE_FAIL_X if sec == 0 else q.CONVERGENCE_FAIL_Z
            assert np.array_equal(full[2][solved0] & (bit | cbit), one[2][solved0] & (bit | cbit))
            sl = slice(0, mX * D) if sec == 0 else slice(mX * D, None)
            assert same_floats(full[4][solved0][:, sl], one[4][solved0][:, sl])
            assert not (((full[2] & bit) != 0) & solved0).any()       # failure under L legs => failure under leg 0
            assert ((full[2] & bit) != 0).sum() <= ((one[2] & bit) != 0).sum()


# ---- coverage -----------------------------------------------------------------------------------------------------------
# codes whose 51 rows show no sector that is solved in a leg >= 1 (and so none whose winner is a later solution)
NO_LATE_SOLUTION = ()


def test_coverage():
    """On the yardstick, cap 20: hgp_ham by itself has a sector solved in leg 0, one solved in a leg >= 1, one that no
    leg solves, a row whose two sectors end in different legs, under S = 3 a sector whose winner is not its first
    solution, and under FIXED and under REF a sector that runs more than one leg."""
    name = "hgp_ham"
    (legsX, firstX, _), (legsZ, firstZ, _) = ryard(name, "scalar", "syndrome", 20, 1)[5]
    first = np.concatenate([firstX, firstZ])
    assert (first == 0).any() and (first >= 1).any() and (first == -1).any()
    assert (legsX != legsZ).any()
    later = [((win != first) & (first >= 0)) for _, first, win in ryard(name, "scalar", "syndrome", 20, 3)[5]]
    assert any(x.any() for x in later)  # S = 3: the winner is not the first solution
    for stop, p in (("fixed", None), ("ref", None), ("ref", MS_P_REF)):
        info = ryard(name, "scalar", stop, 20, 1, p)[5]
        assert any((i[0] > 1).any() for i in info), stop
    it = ryard(name, "scalar", "syndrome", 20, 1)[3]
    assert (it > 20).any() and (it == 1).any() and (it == LEGS * 20).any()
    for other in SMALL:
        f = np.concatenate([i[1] for i in ryard(other, "scalar", "syndrome", 20, 1)[5]])
        assert (f >= 1).any() != (other in NO_LATE_SOLUTION), other


def test_the_relay_repairs_what_plain_minsum_leaves():
    """Fewer unsatisfied sectors than min-sum alone on hgp_ham's rows (the count, not a rate)."""
    plain = yard("hgp_ham", "scalar", "syndrome", 20)[2]
    relay = ryard("hgp_ham", "scalar", "syndrome", 20, 1)[2]
    count = lambda f: int(((f & 1) != 0).sum() + ((f & 2) != 0).sum())  # noqa: E731
    assert count(relay) < count(plain)


# ---- the options --------------------------------------------------------------------------------------------------------
def test_option_values_refusals_and_round_trip():
    code = code_of("hgp_ham", "general")
    n = code.n
    dec = minsum_cpu(code)
    L = q.lib()
    assert q.PATH["relay"] == 4096 and L.qec_abi_version() == 4
    assert {"qec_decoder_set_relay", "qec_decoder_get_relay"} <= set(q.EXPORTS)
    assert dec.get_relay() is None
    gX, gZ = tables(n)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    dec.set_relay(gX, gZ, solutions=3)

    def unchanged():
        got = dec.get_relay()
        return got is not None and np.array_equal(got[0].view(U32), gX.view(U32)) and \
            np.array_equal(got[1].view(U32), gZ.view(U32)) and got[2] == 3

    assert unchanged()
    bad = gX.copy()
    for value in (1.5, -1.0000001, np.nan, np.inf):
        bad[2, 5] = value
        with pytest.raises(q.QecError, match=r"gammaX\[2\]\[5\]"):
            dec.set_relay(bad, gZ)
        with pytest.raises(q.QecError, match=r"gammaZ\[2\]\[5\]"):
            dec.set_relay(gX, bad)
        assert L.qec_decoder_set_relay(dec._h, ptr(bad), ptr(gZ), LEGS, 1) == -1  # QEC_ERR_ARG
        assert unchanged()
    for legs, sol in ((0, 1), (-1, 1), (1025, 1), (LEGS, 0), (LEGS, 65), (LEGS, -2)):
        big = np.zeros((max(legs, 1), n), dtype=F32)
        assert L.qec_decoder_set_relay(dec._h, ptr(big), ptr(big), legs, sol) == -1, (legs, sol)
        assert unchanged()
    assert L.qec_decoder_set_relay(dec._h, ptr(gX), None, LEGS, 1) == -1 and unchanged()
    assert L.qec_decoder_set_relay(dec._h, None, None, LEGS, 1) == -1 and unchanged()
    with pytest.raises(q.QecError):
        dec.set_relay(gX, None)
    with pytest.raises(q.QecError, match="shape"):
        dec.set_relay(gX[:, :-1], gZ[:, :-1])
    with pytest.raises(q.QecError, match="same number of legs"):
        dec.set_relay(gX, gZ[:2])
    assert unchanged()
    # legs * n <= 2^22
    H = np.kron(np.eye(17, dtype=np.uint8), np.ones((1, 241), dtype=np.uint8))  # n = 4097, 17 checks of weight 241
    wide = q.DecoderCPU(q.Quantum_LDPC_Code.createFromMatrices(H, H))
    z = np.zeros((1024, 4097), dtype=F32)
    assert L.qec_decoder_set_relay(wide._h, ptr(z), ptr(z), 1024, 1) == -1
    assert L.qec_decoder_set_relay(wide._h, ptr(z), ptr(z), 1023, 1) == 0
    # the counts alone, and the shapes set_relay takes
    legs, sol = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.qec_decoder_get_relay(dec._h, None, None, ctypes.byref(legs), ctypes.byref(sol)) == 0
    assert (legs.value, sol.value) == (LEGS, 3)
    dec.set_relay(gX[1], gZ[1])
    got = dec.get_relay()
    assert got[0].shape == (1, n) and np.array_equal(got[0][0], gX[1]) and got[2] == 1
    dec.set_relay(0.25, -0.5, solutions=2)
    got = dec.get_relay()
    assert (got[0] == F32(0.25)).all() and (got[1] == F32(-0.5)).all() and got[0].shape == (1, n) and got[2] == 2
    dec.set_relay(None, None)
    assert dec.get_relay() is None
    assert L.qec_decoder_get_relay(dec._h, None, None, ctypes.byref(legs), ctypes.byref(sol)) == 0
    assert (legs.value, sol.value) == (0, 0)
    # the existing mutual refusals are untouched by tables
    dec.set_relay(gX, gZ)
    for other in ("correlated", "bp_schedule"):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
            dec.set_option(other, 1)
        assert dec.get_option(other) == 0


def test_relay_gammas():
    g = q.relay_gammas(58, 5)
    assert g.dtype == F32 and g.shape == (5, 58) and (g[0] == F32(0.125)).all()
    want = np.random.default_rng(0).uniform(-0.24, 0.66, (4, 58)).astype(F32)
    assert np.array_equal(g[1:], want) and (g[1:] < 0).any() and (np.abs(g) <= 1).all()
    h = q.relay_gammas(7, 3, gamma0=-0.5, lo=0.0, hi=0.1, seed=9)
    assert (h[0] == F32(-0.5)).all() and (h[1:] >= 0).all() and (h[1:] <= F32(0.1)).all()
    assert q.relay_gammas(7, 1).shape == (1, 7)


def test_clear_then_decode_equals_plain_minsum_and_the_product_rule_ignores_the_tables():
    name = "hgp_ham"
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    dec = relay_cpu(code, 3)
    relayed = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert "relay" in dec.last_path()
    assert_same_decode(relayed, ryard(name, "scalar", "syndrome", 20, 3), "relay")
    dec.set_relay(None, None)
    plain = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert_same_decode(plain, yard(name, "scalar", "syndrome", 20), "cleared")
    assert dec.last_path() == {"minsum"}
    assert not np.array_equal(plain[2], relayed[2])
    # tables set, method 0: the handle without tables, and last_path lacks relay
    dec.set_relay(*tables(code.n))
    dec.set_option("bp_method", 0)
    prod = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert_same_decode(prod, q.DecoderCPU(code).decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True), "method 0")
    assert "relay" not in dec.last_path() and "minsum" not in dec.last_path()
    dec.set_option("bp_method", 1)
    assert_same_decode(dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True),
                       ryard(name, "scalar", "syndrome", 20, 1), "method 1 again")


def test_get_statistics_honours_the_relay():
    code = q.Quantum_LDPC_Code.createFromMatrices(*code_matrices("hgp_ham")).with_logical("degenerate")
    plain, relay = minsum_cpu(code), relay_cpu(code)
    a = plain.GetStatistics(4, 600, 0.05, 20, seed=3)
    b = relay.GetStatistics(4, 600, 0.05, 20, seed=3)
    assert "relay" in relay.last_path() and "relay" not in plain.last_path()
    assert a["numErrorsTested"] == b["numErrorsTested"]
    assert b["syndromeErrorsX"] + b["syndromeErrorsZ"] <= a["syndromeErrorsX"] + a["syndromeErrorsZ"]


# ---- OSD behind the relay -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0, 10])
def test_osd_behind_the_relay(lam):
    """osd = 1: a sector the relay solves keeps the relay's output; a sector that fails under the relay and also under
    plain min-sum gets the same stage output from the handle with tables and from the handle without (the stage's soft
    decode starts from the syndrome alone and ignores the tables); nothing stays failed."""
    code, sX, sZ, p = osd_case("hgp_ham")[:4]
    n = code.n
    alone = relay_cpu(code).decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    both = relay_cpu(code)
    plain = minsum_cpu(code)
    plain_alone = plain.decode_batch(sX, sZ, p, 20, "syndrome")
    for d in (both, plain):
        d.set_option("osd_order", lam)
        d.set_option("osd", 1)
    got = both.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    ref = plain.decode_batch(sX, sZ, p, 20, "syndrome")
    assert both.last_path() == {"minsum", "relay", "osd"}
    assert np.array_equal(got[3], alone[3])
    assert not (got[2] & 3).any()
    shared = 0
    for sec, bit in ((0, 1), (1, 2)):
        ok = (alone[2] & bit) == 0
        assert np.array_equal(got[sec][ok], alone[sec][ok])
        fail_both = ~ok & ((plain_alone[2] & bit) != 0)
        shared += int(fail_both.sum())
        assert np.array_equal(got[sec][fail_both], ref[sec][fail_both])
        assert both.get_option("osd_sectors") <= plain.get_option("osd_sectors")
    assert shared > 0 and both.get_option("osd_sectors") == int(((alone[2] & 1) != 0).sum() + ((alone[2] & 2) != 0).sum())


# ---- the RELAY kernels of bp_sparse.hip, restated -------------------------------------------------------------------------
# sparse_kernels_of_stop / launch_decode_sparse: the shape and the workspace are the scalar plan's (plan_of), priors and S
# are runtime branches of the one body, and the route chooses GENERAL: 2 routes x 3 shapes x LDS / HBM x 3 stops
RELAY_INSTANCES = {(k, s, mem, stop) for k in KERNELS for s in SHAPES for mem in ("lds", "hbm") for stop in STOPS}
GPU_CASES = CASES


def relay_instance_of(code, general, stop):
    p = plan_of(code, general)
    return (p["kernel"], p["shape"], p["mem"], stop)


def test_gpu_case_table_reaches_every_relay_instantiation():
    reached = {relay_instance_of(code_of(name, route), route == "general", stop) for name, route in GPU_CASES for stop in STOPS}
    assert len(RELAY_INSTANCES) == 36
    assert reached == RELAY_INSTANCES, sorted(RELAY_INSTANCES - reached)
    lds = {relay_instance_of(code_of(name, route), route == "general", stop) for name, route in LDS_CASES for stop in STOPS}
    assert lds == {i for i in RELAY_INSTANCES if i[2] == "lds"} and len(lds) == 18


# ---- CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_relay_on_the_cpu_engine(tmp_path):
    """--relay FILE [--relay-solutions S] with --bp-method minsum reproduces the Python counters of GetStatistics under
    the same tables; without the method, with a malformed file or a bad S it is refused."""
    from qec_ldpc_amd.codes import write_css_file
    from test_osd_host import _cli, _fields
    HX, HZ = code_matrices("hgp_ham")
    path = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    code = q.Quantum_LDPC_Code.createFromFile(path).with_logical("degenerate")
    gX, gZ = tables(code.n)
    table = tmp_path / "relay.txt"
    table.write_text("".join(" ".join(repr(float(x)) for x in row) + "\n" for row in np.concatenate([gX, gZ])))
    W, B, N, p, seed = 4, 1500, 20, 0.05, 7
    base = ["--engine", "cpu", "--seed", str(seed), "--logical", "degenerate"]
    keys = {"Corrected": "corrected", "Syndrome Errors X": "syndromeErrorsX", "Syndrome Errors Z": "syndromeErrorsZ",
            "Logical Errors": "logicalErrors", "Convergence Fail X": "convergenceFailX",
            "Convergence Fail Z": "convergenceFailZ", "Errors Tested": "numErrorsTested"}
    out = {}
    for tag, flags, S in (("plain", ["--bp-method", "minsum"], 0),
                          ("relay", ["--bp-method", "minsum", "--relay", str(table)], 1),
                          ("relay3", ["--bp-method", "minsum", "--relay", str(table), "--relay-solutions", "3"], 3)):
        d = tmp_path / tag
        d.mkdir()
        r = _cli(d, base + flags, path, "%d %d %d %d %g" % (W, W, B, N, p))
        assert r.returncode == 0, r.stderr
        f = _fields(d)
        dec = minsum_cpu(code)
        if S:
            dec.set_relay(gX, gZ, solutions=S)
        tested = int(f["Errors Tested"])
        assert B // 2 < tested <= B
        st = dec.GetStatistics(W, tested, p, N, seed=seed)
        out[tag] = {k: int(f[k]) for k in keys}
        assert out[tag] == {k: st[v] for k, v in keys.items()}, tag
    assert out["relay"] != out["plain"]
    short = tmp_path / "short.txt"
    short.write_text("\n".join(table.read_text().splitlines()[:-1]) + "\n")
    ragged = tmp_path / "ragged.txt"
    ragged.write_text(table.read_text() + "0.5\n")
    bad = (["--relay", str(table)], ["--bp-method", "product", "--relay", str(table)],
           ["--bp-method", "minsum", "--relay-solutions", "3"], ["--bp-method", "minsum", "--relay", str(table), "--relay-solutions", "0"],
           ["--bp-method", "minsum", "--relay", str(table), "--relay-solutions", "65"])
    for k, flags in enumerate(bad):
        d = tmp_path / ("bad%d" % k)
        d.mkdir()
        assert _cli(d, base + flags, path, "4 4 10 20 0.05").returncode == 2, flags
    # a file that cannot be read as 2 L lines of n floats ends the run with the message, as --priors does
    for k, name in enumerate((tmp_path / "missing.txt", short, ragged)):
        d = tmp_path / ("file%d" % k)
        d.mkdir()
        r = _cli(d, base + ["--bp-method", "minsum", "--relay", str(name)], path, "4 4 10 20 0.05")
        assert r.returncode == 1 and "--relay" in r.stderr, name

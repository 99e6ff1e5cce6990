"""Scaled min-sum BP in the LLR domain, set_option("bp_method", 1) with set_option("minsum_scale", k): DESIGN.md
section 2, "The min-sum form", restated in numpy (float32 adds in the stated order, one float32 multiply, integer
operations on .view(np.uint32)) and held against the CPU engine; the channel LLR (qec_minsum_llr) against numpy; the
OSD stage under the LLR column key against the numpy restatements of tests/test_osd_host.py / test_osd_cs_host.py; the
options and their refusals; the CLI; and the restated choice among the 36 MINSUM kernels of bp_sparse.hip over the
case table that tests/test_gpu_minsum.py runs on the device (asserted here to reach all 36).  The refusal of a
wave-circulant handle needs a device and is in tests/test_gpu_minsum.py.

Every comparison is bit for bit (q_final as uint32 patterns).  There is no tolerance, and no NaN to match: every
value of the min-sum form is finite, which is asserted.  The tests take the channel LLRs from the library, so that
exactness does not hang on one libm's log; the table itself is held to numpy's value within 1 ulp.

Iteration counts of the yardstick, X / Z, the 51 rows of test_sparse_shapes.inputs, cap 20, scale 160 (MS_P is the
decode p chosen per code so that the stop rules end sectors at the first test, at the cap and, under the syndrome
stop, between; p = 0.05 serves every code, as it serves the serial schedule's file; at MS_P_REF = 0.005 the channel
LLR ln 299 = 5.70 is outside the band, so the reference stop can end a sector at its first test):

  code         syndrome stop, p = 0.05                          ref stop, p = 0.005
  hgp_ham      {1,2,3,7,20} / {1,2,4,20}                        {1,11,20} / {1,11,20}
  mid          {1,2,5,6,8,20} / {1,2,3,20}                      {1,20} / {1,11,20}
  wide         {1,2,20} / {1,3,5,9,16,17,20}                    {1,20} / {1,11,20}
  dense32      {1,3,20} / {1,20}                                {1,20} / {1,11,20}
  tall         {1,20} / {1,6,20}                                {1,20} / {1,11,20}
  r3-3-6-13    {1,2,4,5,9,10,14,20} / {1,2,3,4,5,20}            {1,11,20} / {1,11,20}
  r4-5-10-7    {1,3,20} / {1,20}                                {1,11,20} / {1,11,20}
  r3-9-20-7    {1,2,20} / {1,2,3,5,8,9,10,12,14,20}             {1,11,20} / {1,11,20}
  r2-12-6-13   {1,2,4,20} / {1,2,20}                            {1,20} / {1,11}
  r3-3-18-5    {1,20} / {1,20}                                  {1,11,20} / {1,11,20}

r3-3-18-5 has no exit strictly between 1 and the cap (NO_MID_RUN_EXIT); r2-12-6-13's Z sector (column weight 12)
never runs to the cap under the reference stop, at p = 0.002, 0.005, 0.009, 0.013 and 0.02 alike, as under the
product rule (test_sparse_shapes.NEVER_TO_CAP): its distribution is asserted instead.
"""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from test_general_code import NS, STOPS, assert_same_decode, code_matrices, general_code, same_floats
from test_osd_cs_host import YardstickCS
from test_osd_host import gf2_rank
from test_priors import VECTORS, prior_vectors
from test_sparse_shapes import CASES, KERNELS, LDS_CASES, REGULAR, SHAPES, SMALL_GENERAL, SMALL_REGULAR, code_of, inputs, matrices, plan_of

F32 = np.float32
U32 = np.uint32
CAP = U32(0x49800000)          # K: the pattern of 2^20
LLR_MAX = F32(1073741824.0)    # Lambda = 2^30
INSIDE = F32(4.5951198)        # ln 99
SCALES = (160, 256)


# ---- the yardstick: "The min-sum form" of DESIGN.md section 2 in numpy ------------------------------------------------
def minsum_sector(H, s, llr, alpha_k, N, stop, D):
    """One sector of a batch, elementwise over the batch.  llr: the channel LLR of every variable.
    -> (e [B, n], syndrome failed [B], convergence failed [B], iterations [B], q [B, m, D])."""
    m, n = H.shape
    B = s.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]                                  # N(c), ascending
    edges = [[(int(c), int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]  # M(v)
    real = np.zeros((m, D), dtype=bool)
    for c in range(m):
        real[c, :len(nbr[c])] = True
    lam = np.asarray(llr, dtype=F32)
    alpha = F32(alpha_k) / F32(256.0)
    connected = np.array([len(edges[v]) > 0 for v in range(n)])
    M = np.zeros((B, m, D), dtype=F32)                                             # unused slots read +0.0f
    for c in range(m):
        M[:, c, :len(nbr[c])] = lam[nbr[c]]
    d = np.broadcast_to(((lam < F32(0.0)) & connected).astype(np.uint8), (B, n)).copy()  # N = 0
    t = (s != 0).astype(U32)                                                       # truthiness of the syndrome entry
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)

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
            others = ~np.eye(dc, dtype=bool)[None]                                 # [1, slot i, input k]: k != i
            mag = np.where(others, a[:, None, :], U32(0xFFFFFFFF)).min(axis=2)     # as unsigned integers
            mag = np.minimum(mag, CAP)                                             # a check of degree 1 sends K
            sign = np.bitwise_xor.reduce(np.where(others, g[:, None, :], U32(0)), axis=2) ^ t[:, c, None]
            out = (alpha * np.ascontiguousarray(mag).view(F32)).astype(F32)
            R[:, c, :dc] = (out.view(U32) | (sign << U32(31))).view(F32)
        return R

    def variable_update(R, last):
        new = np.zeros_like(R)
        dec = np.zeros((B, n), dtype=np.uint8)
        for v in range(n):
            if not connected[v]:
                continue                                                           # decides 0, takes part in no test
            rs = [R[:, c, k] for c, k in edges[v]]
            post = np.full(B, lam[v], dtype=F32)
            for r in rs:
                post = post + r
            dec[:, v] = post < F32(0.0)
            for j, (c, k) in enumerate(edges[v]):
                if last:
                    new[:, c, k] = post
                else:
                    x = np.full(B, lam[v], dtype=F32)
                    for i, r in enumerate(rs):
                        if i != j:
                            x = x + r
                    new[:, c, k] = x
        return new, dec

    with np.errstate(all="ignore"):
        for it in range(N):
            if not active.any():
                break
            iters += active
            new, dec = variable_update(check_update(M), it == N - 1)
            M = np.where(active[:, None, None], new, M)
            d = np.where(active[:, None], dec, d)
            if stop == "ref" and it % 10 == 0:
                active &= inside_any(M)
            elif stop == "syndrome":
                active &= syndrome_fails(d)
    return d, syndrome_fails(d), inside_any(M), iters, M


def library_llr(pi):
    return np.array([q.minsum_llr(x) for x in np.asarray(pi, dtype=F32)], dtype=F32)


def minsum_yardstick(HX, HZ, sX, sZ, piX, piZ, alpha_k, N, stop):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D]); piX / piZ: n priors each, or a scalar p for both.
    The channel LLRs are the library's."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    n = HX.shape[1]
    if np.ndim(piX) == 0:
        lX = lZ = np.full(n, q.minsum_llr(F32(2.0) / F32(3.0) * F32(piX)), dtype=F32)
    else:
        lX, lZ = library_llr(piX), library_llr(piZ)
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fx, cx, ix, qx = minsum_sector(HX, sX, lX, alpha_k, N, stop, D)
    eZ, fz, cz, iz, qz = minsum_sector(HZ, sZ, lZ, alpha_k, N, stop, D)
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32)


SMALL = SMALL_GENERAL + tuple(SMALL_REGULAR)
MS_P = dict.fromkeys(SMALL, 0.05)
MS_P_REF = 0.005
PRIOR_NS = (0, 1, 11)  # under priors, as test_serial.py thins them
_yard = {}


def yard(name, kind, stop, N, scale=160, p=None):
    """The yardstick's decode of inputs(name), computed once and shared with tests/test_gpu_minsum.py.
    kind: "scalar" (p, default MS_P[name]) or one of test_priors.VECTORS."""
    if kind == "scalar" and p is None:
        p = MS_P[name]
    key = (name, kind, stop, N, scale, p)
    if key not in _yard:
        HX, HZ = matrices(name)
        pri = (p, p) if kind == "scalar" else prior_vectors(HX.shape[1], kind)
        _yard[key] = minsum_yardstick(HX, HZ, *inputs(name), pri[0], pri[1], scale, N, stop)
    return _yard[key]


def minsum_cpu(code, scale=160, priors=None):
    dec = q.DecoderCPU(code)
    dec.set_option("minsum_scale", scale)
    dec.set_option("bp_method", 1)
    if priors is not None:
        dec.set_priors(*priors)
    return dec


def routes(name):
    return ("graph", "general") if name in REGULAR else ("general",)


# ---- the CPU engine against the yardstick -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_cpu_engine_matches_the_yardstick(name):
    """Scalar p: every stop rule, every N, scale 160 and 256, both routes of a regular code."""
    sX, sZ = inputs(name)
    for scale in SCALES:
        decs = [minsum_cpu(code_of(name, r), scale) for r in routes(name)]
        for stop in STOPS:
            for N in NS:
                for p in (MS_P[name],) + ((MS_P_REF,) if stop == "ref" and N in (11, 20) else ()):
                    want = yard(name, "scalar", stop, N, scale, p)
                    assert np.isfinite(want[4]).all()
                    for r, dec in zip(routes(name), decs):
                        got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                        assert_same_decode(got, want, "%s %s %s k=%d p=%g N=%d" % (name, r, stop, scale, p, N))
                        assert dec.last_path() == {"minsum"}


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("kind", VECTORS)
def test_cpu_engine_matches_the_yardstick_under_priors(name, kind):
    """The prior vectors of test_priors (the special one holds 0, 1/2 and 1)."""
    HX, HZ = matrices(name)
    sX, sZ = inputs(name)
    pri = prior_vectors(HX.shape[1], kind)
    for scale in SCALES:
        decs = [minsum_cpu(code_of(name, r), scale, pri) for r in routes(name)]
        for stop in STOPS:
            for N in PRIOR_NS:
                want = yard(name, kind, stop, N, scale)
                assert np.isfinite(want[4]).all()  # 0, 1/2 and 1 among the priors, an entry > 1 among the syndromes
                for r, dec in zip(routes(name), decs):
                    got = dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)  # p is not used
                    assert_same_decode(got, want, "%s %s %s %s k=%d N=%d" % (name, r, kind, stop, scale, N))
    assert not same_floats(yard(name, "scalar", "fixed", 11)[4], yard(name, kind, "fixed", 11)[4])  # the priors matter


# ---- coverage -----------------------------------------------------------------------------------------------------------
# the table of the module docstring: (code, stop) -> the iteration counts of sector X, of sector Z
ITERATIONS = {
    ("hgp_ham", "syndrome"): ({1, 2, 3, 7, 20}, {1, 2, 4, 20}), ("hgp_ham", "ref"): ({1, 11, 20}, {1, 11, 20}),
    ("mid", "syndrome"): ({1, 2, 5, 6, 8, 20}, {1, 2, 3, 20}), ("mid", "ref"): ({1, 20}, {1, 11, 20}),
    ("wide", "syndrome"): ({1, 2, 20}, {1, 3, 5, 9, 16, 17, 20}), ("wide", "ref"): ({1, 20}, {1, 11, 20}),
    ("dense32", "syndrome"): ({1, 3, 20}, {1, 20}), ("dense32", "ref"): ({1, 20}, {1, 11, 20}),
    ("tall", "syndrome"): ({1, 20}, {1, 6, 20}), ("tall", "ref"): ({1, 20}, {1, 11, 20}),
    ("r3-3-6-13", "syndrome"): ({1, 2, 4, 5, 9, 10, 14, 20}, {1, 2, 3, 4, 5, 20}), ("r3-3-6-13", "ref"): ({1, 11, 20}, {1, 11, 20}),
    ("r4-5-10-7", "syndrome"): ({1, 3, 20}, {1, 20}), ("r4-5-10-7", "ref"): ({1, 11, 20}, {1, 11, 20}),
    ("r3-9-20-7", "syndrome"): ({1, 2, 20}, {1, 2, 3, 5, 8, 9, 10, 12, 14, 20}), ("r3-9-20-7", "ref"): ({1, 11, 20}, {1, 11, 20}),
    ("r2-12-6-13", "syndrome"): ({1, 2, 4, 20}, {1, 2, 20}), ("r2-12-6-13", "ref"): ({1, 20}, {1, 11}),
    ("r3-3-18-5", "syndrome"): ({1, 20}, {1, 20}), ("r3-3-18-5", "ref"): ({1, 11, 20}, {1, 11, 20}),
}
# codes whose run under the syndrome stop has no exit strictly between 1 and the cap
NO_MID_RUN_EXIT = ("r3-3-18-5",)
# (code, stop, sector) that never runs to the cap, at any decode p tried (module docstring)
NEVER_TO_CAP = {("r2-12-6-13", "ref", 1): {1, 11}}


def iteration_sets(name, stop, p):
    it = yard(name, "scalar", stop, 20, 160, p)[3]
    return [set(int(x) for x in it[:, sec]) for sec in (0, 1)]


def test_coverage():
    """On the yardstick, cap 20: the distributions of the module docstring.  Under the syndrome stop and under the
    reference stop (at MS_P_REF) every sector has a row ending at the first test and, but for NEVER_TO_CAP, one running
    to the cap; under the syndrome stop every code outside NO_MID_RUN_EXIT has an exit strictly between."""
    flags = []
    for name in SMALL:
        for stop, p in (("syndrome", MS_P[name]), ("ref", MS_P_REF)):
            seen = iteration_sets(name, stop, p)
            assert tuple(seen) == ITERATIONS[name, stop], (name, stop, seen)
            for sec in (0, 1):
                assert 1 in seen[sec], (name, stop, sec, seen)
                if (name, stop, sec) in NEVER_TO_CAP:
                    assert seen[sec] == NEVER_TO_CAP[name, stop, sec]
                else:
                    assert 20 in seen[sec], (name, stop, sec, seen)
            if stop == "syndrome":
                mid = any(1 < k < 20 for s in seen for k in s)
                assert mid != (name in NO_MID_RUN_EXIT), (name, seen)
            flags.append(yard(name, "scalar", stop, 20, 160, p)[2])
    flags = np.concatenate(flags)
    assert (flags == 0).any()
    for bit in (q.SYNDROME_FAIL_X, q.SYNDROME_FAIL_Z, q.CONVERGENCE_FAIL_X, q.CONVERGENCE_FAIL_Z):
        assert (flags & bit).any(), bit


def test_finiteness_and_bounds():
    """Every message is finite: |lambda| <= 2^30, a check output is at most alpha 2^20, and a sum has at most dv + 1
    terms.  The special priors and the row with a syndrome entry > 1 are among the inputs."""
    for name in ("dense32", "tall", "r2-12-6-13"):
        dv = max(int(H.sum(axis=0).max()) for H in matrices(name))
        for kind in ("scalar", "special"):
            for N in (1, 11):
                qf = yard(name, kind, "fixed", N)[4]
                assert np.isfinite(qf).all()
                assert np.abs(qf).max() <= float(LLR_MAX) + dv * 0.625 * 2.0 ** 20


# ---- consequences -------------------------------------------------------------------------------------------------------
def test_uniform_priors_equal_the_scalar_call():
    name, p = "mid", 0.05
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    uniform = np.full(code.n, F32(2.0) / F32(3.0) * F32(p), dtype=F32)
    a, b = minsum_cpu(code), minsum_cpu(code, priors=(uniform, uniform))
    for stop, N in (("fixed", 11), ("syndrome", 20), ("ref", 20), ("fixed", 0)):
        assert_same_decode(b.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True),
                           a.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True), "%s N=%d" % (stop, N))


def test_scale_and_method_matter():
    name, p = "hgp_ham", 0.05
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    k160 = minsum_cpu(code, 160).decode_batch(sX, sZ, p, 5, "fixed", want_q=True)
    k256 = minsum_cpu(code, 256).decode_batch(sX, sZ, p, 5, "fixed", want_q=True)
    prod = q.DecoderCPU(code).decode_batch(sX, sZ, p, 5, "fixed", want_q=True)
    assert not same_floats(k160[4], k256[4])
    assert not same_floats(k160[4], prod[4])
    assert (k160[4] > 1.0).any() and not (prod[4] > 1.0).any()  # LLRs there, probabilities here


def test_zero_syndrome_row():
    for name in ("hgp_ham", "tall", "r4-5-10-7"):
        sX, sZ = inputs(name)
        row = len(sX) - 3
        assert not sX[row].any() and not sZ[row].any()
        eX, eZ, flags, iters = minsum_cpu(code_of(name, "general")).decode_batch(sX, sZ, MS_P[name], 20, "syndrome",
                                                                                  want_iters=True)[:4]
        assert not eX[row].any() and not eZ[row].any() and (iters[row] == 1).all() and not flags[row] & 3


def test_round_trip_restores_the_product_rule():
    name = "hgp_ham"
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    dec = q.DecoderCPU(code)
    first = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    dec.set_option("bp_method", 1)
    dec.decode_batch(sX, sZ, 0.05, 20, "syndrome")
    dec.set_option("bp_method", 0)
    assert_same_decode(dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True), first, "0 -> 1 -> 0")
    assert "minsum" not in dec.last_path()


def _ulps(a, b):
    def key(x):
        i = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_minsum_llr_against_numpy():
    rng = np.random.default_rng(7)
    pi = np.concatenate([np.exp(rng.uniform(np.log(1e-30), np.log(0.5), 400)), 1.0 - np.exp(rng.uniform(np.log(1e-7), np.log(0.5), 400)),
                         prior_vectors(200, "random")[0]]).astype(F32)
    pi = pi[(pi > 0) & (pi < 1)]
    got = library_llr(pi)
    want = np.log((1.0 - pi.astype(np.float64)) / pi.astype(np.float64)).astype(F32)
    assert _ulps(got, want).max() <= 1
    for x, bits in ((0.0, 0x4E800000), (0.5, 0x00000000), (1.0, 0xCE800000)):
        assert int(np.array([q.minsum_llr(x)], dtype=F32).view(U32)[0]) == bits, x
    assert q.minsum_llr(0.0) == LLR_MAX and q.minsum_llr(1.0) == -LLR_MAX
    # the tables of a handle: built by set_priors whatever the method says, read back by minsum_llr()
    code = code_of("hgp_ham", "general")
    dec = q.DecoderCPU(code)
    with pytest.raises(q.QecError, match="no priors"):
        dec.minsum_llr()
    assert q.lib().qec_decoder_get_minsum_llr(dec._h, None, None) == -1  # QEC_ERR_ARG
    pri = prior_vectors(code.n, "special")
    dec.set_priors(*pri)
    assert dec.get_option("bp_method") == 0
    for got, p in zip(dec.minsum_llr(), pri):
        assert got.dtype == F32 and np.array_equal(got.view(U32), library_llr(p).view(U32))
        assert {0x4E800000, 0x00000000, 0xCE800000} <= set(int(x) for x in got.view(U32))


# ---- OSD under the LLR key ----------------------------------------------------------------------------------------------
def osd_key_llr(r):
    """~(bits ^ (sign ? 0xFFFFFFFF : 0x80000000)): descending keys are ascending LLRs, -0.0f directly before +0.0f."""
    bits = np.ascontiguousarray(r, dtype=F32).view(U32)
    return (~(bits ^ np.where(bits >> U32(31), U32(0xFFFFFFFF), U32(0x80000000)))).astype(U32)


def test_osd_key_llr_orders_by_llr_ascending():
    x = np.array([-LLR_MAX, -5.5, -1e-40, -0.0, 0.0, 1e-40, 0.625, 4.5951198, LLR_MAX], dtype=F32)
    key = osd_key_llr(x).astype(np.int64)
    assert (np.diff(key) < 0).all()
    assert int(osd_key_llr(np.array([0.0], dtype=F32))[0]) == 0x7FFFFFFF


class MinSumOsd(YardstickCS):
    """The restatements of sections 1.2 / 1.3 over any code's matrices, with the LLR key in the column order."""

    def __init__(self, code):
        self.n, self.L = code.n, code.stride
        self.H = [code.pcm(0), code.pcm(1)]
        self.rank = [gf2_rank(h) for h in self.H]
        self.qn = (code.numEqsX + code.numEqsZ) * self.L
        self.pos, base = [], 0
        for H in self.H:
            pos = np.empty(self.n, dtype=np.int64)
            for v in range(self.n):
                c = int(np.nonzero(H[:, v])[0][0])
                pos[v] = base + c * self.L + int(H[c, :v].sum())
            self.pos.append(pos)
            base += H.shape[0] * self.L

    def reduce(self, sec, s, qrow):
        H, n = self.H[sec], self.n
        key = osd_key_llr(qrow[self.pos[sec]]).astype(np.int64)
        order = np.lexsort((np.arange(n), -key))  # key descending, ties by v ascending
        A = np.concatenate([H, np.asarray(s, dtype=np.uint8)[:, None] & 1], axis=1).astype(np.uint8)
        used = np.zeros(H.shape[0], dtype=bool)
        piv = []
        for v in order:
            if len(piv) == self.rank[sec]:
                break
            rows = np.nonzero(A[:, v].astype(bool) & ~used)[0]
            if not len(rows):
                continue
            p = rows[0]
            others = A[:, v].astype(bool)
            others[p] = False
            A[others] ^= A[p]
            used[p] = True
            piv.append((p, v))
        if A[~used, n].any():
            return None
        return A, piv, order


OSD_CODES = {"hgp_ham": (lambda: general_code("hgp_ham"), 0.05, 384, 40),
             "qc-3-3-6-13": (lambda: q.QC_LDPC_CSS(3, 3, 6, 13, 3, 2), 0.05, 256, 40)}  # code, p, samples, failed sectors >=
OSD_SEED = 0x51EC0DE
_osd = {}


def osd_case(name):
    """(code, sX, sZ, p, main decode of the yardstick, its soft decode of the failed samples, their indices)."""
    if name not in _osd:
        make, p, B, _ = OSD_CODES[name]
        code = make()
        HX, HZ = code.pcm(0), code.pcm(1)
        x, z = depolarizing(OSD_SEED, 0, B, code.n, p)
        sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        main = minsum_yardstick(HX, HZ, sX, sZ, p, p, 160, 20, "syndrome")
        bad = np.nonzero(main[2] & 3)[0]
        soft = minsum_yardstick(HX, HZ, sX[bad], sZ[bad], p, p, 160, 3, "fixed")[4]
        _osd[name] = (code, sX, sZ, p, main, soft, bad)
    return _osd[name]


@pytest.mark.parametrize("name", sorted(OSD_CODES))
@pytest.mark.parametrize("lam", [0, 10])
def test_decoder_cpu_with_osd_under_minsum(name, lam):
    """osd = 1, osd_order 0 and 10, method 1: the numpy restatements fed with the yardstick's min-sum soft decode
    (osd_iterations = 3, fixed stop) and the LLR key."""
    code, sX, sZ, p, main, soft, bad = osd_case(name)
    failed = int(((main[2] & 1) != 0).sum() + ((main[2] & 2) != 0).sum())
    assert failed >= OSD_CODES[name][3], failed
    ys = MinSumOsd(code)
    r = ys.repair_cs(sX[bad], sZ[bad], soft, main[0][bad], main[1][bad], main[2][bad], (lam,))[lam]
    wX, wZ, wf = main[0].copy(), main[1].copy(), main[2].copy()
    wX[bad], wZ[bad], wf[bad] = r[0], r[1], r[2]
    dec = minsum_cpu(code)
    assert dec.get_option("osd_iterations") == 3
    dec.set_option("osd_order", lam)
    dec.set_option("osd", 1)
    got = dec.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    assert dec.last_path() == {"minsum", "osd"}
    for a, b, what in zip(got[:4], (wX, wZ, wf, main[3]), ("eX", "eZ", "flags", "iters")):
        assert np.array_equal(a, b), what
    assert dec.get_option("osd_sectors") == r[3] == failed and dec.get_option("osd_cs_sectors") == r[4]
    assert not (got[2] & 3).any()
    # the key matters: the product rule's key on the same soft input gives another repair somewhere
    plain = YardstickCS(ys).repair_cs(sX[bad], sZ[bad], soft, main[0][bad], main[1][bad], main[2][bad], (lam,))[lam]
    assert not (np.array_equal(plain[0], r[0]) and np.array_equal(plain[1], r[1]))
    # qec_osd reads the method at the call
    o = dec.osd(sX[bad], sZ[bad], soft, main[0][bad], main[1][bad], main[2][bad])
    for a, b in zip(o[:3], r[:3]):
        assert np.array_equal(a, b)


# ---- the options --------------------------------------------------------------------------------------------------------
def test_option_values_and_refusals():
    code = code_of("hgp_ham", "general")
    dec = q.DecoderCPU(code)
    assert q.OPTION["bp_method"] == 19 and q.OPTION["minsum_scale"] == 20 and q.PATH["minsum"] == 2048
    assert q.BP_METHOD == {"product": 0, "minsum": 1}
    assert dec.get_option("bp_method") == 0 and dec.get_option("minsum_scale") == 160
    for bad in (2, -1):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
            dec.set_option("bp_method", bad)
        assert q.lib().qec_decoder_set_option(dec._h, 19, bad) == -1  # QEC_ERR_ARG
    for bad in (0, 257, -5):
        with pytest.raises(q.QecError, match="QEC_OPT_MINSUM_SCALE"):
            dec.set_option("minsum_scale", bad)
        assert q.lib().qec_decoder_set_option(dec._h, 20, bad) == -1
    assert dec.get_option("bp_method") == 0 and dec.get_option("minsum_scale") == 160
    for k in (1, 256, 200):
        dec.set_option("minsum_scale", k)
        assert dec.get_option("minsum_scale") == k
    dec.set_option("minsum_scale", 160)
    # the other option first: min-sum is refused, the handle unchanged
    for other, value in (("correlated", 1), ("correlated", 2), ("bp_schedule", 1)):
        dec.set_option(other, value)
        with pytest.raises(q.QecError, match="QEC_OPT_" + other.upper()):
            dec.set_option("bp_method", 1)
        assert q.lib().qec_decoder_set_option(dec._h, 19, 1) == -4  # QEC_ERR_UNSUPPORTED
        assert dec.get_option("bp_method") == 0 and dec.get_option(other) == value
        dec.set_option("bp_method", 0)  # the product rule is always accepted
        dec.set_option(other, 0)
    # min-sum first: the other option is refused, the handle unchanged
    dec.set_option("bp_method", 1)
    for other, value in (("correlated", 1), ("correlated", 2), ("bp_schedule", 1)):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
            dec.set_option(other, value)
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION[other], value) == -4
        assert dec.get_option("bp_method") == 1 and dec.get_option(other) == 0
        dec.set_option(other, 0)
    sX, sZ = inputs("hgp_ham")
    assert_same_decode(dec.decode_batch(sX, sZ, 0.05, 5, "fixed", want_iters=True, want_q=True),
                       minsum_cpu(code).decode_batch(sX, sZ, 0.05, 5, "fixed", want_iters=True, want_q=True), "after refusals")


def test_near_hard_option_changes_nothing_under_minsum():
    code = code_of("r3-3-6-13", "graph")
    sX, sZ = inputs("r3-3-6-13")
    a, b = minsum_cpu(code), minsum_cpu(code)
    b.set_option("near_hard", 0)
    for stop in ("fixed", "ref"):
        assert_same_decode(a.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True),
                           b.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True), stop, with_q=False)
        assert_same_decode(a.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True),
                           yard("r3-3-6-13", "scalar", stop, 20, 160, 0.005), stop, with_q=False)


# ---- the MINSUM kernels of bp_sparse.hip, restated -----------------------------------------------------------------------
# sparse_kernels / sparse_plan_create: the shape and the workspace are the scalar plan's (plan_of), priors are a runtime
# branch of the one kernel, and the route chooses between the two kernels: 2 kernels x 3 shapes x LDS / HBM x 3 stops
MINSUM_INSTANCES = {(k, s, mem, stop) for k in KERNELS for s in SHAPES for mem in ("lds", "hbm") for stop in STOPS}
GPU_CASES = CASES  # the case table of tests/test_gpu_minsum.py: every row, scalar p and priors, every stop rule


def instance_of(code, general, stop):
    p = plan_of(code, general)
    return (p["kernel"], p["shape"], p["mem"], stop)


def test_gpu_case_table_reaches_every_minsum_instantiation():
    reached = {instance_of(code_of(name, route), route == "general", stop) for name, route in GPU_CASES for stop in STOPS}
    assert len(MINSUM_INSTANCES) == 36
    assert reached == MINSUM_INSTANCES, sorted(MINSUM_INSTANCES - reached)
    lds = {instance_of(code_of(name, route), route == "general", stop) for name, route in LDS_CASES for stop in STOPS}
    assert lds == {i for i in MINSUM_INSTANCES if i[2] == "lds"} and len(lds) == 18


# ---- CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_bp_method_on_the_cpu_engine(tmp_path):
    """--bp-method minsum [--minsum-scale K] reproduces the Python counters of GetStatistics under method 1; product
    those under 0; other values, a scale without the method, and --correlated or --bp-schedule serial beside it are
    refused."""
    from qec_ldpc_amd.codes import write_css_file
    from test_osd_host import _cli, _fields
    HX, HZ = code_matrices("hgp_ham")
    path = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    code = q.Quantum_LDPC_Code.createFromFile(path).with_logical("degenerate")
    W, B, N, p, seed = 4, 1500, 20, 0.05, 7
    base = ["--engine", "cpu", "--seed", str(seed), "--logical", "degenerate"]
    keys = {"Corrected": "corrected", "Syndrome Errors X": "syndromeErrorsX", "Syndrome Errors Z": "syndromeErrorsZ",
            "Logical Errors": "logicalErrors", "Convergence Fail X": "convergenceFailX",
            "Convergence Fail Z": "convergenceFailZ", "Errors Tested": "numErrorsTested"}
    out = {}
    for tag, flags, method, scale in (("product", ["--bp-method", "product"], 0, 160),
                                      ("minsum", ["--bp-method", "minsum"], 1, 160),
                                      ("minsum256", ["--bp-method", "minsum", "--minsum-scale", "256"], 1, 256)):
        d = tmp_path / tag
        d.mkdir()
        r = _cli(d, base + flags, path, "%d %d %d %d %g" % (W, W, B, N, p))
        assert r.returncode == 0, r.stderr
        f = _fields(d)
        dec = q.DecoderCPU(code)
        dec.set_option("minsum_scale", scale)
        dec.set_option("bp_method", method)
        tested = int(f["Errors Tested"])  # the CLI tests (B / threads) * threads samples, the first ones of the stream
        assert B // 2 < tested <= B
        st = dec.GetStatistics(W, tested, p, N, seed=seed)
        out[tag] = {k: int(f[k]) for k in keys}
        assert out[tag] == {k: st[v] for k, v in keys.items()}, tag
    assert out["minsum"] != out["product"] and out["minsum256"] != out["minsum"]
    bad = (["--bp-method", "sumproduct"], ["--minsum-scale", "200"], ["--bp-method", "minsum", "--minsum-scale", "0"],
           ["--bp-method", "minsum", "--minsum-scale", "257"], ["--bp-method", "minsum", "--correlated", "xz"],
           ["--bp-method", "minsum", "--bp-schedule", "serial"])
    for k, flags in enumerate(bad):
        d = tmp_path / ("bad%d" % k)
        d.mkdir()
        assert _cli(d, base + flags, path, "4 4 10 20 0.05").returncode == 2, flags

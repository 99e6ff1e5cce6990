"""Layered (check-sequential) min-sum, set_option("minsum_schedule", 1) under set_option("bp_method", 1): DESIGN.md
section 2, "The layered min-sum form", restated in numpy (float32 adds in the stated order, one float32 multiply, integer
operations on .view(np.uint32), sequential over the processing order) and held against the CPU engine; its non-vacuity;
that it is another decode than flooding min-sum and that option 0 restores flooding; that a relay ignores it; unused
slots and degree-0 variables; the option, its constants, its refusals and the CLI's exits; the restated choice among the
36 LAYERED kernels of bp_sparse.hip over the case table that tests/test_gpu_minsum_layered.py runs on the device; the
CPU reference table of the 80 wave codes that tests/test_gpu_wave_minsum_layered.py holds the wave kernels to, with its
non-vacuity conditions; the benefit on P61; and the OSD stage under the option.

Observed on the reference table (test_reference_table_is_not_vacuous): under (syndrome, 0.03, 20) every sector of every
code ends rows at two or more counts, every sector of the 56 codes with G > 1 has a wave of G consecutive rows with
mixed counts, and under (fixed, 0.03, 2) the layered q_final differs from flooding's in every code: none of the 160
(code, sector) rows needed pinning as an exception.  On P61 (test_layered_needs_fewer_iterations_on_p61): 6 010 layered
against 10 554 flooding iterations (0.569), 19 against 32 sectors left unsatisfied.

Every comparison is bit for bit (q_final as uint32 patterns).  There is no tolerance, and every value is finite, which is
asserted.  The channel LLRs are the library's, as in tests/test_minsum.py.
"""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.codes import P61, code_path
from test_circulant_shapes import PS, circulant_matrix, exponent_tables, groups, shape_id
from test_circulant_shapes import SHAPES as TABLE_SHAPES
from test_circulant_shapes import code_of as table_code_of
from test_circulant_shapes import inputs as table_inputs
from test_general_code import NS, STOPS, assert_same_decode, code_matrices, general_code, same_floats
from test_minsum import CAP, INSIDE, MS_P, MS_P_REF, PRIOR_NS, SMALL, library_llr, minsum_cpu, routes
from test_priors import VECTORS, prior_vectors
from test_serial import greedy_colours, processing_order
from test_sparse_shapes import CASES, KERNELS, LDS_CASES, SHAPES, code_of, inputs, matrices, plan_of
from test_wave_minsum import DECODE_CASES, PRIOR_CASES, SCALE, SYN20, YARDSTICK_CODES, count_sets, wave_mixes
from test_wave_minsum import reference as flooding_reference

F32 = np.float32
U32 = np.uint32
LLR_MAX = 1073741824.0  # 2^30


# ---- the yardstick: "The layered min-sum form" of DESIGN.md section 2 in numpy -------------------------------------------
def layered_minsum_sector(H, s, llr, alpha_k, N, stop, D):
    """One sector of a batch, sequential over the processing order, elementwise over the batch.  llr: the channel LLR
    of every variable.  -> (e [B, n], syndrome failed [B], convergence failed [B], iterations [B], q [B, m, D])."""
    m, n = H.shape
    B = s.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]                                  # N(c), ascending
    edges = [[(int(c), int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]  # M(v)
    order = processing_order(greedy_colours(H))
    lam = np.asarray(llr, dtype=F32)
    alpha = F32(alpha_k) / F32(256.0)
    connected = np.array([len(edges[v]) > 0 for v in range(n)])
    R = np.zeros((B, m, D), dtype=F32)                                             # every slot starts at +0.0f
    t = (s != 0).astype(U32)                                                       # truthiness of the syndrome entry
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)

    def fold(R, v, skip):
        x = np.full(B, lam[v], dtype=F32)
        for c, k in edges[v]:                                                      # ascending check order
            if c != skip:
                x = x + R[:, c, k]
        return x

    def posterior(R):
        post = np.zeros((B, n), dtype=F32)
        for v in range(n):
            if connected[v]:
                post[:, v] = fold(R, v, -1)
        return post

    def decide(post):
        return ((post < F32(0.0)) & connected[None]).astype(np.uint8)              # a variable in no check decides 0

    def syndrome_fails(e):
        bad = np.zeros(B, dtype=bool)
        for c in range(m):
            bad |= (e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) != s[:, c]      # the entry's exact value
        return bad

    def inside_any(post):
        return ((np.abs(post) < INSIDE) & connected[None]).any(axis=1)

    def check_update(qs, tc):
        """The min-sum check update of one check: qs [B, dc] -> R [B, dc]."""
        dc = qs.shape[1]
        bits = np.ascontiguousarray(qs).view(U32)
        a, g = bits & U32(0x7FFFFFFF), bits >> U32(31)
        others = ~np.eye(dc, dtype=bool)[None]                                     # [1, slot i, input k]: k != i
        mag = np.where(others, a[:, None, :], U32(0xFFFFFFFF)).min(axis=2)         # as unsigned integers
        mag = np.minimum(mag, CAP)                                                 # a check of degree 1 sends K
        sign = np.bitwise_xor.reduce(np.where(others, g[:, None, :], U32(0)), axis=2) ^ tc[:, None]
        out = (alpha * np.ascontiguousarray(mag).view(F32)).astype(F32)
        return (out.view(U32) | (sign << U32(31))).view(F32)

    with np.errstate(all="ignore"):
        for it in range(N):
            if not active.any():
                break
            iters += active
            new = R.copy()
            for c in order:
                qs = np.stack([fold(new, v, c) for v in nbr[c]], axis=1)
                new[:, c, :len(nbr[c])] = check_update(qs, t[:, c])
            R = np.where(active[:, None, None], new, R)
            if stop == "ref" and it % 10 == 0:
                active &= inside_any(posterior(R))
            elif stop == "syndrome":
                active &= syndrome_fails(decide(posterior(R)))
        post = posterior(R)
    e = decide(post)
    qf = np.zeros((B, m, D), dtype=F32)                                            # unused slots read +0.0f
    for c in range(m):
        qf[:, c, :len(nbr[c])] = post[:, nbr[c]]
    return e, syndrome_fails(e), inside_any(post), iters, qf


def layered_yardstick(HX, HZ, sX, sZ, piX, piZ, alpha_k, N, stop):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D]); piX / piZ: n priors each, or a scalar p for both.
    The channel LLRs are the library's."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    n = HX.shape[1]
    if np.ndim(piX) == 0:
        lX = lZ = np.full(n, q.minsum_llr(F32(2.0) / F32(3.0) * F32(piX)), dtype=F32)
    else:
        lX, lZ = library_llr(piX), library_llr(piZ)
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fx, cx, ix, qx = layered_minsum_sector(HX, sX, lX, alpha_k, N, stop, D)
    eZ, fz, cz, iz, qz = layered_minsum_sector(HZ, sZ, lZ, alpha_k, N, stop, D)
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32)


_yard = {}


def yard(name, kind, stop, N, scale=160, p=None):
    """The yardstick's decode of inputs(name), computed once and shared with tests/test_gpu_minsum_layered.py.
    kind: "scalar" (p, default MS_P[name]) or one of test_priors.VECTORS."""
    if kind == "scalar" and p is None:
        p = MS_P[name]
    key = (name, kind, stop, N, scale, p)
    if key not in _yard:
        HX, HZ = matrices(name)
        pri = (p, p) if kind == "scalar" else prior_vectors(HX.shape[1], kind)
        out = layered_yardstick(HX, HZ, *inputs(name), pri[0], pri[1], scale, N, stop)
        for a in out:
            a.setflags(write=False)
        _yard[key] = out
    return _yard[key]


def layered_cpu(code, scale=160, priors=None):
    dec = minsum_cpu(code, scale, priors)
    dec.set_option("minsum_schedule", 1)
    return dec


# ---- the CPU engine against the yardstick -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_cpu_engine_matches_the_yardstick(name):
    """Scalar p: every stop rule, every N, both routes of a regular code."""
    sX, sZ = inputs(name)
    decs = [layered_cpu(code_of(name, r)) for r in routes(name)]
    for stop in STOPS:
        for N in NS:
            for p in (MS_P[name],) + ((MS_P_REF,) if stop == "ref" and N == 11 else ()):
                want = yard(name, "scalar", stop, N, 160, p)
                assert np.isfinite(want[4]).all()
                for r, dec in zip(routes(name), decs):
                    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                    assert_same_decode(got, want, "%s %s %s p=%g N=%d" % (name, r, stop, p, N))
                    assert dec.last_path() == {"minsum", "serial"}


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("kind", VECTORS)
def test_cpu_engine_matches_the_yardstick_under_priors(name, kind):
    """The prior vectors of test_priors (the special one holds 0, 1/2 and 1)."""
    HX, HZ = matrices(name)
    sX, sZ = inputs(name)
    pri = prior_vectors(HX.shape[1], kind)
    decs = [layered_cpu(code_of(name, r), 160, pri) for r in routes(name)]
    for stop in STOPS:
        for N in PRIOR_NS:
            want = yard(name, kind, stop, N)
            assert np.isfinite(want[4]).all()  # 0, 1/2 and 1 among the priors, an entry > 1 among the syndromes
            dv = max(int(H.sum(axis=0).max()) for H in (HX, HZ))
            assert np.abs(want[4]).max() <= LLR_MAX + dv * 0.625 * 2.0 ** 20
            for r, dec in zip(routes(name), decs):
                got = dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)  # p is not used
                assert_same_decode(got, want, "%s %s %s %s N=%d" % (name, r, kind, stop, N))
    assert not same_floats(yard(name, "scalar", "fixed", 11)[4], yard(name, kind, "fixed", 11)[4])  # the priors matter


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("minsum_layered")


@pytest.mark.parametrize("row", YARDSTICK_CODES, ids=lambda r: "%s-P%d" % (shape_id(r[0]), r[1]))
def test_cpu_engine_matches_numpy_on_table_codes(tmp, row):
    """Four circulant codes of the wave table: their layers are their block rows."""
    shape, P = row
    EX, EZ = exponent_tables(shape, P)
    HX, HZ = circulant_matrix(EX, P), circulant_matrix(EZ, P)
    sX, sZ = table_inputs(tmp, shape, P)
    dec = layered_cpu(table_code_of(tmp, shape, P)[0])
    for stop, p, N in (("fixed", 0.03, 11), ("syndrome", 0.03, 20), ("ref", 0.005, 21), ("fixed", 0.03, 2)):
        want = layered_yardstick(HX, HZ, sX, sZ, p, p, 160, N, stop)
        got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, want, "%s P=%d %s" % (shape_id(shape), P, stop))


# ---- the CPU reference table of the 80 wave codes ---------------------------------------------------------------------------
# test_circulant_shapes' SHAPES x PS with its two batches per code, the decode cases of test_wave_minsum, the yardstick
# the CPU engine under layered min-sum at scale 160: computed here, once, and shared with
# tests/test_gpu_wave_minsum_layered.py as test_wave_minsum.reference shares the flooding outputs.
_cpu_table, _ref_table = {}, {}


def layered_reference(tmp, shape, P, case, kind="table", priors=None, scale=SCALE):
    """The CPU engine's (eX, eZ, flags, iters, q_final) of a decode case under layered min-sum.  priors: None or a kind
    of test_priors.prior_vectors."""
    key = (shape, P, case, kind, priors, scale)
    if key not in _ref_table:
        stop, p, N = case
        if (shape, P, scale) not in _cpu_table:
            _cpu_table[shape, P, scale] = layered_cpu(table_code_of(tmp, shape, P)[0], scale)
        dec = _cpu_table[shape, P, scale]
        try:
            if priors is not None:
                dec.set_priors(*prior_vectors(table_code_of(tmp, shape, P)[0].n, priors))
            out = dec.decode_batch(*table_inputs(tmp, shape, P, kind), p, N, stop, want_iters=True, want_q=True)
        finally:
            dec.set_priors(None, None)
        for a in out:
            a.setflags(write=False)
        _ref_table[key] = out
    return _ref_table[key]


# (shape, P, sector) whose rows all end at one count under (syndrome, 0.03, 20), as observed
ONE_COUNT = {}
# (shape, P, sector), G > 1, in which no wave of G consecutive rows mixes counts under (syndrome, 0.03, 20), as observed
NO_WAVE_MIX = {}
# (shape, P) whose q_final under (fixed, 0.03, 2) equals flooding min-sum's, as observed
SAME_AS_FLOODING = {}


@pytest.mark.parametrize("shape", TABLE_SHAPES, ids=shape_id)
def test_reference_table_is_not_vacuous(tmp, shape):
    one, nomix, same = set(), set(), set()
    for P in PS:
        G = groups(P)
        for case in DECODE_CASES:
            out = layered_reference(tmp, shape, P, case)
            assert np.isfinite(out[4]).all(), (shape, P, case)
            if case[2] == 0:  # the posterior is the channel LLR ln 49, inside: no row converges
                assert ((out[2] & 12) == 12).all() and (out[3] == 0).all(), (shape, P, case)
        for case in PRIOR_CASES:
            assert np.isfinite(layered_reference(tmp, shape, P, case, "table", "random")[4]).all(), (shape, P, case)
        syn = layered_reference(tmp, shape, P, SYN20)[3]
        for sec, seen in enumerate(count_sets(syn)):
            if len(seen) < 2:
                one.add((shape, P, sec))
        if G > 1:
            for sec, mixes in enumerate(wave_mixes(syn, G)):
                if not mixes:
                    nomix.add((shape, P, sec))
        if same_floats(layered_reference(tmp, shape, P, ("fixed", 0.03, 2))[4], flooding_reference(tmp, shape, P, ("fixed", 0.03, 2))[4]):
            same.add((shape, P))
    assert one == {k for k in ONE_COUNT if k[0] == shape}, sorted(one)
    assert nomix == {k for k in NO_WAVE_MIX if k[0] == shape}, sorted(nomix)
    assert same == {k for k in SAME_AS_FLOODING if k[0] == shape}, sorted(same)


def test_the_pinned_exceptions_are_few():
    assert all(s in TABLE_SHAPES and P in PS for s, P, _ in list(ONE_COUNT) + list(NO_WAVE_MIX))
    assert len(set(ONE_COUNT) | set(NO_WAVE_MIX)) <= 16  # of the 160 (code, sector) rows


# ---- non-vacuity --------------------------------------------------------------------------------------------------------
def iteration_sets(name, stop, p, N=20):
    it = layered_cpu(code_of(name, routes(name)[0])).decode_batch(*inputs(name), p, N, stop, want_iters=True)[3]
    return [set(int(x) for x in it[:, sec]) for sec in (0, 1)]


# codes that miss a property of test_not_vacuous, as observed: name -> the properties missed
NOT_VACUOUS_EXCEPTIONS = {}


def test_not_vacuous():
    """On the CPU engine, cap 20, the properties of test_serial.test_not_vacuous: under the syndrome stop every code has
    a sector with a row that stops at 1 and a sector with a row that runs to the cap, and some code ends a sector
    strictly between; under the reference stop at MS_P_REF every code has sectors ending at its first test, and some
    run to the cap; every flag bit and the clean flag word occur."""
    between, ref_cap, flags = [], [], []
    for name in SMALL:
        missed = set()
        seen = iteration_sets(name, "syndrome", MS_P[name])
        if not any(1 in s for s in seen):
            missed.add("syndrome-1")
        if not any(20 in s for s in seen):
            missed.add("syndrome-cap")
        between.append(any(1 < k < 20 for s in seen for k in s))
        ref = iteration_sets(name, "ref", MS_P_REF)
        if not any(1 in s for s in ref):
            missed.add("ref-1")
        ref_cap.append(any(20 in s for s in ref))
        assert missed == NOT_VACUOUS_EXCEPTIONS.get(name, set()), (name, seen, ref)
        for stop, p in (("syndrome", MS_P[name]), ("ref", MS_P_REF)):
            flags.append(layered_cpu(code_of(name, routes(name)[0])).decode_batch(*inputs(name), p, 20, stop)[2])
    assert any(between) and any(ref_cap)
    flags = np.concatenate(flags)
    assert (flags == 0).any()
    for bit in (q.SYNDROME_FAIL_X, q.SYNDROME_FAIL_Z, q.CONVERGENCE_FAIL_X, q.CONVERGENCE_FAIL_Z):
        assert (flags & bit).any(), bit


# ---- consequences -------------------------------------------------------------------------------------------------------
def test_layered_is_a_different_decode_and_option_0_restores_flooding():
    name = "hgp_ham"
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    row = int(np.nonzero(sX.any(axis=1) & sZ.any(axis=1))[0][0])  # a non-zero syndrome in both sectors
    dec, fresh = minsum_cpu(code), minsum_cpu(code)
    assert dec.get_option("minsum_schedule") == 0
    flood = fresh.decode_batch(sX, sZ, 0.05, 2, "fixed", want_iters=True, want_q=True)
    dec.set_option("minsum_schedule", 1)
    assert dec.get_option("minsum_schedule") == 1
    layered = dec.decode_batch(sX, sZ, 0.05, 2, "fixed", want_iters=True, want_q=True)
    assert dec.last_path() == {"minsum", "serial"}
    EX = code.numEqsX * code.stride
    assert not same_floats(layered[4][row, :EX], flood[4][row, :EX]) and not same_floats(layered[4][row, EX:], flood[4][row, EX:])
    dec.set_option("minsum_schedule", 0)
    for N, stop in ((2, "fixed"), (20, "syndrome"), (20, "ref")):
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert dec.last_path() == {"minsum"}
        assert_same_decode(got, fresh.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True), "option 0 again")


def test_the_product_rule_ignores_the_option():
    name = "mid"
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    dec, fresh = q.DecoderCPU(code), q.DecoderCPU(code)
    dec.set_option("minsum_schedule", 1)
    got = dec.decode_batch(sX, sZ, 0.05, 11, "fixed", want_iters=True, want_q=True)
    assert dec.last_path() == set()
    assert_same_decode(got, fresh.decode_batch(sX, sZ, 0.05, 11, "fixed", want_iters=True, want_q=True), "product rule")


def test_a_relay_ignores_the_option():
    """One leg with gamma = 0 is plain flooding min-sum bit for bit, and stays so with the option at 1."""
    name = "r3-3-6-13"
    code = code_of(name, "graph")
    sX, sZ = inputs(name)
    zero = np.zeros((1, code.n), dtype=F32)
    plain = minsum_cpu(code)
    dec = minsum_cpu(code)
    dec.set_relay(zero, zero)
    dec.set_option("minsum_schedule", 1)
    for stop, N in (("fixed", 11), ("syndrome", 20)):
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert dec.last_path() == {"minsum", "relay"}
        assert_same_decode(got, plain.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True), stop)
    layered = layered_cpu(code).decode_batch(sX, sZ, 0.05, 11, "fixed", want_q=True)
    assert not same_floats(layered[4], plain.decode_batch(sX, sZ, 0.05, 11, "fixed", want_q=True)[4])


def test_unused_slots_and_degree_zero_variables():
    """tall: qubits 0, 1 and 2 are in no X check and decide 0; unused slots of q_final hold +0.0f; every real slot
    of a variable holds the same value."""
    HX, HZ = matrices("tall")
    sX, sZ = inputs("tall")
    eX, _, _, _, qf = layered_cpu(code_of("tall", "general")).decode_batch(sX, sZ, 0.05, 11, "fixed", want_q=True)
    assert not eX[:, :3].any()
    D = 7
    qx = qf[:, :HX.shape[0] * D].reshape(len(sX), HX.shape[0], D)
    for c in range(HX.shape[0]):
        w = int(HX[c].sum())
        assert (qx[:, c, w:].view(np.uint32) == 0).all()
    v = int(np.nonzero(HX.sum(axis=0) > 1)[0][0])
    slots = [(c, int(np.nonzero(np.nonzero(HX[c])[0] == v)[0][0])) for c in np.nonzero(HX[:, v])[0]]
    vals = np.stack([qx[:, c, k] for c, k in slots])
    assert same_floats(vals[0], vals[1])


def test_n_zero_gives_the_channel_llr():
    name = "mid"
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    lam = F32(q.minsum_llr(F32(2.0) / F32(3.0) * F32(0.05)))
    out = layered_cpu(code).decode_batch(sX, sZ, 0.05, 0, "syndrome", want_iters=True, want_q=True)
    assert (out[3] == 0).all() and not out[0].any() and not out[1].any()
    assert set(int(x) for x in out[4].view(U32).ravel()) == {0, int(np.array([lam]).view(U32)[0])}
    assert ((out[2] & 12) == 12).all()  # ln(0.9667 / 0.0333) = 3.37 is inside


def test_near_hard_option_changes_nothing():
    code = code_of("r3-3-6-13", "graph")
    sX, sZ = inputs("r3-3-6-13")
    a, b = layered_cpu(code), layered_cpu(code)
    b.set_option("near_hard", 0)
    for stop in ("fixed", "ref"):
        assert_same_decode(a.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True),
                           b.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True), stop, with_q=False)
        assert_same_decode(a.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True),
                           yard("r3-3-6-13", "scalar", stop, 20, 160, 0.005), stop, with_q=False)


# ---- the option -----------------------------------------------------------------------------------------------------------
def test_option_values_and_refusals():
    code = code_of("hgp_ham", "general")
    dec = q.DecoderCPU(code)
    assert q.OPTION["minsum_schedule"] == 23 and q.lib().qec_abi_version() == 4
    assert q.PATH["serial"] == 1024 and q.PATH["minsum"] == 2048
    assert dec.get_option("minsum_schedule") == 0
    for bad in (2, -1):
        with pytest.raises(q.QecError, match="QEC_OPT_MINSUM_SCHEDULE"):
            dec.set_option("minsum_schedule", bad)
        assert q.lib().qec_decoder_set_option(dec._h, 23, bad) == -1  # QEC_ERR_ARG
        assert dec.get_option("minsum_schedule") == 0
    # the option is data: it is accepted whatever the other options say, and they refuse each other as before
    dec.set_option("minsum_schedule", 1)
    dec.set_option("bp_schedule", 1)
    with pytest.raises(q.QecError, match="QEC_OPT_BP_SCHEDULE"):
        dec.set_option("bp_method", 1)
    assert dec.get_option("bp_method") == 0 and dec.get_option("bp_schedule") == 1 and dec.get_option("minsum_schedule") == 1
    dec.set_option("bp_schedule", 0)
    dec.set_option("bp_method", 1)
    for other, value in (("correlated", 1), ("correlated", 2), ("bp_schedule", 1)):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
            dec.set_option(other, value)
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION[other], value) == -4  # QEC_ERR_UNSUPPORTED
        assert dec.get_option(other) == 0
    sX, sZ = inputs("hgp_ham")
    assert_same_decode(dec.decode_batch(sX, sZ, 0.05, 5, "fixed", want_iters=True, want_q=True),
                       layered_cpu(code).decode_batch(sX, sZ, 0.05, 5, "fixed", want_iters=True, want_q=True), "after refusals")


# ---- the LAYERED kernels of bp_sparse.hip, restated ------------------------------------------------------------------------
# sparse_kernels / sparse_plan_create: the shape and the workspace are the scalar plan's (plan_of), priors are a runtime
# branch of the one kernel, and the route chooses regular or general: 2 x 3 shapes x LDS / HBM x 3 stops
LAYERED_INSTANCES = {(k, s, mem, stop) for k in KERNELS for s in SHAPES for mem in ("lds", "hbm") for stop in STOPS}
GPU_CASES = CASES  # the case table of tests/test_gpu_minsum_layered.py: every row, scalar p and priors, every stop rule


def instance_of(code, general, stop):
    p = plan_of(code, general)
    return (p["kernel"], p["shape"], p["mem"], stop)


def test_gpu_case_table_reaches_every_layered_instantiation():
    reached = {instance_of(code_of(name, route), route == "general", stop) for name, route in GPU_CASES for stop in STOPS}
    assert len(LAYERED_INSTANCES) == 36
    assert reached == LAYERED_INSTANCES, sorted(LAYERED_INSTANCES - reached)
    lds = {instance_of(code_of(name, route), route == "general", stop) for name, route in LDS_CASES for stop in STOPS}
    assert lds == {i for i in LAYERED_INSTANCES if i[2] == "lds"} and len(lds) == 18


# ---- the benefit on P61 -----------------------------------------------------------------------------------------------------
BENEFIT_SEED, BENEFIT_B, BENEFIT_P = 0x51EC0DE, 1024, 0.05


def test_layered_needs_fewer_iterations_on_p61():
    """1024 depolarising samples of the project's sampler at p = 0.05, syndrome stop, cap 20, scale 160: layered
    iterations summed over both sectors are at most 0.70 of flooding's, and layered leaves no more sectors unsatisfied."""
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P61))
    HX, HZ = code.pcm(0), code.pcm(1)
    x, z = depolarizing(BENEFIT_SEED, 0, BENEFIT_B, code.n, BENEFIT_P)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    flood = minsum_cpu(code).decode_batch(sX, sZ, BENEFIT_P, 20, "syndrome", want_iters=True)
    layered = layered_cpu(code).decode_batch(sX, sZ, BENEFIT_P, 20, "syndrome", want_iters=True)
    itf, itl = int(flood[3].sum()), int(layered[3].sum())
    bad = [int(((o[2] & 1) != 0).sum() + ((o[2] & 2) != 0).sum()) for o in (flood, layered)]
    print("P61 p=%g: iterations flooding %d, layered %d (ratio %.3f); sectors left unsatisfied flooding %d, layered %d"
          % (BENEFIT_P, itf, itl, itl / itf, bad[0], bad[1]))
    assert itl <= 0.70 * itf, (itl, itf)
    assert bad[1] <= bad[0], bad


# ---- OSD --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0, 10])
def test_osd_soft_decode_is_layered(lam):
    """osd = 1 under the option: no syndrome failure remains, and the result is dec.osd fed with the q_final of a
    layered fixed-stop decode of osd_iterations iterations."""
    HX, HZ = code_matrices("hgp_ham")
    p = 0.05
    x, z = depolarizing(BENEFIT_SEED, 0, 512, HX.shape[1], p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    code = general_code("hgp_ham")
    dec = layered_cpu(code)
    dec.set_option("osd_order", lam)
    main = dec.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    failed = int(((main[2] & 1) != 0).sum() + ((main[2] & 2) != 0).sum())
    assert failed >= 10
    K = dec.get_option("osd_iterations")
    soft = dec.decode_batch(sX, sZ, p, K, "fixed", want_q=True)[4]
    flood_soft = minsum_cpu(code).decode_batch(sX, sZ, p, K, "fixed", want_q=True)[4]
    assert not same_floats(soft, flood_soft)
    want = dec.osd(sX, sZ, soft, main[0], main[1], main[2])
    dec.set_option("osd", 1)
    got = dec.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    assert dec.last_path() == {"minsum", "serial", "osd"}
    for a, b in zip(got[:3], want):
        assert np.array_equal(a, b)
    assert np.array_equal(got[3], main[3])
    assert not (got[2] & 3).any() and dec.get_option("osd_sectors") == failed
    assert np.array_equal((got[0] @ HX.T) & 1, sX) and np.array_equal((got[1] @ HZ.T) & 1, sZ)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_minsum_schedule_on_the_cpu_engine(tmp_path):
    """--minsum-schedule serial reproduces the Python counters of GetStatistics under the option at 1, flooding those at
    0; other values exit 2, and so does the flag without --bp-method minsum, before a decoder is made."""
    from qec_ldpc_amd.codes import write_css_file
    from test_osd_host import _cli, _fields
    HX, HZ = code_matrices("hgp_ham")
    path = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    code = q.Quantum_LDPC_Code.createFromFile(path).with_logical("degenerate")
    W, B, N, p, seed = 4, 1500, 20, 0.05, 7
    base = ["--engine", "cpu", "--seed", str(seed), "--logical", "degenerate", "--bp-method", "minsum"]
    keys = {"Corrected": "corrected", "Syndrome Errors X": "syndromeErrorsX", "Syndrome Errors Z": "syndromeErrorsZ",
            "Logical Errors": "logicalErrors", "Convergence Fail X": "convergenceFailX",
            "Convergence Fail Z": "convergenceFailZ", "Errors Tested": "numErrorsTested"}
    out = {}
    for sched, value in (("flooding", 0), ("serial", 1)):
        d = tmp_path / sched
        d.mkdir()
        r = _cli(d, base + ["--minsum-schedule", sched], path, "%d %d %d %d %g" % (W, W, B, N, p))
        assert r.returncode == 0, r.stderr
        f = _fields(d)
        dec = minsum_cpu(code)
        dec.set_option("minsum_schedule", value)
        tested = int(f["Errors Tested"])  # the CLI tests (B / threads) * threads samples, the first ones of the stream
        assert B // 2 < tested <= B
        st = dec.GetStatistics(W, tested, p, N, seed=seed)
        out[sched] = {k: int(f[k]) for k in keys}
        assert out[sched] == {k: st[v] for k, v in keys.items()}, sched
    assert out["serial"] != out["flooding"]
    bad = (["--engine", "cpu", "--minsum-schedule", "serial"], ["--engine", "cpu", "--minsum-schedule", "flooding"],
           ["--minsum-schedule", "serial"], ["--engine", "cpu", "--bp-method", "minsum", "--minsum-schedule", "layered"],
           ["--engine", "cpu", "--bp-method", "product", "--minsum-schedule", "serial"])
    for k, flags in enumerate(bad):
        d = tmp_path / ("bad%d" % k)
        d.mkdir()
        r = _cli(d, flags, path, "4 4 10 20 0.05")
        assert r.returncode == 2 and "minsum-schedule" in r.stderr, (flags, r.stderr)

"""Noisy syndromes in min-sum BP (set_syndrome_priors) on the device, the sparse-graph kernels: every row of the case
table of tests/test_sparse_shapes.py -- so every MINSUM and LAYERED shape of bp_sparse.hip runs its SOFT instantiation,
LDS and HBM, regular and general -- against the CPU engine with the same syndrome priors, which
tests/test_soft_syndrome.py holds to the numpy yardstick: the three stop rules, scalar p and data priors, with and
without q_final, with and without f, B = 1 and a batch that is no multiple of anything.  Then decode_batch_soft_dev in a
captured graph replayed after a second set_syndrome_priors, flip_syndrome_dev against numpy (a shard taken alone too),
the Monte-Carlo counters against a count by hand, the path, the refusals of a wave-circulant handle and a two-part group.

Bit for bit everywhere: eX, eZ, fX, fZ, flags, iteration counts and q_final as uint32 patterns."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.codes import P7, code_path
from test_general_code import assert_same_decode, same_floats
from test_gpu_general_code import count
from test_minsum import MS_P, MS_P_REF
from test_priors import prior_vectors
from test_soft_syndrome import (SCHEDULES, assert_same_soft, flip_reference, flipped, soft_cpu, soft_decode, soft_inputs,
                                syndrome_priors)
from test_sparse_shapes import (HBM_CASES, LDS_CASES, P_MAIN, P_REF, case_id, code_of, hbm_inputs, hbm_priors)

pytestmark = pytest.mark.gpu

_decoders = {}


def soft_gpu(code, qX, qZ, schedule="flooding", **kw):
    dec = q.DecoderGPU(code, 0, engine="sparse", **kw)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_schedule", SCHEDULES.index(schedule))
    dec.set_syndrome_priors(qX, qZ)
    return dec


def gpu(case, qX, qZ):
    """One sparse-engine decoder per row of the case table (a test that changes an option or sets priors puts it back)."""
    if case not in _decoders:
        _decoders[case] = soft_gpu(code_of(*case), qX, qZ)
        assert _decoders[case].describe().endswith("[soft syndrome]")
    return _decoders[case]


def decode(dec, sX, sZ, p, N, stop, want_q=True, layered=False):
    got = soft_decode(dec, sX, sZ, p, N, stop, want_q)
    assert {"minsum", "soft", "sparse"} <= dec.last_path() and "wave" not in dec.last_path()
    assert ("serial" in dec.last_path()) == layered
    assert dec.get_option("last_path") & q.PATH["soft"] == 16384
    return got


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("kind", ["scalar", "random"])
@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
def test_lds_matches_the_cpu_engine(case, kind, schedule):
    name, _ = case
    sX, sZ, qX, qZ = soft_inputs(name)
    dec = gpu(case, qX, qZ)
    pri = None if kind == "scalar" else prior_vectors(code_of(*case).n, kind)
    cpu = soft_cpu(code_of(*case), qX, qZ, 160, pri, schedule)
    layered = schedule == "layered"
    p0 = MS_P[name]
    runs = (("fixed", p0, 0), ("fixed", p0, 1), ("fixed", p0, 11), ("syndrome", p0, 20), ("ref", p0, 11), ("ref", MS_P_REF, 20))
    B = len(sX)
    assert B == 51  # 3 x 17: no multiple of a wave, a workgroup or a power of two
    try:
        dec.set_option("minsum_schedule", int(layered))
        if pri:
            dec.set_priors(*pri)
        for stop, p, N in runs:
            want = soft_decode(cpu, sX, sZ, p, N, stop)
            what = "%s %s %s %s p=%g N=%d" % (case_id(case), kind, schedule, stop, p, N)
            assert_same_soft(decode(dec, sX, sZ, p, N, stop, True, layered), want, what)
            if N in (0, 20):
                assert_same_soft(decode(dec, sX, sZ, p, N, stop, False, layered), want, what + " no q", with_q=False)
                plain = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)  # without f
                assert_same_decode(plain, want, what + " no f")
                one = decode(dec, sX[7:8], sZ[7:8], p, N, stop, True, layered)
                assert_same_soft(one, tuple(a[7:8] for a in want), what + " B = 1")
    finally:
        dec.set_priors(None, None)
        dec.set_option("minsum_schedule", 0)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
def test_hbm_matches_the_cpu_engine(case, priors, schedule):
    name, _ = case
    code = code_of(*case)
    qX, qZ = syndrome_priors(code.numEqsX, 51), syndrome_priors(code.numEqsZ, 52)
    hX, hZ = hbm_inputs(name)
    sX, sZ = flipped(hX, qX, 61, keep=3), flipped(hZ, qZ, 62, keep=3)
    dec = gpu(case, qX, qZ)
    pri = hbm_priors(name) if priors else None
    cpu = soft_cpu(code, qX, qZ, 160, pri, schedule)
    layered = schedule == "layered"
    try:
        dec.set_option("minsum_schedule", int(layered))
        if pri:
            dec.set_priors(*pri)
        for stop, p, N in (("ref", P_REF, 11), ("fixed", P_MAIN, 3), ("syndrome", P_MAIN, 6)):
            want = soft_decode(cpu, sX, sZ, p, N, stop)
            what = "%s priors=%s %s %s" % (name, priors, schedule, stop)
            assert_same_soft(decode(dec, sX, sZ, p, N, stop, True, layered), want, what)
            assert_same_soft(decode(dec, sX, sZ, p, N, stop, False, layered), want, what + " no q", with_q=False)
        plain = dec.decode_batch(sX, sZ, P_MAIN, 6, "syndrome", want_iters=True, want_q=True)
        assert_same_decode(plain, want, "%s no f" % name)
    finally:
        dec.set_priors(None, None)
        dec.set_option("minsum_schedule", 0)


def test_q_zero_and_cleared_priors_equal_the_plain_kernels():
    case = ("r4-5-10-7", "graph")
    code = code_of(*case)
    sX, sZ, qX, qZ = soft_inputs(case[0])
    dec = soft_gpu(code, 0.0, 0.0)
    plain = q.DecoderGPU(code, 0, engine="sparse")
    plain.set_option("bp_method", 1)
    for sched in (0, 1):
        dec.set_option("minsum_schedule", sched)
        plain.set_option("minsum_schedule", sched)
        for stop, N in (("fixed", 11), ("syndrome", 20), ("ref", 20), ("fixed", 0)):
            want = plain.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
            assert "soft" not in plain.last_path()
            got = soft_decode(dec, sX, sZ, 0.05, N, stop)
            assert "soft" in dec.last_path()
            assert_same_decode(got, want, "q = 0 %s N=%d" % (stop, N))
            assert not got[5].any() and not got[6].any()
            none = soft_decode(plain, sX, sZ, 0.05, N, stop)  # the soft call without syndrome priors: f = 0
            assert_same_decode(none, want, "no priors")
            assert not none[5].any() and not none[6].any()
    dec.set_syndrome_priors(qX, qZ)
    assert soft_decode(dec, sX, sZ, 0.05, 20, "syndrome")[5].any()
    dec.set_syndrome_priors(None, None)
    got = dec.decode_batch(sX, sZ, 0.05, 11, "fixed", want_iters=True, want_q=True)
    assert "soft" not in dec.last_path() and "soft" not in dec.describe()
    assert_same_decode(got, plain.decode_batch(sX, sZ, 0.05, 11, "fixed", want_iters=True, want_q=True), "cleared")


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_soft_dev_decode_in_a_captured_graph_reads_new_syndrome_priors(schedule):
    """decode_batch_soft_dev allocates nothing: the replay equals the direct call, and a replay after a second
    set_syndrome_priors decodes with the new values (the table is rewritten in place)."""
    import torch
    name = "r3-3-6-13"
    code = code_of(name, "graph")
    sX, sZ, qX, qZ = soft_inputs(name)
    B = len(sX)
    first, second = (qX, qZ), (syndrome_priors(code.numEqsX, 91), syndrome_priors(code.numEqsZ, 92))
    dec = soft_gpu(code, *first, schedule=schedule, max_batch=B)  # the first set allocates the device table
    dev = torch.device("cuda", 0)
    u8 = torch.uint8
    tX, tZ = torch.from_numpy(np.array(sX)).to(dev), torch.from_numpy(np.array(sZ)).to(dev)
    eX, eZ = torch.zeros((B, code.n), dtype=u8, device=dev), torch.zeros((B, code.n), dtype=u8, device=dev)
    fX = torch.zeros((B, code.numEqsX), dtype=u8, device=dev)
    fZ = torch.zeros((B, code.numEqsZ), dtype=u8, device=dev)
    fl = torch.zeros((B,), dtype=u8, device=dev)
    it = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    qf = torch.zeros((B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    outs = (eX, eZ, fl, it, qf, fX, fZ)

    def call(stream=None):
        dec.decode_batch_soft_dev(tX, tZ, 0.05, 20, "syndrome", eX, eZ, fl, fX=fX, fZ=fZ, iters=it, q=qf, stream=stream)

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(s)
    assert {"minsum", "soft", "sparse"} <= dec.last_path()

    def run(f):
        for t in outs:
            t.fill_(7)
        f()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    wants = []
    for pri in (first, second):
        dec.set_syndrome_priors(*pri)
        wants.append(run(call))
        assert_same_soft(run(g.replay), wants[-1], "replay")
        host = soft_decode(soft_cpu(code, pri[0], pri[1], 160, None, schedule), sX, sZ, 0.05, 20, "syndrome")
        assert_same_soft(wants[-1], host, "against the CPU engine")
    assert not np.array_equal(wants[0][5], wants[1][5]) or not same_floats(wants[0][4], wants[1][4])


def test_flip_syndrome_dev_against_numpy():
    import torch
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P7))
    mX, mZ = code.numEqsX, code.numEqsZ
    qX, qZ = syndrome_priors(mX, 1), syndrome_priors(mZ, 2)
    qX[0], qX[1], qZ[0], qZ[1] = 0.0, 1.0, 1.0, 0.0
    dec = soft_gpu(code, qX, qZ)
    dev = torch.device("cuda", 0)
    seed, start, B = 0xC0FFEE1234, (1 << 32) - 100, 1003  # the sample index crosses 2^32
    rng = np.random.default_rng(3)
    sX = rng.integers(0, 2, (B, mX), dtype=np.uint8)
    sZ = rng.integers(0, 2, (B, mZ), dtype=np.uint8)
    wX, wZ = flip_reference(seed, start, B, qX, qZ)
    assert wX.any() and wZ.any() and not wX[:, 0].any() and wX[:, 1].all()
    tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
    fX, fZ = torch.zeros_like(tX), torch.zeros_like(tZ)
    dec.flip_syndrome_dev(seed, start, tX, tZ, fX, fZ)
    torch.cuda.synchronize()
    assert np.array_equal(fX.cpu().numpy(), wX) and np.array_equal(fZ.cpu().numpy(), wZ)
    assert np.array_equal(tX.cpu().numpy(), sX ^ wX) and np.array_equal(tZ.cpu().numpy(), sZ ^ wZ)
    # a shard taken alone, without the flip outputs
    lo, k = 401, 77
    aX, aZ = torch.from_numpy(sX[lo:lo + k].copy()).to(dev), torch.from_numpy(sZ[lo:lo + k].copy()).to(dev)
    dec.flip_syndrome_dev(seed, start + lo, aX, aZ)
    torch.cuda.synchronize()
    assert np.array_equal(aX.cpu().numpy(), (sX ^ wX)[lo:lo + k]) and np.array_equal(aZ.cpu().numpy(), (sZ ^ wZ)[lo:lo + k])
    # sample_syndrome_dev applies the same flips behind the syndrome, errp stays the data error
    p = 0.02
    x, z = depolarizing(seed, start, B, code.n, p)
    bX, bZ = torch.zeros_like(tX), torch.zeros_like(tZ)
    errp = torch.zeros((B, 2 * ((code.n + 7) // 8)), dtype=torch.uint8, device=dev)
    dec.sample_syndrome_dev(seed, start, p, bX, bZ, errp)
    torch.cuda.synchronize()
    assert np.array_equal(bX.cpu().numpy(), code.syndrome(0, x) ^ wX) and np.array_equal(bZ.cpu().numpy(), code.syndrome(1, z) ^ wZ)
    nb = (code.n + 7) // 8
    assert np.array_equal(errp.cpu().numpy()[:, :nb], np.packbits(x, axis=1, bitorder="little"))
    # without syndrome priors the call is refused
    dec.set_syndrome_priors(None, None)
    with pytest.raises(q.QecError, match="no syndrome priors"):
        dec.flip_syndrome_dev(seed, start, tX, tZ)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_monte_carlo_counters(schedule):
    """P7, 2^12 samples, syndrome stop: monte_carlo's counters equal counting the same samples by hand through
    sample_syndrome_dev + decode + statistics_dev on the device, and through the CPU engine on the host."""
    import torch
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P7))
    mX, mZ, n = code.numEqsX, code.numEqsZ, code.n
    qX, qZ = syndrome_priors(mX, 5), syndrome_priors(mZ, 6)
    dec = soft_gpu(code, qX, qZ, schedule)
    seed, B, p, N = 11, 4096, 0.02, 20
    got = dec.monte_carlo(seed, 0, B, p, N, "syndrome", batch=1024)
    assert {"minsum", "soft", "sparse"} <= dec.last_path()
    # by hand on the host: the sampler's errors, their syndromes through the channel, the CPU engine, the counters
    x, z = depolarizing(seed, 0, B, n, p)
    wX, wZ = flip_reference(seed, 0, B, qX, qZ)
    sX, sZ = code.syndrome(0, x) ^ wX, code.syndrome(1, z) ^ wZ
    cpu = soft_cpu(code, qX, qZ, 160, None, schedule)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    assert {k: got[k] for k in want} == want
    assert want["synX"] + want["synZ"] > 0 and want["corrected"] > 0
    # by hand on the device
    dev = torch.device("cuda", 0)
    u8 = torch.uint8
    tX, tZ = torch.zeros((B, mX), dtype=u8, device=dev), torch.zeros((B, mZ), dtype=u8, device=dev)
    dec.sample_syndrome_dev(seed, 0, p, tX, tZ)
    dX, dZ = torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev)
    oX, oZ = torch.zeros((B, n), dtype=u8, device=dev), torch.zeros((B, n), dtype=u8, device=dev)
    ofl = torch.zeros((B,), dtype=u8, device=dev)
    dec.decode_batch_dev(tX, tZ, p, N, "syndrome", oX, oZ, ofl)
    cnt = torch.zeros(len(q.MC_COUNTERS), dtype=torch.int64, device=dev)
    dec.statistics_dev(dX, dZ, oX, oZ, ofl, cnt)
    torch.cuda.synchronize()
    hand = dict(zip(q.MC_COUNTERS, (int(v) for v in cnt.cpu().numpy())))
    assert hand == {k: want[k] for k in q.MC_COUNTERS}
    # the decode that ignores the noise fails more syndromes on the same samples
    blind = q.DecoderGPU(code, 0, engine="sparse")
    blind.set_option("bp_method", 1)
    blind.set_option("minsum_schedule", SCHEDULES.index(schedule))
    bfl = blind.decode_batch(sX, sZ, p, N, "syndrome")[2]
    assert int(((bfl & 3) != 0).sum()) > int(((fl & 3) != 0).sum())


def test_refusals_on_the_device():
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P7))
    wave = q.DecoderGPU(code, 0)  # engine auto: the wave-circulant engine, which refuses min-sum
    before = wave.describe()
    rc = q.lib().qec_decoder_set_syndrome_priors(wave._h, q._ptr(np.full(code.numEqsX, 0.1, np.float32)),
                                                 q._ptr(np.full(code.numEqsZ, 0.1, np.float32)))
    assert rc == -4 and "QEC_ENGINE_SPARSE" in q.last_error()  # QEC_ERR_UNSUPPORTED
    assert wave.get_syndrome_priors() is None and wave.describe() == before
    sp = q.DecoderGPU(code, 0, engine="sparse")
    with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
        sp.set_syndrome_priors(0.1, 0.1)
    sp.set_option("bp_method", 1)
    sp.set_syndrome_priors(0.1, 0.1)
    gam = q.relay_gammas(code.n, 2)
    for f, args in ((sp.set_option, ("bp_method", 0)), (sp.set_option, ("osd", 1)), (sp.set_relay, (gam, gam))):
        with pytest.raises(q.QecError, match="syndrome priors"):
            f(*args)
    assert sp.get_option("bp_method") == 1 and sp.get_option("osd") == 0 and sp.get_relay() is None
    sp.set_syndrome_priors(None, None)
    sp.set_relay(gam, gam)
    with pytest.raises(q.QecError, match="relay"):
        sp.set_syndrome_priors(0.1, 0.1)
    sp.set_relay(None, None)
    sp.set_option("osd", 1)
    with pytest.raises(q.QecError, match="OSD"):
        sp.set_syndrome_priors(0.1, 0.1)
    assert sp.get_syndrome_priors() is None


def test_a_two_part_group_decodes_like_one_part():
    name = "mid"
    code = code_of(name, "general")
    sX, sZ, qX, qZ = soft_inputs(name)
    two = q.DecoderGPU(code, devices=[0, 0])
    two.set_option("bp_method", 1)
    two.set_syndrome_priors(qX, qZ)
    assert all(p.get_syndrome_priors() is not None for p in two.parts()) and two.get_syndrome_priors() is not None
    for schedule in SCHEDULES:
        two.set_option("minsum_schedule", SCHEDULES.index(schedule))
        cpu = soft_cpu(code, qX, qZ, 160, None, schedule)
        for stop, N in (("fixed", 5), ("syndrome", 20)):
            got = soft_decode(two, sX, sZ, 0.05, N, stop)
            assert {"minsum", "soft"} <= two.last_path()
            assert_same_soft(got, soft_decode(cpu, sX, sZ, 0.05, N, stop), "group %s %s" % (schedule, stop))
    two.set_syndrome_priors(None, None)
    assert all(p.get_syndrome_priors() is None for p in two.parts())

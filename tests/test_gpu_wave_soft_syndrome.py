"""Noisy syndromes in min-sum BP (set_syndrome_priors) on the device, the register-resident wave kernels
(set_option("minsum_wave", 1) on a sparse-engine handle; the SOFT kernels of bp_wave_minsum.hip): the case table of
tests/test_circulant_shapes.py -- eight block shapes x ten P, so each of the 48 SOFT kernels runs at every group count
G = 64 // P and every idle-lane count of the table -- against the CPU engine's outputs that tests/test_soft_syndrome.py
computes, holds to numpy and checks for non-vacuity (groups of one wave that stop at different iterations among them):
flooding and layered, the "table" and "waves" batches, the ragged prefix and B = 1, scalar p and data priors, the three
stop rules, with and without q_final and f.  Then minsum_wave = 0 on the same handle, the shipped codes, the soft _dev
call in a captured graph, the Monte-Carlo counters and a two-part group.

These are the smallest shapes at which the lane <-> check index of mu, the group freeze of f and a ragged last wave can
go wrong.  Bit for bit everywhere: eX, eZ, fX, fZ, flags, iteration counts and q_final as uint32 patterns."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.codes import P7, P61, code_path
from test_circulant_shapes import KINDS, PS, SHAPES, batch, code_of, groups, ragged, shape_id
from test_general_code import assert_same_decode, same_floats
from test_gpu_general_code import count
from test_soft_syndrome import (SCHEDULES, assert_same_soft, flip_reference, flipped, soft_cpu, soft_decode,
                                syndrome_priors, table_inputs, table_reference)
from test_wave_minsum import DECODE_CASES, PRIOR_CASES

pytestmark = pytest.mark.gpu

_decoders = {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_wave_soft_syndrome")


def wave_decoder(code, qX, qZ, schedule="flooding", **kw):
    dec = q.DecoderGPU(code, 0, engine="sparse", **kw)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", 1)
    dec.set_option("minsum_schedule", SCHEDULES.index(schedule))
    dec.set_syndrome_priors(qX, qZ)
    return dec


def gpu(tmp, shape, P, schedule):
    """One sparse-engine decoder per row of the table and schedule, with the wave kernels and the row's syndrome priors
    (a test that changes an option or sets priors puts it back)."""
    key = (shape, P, schedule)
    if key not in _decoders:
        _, _, qX, qZ = table_inputs(tmp, shape, P)
        _decoders[key] = wave_decoder(code_of(tmp, shape, P)[0], qX, qZ, schedule)
    return _decoders[key]


def decode(dec, sX, sZ, case, schedule, want_q=True):
    stop, p, N = case
    got = soft_decode(dec, sX, sZ, p, N, stop, want_q)
    assert {"minsum", "soft", "wave", "sparse"} <= dec.last_path()
    assert ("serial" in dec.last_path()) == (schedule == "layered")
    return got


def rows(ref, k):
    return tuple(a[:k] for a in ref)


def label(shape, P, kind, schedule, case, what):
    return "%s P=%d %s %s %s p=%g N=%d %s" % ((shape_id(shape), P, kind, schedule) + case + (what,))


# ---- 1. the table, scalar p ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_table_scalar(tmp, shape, schedule):
    for P in PS:
        dec = gpu(tmp, shape, P, schedule)
        assert "P=%d G=%d" % (P, groups(P)) in dec.describe() and dec.describe().endswith("[soft syndrome]"), dec.describe()
        for kind in KINDS:
            sX, sZ, _, _ = table_inputs(tmp, shape, P, kind)
            for case in DECODE_CASES:
                want = table_reference(tmp, shape, P, case, kind, None, schedule)
                assert_same_soft(decode(dec, sX, sZ, case, schedule, True), want, label(shape, P, kind, schedule, case, "q, f"))
                assert_same_soft(decode(dec, sX, sZ, case, schedule, False), want,
                                 label(shape, P, kind, schedule, case, "f, no q"), with_q=False)
                stop, p, N = case  # the existing entry point: no f
                plain = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                assert_same_decode(plain, want, label(shape, P, kind, schedule, case, "q, no f"))
                if kind != "table":
                    continue
                k = ragged(P)
                if k != batch(P):  # G divides the batch: its first k rows leave a ragged wave
                    for want_q in (True, False):
                        assert_same_soft(decode(dec, sX[:k], sZ[:k], case, schedule, want_q), rows(want, k),
                                         label(shape, P, kind, schedule, case, "ragged, q %s" % want_q), with_q=want_q)
                assert_same_soft(decode(dec, sX[:1], sZ[:1], case, schedule, True), rows(want, 1),
                                 label(shape, P, kind, schedule, case, "B = 1"))


# ---- 2. the table, data priors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_table_priors(tmp, shape, schedule):
    from test_priors import prior_vectors
    for P in PS:
        dec = gpu(tmp, shape, P, schedule)
        n = code_of(tmp, shape, P)[0].n
        sX, sZ, _, _ = table_inputs(tmp, shape, P)
        try:
            dec.set_priors(*prior_vectors(n, "random"))
            for case in PRIOR_CASES:
                want = table_reference(tmp, shape, P, case, "table", "random", schedule)
                assert_same_soft(decode(dec, sX, sZ, case, schedule), want, label(shape, P, "random", schedule, case, "priors"))
        finally:
            dec.set_priors(None, None)
        assert not same_floats(table_reference(tmp, shape, P, PRIOR_CASES[0], "table", "random", schedule)[4],
                               table_reference(tmp, shape, P, ("fixed", 0.03, 11), "table", None, schedule)[4])


# ---- 3. minsum_wave = 0 on the same handle: the sparse SOFT kernels, the same bits --------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_minsum_wave_0_gives_the_same_bits(tmp, schedule):
    for shape, P in (((4, 4, 8), 22), ((2, 3, 6), 9), ((4, 6, 12), 64)):
        dec = gpu(tmp, shape, P, schedule)
        sX, sZ, _, _ = table_inputs(tmp, shape, P)
        try:
            dec.set_option("minsum_wave", 0)
            for case in (("syndrome", 0.03, 20), ("fixed", 0.03, 11), ("ref", 0.005, 21)):
                stop, p, N = case
                got = soft_decode(dec, sX, sZ, p, N, stop)
                assert {"minsum", "soft", "sparse"} <= dec.last_path() and "wave" not in dec.last_path()
                assert_same_soft(got, table_reference(tmp, shape, P, case, "table", None, schedule),
                                 label(shape, P, "table", schedule, case, "minsum_wave 0"))
        finally:
            dec.set_option("minsum_wave", 1)


def test_q_zero_equals_the_plain_wave_kernels(tmp):
    shape, P = (3, 4, 8), 21
    code = code_of(tmp, shape, P)[0]
    sX, sZ, _, _ = table_inputs(tmp, shape, P)
    soft = wave_decoder(code, 0.0, 0.0)
    plain = q.DecoderGPU(code, 0, engine="sparse")
    plain.set_option("bp_method", 1)
    plain.set_option("minsum_wave", 1)
    for sched in (0, 1):
        soft.set_option("minsum_schedule", sched)
        plain.set_option("minsum_schedule", sched)
        for stop, p, N in DECODE_CASES:
            want = plain.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            assert "soft" not in plain.last_path() and "wave" in plain.last_path()
            got = soft_decode(soft, sX, sZ, p, N, stop)
            assert {"soft", "wave"} <= soft.last_path()
            assert_same_decode(got, want, "q = 0 %s N=%d" % (stop, N))
            assert not got[5].any() and not got[6].any()
            none = soft_decode(plain, sX, sZ, p, N, stop)  # the soft call without syndrome priors: the plain kernels
            assert_same_decode(none, want, "no priors")
            assert not none[5].any() and not none[6].any()


# ---- 4. the shipped codes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", [P61, P7], ids=["P61", "P7"])
def test_shipped_codes(name, schedule):
    code = q.Quantum_LDPC_Code.createFromFile(code_path(name))
    qX, qZ = syndrome_priors(code.numEqsX, 71), syndrome_priors(code.numEqsZ, 72)
    dec, cpu = wave_decoder(code, qX, qZ, schedule), soft_cpu(code, qX, qZ, 160, None, schedule)
    x, z = depolarizing(0x51EC0DE, 0, 130, code.n, 0.02)
    sX, sZ = flipped(code.syndrome(0, x), qX, 73), flipped(code.syndrome(1, z), qZ, 74)
    for stop, N in (("syndrome", 20), ("fixed", 11), ("ref", 20)):
        want = soft_decode(cpu, sX, sZ, 0.02, N, stop)
        assert_same_soft(decode(dec, sX, sZ, (stop, 0.02, N), schedule), want, "%s %s %s" % (name, schedule, stop))


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_monte_carlo_counters_on_p7(schedule):
    """2^12 samples under the syndrome stop: the wave kernels' counters equal the sparse kernels' on the same handle and
    the count by hand through the CPU engine (the sampler's errors, their syndromes through the channel)."""
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P7))
    qX, qZ = syndrome_priors(code.numEqsX, 5), syndrome_priors(code.numEqsZ, 6)
    dec = wave_decoder(code, qX, qZ, schedule)
    seed, B, p, N = 11, 4096, 0.02, 20
    out = []
    for wave in (1, 0):
        dec.set_option("minsum_wave", wave)
        r = dec.monte_carlo(seed, 0, B, p, N, "syndrome", batch=1024)
        assert ("wave" in dec.last_path()) == bool(wave) and {"minsum", "soft", "sparse"} <= dec.last_path()
        out.append({k: r[k] for k in ("tested",) + q.MC_COUNTERS_ALL})
    assert out[0] == out[1]
    x, z = depolarizing(seed, 0, B, code.n, p)
    wX, wZ = flip_reference(seed, 0, B, qX, qZ)
    sX, sZ = code.syndrome(0, x) ^ wX, code.syndrome(1, z) ^ wZ
    eX, eZ, fl, it, _ = soft_cpu(code, qX, qZ, 160, None, schedule).decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    assert {k: out[0][k] for k in want} == want


# ---- 5. a captured graph ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_soft_dev_decode_in_a_captured_graph_reads_new_syndrome_priors(tmp, schedule):
    import torch
    shape, P = (4, 5, 10), 33
    code = code_of(tmp, shape, P)[0]
    sX, sZ, qX, qZ = table_inputs(tmp, shape, P)
    B = len(sX)
    first, second = (qX, qZ), (syndrome_priors(code.numEqsX, 91), syndrome_priors(code.numEqsZ, 92))
    dec = wave_decoder(code, *first, schedule=schedule, max_batch=B)  # the first set allocates the device table
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
        dec.decode_batch_soft_dev(tX, tZ, 0.03, 20, "syndrome", eX, eZ, fl, fX=fX, fZ=fZ, iters=it, q=qf, stream=stream)

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(s)
    assert {"minsum", "soft", "wave", "sparse"} <= dec.last_path()

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
        host = soft_decode(soft_cpu(code, pri[0], pri[1], 160, None, schedule), sX, sZ, 0.03, 20, "syndrome")
        assert_same_soft(wants[-1], host, "against the CPU engine")
    assert not np.array_equal(wants[0][5], wants[1][5]) or not same_floats(wants[0][4], wants[1][4])


# ---- 6. a group -------------------------------------------------------------------------------------------------------------------
def test_a_two_part_group_decodes_like_one_part(tmp):
    shape, P = (3, 5, 10), 9
    code = code_of(tmp, shape, P)[0]
    _, _, qX, qZ = table_inputs(tmp, shape, P)
    two = q.DecoderGPU(code, devices=[0, 0], engine="sparse")
    two.set_option("bp_method", 1)
    two.set_option("minsum_wave", 1)
    two.set_syndrome_priors(qX, qZ)
    assert all(p.get_syndrome_priors() is not None for p in two.parts())
    for schedule in SCHEDULES:
        two.set_option("minsum_schedule", SCHEDULES.index(schedule))
        for kind in KINDS:
            sX, sZ, _, _ = table_inputs(tmp, shape, P, kind)
            for case in (("fixed", 0.03, 11), ("syndrome", 0.03, 20)):
                stop, p, N = case
                got = soft_decode(two, sX, sZ, p, N, stop)
                assert {"minsum", "soft", "wave", "sparse"} <= two.last_path()
                assert_same_soft(got, table_reference(tmp, shape, P, case, kind, None, schedule),
                                 label(shape, P, kind, schedule, case, "group"))

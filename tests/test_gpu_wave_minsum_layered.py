"""The layered wave min-sum kernels on the device (set_option("minsum_schedule", 1) beside set_option("minsum_wave", 1)
on a sparse-engine handle; bp_wave_minsum.hip): the case table of tests/test_wave_minsum.py -- eight block shapes x ten
P, so each of the 24 kernels runs at every group count G = 64 // P and every idle-lane count of the table -- against the
CPU engine's outputs that tests/test_minsum_layered.py computes and checks for non-vacuity, with the scalar p and with
priors; the scale, a syndrome byte other than 0 / 1; the shipped codes through decode_batch and the Monte-Carlo pipeline
with and without the OSD stage; packed records in a captured graph; the path; the sparse LAYERED kernels with minsum_wave
at 0, bit-identical; a two-part group.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns.  There is no tolerance."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.codes import P7, P61, code_path
from qec_ldpc_amd.gather import pack_records
from test_circulant_shapes import KINDS, PS, SHAPES, batch, code_of, groups, inputs, ragged, shape_id
from test_general_code import assert_same_decode, same_floats
from test_gpu_general_code import count
from test_minsum import PRIOR_NS
from test_minsum_layered import layered_cpu, layered_reference
from test_priors import prior_vectors
from test_wave_minsum import DECODE_CASES, PRIOR_CASES, SCALE, reference

pytestmark = pytest.mark.gpu

_decoders = {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_wave_minsum_layered")


def wave_decoder(code, **kw):
    dec = q.DecoderGPU(code, 0, engine="sparse", **kw)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", 1)
    dec.set_option("minsum_schedule", 1)
    return dec


def gpu(tmp, shape, P):
    """One sparse-engine decoder per row of the table, under layered min-sum with the wave kernels (a test that changes
    an option or sets priors puts it back)."""
    key = (shape, P)
    if key not in _decoders:
        _decoders[key] = wave_decoder(code_of(tmp, shape, P)[0])
    return _decoders[key]


def decode(dec, sX, sZ, case, want_q=True):
    stop, p, N = case
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=want_q)
    assert {"minsum", "serial", "wave", "sparse"} <= dec.last_path()
    return got


def rows(ref, k):
    return tuple(a[:k] for a in ref)


def label(shape, P, kind, case, what):
    return "%s P=%d %s %s p=%g N=%d %s" % ((shape_id(shape), P, kind) + case + (what,))


# ---- 1. the table, scalar p ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_table_scalar(tmp, shape):
    for P in PS:
        dec = gpu(tmp, shape, P)
        assert "P=%d G=%d" % (P, groups(P)) in dec.describe(), dec.describe()
        for kind in KINDS:
            sX, sZ = inputs(tmp, shape, P, kind)
            for case in DECODE_CASES:
                want = layered_reference(tmp, shape, P, case, kind)
                assert_same_decode(decode(dec, sX, sZ, case, True), want, label(shape, P, kind, case, "with q"))
                assert_same_decode(decode(dec, sX, sZ, case, False), want, label(shape, P, kind, case, "without q"),
                                   with_q=False)
                if kind != "table":
                    continue
                k = ragged(P)
                if k != batch(P):  # G divides the batch: its first k rows leave a ragged wave
                    for want_q in (True, False):
                        assert_same_decode(decode(dec, sX[:k], sZ[:k], case, want_q), rows(want, k),
                                           label(shape, P, kind, case, "ragged, q %s" % want_q), with_q=want_q)
                assert_same_decode(decode(dec, sX[:1], sZ[:1], case, True), rows(want, 1),
                                   label(shape, P, kind, case, "B = 1"))


# ---- 2. the table, priors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_table_priors(tmp, shape):
    for P in PS:
        dec = gpu(tmp, shape, P)
        n = code_of(tmp, shape, P)[0].n
        sX, sZ = inputs(tmp, shape, P)
        runs = [("random", PRIOR_CASES)]
        if P in (3, 22, 33, 64):  # priors 0, 1 and 1/2 among them
            runs.append(("special", tuple((stop, 0.3, N) for stop in ("fixed", "syndrome", "ref") for N in PRIOR_NS)))
        try:
            for vec, cases in runs:
                dec.set_priors(*prior_vectors(n, vec))
                for case in cases:
                    want = layered_reference(tmp, shape, P, case, "table", vec)
                    assert_same_decode(decode(dec, sX, sZ, case), want, label(shape, P, vec, case, "priors"))
        finally:
            dec.set_priors(None, None)
        # the priors matter
        assert not same_floats(layered_reference(tmp, shape, P, PRIOR_CASES[0], "table", "random")[4],
                               layered_reference(tmp, shape, P, ("fixed", 0.03, 11))[4])


# ---- 3. the scale, a syndrome byte other than 0 / 1 ------------------------------------------------------------------------
def test_scales_1_and_256(tmp):
    shape, P = (3, 4, 8), 21
    dec = gpu(tmp, shape, P)
    sX, sZ = inputs(tmp, shape, P)
    try:
        for scale in (1, 256):
            dec.set_option("minsum_scale", scale)
            for case in (("fixed", 0.03, 11), ("syndrome", 0.03, 20)):
                want = layered_reference(tmp, shape, P, case, scale=scale)
                assert_same_decode(decode(dec, sX, sZ, case), want, label(shape, P, "scale %d" % scale, case, ""))
    finally:
        dec.set_option("minsum_scale", SCALE)
    assert not same_floats(layered_reference(tmp, shape, P, ("fixed", 0.03, 11), scale=1)[4],
                           layered_reference(tmp, shape, P, ("fixed", 0.03, 11), scale=256)[4])


def test_a_syndrome_byte_of_2(tmp):
    """Truthy in the check update, equal to no parity: SYNDROME_FAIL in both sectors, and the syndrome stop runs that
    row to the cap."""
    shape, P = (3, 3, 6), 9
    code = code_of(tmp, shape, P)[0]
    dec = gpu(tmp, shape, P)
    sX, sZ = (np.array(a) for a in inputs(tmp, shape, P))
    row = 5
    sX[row, 7] = 2
    sZ[row, 11] = 2
    cpu = layered_cpu(code, SCALE)
    for case in (("syndrome", 0.03, 20), ("fixed", 0.03, 11), ("ref", 0.03, 20)):
        stop, p, N = case
        want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
        got = decode(dec, sX, sZ, case)
        assert_same_decode(got, want, label(shape, P, "byte 2", case, ""))
        assert got[2][row] & q.SYNDROME_FAIL_X and got[2][row] & q.SYNDROME_FAIL_Z
        if stop == "syndrome":
            assert got[3][row].tolist() == [20, 20]


# ---- 4. the shipped codes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [P61, P7], ids=["P61", "P7"])
def test_shipped_codes(name):
    code = q.Quantum_LDPC_Code.createFromFile(code_path(name))
    dec, cpu = wave_decoder(code), layered_cpu(code, SCALE)
    for p in (0.02, 0.05):
        x, z = depolarizing(0x51EC0DE, 0, 256, code.n, p)
        sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
        for stop, N in (("syndrome", 20), ("fixed", 11)):
            want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            assert_same_decode(decode(dec, sX, sZ, (stop, p, N)), want, "%s p=%g %s" % (name, p, stop))


@pytest.mark.parametrize("osd", [0, 1])
@pytest.mark.parametrize("name", [P61, P7], ids=["P61", "P7"])
def test_shipped_codes_monte_carlo(name, osd):
    """Every counter and osd_sectors equal the same handle's with minsum_wave at 0 (the sparse LAYERED kernels), and
    the CPU engine's on the same samples."""
    code = q.Quantum_LDPC_Code.createFromFile(code_path(name))
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_schedule", 1)
    dec.set_option("osd", osd)
    dec.set_option("osd_order", 10 if osd else 0)
    out = []
    for wave in (0, 1):
        dec.set_option("minsum_wave", wave)
        r = dec.monte_carlo(1, 0, 4096, 0.05, 20, "syndrome", batch=1024)
        assert ("wave" in dec.last_path()) == bool(wave) and {"minsum", "serial", "sparse"} <= dec.last_path()
        assert ("osd" in dec.last_path()) == bool(osd)
        out.append(({k: r[k] for k in ("tested",) + q.MC_COUNTERS_ALL}, dec.get_option("osd_sectors")))
    assert out[0] == out[1], (name, osd)
    assert out[0][0]["tested"] == 4096 and (out[0][1] > 0) == bool(osd)
    # against the CPU engine on the same samples: the BP counters
    x, z = depolarizing(1, 0, 4096, code.n, 0.05)
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    cpu = layered_cpu(code, SCALE)
    cpu.set_option("osd", osd)
    cpu.set_option("osd_order", 10 if osd else 0)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    got = dec.monte_carlo(1, 0, 4096, 0.05, 20, "syndrome", batch=1024)
    assert {k: got[k] for k in want} == want, (name, osd)
    assert dec.get_option("osd_sectors") == cpu.get_option("osd_sectors")


# ---- 5. the round trip, the path, the sparse kernels --------------------------------------------------------------------------
def test_round_trip_and_the_sparse_layered_kernels(tmp):
    """minsum_schedule 0 -> 1 -> 0 on the wave kernels restores flooding; with minsum_wave at 0 the sparse LAYERED
    kernels run instead and give the same bits."""
    shape, P = (4, 4, 8), 22
    dec = q.DecoderGPU(code_of(tmp, shape, P)[0], 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", 1)
    sX, sZ = inputs(tmp, shape, P)
    case = ("syndrome", 0.03, 20)
    outs, words = [], []
    for sched in (0, 1, 0):
        dec.set_option("minsum_schedule", sched)
        assert dec.get_option("minsum_schedule") == sched
        outs.append(dec.decode_batch(sX, sZ, 0.03, 20, "syndrome", want_iters=True, want_q=True))
        assert ("serial" in dec.last_path()) == bool(sched) and {"minsum", "wave", "sparse"} <= dec.last_path()
        words.append(dec.get_option("last_path"))
    assert words[0] == words[2] and words[1] == words[0] | q.PATH["serial"]
    assert words[1] & (q.PATH["sparse"] | q.PATH["minsum"] | q.PATH["serial"] | q.PATH["wave"]) == 64 + 2048 + 1024 + 8192
    want = layered_reference(tmp, shape, P, case)
    assert_same_decode(outs[1], want, "layered")
    assert_same_decode(outs[0], reference(tmp, shape, P, case), "flooding")
    assert_same_decode(outs[2], outs[0], "0 -> 1 -> 0")
    assert not same_floats(outs[1][4], outs[0][4])
    dec.set_option("minsum_schedule", 1)
    dec.set_option("minsum_wave", 0)
    for c in (case, ("fixed", 0.03, 11), ("ref", 0.03, 20)):
        stop, p, N = c
        got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
        assert {"minsum", "serial", "sparse"} <= dec.last_path() and "wave" not in dec.last_path()
        assert_same_decode(got, layered_reference(tmp, shape, P, c), "sparse LAYERED kernels %s" % stop)
    # under the product rule the options do nothing
    dec.set_option("minsum_wave", 1)
    dec.set_option("bp_method", 0)
    dec.decode_batch(sX, sZ, 0.03, 5, "fixed")
    assert dec.last_path() == {"sparse"}


# ---- 6. a captured graph ------------------------------------------------------------------------------------------------------
def test_packed_records_in_a_captured_graph_read_new_priors(tmp):
    """decode_batch_packed_dev with the options set before the capture: the replay's records equal the direct call's,
    and a replay after a second set_priors decodes with the new tables (nothing is allocated by the call)."""
    import torch
    shape, P = (4, 5, 10), 33
    code = code_of(tmp, shape, P)[0]
    sX, sZ = inputs(tmp, shape, P)
    B = len(sX)
    dec = wave_decoder(code, max_batch=B)
    first, second = prior_vectors(code.n, "random"), prior_vectors(code.n, "special", seed=7)
    dev = torch.device("cuda", 0)
    tX, tZ = torch.from_numpy(np.array(sX)).to(dev), torch.from_numpy(np.array(sZ)).to(dev)
    rec = torch.zeros((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    it = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    qf = torch.zeros((B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    outs = (rec, it, qf)

    def capture():
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                dec.decode_batch_packed_dev(tX, tZ, 0.03, 11, "syndrome", rec, iters=it, q=qf, stream=s)
        assert {"minsum", "serial", "wave", "sparse", "records"} <= dec.last_path()
        return g

    def replay(g):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    def direct():
        for t in outs:
            t.zero_()
        dec.decode_batch_packed_dev(tX, tZ, 0.03, 11, "syndrome", rec, iters=it, q=qf)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    def same(got, want, what):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_floats(got[2], want[2]), what

    def host(pri):
        w = layered_cpu(code, SCALE, pri).decode_batch(sX, sZ, 0.03, 11, "syndrome", want_iters=True, want_q=True)
        return [pack_records(w[0], w[1], w[2]), w[3], w[4]]

    dec.set_priors(*first)  # allocates the device buffers before the capture
    with_priors = capture()
    wants = []
    for pri in (first, second):
        dec.set_priors(*pri)  # rewrites the buffers the captured kernel reads
        wants.append(direct())
        same(replay(with_priors), wants[-1], "replay with priors")
        same(wants[-1], host(pri), "priors against the CPU engine")
    assert not np.array_equal(wants[0][0], wants[1][0]) or not same_floats(wants[0][2], wants[1][2])
    dec.set_option("minsum_schedule", 0)  # the graph keeps the kernels it captured
    same(replay(with_priors), wants[-1], "replay after the option went back to 0")


# ---- 7. a group ---------------------------------------------------------------------------------------------------------------
def test_a_two_part_group_decodes_like_one_part(tmp):
    shape, P = (3, 5, 10), 9
    code = code_of(tmp, shape, P)[0]
    two = q.DecoderGPU(code, devices=[0, 0], engine="sparse")
    two.set_option("bp_method", 1)
    two.set_option("minsum_wave", 1)
    two.set_option("minsum_schedule", 1)
    assert all(p.get_option("minsum_schedule") == 1 for p in two.parts()) and two.get_option("minsum_schedule") == 1
    for kind in KINDS:
        sX, sZ = inputs(tmp, shape, P, kind)
        for case in (("fixed", 0.03, 11), ("syndrome", 0.03, 20)):
            stop, p, N = case
            got = two.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            assert {"minsum", "serial", "wave", "sparse"} <= two.last_path()
            assert_same_decode(got, layered_reference(tmp, shape, P, case, kind), label(shape, P, kind, case, "group, CPU"))

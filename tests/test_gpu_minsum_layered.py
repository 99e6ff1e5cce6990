"""Layered min-sum (set_option("minsum_schedule", 1) under set_option("bp_method", 1)) on the device: every row of the
case table of test_sparse_shapes.py -- all 36 LAYERED kernels of bp_sparse.hip, asserted in test_minsum_layered.py --
with the scalar p and with priors under every stop rule, with and without q_final.  The LDS codes are held to the numpy
yardstick of test_minsum_layered.py (the outputs computed there, once), the replicated HBM codes to the block-by-block
reference put together from the yardstick of the small code under the fixed stop (it does not pass through the CPU
engine) and to the CPU engine under the other stops, the large regular codes to the CPU engine, which
test_minsum_layered.py holds to the yardstick.  Then the _dev decode in a captured graph replayed after set_priors, the
round trip 0 -> 1 -> 0, the Monte-Carlo counters on QC_LDPC_CSS(3,3,6,13,3,2) against the CPU engine, minsum_wave beside
the option, the refusals and a two-part group.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from test_general_code import assert_same_decode, mixed_syndromes, same_floats
from test_gpu_general_code import count
from test_minsum import MS_P, MS_P_REF, PRIOR_NS, minsum_cpu
from test_minsum_layered import GPU_CASES, layered_cpu, layered_yardstick, yard
from test_priors import prior_vectors
from test_sparse_shapes import (HBM_CASES, HBM_N, HBM_ROWS, LDS_CASES, P_MAIN, P_REF, REPLICATED, block_rows, case_id,
                                code_of, hbm_inputs, hbm_priors, inputs, matrices)

pytestmark = pytest.mark.gpu

_decoders, _block = {}, {}


def gpu(case):
    """One sparse-engine decoder per row of the case table, under layered min-sum at the default scale (a test that
    changes an option or sets priors puts it back)."""
    if case not in _decoders:
        _decoders[case] = q.DecoderGPU(code_of(*case), 0, engine="sparse")
        _decoders[case].set_option("bp_method", 1)
        _decoders[case].set_option("minsum_schedule", 1)
    return _decoders[case]


def decode(dec, sX, sZ, p, N, stop, want_q=True):
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=want_q)
    assert {"minsum", "serial", "sparse"} <= dec.last_path() and "wave" not in dec.last_path()
    return got


def test_the_case_table_is_the_one_asserted_to_reach_all_36():
    assert set(LDS_CASES + HBM_CASES) == set(GPU_CASES)


@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
@pytest.mark.parametrize("kind", ["scalar", "random", "special"])
def test_lds_matches_the_yardstick(case, kind):
    name, _ = case
    dec = gpu(case)
    sX, sZ = inputs(name)
    if kind == "scalar":
        runs = (("fixed", MS_P[name], (0, 1, 2, 11)), ("syndrome", MS_P[name], (20,)), ("ref", MS_P[name], (11,)),
                ("ref", MS_P_REF, (11,)))
    else:
        runs = tuple((stop, None, PRIOR_NS) for stop in ("fixed", "syndrome", "ref"))
    split = False
    try:
        if kind != "scalar":
            dec.set_priors(*prior_vectors(code_of(*case).n, kind))
        for stop, p, Ns in runs:
            for N in Ns:
                want = yard(name, kind, stop, N, 160, p)
                split |= bool((want[3][:, 0] != want[3][:, 1]).any())
                got = decode(dec, sX, sZ, 0.3 if p is None else p, N, stop)  # under priors p is not used
                assert np.isfinite(got[4]).all()
                assert_same_decode(got, want, "%s %s %s N=%d" % (case_id(case), kind, stop, N))
                if N == Ns[-1]:  # without q_final: the export is skipped, nothing else changes
                    bare = decode(dec, sX, sZ, 0.3 if p is None else p, N, stop, want_q=False)
                    assert_same_decode(bare, want, "%s %s %s N=%d no q" % (case_id(case), kind, stop, N), with_q=False)
    finally:
        dec.set_priors(None, None)
    # a row whose sectors stop at different iterations: one idles while the other runs
    assert split or kind != "scalar"


def test_scale_256_on_the_device():
    case = ("mid", "general")
    dec = gpu(case)
    sX, sZ = inputs("mid")
    try:
        dec.set_option("minsum_scale", 256)
        for stop, N in (("fixed", 11), ("syndrome", 20)):
            assert_same_decode(decode(dec, sX, sZ, MS_P["mid"], N, stop), yard("mid", "scalar", stop, N, 256), stop)
    finally:
        dec.set_option("minsum_scale", 160)
    assert not same_floats(yard("mid", "scalar", "fixed", 11, 256)[4], yard("mid", "scalar", "fixed", 11, 160)[4])


def block_reference(name, priors):
    """test_sparse_shapes.block_reference's construction with the layered yardstick: the fixed-stop decode of
    block_rows(name) put together from the small code's rows (the blocks share no variable, so the layers of the
    replicated code are the small code's, block by block)."""
    key = (name, priors)
    if key not in _block:
        base, r = REPLICATED[name]
        HX, HZ = matrices(base)
        sx, sz = block_rows(name)[:2]
        pri = prior_vectors(HX.shape[1], "random") if priors else (P_MAIN, P_MAIN)
        small = layered_yardstick(HX, HZ, sx, sz, pri[0], pri[1], 160, HBM_N, "fixed")
        D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
        EX = HX.shape[0] * D
        qs = small[4].reshape(HBM_ROWS, r, -1)
        qf = np.concatenate([qs[:, :, :EX].reshape(HBM_ROWS, -1), qs[:, :, EX:].reshape(HBM_ROWS, -1)], axis=1)
        flags = np.bitwise_or.reduce(small[2].reshape(HBM_ROWS, r), axis=1)
        iters = small[3].reshape(HBM_ROWS, r, 2)
        assert (iters == HBM_N).all()
        _block[key] = (small[0].reshape(HBM_ROWS, -1), small[1].reshape(HBM_ROWS, -1), flags,
                       np.ascontiguousarray(iters[:, 0]), np.ascontiguousarray(qf))
    return _block[key]


@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
def test_hbm(case, priors):
    name, _ = case
    dec = gpu(case)
    pri = hbm_priors(name) if priors else None
    cpu = layered_cpu(code_of(*case), 160, pri)
    sX, sZ = hbm_inputs(name)
    try:
        if pri:
            dec.set_priors(*pri)
        if name in REPLICATED:  # the fixed stop: block by block from the yardstick
            bX, bZ = block_rows(name)[2:]
            assert_same_decode(decode(dec, bX, bZ, P_MAIN, HBM_N, "fixed"), block_reference(name, priors),
                               "%s priors=%s blocks" % (name, priors))
            stops = (("ref", P_REF, 11), ("syndrome", P_MAIN, 6))
        else:
            stops = (("ref", P_REF, 11), ("fixed", P_MAIN, 3), ("syndrome", P_MAIN, 6))
        for stop, p, N in stops:
            want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            if stop == "syndrome":  # the all-zero row stops at the first test, a sampled row runs on
                assert (want[3].min(axis=0) == 1).all() and (want[3].max(axis=0) > 1).all(), want[3].tolist()
            assert_same_decode(decode(dec, sX, sZ, p, N, stop), want, "%s priors=%s %s" % (name, priors, stop))
            assert_same_decode(decode(dec, sX, sZ, p, N, stop, want_q=False), want, "%s priors=%s %s no q" % (name, priors, stop),
                               with_q=False)
    finally:
        dec.set_priors(None, None)
    if priors and name in REPLICATED:
        assert not same_floats(block_reference(name, True)[4], block_reference(name, False)[4])


def test_dev_decode_in_a_captured_graph_reads_new_priors():
    """decode_batch_dev with the option set before the capture: the replay's outputs equal the direct call's, the path
    carries QEC_PATH_MINSUM | QEC_PATH_SERIAL, and with priors a replay after a second set_priors decodes with the new
    ones (the LLR tables are rewritten in place; nothing is allocated by set_option or by the call).  A graph captured
    with the option at 1 keeps the LAYERED kernels after the option goes back to 0."""
    import torch
    name, B = "mid", 129
    code = code_of(name, "general")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_schedule", 1)
    first, second = prior_vectors(code.n, "random"), prior_vectors(code.n, "special", seed=7)
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(matrices(name), 77, B, (0.01, 0.05))
    tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
    eX = torch.zeros((B, code.n), dtype=torch.uint8, device=dev)
    eZ = torch.zeros((B, code.n), dtype=torch.uint8, device=dev)
    fl = torch.zeros((B,), dtype=torch.uint8, device=dev)
    it = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    qf = torch.zeros((B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    outs = (eX, eZ, fl, it, qf)

    def capture():
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                dec.decode_batch_dev(tX, tZ, 0.05, 11, "syndrome", eX, eZ, fl, iters=it, q=qf, stream=s)
        assert {"minsum", "serial", "sparse"} <= dec.last_path()
        assert dec.get_option("last_path") & (q.PATH["minsum"] | q.PATH["serial"]) == 2048 + 1024
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
        dec.decode_batch_dev(tX, tZ, 0.05, 11, "syndrome", eX, eZ, fl, iters=it, q=qf)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    def host(pri, layered=True):
        cpu = layered_cpu(code, 160, pri) if layered else minsum_cpu(code, 160, pri)
        return cpu.decode_batch(sX, sZ, 0.05, 11, "syndrome", want_iters=True, want_q=True)

    scalar = capture()
    want = direct()
    assert_same_decode(replay(scalar), want, "replay")
    assert_same_decode(want, host(None), "the direct call against the CPU engine")
    dec.set_priors(*first)  # allocates the device buffers before the capture
    with_priors = capture()
    wants = []
    for pri in (first, second):
        dec.set_priors(*pri)  # rewrites the buffers the captured kernels read
        wants.append(direct())
        assert_same_decode(replay(with_priors), wants[-1], "replay with priors")
        assert_same_decode(wants[-1], host(pri), "priors against the CPU engine")
    assert not np.array_equal(wants[0][0], wants[1][0]) or not same_floats(wants[0][4], wants[1][4])
    dec.set_option("minsum_schedule", 0)
    assert_same_decode(direct(), host(second, layered=False), "option 0: flooding")
    assert_same_decode(replay(with_priors), wants[-1], "the graph keeps the kernels it captured")


def test_monte_carlo_counters():
    """QC_LDPC_CSS(3,3,6,13,3,2) with the degenerate check (the case table's r3-3-6-13 is a random regular pair whose X
    and Z checks do not commute, so it has no logical check to count with), seed 1, 2048 samples at p = 0.05 under the
    syndrome stop: every counter equals the CPU engine's on the same samples."""
    code = q.QC_LDPC_CSS(3, 3, 6, 13, 3, 2).with_logical("degenerate")
    HX, HZ = code.pcm(0), code.pcm(1)
    dec, cpu = q.DecoderGPU(code, 0, engine="sparse"), layered_cpu(code)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_schedule", 1)
    seed, B, p = 1, 2048, 0.05
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    flood = minsum_cpu(code).decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    assert int(it.sum()) < int(flood[3].sum())  # the schedule shows in the counters
    got = dec.monte_carlo(seed, 0, B, p, 20, "syndrome", batch=1024)
    assert {k: got[k] for k in want} == want
    assert {"minsum", "serial", "sparse"} <= dec.last_path()


def test_round_trip_restores_the_flooding_kernels():
    case = ("hgp_ham", "general")
    code = code_of(*case)
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    sX, sZ = inputs("hgp_ham")
    first = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    path = dec.get_option("last_path")
    assert dec.last_path() == {"sparse", "minsum"}
    assert_same_decode(first, minsum_cpu(code).decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True), "option 0")
    dec.set_option("minsum_schedule", 1)
    assert not same_floats(decode(dec, sX, sZ, 0.05, 11, "ref")[4], first[4])
    dec.set_option("minsum_schedule", 0)
    again = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    assert dec.get_option("last_path") == path
    assert_same_decode(again, first, "0 -> 1 -> 0")
    # under the product rule the option does nothing
    dec.set_option("bp_method", 0)
    dec.set_option("minsum_schedule", 1)
    prod = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    assert dec.last_path() == {"sparse"}
    assert_same_decode(prod, q.DecoderCPU(code).decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True), "product")


def test_a_relay_ignores_the_option_on_the_device():
    case = ("r3-3-6-13", "graph")
    code = code_of(*case)
    sX, sZ = inputs("r3-3-6-13")
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    zero = np.zeros((1, code.n), dtype=np.float32)
    dec.set_relay(zero, zero)
    dec.set_option("minsum_schedule", 1)
    got = dec.decode_batch(sX, sZ, 0.05, 11, "fixed", want_iters=True, want_q=True)
    assert {"minsum", "relay", "sparse"} <= dec.last_path() and "serial" not in dec.last_path()
    assert_same_decode(got, minsum_cpu(code).decode_batch(sX, sZ, 0.05, 11, "fixed", want_iters=True, want_q=True), "relay")


def test_minsum_wave_beside_the_option():
    """With minsum_wave = 0 the LAYERED kernels of the sparse-graph engine run and the path carries no "wave"; with
    minsum_wave = 1 the layered wave kernels give the same bits (tests/test_gpu_wave_minsum_layered.py holds them to the
    table); with the schedule back at 0 the flooding wave kernels run again."""
    code = q.QC_LDPC_CSS(3, 3, 6, 13, 3, 2)
    HX, HZ = code.pcm(0), code.pcm(1)
    x, z = depolarizing(3, 0, 96, code.n, 0.05)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_schedule", 1)
    want = layered_cpu(code).decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert_same_decode(decode(dec, sX, sZ, 0.05, 20, "syndrome"), want, "the sparse LAYERED kernels")
    dec.set_option("minsum_wave", 1)
    got = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert {"minsum", "serial", "wave", "sparse"} <= dec.last_path()
    assert_same_decode(got, want, "the layered wave kernels")
    dec.set_option("minsum_schedule", 0)
    got = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert {"minsum", "wave"} <= dec.last_path() and "serial" not in dec.last_path()
    assert_same_decode(got, minsum_cpu(code).decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True), "flooding")


def test_refusals():
    from test_priors import code_of as named
    dec = q.DecoderGPU(named("P7"), 0)  # engine auto: the wave-circulant engine
    before = dec.describe()
    with pytest.raises(q.QecError, match="create the decoder with QEC_ENGINE_SPARSE"):
        dec.set_option("minsum_schedule", 1)
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["minsum_schedule"], 1) == -4  # QEC_ERR_UNSUPPORTED
    assert dec.get_option("minsum_schedule") == 0 and dec.describe() == before
    dec.set_option("minsum_schedule", 0)
    with pytest.raises(q.QecError, match="QEC_OPT_MINSUM_SCHEDULE"):
        dec.set_option("minsum_schedule", 2)
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["minsum_schedule"], 2) == -1  # QEC_ERR_ARG
    # a sparse handle: the option is data, and min-sum and the serial schedule refuse each other as before
    sp = q.DecoderGPU(named("P7"), 0, engine="sparse")
    sp.set_option("minsum_schedule", 1)
    sp.set_option("bp_method", 1)
    for other in ("correlated", "bp_schedule"):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
            sp.set_option(other, 1)
        assert sp.get_option(other) == 0
    sp.set_option("bp_method", 0)
    sp.set_option("bp_schedule", 1)
    with pytest.raises(q.QecError, match="QEC_OPT_BP_SCHEDULE"):
        sp.set_option("bp_method", 1)
    assert sp.get_option("bp_method") == 0 and sp.get_option("minsum_schedule") == 1


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one-device", "two-devices"])
def test_a_two_part_group_decodes_like_one_part(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("the box shows one device")
    name = "mid"
    code = code_of(name, "general")
    one, two = gpu((name, "general")), q.DecoderGPU(code, devices=list(devices))
    two.set_option("bp_method", 1)
    two.set_option("minsum_schedule", 1)
    assert all(p.get_option("minsum_schedule") == 1 for p in two.parts()) and two.get_option("minsum_schedule") == 1
    sX, sZ = inputs(name)
    pri = prior_vectors(code.n, "special")
    try:
        for priors in (None, pri):
            if priors:
                one.set_priors(*priors)
                two.set_priors(*priors)
            for stop, N in (("fixed", 5), ("syndrome", 20)):
                a = one.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                b = two.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                assert_same_decode(b, a, "%s %s" % (stop, priors is not None))
                assert {"minsum", "serial"} <= two.last_path()
    finally:
        one.set_priors(None, None)

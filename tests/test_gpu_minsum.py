"""Scaled min-sum BP (set_option("bp_method", 1)) on the device: every row of the case table of test_sparse_shapes.py --
all 36 MINSUM kernels of bp_sparse.hip, asserted in test_minsum.py -- with the scalar p and with priors under every
stop rule.  The LDS codes are held to the numpy yardstick of test_minsum.py (the outputs computed there, once), the
replicated HBM codes to the block-by-block reference put together from the yardstick of the small code under the
fixed stop (it does not pass through the CPU engine) and to the CPU engine under the other stops, the large regular
codes to the CPU engine, which test_minsum.py holds to the yardstick.  The table already holds the smallest shapes
that can go wrong: dense32 (degree 32, every column weight 1 .. 16, 64 threads), tall (qubits in no X check), wide
(the variable pass loops).  Then packed records in a captured graph, osd_dev, the Monte-Carlo pipeline with and
without OSD, the wave-circulant refusal, the round trip 0 -> 1 -> 0 and a two-part group.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.gather import pack_records
from test_general_code import assert_same_decode, code_matrices, mixed_syndromes, same_floats
from test_gpu_general_code import count, logical_code
from test_minsum import GPU_CASES, MS_P, MS_P_REF, PRIOR_NS, minsum_cpu, minsum_yardstick, yard
from test_priors import prior_vectors
from test_sparse_shapes import (HBM_CASES, HBM_N, HBM_ROWS, LDS_CASES, P_MAIN, P_REF, REPLICATED, block_rows, case_id,
                                code_of, hbm_inputs, hbm_priors, inputs, matrices)

pytestmark = pytest.mark.gpu

_decoders, _block = {}, {}


def gpu(case):
    """One sparse-engine decoder per row of the case table, under min-sum at the default scale (a test that changes
    an option or sets priors puts it back)."""
    if case not in _decoders:
        _decoders[case] = q.DecoderGPU(code_of(*case), 0, engine="sparse")
        _decoders[case].set_option("bp_method", 1)
    return _decoders[case]


def decode(dec, sX, sZ, p, N, stop):
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
    assert {"minsum", "sparse"} <= dec.last_path()
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
                ("ref", MS_P_REF, (20,)))
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
    finally:
        dec.set_priors(None, None)
    # a row whose sectors stop at different iterations: one idles while the other runs (under priors the thinned N
    # and a prior of 1, which no syndrome of the table agrees with, can leave every row at the cap in both sectors)
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
    """test_sparse_shapes.block_reference's construction with the min-sum yardstick: the fixed-stop decode of
    block_rows(name) put together from the small code's rows."""
    key = (name, priors)
    if key not in _block:
        base, r = REPLICATED[name]
        HX, HZ = matrices(base)
        sx, sz = block_rows(name)[:2]
        pri = prior_vectors(HX.shape[1], "random") if priors else (P_MAIN, P_MAIN)
        small = minsum_yardstick(HX, HZ, sx, sz, pri[0], pri[1], 160, HBM_N, "fixed")
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
    cpu = minsum_cpu(code_of(*case), 160, pri)
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
    finally:
        dec.set_priors(None, None)
    if priors and name in REPLICATED:
        assert not same_floats(block_reference(name, True)[4], block_reference(name, False)[4])


def test_packed_records_in_a_captured_graph_read_new_priors():
    """decode_batch_packed_dev with method 1 set before the capture: the replay's records equal the direct call's,
    the path carries QEC_PATH_MINSUM, and with priors a replay after a second set_priors decodes with the new ones
    (the LLR tables are rewritten in place; nothing is allocated by set_option or by the call)."""
    import torch
    name, B = "mid", 129
    code = code_of(name, "general")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    dec.set_option("bp_method", 1)
    first, second = prior_vectors(code.n, "random"), prior_vectors(code.n, "special", seed=7)
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(matrices(name), 77, B, (0.01, 0.05))
    tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
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
                dec.decode_batch_packed_dev(tX, tZ, 0.05, 11, "syndrome", rec, iters=it, q=qf, stream=s)
        assert {"minsum", "sparse", "records"} <= dec.last_path()
        assert dec.get_option("last_path") & q.PATH["minsum"] == 2048
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
        dec.decode_batch_packed_dev(tX, tZ, 0.05, 11, "syndrome", rec, iters=it, q=qf)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    def same(got, want, what):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_floats(got[2], want[2]), what

    def host(pri):
        w = minsum_cpu(code, 160, pri).decode_batch(sX, sZ, 0.05, 11, "syndrome", want_iters=True, want_q=True)
        return [pack_records(w[0], w[1], w[2]), w[3], w[4]]

    scalar = capture()
    want = direct()
    same(replay(scalar), want, "replay")
    same(want, host(None), "the direct call against the CPU engine")
    dec.set_priors(*first)  # allocates the device buffers before the capture
    with_priors = capture()
    wants = []
    for pri in (first, second):
        dec.set_priors(*pri)  # rewrites the buffers the captured kernels read
        wants.append(direct())
        same(replay(with_priors), wants[-1], "replay with priors")
        same(wants[-1], host(pri), "priors against the CPU engine")
    assert not np.array_equal(wants[0][0], wants[1][0]) or not same_floats(wants[0][2], wants[1][2])


@pytest.mark.parametrize("lam", [0, 10])
def test_osd_dev_under_minsum(lam):
    """osd_dev under method 1 (the LLR column key) equals DecoderCPU's qec_osd on the same decoded batch."""
    import torch
    name, p, B = "hgp_ham", 0.05, 384
    code = code_of(name, "general")
    HX, HZ = matrices(name)
    x, z = depolarizing(0x51EC0DE, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    cpu = minsum_cpu(code)
    main = cpu.decode_batch(sX, sZ, p, 20, "syndrome")
    assert ((main[2] & 1) != 0).sum() + ((main[2] & 2) != 0).sum() >= 40
    soft = cpu.decode_batch(sX, sZ, p, 3, "fixed", want_q=True)[4]
    cpu.set_option("osd_order", lam)
    want = cpu.osd(sX, sZ, soft, main[0], main[1], main[2])
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_option("osd_order", lam)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sX, sZ, soft, main[0], main[1], main[2])]
    dec.osd_dev(*t)
    torch.cuda.synchronize()
    for a, b, what in zip(t[3:], want, ("eX", "eZ", "flags")):
        assert np.array_equal(a.cpu().numpy(), b), what
    assert not (want[2] & 3).any()
    # the same call under method 0 reads q as probabilities: another order, another repair somewhere
    dec.set_option("bp_method", 0)
    u = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sX, sZ, soft, main[0], main[1], main[2])]
    dec.osd_dev(*u)
    torch.cuda.synchronize()
    assert not (np.array_equal(u[3].cpu().numpy(), want[0]) and np.array_equal(u[4].cpu().numpy(), want[1]))


@pytest.mark.parametrize("osd", [0, 1])
def test_monte_carlo_counters(osd):
    """hgp_ham with the degenerate check, seed 1, 4096 samples at p = 0.02 under the syndrome stop: every counter and
    osd_sectors equal DecoderCPU's on the same samples (the unfused pipeline: no shortcut of the product rule runs)."""
    code = logical_code("hgp_ham")
    HX, HZ = code_matrices("hgp_ham")
    dec, cpu = q.DecoderGPU(code, 0, engine="sparse"), minsum_cpu(code)
    dec.set_option("bp_method", 1)
    seed, B, p = 1, 4096, 0.02
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    bp_only = cpu.decode_batch(sX, sZ, p, 20, "syndrome")[2]
    assert (bp_only & 3).any()  # min-sum BP alone leaves failures
    for d in (dec, cpu):
        d.set_option("osd", osd)
        d.set_option("osd_order", 10 if osd else 0)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    if osd:
        assert want["synX"] == want["synZ"] == 0
    got = dec.monte_carlo(seed, 0, B, p, 20, "syndrome", batch=1024)
    assert {k: got[k] for k in want} == want, osd
    assert {"minsum", "sparse"} <= dec.last_path() and ("osd" in dec.last_path()) == bool(osd)
    assert dec.get_option("osd_sectors") == cpu.get_option("osd_sectors")
    assert (dec.get_option("osd_sectors") > 0) == bool(osd)


def test_round_trip_restores_the_product_kernels():
    case = ("hgp_ham", "general")
    code = code_of(*case)
    dec = q.DecoderGPU(code, 0, engine="sparse")
    sX, sZ = inputs("hgp_ham")
    first = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    path = dec.get_option("last_path")
    assert dec.last_path() == {"sparse"}
    assert_same_decode(first, q.DecoderCPU(code).decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True), "method 0")
    dec.set_option("bp_method", 1)
    assert not same_floats(decode(dec, sX, sZ, 0.05, 11, "ref")[4], first[4])
    dec.set_option("bp_method", 0)
    again = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    assert dec.get_option("last_path") == path
    assert_same_decode(again, first, "0 -> 1 -> 0")


def test_circulant_handle_refuses():
    from test_priors import code_of as named
    dec = q.DecoderGPU(named("P7"), 0)  # engine auto: the wave-circulant engine
    with pytest.raises(q.QecError, match="create the decoder with QEC_ENGINE_SPARSE"):
        dec.set_option("bp_method", 1)
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["bp_method"], 1) == -4  # QEC_ERR_UNSUPPORTED
    assert dec.get_option("bp_method") == 0
    dec.set_option("bp_method", 0)
    dec.set_option("minsum_scale", 200)  # the factor alone is only a number
    with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
        dec.set_option("bp_method", 2)
    # a sparse handle: min-sum and the correlated form / the serial schedule refuse each other
    sp = q.DecoderGPU(named("P7"), 0, engine="sparse")
    sp.set_option("bp_method", 1)
    for other in ("correlated", "bp_schedule"):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_METHOD"):
            sp.set_option(other, 1)
        assert sp.get_option(other) == 0
    sp.set_option("bp_method", 0)
    sp.set_option("correlated", 2)
    with pytest.raises(q.QecError, match="QEC_OPT_CORRELATED"):
        sp.set_option("bp_method", 1)
    assert sp.get_option("bp_method") == 0 and sp.get_option("correlated") == 2


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one-device", "two-devices"])
def test_a_two_part_group_decodes_like_one_part(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("the box shows one device")
    name = "mid"
    code = code_of(name, "general")
    one, two = gpu((name, "general")), q.DecoderGPU(code, devices=list(devices))
    two.set_option("minsum_scale", 200)
    two.set_option("bp_method", 1)
    assert all(p.get_option("bp_method") == 1 and p.get_option("minsum_scale") == 200 for p in two.parts())
    sX, sZ = inputs(name)
    pri = prior_vectors(code.n, "special")
    try:
        one.set_option("minsum_scale", 200)
        for priors in (None, pri):
            if priors:
                one.set_priors(*priors)
                two.set_priors(*priors)
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                           for a, b in zip(two.parts()[1].minsum_llr(), one.minsum_llr()))
            for stop, N in (("fixed", 5), ("syndrome", 20)):
                a = one.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                b = two.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                assert_same_decode(b, a, "%s %s" % (stop, priors is not None))
                assert "minsum" in two.last_path()
    finally:
        one.set_option("minsum_scale", 160)
        one.set_priors(None, None)

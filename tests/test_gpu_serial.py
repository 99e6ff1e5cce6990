"""The serial BP schedule (set_option("bp_schedule", 1)) on the device: every row of the case table of
test_sparse_shapes.py -- all 36 SERIAL kernels of bp_sparse.hip, asserted in test_serial.py -- with the scalar p and
with priors under every stop rule, held to the CPU engine, which test_serial.py holds to the numpy yardstick.  Where
the failure modes live: a layer larger than the workgroup (r3-3-6-1013: 1013 checks per layer on 256 threads), layers
of one check (dense32), variables in no check (tall), sectors with different layer counts (r4-5-10-7, tall, wide), one
sector stopped while the other runs (asserted on the references), a scratch slice reused by a second row.  Then packed
records, graph capture, the Monte-Carlo pipeline with and without OSD, the wave-circulant refusal and option 0.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns (NaN matches NaN)."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.gather import pack_records
from test_general_code import assert_same_decode, code_matrices, mixed_syndromes, same_floats
from test_gpu_general_code import count, logical_code
from test_priors import prior_vectors
from test_serial import GPU_CASES, SERIAL_P, SERIAL_P_REF, serial_cpu
from test_sparse_shapes import (HBM_CASES, LDS_CASES, P_MAIN, P_REF, case_id, code_of, hbm_inputs, hbm_priors,
                                inputs, matrices)

pytestmark = pytest.mark.gpu

_decoders = {}


def gpu(case):
    """One sparse-engine decoder per row of the case table, under the serial schedule (a test that changes the
    option or sets priors puts both back)."""
    if case not in _decoders:
        _decoders[case] = q.DecoderGPU(code_of(*case), 0, engine="sparse")
        _decoders[case].set_option("bp_schedule", 1)
    return _decoders[case]


def decode(dec, sX, sZ, p, N, stop):
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
    assert {"serial", "sparse"} <= dec.last_path()
    return got


def test_the_case_table_is_the_one_asserted_to_reach_all_36():
    assert set(LDS_CASES + HBM_CASES) == set(GPU_CASES)


@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
@pytest.mark.parametrize("priors", [None, "random", "special"], ids=["scalar", "random", "special"])
def test_lds_matches_cpu_engine(case, priors):
    name, _ = case
    code = code_of(*case)
    dec = gpu(case)
    pri = prior_vectors(code.n, priors) if priors else None
    cpu = serial_cpu(code, pri)
    sX, sZ = inputs(name)
    split = False
    try:
        if pri:
            dec.set_priors(*pri)
        for stop, p, Ns in (("fixed", SERIAL_P[name], (0, 1, 2, 11)), ("syndrome", SERIAL_P[name], (1, 20)),
                            ("ref", SERIAL_P[name], (11,)), ("ref", SERIAL_P_REF, (20,))):
            for N in Ns:
                want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                split |= bool((want[3][:, 0] != want[3][:, 1]).any())
                assert_same_decode(decode(dec, sX, sZ, p, N, stop), want,
                                   "%s %s %s p=%g N=%d" % (case_id(case), priors, stop, p, N))
    finally:
        dec.set_priors(None, None)
    assert split  # a row whose sectors stop at different iterations: one idles while the other runs


@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
def test_hbm_matches_cpu_engine(case, priors):
    name, _ = case
    dec = gpu(case)
    pri = hbm_priors(name) if priors else None
    cpu = serial_cpu(code_of(*case), pri)
    sX, sZ = hbm_inputs(name)
    try:
        if pri:
            dec.set_priors(*pri)
        for stop, p, N in (("ref", P_REF, 11), ("fixed", P_MAIN, 3), ("syndrome", P_MAIN, 6)):
            want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            if stop == "syndrome":  # the all-zero row stops at the first test, a sampled row runs on
                assert (want[3].min(axis=0) == 1).all() and (want[3].max(axis=0) > 1).all(), want[3].tolist()
            assert_same_decode(decode(dec, sX, sZ, p, N, stop), want, "%s priors=%s %s" % (name, priors, stop))
    finally:
        dec.set_priors(None, None)


def test_hbm_workgroups_reuse_their_scratch_slice():
    """More rows than the grid (4 workgroups per CU): zero syndromes except three sampled rows at the front and two
    past the grid, so a workgroup decodes a non-trivial row after a trivial one in the same slice."""
    import torch
    case = ("r3-3-6-1013", "graph")
    name = case[0]
    dec, cpu = gpu(case), serial_cpu(code_of(*case))
    grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    B = grid + 5
    hX, hZ = hbm_inputs(name)
    sX, sZ = np.zeros((B, hX.shape[1]), dtype=np.uint8), np.zeros((B, hZ.shape[1]), dtype=np.uint8)
    rows = [0, 1, 2, grid + 1, grid + 3]
    sX[rows], sZ[rows] = hX[:5], hZ[:5]
    want = cpu.decode_batch(sX, sZ, P_MAIN, 6, "syndrome", want_iters=True)
    assert (want[3][rows] > 1).all() and (np.delete(want[3], rows, axis=0) == 1).all()
    got = dec.decode_batch(sX, sZ, P_MAIN, 6, "syndrome", want_iters=True)
    assert {"serial", "sparse"} <= dec.last_path()
    assert_same_decode(got, want, "%s B=%d" % (name, B), with_q=False)


@pytest.mark.parametrize("case", [("wide", "general"), ("r3-9-20-7", "graph")], ids=case_id)
@pytest.mark.parametrize("B", [1, 63, 257])
def test_packed_records(case, B):
    name, _ = case
    dec, cpu = gpu(case), serial_cpu(code_of(*case))
    sX, sZ = mixed_syndromes(matrices(name), 1000 + B, B + 3, (0.01, 0.05))
    sX, sZ = sX[-B:], sZ[-B:]  # keeps the special rows
    for stop, N in (("ref", 20), ("fixed", 5), ("syndrome", 20)):
        want = cpu.decode_batch(sX, sZ, P_MAIN, N, stop, want_iters=True)
        rec, it = dec.decode_batch_packed(sX, sZ, P_MAIN, N, stop, want_iters=True)
        assert {"serial", "sparse", "records"} <= dec.last_path()
        assert np.array_equal(rec, pack_records(want[0], want[1], want[2])) and np.array_equal(it, want[3])


def test_a_captured_graph_keeps_its_serial_kernels_and_reads_new_priors():
    """decode_batch_dev captured under option 1: the replay after option 0 still runs the serial kernels (the option
    is read at the call), and with priors a replay after a second set_priors decodes with the new values."""
    import torch
    name, B = "mid", 129
    code = code_of(name, "general")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    dec.set_option("bp_schedule", 1)
    first, second = prior_vectors(code.n, "random"), prior_vectors(code.n, "special", seed=7)
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(matrices(name), 77, B, (0.01, 0.05))
    tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
    eX = torch.zeros((B, code.n), dtype=torch.uint8, device=dev)
    eZ, fl = torch.zeros_like(eX), torch.zeros(B, dtype=torch.uint8, device=dev)
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
        assert {"serial", "sparse"} <= dec.last_path()
        return g

    def replay(g):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    scalar = capture()
    want = serial_cpu(code).decode_batch(sX, sZ, 0.05, 11, "syndrome", want_iters=True, want_q=True)
    assert_same_decode(replay(scalar), want, "replay under option 1")
    dec.set_option("bp_schedule", 0)
    assert_same_decode(replay(scalar), want, "replay after option 0")
    flood = dec.decode_batch(sX, sZ, 0.05, 11, "syndrome", want_iters=True, want_q=True)
    assert "serial" not in dec.last_path() and not same_floats(flood[4], want[4])
    dec.set_option("bp_schedule", 1)
    dec.set_priors(*first)  # allocates the device buffer before the capture
    with_priors = capture()
    wants = []
    for pri in (first, second):
        dec.set_priors(*pri)  # rewrites the buffer the captured kernels read
        wants.append(serial_cpu(code, pri).decode_batch(sX, sZ, 0.05, 11, "syndrome", want_iters=True, want_q=True))
        assert_same_decode(replay(with_priors), wants[-1], "replay with priors")
    assert not same_floats(wants[0][4], wants[1][4])


@pytest.mark.parametrize("osd", [0, 1])
def test_monte_carlo_counters(osd):
    """hgp_ham with the degenerate check, 4096 samples in batches of 1024: the counters equal counting the CPU
    engine's serial decode of the same samples."""
    code = logical_code("hgp_ham")
    HX, HZ = code_matrices("hgp_ham")
    dec, cpu = q.DecoderGPU(code, 0, engine="sparse"), serial_cpu(code)
    dec.set_option("bp_schedule", 1)
    seed, B, p = 0x51EC0DE, 4096, 0.05
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    bp_only = cpu.decode_batch(sX, sZ, p, 20, "syndrome")[2]
    assert (bp_only & 1).any() and (bp_only & 2).any()  # serial BP still leaves failures in both sectors
    for d in (dec, cpu):
        d.set_option("osd", osd)
        d.set_option("osd_order", 10 if osd else 0)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    if osd:
        assert want["synX"] == want["synZ"] == 0
    got = dec.monte_carlo(seed, 0, B, p, 20, "syndrome", batch=1024)
    assert {k: got[k] for k in want} == want, osd
    assert {"serial", "sparse"} <= dec.last_path() and ("osd" in dec.last_path()) == bool(osd)


def test_option_0_launches_the_flooding_kernels():
    case = ("hgp_ham", "general")
    code = code_of(*case)
    dec, cpu = q.DecoderGPU(code, 0, engine="sparse"), q.DecoderCPU(code)
    sX, sZ = inputs("hgp_ham")
    want = cpu.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    for _ in range(2):
        got = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
        assert dec.last_path() == {"sparse"}
        assert_same_decode(got, want, "option 0")
        dec.set_option("bp_schedule", 1)
        dec.decode_batch(sX, sZ, 0.05, 11, "ref")
        assert "serial" in dec.last_path()
        dec.set_option("bp_schedule", 0)


def test_circulant_handle_refuses():
    from test_priors import code_of as named
    dec = q.DecoderGPU(named("P7"), 0, engine="circulant")
    with pytest.raises(q.QecError, match="QEC_ENGINE_SPARSE"):
        dec.set_option("bp_schedule", 1)
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["bp_schedule"], 1) == -4  # QEC_ERR_UNSUPPORTED
    assert dec.get_option("bp_schedule") == 0
    dec.set_option("bp_schedule", 0)
    with pytest.raises(q.QecError, match="QEC_OPT_BP_SCHEDULE"):
        dec.set_option("bp_schedule", 2)
    auto = q.DecoderGPU(named("P61"), 0)
    with pytest.raises(q.QecError, match="sparse"):
        auto.set_option("bp_schedule", 1)
    # a sparse handle: serial and correlated refuse each other, whichever comes second
    sp = q.DecoderGPU(named("P7"), 0, engine="sparse")
    sp.set_option("bp_schedule", 1)
    with pytest.raises(q.QecError, match="QEC_OPT_BP_SCHEDULE"):
        sp.set_option("correlated", 1)
    sp.set_option("bp_schedule", 0)
    sp.set_option("correlated", 2)
    with pytest.raises(q.QecError, match="QEC_OPT_CORRELATED"):
        sp.set_option("bp_schedule", 1)
    assert sp.get_option("bp_schedule") == 0 and sp.get_option("correlated") == 2

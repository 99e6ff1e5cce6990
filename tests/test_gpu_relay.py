"""Relay-BP (set_relay under set_option("bp_method", 1)) on the device: every row of the case table of
test_sparse_shapes.py -- all 36 RELAY kernels of bp_sparse.hip, asserted in test_relay.py -- with the scalar p and with
priors, under every stop rule, with S = 1 and S = 3.  The LDS codes are held to the numpy yardstick of test_relay.py
(the outputs computed there, once), the HBM codes to the CPU engine, which test_relay.py holds to the yardstick.  Then
the gamma = 0 anchor against the MINSUM kernels on the device, packed records in a captured graph replayed after
set_relay has replaced the tables in place, the Monte-Carlo pipeline with and without OSD against the composed _dev
calls, the wave-circulant refusal, the round trip set -> clear -> set and a two-part group.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns.  L = 4 legs, a cap of at most
20 per leg."""
import ctypes

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.gather import pack_records
from test_general_code import assert_same_decode, code_matrices, mixed_syndromes, same_floats
from test_gpu_general_code import count, logical_code
from test_minsum import MS_P, MS_P_REF, minsum_cpu
from test_priors import prior_vectors
from test_relay import GPU_CASES, LEGS, relay_cpu, ryard, tables
from test_sparse_shapes import HBM_CASES, LDS_CASES, P_MAIN, P_REF, case_id, code_of, hbm_inputs, hbm_priors, inputs, matrices

pytestmark = pytest.mark.gpu

F32 = np.float32
_decoders = {}


def gpu(case):
    """One sparse-engine decoder per row of the case table, under min-sum at the default scale; a test sets the
    tables it needs and leaves the handle without tables and without priors."""
    if case not in _decoders:
        _decoders[case] = q.DecoderGPU(code_of(*case), 0, engine="sparse")
        _decoders[case].set_option("bp_method", 1)
    return _decoders[case]


def decode(dec, sX, sZ, p, N, stop):
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
    assert {"minsum", "relay", "sparse"} <= dec.last_path()
    return got


def test_the_case_table_is_the_one_asserted_to_reach_all_36():
    assert set(LDS_CASES + HBM_CASES) == set(GPU_CASES)


# (S, stop, p or None for MS_P, N): every stop rule under both S, N = 0, and the reference stop at both p
SCALAR_RUNS = ((1, "fixed", None, 0), (1, "fixed", None, 1), (1, "fixed", None, 11), (1, "syndrome", None, 20),
               (1, "ref", MS_P_REF, 20), (3, "fixed", None, 11), (3, "syndrome", None, 20), (3, "ref", None, 11))
PRIOR_RUNS = ((1, "fixed", 1), (1, "syndrome", 11), (1, "ref", 11), (3, "fixed", 0), (3, "fixed", 11), (3, "syndrome", 11),
              (3, "ref", 11))  # (S, stop, N)


@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
@pytest.mark.parametrize("kind", ["scalar", "random", "special"])
def test_lds_matches_the_yardstick(case, kind):
    name, _ = case
    dec = gpu(case)
    n = code_of(*case).n
    sX, sZ = inputs(name)
    split = False
    try:
        if kind != "scalar":
            dec.set_priors(*prior_vectors(n, kind))
        runs = SCALAR_RUNS if kind == "scalar" else tuple((S, stop, None, N) for S, stop, N in PRIOR_RUNS)
        for S, stop, p, N in runs:
            dec.set_relay(*tables(n), solutions=S)
            want = ryard(name, kind, stop, N, S, p)
            split |= bool((want[5][0][0] != want[5][1][0]).any())
            got = decode(dec, sX, sZ, 0.3 if kind != "scalar" else (MS_P[name] if p is None else p), N, stop)
            assert np.isfinite(got[4]).all()
            assert_same_decode(got, want, "%s %s S=%d %s N=%d" % (case_id(case), kind, S, stop, N))
    finally:
        dec.set_priors(None, None)
        dec.set_relay(None, None)
    # a row whose sectors end in different legs: one re-initialises its slots or idles while the other runs on
    assert split or kind != "scalar"


@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
def test_hbm_matches_the_cpu_engine(case, priors):
    name, _ = case
    dec = gpu(case)
    code = code_of(*case)
    pri = hbm_priors(name) if priors else None
    sX, sZ = hbm_inputs(name)
    try:
        if pri:
            dec.set_priors(*pri)
        for S, stop, p, N in ((1, "ref", P_REF, 11), (3, "fixed", P_MAIN, 3), (1, "syndrome", P_MAIN, 6), (3, "syndrome", P_MAIN, 6)):
            cpu = relay_cpu(code, S, pri)
            dec.set_relay(*tables(code.n), solutions=S)
            want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            if stop == "syndrome":  # the all-zero row ends every leg at its first test, the all-one row runs every leg out
                assert (want[3].min(axis=0) <= S).all() and (want[3].max(axis=0) == LEGS * N).all(), want[3].tolist()
            assert_same_decode(decode(dec, sX, sZ, p, N, stop), want, "%s priors=%s S=%d %s" % (name, priors, S, stop))
    finally:
        dec.set_priors(None, None)
        dec.set_relay(None, None)


@pytest.mark.parametrize("case", [("hgp_ham", "general"), ("dense32", "general"), ("tall", "general"), ("r3-3-6-13", "graph"),
                                  ("wide*15", "general")], ids=case_id)
def test_gamma_zero_is_the_minsum_kernel(case):
    """L = 1 and gamma = 0: every output bit of the RELAY kernel equals the MINSUM kernel's on the device."""
    name, _ = case
    dec = gpu(case)
    n = code_of(*case).n
    sX, sZ = hbm_inputs(name) if case in HBM_CASES else inputs(name)
    zero = np.zeros((1, n), dtype=F32)
    try:
        for priors in (False, True):
            if priors:
                dec.set_priors(*(hbm_priors(name) if case in HBM_CASES else prior_vectors(n, "special")))
            for stop, N in (("fixed", 0), ("fixed", 5), ("syndrome", 11), ("ref", 11)):
                dec.set_relay(None, None)
                want = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                assert "relay" not in dec.last_path() and "minsum" in dec.last_path()
                for S in (1, 3):
                    dec.set_relay(zero, zero, solutions=S)
                    assert_same_decode(decode(dec, sX, sZ, 0.05, N, stop), want, "%s %s N=%d S=%d" % (name, stop, N, S))
    finally:
        dec.set_priors(None, None)
        dec.set_relay(None, None)


def test_packed_records_in_a_captured_graph_read_new_tables():
    """decode_batch_packed_dev with the tables set before the capture: the replay's records equal the direct call's and
    the CPU engine's, the path carries QEC_PATH_RELAY, and a replay after a second set_relay (the same L and S) decodes
    with the new tables: they are rewritten in place, and neither set_option nor the call allocates."""
    import torch
    name, B = "mid", 129
    code = code_of(name, "general")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    dec.set_option("bp_method", 1)
    first = tables(code.n)
    second = (q.relay_gammas(code.n, LEGS, gamma0=0.3, seed=5), q.relay_gammas(code.n, LEGS, gamma0=-0.2, seed=6))
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(matrices(name), 77, B, (0.01, 0.05))
    tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
    rec = torch.zeros((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    it = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    qf = torch.zeros((B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    outs = (rec, it, qf)

    def run(how):
        for t in outs:
            t.zero_()
        how()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    def same(got, want, what):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_floats(got[2], want[2]), what

    def host(tab):
        cpu = minsum_cpu(code)
        cpu.set_relay(*tab, solutions=3)
        w = cpu.decode_batch(sX, sZ, 0.05, 11, "syndrome", want_iters=True, want_q=True)
        return [pack_records(w[0], w[1], w[2]), w[3], w[4]]

    dec.set_relay(*first, solutions=3)  # allocates the device table and the kernels' state before the capture
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_batch_packed_dev(tX, tZ, 0.05, 11, "syndrome", rec, iters=it, q=qf, stream=s)
    assert {"minsum", "relay", "sparse", "records"} <= dec.last_path()
    assert dec.get_option("last_path") & q.PATH["relay"] == 4096
    wants = []
    for tab in (first, second):
        dec.set_relay(*tab, solutions=3)  # rewrites the table the captured kernel reads
        wants.append(run(lambda: dec.decode_batch_packed_dev(tX, tZ, 0.05, 11, "syndrome", rec, iters=it, q=qf)))
        same(run(g.replay), wants[-1], "replay")
        same(wants[-1], host(tab), "the direct call against the CPU engine")
    assert not np.array_equal(wants[0][0], wants[1][0]) or not same_floats(wants[0][2], wants[1][2])


@pytest.mark.parametrize("osd", [0, 1])
def test_monte_carlo_counters(osd):
    """hgp_ham with the degenerate check, seed 1, 4096 samples at p = 0.05 under the syndrome stop, S = 3: every counter
    of monte_carlo equals the count over the composed _dev calls' outputs (decode_batch on the same samples, with the
    OSD stage when on) and over DecoderCPU's; the relay leaves fewer sectors to the stage than plain min-sum."""
    code = logical_code("hgp_ham")
    HX, HZ = code_matrices("hgp_ham")
    dec, cpu = q.DecoderGPU(code, 0, engine="sparse"), relay_cpu(code, 3)
    dec.set_option("bp_method", 1)
    dec.set_relay(*tables(code.n), solutions=3)
    seed, B, p = 1, 4096, 0.05
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    plain = minsum_cpu(code).decode_batch(sX, sZ, p, 20, "syndrome")[2]
    relay_only = cpu.decode_batch(sX, sZ, p, 20, "syndrome")[2]
    failed = lambda f: int(((f & 1) != 0).sum() + ((f & 2) != 0).sum())  # noqa: E731
    assert 0 < failed(relay_only) < failed(plain)
    for d in (dec, cpu):
        d.set_option("osd", osd)
        d.set_option("osd_order", 10 if osd else 0)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    composed = dec.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    assert_same_decode(composed, (eX, eZ, fl, it), "decode_batch", with_q=False)
    if osd:
        assert want["synX"] == want["synZ"] == 0
    got = dec.monte_carlo(seed, 0, B, p, 20, "syndrome", batch=1024)
    assert {k: got[k] for k in want} == want, osd
    assert {"minsum", "relay", "sparse"} <= dec.last_path() and ("osd" in dec.last_path()) == bool(osd)
    assert dec.get_option("osd_sectors") == cpu.get_option("osd_sectors") == (failed(relay_only) if osd else 0)


def test_circulant_handle_refuses():
    from test_priors import code_of as named
    code = named("P7")
    dec = q.DecoderGPU(code, 0)  # engine auto: the wave-circulant engine
    g = tables(code.n)
    with pytest.raises(q.QecError, match="create the decoder with QEC_ENGINE_SPARSE"):
        dec.set_relay(*g)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert q.lib().qec_decoder_set_relay(dec._h, ptr(g[0]), ptr(g[1]), LEGS, 1) == -4  # QEC_ERR_UNSUPPORTED
    assert q.lib().qec_decoder_set_relay(dec._h, ptr(g[0]), ptr(g[1]), LEGS, 0) == -1  # an illegal value: QEC_ERR_ARG
    assert dec.get_relay() is None
    dec.set_relay(None, None)  # clearing is always accepted
    assert dec.get_relay() is None


def test_round_trip_set_clear_set():
    case = ("hgp_ham", "general")
    code = code_of(*case)
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    sX, sZ = inputs("hgp_ham")
    plain = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    path = dec.get_option("last_path")
    dec.set_relay(*tables(code.n), solutions=3)
    first = decode(dec, sX, sZ, 0.05, 20, "syndrome")
    assert_same_decode(first, ryard("hgp_ham", "scalar", "syndrome", 20, 3), "set")
    got = dec.get_relay()
    assert got[2] == 3 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[:2], tables(code.n)))
    dec.set_relay(None, None)
    assert dec.get_relay() is None
    again = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert dec.get_option("last_path") == path
    assert_same_decode(again, plain, "set -> clear")
    dec.set_relay(*tables(code.n), solutions=3)
    assert_same_decode(decode(dec, sX, sZ, 0.05, 20, "syndrome"), first, "set -> clear -> set")
    # tables under the product rule: the handle without tables
    dec.set_option("bp_method", 0)
    prod = dec.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True, want_q=True)
    assert dec.last_path() == {"sparse"}
    assert_same_decode(prod, q.DecoderGPU(code, 0, engine="sparse").decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True,
                                                                              want_q=True), "method 0")


def test_a_two_part_group_decodes_like_one_part():
    name = "mid"
    code = code_of(name, "general")
    one, two = gpu((name, "general")), q.DecoderGPU(code, devices=[0, 0])
    two.set_option("bp_method", 1)
    g = tables(code.n)
    sX, sZ = inputs(name)
    pri = prior_vectors(code.n, "special")
    try:
        one.set_relay(*g, solutions=3)
        two.set_relay(*g, solutions=3)
        for part in two.parts():
            got = part.get_relay()
            assert got[2] == 3 and np.array_equal(got[0], g[0]) and np.array_equal(got[1], g[1])
        for priors in (None, pri):
            if priors:
                one.set_priors(*priors)
                two.set_priors(*priors)
            for stop, N in (("fixed", 5), ("syndrome", 11)):
                a = one.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                b = two.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
                assert_same_decode(b, a, "%s %s" % (stop, priors is not None))
                assert "relay" in two.last_path()
        assert_same_decode(b, ryard(name, "special", "syndrome", 11, 3), "the group's last decode against the yardstick")
        two.set_relay(None, None)
        assert all(p.get_relay() is None for p in two.parts())
    finally:
        one.set_priors(None, None)
        one.set_relay(None, None)

"""Every instantiation of the sparse-graph BP kernels on the device: the case table of test_sparse_shapes.py
(72 of 72 decode kernels of bp_sparse.hip, asserted there) with the scalar p and with priors under every stop
rule.  describe() confirms the instantiation that the restated plan predicts; the LDS codes are held to the CPU
engine and to the numpy yardstick / the oracle, the HBM codes to the CPU engine and, under the fixed stop, to the
block decomposition of the small code's yardstick.  On `wide` (row weights to 22, column weights to 14) also the
packed records, a captured graph replayed under two prior vectors, the fused sampler and the Monte-Carlo pipeline
with and without OSD.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns (NaN matches NaN)."""
import contextlib
import re

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.gather import pack_records
from test_general_code import assert_same_decode, mixed_syndromes, same_floats
from test_gpu_general_code import count
from test_priors import VECTORS, prior_vectors
from test_sparse_shapes import (HBM_CASES, HBM_N, HBM_STOPS, LARGE_REGULAR, LDS_CASES, P_MAIN, PRIOR_CASES, PRIOR_YARDSTICK,
                                REPLICATED, SCALAR_CASES, STOPS, assert_hbm_stops, assert_not_vacuous,
                                block_reference, block_rows, case_id, code_of, hbm_inputs, hbm_priors, inputs,
                                instance_of, matrices, oracles, plan_of, prior_cases, scalar_reference,
                                yardstick_priors)

pytestmark = pytest.mark.gpu

_decoders = {}


def gpu(case):
    """One sparse-engine decoder per row of the case table (priors are set through priors_set alone)."""
    if case not in _decoders:
        _decoders[case] = q.DecoderGPU(code_of(*case), 0, engine="sparse")
    return _decoders[case]


@contextlib.contextmanager
def priors_set(pri, *decoders):
    """The priors on every decoder, cleared again whatever the body does: a failed comparison must not leave them
    on a cached decoder for the tests behind it."""
    try:
        for d in decoders:
            d.set_priors(*pri)
        yield
    finally:
        for d in decoders:
            d.set_priors(None, None)


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return oracles(tmp_path_factory.mktemp("gpu_sparse_shapes"))


def decode(dec, sX, sZ, p, N, stop):
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
    assert "sparse" in dec.last_path()
    return got


# ---- which kernel runs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LDS_CASES + HBM_CASES, ids=case_id)
def test_describe_confirms_the_predicted_instantiation(case):
    name, route = case
    code = code_of(*case)
    plan = plan_of(code, route == "general")
    d = gpu(case).describe()
    if route == "general":
        assert d.startswith("sparse-general %s threads=%d " % (plan["mem"], plan["threads"])), d
        assert " D=%d dv=%d/%d " % ((plan["D"],) + plan["dv"]) in d, d
    else:
        assert d.startswith("sparse-graph %s " % plan["mem"]), d
        assert " dc=%d dv=%d/%d " % ((plan["D"],) + plan["dv"]) in d, d
        if name in LARGE_REGULAR:  # P > 64 has no wave-circulant kernel: auto is the sparse engine
            assert q.DecoderGPU(code, 0).describe() == d
    # the kernel behind that line, for every stop rule and both prior forms
    kernel = "general" if d.startswith("sparse-general") else "regular"
    mem = "hbm" if " hbm " in d else "lds"
    for pri in (False, True):
        for stop in STOPS:
            assert instance_of(code, route == "general", pri, stop) == (kernel, plan["shape"], mem, pri, stop)


# ---- LDS codes: GPU = CPU engine = yardstick / oracle -----------------------------------------------------------------
@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
def test_lds_scalar(case, orc):
    name, _ = case
    dec, cpu = gpu(case), q.DecoderCPU(code_of(*case))
    sX, sZ = inputs(name)
    assert_not_vacuous(name, orc)
    for stop, p, N in SCALAR_CASES:
        what = "%s %s p=%g N=%d" % (case_id(case), stop, p, N)
        got = decode(dec, sX, sZ, p, N, stop)
        assert_same_decode(got, cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True), what + " vs the CPU engine")
        assert_same_decode(got, scalar_reference(name, stop, p, N, orc), what + " vs the reference")


@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
@pytest.mark.parametrize("kind", VECTORS)
def test_lds_priors(case, kind):
    """Every stop and every N of NS against the CPU engine; against the numpy yardstick where the host module
    computes it (prior_cases: the regular codes' yardstick runs N = 1 and 11 only)."""
    name, _ = case
    code = code_of(*case)
    dec, cpu = gpu(case), q.DecoderCPU(code)
    sX, sZ = inputs(name)
    with priors_set(prior_vectors(code.n, kind), dec, cpu):
        for k, stop, N in PRIOR_CASES:
            if k != kind:
                continue
            what = "%s %s %s N=%d" % (case_id(case), kind, stop, N)
            got = decode(dec, sX, sZ, 0.3, N, stop)  # p is not used
            want = cpu.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)
            assert_same_decode(got, want, what + " vs the CPU engine")
            if name in PRIOR_YARDSTICK and (k, stop, N) in prior_cases(name):
                assert_same_decode(got, yardstick_priors(name, kind, stop, N), what + " vs the yardstick")
    assert dec.get_priors() is None


# ---- HBM codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
def test_hbm_matches_cpu_engine(case, priors):
    name, _ = case
    dec, cpu = gpu(case), q.DecoderCPU(code_of(*case))
    sX, sZ = hbm_inputs(name)
    scalar = {}
    for stop, p, N in HBM_STOPS:
        scalar[stop] = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
        assert_hbm_stops(name, stop, N, scalar[stop][3])
    with priors_set(hbm_priors(name) if priors else (None, None), dec, cpu):
        for stop, p, N in HBM_STOPS:
            want = cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True) if priors else scalar[stop]
            if priors:  # the priors matter: the reference is not the scalar decode
                assert not same_floats(want[4], scalar[stop][4]), (name, stop)
            assert_same_decode(decode(dec, sX, sZ, p, N, stop), want, "%s priors=%s %s" % (name, priors, stop))


@pytest.mark.parametrize("name", sorted(REPLICATED))
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
def test_hbm_block_decomposition(name, priors):
    """A reference for the HBM kernels that does not go through the CPU engine."""
    dec = gpu((name, "general"))
    sX, sZ = block_rows(name)[2:]
    with priors_set(hbm_priors(name) if priors else (None, None), dec):
        assert_same_decode(decode(dec, sX, sZ, P_MAIN, HBM_N, "fixed"), block_reference(name, priors),
                           "%s priors=%s" % (name, priors))


@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
def test_hbm_workgroups_reuse_their_scratch_slice(case):
    """More rows than the grid (4 workgroups per CU): zero syndromes except three sampled rows at the front and
    two past the grid, so a workgroup decodes a non-trivial row after a trivial one in the same slice."""
    import torch
    name, route = case
    dec, cpu = gpu(case), q.DecoderCPU(code_of(*case))
    grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    if route == "general":
        assert int(re.search(r" grid=(\d+) ", dec.describe()).group(1)) == grid
    B = grid + 5
    hX, hZ = hbm_inputs(name)
    sX, sZ = np.zeros((B, hX.shape[1]), dtype=np.uint8), np.zeros((B, hZ.shape[1]), dtype=np.uint8)
    rows = [0, 1, 2, grid + 1, grid + 3]
    sX[rows], sZ[rows] = hX[:5], hZ[:5]
    want = cpu.decode_batch(sX, sZ, P_MAIN, 20, "syndrome", want_iters=True)
    assert (want[3][rows] == 20).any(axis=0).all() and (np.delete(want[3], rows, axis=0) == 1).all()
    got = dec.decode_batch(sX, sZ, P_MAIN, 20, "syndrome", want_iters=True)
    assert "sparse" in dec.last_path()
    assert_same_decode(got, want, "%s B=%d" % (name, B), with_q=False)


# ---- packed records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B", [(("wide", "general"), 1), (("wide", "general"), 63), (("wide", "general"), 257),
                                    (("r3-9-20-7", "graph"), 1), (("r3-9-20-7", "graph"), 63),
                                    (("r3-9-20-7", "graph"), 257), (("wide*15", "general"), 9)],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_packed_records(case, B):
    name, _ = case
    dec, cpu = gpu(case), q.DecoderCPU(code_of(*case))
    if name in REPLICATED:
        sX, sZ = hbm_inputs(name)
    else:
        sX, sZ = mixed_syndromes(matrices(name), 1000 + B, B + 3, (0.01, 0.05))
        sX, sZ = sX[-B:], sZ[-B:]  # keeps the special rows
    for stop, N in (("ref", 20), ("fixed", 11), ("syndrome", 20)):
        want = cpu.decode_batch(sX, sZ, P_MAIN, N, stop, want_iters=True)
        rec, it = dec.decode_batch_packed(sX, sZ, P_MAIN, N, stop, want_iters=True)
        assert "sparse" in dec.last_path()
        assert np.array_equal(rec, pack_records(want[0], want[1], want[2])) and np.array_equal(it, want[3])


# ---- graph capture ------------------------------------------------------------------------------------------------------------
def test_wide_decodes_in_a_graph_with_priors():
    """The PRIORS (32,16) kernels read the prior buffer at replay time."""
    import torch
    name, B = "wide", 257
    code = code_of(name, "general")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    assert dec.describe().startswith("sparse-general lds threads=256 "), dec.describe()
    cpu = q.DecoderCPU(code)
    first = prior_vectors(code.n, "random")
    second = prior_vectors(code.n, "special", seed=7)
    dec.set_priors(*first)  # allocates the device buffer before the capture
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(matrices(name), 77, B, (0.01, 0.05))
    tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
    eX = torch.zeros((B, code.n), dtype=torch.uint8, device=dev)
    eZ, fl = torch.zeros_like(eX), torch.zeros(B, dtype=torch.uint8, device=dev)
    it = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    qf = torch.zeros((B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    rec = torch.zeros((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_batch_dev(tX, tZ, 0.05, 11, "ref", eX, eZ, fl, iters=it, q=qf, stream=s)
            dec.decode_batch_packed_dev(tX, tZ, 0.05, 11, "ref", rec, stream=s)
    assert "sparse" in dec.last_path()
    wants = []
    for pri in (first, second):
        dec.set_priors(*pri)  # rewrites the buffer the captured kernels read
        cpu.set_priors(*pri)
        want = cpu.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
        wants.append(want)
        for t in (eX, eZ, fl, it, qf, rec):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same_decode([t.cpu().numpy() for t in (eX, eZ, fl, it, qf)], want, "graph replay")
        assert np.array_equal(rec.cpu().numpy(), pack_records(want[0], want[1], want[2]))
    assert not np.array_equal(wants[0][4].view(np.uint32), wants[1][4].view(np.uint32))


# ---- one level up, on wide ------------------------------------------------------------------------------------------------------
_logical = {}


def wide_logical():
    if "wide" not in _logical:
        _logical["wide"] = code_of("wide", "general").with_logical("degenerate")
    return _logical["wide"]


def test_wide_sample_syndrome_dev_matches_numpy():
    """The varEdge walk of the fused sampler with dc = 22 and dvZ = 14."""
    import torch
    code = wide_logical()
    HX, HZ = matrices("wide")
    dec = q.DecoderGPU(code, 0)
    dev = torch.device("cuda", 0)
    B, lo, seed, p = 5000, 300001, 5, 0.05
    sX, sZ, errp = (torch.empty((B, w), dtype=torch.uint8, device=dev)
                    for w in (code.numEqsX, code.numEqsZ, 2 * ((code.n + 7) // 8)))
    dec.sample_syndrome_dev(seed, lo, p, sX, sZ, errp)
    x, z = depolarizing(seed, lo, B, code.n, p)
    assert np.array_equal(sX.cpu().numpy(), (x @ HX.T) & 1)
    assert np.array_equal(sZ.cpu().numpy(), (z @ HZ.T) & 1)
    exp = np.concatenate([np.packbits(x, axis=1, bitorder="little"), np.packbits(z, axis=1, bitorder="little")], 1)
    assert np.array_equal(errp.cpu().numpy(), exp)


@pytest.mark.parametrize("osd", [0, 1])
def test_wide_monte_carlo_counters(osd):
    code = wide_logical()
    HX, HZ = matrices("wide")
    dec, cpu = q.DecoderGPU(code, 0), q.DecoderCPU(code)
    seed, B, p = 0x51EC0DE, 4096, 0.02
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    bp_only = cpu.decode_batch(sX, sZ, p, 20, "syndrome")[2]
    assert (bp_only & 1).any() and (bp_only & 2).any()  # BP leaves failures in both sectors
    for d in (dec, cpu):
        d.set_option("osd", osd)
        d.set_option("osd_order", 10 if osd else 0)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    if osd:
        assert want["synX"] == want["synZ"] == 0
    got = dec.monte_carlo(seed, 0, B, p, 20, "syndrome", batch=1024)
    assert {k: got[k] for k in want} == want, osd
    assert ("osd" in dec.last_path()) == bool(osd)

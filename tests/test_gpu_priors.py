"""Per-qubit priors on the GPU: the PRIORS instantiations of bp_sparse_kernel, GENERAL (general codes) and
regular (regular codes through engine="sparse"), against the CPU engine and the numpy yardstick of
test_priors.py, the independent sampler against its numpy restatement, and the Monte-Carlo pipeline with priors
against a host recount."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from qec_ldpc_amd.gather import pack_records
from test_general_code import NS, STOPS, assert_same_decode, code_matrices, general_code, mixed_syndromes
from test_gpu_general_code import count, logical_code
from test_priors import F32, VECTORS, code_of, independent, inputs, matrices, prior_vectors, yardstick_priors

pytestmark = pytest.mark.gpu

GENERAL = ("surf3", "hgp_ham", "ham_rep3+1")     # bp_sparse_kernel, GENERAL
REGULAR_SPARSE = ("G13", "P7")                    # bp_sparse_kernel, regular
_decoders = {}


def gpu(name):
    """One sparse-engine decoder per test code (priors are set by each test)."""
    if name not in _decoders:
        _decoders[name] = q.DecoderGPU(code_of(name), 0, engine="sparse")
    return _decoders[name]


def test_engines_under_test():
    for name in GENERAL:
        assert gpu(name).describe().startswith("sparse-general "), gpu(name).describe()
    for name in REGULAR_SPARSE + ("P61",):
        assert gpu(name).describe().startswith("sparse-graph "), gpu(name).describe()


# ---- GPU = CPU engine = yardstick -------------------------------------------------------------------------
@pytest.mark.parametrize("name", GENERAL + REGULAR_SPARSE)
@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("kind", VECTORS)
def test_gpu_matches_prior_yardstick_and_cpu_engine(name, stop, kind):
    code = code_of(name)
    dec, cpu = gpu(name), q.DecoderCPU(code)
    pX, pZ = prior_vectors(code.n, kind)
    dec.set_priors(pX, pZ)
    cpu.set_priors(pX, pZ)
    sX, sZ = inputs(name)
    for N in NS:
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert "sparse" in dec.last_path()
        assert_same_decode(got, cpu.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True),
                           "%s %s %s N=%d vs the CPU engine" % (name, kind, stop, N))
        assert_same_decode(got, yardstick_priors(name, kind, stop, N),
                           "%s %s %s N=%d vs the yardstick" % (name, kind, stop, N))


@pytest.mark.parametrize("name", ["hgp_ham", "ham_rep3+1", "G13"])
@pytest.mark.parametrize("B", [1, 63, 257])
def test_ragged_batches_byte_and_packed(name, B):
    """Fewer rows than workgroups and rows that a workgroup loops over; the packed records are the byte outputs
    packed."""
    code = code_of(name)
    sX, sZ = mixed_syndromes(matrices(name), 2000 + B, B + 3, (0.03, 0.1))
    sX, sZ = sX[-B:], sZ[-B:]  # keeps the special rows
    dec, cpu = gpu(name), q.DecoderCPU(code)
    pX, pZ = prior_vectors(code.n, "special")
    dec.set_priors(pX, pZ)
    cpu.set_priors(pX, pZ)
    for stop, N in (("ref", 20), ("fixed", 11), ("syndrome", 20)):
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, cpu.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True),
                           "%s B=%d %s" % (name, B, stop))
        rec, it = dec.decode_batch_packed(sX, sZ, 0.05, N, stop, want_iters=True)
        assert np.array_equal(rec, pack_records(got[0], got[1], got[2])) and np.array_equal(it, got[3])


def test_workgroups_loop_over_rows():
    """More rows than the grid of the regular kernel holds at once (one workgroup per row up to the plan's grid)."""
    name, B = "G13", 9000
    code = code_of(name)
    sX, sZ = mixed_syndromes(matrices(name), 5, B, (0.02, 0.06))
    dec, cpu = gpu(name), q.DecoderCPU(code)
    pX, pZ = prior_vectors(code.n, "random")
    dec.set_priors(pX, pZ)
    cpu.set_priors(pX, pZ)
    got = dec.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
    assert_same_decode(got, cpu.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True), "G13 B=9000")


@pytest.mark.parametrize("stop", STOPS)
def test_uniform_priors_equal_the_scalar_path_on_p61(stop):
    """Ties the PRIORS kernels to the oracle-pinned scalar path at the largest LDS footprint."""
    code = code_of("P61")
    dec = gpu("P61")
    sX, sZ = mixed_syndromes(matrices("P61"), 3, 96, (0.01, 0.04))
    p = 0.02
    uni = F32(2.0) / F32(3.0) * F32(p)
    for N in (1, 11, 50):
        dec.set_priors(None, None)
        want = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
        dec.set_priors(uni, uni)
        assert_same_decode(dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True), want,
                           "P61 %s N=%d" % (stop, N))
    dec.set_priors(None, None)
    assert code.n == 610


def test_circulant_handle_refuses():
    dec = q.DecoderGPU(code_of("P7"), 0, engine="circulant")
    with pytest.raises(q.QecError, match="sparse"):
        dec.set_priors(0.01, 0.02)
    assert dec.get_priors() is None
    dec.set_priors(None, None)  # clearing nothing is no error
    auto = q.DecoderGPU(code_of("P61"), 0)
    with pytest.raises(q.QecError, match="QEC_ENGINE_SPARSE"):
        auto.set_priors(0.01, 0.02)


def test_validation_on_a_gpu_handle():
    dec = gpu("surf3")
    pX, pZ = prior_vectors(13, "random")
    dec.set_priors(pX, pZ)
    bad = pZ.copy()
    bad[4] = np.nan
    with pytest.raises(q.QecError, match=r"priorZ\[4\]"):
        dec.set_priors(pX, bad)
    gX, gZ = dec.get_priors()
    assert np.array_equal(gX, pX) and np.array_equal(gZ, pZ)


# ---- graph capture ----------------------------------------------------------------------------------------------
def test_dev_decodes_in_a_graph_with_priors():
    import torch
    name, B = "hgp_ham", 257
    code = general_code(name)
    dec = q.DecoderGPU(code, 0, max_batch=B)
    cpu = q.DecoderCPU(code)
    first = prior_vectors(code.n, "random")
    second = prior_vectors(code.n, "special", seed=7)
    dec.set_priors(*first)  # allocates the device buffer before the capture
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(code_matrices(name), 77, B, (0.05,))
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
    for pri in (first, second):
        dec.set_priors(*pri)  # rewrites the buffer the captured kernels read
        cpu.set_priors(*pri)
        want = cpu.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
        for t in (eX, eZ, fl, it, qf, rec):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same_decode([t.cpu().numpy() for t in (eX, eZ, fl, it, qf)], want, "graph replay")
        assert np.array_equal(rec.cpu().numpy(), pack_records(want[0], want[1], want[2]))


# ---- the independent sampler ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["surf3", "hgp_ham"])
@pytest.mark.parametrize("start", [0, (1 << 32) - 64])
def test_sample_independent_dev_matches_numpy(name, start):
    import torch
    code = general_code(name)
    HX, HZ = code_matrices(name)
    dec = gpu(name)
    dev = torch.device("cuda", 0)
    B, seed = 130, 0xC0FFEE1234567
    pX, pZ = prior_vectors(code.n, "special")
    pX[1] = F32(2.0) ** -32  # thr = 1
    dec.set_priors(pX, pZ)
    x, z = independent(seed, start, B, pX, pZ)
    assert x.any() and z.any() and not x.all()
    tx = torch.full((B, code.n), 7, dtype=torch.uint8, device=dev)
    tz = torch.full((B, code.n), 7, dtype=torch.uint8, device=dev)
    dec.sample_independent_dev(seed, start, tx, tz)
    assert np.array_equal(tx.cpu().numpy(), x) and np.array_equal(tz.cpu().numpy(), z)
    # a shard drawn alone
    dec.sample_independent_dev(seed, start + 100, tx[:30], tz[:30])
    assert np.array_equal(tx[:30].cpu().numpy(), x[100:]) and np.array_equal(tz[:30].cpu().numpy(), z[100:])
    # the fused front end: the same errors' syndromes and packed errors (p is not used)
    sX, sZ, errp = (torch.empty((B, w), dtype=torch.uint8, device=dev)
                    for w in (code.numEqsX, code.numEqsZ, 2 * ((code.n + 7) // 8)))
    dec.sample_syndrome_dev(seed, start, 0.9, sX, sZ, errp)
    assert np.array_equal(sX.cpu().numpy(), (x @ HX.T) & 1)
    assert np.array_equal(sZ.cpu().numpy(), (z @ HZ.T) & 1)
    exp = np.concatenate([np.packbits(x, axis=1, bitorder="little"), np.packbits(z, axis=1, bitorder="little")], 1)
    assert np.array_equal(errp.cpu().numpy(), exp)


def test_sample_independent_dev_needs_priors():
    import torch
    code = general_code("surf3")
    dec = q.DecoderGPU(code, 0)
    t = torch.zeros((4, code.n), dtype=torch.uint8, device=torch.device("cuda", 0))
    with pytest.raises(q.QecError, match="no priors"):
        dec.sample_independent_dev(1, 0, t, t.clone())


# ---- Monte-Carlo ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("osd", [0, 1])
def test_monte_carlo_with_priors(osd):
    """Every counter equals a host recount from the restated samples, decode_batch and check_logical; a two-part
    handle on device 0 gives the same counters."""
    name, seed, n_samples = "hgp_ham", 0xB1A5ED, 1000
    code = logical_code(name)
    HX, HZ = code_matrices(name)
    pX, pZ = prior_vectors(code.n, "random")
    one, two = q.DecoderGPU(code, 0), q.DecoderGPU(code, devices=[0, 0])
    for d in (one, two):
        d.set_priors(pX, pZ)
        d.set_option("osd", osd)
        d.set_option("osd_order", 10 if osd else 0)
    assert all(np.array_equal(a, b) for a, b in zip(two.parts()[1].get_priors(), (pX, pZ)))
    x, z = independent(seed, 0, n_samples, pX, pZ)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    eX, eZ, fl, it, _ = one.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True)
    want = count(code, x, z, eX, eZ, fl, it)
    plain = q.DecoderCPU(code)
    plain.set_priors(pX, pZ)
    bp_only = plain.decode_batch(sX, sZ, 0.05, 20, "syndrome")[2]
    assert (bp_only & 3).any()  # BP leaves failures for the OSD stage to repair
    if osd:
        assert want["synX"] == want["synZ"] == 0
    else:
        assert np.array_equal(fl, bp_only)
    for d in (one, two):
        got = d.monte_carlo(seed, 0, n_samples, 0.7, 20, "syndrome", batch=384)
        assert {k: got[k] for k in want} == want, (osd, d.describe())
        assert ("osd" in one.last_path()) == bool(osd)

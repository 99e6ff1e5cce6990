"""The correlated form (QEC_OPT_CORRELATED) and the per-qubit Pauli channel on the device: all 36 CORR instantiations
of bp_sparse.hip through the case tables of test_sparse_shapes.py (asserted to cover them in test_correlated.py),
held to the CPU engine, to the numpy yardstick of test_correlated.py and, for the HBM codes under the fixed stop, to
the block decomposition; the identities; the device contract (graph capture, two streams, the wave-circulant
refusal); the Pauli sampler against its numpy restatement; the Monte-Carlo pipeline against a host recount.

Bit for bit everywhere: eX, eZ, flags, iteration counts and q_final as uint32 patterns.  There is no tolerance."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from qec_ldpc_amd.gather import pack_records
from test_correlated import (OPTIONS, P_SCALAR, assert_not_vacuous, channel_tables, corr_instance_of, corr_yardstick,
                             first_sector_equal, pauli_samples, pauli_vectors, scalar_tables, yardstick)
from test_general_code import assert_same_decode, code_matrices, mixed_syndromes, same_floats
from test_gpu_general_code import count, logical_code
from test_priors import F32, code_of as prior_code_of, inputs as prior_inputs, prior_vectors
from test_sparse_shapes import (HBM_CASES, HBM_N, HBM_ROWS, HBM_STOPS, LDS_CASES, P_MAIN, P_REF, PINNED, REPLICATED, STOPS,
                                block_rows, case_id, code_of, hbm_inputs, inputs, matrices, plan_of)

pytestmark = pytest.mark.gpu

# (stop, p, N): every stop rule at the cap and below it, N = 0 (no iteration), 1 (the first iteration is the last)
# and 2, and the ref stop at the p where it ends sectors at its tests of iterations 1 and 11
LDS_RUNS = (("ref", P_REF, 20), ("ref", P_MAIN, 11), ("fixed", P_MAIN, 11), ("fixed", P_MAIN, 0), ("fixed", P_MAIN, 1),
            ("syndrome", P_MAIN, 20), ("syndrome", P_MAIN, 2))
YARDSTICK_CODES = ("hgp_ham", "mid")  # LDS codes also held to the numpy yardstick (fixed and syndrome stop, N = 11)
_decoders = {}


def gpu(case):
    """One sparse-engine decoder per row of the case table; every test leaves it without priors and at option 0."""
    if case not in _decoders:
        _decoders[case] = q.DecoderGPU(code_of(*case), 0, engine="sparse")
    return _decoders[case]


def reset(*decoders):
    for d in decoders:
        d.set_pauli_channel(None, None, None)
        d.set_option("correlated", 0)


def channel_of(name):
    """A replicated code: the small code's random channel tiled over the blocks; any other: its own."""
    if name in REPLICATED:
        base, r = REPLICATED[name]
        return tuple(np.tile(a, r) for a in pauli_vectors(matrices(base)[0].shape[1], "random"))
    return pauli_vectors(PINNED[name][0], "random")


def decode(dec, sX, sZ, p, N, stop, option):
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
    path = dec.last_path()
    assert "sparse" in path and ("correlated" in path) == bool(option)
    return got


def run_case(case, sX, sZ, runs, with_yardstick=False):
    name, route = case
    code = code_of(*case)
    dec, cpu = gpu(case), q.DecoderCPU(code)
    described = dec.describe()
    seen = set()
    try:
        for mode in ("scalar", "channel"):
            for d in (dec, cpu):
                if mode == "channel":
                    d.set_pauli_channel(*channel_of(name))
            for option in OPTIONS:
                dec.set_option("correlated", option)
                cpu.set_option("correlated", option)
                assert dec.describe() == described  # the plan is the scalar plan's
                for stop, p, N in runs:
                    what = "%s %s option %d %s p=%g N=%d" % (case_id(case), mode, option, stop, p, N)
                    got = decode(dec, sX, sZ, p, N, stop, option)
                    assert_same_decode(got, cpu.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True),
                                       what + " vs the CPU engine")
                    seen.add(corr_instance_of(code, route == "general", stop))
                    if with_yardstick and N == 11 and stop != "ref":
                        tab = scalar_tables(p, code.n) if mode == "scalar" else channel_tables(*channel_of(name))
                        key = (name, mode, stop, p, N)
                        if key not in _yard:
                            _yard[key] = corr_yardstick(*matrices(name), sX, sZ, tab, N, stop)
                        assert_same_decode(got, _yard[key][option], what + " vs the yardstick")
    finally:
        reset(dec, cpu)
    plan = plan_of(code, route == "general")
    assert seen == {(plan["kernel"], plan["shape"], plan["mem"], stop) for stop in STOPS}


_yard = {}


# ---- all 36 instantiations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LDS_CASES, ids=case_id)
def test_lds_instantiations(case):
    run_case(case, *inputs(case[0]), LDS_RUNS, with_yardstick=case[0] in YARDSTICK_CODES)


@pytest.mark.parametrize("case", HBM_CASES, ids=case_id)
def test_hbm_instantiations(case):
    run_case(case, *hbm_inputs(case[0]), HBM_STOPS)


@pytest.mark.parametrize("name", sorted(REPLICATED))
@pytest.mark.parametrize("mode", ["scalar", "channel"])
def test_hbm_block_decomposition(name, mode):
    """Conditioning is per qubit, so under the fixed stop a replicated code still decodes block by block: the small
    code's yardstick, put together as block_reference of test_sparse_shapes.py does, is a reference for the HBM
    CORR kernels that does not go through the CPU engine."""
    base, r = REPLICATED[name]
    HX, HZ = matrices(base)
    sx, sz, sX, sZ = block_rows(name)
    tab = scalar_tables(P_MAIN, HX.shape[1]) if mode == "scalar" else channel_tables(*pauli_vectors(HX.shape[1], "random"))
    small = corr_yardstick(HX, HZ, sx, sz, tab, HBM_N, "fixed")
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    EX = HX.shape[0] * D
    dec = gpu((name, "general"))
    try:
        if mode == "channel":
            dec.set_pauli_channel(*channel_of(name))
        for option in OPTIONS:
            s = small[option]
            qs = s[4].reshape(HBM_ROWS, r, -1)
            qf = np.concatenate([qs[:, :, :EX].reshape(HBM_ROWS, -1), qs[:, :, EX:].reshape(HBM_ROWS, -1)], axis=1)
            want = (s[0].reshape(HBM_ROWS, -1), s[1].reshape(HBM_ROWS, -1),
                    np.bitwise_or.reduce(s[2].reshape(HBM_ROWS, r), axis=1),
                    np.ascontiguousarray(s[3].reshape(HBM_ROWS, r, 2)[:, 0]), np.ascontiguousarray(qf))
            dec.set_option("correlated", option)
            assert_same_decode(decode(dec, sX, sZ, P_MAIN, HBM_N, "fixed", option), want, "%s %s option %d" % (name, mode, option))
    finally:
        reset(dec)


@pytest.mark.parametrize("case,B", [(("wide", "general"), 1), (("wide", "general"), 63), (("wide", "general"), 257),
                                    (("r3-9-20-7", "graph"), 257), (("wide*15", "general"), 0)],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_ragged_batches_and_workspace_reuse(case, B):
    """Fewer rows than workgroups, rows that a workgroup loops over (the HBM code, B = 0 in the table: five rows more
    than its grid of 4 workgroups per CU, zero syndromes but three sampled rows at the front and two past the grid,
    under the syndrome stop), and the packed records."""
    import torch
    name, _ = case
    dec, cpu = gpu(case), q.DecoderCPU(code_of(*case))
    stops = (("ref", 20), ("fixed", 11), ("syndrome", 20))
    if name in REPLICATED:
        B = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 5
        stops = (("syndrome", 20),)
        hX, hZ = hbm_inputs(name)
        sX, sZ = np.zeros((B, hX.shape[1]), dtype=np.uint8), np.zeros((B, hZ.shape[1]), dtype=np.uint8)
        rows = [0, 1, 2, B - 4, B - 2]
        sX[rows], sZ[rows] = hX[:5], hZ[:5]
    else:
        sX, sZ = mixed_syndromes(matrices(name), 1000 + B, B + 3, (0.01, 0.05))
        sX, sZ = sX[-B:], sZ[-B:]  # keeps the special rows
    try:
        for option in OPTIONS:
            for d in (dec, cpu):
                d.set_option("correlated", option)
            for stop, N in stops:
                want = cpu.decode_batch(sX, sZ, P_MAIN, N, stop, want_iters=True, want_q=True)
                assert_same_decode(decode(dec, sX, sZ, P_MAIN, N, stop, option), want, "%s B=%d %s" % (name, B, stop))
                rec, it = dec.decode_batch_packed(sX, sZ, P_MAIN, N, stop, want_iters=True)
                assert {"sparse", "correlated", "records"} <= dec.last_path()
                assert np.array_equal(rec, pack_records(want[0], want[1], want[2])) and np.array_equal(it, want[3])
    finally:
        reset(dec)


# ---- identities -----------------------------------------------------------------------------------------------------
IDENTITY_CASES = (("hgp_ham", "general"), ("tall", "general"), ("r4-5-10-7", "graph"), ("mid*40", "general"),
                  ("r3-9-20-163", "graph"))


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=case_id)
def test_identities(case):
    name, _ = case
    code = code_of(*case)
    dec = gpu(case)
    lds = case in LDS_CASES
    sX, sZ = inputs(name) if lds else hbm_inputs(name)
    runs = (("ref", P_REF, 20), ("fixed", P_MAIN, 11), ("syndrome", P_MAIN, 20))
    c0, _ = q.correlated_priors(P_MAIN)
    pp = F32(2.0) / F32(3.0) * F32(P_MAIN)
    EX = code.numEqsX * code.stride
    try:
        for stop, p, N in runs:
            what = "%s %s" % (case_id(case), stop)
            # F's outputs are option 0's, scalar and under a channel; option back to 0 restores every bit
            for mode in ("scalar", "channel"):
                if mode == "channel":
                    dec.set_pauli_channel(*channel_of(name))
                base = decode(dec, sX, sZ, p, N, stop, 0)
                for option in OPTIONS:
                    dec.set_option("correlated", option)
                    first_sector_equal(decode(dec, sX, sZ, p, N, stop, option), base, option, code, what)
                dec.set_option("correlated", 0)
                assert_same_decode(decode(dec, sX, sZ, p, N, stop, 0), base, what + " option back to 0")
            # plain priors carry no correlation
            dec.set_priors(*prior_vectors(code.n, "random"))
            base = decode(dec, sX, sZ, p, N, stop, 0)
            for option in OPTIONS:
                dec.set_option("correlated", option)
                assert_same_decode(decode(dec, sX, sZ, p, N, stop, option), base, what + " plain priors")
            dec.set_option("correlated", 0)
            dec.set_priors(None, None)
        # scalar mode, rows whose F estimate is all zero: S is a set_priors decode whose S prior is c0 everywhere
        if lds:
            for option in OPTIONS:
                sec = 2 - option
                dec.set_option("correlated", option)
                got = decode(dec, sX, sZ, P_MAIN, 11, "fixed", option)
                dec.set_option("correlated", 0)
                dec.set_priors(*((pp, c0) if sec == 1 else (c0, pp)))
                want = decode(dec, sX, sZ, P_MAIN, 11, "fixed", 0)
                dec.set_priors(None, None)
                rows = ~got[1 - sec].any(axis=1)
                assert rows.sum() >= 2
                blk = slice(EX, None) if sec else slice(0, EX)
                assert np.array_equal(got[sec][rows], want[sec][rows])
                assert same_floats(got[4][rows][:, blk], want[4][rows][:, blk])
    finally:
        reset(dec)


@pytest.mark.parametrize("N", [11, 20])
def test_the_correlated_decode_differs_on_the_device(N):
    """hgp_ham (the codes of test_priors.py), scalar p = 0.05: S's q_final block and at least one sampled row's S
    decisions differ from option 0's, and the device equals the yardstick that showed it."""
    code = prior_code_of("hgp_ham")
    dec = q.DecoderGPU(code, 0, engine="sparse")
    sX, sZ = prior_inputs("hgp_ham")
    base = dec.decode_batch(sX, sZ, P_SCALAR, N, "syndrome", want_iters=True, want_q=True)
    for option in OPTIONS:
        dec.set_option("correlated", option)
        got = dec.decode_batch(sX, sZ, P_SCALAR, N, "syndrome", want_iters=True, want_q=True)
        assert_not_vacuous(base, got, option, code, "N=%d option %d" % (N, option))
        assert_same_decode(got, yardstick("hgp_ham", "scalar", "syndrome", N)[option], "N=%d option %d" % (N, option))


# ---- device contract ---------------------------------------------------------------------------------------------------
def test_dev_decodes_in_a_graph_with_a_channel():
    """The CORR kernels read the prior and conditional tables at replay time."""
    import torch
    name, B = "hgp_ham", 257
    code = prior_code_of(name)
    dec = q.DecoderGPU(code, 0, max_batch=B)
    cpu = q.DecoderCPU(code)
    first = pauli_vectors(code.n, "random")
    second = pauli_vectors(code.n, "special", seed=7)
    dec.set_pauli_channel(*first)  # allocates the device buffers before the capture
    dec.set_option("correlated", 1)
    cpu.set_option("correlated", 1)
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
    assert "correlated" in dec.last_path()
    dec.set_option("correlated", 0)  # read at the call: the graph keeps the kernels it captured
    wants = []
    for pv in (first, second):
        dec.set_pauli_channel(*pv)  # rewrites the buffers the captured kernels read
        cpu.set_pauli_channel(*pv)
        want = cpu.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
        wants.append(want)
        for t in (eX, eZ, fl, it, qf, rec):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same_decode([t.cpu().numpy() for t in (eX, eZ, fl, it, qf)], want, "graph replay")
        assert np.array_equal(rec.cpu().numpy(), pack_records(want[0], want[1], want[2]))
    assert not same_floats(wants[0][4], wants[1][4])


def test_two_streams_on_one_decoder():
    import torch
    code = prior_code_of("hgp_ham")
    B = 300
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    cpu = q.DecoderCPU(code)
    for d in (dec, cpu):
        d.set_option("correlated", 2)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    outs, wants = [], []
    for k, s in enumerate(streams):
        sX, sZ = mixed_syndromes(code_matrices("hgp_ham"), 90 + k, B, (0.03, 0.06))
        wants.append(cpu.decode_batch(sX, sZ, P_SCALAR, 20, "syndrome", want_iters=True, want_q=True))
        tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
        eX = torch.zeros((B, code.n), dtype=torch.uint8, device=dev)
        eZ, fl = torch.zeros_like(eX), torch.zeros(B, dtype=torch.uint8, device=dev)
        it = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        qf = torch.zeros((B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
        outs.append((tX, tZ, eX, eZ, fl, it, qf))
    torch.cuda.synchronize()
    for _ in range(3):
        for s, (tX, tZ, eX, eZ, fl, it, qf) in zip(streams, outs):
            dec.decode_batch_dev(tX, tZ, P_SCALAR, 20, "syndrome", eX, eZ, fl, iters=it, q=qf, stream=s)
    torch.cuda.synchronize()
    for o, want in zip(outs, wants):
        assert_same_decode([t.cpu().numpy() for t in o[2:]], want, "two streams")


def test_circulant_handle_refuses():
    from test_priors import code_of as named
    dec = q.DecoderGPU(named("P7"), 0, engine="circulant")
    for v in (1, 2):
        with pytest.raises(q.QecError, match="QEC_ENGINE_SPARSE"):
            dec.set_option("correlated", v)
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["correlated"], v) == -4  # QEC_ERR_UNSUPPORTED
    assert dec.get_option("correlated") == 0
    dec.set_option("correlated", 0)
    with pytest.raises(q.QecError, match="QEC_ENGINE_SPARSE"):
        dec.set_pauli_channel(0.01, 0.01, 0.01)
    arr = np.full(dec.code.n, 0.01, dtype=F32)
    assert q.lib().qec_decoder_set_pauli_channel(dec._h, q._ptr(arr), q._ptr(arr), q._ptr(arr)) == -4
    assert dec.get_pauli_channel() is None and dec.get_priors() is None
    dec.set_pauli_channel(None, None, None)  # clearing nothing is no error
    with pytest.raises(q.QecError, match="QEC_OPT_CORRELATED"):
        dec.set_option("correlated", 3)
    auto = q.DecoderGPU(named("P61"), 0)
    with pytest.raises(q.QecError, match="sparse"):
        auto.set_option("correlated", 1)


# ---- the sampler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["surf3", "hgp_ham"])
@pytest.mark.parametrize("start", [0, (1 << 32) - 64])
def test_sample_pauli_dev_matches_numpy(name, start):
    import torch
    from test_general_code import general_code
    code = general_code(name)
    HX, HZ = code_matrices(name)
    dec = q.DecoderGPU(code, 0)
    dev = torch.device("cuda", 0)
    B, seed = 130, 0xC0FFEE1234567
    pX, pY, pZ = pauli_vectors(code.n, "special")
    pX[1], pY[1], pZ[1] = F32(2.0) ** -32, 0.0, F32(2.0) ** -32  # tX = 1, tXYZ = 2
    pX[2], pY[2], pZ[2] = 0.0, F32(2.0) ** -32, 0.0              # tXY = 1
    dec.set_pauli_channel(pX, pY, pZ)
    x, z = pauli_samples(seed, start, B, pX, pY, pZ)
    assert x.any() and z.any() and (x & z).any() and (x & ~z & 1).any() and (z & ~x & 1).any()
    tx = torch.full((B, code.n), 7, dtype=torch.uint8, device=dev)
    tz = torch.full((B, code.n), 7, dtype=torch.uint8, device=dev)
    dec.sample_pauli_dev(seed, start, tx, tz)
    assert np.array_equal(tx.cpu().numpy(), x) and np.array_equal(tz.cpu().numpy(), z)
    # a shard drawn alone
    dec.sample_pauli_dev(seed, start + 100, tx[:30], tz[:30])
    assert np.array_equal(tx[:30].cpu().numpy(), x[100:]) and np.array_equal(tz[:30].cpu().numpy(), z[100:])
    # the fused front end: the same errors' syndromes and packed errors (p is not used), whatever the option says
    for option in (0, 1):
        dec.set_option("correlated", option)
        sX, sZ, errp = (torch.empty((B, w), dtype=torch.uint8, device=dev)
                        for w in (code.numEqsX, code.numEqsZ, 2 * ((code.n + 7) // 8)))
        dec.sample_syndrome_dev(seed, start, 0.9, sX, sZ, errp)
        assert np.array_equal(sX.cpu().numpy(), (x @ HX.T) & 1)
        assert np.array_equal(sZ.cpu().numpy(), (z @ HZ.T) & 1)
        exp = np.concatenate([np.packbits(x, axis=1, bitorder="little"), np.packbits(z, axis=1, bitorder="little")], 1)
        assert np.array_equal(errp.cpu().numpy(), exp)


def test_sample_pauli_dev_needs_a_channel():
    import torch
    from test_general_code import general_code
    code = general_code("surf3")
    dec = q.DecoderGPU(code, 0)
    t = torch.zeros((4, code.n), dtype=torch.uint8, device=torch.device("cuda", 0))
    with pytest.raises(q.QecError, match="no Pauli channel"):
        dec.sample_pauli_dev(1, 0, t, t.clone())
    dec.set_priors(0.01, 0.02)  # plain priors are no channel
    with pytest.raises(q.QecError, match="no Pauli channel"):
        dec.sample_pauli_dev(1, 0, t, t.clone())
    assert q.lib().qec_sample_pauli_dev(dec._h, 1, 0, 4, t.data_ptr(), t.data_ptr(), None) == -1  # QEC_ERR_ARG


# ---- Monte-Carlo ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["channel", "depolarizing"])
@pytest.mark.parametrize("osd", [0, 1])
def test_monte_carlo_counters(noise, osd):
    """Every counter equals a host recount: the sampler's numpy errors, then decode_batch, then check_logical; a
    two-part handle on device 0 gives the same counters."""
    name, seed, n_samples, p = "hgp_ham", 0xB1A5ED, 4096, 0.02
    code = logical_code(name)
    HX, HZ = code_matrices(name)
    one, two = q.DecoderGPU(code, 0, engine="sparse"), q.DecoderGPU(code, devices=[0, 0])
    host = q.DecoderCPU(code)
    if noise == "channel":
        pv = pauli_vectors(code.n, "random")
        for d in (one, two, host):
            d.set_pauli_channel(*pv)
        assert all(np.array_equal(a, b) for a, b in zip(two.parts()[1].get_pauli_channel(), pv))
        x, z = pauli_samples(seed, 0, n_samples, *pv)
    else:
        x, z = depolarizing(seed, 0, n_samples, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    results = {}
    for option in (0, 1, 2):
        for d in (one, two, host):
            d.set_option("osd", osd)
            d.set_option("osd_order", 10 if osd else 0)
            d.set_option("correlated", option)
        eX, eZ, fl, it, _ = host.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
        want = count(code, x, z, eX, eZ, fl, it)
        if osd:
            assert want["synX"] == want["synZ"] == 0
        for d in (one, two):
            got = d.monte_carlo(seed, 0, n_samples, p, 20, "syndrome", batch=1500)
            assert {k: got[k] for k in want} == want, (noise, osd, option, d.describe())
        assert ("osd" in one.last_path()) == bool(osd) and ("correlated" in one.last_path()) == bool(option)
        results[option] = want
    assert results[1] != results[0] and results[2] != results[0]

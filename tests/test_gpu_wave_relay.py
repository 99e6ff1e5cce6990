"""The wave relay kernels on the device (set_option("relay_wave", 1) on a sparse-engine handle; bp_wave_relay.hip): the
case table of tests/test_wave_relay.py -- eight block shapes x ten P, so each of the 24 kernels runs at every group
count G = 64 // P and every idle-lane count of the table -- against the CPU engine's outputs that module computes and
checks for non-vacuity, with the scalar p and with priors, S = 1 and S = 3; the anchors on the device (one leg with
gamma = 0 against the wave min-sum kernels, 17 legs and S = 5 on the shipped codes against the sparse RELAY kernels); a
syndrome byte other than 0 / 1, the scale 256, B = 1, the round trip 0 -> 1 -> 0, cleared tables, the independence of
minsum_wave, the refusals, a two-part group; packed records in a captured graph replayed after a second set_relay; the
Monte-Carlo counters with and without the OSD stage; the command-line tool.

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
from test_minsum import minsum_cpu
from test_priors import prior_vectors
from test_relay import LEGS, relay_cpu, tables
from test_wave_minsum import no_wave_codes
from test_wave_relay import DECODE_CASES, PRIOR_CASES, PRIOR_KINDS, SCALE, reference, relay_file

pytestmark = pytest.mark.gpu

F32 = np.float32
WAVE_PATH = {"sparse", "minsum", "relay", "wave"}
_decoders = {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_wave_relay")


def relay_decoder(code, S=1, wave=1, legs=LEGS, **kw):
    dec = q.DecoderGPU(code, 0, engine="sparse", **kw)
    dec.set_option("bp_method", 1)
    dec.set_relay(*tables(code.n, legs), solutions=S)
    dec.set_option("relay_wave", wave)
    return dec


def gpu(tmp, shape, P):
    """One sparse-engine decoder per row of the table, under min-sum with the wave relay kernels; a test sets the
    tables it needs (the option stays) and puts back the priors or options it changes."""
    key = (shape, P)
    if key not in _decoders:
        _decoders[key] = relay_decoder(code_of(tmp, shape, P)[0])
    return _decoders[key]


def decode(dec, sX, sZ, case, want_q=True):
    _, stop, p, N = case
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=want_q)
    assert WAVE_PATH <= dec.last_path(), dec.last_path()
    return got


def rows(ref, k):
    return tuple(a[:k] for a in ref)


def label(shape, P, kind, case, what):
    return "%s P=%d %s S=%d %s p=%g N=%d %s" % ((shape_id(shape), P, kind) + case + (what,))


# ---- 1. the table, scalar p ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_table_scalar(tmp, shape):
    J, K, L = shape
    for P in PS:
        dec = gpu(tmp, shape, P)
        n = code_of(tmp, shape, P)[0].n
        assert "[relay: wave-relay J=%d K=%d L=%d P=%d G=%d]" % (J, K, L, P, groups(P)) in dec.describe(), dec.describe()
        for S in (1, 3):
            dec.set_relay(*tables(n), solutions=S)
            for kind in KINDS:
                sX, sZ = inputs(tmp, shape, P, kind)
                for case in DECODE_CASES:
                    if case[0] != S:
                        continue
                    want = reference(tmp, shape, P, case, kind)
                    assert_same_decode(decode(dec, sX, sZ, case, True), want, label(shape, P, kind, case, "with q"))
                    if kind != "table":
                        continue
                    assert_same_decode(decode(dec, sX, sZ, case, False), want, label(shape, P, kind, case, "without q"),
                                       with_q=False)
                    k = ragged(P)
                    if k != batch(P):  # G divides the batch: its first k rows leave a ragged wave
                        assert_same_decode(decode(dec, sX[:k], sZ[:k], case, True), rows(want, k),
                                           label(shape, P, kind, case, "ragged"))
                    assert_same_decode(decode(dec, sX[:1], sZ[:1], case, True), rows(want, 1),
                                       label(shape, P, kind, case, "B = 1"))


# ---- 2. the table, priors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_table_priors(tmp, shape):
    for P in PS:
        dec = gpu(tmp, shape, P)
        n = code_of(tmp, shape, P)[0].n
        sX, sZ = inputs(tmp, shape, P)
        k = ragged(P)
        try:
            for vec in PRIOR_KINDS:
                dec.set_priors(*prior_vectors(n, vec))
                for case in PRIOR_CASES:
                    dec.set_relay(*tables(n), solutions=case[0])
                    want = reference(tmp, shape, P, case, "table", vec)
                    assert_same_decode(decode(dec, sX, sZ, case), want, label(shape, P, vec, case, "priors"))
                    if k != batch(P):
                        assert_same_decode(decode(dec, sX[:k], sZ[:k], case), rows(want, k),
                                           label(shape, P, vec, case, "priors, ragged"))
        finally:
            dec.set_priors(None, None)
        # the priors matter
        assert not same_floats(reference(tmp, shape, P, PRIOR_CASES[0], "table", "random")[4],
                               reference(tmp, shape, P, (3, "fixed", 0.03, 11))[4])


# ---- 3. anchors on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [((4, 5, 10), 33), ((3, 4, 8), 21), ((2, 3, 6), 1)], ids=["G1", "G3", "G64"])
def test_one_leg_with_gamma_zero_is_the_wave_minsum_kernel(tmp, row):
    """L = 1 and gamma = 0: every output bit equals the minsum_wave kernels' on the device, with and without priors."""
    shape, P = row
    code = code_of(tmp, shape, P)[0]
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", 1)
    dec.set_option("relay_wave", 1)
    zero = np.zeros((1, code.n), dtype=F32)
    sX, sZ = inputs(tmp, shape, P)
    for priors in (False, True):
        if priors:
            dec.set_priors(*prior_vectors(code.n, "special"))
        for stop in ("fixed", "syndrome", "ref"):
            for N in (0, 5, 11):
                dec.set_relay(None, None)
                want = dec.decode_batch(sX, sZ, 0.03, N, stop, want_iters=True, want_q=True)
                assert "relay" not in dec.last_path() and {"minsum", "wave"} <= dec.last_path()
                for S in (1, 3):
                    dec.set_relay(zero, zero, solutions=S)
                    assert_same_decode(decode(dec, sX, sZ, (S, stop, 0.03, N)), want,
                                       label(shape, P, "gamma 0", (S, stop, 0.03, N), "priors %s" % priors))


@pytest.mark.parametrize("name", [P61, P7], ids=["P61", "P7"])
def test_shipped_codes_17_legs_5_solutions(name):
    """relay_wave 1 equals relay_wave 0 (the sparse RELAY kernels) on a long chain and a larger S than the table's."""
    code = q.Quantum_LDPC_Code.createFromFile(code_path(name))
    dec = relay_decoder(code, S=5, wave=0, legs=17)
    x, z = depolarizing(0x51EC0DE, 0, 256, code.n, 0.05)
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    for N in (20, 7):
        dec.set_option("relay_wave", 0)
        want = dec.decode_batch(sX, sZ, 0.05, N, "syndrome", want_iters=True, want_q=True)
        assert "wave" not in dec.last_path() and "relay" in dec.last_path()
        dec.set_option("relay_wave", 1)
        got = decode(dec, sX, sZ, (5, "syndrome", 0.05, N))
        assert_same_decode(got, want, "%s N=%d" % (name, N))
        assert (want[3] > LEGS * N).any(), "some sector runs more legs than the table's tables have"


# ---- 4. in the interface ---------------------------------------------------------------------------------------------------
def test_a_syndrome_byte_of_2(tmp):
    """Truthy in the check update, equal to no parity: SYNDROME_FAIL in both sectors, and every leg runs to the cap."""
    shape, P = (3, 3, 6), 9
    code = code_of(tmp, shape, P)[0]
    dec = gpu(tmp, shape, P)
    sX, sZ = (np.array(a) for a in inputs(tmp, shape, P))
    row = 5
    sX[row, 7] = 2
    sZ[row, 11] = 2
    for S in (1, 3):
        cpu = relay_cpu(code, S)
        dec.set_relay(*tables(code.n), solutions=S)
        for stop, N in (("syndrome", 20), ("fixed", 11), ("ref", 11)):
            want = cpu.decode_batch(sX, sZ, 0.03, N, stop, want_iters=True, want_q=True)
            got = decode(dec, sX, sZ, (S, stop, 0.03, N))
            assert_same_decode(got, want, label(shape, P, "byte 2", (S, stop, 0.03, N), ""))
            assert got[2][row] & q.SYNDROME_FAIL_X and got[2][row] & q.SYNDROME_FAIL_Z
            if stop == "syndrome":
                assert got[3][row].tolist() == [LEGS * 20, LEGS * 20]


def test_scale_256(tmp):
    shape, P = (3, 4, 8), 21
    dec = gpu(tmp, shape, P)
    n = code_of(tmp, shape, P)[0].n
    sX, sZ = inputs(tmp, shape, P)
    cases = ((3, "fixed", 0.03, 11), (3, "syndrome", 0.03, 20))
    try:
        dec.set_option("minsum_scale", 256)
        dec.set_relay(*tables(n), solutions=3)
        for case in cases:
            want = reference(tmp, shape, P, case, scale=256)
            assert_same_decode(decode(dec, sX, sZ, case), want, label(shape, P, "scale 256", case, ""))
    finally:
        dec.set_option("minsum_scale", SCALE)
    assert not same_floats(reference(tmp, shape, P, cases[0], scale=256)[4], reference(tmp, shape, P, cases[0])[4])


def test_round_trip_and_cleared_tables(tmp):
    shape, P = (4, 4, 8), 22
    code = code_of(tmp, shape, P)[0]
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_relay(*tables(code.n), solutions=3)
    sX, sZ = inputs(tmp, shape, P)
    case = (3, "syndrome", 0.03, 20)
    before = dec.describe()
    outs, paths, words = [], [], []
    for wave in (0, 1, 0):
        dec.set_option("relay_wave", wave)
        assert dec.get_option("relay_wave") == wave
        assert dec.describe() == before + (" [relay: wave-relay J=4 K=4 L=8 P=22 G=2]" if wave else "")
        outs.append(dec.decode_batch(sX, sZ, 0.03, 20, "syndrome", want_iters=True, want_q=True))
        paths.append(dec.last_path())
        words.append(dec.get_option("last_path"))
    assert [("wave" in p) for p in paths] == [False, True, False] and all("relay" in p for p in paths)
    assert words[0] == words[2] and words[1] == words[0] | q.PATH["wave"]
    want = reference(tmp, shape, P, case)
    for k, got in enumerate(outs):
        assert_same_decode(got, want, "round trip, call %d" % k)
    # the tables gone with the option at 1: plain min-sum, by whichever kernels minsum_wave says
    dec.set_option("relay_wave", 1)
    dec.set_relay(None, None)
    plain = minsum_cpu(code, SCALE).decode_batch(sX, sZ, 0.03, 20, "syndrome", want_iters=True, want_q=True)
    for mw in (0, 1):
        dec.set_option("minsum_wave", mw)
        got = dec.decode_batch(sX, sZ, 0.03, 20, "syndrome", want_iters=True, want_q=True)
        assert "relay" not in dec.last_path() and ("wave" in dec.last_path()) == bool(mw)
        assert_same_decode(got, plain, "cleared tables, minsum_wave %d" % mw)
    # under the product rule the option does nothing
    dec.set_relay(*tables(code.n), solutions=3)
    dec.set_option("minsum_wave", 0)
    dec.set_option("bp_method", 0)
    dec.decode_batch(sX, sZ, 0.03, 5, "fixed")
    assert dec.last_path() == {"sparse"}


def test_minsum_wave_alone_leaves_the_relay_on_the_sparse_kernels(tmp):
    """minsum_wave 1, relay_wave 0, tables set: the sparse RELAY kernels, no "wave" in the path; relay_wave 1 with
    minsum_wave 0 runs the wave relay kernels."""
    shape, P = (3, 3, 6), 21
    code = code_of(tmp, shape, P)[0]
    sX, sZ = inputs(tmp, shape, P)
    dec = q.DecoderGPU(code, 0, engine="sparse")
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", 1)
    dec.set_relay(*tables(code.n), solutions=3)
    case = (3, "syndrome", 0.03, 11)
    got = dec.decode_batch(sX, sZ, 0.03, 11, "syndrome", want_iters=True, want_q=True)
    assert "relay" in dec.last_path() and "wave" not in dec.last_path()
    assert_same_decode(got, reference(tmp, shape, P, case), "minsum_wave alone")
    dec.set_option("minsum_wave", 0)
    dec.set_option("relay_wave", 1)
    assert_same_decode(decode(dec, sX, sZ, case), reference(tmp, shape, P, case), "relay_wave alone")


def test_refusals(tmp):
    for code in no_wave_codes(tmp):
        dec = q.DecoderGPU(code, 0, engine="sparse")
        dec.set_option("bp_method", 1)
        before = dec.describe()
        with pytest.raises(q.QecError, match="no wave relay kernel for this code"):
            dec.set_option("relay_wave", 1)
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["relay_wave"], 1) == -4  # QEC_ERR_UNSUPPORTED
        assert dec.get_option("relay_wave") == 0 and dec.describe() == before
    dec = q.DecoderGPU(q.Quantum_LDPC_Code.createFromFile(code_path(P7)), 0)  # engine auto: the wave-circulant engine
    with pytest.raises(q.QecError, match="create the decoder with QEC_ENGINE_SPARSE"):
        dec.set_option("relay_wave", 1)
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["relay_wave"], 1) == -4
    assert dec.get_option("relay_wave") == 0
    cpu = q.DecoderCPU(code_of(tmp, (3, 3, 6), 9)[0])
    with pytest.raises(q.QecError, match="CPU engine"):
        cpu.set_option("relay_wave", 1)
    good = q.DecoderGPU(code_of(tmp, (3, 3, 6), 9)[0], 0, engine="sparse")
    for bad in (-1, 2):
        assert q.lib().qec_decoder_set_option(good._h, q.OPTION["relay_wave"], bad) == -1  # QEC_ERR_ARG
    assert good.get_option("relay_wave") == 0


def test_a_two_part_group_decodes_like_one_part(tmp):
    shape, P = (3, 5, 10), 9
    code = code_of(tmp, shape, P)[0]
    two = q.DecoderGPU(code, devices=[0, 0], engine="sparse")
    two.set_option("bp_method", 1)
    two.set_relay(*tables(code.n), solutions=3)
    two.set_option("relay_wave", 1)
    assert all(p.get_option("relay_wave") == 1 for p in two.parts()) and two.get_option("relay_wave") == 1
    for kind in KINDS:
        sX, sZ = inputs(tmp, shape, P, kind)
        for case in ((3, "fixed", 0.03, 11), (3, "syndrome", 0.03, 20)):
            got = decode(two, sX, sZ, case)
            assert_same_decode(got, reference(tmp, shape, P, case, kind), label(shape, P, kind, case, "group, CPU"))


# ---- 5. a captured graph ------------------------------------------------------------------------------------------------------
def test_packed_records_in_a_captured_graph_read_new_tables(tmp):
    """decode_batch_packed_dev with the option and the tables set before the capture: the replay's records equal the
    direct call's and the CPU engine's, and a replay after a second set_relay (the same L and S) decodes with the new
    tables: they are rewritten in place, and the call allocates nothing."""
    import torch
    shape, P = (4, 5, 10), 21
    code = code_of(tmp, shape, P)[0]
    sX, sZ = inputs(tmp, shape, P)
    B = len(sX)
    dec = relay_decoder(code, S=3, max_batch=B)
    first = tables(code.n)
    second = (q.relay_gammas(code.n, LEGS, gamma0=0.3, seed=5), q.relay_gammas(code.n, LEGS, gamma0=-0.2, seed=6))
    dev = torch.device("cuda", 0)
    tX, tZ = torch.from_numpy(np.array(sX)).to(dev), torch.from_numpy(np.array(sZ)).to(dev)
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
        cpu = minsum_cpu(code, SCALE)
        cpu.set_relay(*tab, solutions=3)
        w = cpu.decode_batch(sX, sZ, 0.03, 11, "syndrome", want_iters=True, want_q=True)
        return [pack_records(w[0], w[1], w[2]), w[3], w[4]]

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_batch_packed_dev(tX, tZ, 0.03, 11, "syndrome", rec, iters=it, q=qf, stream=s)
    assert WAVE_PATH | {"records"} <= dec.last_path()
    wants = []
    for tab in (first, second):
        dec.set_relay(*tab, solutions=3)  # rewrites the table the captured kernel reads
        wants.append(run(lambda: dec.decode_batch_packed_dev(tX, tZ, 0.03, 11, "syndrome", rec, iters=it, q=qf)))
        same(run(g.replay), wants[-1], "replay")
        same(wants[-1], host(tab), "the direct call against the CPU engine")
    assert not np.array_equal(wants[0][0], wants[1][0]) or not same_floats(wants[0][2], wants[1][2])


# ---- 6. the Monte-Carlo counters ---------------------------------------------------------------------------------------------
def mc_code(which):
    if which == "P7":
        return q.Quantum_LDPC_Code.createFromFile(code_path(P7))
    return q.QC_LDPC_CSS(3, 3, 6, 13, 3, 2).with_logical("degenerate")


@pytest.mark.parametrize("osd", [0, 1])
@pytest.mark.parametrize("which", ["P7", "G13"])
def test_monte_carlo_counters(which, osd):
    """4096 samples at p = 0.05 under the syndrome stop, cap 20, S = 3: every counter and osd_sectors equal between
    relay_wave 0, relay_wave 1 and DecoderCPU."""
    code = mc_code(which)
    dec, cpu = relay_decoder(code, S=3, wave=0), relay_cpu(code, 3)
    seed, B, p = 1, 4096, 0.05
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    for d in (dec, cpu):
        d.set_option("osd", osd)
        d.set_option("osd_order", 10 if osd else 0)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    want = (count(code, x, z, eX, eZ, fl, it), cpu.get_option("osd_sectors"))
    assert want[0]["tested"] == B
    if which == "G13":  # the relay leaves sectors to the stage (on P7 it solves all of these samples: none)
        assert (want[1] > 0) == bool(osd)
    paths = []
    for wave in (0, 1):
        dec.set_option("relay_wave", wave)
        r = dec.monte_carlo(seed, 0, B, p, 20, "syndrome", batch=1024)
        paths.append(dec.last_path())
        assert {"minsum", "relay", "sparse"} <= paths[-1]
        assert ({k: r[k] for k in want[0]}, dec.get_option("osd_sectors")) == want, (which, osd, wave)
    assert "wave" not in paths[0] and paths[1] == paths[0] | {"wave"}
    if which == "G13":
        assert ("osd" in paths[1]) == bool(osd)


# ---- 7. the command-line tool ----------------------------------------------------------------------------------------------
def test_cli_relay_wave(tmp_path):
    """--engine sparse --bp-method minsum --relay FILE --relay-wave 1 names the kernel and gives --relay-wave 0's
    counters."""
    from test_osd_host import _cli, _fields
    keys = ("Errors Tested", "Corrected", "Syndrome Errors X", "Syndrome Errors Z", "Logical Errors", "Convergence Fail X",
            "Convergence Fail Z")
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P7))
    rf = relay_file(tmp_path / "relay.txt", code.n)
    out = {}
    for wave in ("0", "1"):
        d = tmp_path / ("wave" + wave)
        d.mkdir()
        r = _cli(d, ["--engine", "sparse", "--bp-method", "minsum", "--relay", rf, "--relay-solutions", "3", "--relay-wave",
                     wave, "--seed", "7"], code_path(P7), "3 3 1000 20 0.05")
        assert r.returncode == 0, r.stderr
        assert ("[relay: wave-relay J=3 K=3 L=6 P=7 G=9]" in r.stdout) == (wave == "1"), r.stdout
        f = _fields(d)
        out[wave] = {k: int(f[k]) for k in keys}
    assert out["0"] == out["1"] and out["1"]["Errors Tested"] > 0

"""General CSS codes on the GPU: the sparse-general kernel against the CPU engine and the numpy yardstick of
test_general_code.py, regular codes through it against the oracle, the Monte-Carlo entry points, OSD and
multi-part handles."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from oracle.philox import depolarizing
from qec_ldpc_amd.codes import write_code_file
from qec_ldpc_amd.gather import pack_records
from test_general_code import (CODES, G13, NS, OSD_B, OSD_N, OSD_P, STOPS, assert_same_decode, bp_yardstick,
                               code_matrices, decode_inputs, failed_sectors, general_code, mixed_syndromes, osd_case,
                               same_floats, yardstick)

pytestmark = pytest.mark.gpu

_decoders = {}


def gpu(name):
    if name not in _decoders:
        _decoders[name] = q.DecoderGPU(general_code(name), 0)
    return _decoders[name]


@pytest.fixture(scope="module")
def regular(code_paths, tmp_path_factory):
    """key -> (file code, oracle, the code from its matrices)."""
    tmp = tmp_path_factory.mktemp("gpu_general_regular")
    g = q.QC_LDPC_CSS(*G13)
    paths = dict(code_paths, G13=write_code_file(str(tmp / "g13.txt"), *G13, g.pcm(0), g.pcm(1)))
    out = {}
    for key, path in paths.items():
        code = q.Quantum_LDPC_Code.createFromFile(path)
        out[key] = (code, OracleCode(path), q.Quantum_LDPC_Code.createFromMatrices(code.pcm(0), code.pcm(1)))
    return out


# ---- plan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,threads", [("surf3", 64), ("hgp_ham", 128), ("ham_rep3", 64), ("ham_rep3+1", 64)])
def test_describe_and_workgroup_size(name, threads):
    """The smallest of 64 / 128 / 256 threads >= max(mX + mZ, 2n)."""
    d = gpu(name).describe()
    assert d.startswith("sparse-general lds threads=%d " % threads), d
    code = general_code(name)
    assert max(code.numEqsX + code.numEqsZ, 2 * code.n) <= threads
    assert q.DecoderGPU(code, 0, engine="sparse").describe() == d
    with pytest.raises(q.QecError):
        q.DecoderGPU(code, 0, engine="circulant")


@pytest.mark.parametrize("key,threads", [("P7", 128), ("P61", 256)])
def test_workgroup_size_of_regular_codes(regular, key, threads):
    d = q.DecoderGPU(regular[key][2], 0).describe()
    assert d.startswith("sparse-general lds threads=%d " % threads), d


# ---- GPU = CPU engine = yardstick -------------------------------------------------------------------------
@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("stop", STOPS)
def test_gpu_matches_yardstick_and_cpu_engine(name, stop):
    dec, cpu = gpu(name), q.DecoderCPU(general_code(name))
    sX, sZ = decode_inputs(name)
    for N in NS:
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, yardstick(name, stop, N), "%s %s N=%d vs the yardstick" % (name, stop, N))
        assert_same_decode(got, cpu.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True),
                           "%s %s N=%d vs the CPU engine" % (name, stop, N))


@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("B", [1, 63, 257])
def test_ragged_batches_byte_and_packed(name, B):
    """More rows than workgroups of one round or fewer: every row equals the CPU engine's, the first rows the
    yardstick's, and the packed records are the byte outputs packed."""
    HX, HZ = code_matrices(name)
    sX, sZ = mixed_syndromes((HX, HZ), 1000 + B, B + 3, (0.03, 0.1))
    sX, sZ = sX[-B:], sZ[-B:]  # keeps the special rows
    dec, cpu = gpu(name), q.DecoderCPU(general_code(name))
    for stop, N in (("ref", 20), ("fixed", 11), ("syndrome", 20)):
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, cpu.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True),
                           "%s B=%d %s" % (name, B, stop))
        k = min(B, 16)
        assert_same_decode([a[-k:] for a in got], bp_yardstick(HX, HZ, sX[-k:], sZ[-k:], 0.05, N, stop),
                           "%s B=%d %s vs the yardstick" % (name, B, stop))
        rec, it = dec.decode_batch_packed(sX, sZ, 0.05, N, stop, want_iters=True)
        assert np.array_equal(rec, pack_records(got[0], got[1], got[2])) and np.array_equal(it, got[3])


def test_decode_batch_dev_in_a_graph():
    import torch
    name, B = "hgp_ham", 257
    code = general_code(name)
    dec = q.DecoderGPU(code, 0, max_batch=B)
    dev = torch.device("cuda", 0)
    sX, sZ = mixed_syndromes(code_matrices(name), 77, B, (0.05,))
    want = q.DecoderCPU(code).decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True)
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
    for t in (eX, eZ, fl, it, qf, rec):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_same_decode([t.cpu().numpy() for t in (eX, eZ, fl, it, qf)], want, "graph replay")
    assert np.array_equal(rec.cpu().numpy(), pack_records(want[0], want[1], want[2]))


# ---- regular codes through the general kernel ------------------------------------------------------------------
@pytest.mark.parametrize("key", ["P7", "G13", "P61"])
@pytest.mark.parametrize("stop", STOPS)
def test_regular_code_through_the_general_kernel(regular, key, stop):
    code, orc, gen = regular[key]
    dec = q.DecoderGPU(gen, 0)
    sX, sZ = mixed_syndromes((code.pcm(0), code.pcm(1)), 3, 96, (0.01, 0.04))
    for N in (0, 1, 11, 50):
        want = orc.decode_batch(sX, sZ, 0.02, N, stop, want_q=True)
        assert_same_decode(dec.decode_batch(sX, sZ, 0.02, N, stop, want_iters=True, want_q=True), want,
                           "%s %s N=%d" % (key, stop, N))


def test_p61_general_equals_circulant(regular):
    code, _, gen = regular["P61"]
    x, z = depolarizing(11, 0, 4096, code.n, 0.02)
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    a = q.DecoderGPU(gen, 0)
    b = q.DecoderGPU(code, 0, engine="circulant")
    for stop in STOPS:
        assert_same_decode(a.decode_batch(sX, sZ, 0.02, 50, stop, want_iters=True, want_q=True),
                           b.decode_batch(sX, sZ, 0.02, 50, stop, want_iters=True, want_q=True), "P61 " + stop)


def test_hbm_mode(tmp_path):
    """The n = 4670 code's messages (168 KB) exceed LDS: the HBM slice."""
    J, K, L, P, s, t = 4, 5, 10, 467, 9, 49
    g = q.QC_LDPC_CSS(J, K, L, P, s, t)
    orc = OracleCode(write_code_file(str(tmp_path / "c.txt"), J, K, L, P, s, t, g.pcm(0), g.pcm(1)))
    dec = q.DecoderGPU(q.Quantum_LDPC_Code.createFromMatrices(g.pcm(0), g.pcm(1)), 0)
    assert dec.describe().startswith("sparse-general hbm threads=256 "), dec.describe()
    rng = np.random.default_rng(P)
    x = (rng.random((12, g.n)) < 0.01).astype(np.uint8)
    z = (rng.random((12, g.n)) < 0.01).astype(np.uint8)
    sX, sZ = g.syndrome(0, x), g.syndrome(1, z)
    sX[0] = 0
    sZ[-1] = 1
    for stop, N in (("ref", 25), ("fixed", 11), ("syndrome", 30)):
        assert_same_decode(dec.decode_batch(sX, sZ, 0.015, N, stop, want_iters=True, want_q=True),
                           orc.decode_batch(sX, sZ, 0.015, N, stop, want_q=True), "P=467 " + stop)


# ---- Monte-Carlo ---------------------------------------------------------------------------------------------------
MC_NAMES = ("hgp_ham", "ham_rep3+1")
_logical = {}


def logical_code(name):
    if name not in _logical:
        _logical[name] = general_code(name).with_logical("degenerate")
    return _logical[name]


def count(code, x, z, eX, eZ, flags, iters=None):
    """The CodeStatistics counters of a decoded batch (DecoderCPU.h:392-530)."""
    fx, fz = (flags & q.SYNDROME_FAIL_X) != 0, (flags & q.SYNDROME_FAIL_Z) != 0
    ok = ~(fx | fz)
    logical = code.check_logical(x[ok] ^ eX[ok], z[ok] ^ eZ[ok])
    out = {"tested": len(flags), "withX": int(x.any(axis=1).sum()), "withZ": int(z.any(axis=1).sum()),
           "synX": int(fx.sum()), "synZ": int(fz.sum()), "logical": int(logical.sum()),
           "corrected": int((~logical).sum()), "convX": int(((flags & q.CONVERGENCE_FAIL_X) != 0).sum()),
           "convZ": int(((flags & q.CONVERGENCE_FAIL_Z) != 0).sum())}
    if iters is not None:
        out["iterationsX"], out["iterationsZ"] = int(iters[:, 0].sum()), int(iters[:, 1].sum())
    return out


@pytest.mark.parametrize("name", MC_NAMES)
@pytest.mark.parametrize("p", [0.01, 0.05])
def test_monte_carlo_counters(name, p):
    code = logical_code(name)
    HX, HZ = code_matrices(name)
    dec, cpu = q.DecoderGPU(code, 0), q.DecoderCPU(code)
    seed, B = 0x51EC0DE, 20000
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    for stop in ("syndrome", "ref"):
        eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, 20, stop, want_iters=True)
        want = count(code, x, z, eX, eZ, fl, it)
        got = dec.monte_carlo(seed, 0, B, p, 20, stop, batch=8192)
        assert {k: got[k] for k in want} == want, (name, p, stop)


@pytest.mark.parametrize("name", MC_NAMES)
def test_sample_syndrome_dev_matches_numpy(name):
    import torch
    code = logical_code(name)
    HX, HZ = code_matrices(name)
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
    # the byte form: errors on the device, then their syndromes
    tx, tz = torch.empty((B, code.n), dtype=torch.uint8, device=dev), torch.empty((B, code.n), dtype=torch.uint8, device=dev)
    dec.sample_depolarizing_dev(seed, lo, p, tx, tz)
    assert np.array_equal(tx.cpu().numpy(), x) and np.array_equal(tz.cpu().numpy(), z)
    bX, bZ = torch.empty_like(sX), torch.empty_like(sZ)
    dec.syndrome_dev(tx, tz, bX, bZ)
    assert torch.equal(bX, sX) and torch.equal(bZ, sZ)


@pytest.mark.parametrize("name", MC_NAMES)
def test_get_statistics_counts(name):
    code = logical_code(name)
    HX, HZ = code_matrices(name)
    dec, cpu = q.DecoderGPU(code, 0), q.DecoderCPU(code)
    for W, B, seed in ((2, 4000, 1234), (5, 3000, 99)):
        x, z = q.sample_fixed_weight(seed, W, B, code.n)
        sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        eX, eZ, fl, _, _ = cpu.decode_batch(sX, sZ, 0.03, 30, "ref")
        want = count(code, x, z, eX, eZ, fl)
        for d in (dec, cpu):
            g = d.GetStatistics(W, B, 0.03, 30, seed=seed)
            got = {"tested": g["numErrorsTested"], "withX": g["numXErrorsTested"], "withZ": g["numZErrorsTested"],
                   "synX": g["syndromeErrorsX"], "synZ": g["syndromeErrorsZ"], "logical": g["logicalErrors"],
                   "corrected": g["corrected"], "convX": g["convergenceFailX"], "convZ": g["convergenceFailZ"]}
            assert got == want, (name, W, d.describe())


def test_multi_part_counters_equal_one_part():
    code = logical_code("hgp_ham")
    one, two = q.DecoderGPU(code, 0), q.DecoderGPU(code, devices=[0, 0])
    a = one.monte_carlo(7, 0, 20000, 0.05, 20, "syndrome", batch=8192)
    b = two.monte_carlo(7, 0, 20000, 0.05, 20, "syndrome", batch=8192)
    for k in ("tested", "withX", "withZ", "synX", "synZ", "logical", "corrected", "convX", "convZ", "iterationsX",
              "iterationsZ"):
        assert a[k] == b[k], (k, a[k], b[k])
    sX, sZ = decode_inputs("hgp_ham")
    assert_same_decode(two.decode_batch(sX, sZ, 0.05, 11, "ref", want_iters=True, want_q=True),
                       yardstick("hgp_ham", "ref", 11), "two parts")


# ---- OSD ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC_NAMES)
def test_osd_on_the_gpu(name):
    import torch
    sX, sZ, main, soft, rep = osd_case(name)
    code = general_code(name)
    dec, cpu = q.DecoderGPU(code, 0), q.DecoderCPU(code)
    dev = torch.device("cuda", 0)
    pre = dec.decode_batch(sX, sZ, OSD_P, OSD_N, "syndrome", want_iters=True)
    assert np.array_equal(pre[2], main[2])
    for lam in (0, 10):
        for d in (dec, cpu):
            d.set_option("osd", 1)
            d.set_option("osd_order", lam)
        got = dec.decode_batch(sX, sZ, OSD_P, OSD_N, "syndrome", want_iters=True)
        want = cpu.decode_batch(sX, sZ, OSD_P, OSD_N, "syndrome", want_iters=True)
        assert_same_decode(got, want, "%s osd_order=%d" % (name, lam), with_q=False)
        assert_same_decode(got, rep[lam][:3] + (main[3],), "%s osd_order=%d vs numpy" % (name, lam), with_q=False)
        assert not (got[2] & 3).any()
        assert dec.get_option("osd_sectors") == failed_sectors(main[2]) == cpu.get_option("osd_sectors")
        assert dec.get_option("osd_cs_sectors") == cpu.get_option("osd_cs_sectors") == rep[lam][4]
        # composed on the device: the main decode, the soft decode, osd_dev
        dec.set_option("osd", 0)
        tX, tZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
        eX = torch.empty((OSD_B, code.n), dtype=torch.uint8, device=dev)
        eZ, fl = torch.empty_like(eX), torch.empty(OSD_B, dtype=torch.uint8, device=dev)
        jX, jZ, jf = torch.empty_like(eX), torch.empty_like(eX), torch.empty_like(fl)
        qf = torch.empty((OSD_B, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
        dec.decode_batch_dev(tX, tZ, OSD_P, OSD_N, "syndrome", eX, eZ, fl)
        dec.decode_batch_dev(tX, tZ, OSD_P, 3, "fixed", jX, jZ, jf, q=qf)
        assert same_floats(qf.cpu().numpy(), soft)
        dec.osd_dev(tX, tZ, qf, eX, eZ, fl)
        for t, w in zip((eX, eZ, fl), got[:3]):
            assert np.array_equal(t.cpu().numpy(), w)

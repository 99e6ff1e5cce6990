"""The derived logical check on the device: the per-sample outcome kernel (qec_logical_packed_dev,
montecarlo.hip logical_outcome_kernel) against numpy's GF(2) membership test, and the statistics
pipelines (qec_monte_carlo on the ordered and the fused low-p path, multi-device, GetStatistics) on
codes whose check was derived from their parity-check matrices, against the oracle's counting over
the saved code file."""
import numpy as np
import pytest
import torch

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from oracle.philox import depolarizing
from test_gpu_montecarlo import oracle_counters
from test_logical_derived import G13, GS, MODES, STAT_MAP, Span, cpu_statistics, oracle_statistics, row_xor, save_code

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G17 = (4, 4, 8, 17, 4, 3)
FLAGS = np.array([0, 1, 2, 3, 4, 8, 12], dtype=np.uint8)
GUARD = 64


def base_code(key, code_paths):
    if key in ("P7", "P61"):
        return q.Quantum_LDPC_Code.createFromFile(code_paths[key])
    return q.QC_LDPC_CSS(*{"G13": G13, "G17": G17}[key])


@pytest.fixture(scope="module")
def codes(code_paths):
    """(key, mode) -> code; built once per module."""
    cache = {}

    def get(key, mode):
        if (key, mode) not in cache:
            base = base_code(key, code_paths)
            cache[(key, mode)] = base if mode == "file" else base.with_logical(mode)
        return cache[(key, mode)]
    return get


@pytest.fixture(scope="module")
def decoders(codes):
    cache = {}

    def get(key, mode, engine="auto"):
        if (key, mode, engine) not in cache:
            cache[(key, mode, engine)] = q.DecoderGPU(codes(key, mode), 0, engine=engine)
        return cache[(key, mode, engine)]
    return get


@pytest.fixture(scope="module")
def spans(code_paths):
    """key -> (Span(pcmX), Span(pcmZ), pcmX, pcmZ): numpy's side, shared by every case of a code."""
    cache = {}

    def get(key):
        if key not in cache:
            c = base_code(key, code_paths)
            cache[key] = (Span(c.pcm(0)), Span(c.pcm(1)), c.pcm(0), c.pcm(1))
        return cache[key]
    return get


def pack_bits(bits):
    """[B, n] 0/1 -> [B, ceil(n/8)], bit j of byte k = qubit 8k + j, padding bits 0."""
    return np.packbits(bits, axis=1, bitorder="little")


def outcome_case(HX, HZ, B, seed):
    """Inputs of one logical_packed_dev case: packed errors, records, and the residual bits numpy judges.
    errp at density 0.03; record bits = errp ^ pattern, the pattern drawn per sample from {nothing, an XOR
    of pcmX rows in x, an XOR of pcmZ rows in x, one bit, random sparse}; flags from FLAGS."""
    n = HX.shape[1]
    rng = np.random.default_rng(seed)
    ex = (rng.random((B, n)) < 0.03).astype(np.uint8)
    ez = (rng.random((B, n)) < 0.03).astype(np.uint8)
    px = np.zeros((B, n), dtype=np.uint8)
    pz = np.zeros((B, n), dtype=np.uint8)
    kind = rng.integers(0, 5, B)
    fromX, fromZ = row_xor(HX, rng, B), row_xor(HZ, rng, B)
    bit = rng.integers(0, 2 * n, B)
    sparse = (rng.random((B, 2 * n)) < 0.02).astype(np.uint8)
    for b in range(B):
        if kind[b] == 1:
            px[b] = fromX[b]
        elif kind[b] == 2:
            px[b] = fromZ[b]
        elif kind[b] == 3:
            (px if bit[b] < n else pz)[b, bit[b] % n] = 1
        elif kind[b] == 4:
            px[b], pz[b] = sparse[b, :n], sparse[b, n:]
    flags = FLAGS[rng.integers(0, len(FLAGS), B)]
    errp = np.concatenate([pack_bits(ex), pack_bits(ez)], axis=1)
    rec = np.concatenate([pack_bits(ex ^ px), pack_bits(ez ^ pz), flags[:, None]], axis=1)
    return errp, rec, flags, px, pz


def numpy_outcome(sX, sZ, mode, flags, px, pz):
    """0 corrected, 1 logical, 2 syndrome failure, from the membership test alone.  A file's own matrix
    computes the reference mode's test."""
    a, b = (sZ, sX) if mode == "degenerate" else (sX, sZ)
    logical = ~(a.contains(px) & b.contains(pz))
    return np.where(flags & 3, 2, logical.astype(np.uint8)).astype(np.uint8)


def run_outcome(dec, errp, rec, rec_offset=0):
    B = errp.shape[0]
    out = torch.full((B + GUARD,), 0xAA, dtype=torch.uint8, device=DEV)
    raw = torch.zeros(rec.size + rec_offset, dtype=torch.uint8, device=DEV)
    rec_t = raw[rec_offset:].view(B, rec.shape[1])
    rec_t.copy_(torch.from_numpy(rec))
    assert rec_t.data_ptr() == raw.data_ptr() + rec_offset
    dec.logical_packed_dev(torch.from_numpy(errp).to(DEV), rec_t, out[:B])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[B:] == 0xAA).all()  # nothing written beyond outcome[B)
    return got[:B]


OUTCOME_CASES = ([(k, m, "auto") for k in ("P7", "P61") for m in ("file",) + MODES] +
                 [(k, m, "auto") for k in ("G13", "G17") for m in MODES] + [("G13", m, "sparse") for m in MODES])


# ---- A. the outcome kernel per sample ------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("key,mode,engine", OUTCOME_CASES)
def test_logical_packed_dev_matches_numpy(codes, decoders, spans, key, mode, engine, B):
    sX, sZ, HX, HZ = spans(key)
    errp, rec, flags, px, pz = outcome_case(HX, HZ, B, seed=1000 + B)
    exp = numpy_outcome(sX, sZ, mode, flags, px, pz)
    if B >= 63:
        assert set(exp.tolist()) == {0, 1, 2}  # all three outcomes, by numpy alone
    dec = decoders(key, mode, engine)
    assert ("sparse" in dec.describe()) == (engine == "sparse")
    got = run_outcome(dec, errp, rec)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]


def test_logical_packed_dev_single_sample_outcomes(decoders, spans):
    """B = 1 for each of the three outcomes (one random single-sample case shows only one of them)."""
    sX, sZ, HX, HZ = spans("G13")
    errp, rec, flags, px, pz = outcome_case(HX, HZ, 200, seed=5)
    exp = numpy_outcome(sX, sZ, "degenerate", flags, px, pz)
    dec = decoders("G13", "degenerate")
    for want in (0, 1, 2):
        b = int(np.nonzero(exp == want)[0][0])
        assert run_outcome(dec, errp[b:b + 1], rec[b:b + 1])[0] == want


def test_logical_packed_dev_records_at_odd_address(decoders, spans):
    """The records start at byte 1 of their allocation (rows of 21 bytes: no row is word-aligned)."""
    sX, sZ, HX, HZ = spans("G13")
    errp, rec, flags, px, pz = outcome_case(HX, HZ, 1000, seed=2000)
    exp = numpy_outcome(sX, sZ, "reference", flags, px, pz)
    assert set(exp.tolist()) == {0, 1, 2}
    assert np.array_equal(run_outcome(decoders("G13", "reference"), errp, rec, rec_offset=1), exp)


def test_logical_packed_dev_refusals(codes, decoders):
    plain = q.DecoderGPU(q.QC_LDPC_CSS(*G13), 0)
    errp = torch.zeros((4, 20), dtype=torch.uint8, device=DEV)
    rec = torch.zeros((4, 21), dtype=torch.uint8, device=DEV)
    out = torch.zeros(4, dtype=torch.uint8, device=DEV)
    with pytest.raises(q.QecError, match="I-P"):
        plain.logical_packed_dev(errp, rec, out)
    group = q.DecoderGPU(codes("G13", "reference"), devices=[0, 0])
    with pytest.raises(q.QecError, match="parts"):
        group.logical_packed_dev(errp, rec, out)
    group.parts()[1].logical_packed_dev(errp, rec, out)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0, 0, 0, 0]


# ---- B. qec_monte_carlo on a derived code ----------------------------------------------------------
MC = dict(seed=0xC0DE, start=5, count=3000, p=0.05, max_iter=25, batch=1024)


@pytest.fixture(scope="module")
def g13_files(codes, tmp_path_factory):
    d = tmp_path_factory.mktemp("g13_gpu")
    return {mode: save_code(d / ("g13_%s.txt" % mode), codes("G13", mode)) for mode in MODES}


@pytest.fixture(scope="module")
def mc_expected(g13_files):
    """(mode, stop) -> (counters, iteration sums) by the oracle over the saved file; computed once."""
    cache = {}
    x, z = depolarizing(MC["seed"], MC["start"], MC["count"], 6 * 13, MC["p"])

    def get(mode, stop):
        if (mode, stop) not in cache:
            cache[(mode, stop)] = oracle_counters(OracleCode(g13_files[mode]), x, z, MC["p"], MC["max_iter"], stop)
        return cache[(mode, stop)]
    return get


def test_monte_carlo_expectation_separates_the_modes(mc_expected):
    """Conditions the oracle alone meets: both outcomes of the check occur in every run, and the two
    modes count different logical errors under the reference and syndrome stops."""
    for stop in ("ref", "syndrome", "fixed"):
        for mode in MODES:
            c, _ = mc_expected(mode, stop)
            assert c["logical"] > 0 and c["corrected"] > 0, (mode, stop)
    for stop in ("ref", "syndrome"):
        assert mc_expected("reference", stop)[0]["logical"] != mc_expected("degenerate", stop)[0]["logical"], stop


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("engine,stop", [("auto", "ref"), ("auto", "syndrome"), ("auto", "fixed"),
                                         ("sparse", "syndrome")])
def test_monte_carlo_derived_code_matches_oracle(decoders, mc_expected, mode, engine, stop):
    dec = decoders("G13", mode, engine)
    if engine == "auto":
        assert "runtime-shift" in dec.describe()
    r = dec.monte_carlo(MC["seed"], MC["start"], MC["count"], MC["p"], MC["max_iter"], stop, batch=MC["batch"])
    exp, it = mc_expected(mode, stop)
    assert {k: r[k] for k in q.MC_COUNTERS} == exp
    assert r["tested"] == MC["count"]
    assert r["iterationsX"] == int(it[:, 0].sum()) and r["iterationsZ"] == int(it[:, 1].sum())


# ---- C. the fused low-p pipeline with a derived check ----------------------------------------------
def test_monte_carlo_fused_pipeline_degenerate_p7(codes, decoders, tmp_path):
    code = codes("P7", "degenerate")
    path = save_code(tmp_path / "p7_degenerate.txt", code)
    count, p = 20000, 0.005
    r = decoders("P7", "degenerate").monte_carlo(0xBEEF, 17, count, p, 25, "syndrome", batch=1000)
    x, z = depolarizing(0xBEEF, 17, count, code.n, p)
    exp, it = oracle_counters(OracleCode(path), x, z, p, 25, "syndrome")
    assert {k: r[k] for k in q.MC_COUNTERS} == exp
    assert r["iterationsX"] == int(it[:, 0].sum()) and r["iterationsZ"] == int(it[:, 1].sum())


# ---- D. outcomes and counters of one decoded batch agree -------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_outcomes_add_up_to_the_counters(codes, decoders, mode):
    code, dec = codes("G13", mode), decoders("G13", mode)
    B, p = 1000, 0.05
    sX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=DEV)
    sZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=DEV)
    errp = torch.empty((B, 2 * ((code.n + 7) // 8)), dtype=torch.uint8, device=DEV)
    rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=DEV)
    dec.sample_syndrome_dev(0xC0DE, 5, p, sX, sZ, errp)
    dec.decode_batch_packed_dev(sX, sZ, p, 25, "ref", rec)
    cnt = torch.zeros(8, dtype=torch.int64, device=DEV)
    dec.statistics_packed_dev(errp, rec, cnt)
    out = torch.full((B,), 0xAA, dtype=torch.uint8, device=DEV)
    dec.logical_packed_dev(errp, rec, out)
    torch.cuda.synchronize()
    c = dict(zip(q.MC_COUNTERS, cnt.cpu().tolist()))
    o = out.cpu().numpy()
    assert int((o == q.OUTCOME_LOGICAL).sum()) == c["logical"] > 0
    assert int((o == q.OUTCOME_CORRECTED).sum()) == c["corrected"] > 0
    fl = rec.cpu().numpy()[:, -1]
    assert np.array_equal(o == q.OUTCOME_SYNDROME_FAIL, (fl & 3) != 0)


@pytest.mark.parametrize("key,mode", [("P7", "file"), ("P61", "file"), ("G13", "reference"), ("G13", "degenerate")])
def test_statistics_kernels_on_stabilizer_residuals(decoders, spans, key, mode):
    """The counting kernels on the same synthetic batch (dense residuals that are products of
    stabilizers, which a decoder's own residuals almost never are): logical / corrected equal numpy's
    counts, from packed rows and from byte rows.  A residual word with bit 31 set used to sign-extend
    over bits 32..63 in logical_from_columns."""
    sX, sZ, HX, HZ = spans(key)
    n, B = HX.shape[1], 1000
    errp, rec, flags, px, pz = outcome_case(HX, HZ, B, seed=77)
    exp = numpy_outcome(sX, sZ, mode, flags, px, pz)
    assert (px[exp == 0, 31] == 1).any()  # corrected samples with x qubit 31 in the residual
    dec = decoders(key, mode)
    cnt = torch.zeros(8, dtype=torch.int64, device=DEV)
    dec.statistics_packed_dev(torch.from_numpy(errp).to(DEV), torch.from_numpy(rec).to(DEV), cnt)
    ex = np.unpackbits(errp[:, :errp.shape[1] // 2], axis=1, bitorder="little")[:, :n]
    ez = np.unpackbits(errp[:, errp.shape[1] // 2:], axis=1, bitorder="little")[:, :n]
    cnt2 = torch.zeros(8, dtype=torch.int64, device=DEV)
    dec.statistics_dev(*(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ex, ez, ex ^ px, ez ^ pz, flags)),
                       cnt2)
    torch.cuda.synchronize()
    for c in (cnt, cnt2):
        got = dict(zip(q.MC_COUNTERS, c.cpu().tolist()))
        assert got["logical"] == int((exp == 1).sum()) and got["corrected"] == int((exp == 0).sum())
        assert got["synX"] == int((flags & 1 != 0).sum()) and got["synZ"] == int((flags & 2 != 0).sum())


# ---- E. multi-device ---------------------------------------------------------------------------
def test_monte_carlo_multi_device_derived_code(codes, decoders):
    code = codes("G13", "degenerate")
    one = decoders("G13", "degenerate").monte_carlo(MC["seed"], MC["start"], MC["count"], MC["p"], MC["max_iter"],
                                                    "syndrome", batch=MC["batch"])
    two = q.DecoderGPU(code, devices=[0, 0]).monte_carlo(MC["seed"], MC["start"], MC["count"], MC["p"],
                                                         MC["max_iter"], "syndrome", batch=MC["batch"])
    for k in q.MC_COUNTERS + ("tested", "iterationsX", "iterationsZ"):
        assert one[k] == two[k], k
    assert one["logical"] > 0


# ---- F. DecoderGPU::GetStatistics ------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_gpu_get_statistics_matches_cpu_and_oracle(codes, decoders, g13_files, mode):
    st = decoders("G13", mode).GetStatistics(GS["W"], GS["count"], GS["p"], GS["max_iter"], GS["seed"])
    got = {k: st[v] for k, v in STAT_MAP.items()}
    assert got == cpu_statistics(codes("G13", mode), mode, GS["count"])
    assert got == oracle_statistics(g13_files[mode], GS["count"])

"""Every runtime-shift wave-circulant kernel on the device: the case table of test_circulant_shapes.py (the eight
rt<J,K,L> shapes of bp_decode.hip's kVariants x P in {1, 2, 3, 9, 21, 22, 32, 33, 63, 64} x three stop rules, so
each of the 24 kernels runs at all ten P) against the oracle's outputs that module computes and checks for
non-vacuity.  Every code decodes two batches: the table's mixed inputs, and the "waves" batch, whose first two waves
are zero in one sector with all their G groups (without final messages such a wave takes the zero-syndrome
shortcut in that sector; the table batch holds a whole zero wave only at G = 1) and whose third ends hard in every
group (the state the near-hard jump and the cycle jump skip from); the host module asserts both on the inputs and
the oracle's outputs.  describe() confirms the engine and G; then byte decodes with and without final messages, a
ragged batch of its own where G divides the table's, hard_paths / cycle_jump / near_hard off in turn, packed
records from byte rows and from bit rows with a guard row behind the record buffer, dispatch order 0 and 2 (the
order pass groups the zero syndromes of a batch into waves of their own), the syndrome kernel and the fused
sampler on every code, and the Monte-Carlo pipeline on the codes with n <= 132.  One decode case, p = 1.5
(p' = 1), ends every code with NaN messages and lies outside the hard-message forms and the scaled division.

Bit for bit everywhere: eX, eZ, flags, iteration counts, q_final as uint32 patterns (NaN matches NaN), records,
syndromes, packed errors and counters.  There is no tolerance."""
import numpy as np
import pytest
import torch

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from oracle.philox import depolarizing
from qec_ldpc_amd.gather import pack_records
from test_circulant_shapes import (KINDS, PS, SHAPES, STOPS, batch, cases_of, code_of, exponent_tables, groups, inputs, ragged,
                                   reference, shape_id, write_file)
from test_general_code import assert_same_decode
from test_gpu_montecarlo import oracle_counters
from test_gpu_triage import bit_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 0xA5

_decoders = {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_circulant_shapes")


def gpu(tmp, shape, P):
    """One decoder per row of the table, engine chosen by the library."""
    key = (shape, P)
    if key not in _decoders:
        _decoders[key] = q.DecoderGPU(code_of(tmp, shape, P)[0], 0)
    return _decoders[key]


def decode(dec, sX, sZ, case, want_q):
    stop, p, N = case
    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=want_q)
    assert "sparse" not in dec.last_path()
    return got


def rows(ref, k):
    return tuple(a[:k] for a in ref)


def label(shape, P, kind, case, what):
    return "%s P=%d %s %s p=%g N=%d %s" % ((shape_id(shape), P, kind) + case + (what,))


# ---- which kernel runs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_engine_selection(tmp, shape):
    J, K, L = shape
    for P in PS:
        d = gpu(tmp, shape, P).describe()
        assert "runtime-shift J=%d K=%d L=%d P=%d G=%d" % (J, K, L, P, groups(P)) in d, d
    # one past the wave: the sparse engine, and no circulant kernel on request
    code = q.Quantum_LDPC_Code.createFromFile(write_file(tmp, shape, 65))
    assert np.array_equal(code.exponents(0), exponent_tables(shape, 65)[0])
    assert q.DecoderGPU(code, 0).describe().startswith("sparse-graph")
    with pytest.raises(q.QecError):
        q.DecoderGPU(code, 0, engine="circulant")


def test_shape_outside_the_table_goes_to_the_sparse_engine(tmp):
    code = q.Quantum_LDPC_Code.createFromFile(write_file(tmp, (3, 6, 12), 7))
    assert np.array_equal(code.exponents(1), exponent_tables((3, 6, 12), 7)[1])
    assert q.DecoderGPU(code, 0).describe().startswith("sparse-graph")
    with pytest.raises(q.QecError):
        q.DecoderGPU(code, 0, engine="circulant")


# ---- decodes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_byte_decode(tmp, shape, stop):
    for P in PS:
        dec = gpu(tmp, shape, P)
        for kind in KINDS:
            sX, sZ = inputs(tmp, shape, P, kind)
            for case in cases_of(stop):
                want = reference(tmp, shape, P, case, kind)
                assert_same_decode(decode(dec, sX, sZ, case, True), want, label(shape, P, kind, case, "with q"))
                assert_same_decode(decode(dec, sX, sZ, case, False), want, label(shape, P, kind, case, "without q"),
                                   with_q=False)
                k = ragged(P)
                if kind == "table" and k != batch(P):  # G divides the batch: its first k rows leave a ragged wave
                    for want_q in (True, False):
                        assert_same_decode(decode(dec, sX[:k], sZ[:k], case, want_q), rows(want, k),
                                           label(shape, P, kind, case, "ragged, q %s" % want_q), with_q=want_q)


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_options_change_no_bit(tmp, shape, stop):
    for P in PS:
        dec = gpu(tmp, shape, P)
        for option in ("hard_paths", "cycle_jump", "near_hard"):
            assert dec.get_option(option) == 1
            dec.set_option(option, 0)
            try:
                for kind in KINDS:
                    sX, sZ = inputs(tmp, shape, P, kind)
                    for case in cases_of(stop):
                        want = reference(tmp, shape, P, case, kind)
                        for want_q in (True, False):
                            assert_same_decode(decode(dec, sX, sZ, case, want_q), want,
                                               label(shape, P, kind, case, "%s off, q %s" % (option, want_q)), with_q=want_q)
            finally:
                dec.set_option(option, 1)


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_dispatch_order_changes_no_bit(tmp, shape, stop):
    for P in PS:
        dec = gpu(tmp, shape, P)
        assert dec.get_option("schedule") == 1
        for schedule in (0, 2):
            dec.set_option("schedule", schedule)
            try:
                for kind in KINDS:
                    sX, sZ = inputs(tmp, shape, P, kind)
                    for case in cases_of(stop):
                        want = reference(tmp, shape, P, case, kind)
                        for want_q in (True, False):
                            got = decode(dec, sX, sZ, case, want_q)
                            # the launch took the order pass, or did not: the option is not silently dropped
                            assert ("ordered" in dec.last_path()) == (schedule == 2), (schedule, dec.last_path())
                            assert_same_decode(got, want, label(shape, P, kind, case, "schedule %d, q %s" % (schedule, want_q)),
                                               with_q=want_q)
            finally:
                dec.set_option("schedule", 1)


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_packed_and_bit_row_decode(tmp, shape, stop):
    """Records [B, 2 ceil(n/8) + 1] from byte rows and from bit rows of ceil(m/32) words; the row behind the
    record buffer keeps its fill pattern."""
    for P in PS:
        for kind in KINDS:
            packed_decodes(tmp, shape, P, kind, stop)


def packed_decodes(tmp, shape, P, kind, stop):
    dec = gpu(tmp, shape, P)
    sX, sZ = inputs(tmp, shape, P, kind)
    B, rb = len(sX), dec.record_bytes()
    assert rb == 2 * ((shape[2] * P + 7) // 8) + 1
    tX, tZ = torch.from_numpy(sX.copy()).to(DEV), torch.from_numpy(sZ.copy()).to(DEV)
    bX, bZ = bit_rows(sX), bit_rows(sZ)
    assert bX.shape == (B, (shape[0] * P + 31) // 32) and bZ.shape == (B, (shape[1] * P + 31) // 32)
    for case in cases_of(stop):
        _, p, N = case
        want = reference(tmp, shape, P, case, kind)
        records = pack_records(want[0], want[1], want[2])
        for form, call, a, b in (("byte rows", dec.decode_batch_packed_dev, tX, tZ),
                                 ("bit rows", dec.decode_bits_packed_dev, bX, bZ)):
            buf = torch.full((B + 1, rb), GUARD, dtype=torch.uint8, device=DEV)
            its = torch.full((B + 1, 2), -7, dtype=torch.int32, device=DEV)
            call(a, b, p, N, stop, buf[:B], its[:B])
            torch.cuda.synchronize()
            path = dec.last_path()
            assert "records" in path and "sparse" not in path and ("bit_rows" in path) == (form == "bit rows"), path
            what = label(shape, P, kind, case, form)
            assert np.array_equal(buf[:B].cpu().numpy(), records), what
            assert np.array_equal(its[:B].cpu().numpy(), want[3]), what
            assert bool((buf[B] == GUARD).all()) and bool((its[B] == -7).all()), what + ": guard row written"


# ---- front end ----------------------------------------------------------------------------------------------------------
FRONT_B = 211  # a prime below the 224-sample bound: ragged for every number of samples per wave


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_syndrome_kernel_and_fused_sampler(tmp, shape):
    for P in PS:
        code = code_of(tmp, shape, P)[0]
        dec = gpu(tmp, shape, P)
        B, n = FRONT_B, code.n
        rng = np.random.default_rng(100 * P + shape[2])
        ex = (rng.random((B, n)) < 0.3).astype(np.uint8)
        ez = (rng.random((B, n)) < 0.3).astype(np.uint8)
        ex[0], ez[0], ex[1], ez[1] = 0, 1, 1, 0
        sX = torch.full((B + 1, code.numEqsX), GUARD, dtype=torch.uint8, device=DEV)
        sZ = torch.full((B + 1, code.numEqsZ), GUARD, dtype=torch.uint8, device=DEV)
        dec.syndrome_dev(torch.from_numpy(ex).to(DEV), torch.from_numpy(ez).to(DEV), sX[:B], sZ[:B])
        torch.cuda.synchronize()
        what = "%s P=%d" % (shape_id(shape), P)
        assert np.array_equal(sX[:B].cpu().numpy(), code.syndrome(0, ex)), what
        assert np.array_equal(sZ[:B].cpu().numpy(), code.syndrome(1, ez)), what
        assert bool((sX[B] == GUARD).all()) and bool((sZ[B] == GUARD).all()), what

        seed, start, p = 0x51EC0DE + P, (1 << 32) - 100, 0.05
        nb = (n + 7) // 8
        sX.fill_(GUARD)
        sZ.fill_(GUARD)
        errp = torch.full((B + 1, 2 * nb), GUARD, dtype=torch.uint8, device=DEV)
        dec.sample_syndrome_dev(seed, start, p, sX[:B], sZ[:B], errp[:B])
        torch.cuda.synchronize()
        x, z = depolarizing(seed, start, B, n, p)
        assert x.any() and z.any(), what
        assert np.array_equal(sX[:B].cpu().numpy(), code.syndrome(0, x)), what
        assert np.array_equal(sZ[:B].cpu().numpy(), code.syndrome(1, z)), what
        packed = np.concatenate([np.packbits(x, axis=1, bitorder="little"), np.packbits(z, axis=1, bitorder="little")], 1)
        assert np.array_equal(errp[:B].cpu().numpy(), packed), what
        assert bool((sX[B] == GUARD).all()) and bool((sZ[B] == GUARD).all()) and bool((errp[B] == GUARD).all()), what


# ---- Monte-Carlo on the small codes -----------------------------------------------------------------------------------------
# p = 0.08: at 0.05 ten of the 120 runs have no sample that satisfies its syndrome with a non-zero residual (no
# logical outcome in the oracle's count), at 0.15 eight codes lose one of the outcomes; at 0.08 and 0.1 all have both
MC_N, MC_COUNT, MC_BATCH, MC_P, MC_ITERS = 132, 500, 128, 0.08, 20


def mc_rows(shape):
    return [P for P in PS if shape[2] * P <= MC_N]


def i_minus_p(shape, P):
    """A random sparse 0/1 matrix for the file's fourth line (any such matrix is a valid logical check), about
    three ones per row, so that both outcomes occur on codes of a few qubits too."""
    n2 = 2 * shape[2] * P
    rng = np.random.default_rng(31 * P + shape[0] + shape[1])
    return (rng.random((n2, n2)) < min(0.5, max(0.02, 3.0 / n2))).astype(np.uint8)


_mc = {}


def mc_code(tmp, shape, P):
    key = (shape, P)
    if key not in _mc:
        path = write_file(tmp, shape, P, i_minus_p(shape, P), "_imp")
        code = q.Quantum_LDPC_Code.createFromFile(path)
        _mc[key] = (code, q.DecoderGPU(code, 0), OracleCode(path))
    return _mc[key]


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_monte_carlo_counters(tmp, shape, stop):
    assert mc_rows(shape)[:4] == [1, 2, 3, 9]
    for P in mc_rows(shape):
        code, dec, orc = mc_code(tmp, shape, P)
        assert "runtime-shift" in dec.describe() and "G=%d" % groups(P) in dec.describe()
        seed, start = 0xC0DE + P, 5
        got = dec.monte_carlo(seed, start, MC_COUNT, MC_P, MC_ITERS, stop, batch=MC_BATCH)
        x, z = depolarizing(seed, start, MC_COUNT, code.n, MC_P)
        want, it = oracle_counters(orc, x, z, MC_P, MC_ITERS, stop)
        what = "%s P=%d %s" % (shape_id(shape), P, stop)
        assert want["logical"] > 0 and want["corrected"] > 0, what  # both outcomes of the I-P check occur
        assert {k: got[k] for k in q.MC_COUNTERS} == want, what
        assert got["tested"] == MC_COUNT, what
        assert got["iterationsX"] == int(it[:, 0].sum()) and got["iterationsZ"] == int(it[:, 1].sum()), what

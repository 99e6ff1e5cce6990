"""The wave min-sum kernels (set_option("minsum_wave", 1), bp_wave_minsum.hip) -- the host side: the case table that
tests/test_gpu_wave_minsum.py runs on the device, the CPU engine's outputs those runs are held to (computed here,
once), their non-vacuity, the CPU engine against the numpy restatement on four of the table's codes, the host query
has_wave_minsum, the constants, the CPU engine's refusal and the CLI's.

Table: test_circulant_shapes' SHAPES x PS = 80 codes with its two batches per code ("table", "waves"), the yardstick
the CPU engine under min-sum at scale 160 (test_minsum.minsum_cpu).  Decode cases (stop, p, N):

  fixed     0.03   0, 1, 2, 11
  syndrome  0.03   20 and 11
  ref       0.03   20
  ref       0.005  21

Non-vacuity, on the CPU outputs of the "table" batch alone (test_not_vacuous): every q_final finite; flags 0 in every
code under every case with N >= 1 (at N = 0 no row can have it: every slot is still the channel LLR of p' = 0.02,
ln 49 = 3.89 < ln 99, inside, so both convergence bits are set in all rows of all 80 codes, which is asserted instead);
under (syndrome, 0.03, 20) both sectors of every code hold the counts 1 and 20, and in all 56
codes with G > 1 some wave (G consecutive rows) ends its groups at different counts in both sectors; the same wave
condition under (ref, 0.03, 20), where both sectors hold 1 and 20 in every code except Z of (4,6,12) at P = 1, which
gives {1, 11} (pinned as observed).

Every comparison is bit for bit (q_final as uint32 patterns).  There is no tolerance."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from qec_ldpc_amd.codes import P7, P61, code_path
from test_circulant_shapes import (PS, SHAPES, circulant_matrix, code_of, exponent_tables, groups, inputs, shape_id,
                                   write_file)
from test_general_code import assert_same_decode
from test_minsum import minsum_cpu, minsum_yardstick
from test_priors import prior_vectors

SCALE = 160
FIXED_CASES = (("fixed", 0.03, 0), ("fixed", 0.03, 1), ("fixed", 0.03, 2), ("fixed", 0.03, 11))
SYNDROME_CASES = (("syndrome", 0.03, 20), ("syndrome", 0.03, 11))
REF_CASES = (("ref", 0.03, 20), ("ref", 0.005, 21))
DECODE_CASES = FIXED_CASES + SYNDROME_CASES + REF_CASES
PRIOR_CASES = (("fixed", 0.3, 11), ("syndrome", 0.3, 20))  # under priors p is not used
SYN20, REF20 = ("syndrome", 0.03, 20), ("ref", 0.03, 20)
# (shape, P, sector) -> the counts under (ref, 0.03, 20) where they are not a superset of {1, 20} (as observed)
REF_COUNTS_PINNED = {((4, 6, 12), 1, 1): {1, 11}}
YARDSTICK_CODES = (((2, 2, 4), 3), ((3, 3, 6), 9), ((4, 6, 12), 2), ((4, 5, 10), 22))

_cpu, _ref = {}, {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("wave_minsum")


def cpu_of(tmp, shape, P, scale=SCALE):
    key = (shape, P, scale)
    if key not in _cpu:
        _cpu[key] = minsum_cpu(code_of(tmp, shape, P)[0], scale)
    return _cpu[key]


def reference(tmp, shape, P, case, kind="table", priors=None, scale=SCALE):
    """The CPU engine's (eX, eZ, flags, iters, q_final) of a decode case under min-sum, computed once and shared with
    tests/test_gpu_wave_minsum.py.  priors: None or a kind of test_priors.prior_vectors."""
    key = (shape, P, case, kind, priors, scale)
    if key not in _ref:
        stop, p, N = case
        dec = cpu_of(tmp, shape, P, scale)
        try:
            if priors is not None:
                dec.set_priors(*prior_vectors(code_of(tmp, shape, P)[0].n, priors))
            out = dec.decode_batch(*inputs(tmp, shape, P, kind), p, N, stop, want_iters=True, want_q=True)
        finally:
            dec.set_priors(None, None)
        for a in out:
            a.setflags(write=False)
        _ref[key] = out
    return _ref[key]


def count_sets(it):
    return [set(int(x) for x in it[:, sec]) for sec in (0, 1)]


def wave_mixes(it, G):
    """Per sector: whether some wave (G consecutive rows) ends its groups at different counts."""
    return [any(len(set(int(x) for x in it[k:k + G, sec])) > 1 for k in range(0, len(it), G)) for sec in (0, 1)]


# ---- non-vacuity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_not_vacuous(tmp, shape):
    for P in PS:
        G = groups(P)
        for case in DECODE_CASES:
            out = reference(tmp, shape, P, case)
            assert np.isfinite(out[4]).all(), (shape, P, case)
            if case[2] == 0:  # the slots are the channel LLR ln 49, inside: no row converges
                assert ((out[2] & 12) == 12).all() and (out[3] == 0).all(), (shape, P, case)
            else:
                assert (out[2] == 0).any(), (shape, P, case)
        syn = reference(tmp, shape, P, SYN20)[3]
        for sec, seen in enumerate(count_sets(syn)):
            assert {1, 20} <= seen, (shape, P, sec, seen)
        ref = reference(tmp, shape, P, REF20)[3]
        for sec, seen in enumerate(count_sets(ref)):
            pinned = REF_COUNTS_PINNED.get((shape, P, sec))
            if pinned is not None:
                assert seen == pinned, (shape, P, sec, seen)
            else:
                assert {1, 20} <= seen, (shape, P, sec, seen)
        if G > 1:
            assert wave_mixes(syn, G) == [True, True], (shape, P, "syndrome")
            assert wave_mixes(ref, G) == [True, True], (shape, P, "ref")


def test_the_pinned_rows_are_table_rows():
    assert all(shape in SHAPES and P in PS for shape, P, _ in REF_COUNTS_PINNED)
    assert sum(1 for P in PS if groups(P) > 1) * len(SHAPES) == 56


# ---- the CPU engine against numpy on four of the table's codes -----------------------------------------------------------
@pytest.mark.parametrize("row", YARDSTICK_CODES, ids=lambda r: "%s-P%d" % (shape_id(r[0]), r[1]))
def test_cpu_engine_matches_numpy_on_table_codes(tmp, row):
    shape, P = row
    EX, EZ = exponent_tables(shape, P)
    HX, HZ = circulant_matrix(EX, P), circulant_matrix(EZ, P)
    sX, sZ = inputs(tmp, shape, P)
    for case in (("fixed", 0.03, 11), SYN20):
        stop, p, N = case
        want = minsum_yardstick(HX, HZ, sX, sZ, p, p, SCALE, N, stop)
        assert_same_decode(reference(tmp, shape, P, case), want, "%s P=%d %s" % (shape_id(shape), P, stop))


# ---- the host query --------------------------------------------------------------------------------------------------------
def test_has_wave_minsum(tmp):
    for shape in SHAPES:
        for P in PS:
            assert q.has_wave_minsum(code_of(tmp, shape, P)[0]) is True, (shape, P)
    for name in (P61, P7):
        assert q.has_wave_minsum(q.Quantum_LDPC_Code.createFromFile(code_path(name)))
    assert q.has_wave_minsum(q.QC_LDPC_CSS(3, 3, 6, 13, 3, 2))
    for code in no_wave_codes(tmp):
        assert q.has_wave_minsum(code) is False


def no_wave_codes(tmp):
    """A general code (matrices), a table shape one past the wave (P = 65) and a QC code whose block shape is not in
    the table."""
    from test_sparse_shapes import code_of as named
    return (named("hgp_ham", "general"), q.Quantum_LDPC_Code.createFromFile(write_file(tmp, (4, 5, 10), 65)),
            q.Quantum_LDPC_Code.createFromFile(write_file(tmp, (3, 6, 12), 7)))


# ---- constants, the CPU engine's refusal -----------------------------------------------------------------------------------
def test_constants_and_cpu_refusal(tmp):
    assert q.OPTION["minsum_wave"] == 21 and q.PATH["wave"] == 8192
    dec = q.DecoderCPU(code_of(tmp, (3, 3, 6), 9)[0])
    assert dec.get_option("minsum_wave") == 0
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["minsum_wave"], 1) == -4  # QEC_ERR_UNSUPPORTED
    with pytest.raises(q.QecError, match="CPU engine"):
        dec.set_option("minsum_wave", 1)
    assert dec.get_option("minsum_wave") == 0
    dec.set_option("minsum_wave", 0)
    for bad in (-1, 2):
        with pytest.raises(q.QecError, match="QEC_OPT_MINSUM_WAVE"):
            dec.set_option("minsum_wave", bad)


# ---- CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_minsum_wave_without_the_sparse_engine_and_min_sum(tmp, tmp_path):
    """--minsum-wave 1 needs --engine sparse and --bp-method minsum; other values are refused.  (All of them end
    before a decoder is made.)"""
    from test_osd_host import _cli
    path = write_file(tmp, (2, 2, 4), 3)
    bad = (["--minsum-wave", "1"], ["--engine", "sparse", "--minsum-wave", "1"],
           ["--engine", "cpu", "--bp-method", "minsum", "--minsum-wave", "1"],
           ["--bp-method", "minsum", "--minsum-wave", "1"],
           ["--engine", "sparse", "--bp-method", "minsum", "--minsum-wave", "2"])
    for k, flags in enumerate(bad):
        d = tmp_path / ("bad%d" % k)
        d.mkdir()
        r = _cli(d, flags, path, "2 2 10 20 0.05")
        assert r.returncode == 2 and "minsum-wave" in r.stderr, (flags, r.stderr)

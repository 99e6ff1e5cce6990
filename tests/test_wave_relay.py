"""The wave relay kernels (set_option("relay_wave", 1), bp_wave_relay.hip) -- the host side: the case table that
tests/test_gpu_wave_relay.py runs on the device, the CPU engine's outputs those runs are held to (computed here, once),
their non-vacuity, the CPU engine against the numpy yardstick of test_relay.py on four of the table's codes, the
constants, the CPU engine's refusal and the CLI's.

Table: test_circulant_shapes' SHAPES x PS = 80 codes with its two batches per code ("table", "waves"), the relay tables
test_relay.tables(n) (L = 4 legs), min-sum at scale 160.  Decode cases (S, stop, p, N):

  scalar p   (1, fixed, 0.03, 0) (1, fixed, 0.03, 1) (1, fixed, 0.03, 11) (3, fixed, 0.03, 11)
             (1, syndrome, 0.03, 20) (3, syndrome, 0.03, 20) (3, syndrome, 0.03, 11)
             (1, ref, 0.03, 11) (3, ref, 0.005, 21)
  priors     test_priors.prior_vectors(n, "random") and "special": (3, fixed, 11) (1, syndrome, 20) (3, syndrome, 20)
             (3, ref, 11)

Non-vacuity, on the CPU outputs alone (test_not_vacuous, test_later_solutions): every q_final finite; under
(1, fixed, 0.03, 11) iters / 11 holds 1 and 4 in every code, both sectors, both batches; in all 56 codes with G > 1, on
the "table" batch, both sectors, some wave (G consecutive rows) ends its groups at different counts under
(1, fixed, 0.03, 11) -- groups in different legs under the fixed stop -- and under (1, syndrome, 0.03, 20); under the
latter every shape has, in both sectors, at some P a row solved after leg 0 (no syndrome-fail bit, iters > 20); under
the syndrome stop at N = 20 every shape has, in both sectors, at some P a row solved at S = 1 whose estimate at S = 3
differs (a later, lighter solution replaced the first), and under "random" priors in at least one sector.

Every comparison is bit for bit (q_final as uint32 patterns).  There is no tolerance."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from test_circulant_shapes import (KINDS, PS, SHAPES, circulant_matrix, code_of, exponent_tables, groups, inputs, shape_id,
                                   write_file)
from test_general_code import assert_same_decode
from test_minsum import minsum_cpu
from test_priors import prior_vectors
from test_relay import LEGS, relay_yardstick, tables
from test_wave_minsum import YARDSTICK_CODES, wave_mixes

SCALE = 160
FIX11, SYN20 = (1, "fixed", 0.03, 11), (1, "syndrome", 0.03, 20)
SYN20_S3 = (3, "syndrome", 0.03, 20)
DECODE_CASES = ((1, "fixed", 0.03, 0), (1, "fixed", 0.03, 1), FIX11, (3, "fixed", 0.03, 11),
                SYN20, SYN20_S3, (3, "syndrome", 0.03, 11),
                (1, "ref", 0.03, 11), (3, "ref", 0.005, 21))
PRIOR_CASES = ((3, "fixed", 0.3, 11), (1, "syndrome", 0.3, 20), (3, "syndrome", 0.3, 20), (3, "ref", 0.3, 11))  # p is not used
PRIOR_KINDS = ("random", "special")
FAIL_BIT = (q.SYNDROME_FAIL_X, q.SYNDROME_FAIL_Z)

_cpu, _ref = {}, {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("wave_relay")


def cpu_of(tmp, shape, P, scale=SCALE):
    key = (shape, P, scale)
    if key not in _cpu:
        _cpu[key] = minsum_cpu(code_of(tmp, shape, P)[0], scale)
    return _cpu[key]


def reference(tmp, shape, P, case, kind="table", priors=None, scale=SCALE):
    """The CPU engine's (eX, eZ, flags, iters, q_final) of a decode case under the relay tables of test_relay.py,
    computed once and shared with tests/test_gpu_wave_relay.py.  priors: None or a kind of test_priors.prior_vectors."""
    key = (shape, P, case, kind, priors, scale)
    if key not in _ref:
        S, stop, p, N = case
        dec = cpu_of(tmp, shape, P, scale)
        n = code_of(tmp, shape, P)[0].n
        try:
            if priors is not None:
                dec.set_priors(*prior_vectors(n, priors))
            dec.set_relay(*tables(n), solutions=S)
            out = dec.decode_batch(*inputs(tmp, shape, P, kind), p, N, stop, want_iters=True, want_q=True)
            assert dec.last_path() == {"minsum", "relay"}
        finally:
            dec.set_priors(None, None)
            dec.set_relay(None, None)
        for a in out:
            a.setflags(write=False)
        _ref[key] = out
    return _ref[key]


# ---- non-vacuity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_not_vacuous(tmp, shape):
    late = [False, False]  # per sector: some P has a row solved after leg 0 under (1, syndrome, 0.03, 20)
    for P in PS:
        G = groups(P)
        for kind in KINDS:
            for case in DECODE_CASES:
                assert np.isfinite(reference(tmp, shape, P, case, kind)[4]).all(), (shape, P, kind, case)
            it = reference(tmp, shape, P, FIX11, kind)[3]
            assert (it % 11 == 0).all()
            for sec in (0, 1):
                legs = set(int(x) // 11 for x in it[:, sec])
                assert {1, LEGS} <= legs, (shape, P, kind, sec, legs)
        for kind in PRIOR_KINDS:
            for case in PRIOR_CASES:
                assert np.isfinite(reference(tmp, shape, P, case, "table", kind)[4]).all(), (shape, P, kind, case)
        fix, syn = reference(tmp, shape, P, FIX11), reference(tmp, shape, P, SYN20)
        if G > 1:
            assert wave_mixes(fix[3], G) == [True, True], (shape, P, "fixed")
            assert wave_mixes(syn[3], G) == [True, True], (shape, P, "syndrome")
        for sec in (0, 1):
            late[sec] |= bool((((syn[2] & FAIL_BIT[sec]) == 0) & (syn[3][:, sec] > 20)).any())
    assert late == [True, True], (shape, late)


def replaced(tmp, shape, priors=None):
    """Per sector: at some P a row of the "table" batch is solved at S = 1 and has another estimate at S = 3."""
    p = 0.03 if priors is None else 0.3
    out = [False, False]
    for P in PS:
        one = reference(tmp, shape, P, (1, "syndrome", p, 20), "table", priors)
        three = reference(tmp, shape, P, (3, "syndrome", p, 20), "table", priors)
        for sec in (0, 1):
            solved = (one[2] & FAIL_BIT[sec]) == 0
            out[sec] |= bool((solved & (one[sec] != three[sec]).any(axis=1)).any())
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_later_solutions(tmp, shape):
    assert replaced(tmp, shape) == [True, True], shape
    got = replaced(tmp, shape, "random")
    assert got[0] or got[1], shape
    if shape == (3, 3, 6):
        assert got == [True, False]  # as observed


def test_the_table():
    assert sum(1 for P in PS if groups(P) > 1) * len(SHAPES) == 56 and len(SHAPES) * len(PS) == 80 and LEGS == 4


# ---- the CPU engine against numpy on four of the table's codes -----------------------------------------------------------
@pytest.mark.parametrize("row", YARDSTICK_CODES, ids=lambda r: "%s-P%d" % (shape_id(r[0]), r[1]))
def test_cpu_engine_matches_numpy_on_table_codes(tmp, row):
    shape, P = row
    EX, EZ = exponent_tables(shape, P)
    HX, HZ = circulant_matrix(EX, P), circulant_matrix(EZ, P)
    sX, sZ = inputs(tmp, shape, P)
    gX, gZ = tables(HX.shape[1])
    for case in (FIX11, SYN20_S3):
        S, stop, p, N = case
        want = relay_yardstick(HX, HZ, sX, sZ, p, p, gX, gZ, S, None, None, SCALE, N, stop)
        assert_same_decode(reference(tmp, shape, P, case), want[:5], "%s P=%d %s S=%d" % (shape_id(shape), P, stop, S))


# ---- constants, the CPU engine's refusal -----------------------------------------------------------------------------------
def test_constants_and_cpu_refusal(tmp):
    assert q.OPTION["relay_wave"] == 22 and q.PATH["wave"] == 8192 and q.PATH["relay"] == 4096
    dec = q.DecoderCPU(code_of(tmp, (3, 3, 6), 9)[0])
    assert dec.get_option("relay_wave") == 0
    assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["relay_wave"], 1) == -4  # QEC_ERR_UNSUPPORTED
    with pytest.raises(q.QecError, match="CPU engine"):
        dec.set_option("relay_wave", 1)
    assert dec.get_option("relay_wave") == 0
    dec.set_option("relay_wave", 0)
    for bad in (-1, 2):
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["relay_wave"], bad) == -1  # QEC_ERR_ARG
        with pytest.raises(q.QecError, match="QEC_OPT_RELAY_WAVE"):
            dec.set_option("relay_wave", bad)
    assert dec.get_option("relay_wave") == 0 and dec.get_option("minsum_wave") == 0


# ---- CLI -------------------------------------------------------------------------------------------------------------------
def relay_file(path, n, legs=LEGS):
    gX, gZ = tables(n, legs)
    with open(path, "w") as f:
        for g in (gX, gZ):
            for row in g:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
    return str(path)


def test_cli_refuses_relay_wave_without_its_companions(tmp, tmp_path):
    """--relay-wave needs --engine sparse, --bp-method minsum and --relay FILE; values other than 0 / 1 are refused.
    (All of them end before a decoder is made.)"""
    from test_osd_host import _cli
    path = write_file(tmp, (2, 2, 4), 3)
    rf = relay_file(tmp_path / "relay.txt", 12)
    bad = (["--relay-wave", "1"],
           ["--engine", "sparse", "--bp-method", "minsum", "--relay-wave", "1"],
           ["--engine", "sparse", "--relay", rf, "--relay-wave", "1"],
           ["--bp-method", "minsum", "--relay", rf, "--relay-wave", "1"],
           ["--engine", "cpu", "--bp-method", "minsum", "--relay", rf, "--relay-wave", "1"],
           ["--engine", "sparse", "--bp-method", "minsum", "--relay", rf, "--relay-wave", "2"])
    for k, flags in enumerate(bad):
        d = tmp_path / ("bad%d" % k)
        d.mkdir()
        r = _cli(d, flags, path, "2 2 10 20 0.05")
        assert r.returncode == 2 and "relay-wave" in r.stderr, (flags, r.stderr)

"""Every runtime-shift wave-circulant kernel (bp_decode.hip, the rt<J,K,L> entries of kVariants) at the edges of
its lane layout: the case table that tests/test_gpu_circulant_shapes.py runs on the device, the codes it runs on,
and the oracle's outputs those runs are held to, checked here against the CPU engine and for non-vacuity.

Table: the eight block shapes of the runtime-shift variants (asserted to be exactly kVariants' rt<...> entries)

  (4,5,10) (3,3,6) (2,3,6) (3,4,8) (4,4,8) (3,5,10) (4,6,12) (2,2,4)

at P in {1, 2, 3, 9, 21, 22, 32, 33, 63, 64}: 80 codes, each under three stop rules.  A wave holds G = 64 // P
syndromes on lanes g P + i; the table's P give

  P   1   2   3   9  21  22  32  33  63  64
  G  64  32  21   7   3   2   2   1   1   1
  idle lanes (64 - G P)
      0   0   1   1   1  20   0  31   1   0

Codes: files in the reference's four-line format with the header "J K L P 0 0", the blocks circulant
permutations with explicit exponent tables: default_rng(1000 J + 100 K + P), EX then EZ drawn uniformly from
[0, P), then E[0][0] = 0 and E[R-1][L-1] = P - 1 in both sectors.  The matrices need not commute (BP decodes the
sectors separately).  Inputs: test_gpu_parity.mixed_inputs(code, B, 9 + P, 0.03) -- depolarising, fixed-weight,
random, all-zero and all-one syndromes -- with B = max(24, 3 G + max(1, G // 2)): full waves and, but at P = 21,
22 and 32 (G divides 24), a ragged last one; there the first B - 1 rows are the ragged batch (ragged()).  (With the
seed 7 + P the X sectors of (2,3,6) at P = 33 and (2,2,4) at P = 32 end with {1, 20} alone under both stop rules;
9 + P is the first seed base at which every condition below holds.)  Decode cases (stop, p, N): (fixed, 0.03, 11),
(ref, 0.005, 20), (syndrome, 0.03, 20), and one further N per stop rule of the other parity, (fixed, 0.03, 20),
(ref, 0.005, 21), (syndrome, 0.03, 11); and NAN_CASE, (fixed, 1.5, 5): p' = 1, NaN messages in every code and
batch, outside the domains of the hard-message forms and the scaled division.

A second batch per code, "waves" (wave_inputs, 3 G + max(1, G // 2) rows), is there for the wave-wide votes
(all_live) over several groups, which the table batch cannot pass at G > 1: it holds one or two all-zero rows, so
only at G = 1 a whole wave of zero syndromes.  Wave 0 is zero in X beside non-zero Z syndromes, wave 1 the reverse,
wave 2 holds one single-error syndrome among zero syndromes in both sectors, and dense rows make a ragged last
wave.  assert_waves_not_vacuous holds, on the inputs and the oracle's outputs: the zero waves are G-aligned and
whole; under the fixed stop their G zero-syndrome groups all end hard (every message +0 or 1), so with final
messages the wave-wide hard votes pass with G groups, and without them the zero-syndrome shortcut is taken; the
rows beside a zero wave end at different counts (G >= 7: under both stop rules; G = 3, 2: under the syndrome stop,
but WAVE_MIX_EXEMPT); wave 2 ends hard with clean flags at N = 11 and 20 in 52 of the 80 codes in both sectors
(WAVE2_NOT_HARD pins the rest: P <= 3 mostly, and the X sectors of column weight 2).

Every comparison is bit for bit (q_final as uint32 patterns, NaN matching NaN).  There is no tolerance.

Iteration counts of the oracle on these inputs, X / Z (assert_not_vacuous):

  ref stop, p = 0.005, N = 20   {1, 11, 20} / {1, 11, 20} in all 56 codes with P >= 9 and in 14 of the 24 with
                                P <= 3; the other ten are REF_SMALL_P: (4,5,10), (4,4,8), (4,6,12) at P = 1
                                {1, 11} / {1, 11}; (3,4,8) P = 1 {1, 11, 20} / {1, 11}; (3,5,10) P = 1 {1, 20} /
                                {1, 11}; (2,3,6) P = 1, 2, 3 {1, 20} / {1, 11, 20}; (2,2,4) P = 1 {1, 20} / {1, 20},
                                P = 3 {1, 11, 20} / {1, 20}
  ref stop, N = 21              the same sets with 21 for 20
  syndrome stop, p = 0.03       N = 20: every sector of every code holds 1 and 20, and at least three different
                                counts but in the 14 rows of TWO_COUNTS (all P <= 3: every P = 1 code, (3,3,6) and
                                (2,3,6) at P = 2 and 3, (4,6,12) at P = 2, (2,2,4) at P = 3), where a sector gives
                                {1, 20} alone.  Examples: (4,5,10) P = 64 {1,2,3,4,15,20} / {1,2,3,10,13,20}; (2,2,4)
                                P = 2 {1,2,20} / {1,2,20}; (4,6,12) P = 2 {1,20} / {1,2,6,8,9,20}.  N = 11: the
                                same rule with 11 for 20
  G > 1, ref and syndrome stop  in every code and in both sectors some wave (G consecutive samples) ends its groups
                                at different counts: no row is exempt
  flags                         0 and 15 both occur in every code under every decode case, but 15 under the ref
                                stop at P = 1 in every shape except (2,2,4) (REF_NEVER_15): there no Z syndrome at
                                all ends with both failure bits (test_p1_ref_stop_cannot_fail_everything)
  final messages                at p = 0.03 / 0.005 every shape but (2,2,4) ends cases with NaN messages (observed: up
                                to 18 361 per case; the figure is not asserted, their presence per shape is); under
                                NAN_CASE every code does in both batches, (2,2,4) included (asserted)
"""
import os
import re

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import write_code_file
from test_general_code import assert_same_decode
from test_gpu_parity import mixed_inputs

SHAPES = ((4, 5, 10), (3, 3, 6), (2, 3, 6), (3, 4, 8), (4, 4, 8), (3, 5, 10), (4, 6, 12), (2, 2, 4))
PS = (1, 2, 3, 9, 21, 22, 32, 33, 63, 64)
STOPS = ("fixed", "ref", "syndrome")
# (stop, p, N): the three main cases, then one further N per stop rule of the other parity (the cycle jump
# depends on the parity of the remaining count)
MAIN_CASES = (("fixed", 0.03, 11), ("ref", 0.005, 20), ("syndrome", 0.03, 20))
PARITY_CASES = (("fixed", 0.03, 20), ("ref", 0.005, 21), ("syndrome", 0.03, 11))
# p' = (2/3) 1.5 = 1, 1 - p' = 0: 0/0 in the variable update, NaN messages in every code ((2,2,4) has none at
# p = 0.03), and a p' outside the domains of the hard-message forms and the scaled division
NAN_CASE = ("fixed", 1.5, 5)
DECODE_CASES = MAIN_CASES + PARITY_CASES + (NAN_CASE,)
P_INPUT = 0.03
INPUT_SEED = 9


def shape_id(shape):
    return "%d-%d-%d" % shape


def groups(P):
    """Syndromes per wave."""
    return 64 // P


def batch(P):
    G = groups(P)
    return max(24, 3 * G + max(1, G // 2))


def ragged(P):
    """Rows of the batch that leave the last wave partly filled: all of them, or one fewer where G divides the
    batch (P = 21, 22, 32).  The device module decodes these rows as a batch of their own."""
    B, G = batch(P), groups(P)
    return B - 1 if G > 1 and B % G == 0 else B


def cases_of(stop):
    return tuple(c for c in DECODE_CASES if c[0] == stop)


def variant_shapes():
    """The rt<J, K, L, ...> entries of kVariants, read out of bp_decode.hip."""
    src = os.path.join(os.path.dirname(os.path.abspath(q.__file__)), "csrc", "bp_decode.hip")
    text = open(src).read()
    table = re.search(r"static const Variant kVariants\[\] = \{(.*?)\n\};", text, re.S).group(1)
    table = re.sub(r"//[^\n]*", "", table)  # comments may speak of rt<...>
    return [tuple(int(x) for x in m) for m in re.findall(r"\brt<\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*[,>]", table)]


# ---- the codes ---------------------------------------------------------------------------------------------
def exponent_tables(shape, P):
    J, K, L = shape
    rng = np.random.default_rng(1000 * J + 100 * K + P)
    EX = rng.integers(0, P, (J, L)).astype(np.int32)
    EZ = rng.integers(0, P, (K, L)).astype(np.int32)
    for E in (EX, EZ):
        E[0, 0] = 0
        E[-1, -1] = P - 1  # shift 0 and the largest shift both occur
    return EX, EZ


def circulant_matrix(E, P):
    """Block (r, l) is the circulant permutation whose row i has its 1 at column (E[r][l] + i) mod P."""
    R, L = E.shape
    H = np.zeros((R * P, L * P), dtype=np.uint8)
    i = np.arange(P)
    for r in range(R):
        for l in range(L):
            H[r * P + i, l * P + (E[r, l] + i) % P] = 1
    return H


_codes, _inputs, _ref = {}, {}, {}


def write_file(tmp, shape, P, IMP=None, tag=""):
    J, K, L = shape
    EX, EZ = exponent_tables(shape, P)
    path = str(tmp / ("rt_%s_P%d%s.txt" % (shape_id(shape), P, tag)))
    # a one-entry I-P line stands for the all-zero matrix (both loaders zero-fill a short line)
    imp = np.zeros((1, 1), dtype=np.uint8) if IMP is None else IMP
    return write_code_file(path, J, K, L, P, 0, 0, circulant_matrix(EX, P), circulant_matrix(EZ, P), imp)


def code_of(tmp, shape, P):
    """(code, oracle) of a table row, its file written under tmp on first use."""
    key = (shape, P)
    if key not in _codes:
        path = write_file(tmp, shape, P)
        _codes[key] = (q.Quantum_LDPC_Code.createFromFile(path), OracleCode(path))
    return _codes[key]


KINDS = ("table", "waves")  # the two batches of every code


def wave_rows(P):
    """Rows of the "waves" batch: three full waves and a ragged one."""
    G = groups(P)
    return 3 * G + max(1, G // 2)


def single_error(code, G, sector):
    """G syndromes, all zero but the first: that of one error on qubit 3 mod n."""
    e = np.zeros((G, code.n), dtype=np.uint8)
    e[0, 3 % code.n] = 1
    return code.syndrome(sector, e)


def wave_inputs(tmp, shape, P):
    """The batch that lets whole waves of several groups pass the wave-wide votes (bp_decode.hip, all_live): wave 0
    (rows [0, G)) has zero X syndromes beside mixed Z syndromes, wave 1 the reverse, wave 2 holds in both sectors one
    single-error syndrome among zero syndromes (not a zero wave, yet every group can end hard), and max(1, G // 2)
    dense rows make the ragged last wave.  The mixed rows are rows B - 1, 0, B - 2, 1, ... of the table batch
    (dense random syndromes from its back, the all-one row first, and depolarising samples from its front), the
    dense rows its last."""
    code = code_of(tmp, shape, P)[0]
    G, B = groups(P), batch(P)
    tX, tZ = inputs(tmp, shape, P)
    mix = np.where(np.arange(G) % 2 == 0, B - 1 - np.arange(G) // 2, np.arange(G) // 2)
    tail = max(1, G // 2)
    zX, zZ = np.zeros((G, tX.shape[1]), np.uint8), np.zeros((G, tZ.shape[1]), np.uint8)
    sX = np.concatenate([zX, tX[mix], single_error(code, G, 0), tX[-tail:]])
    sZ = np.concatenate([tZ[mix], zZ, single_error(code, G, 1), tZ[-tail:]])
    assert len(sX) == len(sZ) == wave_rows(P)
    return sX, sZ


def inputs(tmp, shape, P, kind="table"):
    key = (shape, P, kind)
    if key not in _inputs:
        if kind == "table":
            sX, sZ = mixed_inputs(code_of(tmp, shape, P)[0], batch(P), INPUT_SEED + P, P_INPUT)
        else:
            assert kind == "waves"
            sX, sZ = wave_inputs(tmp, shape, P)
        for s in (sX, sZ):
            s.setflags(write=False)
        _inputs[key] = (sX, sZ)
    return _inputs[key]


def reference(tmp, shape, P, case, kind="table"):
    """The oracle's (eX, eZ, flags, iters, q_final) of a decode case, computed once."""
    key = (shape, P, case, kind)
    if key not in _ref:
        stop, p, N = case
        out = code_of(tmp, shape, P)[1].decode_batch(*inputs(tmp, shape, P, kind), p, N, stop, want_q=True)
        for a in out:
            a.setflags(write=False)
        _ref[key] = out
    return _ref[key]


# ---- non-vacuity, on the oracle's outputs alone ------------------------------------------------------------------
FULL = ({1, 11, 20}, {1, 11, 20})
# Ref stop at P <= 3: (shape, P) -> (counts X, counts Z) where they are not FULL (asserted as observed).  A sector
# of R <= 18 checks has few syndromes: on some of these codes none of them stops at the second test, or none runs
# to the cap.
REF_SMALL_P = {
    ((4, 5, 10), 1): ({1, 11}, {1, 11}),
    ((2, 3, 6), 1): ({1, 20}, {1, 11, 20}),
    ((2, 3, 6), 2): ({1, 20}, {1, 11, 20}),
    ((2, 3, 6), 3): ({1, 20}, {1, 11, 20}),
    ((3, 4, 8), 1): ({1, 11, 20}, {1, 11}),
    ((4, 4, 8), 1): ({1, 11}, {1, 11}),
    ((3, 5, 10), 1): ({1, 20}, {1, 11}),
    ((4, 6, 12), 1): ({1, 11}, {1, 11}),
    ((2, 2, 4), 1): ({1, 20}, {1, 20}),
    ((2, 2, 4), 3): ({1, 11, 20}, {1, 20}),
}
# Syndrome stop: rows (P <= 3 only) where a sector ends with {1, cap} alone -- such a sector satisfies its
# syndrome at the first hard decision or never.  Every other row shows at least three counts in both sectors.
TWO_COUNTS = frozenset([((4, 5, 10), 1), ((3, 3, 6), 1), ((3, 3, 6), 2), ((3, 3, 6), 3), ((2, 3, 6), 1), ((2, 3, 6), 2),
                        ((2, 3, 6), 3), ((3, 4, 8), 1), ((4, 4, 8), 1), ((3, 5, 10), 1), ((4, 6, 12), 1), ((4, 6, 12), 2),
                        ((2, 2, 4), 1), ((2, 2, 4), 3)])
# Ref stop at P = 1: no Z syndrome of these codes (K checks over all L qubits) ends with both of its failure
# bits set, so flags 15 cannot occur on any input (test_p1_ref_stop_cannot_fail_everything enumerates them).
# (2,2,4) at P = 1 is not among them.
REF_NEVER_15 = frozenset((shape, 1) for shape in SHAPES if shape != (2, 2, 4))


def count_sets(it):
    return [set(int(x) for x in it[:, sec]) for sec in (0, 1)]


def wave_mixes(it, G, sec):
    """Some block of G consecutive samples (one wave's groups) ends sector sec at different counts: that wave
    keeps running with some of its groups finished."""
    return any(len(set(it[lo:lo + G, sec].tolist())) > 1 for lo in range(0, len(it), G))


def with_cap(sets, N):
    return tuple({N if k == 20 else k for k in s} for s in sets)


def assert_not_vacuous(tmp, shape, P):
    G = groups(P)
    assert {k for k in REF_SMALL_P} | TWO_COUNTS <= {(s, p) for s in SHAPES for p in PS if p <= 3}
    for kind in KINDS:
        _, _, _, it, qf = reference(tmp, shape, P, NAN_CASE, kind)
        assert (it == NAN_CASE[2]).all() and np.isnan(qf).any(), (shape, P, kind)
    for case in MAIN_CASES + PARITY_CASES:
        stop, _, N = case
        _, _, flags, it, qf = reference(tmp, shape, P, case)
        what = (shape, P, case)
        assert (flags == 0).any(), what
        if stop == "ref" and (shape, P) in REF_NEVER_15:
            assert not (flags == 15).any(), what
        else:
            assert (flags == 15).any(), what
        seen = count_sets(it)
        if stop == "fixed":
            assert seen == [{N}, {N}], (what, seen)
            continue
        if G > 1:  # no row is exempt, and it holds in both sectors
            assert wave_mixes(it, G, 0) and wave_mixes(it, G, 1), what
        if stop == "ref":
            assert tuple(seen) == with_cap(REF_SMALL_P.get((shape, P), FULL), N), (what, seen)
        else:
            for s in seen:
                assert 1 in s and N in s, (what, seen)
            if (shape, P) in TWO_COUNTS:
                assert {1, N} in seen, (what, seen)  # the exemption is not stale
            else:
                assert len(seen[0]) >= 3 and len(seen[1]) >= 3, (what, seen)


# The "waves" batch.  Wave 2 under the fixed stop: (shape, P) -> which sectors (X, Z) do NOT end with every message
# of the whole wave exactly +0 or 1 and clean flags (asserted as observed; every other row and sector does).  A
# single error is beyond BP on the codes of a few qubits, and in every X sector of column weight 2 but one.
WAVE2_NOT_HARD = {
    ((4, 5, 10), 1): "XZ", ((4, 5, 10), 2): "XZ",
    ((3, 3, 6), 1): "XZ", ((3, 3, 6), 2): "XZ", ((3, 3, 6), 3): "X",
    ((2, 3, 6), 1): "XZ", ((2, 3, 6), 2): "XZ", ((2, 3, 6), 3): "XZ", ((2, 3, 6), 9): "X", ((2, 3, 6), 21): "X",
    ((2, 3, 6), 22): "X", ((2, 3, 6), 32): "X", ((2, 3, 6), 33): "X",
    ((3, 4, 8), 1): "XZ", ((3, 4, 8), 2): "XZ", ((3, 4, 8), 3): "X",
    ((4, 4, 8), 1): "XZ",
    ((3, 5, 10), 1): "XZ", ((3, 5, 10), 2): "X",
    ((4, 6, 12), 1): "XZ", ((4, 6, 12), 2): "XZ",
    ((2, 2, 4), 1): "XZ", ((2, 2, 4), 2): "XZ", ((2, 2, 4), 3): "XZ", ((2, 2, 4), 9): "XZ", ((2, 2, 4), 21): "Z",
    ((2, 2, 4), 32): "X", ((2, 2, 4), 33): "X",
}
# (shape, P, sector) with G > 1 whose mixed rows beside the other sector's zero wave all end at one count under
# the syndrome stop (G = 3 and 2: three and two rows)
WAVE_MIX_EXEMPT = frozenset([((2, 3, 6), 21, 0), ((2, 2, 4), 32, 0)])


def assert_waves_not_vacuous(tmp, shape, P):
    """On the inputs and the oracle's outputs.  Rows [0, G) are one wave with zero X syndromes and non-zero Z
    syndromes, rows [G, 2 G) the reverse: without final messages the wave takes the zero-syndrome shortcut in one
    sector with all its G groups and decodes the other; with them it runs BP on G zero syndromes, which all end hard
    (every message +0 or 1): the wave-wide hard-message votes pass with G groups.  Rows [2 G, 3 G) are not a zero
    wave, and but for WAVE2_NOT_HARD end hard with clean flags, at N = 11 as at N = 20: a state that the near-hard
    jump and the cycle jump skip from."""
    J, K, L = shape
    G = groups(P)
    sX, sZ = inputs(tmp, shape, P, "waves")
    assert len(sX) == wave_rows(P) <= 224 and (len(sX) % G != 0 or G == 1)
    assert not sX[:G].any() and sZ[0].all() and not sZ[G:2 * G].any() and sX[G].all()  # the all-one row leads
    for s in (sX, sZ):
        assert s[2 * G].any() and not s[2 * G + 1:3 * G].any() and s[3 * G:].any()
    split = J * P * L
    hard = lambda a: bool(np.isin(a, (0.0, 1.0)).all())  # noqa: E731
    for case in MAIN_CASES + PARITY_CASES:
        stop, _, N = case
        _, _, flags, it, qf = reference(tmp, shape, P, case, "waves")
        what = (shape, P, case)
        qs = (qf[:, :split], qf[:, split:])
        zero = (slice(0, G), slice(G, 2 * G))  # the zero wave of sector X, of sector Z
        for sec in (0, 1):
            if stop == "fixed":
                assert hard(qs[sec][zero[sec]]) and (it[:, sec] == N).all(), what
            else:
                assert (it[zero[sec], sec] == 1).all(), what
                mixed = len(set(it[zero[1 - sec], sec].tolist())) > 1
                if G >= 7:
                    assert mixed, what
                elif G > 1 and case in MAIN_CASES and stop == "syndrome":
                    assert mixed == ((shape, P, sec) not in WAVE_MIX_EXEMPT), what
        if stop == "fixed":
            w2 = slice(2 * G, 3 * G)
            bits = (q.SYNDROME_FAIL_X | q.CONVERGENCE_FAIL_X, q.SYNDROME_FAIL_Z | q.CONVERGENCE_FAIL_Z)
            got = "".join("XZ"[sec] for sec in (0, 1) if not (hard(qs[sec][w2]) and not (flags[w2] & bits[sec]).any()))
            want = WAVE2_NOT_HARD.get((shape, P), "")
            # pinned at N = 11; a sector that is hard by then stays so ((2,2,4) at P = 9: X turns hard later)
            assert got == want if case in MAIN_CASES else set(got) <= set(want), (what, got)
    # in every shape wave 2 ends hard with G > 1 groups at some P, in Z and, but with column weight 2 ((2,3,6)), in X
    for sec in "XZ" if (J, K) != (2, 3) else "Z":
        assert any(groups(p) > 1 and sec not in WAVE2_NOT_HARD.get((shape, p), "") for p in PS), (shape, sec)


# ---- tests ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("circulant_shapes")


def test_table_is_the_variant_table():
    """A runtime-shift variant added to kVariants without a row here fails."""
    got = variant_shapes()
    assert len(got) == len(set(got)) == len(SHAPES)
    assert set(got) == set(SHAPES)
    assert len(SHAPES) * len(PS) == 80
    assert [groups(P) for P in PS] == [64, 32, 21, 7, 3, 2, 2, 1, 1, 1]
    assert [64 - groups(P) * P for P in PS] == [0, 0, 1, 1, 1, 20, 0, 31, 1, 0]
    assert [batch(P) for P in PS] == [224, 112, 73, 24, 24, 24, 24, 24, 24, 24]
    # full waves, and a ragged last one either in the batch itself or in its first ragged(P) rows
    assert [ragged(P) for P in PS] == [224, 112, 73, 24, 23, 23, 23, 24, 24, 24]
    for P in PS:
        assert batch(P) >= 3 * groups(P) and (ragged(P) % groups(P) != 0 or groups(P) == 1)
    # (4,6,12) alone fills the iteration-0 table and has K > 5
    tab = {s: (1 << s[0]) * s[0] + (1 << s[1]) * s[1] for s in SHAPES}
    assert tab[(4, 6, 12)] == 448 == max(tab.values()) and [s for s in SHAPES if max(s[:2]) > 5] == [(4, 6, 12)]


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_codes_load_with_the_written_exponents(tmp, shape):
    J, K, L = shape
    for P in PS:
        code, orc = code_of(tmp, shape, P)
        EX, EZ = exponent_tables(shape, P)
        assert (code.J, code.K, code.L, code.P, code.sigma, code.tau) == (J, K, L, P, 0, 0)
        assert (code.n, code.numEqsX, code.numEqsZ) == (L * P, J * P, K * P) == (orc.n, orc.mX, orc.mZ)
        assert np.array_equal(code.exponents(0), EX) and np.array_equal(code.exponents(1), EZ)
        for E in (EX, EZ):
            assert E.min() == 0 and E.max() == P - 1 and E[0, 0] == 0 and E[-1, -1] == P - 1
        assert np.array_equal(code.pcm(0), circulant_matrix(EX, P))
        assert np.array_equal(code.pcm(1), circulant_matrix(EZ, P))
        sX, sZ = inputs(tmp, shape, P)
        assert len(sX) == len(sZ) == batch(P) <= 224 and code.n <= 768
        assert (~sX.any(1) & ~sZ.any(1)).any() and (sX.all(1) & sZ.all(1)).any()  # all-zero and all-one rows


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_cpu_engine_matches_oracle(tmp, shape):
    nans = 0
    for P in PS:
        dec = q.DecoderCPU(code_of(tmp, shape, P)[0])
        for kind in KINDS:
            sX, sZ = inputs(tmp, shape, P, kind)
            for case in DECODE_CASES:
                stop, p, N = case
                got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                want = reference(tmp, shape, P, case, kind)
                assert_same_decode(got, want, "%s P=%d %s %s p=%g N=%d" % (shape_id(shape), P, kind, stop, p, N))
                if kind == "table" and case != NAN_CASE:
                    nans += int(np.isnan(want[4]).sum())
    # at p = 0.03 / 0.005 the comparisons include non-finite final messages too, but for (2,2,4) (four messages per
    # check); NAN_CASE brings them to every code (assert_not_vacuous)
    assert (nans > 0) == (shape != (2, 2, 4))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_oracle_outputs_are_not_vacuous(tmp, shape):
    for P in PS:
        assert_not_vacuous(tmp, shape, P)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_waves_batch_is_not_vacuous(tmp, shape):
    for P in PS:
        assert_waves_not_vacuous(tmp, shape, P)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_p1_ref_stop_cannot_fail_everything(tmp, shape):
    """REF_NEVER_15 is a property of the P = 1 codes, not of the sampled inputs: over every Z syndrome (the
    sectors decode independently) no sector ends with SYNDROME_FAIL_Z and CONVERGENCE_FAIL_Z together."""
    import itertools
    J, K, _ = shape
    orc = code_of(tmp, shape, 1)[1]
    sZ = np.array(list(itertools.product((0, 1), repeat=K)), dtype=np.uint8)
    sX = np.zeros((len(sZ), J), dtype=np.uint8)
    both = q.SYNDROME_FAIL_Z | q.CONVERGENCE_FAIL_Z
    for stop, p, N in cases_of("ref"):
        flags = orc.decode_batch(sX, sZ, p, N, stop)[2]
        assert ((flags & both) == both).any() == ((shape, 1) not in REF_NEVER_15), (shape, N)

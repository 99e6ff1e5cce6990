"""The OSD stage (osd.hip, osd_host.cpp; DESIGN.md sections 1.2 - 1.4, section 6) at the boundaries of its own
arithmetic, without a GPU: a table of seven shapes built to sit on them, one numpy yardstick for both column keys and
both scores, the conditions that keep the table from being vacuous (asserted on the yardstick alone), and the host
implementation held to the yardstick on every row.  tests/test_gpu_osd_shapes.py holds the kernel to the same table.

What each shape pins (sw = n >> 5 and sbit = 1 << (n & 31) place the syndrome column, W = ceil((n + 1) / 32) words a
row, chunks of 64 rows with one bit of the `used` mask each):

  w31    n = 31: W = 1, the syndrome column is bit 31 of the only word; X has one row (rank 1); Z is 31 x 31 and
         invertible (unit upper triangular), so f = 0 and the sweep has nothing to flip
  w32    n = 32: the syndrome column alone in word 1; mZ = 33 > n, deficient by count
  w63    n = 63: the syndrome column is bit 31 of word 1; X full rank, Z deficient
  w64    n = 64: W = 3; X is 64 x 64 and invertible: one full chunk in which every row is a pivot row, and the
         consistency scan must find nothing; Z has 65 rows: a second chunk of one row
  c128   n = 160, 128 / 129 rows: two full chunks beside a third of one row, rows across five words; qubits
         152 .. 159 are in no X check and 0 .. 7 in no Z check
  n2048  n = 2048 = the kernel's limit, 192 / 40 rows: W = Ws = 65, so the "words" form of the row update takes its
         second trip (word 64 holds the syndrome column alone); mmax = 192 while the Z loops run to 40; at most 1280
         qubits are in a Z check; the largest LDS image
  m2048  n = 160, 3 / 2048 rows: 32 chunks, bit 31 of `used`; Z rows of weight 1 and 2; X has 3 rows in an LDS
         image sized for 2048

Two conditions cannot hold as they are usually worded, for any matrix.  No qubit column lies in word 64 of n2048
(columns 2016 .. 2047 are word 63, the 64th): the conditions below ask for a pivot and for one of the first lambda
non-pivot columns in word 63, and for an elimination that changes the syndrome column, the only bit of word 64.  And a
column in no check is all zero, so it is never a pivot column: the conditions ask that such a column is walked before
the last pivot is found (the kernel's "no row has the bit" path) and that one is among the first lambda non-pivot
columns."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from qec_ldpc_amd.synthetic import depolarizing_errors
from test_minsum import osd_key_llr
from test_osd_host import FAIL, gf2_rank, inconsistent_syndrome, osd_keys, random_soft
from test_osd_weighted_host import LDS_LIMIT, WeightedYardstick, kind_of, lds_words, priors_of

F32 = np.float32
ORDERS = (0, 1, 2, 10, 64)
METHODS = (0, 1)                 # QEC_OPT_BP_METHOD: the product rule's key, the LLR key
RULES = ("h", "random", "two")   # the Hamming score; the weighted score under priors_of(n, kind)
MAX_ROW, MAX_COL = 32, 16        # what the sparse-graph engine takes

# name -> (n, mX, mZ, rank X, rank Z)
OSD_SHAPES = {
    "w31": (31, 1, 31, 1, 31),
    "w32": (32, 7, 33, 7, 29),
    "w63": (63, 20, 40, 20, 33),
    "w64": (64, 64, 65, 64, 57),
    "c128": (160, 128, 129, 118, 120),
    "n2048": (2048, 192, 40, 180, 40),
    "m2048": (160, 3, 2048, 3, 150),
}
SMALL_B = {"n2048": 4, "m2048": 4}
B_DEFAULT = 12
SEEDS = {"w31": 31, "w32": 32, "w63": 63, "w64": 64, "c128": 128, "n2048": 2048, "m2048": 2049}
ERROR_P = {"n2048": 0.01}
# n2048: the walk ends after a few hundred of the 2048 columns, and a column in no check (the key of 0.5f or of
# +0.0f) is walked only if few real columns rank above it: the share of soft values above 0.5 / below zero there
FEW_SUSPECTS = {"n2048": 0.03}


# ---- the matrices ----------------------------------------------------------------------------------------------
def _fill(rng, H, rows, cols, wlo, whi, cap):
    """For each of `rows`, ones in w more columns drawn from `cols`, w in [wlo, whi], no column above `cap`."""
    cols = np.asarray(cols, dtype=np.int64)
    for r in rows:
        w = int(rng.integers(wlo, whi + 1))
        free = cols[H[:, cols].sum(axis=0) < cap]
        if w and len(free):
            H[r, rng.choice(free, size=min(w, len(free)), replace=False)] = 1


def systematic(rng, m, n, wlo, whi, cols=None, cap=MAX_COL):
    """[I | R] up to a column permutation, on the columns `cols` (all n by default): full row rank m.  Each row
    has wlo .. whi ones in R."""
    cols = rng.permutation(np.arange(n) if cols is None else np.asarray(cols))
    assert m <= len(cols)
    H = np.zeros((m, n), dtype=np.uint8)
    H[np.arange(m), cols[:m]] = 1
    _fill(rng, H, range(m), cols[m:], wlo, whi, cap)
    return H


def unit_upper(rng, m, whi):
    """m x m, ones on the diagonal and up to whi more to the right of it in each row: invertible."""
    H = np.eye(m, dtype=np.uint8)
    for r in range(m - 1):
        _fill(rng, H, [r], np.arange(r + 1, m), 0, whi, MAX_COL)
    return H


def deficient(rng, m, n, r, wlo, whi, cols=None):
    """r independent rows [I | R] and m - r dependent ones, by turns a duplicate of an earlier row and the XOR of
    two earlier rows with disjoint supports (never of row 0); then the rows shuffled, so that the rows the
    elimination leaves without a pivot are not the last ones, with row 0 put last: no other row has its identity
    column, so the last row is a pivot row in every column order.  Rank r."""
    H = np.zeros((m, n), dtype=np.uint8)
    H[:r] = systematic(rng, r, n, wlo, whi, cols, cap=MAX_COL - 6)
    for i in range(r, m):
        for attempt in range(4000):
            a, b = (int(x) for x in rng.integers(1, i, 2))
            xor = (i - r) % 2 == 1 and attempt < 2000
            if xor and (a == b or (H[a] & H[b]).any()):
                continue
            row = H[a] ^ H[b] if xor else H[a].copy()
            if row.sum() <= MAX_ROW and ((H[:i].sum(axis=0) + row) <= MAX_COL).all():
                H[i] = row
                break
        else:
            raise AssertionError("no dependent row fits")
    return np.ascontiguousarray(H[np.append(1 + rng.permutation(m - 1), 0)])


def _m2048_z():
    """2048 rows on the qubits 0 .. 149: row r holds qubit floor(150 r / 2048), so a qubit's rows are about 14 in
    a run; every eighth row holds a second qubit, 97 (r / 8) mod 140 (unless that is the first).  The
    qubits 140 .. 149 are in the rows of their own runs only, so the pivot rows of 146 .. 149 are in the last chunk
    of 64 rows (1984 .. 2047)."""
    H = np.zeros((2048, 160), dtype=np.uint8)
    for r in range(2048):
        c = 150 * r // 2048
        H[r, c] = 1
        if r % 8 == 7:
            d = (97 * (r // 8)) % 140
            H[r, d] = 1
    return H


def _build(name):
    rng = np.random.default_rng(20250000 + SEEDS[name])
    if name == "w31":
        HX = np.zeros((1, 31), dtype=np.uint8)
        HX[0, rng.choice(31, 9, replace=False)] = 1
        return HX, unit_upper(rng, 31, 2)
    if name == "w32":
        return systematic(rng, 7, 32, 3, 8), deficient(rng, 33, 32, 29, 0, 2)
    if name == "w63":
        return systematic(rng, 20, 63, 3, 9), deficient(rng, 40, 63, 33, 1, 5)
    if name == "w64":
        return unit_upper(rng, 64, 3), deficient(rng, 65, 64, 57, 0, 3)
    if name == "c128":
        return (deficient(rng, 128, 160, 118, 1, 4, cols=np.arange(0, 152)),
                deficient(rng, 129, 160, 120, 1, 4, cols=np.arange(8, 160)))
    if name == "n2048":
        return deficient(rng, 192, 2048, 180, 6, 28), systematic(rng, 40, 2048, 24, 31)
    assert name == "m2048"
    return systematic(rng, 3, 160, 14, 24), _m2048_z()


_mats, _codes, _ys, _batches, _weights, _want = {}, {}, {}, {}, {}, {}


def matrices(name):
    if name not in _mats:
        _mats[name] = tuple(np.ascontiguousarray(H, dtype=np.uint8) for H in _build(name))
    return _mats[name]


def code_of(name):
    if name not in _codes:
        _codes[name] = q.Quantum_LDPC_Code.createFromMatrices(*matrices(name))
    return _codes[name]


def fits(name, lam, weighted):
    """Whether osd_dev_unsupported lets the kernel run this shape at lambda, by the restated osd_lds_words."""
    n, mX, mZ = OSD_SHAPES[name][:3]
    return lds_words(max(mX, mZ), n, lam, weighted) <= LDS_LIMIT


# ---- the yardstick ------------------------------------------------------------------------------------------------
class ShapeYardstick(WeightedYardstick):
    """WeightedYardstick with the key of the BP method, and the three inputs that leave a sector as it is looked
    at before `reduce` (which masks the syndrome with & 1)."""

    def __init__(self, HX, HZ, method):
        if method:
            super().__init__(HX, HZ, key_fn=osd_key_llr, absent=F32(0.0))
        else:
            super().__init__(HX, HZ, key_fn=osd_keys, absent=F32(0.5))

    def sector(self, sec, s, qrow):
        """For inconsistent_syndrome: None if [H | s] is inconsistent."""
        return None if self.reduce(sec, s, qrow) is None else True

    def outcome(self, sec, s, qrow, fail):
        """-> ("skipped" | "bad" | "inconsistent", None) or ("ok", the reduced sector)."""
        if not fail:
            return "skipped", None
        if (np.asarray(s) > 1).any():
            return "bad", None
        red = self.reduce(sec, s, qrow)
        return ("inconsistent", None) if red is None else ("ok", red)


def yardstick(name, method):
    if (name, method) not in _ys:
        _ys[name, method] = ShapeYardstick(*matrices(name), method)
    return _ys[name, method]


def weights_of(name, kind):
    """The integer weight tables (wX, wZ) of priors_of(n, kind), read from the library (test_weight_table of
    tests/test_osd_weighted_host.py holds them to the formula)."""
    if (name, kind) not in _weights:
        dec = q.DecoderCPU(code_of(name))
        dec.set_priors(*priors_of(OSD_SHAPES[name][0], kind))
        _weights[name, kind] = dec.osd_weights()
    return _weights[name, kind]


# ---- the batch of a shape ------------------------------------------------------------------------------------------
def random_llr(rng, B, qn, negative=0.5):
    """LLR soft input: both signs (a share `negative` below zero), magnitudes from 2^-12 up to 2^30 (the cap, which some values take exactly),
    exact ties (half the values on a coarse grid), and +0.0 / -0.0, the former being the value that a column in no
    check stands for, so that such columns tie with real ones and the index breaks the tie."""
    mag = np.exp2(rng.uniform(-12.0, 30.0, (B, qn))).astype(F32)
    grid = np.exp2(rng.integers(-3, 31, (B, qn)).astype(np.float64)).astype(F32)
    v = np.where(rng.random((B, qn)) < 0.5, grid, mag).astype(F32)
    v = np.minimum(v, F32(2.0 ** 30))
    v = np.where(rng.random((B, qn)) < negative, -v, v).astype(F32)
    bits = v.view(np.uint32).copy()
    r = rng.random((B, qn))
    bits[r < 0.10] = 0x00000000
    bits[(r >= 0.10) & (r < 0.15)] = 0x80000000
    return bits.view(F32)


def batch(name, method, B=None):
    """(sX, sZ, soft, eX, eZ, flags) of a shape: syndromes sampled from errors; sample 1 of every rank-deficient
    sector made inconsistent; a byte 2 in sample 2's X syndrome and a byte 255 in sample 3's Z syndrome; junk
    estimates, random convergence bits; fail bits: sample 0 X only, sample 5 Z only, the last sample none (both
    where there are 12 samples: a batch of 4 has a role for each sample already), all others both."""
    B = SMALL_B.get(name, B_DEFAULT) if B is None else B
    if (name, method, B) not in _batches:
        n, mX, mZ, rX, rZ = OSD_SHAPES[name]
        HX, HZ = matrices(name)
        ys = yardstick(name, method)
        rng = np.random.default_rng(7000 + SEEDS[name])  # the same draws for both keys, up to the soft input
        x, z = depolarizing_errors(n, 4000 + SEEDS[name], B, ERROR_P.get(name, 0.08))
        sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        if B > 1:
            for sec, s in enumerate((sX, sZ)):
                if ys.rank[sec] < ys.H[sec].shape[0]:
                    s[1] = inconsistent_syndrome(ys, sec, s[1], rng)
        if B > 2:
            sX[2, mX // 2] = 2
        if B > 3:
            sZ[3, mZ - 1] = 255
        eX = rng.integers(0, 2, (B, n), dtype=np.uint8)
        eZ = rng.integers(0, 2, (B, n), dtype=np.uint8)
        fail = np.full(B, 3, dtype=np.uint8)
        fail[0] = 1
        if B > 5:
            fail[5] = 2
        if B >= B_DEFAULT:
            fail[B - 1] = 0
        flags = (fail | (rng.integers(0, 4, B) << 2)).astype(np.uint8)
        srng = np.random.default_rng(9000 + SEEDS[name] + method)
        if name not in FEW_SUSPECTS:
            soft = random_llr(srng, B, ys.qn) if method else random_soft(srng, B, ys.qn)
        elif method:
            soft = random_llr(srng, B, ys.qn, negative=FEW_SUSPECTS[name])
        else:  # halving is exact: ties, NaN, zeros and signs stay what random_soft made them
            soft = random_soft(srng, B, ys.qn)
            soft = np.where(srng.random(soft.shape) < 1.0 - 2 * FEW_SUSPECTS[name], soft * F32(0.5), soft)
        _batches[name, method, B] = (sX, sZ, np.ascontiguousarray(soft, dtype=F32), eX, eZ, flags)
    return _batches[name, method, B]


def repair(ys, data, weights, orders=ORDERS):
    """The yardstick's repair of a batch -> ({(lambda, rule): [eX, eZ, flags, repaired, swept]}, sector records).
    `weights`: {rule: (wX, wZ) or None}.  A record: b, sec, what ("skipped", "bad", "inconsistent" or "ok"), and
    for "ok" the pivots, the column order, T, whether the elimination changed the syndrome column, and per
    (lambda, rule) the winner's (index, f, candidates tied at the least score)."""
    sX, sZ, soft, eX, eZ, flags = data
    out = {(lam, rule): [eX.copy(), eZ.copy(), flags.copy(), 0, 0] for lam in orders for rule in weights}
    records = []
    for b in range(len(flags)):
        for sec, s in enumerate((sX, sZ)):
            what, red = ys.outcome(sec, s[b], soft[b], flags[b] & FAIL[sec])
            rec = {"b": b, "sec": sec, "what": what}
            records.append(rec)
            if what != "ok":
                continue
            A, piv, order = red
            pcol = [int(v) for _, v in piv]
            rec.update(piv=piv, order=order, T=[int(v) for v in order if int(v) not in set(pcol)], win={},
                       s_changed=bool((A[:, ys.n] != (np.asarray(s[b]) & 1)).any()))
            for (lam, rule), o in out.items():
                w = None if weights[rule] is None else np.asarray(weights[rule][sec], dtype=np.int64)
                e, index, f, ties = ys.sweep_scored(red, lam, w)[:4]
                o[sec][b] = e
                o[2][b] &= ~FAIL[sec] & 0xFF
                o[3] += 1
                o[4] += index > 0
                rec["win"][lam, rule] = (index, f, ties)
    return out, records


def want(name, method):
    """repair() of batch(name, method) under the three rules, once per session."""
    if (name, method) not in _want:
        weights = {"h": None, "random": weights_of(name, "random"), "two": weights_of(name, "two")}
        _want[name, method] = repair(yardstick(name, method), batch(name, method), weights)
    return _want[name, method]


def apply_rule(dec, name, rule):
    """Priors and QEC_OPT_OSD_SCORE of a rule on a handle (the order is set by the caller, before or after)."""
    dec.set_option("osd_score", 0)
    if rule == "h":
        dec.set_priors(None, None)
    else:
        dec.set_priors(*priors_of(OSD_SHAPES[name][0], rule))


# ---- 1. the table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OSD_SHAPES))
def test_pinned_shapes(name):
    n, mX, mZ, rX, rZ = OSD_SHAPES[name]
    HX, HZ = matrices(name)
    assert HX.shape == (mX, n) and HZ.shape == (mZ, n)
    assert (gf2_rank(HX), gf2_rank(HZ)) == (rX, rZ)
    for H in (HX, HZ):
        assert set(np.unique(H)) <= {0, 1}
        assert H.sum(axis=1).max() <= MAX_ROW and H.sum(axis=1).min() >= 1 and H.sum(axis=0).max() <= MAX_COL
    code = code_of(name)
    assert (code.n, code.numEqsX, code.numEqsZ) == (n, mX, mZ)
    ys = yardstick(name, 0)
    assert ys.rank == [rX, rZ] and ys.L == code.stride and ys.qn == (mX + mZ) * code.stride


def test_what_the_shapes_are_there_for():
    S = OSD_SHAPES
    words = lambda name: (S[name][0] + 1 + 31) // 32  # noqa: E731
    assert S["w31"][0] % 32 == 31 and words("w31") == 1 and S["w31"][3] == 1 and S["w31"][4] == S["w31"][0]
    assert S["w32"][0] % 32 == 0 and words("w32") == 2 and S["w32"][2] > S["w32"][0]
    assert S["w63"][0] % 32 == 31 and words("w63") == 2 and S["w63"][3] == S["w63"][1] and S["w63"][4] < S["w63"][2]
    assert S["w64"][0] % 32 == 0 and words("w64") == 3 and S["w64"][1:4] == (64, 65, 64)
    assert S["c128"][1:3] == (128, 129)
    assert S["n2048"][0] == 2048 and words("n2048") == 65 == words("n2048") | 1 and S["n2048"][1] != S["n2048"][2]
    assert S["m2048"][2] == 2048 and S["m2048"][4] <= S["m2048"][0] and (2048 + 63) // 64 == 32
    for name in S:  # every sector kind occurs: full rank, deficient, rank 1
        assert S[name][3] <= S[name][1] and S[name][4] <= S[name][2]
    HX, HZ = matrices("c128")
    noX, noZ = np.nonzero(~HX.any(axis=0))[0], np.nonzero(~HZ.any(axis=0))[0]
    assert len(noX) >= 8 and len(noZ) >= 8 and not set(noX) & set(noZ)
    assert np.unique(np.nonzero(HX)[1] // 64).size >= 3  # rows across the 64-bit word pairs
    HX, HZ = matrices("n2048")
    assert HZ.any(axis=0).sum() <= 1280 and HX.any(axis=0).sum() < 2048
    HX, HZ = matrices("m2048")
    assert set(HZ.sum(axis=1)) == {1, 2}


def test_lds_footprints():
    n, mX, mZ = OSD_SHAPES["n2048"][:3]
    assert lds_words(max(mX, mZ), n, 64, False) == 16103
    assert lds_words(max(mX, mZ), n, 64, True) == 16283
    assert LDS_LIMIT == 16384
    assert lds_words(193, 2048, 64, False) <= LDS_LIMIT < lds_words(193, 2048, 64, True)  # one more row: not the weighted sweep
    assert all(fits("n2048", lam, weighted) for lam in ORDERS for weighted in (False, True))
    assert all(fits("m2048", lam, False) for lam in (0, 1, 2, 10)) and not fits("m2048", 64, False)
    assert not any(fits("m2048", lam, True) for lam in (1, 2, 10, 64))
    for name in ("w31", "w32", "w63", "w64", "c128"):
        assert all(fits(name, lam, weighted) for lam in ORDERS for weighted in (False, True))


# ---- 2. conditions that keep the table from being vacuous (the yardstick alone) ---------------------------------------
def _ok(name, method):
    return [r for r in want(name, method)[1] if r["what"] == "ok"]


def cond_lambda(name):
    return 64 if fits(name, 64, False) else 10


@pytest.mark.parametrize("name", sorted(OSD_SHAPES))
@pytest.mark.parametrize("method", METHODS)
def test_batch_roles(name, method):
    n, mX, mZ, rX, rZ = OSD_SHAPES[name]
    sX, sZ, soft, eX, eZ, flags = batch(name, method)
    B = len(flags)
    assert B == SMALL_B.get(name, B_DEFAULT)
    recs = {(r["b"], r["sec"]): r["what"] for r in want(name, method)[1]}
    for sec, (m, rank) in enumerate(((mX, rX), (mZ, rZ))):
        kinds = [recs[b, sec] for b in range(B)]
        if rank < m:   # sample 1 of a deficient sector is inconsistent, and no other
            assert kinds[1] == "inconsistent" and kinds.count("inconsistent") == 1
        else:
            assert "inconsistent" not in kinds
    assert recs[2, 0] == "bad" and recs[3, 1] == "bad" and list(recs.values()).count("bad") == 2
    assert sX[2].max() == 2 and sZ[3].max() == 255
    assert recs[0, 0] != "skipped" and recs[0, 1] == "skipped"
    if B == B_DEFAULT:
        assert recs[5, 0] == "skipped" and recs[5, 1] == "ok"
        assert recs[B - 1, 0] == recs[B - 1, 1] == "skipped"
    assert list(recs.values()).count("ok") >= (12 if B == B_DEFAULT else 4)
    # the yardstick leaves what it does not repair exactly as it was
    for (lam, rule), (wX, wZ, wf, cnt, swept) in want(name, method)[0].items():
        assert cnt == list(recs.values()).count("ok")
        for (b, sec), what in recs.items():
            if what != "ok":
                assert np.array_equal((wX, wZ)[sec][b], (eX, eZ)[sec][b])
                assert (wf[b] & FAIL[sec]) == (flags[b] & FAIL[sec])
        assert np.array_equal(wf & 12, flags & 12)
    if method:  # the LLR input: ties between columns in no check and real +0.0 values
        bits = soft.view(np.uint32)
        assert (bits == 0).any() and (bits == 0x80000000).any() and (soft < 0).any() and (soft > 0).any()
        assert np.abs(soft).max() == F32(2.0 ** 30)


@pytest.mark.parametrize("method", METHODS)
def test_winners_over_the_table(method):
    """Under each key and each score: a sector won by a single flip, one won by a pair, one with candidates tied at
    the least score; under random priors a sector whose weighted winner is not the Hamming winner."""
    seen = {rule: {"single": 0, "pair": 0, "osd0": 0, "tied": 0, "differs": 0} for rule in RULES}
    for name in OSD_SHAPES:
        lam = cond_lambda(name)
        for r in _ok(name, method):
            for rule in RULES:
                index, f, ties = r["win"][lam, rule]
                seen[rule][kind_of(index, f)] += 1
                seen[rule]["tied"] += ties > 1
                seen[rule]["differs"] += index != r["win"][lam, "h"][0]
    print(method, seen)
    for rule in ("h", "random"):
        assert seen[rule]["single"] >= 1 and seen[rule]["pair"] >= 1, (rule, seen[rule])
    assert seen["h"]["tied"] >= 1 and seen["two"]["tied"] >= 1
    assert seen["random"]["differs"] >= 1 and seen["two"]["differs"] >= 1


@pytest.mark.parametrize("method", METHODS)
def test_conditions_of_the_small_shapes(method):
    for r in _ok("w31", method):
        if r["sec"] == 1:  # f = 0: the OSD-0 estimate whatever lambda is
            assert len(r["T"]) == 0 and all(win == (0, 0, 1) for win in r["win"].values())
    assert sum(r["sec"] == 1 for r in _ok("w31", method)) >= 6
    full = [r for r in _ok("w64", method) if r["sec"] == 0]
    assert len(full) >= 6 and all(len(r["piv"]) == 64 for r in full)
    assert all(sorted(p for p, _ in r["piv"]) == list(range(64)) for r in full)  # every row a pivot row
    for name in ("w32", "w63", "w64", "c128"):  # rows without a pivot lie among the pivot rows, not all behind them
        Z = [r for r in _ok(name, method) if r["sec"] == 1]
        m, rank = OSD_SHAPES[name][2], OSD_SHAPES[name][4]
        assert Z and all(len(r["piv"]) == rank < m for r in Z)
        assert any(max(p for p, _ in r["piv"]) > rank for r in Z), name
    # the chunk of one row (w64 Z: row 64; c128 Z: row 128) holds a pivot row
    for name, last in (("w64", 64), ("c128", 128)):
        has = [any(p == last for p, _ in r["piv"]) for r in _ok(name, method) if r["sec"] == 1]
        assert all(has), name


@pytest.mark.parametrize("method", METHODS)
def test_conditions_of_the_large_shapes(method):
    recs = _ok("n2048", method)
    X = [r for r in recs if r["sec"] == 0]
    assert X and all(len(r["piv"]) == 180 for r in X)
    assert any(v >= 2016 for r in recs for _, v in r["piv"])            # a pivot column in the last word of qubits
    assert any(v >= 2016 for r in recs for v in r["T"][:64])            # one of the first lambda non-pivot columns there
    assert any(r["s_changed"] for r in X)                               # word 64: the syndrome column is rewritten
    for name in ("c128", "n2048"):
        H = matrices(name)
        hit_walk = hit_T = 0
        for r in _ok(name, method):
            absent = ~H[r["sec"]].any(axis=0)
            last = int(np.nonzero(r["order"] == r["piv"][-1][1])[0][0])  # where the walk found its last pivot
            hit_walk += bool(absent[r["order"][:last]].any())
            hit_T += bool(absent[r["T"][:cond_lambda(name)]].any())
        assert hit_walk >= 1 and hit_T >= 1, name
    Z = [r for r in _ok("m2048", method) if r["sec"] == 1]
    assert Z and all(len(r["piv"]) == 150 for r in Z)
    assert any(p >= 1984 for r in Z for p, _ in r["piv"])               # bit 31 of the used-row mask
    assert any(p < 64 for r in Z for p, _ in r["piv"])
    if method:  # a column in no check ties with a real +0.0 and the index decides
        ys = yardstick("c128", 1)
        soft = batch("c128", 1)[2]
        ties = 0
        for sec in (0, 1):
            absent = ys.pos[sec] == ys.qn
            vals = np.append(soft, np.zeros((len(soft), 1), dtype=F32), axis=1)[:, ys.pos[sec]].view(np.uint32)
            ties += int(((vals == 0) & ~absent).any(axis=1).sum())
        assert ties >= 6


# ---- 3. the host implementation = the yardstick ------------------------------------------------------------------------
_cpu = {}


def cpu_decoder(name):
    if name not in _cpu:
        _cpu[name] = q.DecoderCPU(code_of(name))
    return _cpu[name]


def run_host(dec, name, method, rule, lam, data):
    """dec.osd under (method, rule, lambda) -> (eX, eZ, flags, osd_sectors, osd_cs_sectors); the options reset."""
    dec.set_option("osd_order", 0)
    apply_rule(dec, name, rule)
    dec.set_option("bp_method", method)
    try:
        dec.set_option("osd_order", lam)
        dec.set_option("osd_score", int(rule != "h"))
        got = dec.osd(*data)
        return got + (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors"))
    finally:
        dec.set_option("osd_score", 0)
        dec.set_option("osd_order", 0)
        dec.set_option("bp_method", 0)
        dec.set_priors(None, None)


def assert_same(got, expect, what):
    for a, b, field in zip(got, expect, ("eX", "eZ", "flags", "osd_sectors", "osd_cs_sectors")):
        assert np.array_equal(a, b), "%s: %s differs" % (what, field)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("lam", ORDERS)
@pytest.mark.parametrize("name", sorted(OSD_SHAPES))
def test_host_implementation_matches_the_yardstick(name, lam, method, rule):
    """DecoderCPU.osd on the batch of a shape, bit for bit: estimates, flags and both counters.  method 1 with a
    rule other than "h" is osd_host_sector with the LLR key and a weight table together."""
    got = run_host(cpu_decoder(name), name, method, rule, lam, batch(name, method))
    assert_same(got, want(name, method)[0][lam, rule], (name, lam, method, rule))


# ---- 4. the inputs of the GPU module's other cases, checked here ------------------------------------------------------------
SYNC = (0.2, 4, 32, 0x51EC0DE)       # c128 behind decode_batch: p, iteration cap (syndrome stop), samples, seed
W31_MC = (0.1, 4, 2048, 0x51EC0DE)   # w31 in qec_monte_carlo: the same


def sync_syndromes():
    from oracle.philox import depolarizing
    p, _, B, seed = SYNC
    HX, HZ = matrices("c128")
    x, z = depolarizing(seed, 0, B, HX.shape[1], p)
    return ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", METHODS)
def test_sync_case_leaves_failed_sectors(method, rule):
    """BP alone, under each method and each set of priors, leaves at least 10 failed sectors of c128 for the OSD
    stage behind decode_batch, and the stage repairs them all."""
    p, N = SYNC[:2]
    sX, sZ = sync_syndromes()
    dec = q.DecoderCPU(code_of("c128"))
    apply_rule(dec, "c128", rule)
    dec.set_option("bp_method", method)
    bp = dec.decode_batch(sX, sZ, p, N, "syndrome")[2]
    failed = int(((bp & 1) != 0).sum() + ((bp & 2) != 0).sum())
    assert failed >= 10, failed
    dec.set_option("osd_order", 10)
    dec.set_option("osd_score", int(rule != "h"))
    dec.set_option("osd", 1)
    after = dec.decode_batch(sX, sZ, p, N, "syndrome")[2]
    assert not (after & 3).any() and dec.get_option("osd_sectors") == failed
    assert dec.last_path() == ({"osd", "minsum"} if method else {"osd"})


# ---- 5. beyond the kernel's sizes: the host implementation has no limit ------------------------------------------------------
OVERSIZE = {"n2049": (2049, 8, 8), "mZ2049": (160, 3, 2049)}  # name -> (n, mX, mZ)
_over = {}


def oversize_code(name):
    if name not in _over:
        rng = np.random.default_rng(2049)
        if name == "n2049":
            HX, HZ = systematic(rng, 8, 2049, 10, 20), systematic(rng, 8, 2049, 10, 20)
        else:
            HX = systematic(rng, 3, 160, 14, 24)
            HZ = np.zeros((2049, 160), dtype=np.uint8)
            HZ[np.arange(2049), np.arange(2049) % 150] = 1
        assert (HX.shape[1], HX.shape[0], HZ.shape[0]) == OVERSIZE[name]
        assert max(H.sum(axis=a).max() for H in (HX, HZ) for a in (0, 1)) <= MAX_ROW and HZ.sum(axis=0).max() <= MAX_COL
        _over[name] = (q.Quantum_LDPC_Code.createFromMatrices(HX, HZ), HX, HZ)
    return _over[name][0]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(OVERSIZE))
def test_host_implementation_repairs_oversize_codes(name, method):
    """The codes that the kernel refuses (tests/test_gpu_osd_shapes.py): DecoderCPU repairs them as the yardstick
    does, on 2 samples."""
    code = oversize_code(name)
    HX, HZ = _over[name][1:]
    ys = ShapeYardstick(HX, HZ, method)
    rng = np.random.default_rng(11)
    B = 2
    x, z = depolarizing_errors(code.n, 99, B, 0.02)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    soft = np.ascontiguousarray((random_llr if method else random_soft)(rng, B, ys.qn), dtype=F32)
    data = (sX, sZ, soft, rng.integers(0, 2, (B, code.n), dtype=np.uint8), rng.integers(0, 2, (B, code.n), dtype=np.uint8),
            np.full(B, 3, dtype=np.uint8))
    expect = repair(ys, data, {"h": None}, (0, 10))[0]
    dec = q.DecoderCPU(code)
    dec.set_option("bp_method", method)
    for lam in (0, 10):
        dec.set_option("osd_order", lam)
        got = dec.osd(*data) + (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors"))
        assert expect[lam, "h"][3] == 2 * B
        assert_same(got, expect[lam, "h"], (name, method, lam))

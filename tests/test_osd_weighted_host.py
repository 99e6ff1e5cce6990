"""The prior-weighted score of the combination sweep (QEC_OPT_OSD_SCORE = 1) without
a GPU: the weight table, the host implementation (osd_host.cpp) through qec_osd and the CPU engine's synchronous
calls, the option, the CLI and the C++ wrapper, against the numpy yardstick of tests/test_osd_cs_host.py with
the candidates' Hamming weights replaced by their scores under the table read from dec.osd_weights().
tests/test_gpu_osd_weighted.py reuses the yardstick and the batches for the kernel."""
import os
import subprocess

import numpy as np
import pytest

import qec_ldpc_amd as q
from conftest import ROOT
from qec_ldpc_amd.gather import pack_records
from qec_ldpc_amd.synthetic import depolarizing_errors
from test_general_code import GeneralOsdYardstick
from test_osd_host import FAIL, _cli, _fields, random_soft
from test_priors import F32, _write_priors, code_of, independent, matrices, prior_vectors

CODES = ("hgp_ham", "surf3", "ham_rep3+1", "G13")
ORDERS = (0, 1, 2, 10, 64)
FORCED_B = 32
FORCED_SMALL = {"P61": 8}  # the GPU tests' largest code: fewer samples, as tests/test_osd_cs_host.py takes
SAMPLED = (0.08, 20, 256)  # the batch of test_cpu_osd_with_priors: p (not used by BP), the cap, the batch


# ---- priors ------------------------------------------------------------------------------------------------
def priors_of(n, kind):
    """(priorX, priorZ): "random" as prior_vectors draws them; "two": 0.1 where the random prior is above its
    sector's median and 0.01 elsewhere (many equal weights: ties between candidates); "uniform": one value in
    (0, 1/2); "half": every weight is zero."""
    rand = prior_vectors(n, "random")
    if kind == "random":
        return rand
    if kind == "two":
        return tuple(np.where(pr > np.median(pr), F32(0.1), F32(0.01)).astype(F32) for pr in rand)
    value = {"uniform": F32(0.03), "half": F32(0.5)}[kind]
    return np.full(n, value, dtype=F32), np.full(n, value, dtype=F32)


# ---- the yardstick: section 1.4 in numpy -----------------------------------------------------------------
class WeightedYardstick(GeneralOsdYardstick):
    """The sweep of test_osd_cs_host.YardstickCS with each candidate scored by the sum of w over its flips
    (w = None: their number, the parent's rule); the first minimum wins.  key_fn: the soft value's sort key
    (osd_keys, the product rule's, unless given: osd_key_llr of test_minsum.py for min-sum); absent: the soft value
    that a column in no check of the sector stands for (0.5f, or +0.0f under min-sum)."""

    def __init__(self, HX, HZ, key_fn=None, absent=None):
        super().__init__(HX, HZ)
        if key_fn is not None:
            self.key_fn = key_fn
        if absent is not None:
            self.absent = F32(absent)

    def sweep_literal(self, red, lam, w=None):
        """YardstickCS.sweep word for word but for the weights -> (estimate, index, f, candidates at the minimum)."""
        A, piv, order = red
        n = self.n
        prow = np.array([p for p, _ in piv], dtype=np.int64)
        pcol = np.array([v for _, v in piv], dtype=np.int64)
        pivots = set(pcol.tolist())
        T = [int(v) for v in order if int(v) not in pivots]
        f = len(T)
        top = min(lam, f)
        flips = [()]
        if lam > 0:
            flips += [(t,) for t in T]
            flips += [(T[i], T[j]) for i in range(top) for j in range(i + 1, top)]

        def estimate(F):
            e = np.zeros(n, dtype=np.uint8)
            x = A[prow, n].copy()
            for t in F:
                x ^= A[prow, t]
            e[pcol] = x
            e[list(F)] = 1
            return e

        if w is None:
            weights = [int(estimate(F).sum()) for F in flips]
        else:
            weights = [int((estimate(F) * w).sum()) for F in flips]
        index = int(np.argmin(weights))  # the first minimum
        return estimate(flips[index]), index, f, weights.count(min(weights))

    def sweep_scored(self, red, lam, w=None):
        """The same, every candidate at once -> (estimate, index, f, candidates at the minimum, its score)."""
        A, piv, order = red
        n = self.n
        prow = np.array([p for p, _ in piv], dtype=np.int64)
        pcol = np.array([v for _, v in piv], dtype=np.int64)
        pivots = set(pcol.tolist())
        T = np.array([int(v) for v in order if int(v) not in pivots], dtype=np.int64)
        f = len(T)
        cost = np.ones(n, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
        x0 = A[prow, n].astype(np.uint8)
        X, flips = x0[None], [()]
        if lam > 0:
            C = A[np.ix_(prow, T)].T.astype(np.uint8)  # [f, rank]
            ii, jj = np.triu_indices(min(lam, f), 1)   # pairs by i, then j
            X = np.concatenate([x0[None], x0[None] ^ C, x0[None] ^ C[ii] ^ C[jj]])
            flips += [(t,) for t in T] + [(T[i], T[j]) for i, j in zip(ii, jj)]
        score = X.astype(np.int64) @ cost[pcol] + np.array([sum(int(cost[t]) for t in F) for F in flips], dtype=np.int64)
        index = int(np.argmin(score))  # the first minimum
        e = np.zeros(n, dtype=np.uint8)
        e[pcol] = X[index]
        e[list(flips[index])] = 1
        return e, index, f, int((score == score[index]).sum()), int(score[index])

    def repair_w(self, sX, sZ, qf, eX, eZ, flags, lams, W):
        """Steps 2-7 with the sweep under both rules for each lambda of `lams` (the elimination is shared);
        W = (wX, wZ) -> {lambda: {"w": (eX, eZ, flags, repaired, swept), "h": the same under Hamming weight,
        "sectors": [(weighted index, Hamming index, f, candidates tied at the least score, the weighted winner's
        score, the Hamming winner's score, the two winners' Hamming weights)]}}."""
        out = {lam: {"w": [eX.copy(), eZ.copy(), flags.copy(), 0, 0], "h": [eX.copy(), eZ.copy(), flags.copy(), 0, 0],
                     "sectors": []} for lam in lams}
        for b in range(len(flags)):
            for sec, s in enumerate((sX, sZ)):
                if not flags[b] & FAIL[sec]:
                    continue
                red = self.reduce(sec, s[b], qf[b])
                if red is None:
                    continue
                w = np.asarray(W[sec], dtype=np.int64)
                for lam, o in out.items():
                    ew, iw, f, ties, score = self.sweep_scored(red, lam, w)
                    eh, ih = self.sweep_scored(red, lam)[:2]
                    for key, e, idx in (("w", ew, iw), ("h", eh, ih)):
                        o[key][sec][b] = e
                        o[key][2][b] &= ~FAIL[sec] & 0xFF
                        o[key][3] += 1
                        o[key][4] += idx > 0
                    o["sectors"].append((iw, ih, f, ties, score, int((eh * w).sum()), int(ew.sum()), int(eh.sum())))
        return out


_ys = {}


def yardstick(name):
    if name not in _ys:
        _ys[name] = WeightedYardstick(*matrices(name))
    return _ys[name]


def kind_of(index, f):
    return "osd0" if index == 0 else "single" if index <= f else "pair"


# ---- the batches -------------------------------------------------------------------------------------------
_batches = {}


def forced(name):
    """forced_batch of test_osd_host.py for any test code: every sector marked failed, sampled (consistent)
    syndromes, junk estimates, random convergence bits, random soft input."""
    B = FORCED_SMALL.get(name, FORCED_B)
    if (name, B) not in _batches:
        HX, HZ = matrices(name)
        code = code_of(name)
        rng = np.random.default_rng(2024)
        x, z = depolarizing_errors(code.n, 31337, B, 0.08)
        sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        eX = rng.integers(0, 2, (B, code.n), dtype=np.uint8)
        eZ = rng.integers(0, 2, (B, code.n), dtype=np.uint8)
        flags = (3 | (rng.integers(0, 4, B) << 2)).astype(np.uint8)
        qf = random_soft(rng, B, (HX.shape[0] + HZ.shape[0]) * code.stride)
        _batches[name, B] = (sX, sZ, qf, eX, eZ, flags)
    return _batches[name, B]


def sampled(name, kind):
    """The batch of test_cpu_osd_with_priors (errors drawn from twice the random priors), decoded by the CPU engine
    under priors_of(n, kind): syndrome stop at the cap for the estimates and flags, the fixed-stop osd_iterations
    decode for the soft input -> (sX, sZ, soft, eX, eZ, flags, iters)."""
    if (name, kind, "sampled") not in _batches:
        p, N, B = SAMPLED
        HX, HZ = matrices(name)
        code = code_of(name)
        pX, pZ = prior_vectors(code.n, "random")
        x, z = independent(777, 0, B, np.minimum(pX * F32(2), F32(1)), np.minimum(pZ * F32(2), F32(1)))
        sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        dec = q.DecoderCPU(code)
        dec.set_priors(*priors_of(code.n, kind))
        main = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
        soft = dec.decode_batch(sX, sZ, p, dec.get_option("osd_iterations"), "fixed", want_q=True)[4]
        _batches[name, kind, "sampled"] = (sX, sZ, soft, main[0], main[1], main[2], main[3])
    return _batches[name, kind, "sampled"]


def weights_of(name, kind):
    dec = q.DecoderCPU(code_of(name))
    dec.set_priors(*priors_of(code_of(name).n, kind))
    return dec.osd_weights()


_want = {}


def want(name, kind, batch):
    """The yardstick's repair, under both rules and for every order, of forced(name) or sampled(name, kind) with
    the weights of priors_of(n, kind)."""
    if (name, kind, batch) not in _want:
        data = forced(name) if batch == "forced" else sampled(name, kind)[:6]
        _want[name, kind, batch] = yardstick(name).repair_w(*data, ORDERS, weights_of(name, kind))
    return _want[name, kind, batch]


class osd_options:
    """`with osd_options(dec, lam, score, osd=1)`: the options for the block, reset behind it."""

    def __init__(self, dec, lam, score, osd=None):
        self.dec, self.lam, self.score, self.osd = dec, lam, score, osd

    def __enter__(self):
        self.dec.set_option("osd_order", self.lam)
        self.dec.set_option("osd_score", self.score)
        if self.osd is not None:
            self.dec.set_option("osd", self.osd)
        return self.dec

    def __exit__(self, *exc):
        self.dec.set_option("osd_order", 0)
        self.dec.set_option("osd_score", 0)
        if self.osd is not None:
            self.dec.set_option("osd", 0)


def assert_repair(dec, data, lam, score, expect, what, counters=True):
    """dec.osd on the batch under (lam, score) equals `expect` = (eX, eZ, flags, repaired, swept)."""
    with osd_options(dec, lam, score):
        gX, gZ, gf = dec.osd(*data)
        assert np.array_equal(gX, expect[0]) and np.array_equal(gZ, expect[1]) and np.array_equal(gf, expect[2]), what
        if counters:
            assert dec.get_option("osd_sectors") == expect[3] and dec.get_option("osd_cs_sectors") == expect[4], what


def lds_words(mmax, n, order, weighted):
    """osd_lds_words of osd.hip: the elimination's image, the sweep's column vectors, the weighted sweep's arrays."""
    W = (n + 1 + 31) // 32
    rws = (2 * ((mmax + 63) // 64)) | 1
    words = mmax * (W | 1) + n + (n + 1) // 2 + (mmax + 1) // 2
    if order > 0:
        words += (order + 1) * rws
        if weighted:
            words += 12 * rws + (mmax + 1) // 2
    return words


LDS_LIMIT = 64 * 1024 // 4  # words of one workgroup's LDS allocation (kOsdMaxLds)


# ---- 1. the weight table ---------------------------------------------------------------------------------------
def test_weight_table():
    code = code_of("hgp_ham")
    n = code.n
    dec = q.DecoderCPU(code)
    assert dec.osd_weights() is None
    pri = prior_vectors(n, "special")
    dec.set_priors(*pri)
    tabs = dec.osd_weights()
    assert all(t.dtype == np.int32 and t.shape == (n,) for t in tabs)
    for pr, w in zip(pri, tabs):
        assert (w[pr == 0] == 4095).all() and (pr == 0).sum() == 1
        assert (w[pr == F32(0.5)] == 0).all() and (w[pr == 1] == 0).all() and (pr >= F32(0.5)).sum() == 2
        d = pr.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = np.clip(np.rint(16.0 * np.log2((1.0 - d) / d)), 0, 4095)
        ref[d >= 0.5] = 0
        ref[d == 0] = 4095
        assert (np.abs(w - ref) <= 1).all() and (w >= 0).all() and (w <= 4095).all()
        low = np.nonzero(pr < F32(0.5))[0]
        low = low[np.argsort(pr[low], kind="stable")]
        assert (np.diff(w[low]) <= 0).all()  # a smaller prior never weighs less
    # the extremes of the formula: the smallest positive float stays below the cap, which only 0 reaches
    dec.set_priors(np.full(n, np.float32(1e-45)), np.full(n, np.nextafter(F32(0.5), F32(0))))
    wX, wZ = dec.osd_weights()
    assert (wX == 2384).all() and (wZ == 0).all()
    dec.set_priors(None, None)
    assert dec.osd_weights() is None


# ---- 2. qec_osd on the CPU engine = the yardstick --------------------------------------------------------------
CASES = [(name, "random", batch) for name in CODES for batch in ("forced", "sampled")] + \
        [(name, "two", "sampled") for name in ("hgp_ham", "G13")]


@pytest.mark.parametrize("name,kind,batch", CASES)
def test_qec_osd_matches_the_weighted_yardstick(name, kind, batch):
    code = code_of(name)
    data = forced(name) if batch == "forced" else sampled(name, kind)[:6]
    exp = want(name, kind, batch)
    dec = q.DecoderCPU(code)
    dec.set_priors(*priors_of(code.n, kind))
    failed = int(np.sum((data[5] & 1) != 0) + np.sum((data[5] & 2) != 0))
    assert failed >= (2 * FORCED_B if batch == "forced" else 10)  # sectors for the sweep to repair
    for lam in ORDERS:
        assert exp[lam]["w"][3] == failed  # every sampled syndrome is consistent
        assert_repair(dec, data, lam, 1, exp[lam]["w"], (name, kind, batch, lam, "weighted"))
        assert_repair(dec, data, lam, 0, exp[lam]["h"], (name, kind, batch, lam, "hamming"))


def test_the_fast_yardstick_is_the_literal_one():
    """sweep_scored (every candidate at once) against YardstickCS.sweep with `weights` replaced, and the latter
    without a table against YardstickCS.sweep itself."""
    ys = yardstick("hgp_ham")
    sX, sZ, qf = forced("hgp_ham")[:3]
    W = weights_of("hgp_ham", "two")
    for b in range(6):
        for sec, s in enumerate((sX, sZ)):
            red = ys.reduce(sec, s[b], qf[b])
            for lam in (0, 1, 10):
                for w in (None, np.asarray(W[sec], dtype=np.int64)):
                    a, b_ = ys.sweep_literal(red, lam, w), ys.sweep_scored(red, lam, w)
                    assert np.array_equal(a[0], b_[0]) and a[1:] == b_[1:4]
                a, c = ys.sweep_literal(red, lam), ys.sweep(red, lam)
                assert np.array_equal(a[0], c[0]) and a[1:] == c[1:]


# ---- 3. conditions on the inputs (the yardstick alone) ---------------------------------------------------------
@pytest.mark.parametrize("name", ["hgp_ham", "G13"])
def test_conditions_on_the_inputs(name):
    sec = want(name, "random", "sampled")[10]["sectors"]
    differ = [s for s in sec if s[0] != s[1]]
    kinds = {k: sum(kind_of(s[0], s[2]) == k for s in differ) for k in ("osd0", "single", "pair")}
    print(name, "sectors", len(sec), "weighted winner differs", len(differ), kinds)
    assert kinds["single"] >= 1 and kinds["pair"] >= 1, kinds
    if name == "hgp_ham":
        assert kinds["osd0"] >= 1, kinds
    assert sum(s[6] > s[7] for s in differ) >= 1  # a heavier candidate that is likelier
    tied = sum(s[3] > 1 for s in want(name, "two", "sampled")[10]["sectors"])
    print(name, "two-level priors: sectors with candidates tied at the least score", tied)
    assert tied >= 1
    # and on the forced batches, which the kernel is held to as well
    forced_differ = [s for s in want(name, "random", "forced")[10]["sectors"] if s[0] != s[1]]
    assert len(forced_differ) >= 1


# ---- 4. invariants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CODES)
def test_rules_coincide_under_uniform_or_no_priors_and_at_order_zero(name):
    code = code_of(name)
    data = forced(name)
    dec = q.DecoderCPU(code)
    for pri in (None, "uniform", "random"):
        if pri:
            dec.set_priors(*priors_of(code.n, pri))
        for lam in ORDERS if pri != "random" else (0,):
            out = []
            for score in (0, 1):
                with osd_options(dec, lam, score):
                    out.append(dec.osd(*data) + (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors")))
            assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1])), (name, pri, lam)
    # the yardstick says the same of uniform weights: score = w |e|, ties included
    hw = want(name, "random", "forced")
    uni = yardstick(name).repair_w(*data, (10,), weights_of(name, "uniform"))[10]
    assert all(np.array_equal(a, b) for a, b in zip(uni["w"], hw[10]["h"]))


@pytest.mark.parametrize("name", CODES)
def test_all_weights_zero_take_the_osd0_estimate(name):
    code = code_of(name)
    data = forced(name)
    dec = q.DecoderCPU(code)
    dec.set_priors(*priors_of(code.n, "half"))
    assert not any(w.any() for w in dec.osd_weights())
    with osd_options(dec, 0, 0):
        zero = dec.osd(*data)
    for lam in (1, 10, 64):
        with osd_options(dec, lam, 1):
            got = dec.osd(*data)
            assert dec.get_option("osd_cs_sectors") == 0 and dec.get_option("osd_sectors") == 2 * FORCED_B
        assert all(np.array_equal(a, b) for a, b in zip(got, zero)), (name, lam)


@pytest.mark.parametrize("name", CODES)
def test_weighted_sweep_properties(name):
    """H e = s for every repaired sector; the weighted winner scores no more than the Hamming winner, and its score
    does not grow with lambda."""
    code = code_of(name)
    HX, HZ = matrices(name)
    sX, sZ, soft, eX, eZ, flags = sampled(name, "random")[:6]
    dec = q.DecoderCPU(code)
    dec.set_priors(*priors_of(code.n, "random"))
    W = [np.asarray(w, dtype=np.int64) for w in dec.osd_weights()]
    fail = [(flags & 1) != 0, (flags & 2) != 0]
    score = {}
    for lam in (0, 1, 10, 64):
        got = {}
        for rule in (0, 1):
            with osd_options(dec, lam, rule):
                got[rule] = dec.osd(sX, sZ, soft, eX, eZ, flags)
            assert not (got[rule][2] & 3).any()
            assert np.array_equal((got[rule][0] @ HX.T) & 1, sX) and np.array_equal((got[rule][1] @ HZ.T) & 1, sZ)
        sc = {rule: np.concatenate([(got[rule][s][fail[s]].astype(np.int64) * W[s]).sum(1) for s in (0, 1)]) for rule in (0, 1)}
        assert (sc[1] <= sc[0]).all(), lam
        score[lam] = sc[1]
    assert (score[64] <= score[10]).all() and (score[10] <= score[1]).all() and (score[1] <= score[0]).all()


# ---- 5. the synchronous calls of DecoderCPU ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hgp_ham", "G13"])
def test_decoder_cpu_synchronous_calls(name):
    p, N, _ = SAMPLED
    code = code_of(name)
    sX, sZ, soft, eX, eZ, flags, iters = sampled(name, "random")
    exp = want(name, "random", "sampled")[10]
    dec = q.DecoderCPU(code)
    dec.set_priors(*priors_of(code.n, "random"))
    assert exp["w"][4] != exp["h"][4] or not np.array_equal(exp["w"][0], exp["h"][0])
    for score, key in ((1, "w"), (0, "h")):  # afterwards the rule back at 0: today's outputs
        with osd_options(dec, 10, score):
            fed = dec.osd(sX, sZ, soft, eX, eZ, flags)
        with osd_options(dec, 10, score, osd=1):
            g = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
            for a, b, c in zip(g[:3], fed, exp[key][:3]):
                assert np.array_equal(a, b) and np.array_equal(a, c), (name, score)
            assert np.array_equal(g[3], iters)
            assert dec.get_option("osd_sectors") == exp[key][3] and dec.get_option("osd_cs_sectors") == exp[key][4]
            rec, its = dec.decode_batch_packed(sX, sZ, p, N, "syndrome", want_iters=True)
            assert np.array_equal(rec, pack_records(*fed)) and np.array_equal(its, iters)
            assert dec.get_option("osd_sectors") == exp[key][3] and dec.get_option("osd_cs_sectors") == exp[key][4]


# ---- 6. the option ---------------------------------------------------------------------------------------------------
def test_option_checks():
    dec = q.DecoderCPU(code_of("surf3"))
    assert dec.get_option("osd_score") == 0
    assert q.OPTION["osd_score"] == 16 and q.OPTIONS["osd_score"] == 16
    dec.set_option("osd_score", 1)
    for value in (-1, 2):
        with pytest.raises(q.QecError, match="QEC_OPT_OSD_SCORE"):
            dec.set_option("osd_score", value)
        assert dec.get_option("osd_score") == 1
    assert dec.get_option("osd") == 0 and dec.get_option("osd_order") == 0  # the option alone turns nothing on
    sX, sZ = np.zeros((3, 6), dtype=np.uint8), np.zeros((3, 6), dtype=np.uint8)
    sX[:, 0] = 1
    dec.decode_batch(sX, sZ, 0.05, 0, "fixed")
    assert dec.last_path() == set() and dec.get_option("osd_sectors") == 0
    dec.set_option("osd_score", 0)
    assert dec.get_option("osd_score") == 0


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------
def test_cli_osd_score(tmp_path):
    from qec_ldpc_amd.codes import write_css_file
    HX, HZ = matrices("hgp_ham")
    code = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    pri = _write_priors(tmp_path / "p.txt", *prior_vectors(HX.shape[1], "random"))
    line = "4 4 1500 20 0.05"
    base = ["--engine", "cpu", "--seed", "7", "--logical", "degenerate"]
    out = {}
    for rule in ("priors", "hamming"):
        d = tmp_path / rule
        d.mkdir()
        r = _cli(d, base + ["--priors", pri, "--osd", "0", "--osd-order", "10", "--osd-score", rule], code, line)
        assert r.returncode == 0, r.stderr
        out[rule] = _fields(d)
        assert int(out[rule]["Syndrome Errors X"]) == 0 and int(out[rule]["Syndrome Errors Z"]) == 0
        assert int(out[rule]["Corrected"]) + int(out[rule]["Logical Errors"]) == int(out[rule]["Errors Tested"]) > 0
    bad = {"nopriors": ["--osd", "0", "--osd-order", "10", "--osd-score", "priors"],
           "noosd": ["--priors", pri, "--osd-score", "priors"],
           "noosd_hamming": ["--osd-score", "hamming"],
           "unknown": ["--priors", pri, "--osd", "0", "--osd-score", "likelihood"]}
    for key, flags in bad.items():
        d = tmp_path / key
        d.mkdir()
        r = _cli(d, base + flags, code, line)
        assert r.returncode == 2 and "usage: qec_ldpc" in r.stderr, key


# ---- 8. the C++ wrapper ------------------------------------------------------------------------------------------------
def test_set_osd_score_from_cpp(tmp_path, code_paths):
    """include/DecoderCPU.h: SetOsdScore(1) sets option 16, and a bad value throws as SetOsd does."""
    src = tmp_path / "m.cpp"
    src.write_text('#include <iostream>\n#include "DecoderCPU.h"\n#include "Quantum_LDPC_Code.h"\n'
                   'int main(int, char** argv){ Quantum_LDPC_Code code = Quantum_LDPC_Code::createFromFile(argv[1]);\n'
                   ' DecoderCPU decoder(code); int v[4] = {-1, -1, -1, -1};\n'
                   ' qec_decoder_get_option(decoder.handle(), 16, &v[0]);\n'
                   ' decoder.SetOsdScore(1);\n'
                   ' qec_decoder_get_option(decoder.handle(), QEC_OPT_OSD_SCORE, &v[1]);\n'
                   ' bool refused = false; try { decoder.SetOsdScore(2); } catch (const std::string&) { refused = true; }\n'
                   ' qec_decoder_get_option(decoder.handle(), QEC_OPT_OSD_SCORE, &v[2]);\n'
                   ' decoder.SetOsdScore(0);\n'
                   ' qec_decoder_get_option(decoder.handle(), QEC_OPT_OSD_SCORE, &v[3]);\n'
                   ' for (int x : v) std::cout << x << " "; std::cout << refused << std::endl; return 0; }\n')
    exe = tmp_path / "m"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", os.path.join(ROOT, "qec_ldpc_amd"), "-lqecldpc",
                        "-Wl,-rpath," + os.path.join(ROOT, "qec_ldpc_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), code_paths["P7"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["0", "1", "1", "0", "1"]

"""Every instantiation of the sparse-graph BP kernels (bp_sparse.hip): the test codes that reach each of
the 72 decode kernels -- bp_sparse_kernel's regular / general route x (8,4) (16,8) (32,16) x LDS / HBM workspace x
scalar prior / PRIORS x 3 stop rules --, a restatement of sparse_plan_create's choice among them, the case
table that tests/test_gpu_sparse_shapes.py runs on the device (asserted here to cover all 72), and the
references those runs are held to, checked here against the CPU engine:

  * general codes with row weights up to 32 and column weights up to 16: the numpy float32 yardsticks of
    test_general_code.py / test_priors.py;
  * small regular codes of the same degree shapes: the oracle (scalar) and the priors yardstick;
  * block-diagonal replications whose workspace exceeds LDS: under the fixed stop, sample b of r blocks is
    r independent samples of the small code, so the small yardstick is a reference for the HBM kernels that
    does not go through the CPU engine.

Every comparison is bit for bit (q_final as uint32 patterns, NaN matching NaN).  There is no tolerance.

Which code runs which shape (each with the scalar p and with priors, under the three stop rules):

  route              shape    LDS                                    HBM
  regular            (8,4)    r3-3-6-13                              r3-3-6-1013 (164 112 B)
                     (16,8)   r4-5-10-7                              r4-5-10-467
                     (32,16)  r3-9-20-7, r2-12-6-13, r3-3-18-5       r3-9-20-163
  general            (8,4)    hgp_ham, r3-3-6-13                     hgp_ham*140 (186 768 B)
                     (16,8)   mid, r4-5-10-7                         mid*40 (169 648 B)
                     (32,16)  wide, dense32, tall, r3-9-20-7,        wide*15 (177 824 B)
                              r2-12-6-13, r3-3-18-5

Iteration counts of the references (assert_not_vacuous, assert_hbm_stops), X / Z, 51 rows, cap 20:

  code         syndrome stop, p = 0.02                    ref stop, p = 0.005
  hgp_ham      {1,20} / {1,20}                            {1,11,20} / {1,11,20}
  mid          {1,3,4,10,17,20} / {1..5,20}               {1,11,20} / {1,11,20}
  wide         {1,20} / {1..6,20}                         {1,11,20} / {1,11,20}
  dense32      {1,20} / {1,20}                            {1,20} / {1,11,20}
  tall         {1,20} / {1,4,20}                          {1,20} / {1,11,20}
  r3-3-6-13    {1..6,9,10,20} / {1..6,20}                 {1,11,20} / {1,11,20}
  r4-5-10-7    {1,3,20} / {1,20}                          {1,11,20} / {1,11,20}
  r3-9-20-7    {1,2,5,20} / {1,4,6,11,12,16,20}           {1,11,20} / {1,11,20}
  r2-12-6-13   {1,2,4,20} / {1,2,3,20}                    {1,11,20} / {1,11} (NEVER_TO_CAP)
  r3-3-18-5    {1,20} / {1,20}                            {1,20} / {1,20}

At the decode p of 0.02 the ref stop never ends a sector of a general code early (every one runs to the cap).
HBM codes, sampled rows (the all-zero row always stops at 1): the replicated codes run to 20 in both sectors under
both rules, but for one Z sector of wide*15 that the ref stop ends at 11; the large regular codes give {4,5,20} /
{4,14,20}, {3,4,20} / {3,20}, {20} / {3,4,20} under the syndrome stop and {11,20} in every sector but X of
r3-9-20-163 ({20}) under the ref stop."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import write_code_file
from qec_ldpc_amd.synthetic import depolarizing_errors
from test_general_code import (HAMMING, NS, STOPS, assert_same_decode, bp_yardstick, code_matrices, hgp,
                               mixed_syndromes, same_floats)
from test_priors import VECTORS, bp_yardstick_priors, prior_vectors

F32 = np.float32


# ---- the test codes ---------------------------------------------------------------------------------------
def _h2():
    """8 x 9: column j has weight 1 + (3 j mod 8), its ones in rows (i + j) mod 8 for i < weight."""
    H = np.zeros((8, 9), dtype=np.uint8)
    for j in range(9):
        for i in range(1 + (3 * j) % 8):
            H[(i + j) % 8, j] = 1
    return H


def _h1():
    """2 x 14: row 0 all ones, row 1 ones in its first 9 columns."""
    H = np.zeros((2, 14), dtype=np.uint8)
    H[0] = 1
    H[1, :9] = 1
    return H


H2, H1 = _h2(), _h1()


def _dense32():
    """n = 32, 4 + 16 checks (64 threads).  HX: a row over every qubit beside rows of weight 23, 11 and 14
    (the largest degree byte and a full-stride check next to short ones); HZ: column v has weight
    1 + (5 v mod 16), so every column weight from 1 to 16 occurs.  The matrices do not commute (BP does not ask)."""
    HX = np.zeros((4, 32), dtype=np.uint8)
    HX[0] = 1
    HX[1, :23] = 1
    HX[2, ::3] = 1
    HX[3, 5::2] = 1
    HZ = np.zeros((16, 32), dtype=np.uint8)
    for v in range(32):
        for i in range(1 + (5 * v) % 16):
            HZ[(i + v) % 16, v] = 1
    return HX, HZ


def _tall():
    """n = 20, 6 + 16 checks of weight 3..7 (D = 7, which alone would choose MAXDC = 8) and two Z columns of
    weight 12 and 10: the (32,16) kernel through the column weight alone.  Qubits 0, 1 and 2 are in no X check."""
    n = 20
    HX = np.zeros((6, n), dtype=np.uint8)
    for r in range(6):
        for i in range(3 + r % 5):
            HX[r, (3 * r + i) % n] = 1
    HZ = np.zeros((16, n), dtype=np.uint8)
    HZ[:12, 0] = 1
    HZ[4:14, 1] = 1
    for r in range(16):
        for i in range(2 + r % 4):
            HZ[r, 2 + (3 * r + i) % 18] = 1
    return HX, HZ


SMALL_GENERAL = ("hgp_ham", "mid", "wide", "dense32", "tall")
REPLICATED = {"hgp_ham*140": ("hgp_ham", 140), "mid*40": ("mid", 40), "wide*15": ("wide", 15)}
SIGMA_TAU = (2, 3)
SMALL_REGULAR = {"r3-3-6-13": (3, 3, 6, 13), "r4-5-10-7": (4, 5, 10, 7), "r3-9-20-7": (3, 9, 20, 7),
                 "r2-12-6-13": (2, 12, 6, 13), "r3-3-18-5": (3, 3, 18, 5)}
LARGE_REGULAR = {"r3-3-6-1013": (3, 3, 6, 1013), "r4-5-10-467": (4, 5, 10, 467), "r3-9-20-163": (3, 9, 20, 163)}
REGULAR = dict(SMALL_REGULAR, **LARGE_REGULAR)
PRIOR_YARDSTICK = SMALL_GENERAL + ("r4-5-10-7", "r3-9-20-7")  # codes with a numpy reference under priors

_mats, _codes = {}, {}


def matrices(name):
    """(HX, HZ) of a test code."""
    if name not in _mats:
        if name in REGULAR:
            g = code_of(name, "graph")
            _mats[name] = (g.pcm(0), g.pcm(1))
        elif name in REPLICATED:
            base, r = REPLICATED[name]
            eye = np.eye(r, dtype=np.uint8)
            _mats[name] = tuple(np.ascontiguousarray(np.kron(eye, H)) for H in matrices(base))
        else:
            _mats[name] = {"hgp_ham": lambda: code_matrices("hgp_ham"), "mid": lambda: hgp(HAMMING, H2),
                           "wide": lambda: hgp(H1, H2), "dense32": _dense32, "tall": _tall}[name]()
    return _mats[name]


def code_of(name, route):
    """route "graph": the generated regular code (bp_sparse_kernel's regular route, GENERAL = false); "general": the
    code from its two matrices (GENERAL = true)."""
    key = (name, route)
    if key not in _codes:
        if route == "graph":
            _codes[key] = q.QC_LDPC_CSS(*REGULAR[name], *SIGMA_TAU)
        else:
            assert route == "general"
            _codes[key] = q.Quantum_LDPC_Code.createFromMatrices(*matrices(name))
    return _codes[key]


# ---- sparse_plan_create, restated -----------------------------------------------------------------------------
KERNELS = ("regular", "general")  # the route: bp_sparse_kernel<..., GENERAL = false / true, BODY>
SHAPES = ((8, 4), (16, 8), (32, 16))
ALL_INSTANCES = {(k, s, mem, pri, stop) for k in KERNELS for s in SHAPES for mem in ("lds", "hbm")
                 for pri in (False, True) for stop in STOPS}


def plan_of(code, general):
    """bp_sparse.hip, sparse_plan_create: ws_bytes and the LDS / HBM threshold (the lines `p->ws_bytes = ...` and
    `p->lds = ...`), wdc / wdv and the smallest instantiated shape that covers both (`const int wdc`, `const int
    wdv` and the if / else-if chain under "instantiated shapes"), and a general code's workgroup of 64 / 128 /
    256 threads (`p->threads = ...`); a regular code always runs kSparseThreads = 256."""
    dc, dvX, dvZ = code.degrees()[4], code.degrees()[2], code.degrees()[3]
    n, m = code.n, code.numEqsX + code.numEqsZ
    ws_bytes = (4 * m * dc + m + 2 * n + 15) // 16 * 16
    lds = ws_bytes <= 160 * 1024 - 64
    wdc = 8 if dc <= 8 else 16 if dc <= 16 else 32
    dv = max(dvX, dvZ)
    wdv = 4 if dv <= 4 else 8 if dv <= 8 else 16
    shape = (8, 4) if wdc <= 8 and wdv <= 4 else (16, 8) if wdc <= 16 and wdv <= 8 else (32, 16)
    wide = max(m, 2 * n)
    threads = (64 if wide <= 64 else 128 if wide <= 128 else 256) if general else 256
    return {"kernel": KERNELS[bool(general)], "shape": shape, "mem": "lds" if lds else "hbm", "ws_bytes": ws_bytes,
            "threads": threads, "D": dc, "dv": (dvX, dvZ)}


def instance_of(code, general, priors, stop):
    """The decode kernel that launch_decode_sparse starts for this code: (kernel, (MAXDC, MAXDV), workspace,
    PRIORS, stop rule)."""
    assert stop in STOPS
    p = plan_of(code, general)
    return (p["kernel"], p["shape"], p["mem"], bool(priors), stop)


# ---- the case table of tests/test_gpu_sparse_shapes.py -----------------------------------------------------------
# (code, route): every row runs with the scalar p and with priors, under every stop rule.
CASES = (tuple((name, "general") for name in SMALL_GENERAL) +
         tuple((name, "general") for name in REPLICATED) +
         tuple((name, "graph") for name in SMALL_REGULAR) +
         tuple((name, "general") for name in SMALL_REGULAR) +
         tuple((name, "graph") for name in LARGE_REGULAR))


def case_id(case):
    return "%s-%s" % case


def is_lds(case):
    return case[0] in SMALL_GENERAL or case[0] in SMALL_REGULAR


LDS_CASES = tuple(c for c in CASES if is_lds(c))
HBM_CASES = tuple(c for c in CASES if not is_lds(c))

# name -> (n, mX, mZ, degrees, (MAXDC, MAXDV), general-route threads or None)
PINNED = {
    "hgp_ham": (58, 21, 21, (7, 7, 4, 4, 7), (8, 4), 128),
    "mid": (87, 27, 56, (12, 10, 7, 8, 12), (16, 8), 256),
    "wide": (142, 18, 112, (22, 9, 7, 14, 22), (32, 16), 256),
    "dense32": (32, 4, 16, (32, 18, 4, 16, 32), (32, 16), 64),
    "tall": (20, 6, 16, (7, 7, 2, 12, 7), (32, 16), 64),
    "hgp_ham*140": (8120, 2940, 2940, (7, 7, 4, 4, 7), (8, 4), 256),
    "mid*40": (3480, 1080, 2240, (12, 10, 7, 8, 12), (16, 8), 256),
    "wide*15": (2130, 270, 1680, (22, 9, 7, 14, 22), (32, 16), 256),
    "r3-3-6-13": (78, 39, 39, (6, 6, 3, 3, 6), (8, 4), 256),
    "r4-5-10-7": (70, 28, 35, (10, 10, 4, 5, 10), (16, 8), 256),
    "r3-9-20-7": (140, 21, 63, (20, 20, 3, 9, 20), (32, 16), 256),
    "r2-12-6-13": (78, 26, 156, (6, 6, 2, 12, 6), (32, 16), 256),
    "r3-3-18-5": (90, 15, 15, (18, 18, 3, 3, 18), (32, 16), 256),
    "r3-3-6-1013": (6078, 3039, 3039, (6, 6, 3, 3, 6), (8, 4), None),
    "r4-5-10-467": (4670, 1868, 2335, (10, 10, 4, 5, 10), (16, 8), None),
    "r3-9-20-163": (3260, 489, 1467, (20, 20, 3, 9, 20), (32, 16), None),
}
LDS_LIMIT = 160 * 1024 - 64  # 163 776
WS_BYTES = {"hgp_ham*140": 186768, "wide*15": 177824, "r3-3-6-1013": 164112}


def test_h1_and_h2():
    assert H2.shape == (8, 9) and H1.shape == (2, 14)
    assert list(H2.sum(axis=1)) == [7, 3, 4, 5, 6, 3, 4, 5]
    assert list(H2.sum(axis=0)) == [1, 4, 7, 2, 5, 8, 3, 6, 1]
    assert list(H1.sum(axis=1)) == [14, 9]


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_shapes(name):
    """A change to a construction cannot move a code into another instantiation unnoticed."""
    n, mX, mZ, degrees, shape, threads = PINNED[name]
    routes = [r for c, r in CASES if c == name]
    assert routes
    for route in routes:
        code = code_of(name, route)
        assert (code.n, code.numEqsX, code.numEqsZ) == (n, mX, mZ)
        assert code.degrees() == degrees
        plan = plan_of(code, route == "general")
        assert plan["shape"] == shape
        assert plan["mem"] == ("lds" if is_lds((name, route)) else "hbm")
        assert plan["kernel"] == ("general" if route == "general" else "regular")
        if route == "general":
            assert plan["threads"] == threads
        if name in WS_BYTES:
            assert plan["ws_bytes"] == WS_BYTES[name]
        if not is_lds((name, route)):
            assert plan["ws_bytes"] > LDS_LIMIT
    if name in REGULAR:
        J, K, L, P = REGULAR[name]
        assert degrees == (L, L, J, K, L) and (n, mX, mZ) == (L * P, J * P, K * P)


def test_pinned_weights_and_commutation():
    def commute(H):
        return not ((H[0].astype(np.int64) @ H[1].T) & 1).any()

    def sets(H):  # row weights X, column weights X, row weights Z, column weights Z
        return [set(int(x) for x in M.sum(axis=a)) for M in H for a in (1, 0)]

    rX, cX, rZ, cZ = sets(matrices("wide"))
    assert rX == set(range(10, 23)) and rZ == set(range(4, 10))
    assert cX == set(range(1, 8)) and cZ == set(range(1, 10)) | {14}
    assert 2 * PINNED["wide"][0] > 256  # the variable pass loops
    assert commute(matrices("mid")) and commute(matrices("wide")) and commute(matrices("hgp_ham"))
    assert code_of("mid", "general").describe() == "[[n=87,k=4]]"
    assert code_of("wide", "general").describe() == "[[n=142,k=12]]"
    rX, cX, rZ, cZ = sets(matrices("dense32"))
    assert 32 in rX and rX & set(range(17, 32)) and max(rZ) <= 32 and cZ == set(range(1, 17))
    assert all(H.sum(axis=1).min() > 0 for H in matrices("dense32"))
    rX, cX, rZ, cZ = sets(matrices("tall"))
    assert max(rX | rZ) <= 8 and max(cX) <= 4 and cZ & set(range(9, 17)) and 0 in cX
    assert all(H.sum(axis=1).min() > 0 for H in matrices("tall"))
    # the (16,8) replication exceeds LDS by the plan's own formula
    m, n, D = 40 * (27 + 56), 40 * 87, 12
    assert plan_of(code_of("mid*40", "general"), True)["ws_bytes"] == (4 * m * D + m + 2 * n + 15) // 16 * 16 > LDS_LIMIT
    assert WS_BYTES["r3-3-6-1013"] - LDS_LIMIT == 336


def test_case_table_reaches_every_instantiation():
    """72 of 72: a shape, a workspace mode or a kernel that the table does not run fails here."""
    reached = {instance_of(code_of(name, route), route == "general", pri, stop)
               for name, route in CASES for pri in (False, True) for stop in STOPS}
    assert len(ALL_INSTANCES) == 72
    assert reached == ALL_INSTANCES, sorted(ALL_INSTANCES - reached)
    lds = {instance_of(code_of(name, route), route == "general", pri, stop)
           for name, route in LDS_CASES for pri in (False, True) for stop in STOPS}
    assert lds == {i for i in ALL_INSTANCES if i[2] == "lds"}


# ---- inputs and references of the LDS codes ----------------------------------------------------------------------
RATES = (0.01, 0.03, 0.08)   # error rates of the sampled syndromes
P_MAIN, P_REF = 0.02, 0.005  # decode p; at p >= 0.02 p' lies inside (0.01, 0.99) and the ref stop never ends early
ROWS = 51
# (stop, p, N); the ref stop a second time at the p where it ends sectors at its tests of iterations 1, 11, 21, ...
SCALAR_CASES = tuple((stop, P_MAIN, N) for stop in STOPS for N in NS) + tuple(("ref", P_REF, N) for N in (11, 20, 50))
PRIOR_CASES = tuple((kind, stop, N) for kind in VECTORS for stop in STOPS for N in NS)
# the regular codes' priors yardstick is the slowest (0.05 s per iteration of r3-9-20-7): N = 1 and 11, where the ref
# stop has made both its tests (after iterations 1 and 11)
REGULAR_PRIOR_CASES = tuple(c for c in PRIOR_CASES if c[2] in (1, 11))
COVERAGE = (("syndrome", P_MAIN, 20), ("ref", P_REF, 20))
# (code, stop, sector) that never runs to the cap: r2-12-6-13's Z sector (column weight 12) under the ref stop gave
# iteration counts {1, 11} at every decode p in (0.002, 0.005, 0.02), every syndrome error-rate set in
# ((0.003, 0.01, 0.03), (0.01, 0.03, 0.08), (0.05,)) and both caps 20 and 50: every message is outside (0.01, 0.99)
# by the second test.  The distribution is asserted instead.
NEVER_TO_CAP = {("r2-12-6-13", "ref", 1): {1, 11}}

_inputs, _yard = {}, {}


def inputs(name):
    """48 sampled syndromes over RATES, the all-zero row, the all-one row and a row with an entry > 1."""
    if name not in _inputs:
        _inputs[name] = mixed_syndromes(matrices(name), 4242, ROWS, RATES)
    return _inputs[name]


def yardstick(name, stop, p, N):
    key = (name, stop, p, N)
    if key not in _yard:
        _yard[key] = bp_yardstick(*matrices(name), *inputs(name), p, N, stop)
    return _yard[key]


def yardstick_priors(name, kind, stop, N):
    key = (name, kind, stop, N)
    if key not in _yard:
        HX, HZ = matrices(name)
        _yard[key] = bp_yardstick_priors(HX, HZ, *inputs(name), *prior_vectors(HX.shape[1], kind), N, stop)
    return _yard[key]


def prior_cases(name):
    return REGULAR_PRIOR_CASES if name in REGULAR else PRIOR_CASES


def oracles(tmp):
    """name -> OracleCode of the small regular codes, their files written under tmp."""
    out = {}
    for name, (J, K, L, P) in SMALL_REGULAR.items():
        HX, HZ = matrices(name)
        out[name] = OracleCode(write_code_file(str(tmp / (name + ".txt")), J, K, L, P, *SIGMA_TAU, HX, HZ))
    return out


_oracle_out = {}


def scalar_reference(name, stop, p, N, orc=None):
    """The numpy yardstick for a general code, the oracle (orc: oracles()) for a regular one."""
    if name in SMALL_GENERAL:
        return yardstick(name, stop, p, N)
    key = (name, stop, p, N)
    if key not in _oracle_out:
        _oracle_out[key] = orc[name].decode_batch(*inputs(name), p, N, stop, want_q=True)
    return _oracle_out[key]


# Codes whose syndrome stop never ends a sector between the first iteration and the cap on these inputs: their
# distribution, {1, 20} in both sectors, is asserted instead (the exits at 1 are rows that the first iteration's
# hard decision already satisfies).  hgp_ham showed a mid-run exit only at other inputs (48 rows at rate 0.05:
# Z {1, 2, 20}); dense32 and r3-3-18-5 at none of the error-rate sets and decode p of 0.02 / 0.05 that were tried.
NO_MID_RUN_EXIT = ("hgp_ham", "dense32", "r3-3-18-5")


def assert_not_vacuous(name, orc=None):
    """On the reference's outputs.  Under the syndrome and the ref stop each sector has a row that stops before the
    cap and one that runs to it, and under the syndrome stop some sector ends strictly between iteration 1 and the
    cap (but NO_MID_RUN_EXIT).  The flags are taken over all scalar cases of the code together, not per batch: a
    syndrome-stop batch sets a convergence bit in nearly every row (its messages are still inside (0.01, 0.99)
    when the hard decision satisfies the syndrome), so the clean row comes from the ref-stop batches and the
    failure bits from either; over them there is a row with flags 0 and a row with each failure bit."""
    for stop, p, N in COVERAGE:
        it = scalar_reference(name, stop, p, N, orc)[3]
        seen = [set(int(x) for x in it[:, sec]) for sec in (0, 1)]
        for sec in (0, 1):
            if (name, stop, sec) in NEVER_TO_CAP:
                assert seen[sec] == NEVER_TO_CAP[(name, stop, sec)], (name, stop, sec, sorted(seen[sec]))
            else:
                assert min(seen[sec]) < N and max(seen[sec]) == N, (name, stop, sec, sorted(seen[sec]))
        if stop == "syndrome":
            if name in NO_MID_RUN_EXIT:
                assert seen == [{1, N}, {1, N}], (name, seen)
            else:
                assert any(1 < k < N for k in seen[0] | seen[1]), (name, seen)
    flags = np.concatenate([scalar_reference(name, *case, orc)[2] for case in SCALAR_CASES])
    assert (flags == 0).any(), name
    for bit in (q.SYNDROME_FAIL_X, q.SYNDROME_FAIL_Z, q.CONVERGENCE_FAIL_X, q.CONVERGENCE_FAIL_Z):
        assert (flags & bit).any(), (name, bit)


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return oracles(tmp_path_factory.mktemp("sparse_shapes"))


@pytest.mark.parametrize("name", SMALL_GENERAL)
def test_cpu_engine_matches_yardstick(name):
    dec = q.DecoderCPU(code_of(name, "general"))
    sX, sZ = inputs(name)
    for stop, p, N in SCALAR_CASES:
        got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, yardstick(name, stop, p, N), "%s %s p=%g N=%d" % (name, stop, p, N))
    assert_not_vacuous(name)


@pytest.mark.parametrize("name", PRIOR_YARDSTICK)
def test_cpu_engine_matches_prior_yardstick(name):
    code = code_of(name, "graph" if name in REGULAR else "general")
    dec = q.DecoderCPU(code)
    sX, sZ = inputs(name)
    for kind, stop, N in prior_cases(name):
        dec.set_priors(*prior_vectors(code.n, kind))
        got = dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)  # p is not used
        assert_same_decode(got, yardstick_priors(name, kind, stop, N), "%s %s %s N=%d" % (name, kind, stop, N))
    # the priors matter: the reference under the random vector is not the scalar decode
    dec.set_priors(None, None)
    scalar = dec.decode_batch(sX, sZ, P_MAIN, 11, "fixed", want_q=True)
    assert not same_floats(scalar[4], yardstick_priors(name, "random", "fixed", 11)[4])


def test_wide_reference_holds_nans_and_denormals():
    """The (32,16) comparisons include non-finite and denormal messages."""
    qf = np.concatenate([yardstick("wide", *case)[4].ravel() for case in SCALAR_CASES])
    assert np.isnan(qf).any()
    assert ((np.abs(qf) < np.finfo(F32).tiny) & (qf != 0)).any()


@pytest.mark.parametrize("name", sorted(SMALL_REGULAR))
def test_cpu_engine_matches_oracle_on_regular_codes(orc, name):
    """Both routes: the generated code (decode_sector) and the same matrices as a general code."""
    sX, sZ = inputs(name)
    for route in ("graph", "general"):
        dec = q.DecoderCPU(code_of(name, route))
        for stop, p, N in SCALAR_CASES:
            got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            assert_same_decode(got, scalar_reference(name, stop, p, N, orc), "%s %s %s p=%g N=%d" % (name, route, stop, p, N))
    assert_not_vacuous(name, orc)


# ---- the HBM codes ------------------------------------------------------------------------------------------------
HBM_RATE, HBM_ROWS, HBM_N = 0.03, 6, 11
HBM_STOPS = (("ref", P_REF, 20), ("fixed", P_MAIN, HBM_N), ("syndrome", P_MAIN, 20))  # (stop, p, N)
_block = {}


def tail_rows(m):
    return np.stack([np.zeros(m), np.ones(m), np.r_[2, np.ones(m - 1)]]).astype(np.uint8)


def hbm_priors(name):
    """A replicated code: the small code's random vector tiled over the blocks (each block then decodes its own
    syndrome under the same priors); a regular code: its own random vector."""
    if name in REPLICATED:
        base, r = REPLICATED[name]
        return tuple(np.tile(pr, r) for pr in prior_vectors(matrices(base)[0].shape[1], "random"))
    return prior_vectors(PINNED[name][0], "random")


def block_rows(name):
    """HBM_ROWS samples of a replicated code as r samples of the small code each: (small sX, small sZ, sX, sZ),
    sample b of the big code being the small rows b r .. b r + r - 1 side by side (different in every block)."""
    if name not in _block:
        base, r = REPLICATED[name]
        HX, HZ = matrices(base)
        x, z = depolarizing_errors(HX.shape[1], 31337, HBM_ROWS * r, HBM_RATE)
        sx, sz = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        assert len(np.unique(sx[:r], axis=0)) > 1 and len(np.unique(sz[:r], axis=0)) > 1
        _block[name] = (sx, sz, np.ascontiguousarray(sx.reshape(HBM_ROWS, -1)), np.ascontiguousarray(sz.reshape(HBM_ROWS, -1)))
    return _block[name]


def block_reference(name, priors):
    """The fixed-stop decode of block_rows(name) put together from the small code's yardstick: eX / eZ are the r
    small rows side by side, a flag is set when it is in any block, and q_final is the X slices of the r blocks
    followed by their Z slices."""
    key = (name, "block", priors)
    if key not in _yard:
        base, r = REPLICATED[name]
        HX, HZ = matrices(base)
        sx, sz = block_rows(name)[:2]
        if priors:
            small = bp_yardstick_priors(HX, HZ, sx, sz, *prior_vectors(HX.shape[1], "random"), HBM_N, "fixed")
        else:
            small = bp_yardstick(HX, HZ, sx, sz, P_MAIN, HBM_N, "fixed")
        D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
        EX = HX.shape[0] * D
        qs = small[4].reshape(HBM_ROWS, r, -1)
        qf = np.concatenate([qs[:, :, :EX].reshape(HBM_ROWS, -1), qs[:, :, EX:].reshape(HBM_ROWS, -1)], axis=1)
        flags = np.bitwise_or.reduce(small[2].reshape(HBM_ROWS, r), axis=1)
        iters = small[3].reshape(HBM_ROWS, r, 2)
        assert (iters == HBM_N).all()
        _yard[key] = (small[0].reshape(HBM_ROWS, -1), small[1].reshape(HBM_ROWS, -1), flags,
                      np.ascontiguousarray(iters[:, 0]), np.ascontiguousarray(qf))
    return _yard[key]


def hbm_inputs(name):
    """HBM_ROWS sampled rows (block_rows for a replicated code), then the three special rows."""
    if name not in _inputs:
        if name in REPLICATED:
            sX, sZ = block_rows(name)[2:]
        else:
            code = code_of(name, "graph")
            # the large regular codes decode HBM_RATE in 3 to 5 iterations: half the rows at a rate they fail at
            half = [depolarizing_errors(code.n, 31337 + k, HBM_ROWS // 2, rate) for k, rate in enumerate((HBM_RATE, 0.1))]
            x, z = np.concatenate([h[0] for h in half]), np.concatenate([h[1] for h in half])
            sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
        _inputs[name] = (np.concatenate([sX, tail_rows(sX.shape[1])]), np.concatenate([sZ, tail_rows(sZ.shape[1])]))
    return _inputs[name]


def assert_hbm_stops(name, stop, N, iters):
    """On the reference: a stop rule tests all blocks of a large code at once, so no sampled row ends at the first
    test and, in each sector, at least one runs to the cap (wide*15 under the ref stop: one Z sector of six ends at
    iteration 11); the all-zero row stops at the first test."""
    if stop == "fixed":
        assert (iters == N).all()
    else:
        assert (iters[:HBM_ROWS] > 1).all(), (name, stop, iters[:HBM_ROWS].tolist())
        assert (iters[:HBM_ROWS].max(axis=0) == N).all(), (name, stop, iters[:HBM_ROWS].tolist())
        assert (iters[HBM_ROWS] == 1).all(), (name, stop, iters[HBM_ROWS].tolist())


@pytest.mark.parametrize("name", sorted(REPLICATED))
@pytest.mark.parametrize("priors", [False, True], ids=["scalar", "priors"])
def test_cpu_engine_decodes_a_replicated_code_block_by_block(name, priors):
    dec = q.DecoderCPU(code_of(name, "general"))
    if priors:
        dec.set_priors(*hbm_priors(name))
    sX, sZ = block_rows(name)[2:]
    got = dec.decode_batch(sX, sZ, P_MAIN, HBM_N, "fixed", want_iters=True, want_q=True)
    assert_same_decode(got, block_reference(name, priors), "%s priors=%s" % (name, priors))
    if priors:
        assert not same_floats(block_reference(name, True)[4], block_reference(name, False)[4])


@pytest.mark.parametrize("name", sorted(REPLICATED))
def test_hbm_stop_coverage_of_the_replicated_codes(name):
    dec = q.DecoderCPU(code_of(name, "general"))
    for stop, p, N in HBM_STOPS:
        assert_hbm_stops(name, stop, N, dec.decode_batch(*hbm_inputs(name), p, N, stop, want_iters=True)[3])

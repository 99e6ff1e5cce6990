"""The serial (layered, check-sequential) BP schedule, set_option("bp_schedule", 1): DESIGN.md section 2, "The serial
schedule", restated in numpy float32 and held against the CPU engine; the layers (qec_code_layers) against the
greedy colouring restated here; the restated choice among the 36 SERIAL kernels of bp_sparse.hip and the case table
that tests/test_gpu_serial.py runs on the device (asserted here to reach all 36); the option's refusals; the OSD
stage's soft decode; the benefit on the [[58,16]] Hamming hypergraph product; the CLI.  The refusal of a
wave-circulant handle needs a device and is in tests/test_gpu_serial.py.

Every comparison is bit for bit (q_final as uint32 patterns, NaN matching NaN).  There is no tolerance.

Layers (X / Z): hgp_ham 7 / 7, mid 8 / 8, wide 8 / 16, dense32 4 / 16 (HZ: one check per layer), tall 2 / 12,
every regular code J / K with the colour of check c equal to c // P.

Iteration counts under the serial schedule on the CPU engine, X / Z, the 51 rows of test_sparse_shapes.inputs, cap 20
(SERIAL_P is the decode p chosen per code so that the stop rules end sectors at the first test, at the cap and,
under the syndrome stop, between):

  code         syndrome stop, p = 0.05                    ref stop, p = 0.005
  hgp_ham      {1,2,3,4,16,20} / {1,2,16,20}              {1,11,20} / {1,11,20}
  mid          {1..5,20} / {1,2,20}                       {1,11,20} / {1,11,20}
  wide         {1,20} / {1,2,5,9,11,20}                   {1,11,20} / {1,11,20}
  dense32      {1,20} / {1,2,3,10,20}                     {1,20} / {1,11,20}
  tall         {1,20} / {1,20}                            {1,20} / {1,20}
  r3-3-6-13    {1,2,3,8,17,20} / {1,2,3,20}               {1,11,20} / {1,11,20}
  r4-5-10-7    {1,2,3,7,9,12,20} / {1,2,4,9,20}           {1,11,20} / {1,11,20}
  r3-9-20-7    {1,20} / {1,8,11,16,20}                    {1,20} / {1,20}
  r2-12-6-13   {1,2,16,20} / {1,2,20}                     {1,11,20} / {1,11,20}
  r3-3-18-5    {1,12,17,19,20} / {1,12,14,15,17,20}       {1,20} / {1,20}

Flooding at the flooding file's p = 0.02 leaves hgp_ham, dense32 and r3-3-18-5 without an exit between 1 and the cap
(test_sparse_shapes.NO_MID_RUN_EXIT); under the serial schedule every code but tall has one.
"""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from test_general_code import NS, STOPS, assert_same_decode, code_matrices, general_code, same_floats
from test_priors import VECTORS, prior_vectors
from test_sparse_shapes import (CASES, KERNELS, REGULAR, SHAPES, SMALL_GENERAL, SMALL_REGULAR, code_of, inputs, matrices,
                                plan_of)

F32 = np.float32


# ---- the layers, restated ---------------------------------------------------------------------------------------
def greedy_colours(H):
    """Walking the checks in ascending index, check c gets the smallest colour none of whose checks shares a
    variable with c."""
    used, colour = [], []
    for row in np.asarray(H, dtype=bool):
        for l, mask in enumerate(used):
            if not (mask & row).any():
                break
        else:
            l = len(used)
            used.append(np.zeros(row.shape, dtype=bool))
        used[l] |= row
        colour.append(l)
    return np.array(colour, dtype=np.int32)


def processing_order(colour):
    return sorted(range(len(colour)), key=lambda c: (colour[c], c))


LAYERS = {"hgp_ham": (7, 7), "mid": (8, 8), "wide": (8, 16), "dense32": (4, 16), "tall": (2, 12), "r4-5-10-7": (4, 5)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_layers_are_the_greedy_colouring(case):
    name, route = case
    code = code_of(*case)
    for sec, H in enumerate(matrices(name)):
        colour = code.layers(sec)
        assert colour.dtype == np.int32 and np.array_equal(colour, greedy_colours(H)), (name, sec)
        assert q.lib().qec_code_layers(code._h, sec, None) == colour.max() + 1  # the count alone
        for l in range(colour.max() + 1):  # checks of one colour share no variable
            assert H[colour == l].sum(axis=0).max() <= 1
        if name in REGULAR:
            J, K, L, P = REGULAR[name]
            assert np.array_equal(colour, np.arange(len(colour)) // P) and colour.max() + 1 == (K if sec else J)
    if name in LAYERS:
        assert tuple(int(code.layers(sec).max()) + 1 for sec in (0, 1)) == LAYERS[name]
    if name == "dense32":
        assert np.array_equal(code.layers(1), np.arange(16))
    assert q.lib().qec_code_layers(code._h, 2, None) == -1  # QEC_ERR_ARG


# ---- the yardstick: "The serial schedule" of DESIGN.md section 2 in numpy float32 ------------------------------------
def _inside(x):
    return (x > F32(0.01)) & (x < F32(0.99))


def serial_sector(H, s, pi, N, stop, D):
    """One sector of a batch, sequential over the processing order, every float32 operation in its stated order,
    elementwise over the batch.  pi: the prior of every variable (the scalar case: p' everywhere).
    -> (e [B, n], syndrome failed [B], convergence failed [B], iterations [B], q [B, m, D])."""
    m, n = H.shape
    B = s.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]                                  # N(c), ascending
    edges = [[(int(c), int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]  # M(v)
    order = processing_order(greedy_colours(H))
    real = np.zeros((m, D), dtype=bool)
    for c in range(m):
        real[c, :len(nbr[c])] = True
    pi = np.asarray(pi, dtype=F32)
    omp = (F32(1.0) - pi).astype(F32)
    R = np.where(real, F32(0.5), F32(0.0)).astype(F32)[None].repeat(B, axis=0)
    h = np.where(s != 0, F32(0.5), F32(-0.5)).astype(F32)                          # truthiness of the syndrome entry
    connected = np.array([len(edges[v]) > 0 for v in range(n)])
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)

    def fold(R, v, skip):
        P0, P1 = np.full(B, omp[v], dtype=F32), np.full(B, pi[v], dtype=F32)
        for c, k in edges[v]:
            if c != skip:
                P0, P1 = P0 * (F32(1.0) - R[:, c, k]), P1 * R[:, c, k]
        return P1 / (P0 + P1)

    def posterior(R):
        post = np.zeros((B, n), dtype=F32)
        for v in range(n):
            if connected[v]:
                post[:, v] = fold(R, v, -1)
        return post

    def decide(post):
        return ((post >= F32(0.5)) & connected[None]).astype(np.uint8)  # a variable in no check decides 0

    def syndrome_fails(e):
        bad = np.zeros(B, dtype=bool)
        for c in range(m):
            bad |= (e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) != s[:, c]  # the entry's exact value
        return bad

    def inside_any(post):
        return (_inside(post) & connected[None]).any(axis=1)

    with np.errstate(all="ignore"):
        for it in range(N):
            if not active.any():
                break
            iters += active
            new = R.copy()
            for c in order:
                qs = [fold(new, v, c) for v in nbr[c]]
                a = [F32(1.0) - F32(2.0) * x for x in qs]
                pre = np.ones(B, dtype=F32)
                for i in range(len(a)):
                    t = pre
                    for k in range(i + 1, len(a)):
                        t = t * a[k]
                    new[:, c, i] = F32(0.5) + h[:, c] * t
                    pre = pre * a[i]
            R = np.where(active[:, None, None], new, R)
            if stop == "ref" and it % 10 == 0:
                active &= inside_any(posterior(R))
            elif stop == "syndrome":
                active &= syndrome_fails(decide(posterior(R)))
        post = posterior(R)
    e = decide(post)
    qf = np.zeros((B, m, D), dtype=F32)
    for c in range(m):
        qf[:, c, :len(nbr[c])] = post[:, nbr[c]]
    return e, syndrome_fails(e), inside_any(post), iters, qf


def serial_yardstick(HX, HZ, sX, sZ, piX, piZ, N, stop):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D]); piX / piZ: n priors each, or a scalar p for both."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    n = HX.shape[1]
    if np.ndim(piX) == 0:
        piX = piZ = np.full(n, F32(2.0) / F32(3.0) * F32(piX), dtype=F32)
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fx, cx, ix, qx = serial_sector(HX, sX, piX, N, stop, D)
    eZ, fz, cz, iz, qz = serial_sector(HZ, sZ, piZ, N, stop, D)
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32)


def serial_cpu(code, priors=None):
    dec = q.DecoderCPU(code)
    dec.set_option("bp_schedule", 1)
    if priors is not None:
        dec.set_priors(*priors)
    return dec


# the decode p per code: see the table in the module docstring
SMALL = SMALL_GENERAL + tuple(SMALL_REGULAR)
SERIAL_P = dict.fromkeys(SMALL, 0.05)  # 0.05 serves every code (0.02, 0.08 and 0.12 were tried too)
SERIAL_P_REF = 0.005  # p' is then outside (0.01, 0.99) and the reference stop can end a sector at its first test
# the numpy yardstick of the codes with the heaviest rows and columns is the slowest (0.04 to 0.09 s per iteration):
# N = 0, 1, 2 and 11 there, where the reference stop has made both its tests (after iterations 1 and 11)
THIN = ("wide", "r3-9-20-7", "r2-12-6-13")


def yard_ns(name):
    return tuple(N for N in NS if N != 20) if name in THIN else NS


def routes(name):
    return ("graph", "general") if name in REGULAR else ("general",)


@pytest.mark.parametrize("name", SMALL)
def test_cpu_engine_matches_the_yardstick(name):
    """Scalar p: every stop rule and every N, both routes of a regular code."""
    HX, HZ = matrices(name)
    sX, sZ = inputs(name)
    decs = [serial_cpu(code_of(name, r)) for r in routes(name)]
    for stop in STOPS:
        for N in yard_ns(name):
            for p in (SERIAL_P[name],) + ((SERIAL_P_REF,) if stop == "ref" and N == 11 else ()):
                want = serial_yardstick(HX, HZ, sX, sZ, p, p, N, stop)
                for r, dec in zip(routes(name), decs):
                    got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                    assert_same_decode(got, want, "%s %s %s p=%g N=%d" % (name, r, stop, p, N))
                    assert dec.last_path() == {"serial"}


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("kind", VECTORS)
def test_cpu_engine_matches_the_yardstick_under_priors(name, kind):
    """The prior vectors of test_priors (the special one holds 0, 1/2 and 1); N thinned to 1 and 11 as prior_cases
    does for the regular codes, plus N = 0."""
    HX, HZ = matrices(name)
    sX, sZ = inputs(name)
    pri = prior_vectors(HX.shape[1], kind)
    decs = [serial_cpu(code_of(name, r), pri) for r in routes(name)]
    for stop in STOPS:
        for N in (0, 1, 11):
            want = serial_yardstick(HX, HZ, sX, sZ, pri[0], pri[1], N, stop)
            for r, dec in zip(routes(name), decs):
                got = dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)  # p is not used
                assert_same_decode(got, want, "%s %s %s %s N=%d" % (name, r, kind, stop, N))
    scalar = serial_cpu(code_of(name, routes(name)[0])).decode_batch(sX, sZ, SERIAL_P[name], 11, "fixed", want_q=True)
    assert not same_floats(scalar[4], want[4])  # the priors matter


def iteration_sets(name, stop, p, N=20):
    it = serial_cpu(code_of(name, routes(name)[0])).decode_batch(*inputs(name), p, N, stop, want_iters=True)[3]
    return [set(int(x) for x in it[:, sec]) for sec in (0, 1)]


def test_not_vacuous():
    """On the CPU engine, cap 20: under the syndrome stop every code has a sector with a row that stops at 1 and a
    sector with a row that runs to the cap, and some code ends a sector strictly between; under the reference stop
    at SERIAL_P_REF every code has sectors ending at its first test, and some run to the cap."""
    between, ref_cap = [], []
    for name in SMALL:
        seen = iteration_sets(name, "syndrome", SERIAL_P[name])
        assert any(1 in s for s in seen) and any(20 in s for s in seen), (name, seen)
        between.append(any(1 < k < 20 for s in seen for k in s))
        ref = iteration_sets(name, "ref", SERIAL_P_REF)
        assert any(1 in s for s in ref), (name, ref)
        ref_cap.append(any(20 in s for s in ref))
    assert any(between) and any(ref_cap)
    flags = np.concatenate([serial_cpu(code_of(n, routes(n)[0])).decode_batch(*inputs(n), p, 20, stop)[2] for n in SMALL
                            for stop, p in (("syndrome", SERIAL_P[n]), ("ref", SERIAL_P_REF))])
    assert (flags == 0).any()
    for bit in (q.SYNDROME_FAIL_X, q.SYNDROME_FAIL_Z, q.CONVERGENCE_FAIL_X, q.CONVERGENCE_FAIL_Z):
        assert (flags & bit).any(), bit


def test_unused_slots_and_degree_zero_variables():
    """tall: qubits 0, 1 and 2 are in no X check and decide 0; unused slots of q_final hold +0.0f; every real slot
    of a variable holds the same value."""
    HX, HZ = matrices("tall")
    sX, sZ = inputs("tall")
    eX, _, _, _, qf = serial_cpu(code_of("tall", "general")).decode_batch(sX, sZ, 0.05, 11, "fixed", want_q=True)
    assert not eX[:, :3].any()
    D = 7
    qx = qf[:, :HX.shape[0] * D].reshape(len(sX), HX.shape[0], D)
    for c in range(HX.shape[0]):
        w = int(HX[c].sum())
        assert (qx[:, c, w:].view(np.uint32) == 0).all()
    v = int(np.nonzero(HX.sum(axis=0) > 1)[0][0])
    slots = [(c, int(np.nonzero(np.nonzero(HX[c])[0] == v)[0][0])) for c in np.nonzero(HX[:, v])[0]]
    vals = np.stack([qx[:, c, k] for c, k in slots])
    assert same_floats(vals[0], vals[1])


def test_serial_is_a_different_decode_and_option_0_restores_flooding():
    name = "hgp_ham"
    code = code_of(name, "general")
    sX, sZ = inputs(name)
    row = int(np.nonzero(sX.any(axis=1) & sZ.any(axis=1))[0][0])  # a non-zero syndrome in both sectors
    dec, fresh = q.DecoderCPU(code), q.DecoderCPU(code)
    assert dec.get_option("bp_schedule") == 0
    flood = fresh.decode_batch(sX, sZ, 0.05, 1, "fixed", want_iters=True, want_q=True)
    dec.set_option("bp_schedule", 1)
    assert dec.get_option("bp_schedule") == 1
    serial = dec.decode_batch(sX, sZ, 0.05, 1, "fixed", want_iters=True, want_q=True)
    assert "serial" in dec.last_path()
    EX = code.numEqsX * code.stride
    assert not same_floats(serial[4][row, :EX], flood[4][row, :EX]) and not same_floats(serial[4][row, EX:], flood[4][row, EX:])
    dec.set_option("bp_schedule", 0)
    for N, stop in ((1, "fixed"), (20, "syndrome"), (20, "ref")):
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert "serial" not in dec.last_path()
        assert_same_decode(got, fresh.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True), "option 0 again")


def test_near_hard_option_changes_nothing_under_serial():
    code = code_of("r3-3-6-13", "graph")
    sX, sZ = inputs("r3-3-6-13")
    a, b = serial_cpu(code), serial_cpu(code)
    b.set_option("near_hard", 0)
    for stop in ("fixed", "ref"):
        assert_same_decode(a.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True),
                           b.decode_batch(sX, sZ, 0.005, 20, stop, want_iters=True), stop, with_q=False)


# ---- the SERIAL kernels of bp_sparse.hip, restated -------------------------------------------------------------------
# sparse_kernels / sparse_plan_create: the shape and the workspace are the scalar plan's (plan_of), priors are a runtime
# branch of the one kernel, and the route chooses between the two kernels: 2 kernels x 3 shapes x LDS / HBM x 3 stops
SERIAL_INSTANCES = {(k, s, mem, stop) for k in KERNELS for s in SHAPES for mem in ("lds", "hbm") for stop in STOPS}
GPU_CASES = CASES  # the case table of tests/test_gpu_serial.py: every row, scalar p and priors, every stop rule


def serial_instance_of(code, general, stop):
    p = plan_of(code, general)
    return (p["kernel"], p["shape"], p["mem"], stop)


def test_gpu_case_table_reaches_every_serial_instantiation():
    reached = {serial_instance_of(code_of(name, route), route == "general", stop) for name, route in GPU_CASES
               for stop in STOPS}
    assert len(SERIAL_INSTANCES) == 36
    assert reached == SERIAL_INSTANCES, sorted(SERIAL_INSTANCES - reached)


# ---- the option --------------------------------------------------------------------------------------------------------
def test_option_values_and_refusals():
    code = code_of("hgp_ham", "general")
    dec = q.DecoderCPU(code)
    assert q.OPTION["bp_schedule"] == 18 and q.PATH["serial"] == 1024 and q.lib().qec_abi_version() == 4
    for bad in (2, -1):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_SCHEDULE"):
            dec.set_option("bp_schedule", bad)
        assert q.lib().qec_decoder_set_option(dec._h, 18, bad) == -1  # QEC_ERR_ARG
        assert dec.get_option("bp_schedule") == 0
    # correlated first: the schedule is refused, the handle unchanged
    dec.set_option("correlated", 1)
    with pytest.raises(q.QecError, match="QEC_OPT_CORRELATED"):
        dec.set_option("bp_schedule", 1)
    assert q.lib().qec_decoder_set_option(dec._h, 18, 1) == -4  # QEC_ERR_UNSUPPORTED
    assert dec.get_option("bp_schedule") == 0 and dec.get_option("correlated") == 1
    dec.set_option("bp_schedule", 0)  # flooding is always accepted
    # the schedule first: the correlated form is refused, the handle unchanged
    dec.set_option("correlated", 0)
    dec.set_option("bp_schedule", 1)
    for v in (1, 2):
        with pytest.raises(q.QecError, match="QEC_OPT_BP_SCHEDULE"):
            dec.set_option("correlated", v)
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["correlated"], v) == -4
    assert dec.get_option("bp_schedule") == 1 and dec.get_option("correlated") == 0
    dec.set_option("correlated", 0)
    sX, sZ = inputs("hgp_ham")
    assert_same_decode(dec.decode_batch(sX, sZ, 0.05, 5, "fixed", want_iters=True, want_q=True),
                       serial_cpu(code).decode_batch(sX, sZ, 0.05, 5, "fixed", want_iters=True, want_q=True), "after refusals")


# ---- OSD and the benefit on hgp_ham ------------------------------------------------------------------------------------
BENEFIT_SEED, BENEFIT_B, BENEFIT_P = 0x51EC0DE, 2048, 0.02


def benefit_samples():
    HX, HZ = code_matrices("hgp_ham")
    x, z = depolarizing(BENEFIT_SEED, 0, BENEFIT_B, HX.shape[1], BENEFIT_P)
    return x, z, ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)


def test_serial_halves_the_syndrome_failures_on_hgp_ham():
    """2048 depolarising samples of the project's sampler at p = 0.02, syndrome stop, cap 20: the samples with a
    SYNDROME_FAIL bit under the serial schedule are at most half of those under flooding."""
    _, _, sX, sZ = benefit_samples()
    code = general_code("hgp_ham")
    flood = q.DecoderCPU(code).decode_batch(sX, sZ, BENEFIT_P, 20, "syndrome", want_iters=True)
    serial = serial_cpu(code).decode_batch(sX, sZ, BENEFIT_P, 20, "syndrome", want_iters=True)
    nf, ns = int(((flood[2] & 3) != 0).sum()), int(((serial[2] & 3) != 0).sum())
    print("hgp_ham p=%g: failed samples flooding %d, serial %d; iterations %d / %d"
          % (BENEFIT_P, nf, ns, int(flood[3].sum()), int(serial[3].sum())))
    assert nf > 0 and 2 * ns <= nf, (nf, ns)


@pytest.mark.parametrize("lam", [0, 10])
def test_osd_soft_decode_is_serial(lam):
    """osd = 1 under the serial schedule: no syndrome failure remains, and the result is dec.osd fed with the
    q_final of a serial fixed-stop decode of osd_iterations iterations."""
    HX, HZ = code_matrices("hgp_ham")
    p = 0.05
    x, z = depolarizing(BENEFIT_SEED, 0, 512, HX.shape[1], p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    code = general_code("hgp_ham")
    dec = serial_cpu(code)
    dec.set_option("osd_order", lam)
    main = dec.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    failed = int(((main[2] & 1) != 0).sum() + ((main[2] & 2) != 0).sum())
    assert failed >= 10
    K = dec.get_option("osd_iterations")
    soft = dec.decode_batch(sX, sZ, p, K, "fixed", want_q=True)[4]
    flood_soft = q.DecoderCPU(code).decode_batch(sX, sZ, p, K, "fixed", want_q=True)[4]
    assert not same_floats(soft, flood_soft)
    want = dec.osd(sX, sZ, soft, main[0], main[1], main[2])
    dec.set_option("osd", 1)
    got = dec.decode_batch(sX, sZ, p, 20, "syndrome", want_iters=True)
    assert dec.last_path() == {"serial", "osd"}
    for a, b in zip(got[:3], want):
        assert np.array_equal(a, b)
    assert np.array_equal(got[3], main[3])
    assert not (got[2] & 3).any() and dec.get_option("osd_sectors") == failed
    assert np.array_equal((got[0] @ HX.T) & 1, sX) and np.array_equal((got[1] @ HZ.T) & 1, sZ)


# ---- CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_bp_schedule_on_the_cpu_engine(tmp_path):
    """--bp-schedule serial reproduces the Python counters of GetStatistics under option 1; flooding those under 0;
    other values and --correlated beside it are refused."""
    from qec_ldpc_amd.codes import write_css_file
    from test_osd_host import _cli, _fields
    HX, HZ = code_matrices("hgp_ham")
    path = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    code = q.Quantum_LDPC_Code.createFromFile(path).with_logical("degenerate")
    W, B, N, p, seed = 4, 1500, 20, 0.05, 7
    base = ["--engine", "cpu", "--seed", str(seed), "--logical", "degenerate"]
    keys = {"Corrected": "corrected", "Syndrome Errors X": "syndromeErrorsX", "Syndrome Errors Z": "syndromeErrorsZ",
            "Logical Errors": "logicalErrors", "Convergence Fail X": "convergenceFailX",
            "Convergence Fail Z": "convergenceFailZ", "Errors Tested": "numErrorsTested"}
    out = {}
    for sched in ("flooding", "serial"):
        d = tmp_path / sched
        d.mkdir()
        r = _cli(d, base + ["--bp-schedule", sched], path, "%d %d %d %d %g" % (W, W, B, N, p))
        assert r.returncode == 0, r.stderr
        f = _fields(d)
        dec = q.DecoderCPU(code)
        dec.set_option("bp_schedule", q.BP_SCHEDULE[sched])
        tested = int(f["Errors Tested"])  # the CLI tests (B / threads) * threads samples, the first ones of the stream
        assert B // 2 < tested <= B
        st = dec.GetStatistics(W, tested, p, N, seed=seed)
        out[sched] = {k: int(f[k]) for k in keys}
        assert out[sched] == {k: st[v] for k, v in keys.items()}, sched
    assert out["serial"] != out["flooding"]
    for flags in (["--bp-schedule", "layered"], ["--bp-schedule", "serial", "--correlated", "xz"]):
        d = tmp_path / ("bad%d" % len(flags))
        d.mkdir()
        assert _cli(d, base + flags, path, "4 4 10 20 0.05").returncode == 2

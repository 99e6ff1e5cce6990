"""General CSS codes (qec_code_from_matrices): the code model, the CPU engine and OSD on codes whose
checks and qubits have their own degrees -- against a numpy float32 restatement of DESIGN.md section 2
that is first validated, bit for bit, against the oracle on regular codes."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import write_code_file, write_css_file
from qec_ldpc_amd.synthetic import depolarizing_errors
from test_osd_cs_host import YardstickCS
from test_osd_host import _cli, _fields, gf2_rank

G13 = (3, 3, 6, 13, 3, 2)
STOPS = ("ref", "fixed", "syndrome")
NS = (0, 1, 2, 11, 20)
F32 = np.float32

REP3 = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)


def hgp(H1, H2):
    """HX = [H1 (x) I | I (x) H2^T], HZ = [I (x) H2 | H1^T (x) I]."""
    m1, n1 = H1.shape
    m2, n2 = H2.shape
    eye = lambda k: np.eye(k, dtype=np.uint8)  # noqa: E731
    HX = np.concatenate([np.kron(H1, eye(n2)), np.kron(eye(m1), H2.T)], axis=1)
    HZ = np.concatenate([np.kron(eye(n1), H2), np.kron(H1.T, eye(m2))], axis=1)
    return np.ascontiguousarray(HX, dtype=np.uint8), np.ascontiguousarray(HZ, dtype=np.uint8)


def code_matrices(name):
    if name == "surf3":
        return hgp(REP3, REP3)
    if name == "hgp_ham":
        return hgp(HAMMING, HAMMING)
    HX, HZ = hgp(HAMMING, REP3)
    if name == "ham_rep3":
        return HX, HZ
    assert name == "ham_rep3+1"  # one more qubit, in Z check 0 only: an all-zero column of HX
    HX = np.concatenate([HX, np.zeros((HX.shape[0], 1), dtype=np.uint8)], axis=1)
    extra = np.zeros((HZ.shape[0], 1), dtype=np.uint8)
    extra[0, 0] = 1
    return np.ascontiguousarray(HX), np.ascontiguousarray(np.concatenate([HZ, extra], axis=1))


CODES = ("surf3", "hgp_ham", "ham_rep3", "ham_rep3+1")
# n, mX, mZ, row weights X, Z, column weights X, Z (sets)
SHAPES = {
    "surf3": (13, 6, 6, {3, 4}, {3, 4}, {1, 2}, {1, 2}),
    "hgp_ham": (58, 21, 21, {5, 6, 7}, {5, 6, 7}, {1, 2, 3, 4}, {1, 2, 3, 4}),
    "ham_rep3": (27, 9, 14, {5, 6}, {3, 4, 5}, {1, 2, 3}, {1, 2, 4}),
}

_codes = {}


def general_code(name):
    if name not in _codes:
        _codes[name] = q.Quantum_LDPC_Code.createFromMatrices(*code_matrices(name))
    return _codes[name]


# ---- the yardstick: DESIGN.md section 2 in numpy float32 -------------------------------------------
def _outside(x):
    return ~((x > F32(0.01)) & (x < F32(0.99)))


def bp_sector(H, s, p, N, stop, D):
    """One sector of a batch: every float32 operation of section 2 in its stated order, elementwise over
    the batch.  -> (e [B, n], syndrome failed [B], convergence failed [B], iterations [B], q [B, m, D])."""
    m, n = H.shape
    B = s.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]                      # N(c), ascending
    edges = [[(c, int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]  # M(v)
    real = np.zeros((m, D), dtype=bool)
    for c in range(m):
        real[c, :len(nbr[c])] = True
    pp = F32(2.0) / F32(3.0) * F32(p)
    omp = F32(1.0) - pp
    msg = np.where(real, pp, F32(0.0)).astype(F32)[None].repeat(B, axis=0)
    h = np.where(s != 0, F32(0.5), F32(-0.5)).astype(F32)              # truthiness of the syndrome entry
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)

    def decide(msg):
        e = np.zeros((B, n), dtype=np.uint8)
        for v in range(n):
            for c, k in edges[v]:
                e[:, v] |= msg[:, c, k] >= F32(0.5)
        return e

    def syndrome_fails(e):
        bad = np.zeros(B, dtype=bool)
        for c in range(m):
            bad |= (e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) != s[:, c]  # the entry's exact value
        return bad

    def inside_any(msg):
        return (~_outside(msg) & real[None]).any(axis=(1, 2))

    with np.errstate(all="ignore"):
        for it in range(N):
            if not active.any():
                break
            iters += active
            last = it == N - 1
            r = msg.copy()
            for c in range(m):
                dc = len(nbr[c])
                a = [F32(1.0) - F32(2.0) * msg[:, c, k] for k in range(dc)]
                pre = np.ones(B, dtype=F32)
                for i in range(dc):
                    t = pre
                    for k in range(i + 1, dc):
                        t = t * a[k]
                    r[:, c, i] = F32(0.5) + h[:, c] * t
                    pre = pre * a[i]
            new = r.copy()
            for v in range(n):
                g = [r[:, c, k] for c, k in edges[v]]
                bv = [F32(1.0) - x for x in g]
                dv = len(g)
                if last:
                    P0, P1 = np.full(B, omp, dtype=F32), np.full(B, pp, dtype=F32)
                    for k in range(dv):
                        P0, P1 = P0 * bv[k], P1 * g[k]
                    for c, k in edges[v]:
                        new[:, c, k] = P1 / (P0 + P1)
                else:
                    pre0, pre1 = np.full(B, omp, dtype=F32), np.full(B, pp, dtype=F32)
                    for j, (c, k) in enumerate(edges[v]):
                        t0, t1 = pre0, pre1
                        for kk in range(j + 1, dv):
                            t0, t1 = t0 * bv[kk], t1 * g[kk]
                        new[:, c, k] = t1 / (t0 + t1)
                        pre0, pre1 = pre0 * bv[j], pre1 * g[j]
            msg = np.where(active[:, None, None], new, msg)
            if stop == "ref" and it % 10 == 0:
                active &= inside_any(msg)
            elif stop == "syndrome":
                active &= syndrome_fails(decide(msg))
    e = decide(msg)
    return e, syndrome_fails(e), inside_any(msg), iters, msg


def bp_yardstick(HX, HZ, sX, sZ, p, N, stop):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D])."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fx, cx, ix, qx = bp_sector(HX, sX, p, N, stop, D)
    eZ, fz, cz, iz, qz = bp_sector(HZ, sZ, p, N, stop, D)
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32)


def same_floats(a, b):
    """Equal as bit patterns, except that any NaN matches any NaN."""
    a, b = np.asarray(a, dtype=F32).ravel(), np.asarray(b, dtype=F32).ravel()
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_same_decode(got, want, what, with_q=True):
    for a, b, name in zip(got[:4], want[:4], ("eX", "eZ", "flags", "iters")):
        assert np.array_equal(a, b), "%s: %s differs" % (what, name)
    if with_q:
        assert same_floats(got[4], want[4]), "%s: final messages differ" % what


def mixed_syndromes(H, seed, B, ps):
    """B - 3 sampled syndromes over the error rates `ps`, then an all-zero row, an all-one row and a row
    with an entry > 1."""
    HX, HZ = H
    n = HX.shape[1]
    rows = []
    per = (B - 3 + len(ps) - 1) // len(ps)
    for k, p in enumerate(ps):
        x, z = depolarizing_errors(n, seed + k, per, p)
        rows.append(((x @ HX.T) & 1, (z @ HZ.T) & 1))
    sX = np.concatenate([r[0] for r in rows])[:B - 3].astype(np.uint8)
    sZ = np.concatenate([r[1] for r in rows])[:B - 3].astype(np.uint8)
    tail = lambda m: np.stack([np.zeros(m), np.ones(m), np.r_[2, np.ones(m - 1)]]).astype(np.uint8)  # noqa: E731
    return np.concatenate([sX, tail(HX.shape[0])]), np.concatenate([sZ, tail(HZ.shape[0])])


def decode_inputs(name):
    """The suite's decode inputs for a test code: 48 depolarising syndromes at p = 0.05 and the three
    special rows."""
    return mixed_syndromes(code_matrices(name), 4242, 51, (0.05,))


_yard = {}


def yardstick(name, stop, N, p=0.05):
    """bp_yardstick on decode_inputs(name), computed once per session."""
    key = (name, stop, N, p)
    if key not in _yard:
        HX, HZ = code_matrices(name)
        _yard[key] = bp_yardstick(HX, HZ, *decode_inputs(name), p, N, stop)
    return _yard[key]


@pytest.fixture(scope="module")
def regular(code_paths, tmp_path_factory):
    """P7 and G13: (file code, oracle, the same code from its matrices)."""
    tmp = tmp_path_factory.mktemp("general_regular")
    g = q.QC_LDPC_CSS(*G13)
    gpath = write_code_file(str(tmp / "g13.txt"), *G13, g.pcm(0), g.pcm(1))
    out = {}
    for key, path in (("P7", code_paths["P7"]), ("G13", gpath)):
        code = q.Quantum_LDPC_Code.createFromFile(path)
        out[key] = (code, OracleCode(path), q.Quantum_LDPC_Code.createFromMatrices(code.pcm(0), code.pcm(1)))
    return out


# ---- the yardstick is the oracle on regular codes ----------------------------------------------------
@pytest.mark.parametrize("key", ["P7", "G13"])
@pytest.mark.parametrize("stop", STOPS)
def test_yardstick_matches_oracle(regular, key, stop):
    code, orc, _ = regular[key]
    H = (code.pcm(0), code.pcm(1))
    sX, sZ = mixed_syndromes(H, 99, 64, (0.02, 0.05, 0.15))
    for N in NS:
        want = orc.decode_batch(sX, sZ, 0.05, N, stop, want_q=True)
        assert_same_decode(bp_yardstick(*H, sX, sZ, 0.05, N, stop), want, "%s %s N=%d" % (key, stop, N))


# ---- CPU engine -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("stop", STOPS)
def test_cpu_engine_matches_yardstick(name, stop):
    dec = q.DecoderCPU(general_code(name))
    sX, sZ = decode_inputs(name)
    for N in NS:
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, yardstick(name, stop, N), "%s %s N=%d" % (name, stop, N))


@pytest.mark.parametrize("name", CODES)
def test_unused_slots_are_plus_zero(name):
    code = general_code(name)
    HX, HZ = code_matrices(name)
    D = code.degrees()[4]
    w = np.concatenate([HX.sum(axis=1), HZ.sum(axis=1)])
    unused = np.arange(D)[None, :] >= w[:, None]
    assert unused.any()
    qf = q.DecoderCPU(code).decode_batch(*decode_inputs(name), 0.05, 11, "fixed", want_q=True)[4]
    bits = qf.view(np.uint32).reshape(len(qf), len(w), D)
    assert not bits[:, unused].any()


@pytest.mark.parametrize("key", ["P7", "G13"])
@pytest.mark.parametrize("stop", STOPS)
def test_regular_code_from_matrices_equals_file_code_and_oracle(regular, key, stop):
    code, orc, gen = regular[key]
    assert gen.degrees() == code.degrees() == (code.L, code.L, code.J, code.K, code.L)
    sX, sZ = mixed_syndromes((code.pcm(0), code.pcm(1)), 7, 64, (0.02, 0.08))
    for N in (0, 1, 11, 20):
        want = orc.decode_batch(sX, sZ, 0.05, N, stop, want_q=True)
        a = q.DecoderCPU(gen).decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        b = q.DecoderCPU(code).decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert_same_decode(a, want, "%s from matrices, %s N=%d" % (key, stop, N))
        assert_same_decode(b, want, "%s from its file, %s N=%d" % (key, stop, N))


# ---- code model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CODES)
def test_code_model(name):
    HX, HZ = code_matrices(name)
    assert not ((HX.astype(int) @ HZ.T) & 1).any()  # the checks commute
    code = general_code(name)
    assert np.array_equal(code.pcm(0), HX) and np.array_equal(code.pcm(1), HZ)
    assert (code.J, code.K, code.L, code.P, code.sigma, code.tau) == (0,) * 6
    assert (code.n, code.numEqsX, code.numEqsZ) == (HX.shape[1], HX.shape[0], HZ.shape[0])
    rw = (int(HX.sum(axis=1).max()), int(HZ.sum(axis=1).max()))
    assert code.degrees() == rw + (int(HX.sum(axis=0).max()), int(HZ.sum(axis=0).max()), max(rw))
    k = code.n - gf2_rank(HX) - gf2_rank(HZ)
    assert code.describe() == "[[n=%d,k=%d]]" % (code.n, k)
    with pytest.raises(q.QecError):
        code.exponents(0)
    if name in SHAPES:
        n, mX, mZ, rX, rZ, cX, cZ = SHAPES[name]
        assert (code.n, code.numEqsX, code.numEqsZ) == (n, mX, mZ)
        assert set(HX.sum(axis=1)) == rX and set(HZ.sum(axis=1)) == rZ
        assert set(HX.sum(axis=0)) == cX and set(HZ.sum(axis=0)) == cZ
    else:
        assert not HX[:, -1].any() and HZ[:, -1].sum() == 1  # the all-zero column is allowed
    x, z = depolarizing_errors(code.n, 5, 16, 0.2)
    assert np.array_equal(code.syndrome(0, x), (x @ HX.T) & 1)
    assert np.array_equal(code.syndrome(1, z), (z @ HZ.T) & 1)


def test_k_of_the_test_codes():
    assert general_code("surf3").describe() == "[[n=13,k=1]]"
    assert general_code("hgp_ham").describe() == "[[n=58,k=16]]"


def test_refusals():
    HX, HZ = code_matrices("surf3")
    bad = HX.copy()
    bad[2, 5] = 2
    with pytest.raises(q.QecError, match=r"HX\[2\]\[5\]"):
        q.Quantum_LDPC_Code.createFromMatrices(bad, HZ)
    wide = HZ.astype(np.int32)
    wide[1, 0] = 256  # would fold to 0 as a byte
    with pytest.raises(q.QecError, match=r"HZ\[1\]\[0\]"):
        q.Quantum_LDPC_Code.createFromMatrices(HX, wide)
    zero = HZ.copy()
    zero[4] = 0
    with pytest.raises(q.QecError, match="row 4 of HZ"):
        q.Quantum_LDPC_Code.createFromMatrices(HX, zero)
    with pytest.raises(q.QecError):
        q.Quantum_LDPC_Code.createFromMatrices(HX[:0], HZ)
    with pytest.raises(q.QecError):
        q.Quantum_LDPC_Code.createFromMatrices(HX[:, :0], HZ[:, :0])
    # the C entry point itself: bytes > 1, and sizes
    L = q.lib()
    raw = np.ascontiguousarray(bad)
    assert not L.qec_code_from_matrices(13, 6, q._ptr(raw), 6, q._ptr(HZ))
    assert "HX[2][5]" in q.last_error()
    for n, mX, mZ in ((0, 6, 6), (13, 0, 6), (13, 6, -1)):
        assert not L.qec_code_from_matrices(n, mX, q._ptr(HX), mZ, q._ptr(HZ))
        assert "must be > 0" in q.last_error()


@pytest.mark.parametrize("name", ["hgp_ham", "ham_rep3+1"])
def test_css_file_round_trip(tmp_path, name):
    HX, HZ = code_matrices(name)
    code = q.Quantum_LDPC_Code.createFromFile(write_css_file(str(tmp_path / "c.txt"), HX, HZ))
    assert np.array_equal(code.pcm(0), HX) and np.array_equal(code.pcm(1), HZ)
    assert code.describe() == general_code(name).describe() and code.degrees() == general_code(name).degrees()
    assert code.logical_rows == 0
    imp = general_code(name).with_logical("degenerate").imp()
    code = q.Quantum_LDPC_Code.createFromFile(write_css_file(str(tmp_path / "d.txt"), HX, HZ, imp))
    assert np.array_equal(code.imp(), imp)
    with open(str(tmp_path / "e.txt"), "w") as f:
        f.write("css 13 6\n")
    with pytest.raises(q.QecError, match="css n mX mZ"):
        q.Quantum_LDPC_Code.createFromFile(str(tmp_path / "e.txt"))
    with open(str(tmp_path / "f.txt"), "w") as f:  # sizes no file of that length could back: refused from the header
        f.write("css 1048576 1048576 6\n1\n1\n")
    with pytest.raises(q.QecError, match="out of range"):
        q.Quantum_LDPC_Code.createFromFile(str(tmp_path / "f.txt"))


def gf2_kernel_dim(H):
    return H.shape[1] - gf2_rank(H)


def test_degenerate_logical_rows_of_hgp_ham():
    """The derived check's rows are bases of ker HZ (x half) and ker HX (z half): (n - rank HZ) +
    (n - rank HX) = 2n - rank HX - rank HZ non-zero rows."""
    HX, HZ = code_matrices("hgp_ham")
    code = general_code("hgp_ham").with_logical("degenerate")
    assert code.logical_mode == "degenerate"
    assert code.logical_rows == gf2_kernel_dim(HZ) + gf2_kernel_dim(HX) == 2 * code.n - gf2_rank(HX) - gf2_rank(HZ)
    # a stabilizer is no logical error, a residual outside the row space with zero syndrome is one
    zero = np.zeros(code.n, dtype=np.uint8)
    assert not code.check_logical(HZ[3], zero)[0] and not code.check_logical(zero, HX[5])[0]
    assert code.describe() == "[[n=58,k=16]]" and code.degrees() == general_code("hgp_ham").degrees()


def test_irregular_matrix_in_a_six_number_file_is_still_refused(tmp_path):
    """The J K L P sigma tau header keeps its meaning: such a code must be regular for the sparse tables."""
    g = q.QC_LDPC_CSS(3, 3, 6, 7, 2, 3)
    HX = g.pcm(0).copy()
    HX[0, np.nonzero(HX[0])[0][0]] = 0
    code = q.Quantum_LDPC_Code.createFromFile(write_code_file(str(tmp_path / "i.txt"), 3, 3, 6, 7, 2, 3, HX, g.pcm(1)))
    assert (code.L, code.n) == (6, 42)
    with pytest.raises(q.QecError, match="irregular"):
        q.DecoderCPU(code)


# ---- OSD on the CPU engine --------------------------------------------------------------------------------
class GeneralOsdYardstick(YardstickCS):
    """DESIGN.md sections 1.2 / 1.3 in numpy (test_osd_host / test_osd_cs_host) for the general layout:
    slot stride D, and a variable in no check of the sector takes the key of `absent` (0.5)."""

    absent = F32(0.5)

    def __init__(self, HX, HZ):
        self.n = HX.shape[1]
        self.L = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
        self.H = [HX, HZ]
        self.rank = [gf2_rank(h) for h in self.H]
        self.qn = (HX.shape[0] + HZ.shape[0]) * self.L
        self.pos = []
        base = 0
        for H in self.H:
            pos = np.full(self.n, self.qn, dtype=np.int64)  # qn: the appended value
            for v in range(self.n):
                cs = np.nonzero(H[:, v])[0]
                if len(cs):
                    pos[v] = base + int(cs[0]) * self.L + int(H[cs[0], :v].sum())
            self.pos.append(pos)
            base += H.shape[0] * self.L

    def reduce(self, sec, s, qrow):
        return super().reduce(sec, s, np.append(qrow, self.absent))


OSD_P, OSD_N, OSD_B = 0.08, 20, 256
_osd = {}


def osd_case(name):
    """The OSD batch of a test code: syndromes, the yardstick's syndrome-stop decode, its 3-iteration
    soft decode and the numpy repair for lambda 0 and 10."""
    if name not in _osd:
        HX, HZ = code_matrices(name)
        x, z = depolarizing_errors(HX.shape[1], 777, OSD_B, OSD_P)
        sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
        main = bp_yardstick(HX, HZ, sX, sZ, OSD_P, OSD_N, "syndrome")
        soft = bp_yardstick(HX, HZ, sX, sZ, OSD_P, 3, "fixed")[4]
        ys = GeneralOsdYardstick(HX, HZ)
        rep = ys.repair_cs(sX, sZ, soft, main[0], main[1], main[2], (0, 10))
        _osd[name] = (sX, sZ, main, soft, rep)
    return _osd[name]


def failed_sectors(flags):
    return int(np.sum((flags & 1) != 0) + np.sum((flags & 2) != 0))


@pytest.mark.parametrize("name", ["hgp_ham", "ham_rep3+1"])
def test_cpu_osd_matches_numpy(name):
    """p = 0.08, N = 20, B = 256 leaves 312 failed sectors on hgp_ham and 141 on ham_rep3+1 (the yardstick's
    count; at least 20 are asserted)."""
    sX, sZ, main, soft, rep = osd_case(name)
    assert failed_sectors(main[2]) >= 20
    dec = q.DecoderCPU(general_code(name))
    for lam in (0, 10):
        want = rep[lam]
        # the stage as a call on decoded data
        dec.set_option("osd", 0)
        dec.set_option("osd_order", lam)
        eX, eZ, fl = dec.osd(sX, sZ, soft, main[0], main[1], main[2])
        assert np.array_equal(eX, want[0]) and np.array_equal(eZ, want[1]) and np.array_equal(fl, want[2])
        assert dec.get_option("osd_sectors") == want[3] and dec.get_option("osd_cs_sectors") == want[4]
        # and behind the decode
        dec.set_option("osd", 1)
        got = dec.decode_batch(sX, sZ, OSD_P, OSD_N, "syndrome", want_iters=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[3], main[3])
        assert dec.get_option("osd_sectors") == want[3] == failed_sectors(main[2])
        assert not (got[2] & 3).any()  # every sampled syndrome is consistent
        assert np.array_equal((got[0] @ code_matrices(name)[0].T) & 1, sX)
        assert np.array_equal((got[1] @ code_matrices(name)[1].T) & 1, sZ)


# ---- CLI ---------------------------------------------------------------------------------------------------
def test_cli_takes_a_css_file_on_the_cpu_engine(tmp_path):
    HX, HZ = code_matrices("hgp_ham")
    path = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    line = "4 4 1500 20 0.05"
    a, b = tmp_path / "off", tmp_path / "on"
    a.mkdir()
    b.mkdir()
    base = ["--engine", "cpu", "--seed", "7", "--logical", "degenerate"]
    r = _cli(a, base, path, line)
    assert r.returncode == 0, r.stderr
    r = _cli(b, base + ["--osd", "0", "--osd-order", "10"], path, line)
    assert r.returncode == 0, r.stderr
    off, on = _fields(a), _fields(b)
    assert int(off["Errors Tested"]) == int(on["Errors Tested"]) > 0
    assert int(off["Syndrome Errors X"]) + int(off["Syndrome Errors Z"]) > 0
    assert int(on["Syndrome Errors X"]) == 0 and int(on["Syndrome Errors Z"]) == 0
    assert int(on["Corrected"]) + int(on["Logical Errors"]) == int(on["Errors Tested"])

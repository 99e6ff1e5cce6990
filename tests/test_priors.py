"""Per-qubit priors (qec_decoder_set_priors) on the CPU engine: the prior form of DESIGN.md section 2 against a
numpy float32 restatement (bp_sector of test_general_code.py with pp and omp as per-variable arrays), the
uniform-prior and clearing identities, validation, OSD behind a decode with priors, and the numpy restatement of
the independent sampler that tests/test_gpu_priors.py holds the device to."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import MASK, philox4x32_10
from qec_ldpc_amd.codes import P7, P61, code_path
from test_general_code import (G13, NS, STOPS, _outside, assert_same_decode, code_matrices, decode_inputs, general_code,
                               mixed_syndromes, same_floats)

F32 = np.float32
PRIOR_CODES = ("surf3", "hgp_ham", "ham_rep3+1", "G13")
VECTORS = ("random", "special")
INDEP_SALT = 0x51ED270B  # include/qec_ldpc.h, qec_sample_independent_dev (kIndepSalt of qec_mc.h)


# ---- the test codes and their inputs ---------------------------------------------------------------------
_reg = {}
REGULAR = ("G13", "P7", "P61")


def matrices(name):
    """(HX, HZ); G13 is the generated n = 78 regular code, P7 / P61 the shipped code files."""
    if name in REGULAR:
        if name not in _reg:
            g = q.QC_LDPC_CSS(*G13) if name == "G13" else q.Quantum_LDPC_Code.createFromFile(code_path({"P7": P7, "P61": P61}[name]))
            _reg[name] = (g, g.pcm(0), g.pcm(1))
        return _reg[name][1:]
    return code_matrices(name)


def code_of(name):
    """G13, P7 and P61 as REGULAR codes (decode_sector / bp_sparse_kernel), the others as general codes."""
    if name in REGULAR:
        matrices(name)
        return _reg[name][0]
    return general_code(name)


def inputs(name):
    """The 51 rows of decode_inputs (48 depolarising syndromes at p = 0.05 and the three special rows)."""
    if name in REGULAR:
        return mixed_syndromes(matrices(name), 4242, 51, (0.05,))
    return decode_inputs(name)


def prior_vectors(n, kind, seed=20240611):
    """(priorX, priorZ): log-uniform in [0.003, 0.25] from a fixed numpy seed; "special": three entries per
    sector overwritten by 0.0, 0.5 and 1.0."""
    rng = np.random.default_rng(seed + n)
    out = []
    for _ in range(2):
        pr = np.exp(rng.uniform(np.log(0.003), np.log(0.25), n)).astype(F32)
        pos = rng.choice(n, 3, replace=False)
        if kind == "special":
            pr[pos] = np.array([0.0, 0.5, 1.0], dtype=F32)
        else:
            assert kind == "random"
        out.append(pr)
    return out[0], out[1]


# ---- the yardstick: the prior form of DESIGN.md section 2 in numpy float32 -----------------------------------
def bp_sector_priors(H, s, prior, N, stop, D):
    """bp_sector of test_general_code.py with pp and omp as per-variable arrays: the initial message of a real
    slot is its variable's prior and variable v's running products start from 1 - prior[v] and prior[v]."""
    m, n = H.shape
    B = s.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]
    edges = [[(c, int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]
    real = np.zeros((m, D), dtype=bool)
    pp = np.asarray(prior, dtype=F32)
    omp = (F32(1.0) - pp).astype(F32)
    init = np.zeros((m, D), dtype=F32)
    for c in range(m):
        real[c, :len(nbr[c])] = True
        init[c, :len(nbr[c])] = pp[nbr[c]]
    msg = init[None].repeat(B, axis=0)
    h = np.where(s != 0, F32(0.5), F32(-0.5)).astype(F32)
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
            bad |= (e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) != s[:, c]
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
                    P0, P1 = np.full(B, omp[v], dtype=F32), np.full(B, pp[v], dtype=F32)
                    for k in range(dv):
                        P0, P1 = P0 * bv[k], P1 * g[k]
                    for c, k in edges[v]:
                        new[:, c, k] = P1 / (P0 + P1)
                else:
                    pre0, pre1 = np.full(B, omp[v], dtype=F32), np.full(B, pp[v], dtype=F32)
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


def bp_yardstick_priors(HX, HZ, sX, sZ, pX, pZ, N, stop):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D])."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fx, cx, ix, qx = bp_sector_priors(HX, sX, pX, N, stop, D)
    eZ, fz, cz, iz, qz = bp_sector_priors(HZ, sZ, pZ, N, stop, D)
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32)


_yard = {}


def yardstick_priors(name, kind, stop, N):
    """bp_yardstick_priors on inputs(name) under prior_vectors(n, kind), computed once per session."""
    key = (name, kind, stop, N)
    if key not in _yard:
        HX, HZ = matrices(name)
        _yard[key] = bp_yardstick_priors(HX, HZ, *inputs(name), *prior_vectors(HX.shape[1], kind), N, stop)
    return _yard[key]


# ---- the independent sampler in numpy ------------------------------------------------------------------------
def prior_threshold(pi):
    """floor(pi 2^32) in double from the float, as an integer that can reach 2^32."""
    return int(float(F32(pi)) * 4294967296.0)


def independent(seed, start, count, pX, pZ):
    """(x, z) uint8 [count, n]: sample b makes Philox calls k = 0, 1, ... with counter (b lo, b hi, k, salt) and
    key (seed lo, seed hi); word 4k + j = output word j of call k; x[v] = word 2v < thrX[v], z[v] = word 2v + 1 <
    thrZ[v]."""
    n = len(pX)
    nc = (n + 1) // 2
    b = (np.arange(count, dtype=np.uint64) + np.uint64(start))[:, None].repeat(nc, axis=1)
    k = np.arange(nc, dtype=np.uint64)[None].repeat(count, axis=0)
    o = philox4x32_10(b & MASK, b >> np.uint64(32), k, np.full(b.shape, INDEP_SALT, np.uint64), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(o, axis=2).reshape(count, 4 * nc).astype(np.int64)  # word 4k + j
    tX = np.array([prior_threshold(p) for p in pX], dtype=np.int64)
    tZ = np.array([prior_threshold(p) for p in pZ], dtype=np.int64)
    x = (words[:, 0:2 * n:2] < tX[None]).astype(np.uint8)
    z = (words[:, 1:2 * n:2] < tZ[None]).astype(np.uint8)
    return x, z


# ---- CPU engine = yardstick ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRIOR_CODES)
@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("kind", VECTORS)
def test_cpu_engine_matches_prior_yardstick(name, stop, kind):
    code = code_of(name)
    dec = q.DecoderCPU(code)
    dec.set_priors(*prior_vectors(code.n, kind))
    sX, sZ = inputs(name)
    for N in NS:
        got = dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True, want_q=True)
        assert_same_decode(got, yardstick_priors(name, kind, stop, N), "%s %s %s N=%d" % (name, kind, stop, N))
        rec, it = dec.decode_batch_packed(sX, sZ, 0.3, N, stop, want_iters=True)  # p is not used
        assert np.array_equal(rec[:, -1], got[2]) and np.array_equal(it, got[3])
        nb = (code.n + 7) // 8
        assert np.array_equal(np.unpackbits(rec[:, :nb], axis=1, bitorder="little")[:, :code.n], got[0])
        assert np.array_equal(np.unpackbits(rec[:, nb:2 * nb], axis=1, bitorder="little")[:, :code.n], got[1])


def test_priors_change_the_decode():
    """The yardstick under the random priors is not the scalar decode (the comparison above is not vacuous)."""
    dec = q.DecoderCPU(code_of("hgp_ham"))
    sX, sZ = inputs("hgp_ham")
    scalar = dec.decode_batch(sX, sZ, 0.05, 11, "fixed", want_q=True)
    assert not same_floats(scalar[4], yardstick_priors("hgp_ham", "random", "fixed", 11)[4])


@pytest.mark.parametrize("name", PRIOR_CODES)
def test_uniform_priors_equal_the_scalar_call_and_clearing_restores_it(name):
    code = code_of(name)
    dec, ref = q.DecoderCPU(code), q.DecoderCPU(code)
    sX, sZ = inputs(name)
    for p in (0.05, 0.003):
        uni = F32(2.0) / F32(3.0) * F32(p)
        for stop in STOPS:
            for N in (0, 1, 11, 20):
                want = ref.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                dec.set_priors(uni, uni)  # a scalar broadcasts
                assert_same_decode(dec.decode_batch(sX, sZ, 0.4, N, stop, want_iters=True, want_q=True), want,
                                   "%s uniform %s N=%d" % (name, stop, N))
                dec.set_priors(None, None)
                assert dec.get_priors() is None
                assert_same_decode(dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True), want,
                                   "%s cleared %s N=%d" % (name, stop, N))


@pytest.mark.parametrize("stop", ["ref", "fixed"])
def test_near_hard_option_changes_nothing_with_priors(stop):
    """G13 is where the CPU engine's jump can fire; with priors it never does, and no output depends on it."""
    code = code_of("G13")
    sX, sZ = inputs("G13")
    outs = []
    for near in (1, 0):
        dec = q.DecoderCPU(code)
        dec.set_option("near_hard", near)
        dec.set_priors(*prior_vectors(code.n, "random"))
        outs.append([dec.decode_batch(sX, sZ, 0.05, N, stop, want_iters=True) for N in (11, 20, 50)])
    for a, b in zip(*outs):
        assert_same_decode(a, b, "near_hard on / off", with_q=False)
    for got, N in zip(outs[0][:2], (11, 20)):
        assert_same_decode(got, yardstick_priors("G13", "random", stop, N), "near_hard on", with_q=False)


# ---- validation ------------------------------------------------------------------------------------------------------
def test_validation_and_round_trip():
    code = code_of("hgp_ham")
    n = code.n
    dec = q.DecoderCPU(code)
    assert dec.get_priors() is None
    pX, pZ = prior_vectors(n, "special")
    dec.set_priors(pX, pZ)
    gX, gZ = dec.get_priors()
    assert same_floats(gX, pX) and same_floats(gZ, pZ)
    for bad in (-0.1, 1.5, float("nan")):
        for sec, idx in (("X", 0), ("Z", 17), ("Z", n - 1)):
            a, b = pX.copy(), pZ.copy()
            (a if sec == "X" else b)[idx] = bad
            with pytest.raises(q.QecError, match=r"prior%s\[%d\]" % (sec, idx)):
                dec.set_priors(a, b)
    gX, gZ = dec.get_priors()  # a refused call leaves the priors as they were
    assert same_floats(gX, pX) and same_floats(gZ, pZ)
    for a, b in ((pX[:-1], pZ), (pX, np.r_[pZ, F32(0.1)])):
        with pytest.raises(q.QecError, match="length n = %d" % n):
            dec.set_priors(a, b)
    with pytest.raises(q.QecError, match="both"):
        dec.set_priors(pX, None)
    # the C entry point itself: exactly one NULL
    L = q.lib()
    assert L.qec_decoder_set_priors(dec._h, q._ptr(pX), None) != 0
    assert "priorX and priorZ" in q.last_error()
    assert L.qec_decoder_set_priors(dec._h, None, q._ptr(pZ)) != 0
    assert dec.get_priors() is not None
    dec.set_priors(None, None)
    assert dec.get_priors() is None
    dec.set_priors(0.0, 1.0)  # the ends are legal
    gX, gZ = dec.get_priors()
    assert not gX.any() and (gZ == 1).all()


# ---- OSD behind a decode with priors -------------------------------------------------------------------------------
def test_cpu_osd_with_priors():
    """osd = 1 with lambda 0 and 10: every repaired sector satisfies its syndrome, and the result is dec.osd fed
    with the q_final of a fixed-stop osd_iterations decode under the same priors."""
    name, p, N, B = "hgp_ham", 0.08, 20, 256
    HX, HZ = code_matrices(name)
    code = general_code(name)
    pX, pZ = prior_vectors(code.n, "random")
    x, z = independent(777, 0, B, np.minimum(pX * F32(2), F32(1)), np.minimum(pZ * F32(2), F32(1)))
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    dec = q.DecoderCPU(code)
    dec.set_priors(pX, pZ)
    main = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
    failed = int(np.sum((main[2] & 1) != 0) + np.sum((main[2] & 2) != 0))
    assert failed >= 20
    soft = dec.decode_batch(sX, sZ, p, dec.get_option("osd_iterations"), "fixed", want_q=True)[4]
    scalar_soft = q.DecoderCPU(code).decode_batch(sX, sZ, p, 3, "fixed", want_q=True)[4]
    assert not same_floats(soft, scalar_soft)
    for lam in (0, 10):
        dec.set_option("osd", 0)
        dec.set_option("osd_order", lam)
        want = dec.osd(sX, sZ, soft, main[0], main[1], main[2])
        dec.set_option("osd", 1)
        got = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
        for a, b in zip(got[:3], want):
            assert np.array_equal(a, b), lam
        assert np.array_equal(got[3], main[3])
        assert dec.get_option("osd_sectors") == failed
        assert not (got[2] & 3).any()
        assert np.array_equal((got[0] @ HX.T) & 1, sX) and np.array_equal((got[1] @ HZ.T) & 1, sZ)


# ---- the sampler's restatement ----------------------------------------------------------------------------------------
def test_independent_restatement_threshold_edges():
    assert prior_threshold(0.0) == 0 and prior_threshold(1.0) == 1 << 32
    assert prior_threshold(F32(2.0) ** -32) == 1 and prior_threshold(0.5) == 1 << 31
    n, B = 13, 4096
    pX = np.full(n, 0.0, dtype=F32)
    pZ = np.full(n, 1.0, dtype=F32)
    pX[3], pZ[5] = 1.0, 0.0
    pX[7] = pZ[7] = F32(2.0) ** -32  # thr = 1: hits only a word that is 0
    pX[9] = 0.5
    x, z = independent(99, (1 << 32) - 64, B, pX, pZ)
    assert x[:, 3].all() and not x[:, [0, 1, 2, 4, 5, 6, 8, 10, 11, 12]].any()
    assert not z[:, 5].any() and z[:, [0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12]].all()
    assert not x[:, 7].any() and not z[:, 7].any()
    assert abs(int(x[:, 9].sum()) - B // 2) < 5 * 32  # sigma = sqrt(B) / 2 = 32
    # any shard can be drawn alone, and the samples do not depend on the batch
    a = independent(99, (1 << 32) - 64, 128, pX, pZ)
    b = independent(99, (1 << 32) - 64 + 100, 28, pX, pZ)
    assert np.array_equal(a[0], x[:128]) and np.array_equal(b[0], x[100:128]) and np.array_equal(b[1], z[100:128])


# ---- CLI ---------------------------------------------------------------------------------------------------
def _write_priors(path, pX, pZ):
    path.write_text("\n".join(" ".join("%.9g" % v for v in pr) for pr in (pX, pZ)) + "\n")
    return str(path)


def test_cli_priors_on_the_cpu_engine(tmp_path):
    """--priors FILE: the uniform vector gives the counters of the scalar run, a biased one does not, and a
    file of the wrong length is refused."""
    from qec_ldpc_amd.codes import write_css_file
    from test_osd_host import _cli, _fields
    HX, HZ = code_matrices("hgp_ham")
    n = HX.shape[1]
    code = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    line = "4 4 1500 20 0.05"
    base = ["--engine", "cpu", "--seed", "7", "--logical", "degenerate"]
    uni = np.full(n, F32(2.0) / F32(3.0) * F32(0.05), dtype=F32)
    runs = {"scalar": [], "uniform": ["--priors", _write_priors(tmp_path / "u.txt", uni, uni)],
            "biased": ["--priors", _write_priors(tmp_path / "b.txt", *prior_vectors(n, "random"))]}
    out = {}
    for key, flags in runs.items():
        d = tmp_path / key
        d.mkdir()
        r = _cli(d, base + flags, code, line)
        assert r.returncode == 0, r.stderr
        out[key] = {k: v for k, v in _fields(d).items() if not k.startswith("Duration")}
    assert out["uniform"] == out["scalar"]
    assert out["biased"] != out["scalar"]
    d = tmp_path / "short"
    d.mkdir()
    r = _cli(d, base + ["--priors", _write_priors(tmp_path / "s.txt", uni[:-1], uni)], code, line)
    assert r.returncode == 1 and "n = %d" % n in r.stderr

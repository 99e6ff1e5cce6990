"""The correlated form (QEC_OPT_CORRELATED) and the per-qubit Pauli channel on the CPU engine:
the yardstick (bp_sector_priors of test_priors.py restated with the prior as a [B, n] array, composed as decode F,
build pi from F's estimate and the tables, decode S), the conditional tables against a numpy double restatement,
the identities, validation, the CLI, and the numpy restatement of the Pauli sampler that
tests/test_gpu_correlated.py holds the device to.

Every comparison is bit for bit (q_final as uint32 patterns).  There is no tolerance."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import MASK, philox4x32_10
from test_general_code import NS, STOPS, _outside, assert_same_decode, code_matrices, same_floats
from test_priors import F32, PRIOR_CODES, code_of, inputs, matrices, prior_vectors

OPTIONS = (1, 2)                         # first sector X / Z
MODES = ("scalar", "random", "special")  # depolarising p, or a Pauli channel of pauli_vectors(n, kind)
P_SCALAR = 0.05
PAULI_SALT = 0x3C6EF372  # include/qec_ldpc.h, qec_sample_pauli_dev (kPauliSalt of qec_mc.h)
# the largest float below 1/3: three of the float nearest to 1/3 sum to 1 + 3e-8 in double, which the channel
# refuses (test_validation asserts that)
THIRD = np.nextafter(F32(1.0) / F32(3.0), F32(0.0))


def pauli_vectors(n, kind, seed=20250317):
    """(pX, pY, pZ): each component log-uniform in [0.002, 0.08] from a fixed numpy seed; "special": five qubits
    overwritten by (0,0,0), (0,1/2,0), (1/3,1/3,1/3), (0,0,1) and (1,0,0)."""
    rng = np.random.default_rng(seed + n)
    out = [np.exp(rng.uniform(np.log(0.002), np.log(0.08), n)).astype(F32) for _ in range(3)]
    pos = rng.choice(n, 5, replace=False)
    if kind == "special":
        rows = ((0, 0, 0), (0, 0.5, 0), (THIRD, THIRD, THIRD), (0, 0, 1), (1, 0, 0))
        for v, row in zip(pos, rows):
            for a in range(3):
                out[a][v] = F32(row[a])
    else:
        assert kind == "random"
    return tuple(out)


# ---- the tables in numpy double ------------------------------------------------------------------------------
def _ratio(num, den):
    with np.errstate(all="ignore"):
        r = np.minimum(1.0, num / den)
    return np.where(den == 0.0, 0.5, r).astype(F32)


def channel_tables(pX, pY, pZ):
    """priorX, priorZ, cZ0, cZ1, cX0, cX1 from the float32 vectors: IEEE double +, -, /, one rounding to float."""
    x, y, z = (np.asarray(a, dtype=F32).astype(np.float64) for a in (pX, pY, pZ))
    return {"priorX": (x + y).astype(F32), "priorZ": (z + y).astype(F32),
            "cZ1": _ratio(y, x + y), "cZ0": _ratio(z, 1.0 - (x + y)),
            "cX1": _ratio(y, z + y), "cX0": _ratio(x, 1.0 - (z + y))}


def scalar_tables(p, n):
    """The tables of a decoder without priors, read back from qec_correlated_priors, and p' for the first sector."""
    c0, c1 = q.correlated_priors(p)
    pp = np.full(n, F32(2.0) / F32(3.0) * F32(p), dtype=F32)
    t0, t1 = np.full(n, c0, dtype=F32), np.full(n, c1, dtype=F32)
    return {"priorX": pp, "priorZ": pp, "cZ0": t0, "cZ1": t1, "cX0": t0, "cX1": t1}


# ---- the yardstick ------------------------------------------------------------------------------------------
def bp_sector_rows(H, s, prior, N, stop, D):
    """bp_sector_priors of test_priors.py with the prior as a [B, n] array: row b starts the real slots of variable
    v at prior[b, v] and v's two running products from 1 - prior[b, v] and prior[b, v]."""
    m, n = H.shape
    B = s.shape[0]
    nbr = [np.nonzero(H[c])[0] for c in range(m)]
    edges = [[(c, int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]
    real = np.zeros((m, D), dtype=bool)
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(prior, dtype=F32), (B, n)))
    omp = (F32(1.0) - pp).astype(F32)
    msg = np.zeros((B, m, D), dtype=F32)
    for c in range(m):
        real[c, :len(nbr[c])] = True
        msg[:, c, :len(nbr[c])] = pp[:, nbr[c]]
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
                    P0, P1 = omp[:, v].copy(), pp[:, v].copy()
                    for k in range(dv):
                        P0, P1 = P0 * bv[k], P1 * g[k]
                    for c, k in edges[v]:
                        new[:, c, k] = P1 / (P0 + P1)
                else:
                    pre0, pre1 = omp[:, v].copy(), pp[:, v].copy()
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


def _assemble(secX, secZ):
    (eX, fx, cx, ix, qx), (eZ, fz, cz, iz, qz) = secX, secZ
    flags = (fx * q.SYNDROME_FAIL_X + fz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = eX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32)


def corr_yardstick(HX, HZ, sX, sZ, tab, N, stop):
    """{0: the independent decode, 1: X first, 2: Z first}, each (eX, eZ, flags, iters [B, 2], q).  Decode F under
    its marginal; pi = where(F's estimate, c1_S, c0_S); decode S under pi."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    fX = bp_sector_rows(HX, sX, tab["priorX"], N, stop, D)
    fZ = bp_sector_rows(HZ, sZ, tab["priorZ"], N, stop, D)
    piZ = np.where(fX[0] != 0, tab["cZ1"][None], tab["cZ0"][None]).astype(F32)
    piX = np.where(fZ[0] != 0, tab["cX1"][None], tab["cX0"][None]).astype(F32)
    return {0: _assemble(fX, fZ), 1: _assemble(fX, bp_sector_rows(HZ, sZ, piZ, N, stop, D)),
            2: _assemble(bp_sector_rows(HX, sX, piX, N, stop, D), fZ)}


def tables_of(n, mode, p=P_SCALAR):
    return scalar_tables(p, n) if mode == "scalar" else channel_tables(*pauli_vectors(n, mode))


_yard = {}


def yardstick(name, mode, stop, N):
    """corr_yardstick on inputs(name), computed once per session."""
    key = (name, mode, stop, N)
    if key not in _yard:
        HX, HZ = matrices(name)
        _yard[key] = corr_yardstick(HX, HZ, *inputs(name), tables_of(HX.shape[1], mode), N, stop)
    return _yard[key]


def configure(dec, mode, option):
    """The decoder in `mode` with the option set; `p` to decode with."""
    if mode == "scalar":
        dec.set_pauli_channel(None, None, None)
    else:
        dec.set_pauli_channel(*pauli_vectors(dec.code.n, mode))
    dec.set_option("correlated", option)
    return P_SCALAR if mode == "scalar" else 0.3  # with a channel p is not used


def unpack(rec, n):
    nb = (n + 7) // 8
    return (np.unpackbits(rec[:, :nb], axis=1, bitorder="little")[:, :n],
            np.unpackbits(rec[:, nb:2 * nb], axis=1, bitorder="little")[:, :n], rec[:, -1])


# ---- the Pauli sampler in numpy --------------------------------------------------------------------------------
def pauli_thresholds(pX, pY, pZ):
    x, y, z = (np.asarray(a, dtype=F32).astype(np.float64) for a in (pX, pY, pZ))
    two32 = 4294967296.0
    return ((x * two32).astype(np.int64), ((x + y) * two32).astype(np.int64),
            (np.minimum(1.0, (x + y) + z) * two32).astype(np.int64))


def pauli_samples(seed, start, count, pX, pY, pZ):
    """(x, z) uint8 [count, n]: sample b makes Philox calls k = 0, 1, ... with counter (b lo, b hi, k, salt) and key
    (seed lo, seed hi); output word j of call k is the word u of qubit 4k + j; x = u < tXY, z = tX <= u < tXYZ."""
    n = len(pX)
    nc = (n + 3) // 4
    b = (np.arange(count, dtype=np.uint64) + np.uint64(start))[:, None].repeat(nc, axis=1)
    k = np.arange(nc, dtype=np.uint64)[None].repeat(count, axis=0)
    o = philox4x32_10(b & MASK, b >> np.uint64(32), k, np.full(b.shape, PAULI_SALT, np.uint64), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    u = np.stack(o, axis=2).reshape(count, 4 * nc).astype(np.int64)[:, :n]
    tX, tXY, tXYZ = pauli_thresholds(pX, pY, pZ)
    return (u < tXY[None]).astype(np.uint8), ((u >= tX[None]) & (u < tXYZ[None])).astype(np.uint8)


# ---- the tables -------------------------------------------------------------------------------------------------
def test_scalar_tables():
    for p in (0.05, 0.003, 0.02, 0.3):
        c0, c1 = q.correlated_priors(p)
        pf = F32(p)
        assert c1 == F32(0.5)
        assert c0 == (pf / F32(3.0)) / (F32(1.0) - F32(2.0) / F32(3.0) * pf)
        assert c0.dtype == np.float32


@pytest.mark.parametrize("kind", ["random", "special"])
def test_channel_tables_and_read_back(kind):
    code = code_of("hgp_ham")
    dec = q.DecoderCPU(code)
    assert dec.get_pauli_channel() is None and dec.get_conditional_priors() is None
    pv = pauli_vectors(code.n, kind)
    dec.set_pauli_channel(*pv)
    assert all(same_floats(a, b) for a, b in zip(dec.get_pauli_channel(), pv))
    tab = channel_tables(*pv)
    gX, gZ = dec.get_priors()
    assert same_floats(gX, tab["priorX"]) and same_floats(gZ, tab["priorZ"])
    for got, key in zip(dec.get_conditional_priors(), ("cZ0", "cZ1", "cX0", "cX1")):
        assert same_floats(got, tab[key]), key
    if kind == "special":  # the zero denominators and the clamp occur
        x, y, z = (a.astype(np.float64) for a in pv)
        assert ((x + y) == 0).any() and ((z + y) == 0).any() and ((1 - (x + y)) == 0).any() and ((1 - (z + y)) == 0).any()
        assert (tab["cZ1"] == F32(0.5)).any() and (tab["cX0"] == F32(1.0)).any()
    # the OSD weight tables are those of the marginals
    ref = q.DecoderCPU(code)
    ref.set_priors(tab["priorX"], tab["priorZ"])
    assert all(np.array_equal(a, b) for a, b in zip(dec.osd_weights(), ref.osd_weights()))
    assert ref.get_pauli_channel() is None
    # a later set_priors, (None, None) included, drops the channel; all three None clears both
    dec.set_priors(gX, gZ)
    assert dec.get_pauli_channel() is None and dec.get_conditional_priors() is None and dec.get_priors() is not None
    dec.set_pauli_channel(*pv)
    dec.set_priors(None, None)
    assert dec.get_pauli_channel() is None and dec.get_priors() is None
    dec.set_pauli_channel(*pv)
    dec.set_pauli_channel(None, None, None)
    assert dec.get_pauli_channel() is None and dec.get_priors() is None
    dec.set_pauli_channel(0.01, 0.02, 0.03)  # scalars broadcast
    assert all((a == F32(v)).all() for a, v in zip(dec.get_pauli_channel(), (0.01, 0.02, 0.03)))


# ---- CPU engine = yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRIOR_CODES)
@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("mode", MODES)
def test_cpu_engine_matches_yardstick(name, stop, mode):
    code = code_of(name)
    dec = q.DecoderCPU(code)
    sX, sZ = inputs(name)
    for N in NS:
        want = yardstick(name, mode, stop, N)
        for option in (0,) + OPTIONS:
            p = configure(dec, mode, option)
            what = "%s %s %s N=%d option %d" % (name, mode, stop, N, option)
            got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            assert_same_decode(got, want[option], what)
            assert ("correlated" in dec.last_path()) == bool(option)
            rec, it = dec.decode_batch_packed(sX, sZ, p, N, stop, want_iters=True)
            assert np.array_equal(it, got[3]), what
            assert all(np.array_equal(a, b) for a, b in zip(unpack(rec, code.n), got[:3])), what


# ---- identities ---------------------------------------------------------------------------------------------------
def first_sector_equal(got, base, option, code, what):
    """F's estimate, its two flag bits, its iters entry and its block of q_final are the option-0 call's."""
    sec = option - 1
    EX = code.numEqsX * code.stride
    bits = (q.SYNDROME_FAIL_X | q.CONVERGENCE_FAIL_X) << sec
    assert np.array_equal(got[sec], base[sec]), what
    assert np.array_equal(got[2] & bits, base[2] & bits), what
    assert np.array_equal(got[3][:, sec], base[3][:, sec]), what
    blk = slice(0, EX) if sec == 0 else slice(EX, None)
    assert same_floats(got[4][:, blk], base[4][:, blk]), what


@pytest.mark.parametrize("name", PRIOR_CODES)
@pytest.mark.parametrize("mode", MODES)
def test_first_sector_is_untouched_and_option_0_restores(name, mode):
    code = code_of(name)
    dec, ref = q.DecoderCPU(code), q.DecoderCPU(code)
    sX, sZ = inputs(name)
    p = configure(ref, mode, 0)
    for stop in STOPS:
        for N in (1, 11, 20):
            base = ref.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
            for option in OPTIONS:
                configure(dec, mode, option)
                got = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)
                first_sector_equal(got, base, option, code, "%s %s %s N=%d option %d" % (name, mode, stop, N, option))
                dec.set_option("correlated", 0)
                assert_same_decode(dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True), base, "option back to 0")


@pytest.mark.parametrize("name", PRIOR_CODES)
def test_plain_priors_carry_no_correlation(name):
    """set_priors alone: c0 = c1 = the marginal, so the correlated decode is the option-0 decode in every bit."""
    code = code_of(name)
    dec = q.DecoderCPU(code)
    dec.set_priors(*prior_vectors(code.n, "random"))
    sX, sZ = inputs(name)
    for stop in STOPS:
        for N in (0, 1, 11, 20):
            dec.set_option("correlated", 0)
            base = dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)
            for option in OPTIONS:
                dec.set_option("correlated", option)
                assert_same_decode(dec.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True), base,
                                   "%s %s N=%d option %d" % (name, stop, N, option))


@pytest.mark.parametrize("name", PRIOR_CODES)
def test_rows_with_a_zero_first_estimate_decode_under_c0(name):
    """Scalar mode: where F's estimate is all zero, S is a set_priors decode whose S prior is c0 everywhere."""
    code = code_of(name)
    dec, ref = q.DecoderCPU(code), q.DecoderCPU(code)
    sX, sZ = inputs(name)
    c0, _ = q.correlated_priors(P_SCALAR)
    pp = F32(2.0) / F32(3.0) * F32(P_SCALAR)
    EX = code.numEqsX * code.stride
    for option in OPTIONS:
        sec = 2 - option  # S
        dec.set_option("correlated", option)
        ref.set_priors(*((pp, c0) if sec == 1 else (c0, pp)))
        for stop in STOPS:
            got = dec.decode_batch(sX, sZ, P_SCALAR, 11, stop, want_iters=True, want_q=True)
            want = ref.decode_batch(sX, sZ, P_SCALAR, 11, stop, want_iters=True, want_q=True)
            rows = ~got[1 - sec].any(axis=1)
            assert rows.sum() >= 2 and not rows.all(), (name, option, int(rows.sum()))
            bits = (q.SYNDROME_FAIL_X | q.CONVERGENCE_FAIL_X) << sec
            blk = slice(EX, None) if sec else slice(0, EX)
            assert np.array_equal(got[sec][rows], want[sec][rows])
            assert np.array_equal((got[2] & bits)[rows], (want[2] & bits)[rows])
            assert np.array_equal(got[3][rows, sec], want[3][rows, sec])
            assert same_floats(got[4][rows][:, blk], want[4][rows][:, blk])


def assert_not_vacuous(base, corr, option, code, what):
    """S's q_final block differs from option 0's and at least one sampled row's S decisions differ."""
    sec = 2 - option
    EX = code.numEqsX * code.stride
    blk = slice(EX, None) if sec else slice(0, EX)
    assert not same_floats(corr[4][:, blk], base[4][:, blk]), what
    rows = int((corr[sec][:48] != base[sec][:48]).any(axis=1).sum())
    assert rows >= 1, what
    return rows


@pytest.mark.parametrize("N", [11, 20])
@pytest.mark.parametrize("option", OPTIONS)
def test_the_correlated_decode_differs(N, option):
    """On the yardstick: hgp_ham, scalar p = 0.05."""
    code = code_of("hgp_ham")
    y = yardstick("hgp_ham", "scalar", "syndrome", N)
    assert_not_vacuous(y[0], y[option], option, code, "hgp_ham N=%d option %d" % (N, option))


def test_near_hard_jump_never_fires_for_the_second_sector():
    """G13 is where the CPU engine's jump can fire: no output depends on it, with the option at 1 or 2 either."""
    code = code_of("G13")
    sX, sZ = inputs("G13")
    for option in OPTIONS:
        outs = []
        for near in (1, 0):
            dec = q.DecoderCPU(code)
            dec.set_option("near_hard", near)
            dec.set_option("correlated", option)
            outs.append([dec.decode_batch(sX, sZ, P_SCALAR, N, stop, want_iters=True) for stop in ("ref", "fixed")
                         for N in (11, 20, 50)])
        for a, b in zip(*outs):
            assert_same_decode(a, b, "near_hard on / off", with_q=False)
        assert_same_decode(outs[0][3], yardstick("G13", "scalar", "fixed", 11)[option], "fixed 11", with_q=False)


# ---- validation ---------------------------------------------------------------------------------------------------
def test_option_values():
    dec = q.DecoderCPU(code_of("surf3"))
    assert dec.get_option("correlated") == 0
    for bad in (-1, 3, 17):
        with pytest.raises(q.QecError, match="QEC_OPT_CORRELATED"):
            dec.set_option("correlated", bad)
        assert q.lib().qec_decoder_set_option(dec._h, q.OPTION["correlated"], bad) == -1  # QEC_ERR_ARG
    for v in (1, 2, 0):
        dec.set_option("correlated", v)
        assert dec.get_option("correlated") == v
    assert q.OPTION["correlated"] == 17 and q.PATH["correlated"] == 512
    assert q.lib().qec_abi_version() == 4


def test_validation():
    code = code_of("hgp_ham")
    n = code.n
    dec = q.DecoderCPU(code)
    pv = pauli_vectors(n, "special")
    dec.set_pauli_channel(*pv)

    def unchanged():
        assert all(same_floats(a, b) for a, b in zip(dec.get_pauli_channel(), pv))
        assert same_floats(dec.get_priors()[0], channel_tables(*pv)["priorX"])

    for bad in (-0.1, 1.5, float("nan")):
        for arr, idx in ((0, 0), (1, 17), (2, n - 1)):
            vs = [a.copy() for a in pv]
            vs[arr][idx] = bad
            with pytest.raises(q.QecError, match=r"p%s\[%d\] = " % ("XYZ"[arr], idx)):
                dec.set_pauli_channel(*vs)
            unchanged()
    third = F32(1.0) / F32(3.0)  # three of them are above 1 in double
    vs = [a.copy() for a in pv]
    for a in vs:
        a[9] = third
    with pytest.raises(q.QecError, match=r"pX\[9\] \+ pY\[9\] \+ pZ\[9\] = "):
        dec.set_pauli_channel(*vs)
    vs = [a.copy() for a in pv]
    vs[0][4], vs[2][4] = 0.6, 0.5
    with pytest.raises(q.QecError, match=r"pX\[4\] \+ pY\[4\] \+ pZ\[4\]"):
        dec.set_pauli_channel(*vs)
    assert q.lib().qec_decoder_set_pauli_channel(dec._h, *[q._ptr(a) for a in vs]) == -1  # QEC_ERR_ARG
    unchanged()
    for k in range(3):  # wrong lengths
        vs = list(pv)
        vs[k] = vs[k][:-1]
        with pytest.raises(q.QecError, match="length n = %d" % n):
            dec.set_pauli_channel(*vs)
    # one or two NULLs
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        with pytest.raises(q.QecError, match="all"):
            dec.set_pauli_channel(*[a if m else None for a, m in zip(pv, mask)])
        assert q.lib().qec_decoder_set_pauli_channel(dec._h, *[q._ptr(a) if m else None for a, m in zip(pv, mask)]) == -1
        assert "pX, pY and pZ" in q.last_error()
    unchanged()


# ---- the sampler's restatement ------------------------------------------------------------------------------------
def test_pauli_restatement_threshold_edges():
    n, B = 13, 4096
    pX, pY, pZ = (np.zeros(n, dtype=F32) for _ in range(3))
    pX[3] = 1.0                       # always X
    pZ[5] = 1.0                       # always Z
    pY[6] = 1.0                       # always Y
    pX[7] = F32(2.0) ** -32           # tX = 1: X only for a word that is 0
    pY[8] = 0.5
    pX[9], pY[9], pZ[9] = 0.25, 0.25, 0.5
    assert [int(t[7]) for t in pauli_thresholds(pX, pY, pZ)] == [1, 1, 1]
    assert [int(t[9]) for t in pauli_thresholds(pX, pY, pZ)] == [1 << 30, 1 << 31, 1 << 32]
    start = (1 << 32) - 64
    x, z = pauli_samples(99, start, B, pX, pY, pZ)
    quiet = [0, 1, 2, 4, 7, 10, 11, 12]
    assert not x[:, quiet].any() and not z[:, quiet].any()
    assert x[:, 3].all() and not z[:, 3].any() and z[:, 5].all() and not x[:, 5].any()
    assert x[:, 6].all() and z[:, 6].all()
    assert np.array_equal(x[:, 8], z[:, 8]) and abs(int(x[:, 8].sum()) - B // 2) < 5 * 32
    assert (x[:, 9] | z[:, 9]).all() and abs(int((x[:, 9] & z[:, 9]).sum()) - B // 4) < 5 * 28
    a = pauli_samples(99, start, 128, pX, pY, pZ)
    b = pauli_samples(99, start + 100, 28, pX, pY, pZ)
    assert np.array_equal(a[0], x[:128]) and np.array_equal(b[0], x[100:128]) and np.array_equal(b[1], z[100:128])


# ---- OSD behind a correlated decode ----------------------------------------------------------------------------------
def test_cpu_osd_soft_decode_is_correlated():
    """osd = 1: the result is dec.osd fed with the q_final of a fixed-stop osd_iterations decode under the same
    option and channel, and it differs from the option-0 stage's."""
    name, N, B = "hgp_ham", 20, 256
    HX, HZ = code_matrices(name)
    code = code_of(name)
    pv = tuple(np.minimum(a * F32(2.5), F32(0.3)) for a in pauli_vectors(code.n, "random"))
    x, z = pauli_samples(777, 0, B, *pv)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    dec = q.DecoderCPU(code)
    dec.set_pauli_channel(*pv)
    results = {}
    for option in (0, 1, 2):
        dec.set_option("osd", 0)
        dec.set_option("osd_order", 10)
        dec.set_option("correlated", option)
        main = dec.decode_batch(sX, sZ, 0.3, N, "syndrome", want_iters=True)
        assert (main[2] & 3).any()
        soft = dec.decode_batch(sX, sZ, 0.3, dec.get_option("osd_iterations"), "fixed", want_q=True)[4]
        want = dec.osd(sX, sZ, soft, main[0], main[1], main[2])
        dec.set_option("osd", 1)
        got = dec.decode_batch(sX, sZ, 0.3, N, "syndrome", want_iters=True)
        for a, b in zip(got[:3], want):
            assert np.array_equal(a, b), option
        assert not (got[2] & 3).any()
        results[option] = got
    assert any(not np.array_equal(results[0][k], results[1][k]) for k in (0, 1))


# ---- CLI --------------------------------------------------------------------------------------------------------
def _write_pauli(path, vectors):
    path.write_text("\n".join(" ".join("%.9g" % v for v in a) for a in vectors) + "\n")
    return str(path)


def test_cli_correlated_and_pauli(tmp_path):
    from qec_ldpc_amd.codes import write_css_file
    from test_osd_host import _cli, _fields
    HX, HZ = code_matrices("hgp_ham")
    n = HX.shape[1]
    code = write_css_file(str(tmp_path / "hgp.txt"), HX, HZ)
    line = "4 4 1500 20 0.05"
    base = ["--engine", "cpu", "--seed", "7", "--logical", "degenerate"]
    pv = pauli_vectors(n, "random")
    runs = {"plain": [], "xz": ["--correlated", "xz"], "zx": ["--correlated", "zx"],
            "pauli": ["--pauli", _write_pauli(tmp_path / "p.txt", pv)],
            "pauli-xz": ["--pauli", _write_pauli(tmp_path / "p.txt", pv), "--correlated", "xz"]}
    out = {}
    for key, flags in runs.items():
        d = tmp_path / key
        d.mkdir()
        r = _cli(d, base + flags, code, line)
        assert r.returncode == 0, r.stderr
        out[key] = {k: v for k, v in _fields(d).items() if not k.startswith("Duration")}
    assert out["xz"] != out["plain"] and out["zx"] != out["plain"] and out["pauli"] != out["plain"]
    assert out["pauli-xz"] != out["pauli"]
    d = tmp_path / "short"
    d.mkdir()
    r = _cli(d, base + ["--pauli", _write_pauli(tmp_path / "s.txt", (pv[0][:-1], pv[1], pv[2]))], code, line)
    assert r.returncode == 1 and "n = %d" % n in r.stderr
    d = tmp_path / "bad"
    d.mkdir()
    r = _cli(d, base + ["--correlated", "yx"], code, line)
    assert r.returncode != 0


# ---- the CORR instantiations of bp_sparse.hip ----------------------------------------------------------------------
def corr_instance_of(code, general, stop):
    """The CORR kernel launch_decode_sparse starts with the option at 1 or 2: the scalar plan's kernel, shape and
    workspace (the plan does not change), whatever the handle's priors."""
    from test_sparse_shapes import plan_of
    p = plan_of(code, general)
    return (p["kernel"], p["shape"], p["mem"], stop)


def test_case_table_reaches_every_corr_instantiation():
    """36 of 36: two kernels x three shapes x LDS / HBM x three stop rules, through the case table that
    tests/test_gpu_correlated.py runs."""
    import test_sparse_shapes as ss
    every = {(k, s, mem, stop) for k in ss.KERNELS for s in ss.SHAPES for mem in ("lds", "hbm") for stop in STOPS}
    assert len(every) == 36
    reached = {corr_instance_of(ss.code_of(name, route), route == "general", stop)
               for name, route in ss.LDS_CASES + ss.HBM_CASES for stop in STOPS}
    assert reached == every, sorted(every - reached)
    lds = {corr_instance_of(ss.code_of(name, route), route == "general", stop) for name, route in ss.LDS_CASES for stop in STOPS}
    assert lds == {i for i in every if i[2] == "lds"}

"""Noisy syndromes in min-sum BP (set_syndrome_priors; DESIGN.md section 2, "The soft-syndrome form") on the CPU engine.

The yardstick is a numpy restatement of the definition, stated natively: `soft_minsum_sector` (flooding) and
`soft_layered_sector` (layered) give every check one virtual input mu_c, form the virtual slot's own output rho_c and the
measurement decision f_c = (mu_c + rho_c < 0), XOR f_c into the syndrome test and keep the inside tests on the data slots /
data posteriors.  They are held twice: against the yardsticks of tests/test_minsum.py and tests/test_minsum_layered.py on
the extended matrix [H | I] under the fixed and syndrome stops (where the two definitions coincide), and the CPU engine is
held against them under all three stops.

  * the CPU engine against the yardstick: the small general and regular codes of tests/test_sparse_shapes.py and the
    shipped P7, every stop rule, N in {0, 1, 11, 20}, scalar p and data priors, scales 160 and 256, both schedules, every
    output including f;
  * equality (b): the handle with syndrome priors against DecoderCPU on the extended code
    createFromMatrices([HX | I | 0], [HZ | 0 | I]) with set_priors(concat(pi, q, q)) -- the path that existed before --
    under the fixed and syndrome stops: eX, eZ, the SYNDROME_FAIL bits, iters, q_final on the real slots, f;
  * equality (a): q = 0 equals the call without syndrome priors;
  * non-vacuity on the reference outputs, the flip sampler's numpy restatement, refusals in both orders, the round trip,
    the CLI flags.

Bit for bit everywhere (q_final as uint32 patterns).  There is no tolerance."""
import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.philox import philox4x32_10
from qec_ldpc_amd.codes import P7, P61, code_path
from test_general_code import STOPS, assert_same_decode, same_floats
from test_minsum import CAP, INSIDE, MS_P, MS_P_REF, PRIOR_NS, SCALES, SMALL, library_llr, minsum_cpu, minsum_sector, routes
from test_minsum_layered import layered_minsum_sector
from test_priors import VECTORS, prior_vectors
from test_serial import greedy_colours, processing_order
from test_sparse_shapes import REGULAR, code_of, inputs, matrices

F32 = np.float32
U32 = np.uint32
FLIP_SALT = 0xA54FF53A  # include/qec_ldpc.h, qec_flip_syndrome_dev
SCHEDULES = ("flooding", "layered")
NS = (0, 1, 11, 20)
CODES = SMALL + ("P7",)
Q_LO, Q_HI = 0.01, 0.2  # the syndrome priors of the tests: log-uniform per check


# ---- the yardstick: "The soft-syndrome form" of DESIGN.md section 2 in numpy -------------------------------------------
def _tables(H):
    m, n = H.shape
    nbr = [np.nonzero(H[c])[0] for c in range(m)]                                  # N(c), ascending
    edges = [[(int(c), int(np.nonzero(nbr[c] == v)[0][0])) for c in np.nonzero(H[:, v])[0]] for v in range(n)]  # M(v)
    return nbr, edges


def _soft_check(qs, tc, mu_c, alpha):
    """One check with its virtual input: qs [B, dc] real inputs, tc [B] the entry's truthiness, mu_c the virtual input.
    -> (R [B, dc] the real slots' outputs, rho [B] the virtual slot's own output)."""
    B, dc = qs.shape
    bits = np.ascontiguousarray(qs).view(U32)
    a, g = bits & U32(0x7FFFFFFF), bits >> U32(31)
    mb = np.array([mu_c], dtype=F32).view(U32)[0]
    am, gm = mb & U32(0x7FFFFFFF), mb >> U32(31)
    others = ~np.eye(dc, dtype=bool)[None]                                         # [1, slot i, input k]: k != i
    mag = np.where(others, a[:, None, :], U32(0xFFFFFFFF)).min(axis=2)             # the other real inputs ...
    mag = np.minimum(np.minimum(mag, am), CAP)                                     # ... the virtual one, and K
    sign = np.bitwise_xor.reduce(np.where(others, g[:, None, :], U32(0)), axis=2) ^ tc[:, None] ^ gm
    out = (alpha * np.ascontiguousarray(mag).view(F32)).astype(F32)
    R = (out.view(U32) | (sign << U32(31))).view(F32)
    vmag = np.minimum(a.min(axis=1), CAP)                                          # min(K, all a_k): the real inputs only
    vsign = np.bitwise_xor.reduce(g, axis=1) ^ tc
    vout = (alpha * np.ascontiguousarray(vmag).view(F32)).astype(F32)
    return R, (vout.view(U32) | (vsign << U32(31))).view(F32)


def soft_minsum_sector(H, s, llr, mu, alpha_k, N, stop, D):
    """Flooding.  llr [n]: the data variables' channel LLRs, mu [m]: the measurement-error variables'.
    -> (e [B, n], f [B, m], syndrome failed [B], convergence failed [B], iterations [B], q [B, m, D])."""
    m, n = H.shape
    B = s.shape[0]
    nbr, edges = _tables(H)
    real = np.zeros((m, D), dtype=bool)
    for c in range(m):
        real[c, :len(nbr[c])] = True
    lam, mu = np.asarray(llr, dtype=F32), np.asarray(mu, dtype=F32)
    alpha = F32(alpha_k) / F32(256.0)
    connected = np.array([len(edges[v]) > 0 for v in range(n)])
    M = np.zeros((B, m, D), dtype=F32)
    for c in range(m):
        M[:, c, :len(nbr[c])] = lam[nbr[c]]
    d = np.broadcast_to(((lam < F32(0.0)) & connected).astype(np.uint8), (B, n)).copy()  # N = 0
    f = np.broadcast_to((mu < F32(0.0)).astype(np.uint8), (B, m)).copy()                 # N = 0
    t = (s != 0).astype(U32)
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)

    def syndrome_fails(e, f):
        bad = np.zeros(B, dtype=bool)
        for c in range(m):
            bad |= ((e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) ^ f[:, c]) != s[:, c]  # the entry's exact value
        return bad

    def inside_any(M):
        return ((np.abs(M) < INSIDE) & real[None]).any(axis=(1, 2))                # the data slots only

    with np.errstate(all="ignore"):
        for it in range(N):
            if not active.any():
                break
            iters += active
            R = np.zeros_like(M)
            fn = np.zeros((B, m), dtype=np.uint8)
            for c in range(m):
                dc = len(nbr[c])
                R[:, c, :dc], rho = _soft_check(M[:, c, :dc], t[:, c], mu[c], alpha)
                fn[:, c] = (mu[c] + rho) < F32(0.0)                                # postm = mu + rho, one fp32 add
            new = np.zeros_like(M)
            dec = np.zeros((B, n), dtype=np.uint8)
            last = it == N - 1
            for v in range(n):
                if not connected[v]:
                    continue
                rs = [R[:, c, k] for c, k in edges[v]]
                post = np.full(B, lam[v], dtype=F32)
                for r in rs:
                    post = post + r
                dec[:, v] = post < F32(0.0)
                for j, (c, k) in enumerate(edges[v]):
                    if last:
                        new[:, c, k] = post
                    else:
                        x = np.full(B, lam[v], dtype=F32)
                        for i, r in enumerate(rs):
                            if i != j:
                                x = x + r
                        new[:, c, k] = x
            M = np.where(active[:, None, None], new, M)
            d = np.where(active[:, None], dec, d)
            f = np.where(active[:, None], fn, f)
            if stop == "ref" and it % 10 == 0:
                active &= inside_any(M)
            elif stop == "syndrome":
                active &= syndrome_fails(d, f)
    return d, f, syndrome_fails(d, f), inside_any(M), iters, M


def soft_layered_sector(H, s, llr, mu, alpha_k, N, stop, D):
    """Layered: the layers are those of H; R[c, virtual] = rho_c is made when c is processed and kept."""
    m, n = H.shape
    B = s.shape[0]
    nbr, edges = _tables(H)
    order = processing_order(greedy_colours(H))
    lam, mu = np.asarray(llr, dtype=F32), np.asarray(mu, dtype=F32)
    alpha = F32(alpha_k) / F32(256.0)
    connected = np.array([len(edges[v]) > 0 for v in range(n)])
    R = np.zeros((B, m, D), dtype=F32)
    Rv = np.zeros((B, m), dtype=F32)                                               # R[c, virtual], +0.0f at the start
    t = (s != 0).astype(U32)
    active = np.ones(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)

    def fold(R, v, skip):
        x = np.full(B, lam[v], dtype=F32)
        for c, k in edges[v]:
            if c != skip:
                x = x + R[:, c, k]
        return x

    def posterior(R):
        post = np.zeros((B, n), dtype=F32)
        for v in range(n):
            if connected[v]:
                post[:, v] = fold(R, v, -1)
        return post

    def decide(post):
        return ((post < F32(0.0)) & connected[None]).astype(np.uint8)

    def flips(Rv):
        return ((mu[None, :] + Rv) < F32(0.0)).astype(np.uint8)                    # postm = mu + R[c, virtual]

    def syndrome_fails(e, f):
        bad = np.zeros(B, dtype=bool)
        for c in range(m):
            bad |= ((e[:, nbr[c]].sum(axis=1) & 1).astype(np.uint8) ^ f[:, c]) != s[:, c]
        return bad

    def inside_any(post):
        return ((np.abs(post) < INSIDE) & connected[None]).any(axis=1)             # the data posteriors only

    with np.errstate(all="ignore"):
        for it in range(N):
            if not active.any():
                break
            iters += active
            new, newv = R.copy(), Rv.copy()
            for c in order:
                qs = np.stack([fold(new, v, c) for v in nbr[c]], axis=1)
                new[:, c, :len(nbr[c])], newv[:, c] = _soft_check(qs, t[:, c], mu[c], alpha)
            R = np.where(active[:, None, None], new, R)
            Rv = np.where(active[:, None], newv, Rv)
            if stop == "ref" and it % 10 == 0:
                active &= inside_any(posterior(R))
            elif stop == "syndrome":
                active &= syndrome_fails(decide(posterior(R)), flips(Rv))
        post = posterior(R)
    e, f = decide(post), flips(Rv)
    qf = np.zeros((B, m, D), dtype=F32)
    for c in range(m):
        qf[:, c, :len(nbr[c])] = post[:, nbr[c]]
    return e, f, syndrome_fails(e, f), inside_any(post), iters, qf


def data_llrs(n, piX, piZ):
    if np.ndim(piX) == 0:
        lX = lZ = np.full(n, q.minsum_llr(F32(2.0) / F32(3.0) * F32(piX)), dtype=F32)
        return lX, lZ
    return library_llr(piX), library_llr(piZ)


def soft_yardstick(HX, HZ, sX, sZ, piX, piZ, qX, qZ, alpha_k, N, stop, schedule="flooding"):
    """-> (eX, eZ, flags, iters [B, 2], q [B, (mX + mZ) D], fX, fZ); piX / piZ: n priors each, or a scalar p for both.
    The channel LLRs are the library's."""
    D = int(max(HX.sum(axis=1).max(), HZ.sum(axis=1).max()))
    lX, lZ = data_llrs(HX.shape[1], piX, piZ)
    sector = soft_minsum_sector if schedule == "flooding" else soft_layered_sector
    sX, sZ = np.asarray(sX, dtype=np.uint8), np.asarray(sZ, dtype=np.uint8)
    eX, fX, bx, cx, ix, qx = sector(HX, sX, lX, library_llr(qX), alpha_k, N, stop, D)
    eZ, fZ, bz, cz, iz, qz = sector(HZ, sZ, lZ, library_llr(qZ), alpha_k, N, stop, D)
    flags = (bx * q.SYNDROME_FAIL_X + bz * q.SYNDROME_FAIL_Z + cx * q.CONVERGENCE_FAIL_X +
             cz * q.CONVERGENCE_FAIL_Z).astype(np.uint8)
    B = sX.shape[0]
    qf = np.concatenate([qx.reshape(B, -1), qz.reshape(B, -1)], axis=1)
    return (eX, eZ, flags, np.stack([ix, iz], axis=1).astype(np.int32), np.ascontiguousarray(qf, dtype=F32),
            fX.astype(np.uint8), fZ.astype(np.uint8))


# ---- codes, inputs, decoders (shared with the device modules) ----------------------------------------------------------
_p7 = {}


def soft_matrices(name):
    if name == "P7":
        c = soft_code(name, "graph")
        return c.pcm(0), c.pcm(1)
    return matrices(name)


def soft_code(name, route):
    if name == "P7":
        if "code" not in _p7:
            _p7["code"] = q.Quantum_LDPC_Code.createFromFile(code_path(P7))
        return _p7["code"]
    return code_of(name, route)


def soft_routes(name):
    return ("graph",) if name == "P7" else routes(name)


def syndrome_priors(m, seed):
    """m flip probabilities, log-uniform in [Q_LO, Q_HI]."""
    u = np.random.default_rng(seed).random(m)
    return (Q_LO * (Q_HI / Q_LO) ** u).astype(F32)


def flipped(s, qs, seed, keep=0):
    """s with its 0 / 1 entries flipped with the probabilities qs (per column); the last `keep` rows stay."""
    s = np.array(s, dtype=np.uint8)
    f = (np.random.default_rng(seed).random(s.shape) < qs[None, :]).astype(np.uint8)
    if keep:
        f[-keep:] = 0
    return np.where(s <= 1, s ^ f, s).astype(np.uint8)


_inputs = {}


def soft_inputs(name):
    """(sX, sZ, qX, qZ): the syndromes of tests/test_sparse_shapes.py (P7: depolarising samples at p = 0.03) measured
    through the channel q -- their sampled rows flipped, the all-zero row, the all-one row and the row with an entry > 1
    as they are."""
    if name not in _inputs:
        HX, HZ = soft_matrices(name)
        if name == "P7":
            from oracle.philox import depolarizing
            x, z = depolarizing(77, 0, 48, HX.shape[1], 0.03)
            c = soft_code(name, "graph")
            tail = lambda m: np.stack([np.zeros(m), np.ones(m), np.r_[2, np.ones(m - 1)]]).astype(np.uint8)  # noqa: E731
            sX = np.concatenate([c.syndrome(0, x), tail(HX.shape[0])])
            sZ = np.concatenate([c.syndrome(1, z), tail(HZ.shape[0])])
        else:
            sX, sZ = inputs(name)
        qX, qZ = syndrome_priors(HX.shape[0], 11), syndrome_priors(HZ.shape[0], 12)
        out = (flipped(sX, qX, 21, keep=3), flipped(sZ, qZ, 22, keep=3), qX, qZ)
        for a in out:
            a.setflags(write=False)
        _inputs[name] = out
    return _inputs[name]


def soft_cpu(code, qX, qZ, scale=160, priors=None, schedule="flooding"):
    dec = minsum_cpu(code, scale, priors)
    dec.set_option("minsum_schedule", SCHEDULES.index(schedule))
    dec.set_syndrome_priors(qX, qZ)
    return dec


def soft_decode(dec, sX, sZ, p, N, stop, want_q=True):
    return dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=want_q, want_flips=True)


def assert_same_soft(got, want, what, with_q=True):
    assert_same_decode(got, want, what, with_q)
    assert np.array_equal(got[5], want[5]), "%s: fX differs" % what
    assert np.array_equal(got[6], want[6]), "%s: fZ differs" % what


_yard = {}


def yard(name, kind, stop, N, scale=160, schedule="flooding", p=None):
    """The yardstick's decode of soft_inputs(name), computed once.  kind: "scalar" (p, default MS_P or 0.03 for P7) or one
    of test_priors.VECTORS."""
    if kind == "scalar" and p is None:
        p = MS_P.get(name, 0.03)
    key = (name, kind, stop, N, scale, schedule, p)
    if key not in _yard:
        HX, HZ = soft_matrices(name)
        sX, sZ, qX, qZ = soft_inputs(name)
        pri = (p, p) if kind == "scalar" else prior_vectors(HX.shape[1], kind)
        out = soft_yardstick(HX, HZ, sX, sZ, pri[0], pri[1], qX, qZ, scale, N, stop, schedule)
        for a in out:
            a.setflags(write=False)
        _yard[key] = out
    return _yard[key]


# ---- the yardstick against the extended matrix under the imported yardsticks -----------------------------------------
def extended(H):
    return np.concatenate([H, np.eye(H.shape[0], dtype=np.uint8)], axis=1)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ("hgp_ham", "r3-3-6-13", "P7"))
def test_yardstick_is_the_extended_code(name, schedule):
    """Fixed and syndrome stops: the native statement equals min-sum on [H | I] with the channel LLRs (lambda, mu) -- the
    decisions of the first n variables and of the m further ones, the syndrome test, the counts, the real slots."""
    HX, _ = soft_matrices(name)
    sX, _, qX, _ = soft_inputs(name)
    m, n = HX.shape
    D = int(HX.sum(axis=1).max())
    lam = data_llrs(n, MS_P.get(name, 0.03), 0)[0]
    mu = library_llr(qX)
    theirs = minsum_sector if schedule == "flooding" else layered_minsum_sector
    ours = soft_minsum_sector if schedule == "flooding" else soft_layered_sector
    if schedule == "layered":  # degree-1 variables add no check adjacency: the same layers
        assert processing_order(greedy_colours(extended(HX))) == processing_order(greedy_colours(HX))
    for stop, N in (("fixed", 0), ("fixed", 1), ("fixed", 11), ("syndrome", 20)):
        e, f, bad, _, it, qf = ours(HX, np.asarray(sX), lam, mu, 160, N, stop, D)
        E, BAD, _, IT, QF = theirs(extended(HX), np.asarray(sX), np.concatenate([lam, mu]), 160, N, stop, D + 1)
        what = (name, schedule, stop, N)
        assert np.array_equal(e, E[:, :n]) and np.array_equal(f, E[:, n:]), what
        assert np.array_equal(bad, BAD) and np.array_equal(it, IT), what
        for c in range(m):
            dc = int(HX[c].sum())
            assert same_floats(qf[:, c, :dc], QF[:, c, :dc]), what


# ---- the CPU engine against the yardstick ------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", CODES)
def test_cpu_engine_matches_the_yardstick(name, schedule):
    """Scalar p: every stop rule, every N, scale 160 and 256, both routes of a regular code; the reference stop also at
    the p where it fires."""
    sX, sZ, qX, qZ = soft_inputs(name)
    for scale in SCALES:
        decs = [soft_cpu(soft_code(name, r), qX, qZ, scale, None, schedule) for r in soft_routes(name)]
        for stop in STOPS:
            for N in NS:
                p0 = MS_P.get(name, 0.03)
                for p in (p0,) + ((MS_P_REF,) if stop == "ref" and N in (11, 20) else ()):
                    want = yard(name, "scalar", stop, N, scale, schedule, p)
                    assert np.isfinite(want[4]).all()
                    for r, dec in zip(soft_routes(name), decs):
                        got = soft_decode(dec, sX, sZ, p, N, stop)
                        assert_same_soft(got, want, "%s %s %s %s k=%d p=%g N=%d" % (name, r, schedule, stop, scale, p, N))
                        assert dec.last_path() == {"minsum", "soft"} | ({"serial"} if schedule == "layered" else set())
                        plain = dec.decode_batch(sX, sZ, p, N, stop, want_iters=True, want_q=True)  # f = NULL
                        assert_same_decode(plain, want, "the existing entry point")


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("kind", VECTORS)
@pytest.mark.parametrize("name", CODES)
def test_cpu_engine_matches_the_yardstick_under_priors(name, kind, schedule):
    HX, _ = soft_matrices(name)
    sX, sZ, qX, qZ = soft_inputs(name)
    pri = prior_vectors(HX.shape[1], kind)
    for scale in SCALES:
        decs = [soft_cpu(soft_code(name, r), qX, qZ, scale, pri, schedule) for r in soft_routes(name)]
        for stop in STOPS:
            for N in PRIOR_NS:
                want = yard(name, kind, stop, N, scale, schedule)
                for r, dec in zip(soft_routes(name), decs):
                    got = soft_decode(dec, sX, sZ, 0.3, N, stop)  # p is not used
                    assert_same_soft(got, want, "%s %s %s %s %s k=%d N=%d" % (name, r, kind, schedule, stop, scale, N))


# ---- non-vacuity, on the reference outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ("r3-3-6-13", "r4-5-10-7"))
def test_not_vacuous(name, schedule):
    """Column weight >= 3 (on hgp_ham's weight-1 columns |rho| stays below mu and no f bit can be set): some f bit is set,
    some eX differs from the decode that ignores the noise, both outcomes of each stop rule occur."""
    HX, HZ = soft_matrices(name)
    assert min(int(H.sum(axis=0).min()) for H in (HX, HZ)) >= 3
    sX, sZ, qX, qZ = soft_inputs(name)
    syn = yard(name, "scalar", "syndrome", 20, 160, schedule)
    assert syn[5][:-3].any() and syn[6][:-3].any()
    plain = minsum_cpu(soft_code(name, "general"))
    plain.set_option("minsum_schedule", SCHEDULES.index(schedule))
    blind = plain.decode_batch(sX, sZ, MS_P[name], 20, "syndrome", want_iters=True)
    assert (blind[0] != syn[0]).any()
    for sec in (0, 1):
        seen = set(int(x) for x in syn[3][:, sec])
        assert min(seen) < 20 and 20 in seen, (name, sec, seen)
    bit = q.SYNDROME_FAIL_X | q.SYNDROME_FAIL_Z
    assert (syn[2] & bit == 0).any() and (syn[2] & bit).any()
    assert (syn[2] & bit == 0).sum() > (blind[2] & bit == 0).sum()  # the priors satisfy more syndromes
    ref = yard(name, "scalar", "ref", 20, 160, schedule, MS_P_REF)
    seen = set(int(x) for x in ref[3].ravel())
    assert min(seen) < 20 and 20 in seen, (name, seen)
    conv = q.CONVERGENCE_FAIL_X | q.CONVERGENCE_FAIL_Z
    assert (ref[2] & conv == 0).any() and (ref[2] & conv).any()


# ---- equality (b): the extended code on the engines as they were ------------------------------------------------------
def extended_code(HX, HZ):
    mX, mZ = HX.shape[0], HZ.shape[0]
    EX = np.concatenate([HX, np.eye(mX, dtype=np.uint8), np.zeros((mX, mZ), dtype=np.uint8)], axis=1)
    EZ = np.concatenate([HZ, np.zeros((mZ, mX), dtype=np.uint8), np.eye(mZ, dtype=np.uint8)], axis=1)
    return q.Quantum_LDPC_Code.createFromMatrices(np.ascontiguousarray(EX), np.ascontiguousarray(EZ))


def assert_equals_the_extended_code(base, HX, HZ, sX, sZ, qX, qZ, piX, piZ, schedule, cases, what):
    """`base` with syndrome priors against DecoderCPU on the extended code under per-column priors."""
    n, mX, mZ = HX.shape[1], HX.shape[0], HZ.shape[0]
    ext = extended_code(HX, HZ)
    for sec in (0, 1):
        assert np.array_equal(ext.layers(sec), base.layers(sec)), (what, "layers", sec)
    dx = [int(r.sum()) for r in HX] + [int(r.sum()) for r in HZ]
    D, De = base.stride, ext.stride
    assert De == D + 1
    half = np.full(mX + mZ, 0.5, dtype=F32)  # a variable in no check of the sector: any prior
    pX = np.concatenate([piX, qX, half[:mZ]]).astype(F32)
    pZ = np.concatenate([piZ, half[:mX], qZ]).astype(F32)
    old = minsum_cpu(ext, 160, (pX, pZ))
    old.set_option("minsum_schedule", SCHEDULES.index(schedule))
    new = soft_cpu(base, qX, qZ, 160, (piX, piZ), schedule)
    for stop, N in cases:
        g = soft_decode(new, sX, sZ, 0.3, N, stop)
        w = old.decode_batch(sX, sZ, 0.3, N, stop, want_iters=True, want_q=True)
        tag = (what, schedule, stop, N)
        assert np.array_equal(g[0], w[0][:, :n]) and np.array_equal(g[1], w[1][:, :n]), tag
        assert np.array_equal(g[5], w[0][:, n:n + mX]) and np.array_equal(g[6], w[1][:, n + mX:]), tag
        bit = q.SYNDROME_FAIL_X | q.SYNDROME_FAIL_Z
        assert np.array_equal(g[2] & bit, w[2] & bit) and np.array_equal(g[3], w[3]), tag
        gq, wq = g[4].reshape(len(sX), mX + mZ, D), w[4].reshape(len(sX), mX + mZ, De)
        for c, dc in enumerate(dx):
            assert same_floats(gq[:, c, :dc], wq[:, c, :dc]), tag + (c,)
            assert not gq[:, c, dc:].view(U32).any(), tag + (c, "unused slots")
    return new


EXT_CASES = (("fixed", 0), ("fixed", 1), ("fixed", 11), ("syndrome", 20), ("syndrome", 11))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ("P7", "hgp_ham", "r3-3-6-13", "r4-5-10-7"))
def test_equals_the_extended_code(name, schedule):
    HX, HZ = soft_matrices(name)
    sX, sZ, qX, qZ = soft_inputs(name)
    n = HX.shape[1]
    uniform = np.full(n, F32(2.0) / F32(3.0) * F32(0.03), dtype=F32)
    for piX, piZ in ((uniform, uniform), prior_vectors(n, "random")):
        for route in soft_routes(name):
            assert_equals_the_extended_code(soft_code(name, route), HX, HZ, sX, sZ, qX, qZ, piX, piZ, schedule, EXT_CASES,
                                            (name, route))


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_equals_the_extended_code_on_p61(schedule):
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P61))
    HX, HZ = code.pcm(0), code.pcm(1)
    from oracle.philox import depolarizing
    x, z = depolarizing(5, 0, 12, code.n, 0.02)
    qX, qZ = syndrome_priors(HX.shape[0], 31), syndrome_priors(HZ.shape[0], 32)
    sX, sZ = flipped(code.syndrome(0, x), qX, 41), flipped(code.syndrome(1, z), qZ, 42)
    uniform = np.full(code.n, F32(2.0) / F32(3.0) * F32(0.02), dtype=F32)
    new = assert_equals_the_extended_code(code, HX, HZ, sX, sZ, qX, qZ, uniform, uniform, schedule,
                                          (("fixed", 5), ("syndrome", 20)), "P61")
    assert soft_decode(new, sX, sZ, 0.02, 20, "syndrome")[5].any()


# ---- equality (a) and the special values ------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ("mid", "r3-3-6-13", "P7"))
def test_q_zero_equals_the_call_without_syndrome_priors(name, schedule):
    sX, sZ, _, _ = soft_inputs(name)  # the row with an entry > 1 among them
    assert (np.asarray(sX) > 1).any() and (np.asarray(sZ) > 1).any()
    code = soft_code(name, soft_routes(name)[0])
    plain = minsum_cpu(code)
    plain.set_option("minsum_schedule", SCHEDULES.index(schedule))
    soft = soft_cpu(code, 0.0, 0.0, 160, None, schedule)
    for stop in STOPS:
        for N in NS:
            want = plain.decode_batch(sX, sZ, 0.03, N, stop, want_iters=True, want_q=True)
            got = soft_decode(soft, sX, sZ, 0.03, N, stop)
            assert_same_decode(got, want, "%s %s %s N=%d" % (name, schedule, stop, N))
            assert not got[5].any() and not got[6].any()
            none = soft_decode(plain, sX, sZ, 0.03, N, stop)  # the soft call of a handle without syndrome priors
            assert_same_decode(none, want, "no priors")
            assert not none[5].any() and not none[6].any()
    soft.set_syndrome_priors(None, None)
    assert soft.get_syndrome_priors() is None and "soft" not in soft.describe()
    assert_same_decode(soft.decode_batch(sX, sZ, 0.03, 11, "fixed", want_iters=True, want_q=True),
                       plain.decode_batch(sX, sZ, 0.03, 11, "fixed", want_iters=True, want_q=True), "cleared")
    assert "soft" not in soft.last_path()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_special_values_in_a_vector(schedule):
    """q in {0, 1/2, 1} mixed into a vector: mu = +2^30, +0.0f, -2^30.  Against the yardstick; a check with q = 1 has its
    bit taken as flipped whatever the messages say, one with q = 0 never."""
    name = "r3-3-6-13"
    HX, HZ = soft_matrices(name)
    sX, sZ, qX, qZ = (np.array(a) for a in soft_inputs(name))
    for qs in (qX, qZ):
        qs[0::7], qs[1::7], qs[2::7] = 0.0, 0.5, 1.0
    assert q.minsum_llr(0.5) == 0.0 and np.signbit(F32(q.minsum_llr(0.5))) == False  # noqa: E712
    dec = soft_cpu(soft_code(name, "graph"), qX, qZ, 160, None, schedule)
    for stop, N in (("fixed", 0), ("fixed", 11), ("syndrome", 20), ("ref", 20)):
        want = soft_yardstick(HX, HZ, sX, sZ, 0.05, 0.05, qX, qZ, 160, N, stop, schedule)
        got = soft_decode(dec, sX, sZ, 0.05, N, stop)
        assert_same_soft(got, want, "%s %s N=%d" % (schedule, stop, N))
        assert np.isfinite(got[4]).all()
        assert got[5][:, 2::7].all() and not got[5][:, 0::7].any()
        assert got[6][:, 2::7].all() and not got[6][:, 0::7].any()


# ---- the flip sampler, restated -----------------------------------------------------------------------------------------
def flip_threshold(qc):
    return int(float(F32(qc)) * 4294967296.0)  # floor(q 2^32) in double from the float: q = 1 gives 2^32, q = 0 gives 0


def flip_reference(seed, start, count, qX, qZ):
    """qec_flip_syndrome_dev: -> (fX [count, mX], fZ [count, mZ]).  Sample b makes Philox calls k = 0, 1, ... with counter
    (b lo, b hi, k, FLIP_SALT) and key (seed lo, seed hi); word 4k + j is output j of call k; X check c reads word c, Z
    check c word mX + c; flipped iff word < floor(q 2^32)."""
    qs = np.concatenate([np.asarray(qX, dtype=F32), np.asarray(qZ, dtype=F32)])
    m, mX = len(qs), len(qX)
    calls = (m + 3) // 4
    b = (np.arange(count, dtype=np.uint64) + np.uint64(start))[:, None]
    k = np.arange(calls, dtype=np.uint64)[None, :]
    out = philox4x32_10(b & np.uint64(0xFFFFFFFF), b >> np.uint64(32), k + np.uint64(0) * b, FLIP_SALT + np.uint64(0) * (b + k),
                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(out, axis=2).reshape(count, 4 * calls)[:, :m].astype(np.uint64)
    thr = np.array([flip_threshold(x) for x in qs], dtype=np.uint64)
    f = (words < thr[None, :]).astype(np.uint8)
    return f[:, :mX], f[:, mX:]


def test_flip_reference():
    qX = np.array([0.0, 1.0, 0.5, 0.25, 0.1], dtype=F32)
    qZ = np.array([1.0, 0.0, 0.03], dtype=F32)
    fX, fZ = flip_reference(0x1234567890ABCDEF, 5, 4000, qX, qZ)
    assert not fX[:, 0].any() and fX[:, 1].all() and fZ[:, 0].all() and not fZ[:, 1].any()
    for col, want in ((fX[:, 2], 0.5), (fX[:, 3], 0.25), (fX[:, 4], 0.1), (fZ[:, 2], 0.03)):
        assert abs(col.mean() - want) < 5 * np.sqrt(want * (1 - want) / 4000)  # five standard deviations
    # any shard of the index space can be drawn alone, and a sample index above 2^32 uses the counter's second word
    aX, aZ = flip_reference(0x1234567890ABCDEF, 1005, 100, qX, qZ)
    assert np.array_equal(aX, fX[1000:1100]) and np.array_equal(aZ, fZ[1000:1100])
    hX, _ = flip_reference(7, (1 << 32) + 5, 64, qX, qZ)
    lX, _ = flip_reference(7, 5, 64, qX, qZ)
    assert not np.array_equal(hX, lX)
    assert flip_threshold(1.0) == 1 << 32 and flip_threshold(0.0) == 0
    # the first word of the stream, pinned against the generator itself
    w = philox4x32_10(np.uint64(3), np.uint64(0), np.uint64(0), np.uint64(FLIP_SALT), 9, 0)[0]
    fX1, _ = flip_reference(9, 3, 1, np.array([0.5], dtype=F32), np.zeros(0, dtype=F32))
    assert int(fX1[0, 0]) == int(int(w) < (1 << 31))


# ---- the public interface ------------------------------------------------------------------------------------------------
def expect(code, f, *args):
    with pytest.raises(q.QecError) as e:
        f(*args)
    assert "(%d)" % code in str(e.value), str(e.value)


ERR_ARG, ERR_UNSUPPORTED = -1, -4


def test_error_codes_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qec_ldpc.h")).read()
    assert int(re.search(r"QEC_ERR_ARG\s*=\s*(-?\d+)", text).group(1)) == ERR_ARG
    assert int(re.search(r"QEC_ERR_UNSUPPORTED\s*=\s*(-?\d+)", text).group(1)) == ERR_UNSUPPORTED
    assert int(re.search(r"QEC_PATH_SOFT\s*=\s*(\d+)", text).group(1)) == 16384 == q.PATH["soft"]


def test_round_trip_validation_and_describe():
    code = soft_code("r3-3-6-13", "graph")
    mX, mZ = code.numEqsX, code.numEqsZ
    dec = minsum_cpu(code)
    assert dec.get_syndrome_priors() is None
    qX, qZ = syndrome_priors(mX, 1), syndrome_priors(mZ, 2)
    dec.set_syndrome_priors(qX, qZ)
    gX, gZ = dec.get_syndrome_priors()
    assert np.array_equal(gX, qX) and np.array_equal(gZ, qZ)
    assert dec.describe().endswith("[soft syndrome]")
    # an illegal value leaves the handle as it was
    for bad in (-0.01, 1.5, float("nan")):
        b = qX.copy()
        b[3] = bad
        expect(ERR_ARG, dec.set_syndrome_priors, b, qZ)
        expect(ERR_ARG, dec.set_syndrome_priors, qX, np.full(mZ, bad, dtype=F32))
    expect(ERR_ARG, lambda: q._check(q.lib().qec_decoder_set_syndrome_priors(dec._h, q._ptr(qX), None), "one NULL"))
    with pytest.raises(q.QecError):
        dec.set_syndrome_priors(qX, None)
    with pytest.raises(q.QecError):
        dec.set_syndrome_priors(qX[:-1], qZ)
    gX, gZ = dec.get_syndrome_priors()
    assert np.array_equal(gX, qX) and np.array_equal(gZ, qZ)
    dec.set_syndrome_priors(0.125, 0.25)  # scalars
    gX, gZ = dec.get_syndrome_priors()
    assert (gX == F32(0.125)).all() and (gZ == F32(0.25)).all()
    dec.set_syndrome_priors(None, None)
    assert dec.get_syndrome_priors() is None and "soft" not in dec.describe()


def test_refusals_in_both_orders():
    code = soft_code("r3-3-6-13", "graph")
    qs = (0.05, 0.05)
    gam = q.relay_gammas(code.n, 2)
    # bp_method: the priors need 1, and 0 is refused while they are set
    dec = q.DecoderCPU(code)
    expect(ERR_UNSUPPORTED, dec.set_syndrome_priors, *qs)
    assert dec.get_syndrome_priors() is None
    dec.set_option("bp_method", 1)
    dec.set_syndrome_priors(*qs)
    expect(ERR_UNSUPPORTED, dec.set_option, "bp_method", 0)
    assert dec.get_option("bp_method") == 1 and dec.get_syndrome_priors() is not None
    # relay tables
    expect(ERR_UNSUPPORTED, dec.set_relay, gam, gam)
    assert dec.get_relay() is None
    dec.set_syndrome_priors(None, None)
    dec.set_relay(gam, gam)
    expect(ERR_UNSUPPORTED, dec.set_syndrome_priors, *qs)
    assert dec.get_syndrome_priors() is None and dec.get_relay() is not None
    dec.set_relay(None, None)
    # the OSD stage
    dec.set_syndrome_priors(*qs)
    expect(ERR_UNSUPPORTED, dec.set_option, "osd", 1)
    assert dec.get_option("osd") == 0
    dec.set_syndrome_priors(None, None)
    dec.set_option("osd", 1)
    expect(ERR_UNSUPPORTED, dec.set_syndrome_priors, *qs)
    assert dec.get_syndrome_priors() is None
    dec.set_option("osd", 0)
    dec.set_syndrome_priors(*qs)
    # qec_osd as a separate call is untouched
    sX, sZ, _, _ = soft_inputs("r3-3-6-13")
    out = dec.decode_batch(sX, sZ, 0.05, 3, "fixed", want_q=True)
    dec.osd(sX, sZ, out[4], out[0], out[1], out[2])
    # min-sum's own refusals stand: the correlated form and the serial schedule refuse min-sum, so they never meet
    expect(ERR_UNSUPPORTED, dec.set_option, "correlated", 1)
    expect(ERR_UNSUPPORTED, dec.set_option, "bp_schedule", 1)
    # the soft call is a min-sum call
    prod = q.DecoderCPU(code)
    with pytest.raises(q.QecError):
        prod.decode_batch(sX, sZ, 0.05, 3, "fixed", want_flips=True)


# ---- GetStatistics and the CLI on the CPU engine ----------------------------------------------------------------------
def test_cli_flags_on_the_cpu_engine(tmp_path):
    """--syndrome-noise Q and --syndrome-priors FILE reproduce the Python counters of GetStatistics under syndrome
    priors; inconsistent flags exit with status 2."""
    from test_osd_host import _cli, _fields
    path = code_path(P7)
    code = q.Quantum_LDPC_Code.createFromFile(path)
    W, B, N, p, seed = 3, 1500, 20, 0.02, 7
    base = ["--engine", "cpu", "--seed", str(seed), "--bp-method", "minsum"]
    keys = {"Corrected": "corrected", "Syndrome Errors X": "syndromeErrorsX", "Syndrome Errors Z": "syndromeErrorsZ",
            "Logical Errors": "logicalErrors", "Convergence Fail X": "convergenceFailX",
            "Convergence Fail Z": "convergenceFailZ", "Errors Tested": "numErrorsTested"}
    qX, qZ = syndrome_priors(code.numEqsX, 3), syndrome_priors(code.numEqsZ, 4)
    table = tmp_path / "q.txt"
    table.write_text(" ".join("%.9g" % x for x in qX) + "\n" + " ".join("%.9g" % x for x in qZ) + "\n")
    out = {}
    for tag, flags, pri in (("plain", [], None), ("noise", ["--syndrome-noise", "0.125"], (0.125, 0.125)),
                            ("file", ["--syndrome-priors", str(table)], (qX, qZ))):
        d = tmp_path / tag
        d.mkdir()
        r = _cli(d, base + flags, path, "%d %d %d %d %g" % (W, W, B, N, p))
        assert r.returncode == 0, r.stderr
        f = _fields(d)
        dec = minsum_cpu(code)
        if pri is not None:
            dec.set_syndrome_priors(*pri)
        tested = int(f["Errors Tested"])
        assert B // 2 < tested <= B
        st = dec.GetStatistics(W, tested, p, N, seed=seed)
        assert ("soft" in dec.last_path()) == (pri is not None)
        out[tag] = {k: int(f[k]) for k in keys}
        assert out[tag] == {k: st[v] for k, v in keys.items()}, tag
    assert out["noise"] != out["plain"] and out["file"] != out["plain"]
    short = tmp_path / "short.txt"
    short.write_text("0.1 0.1\n0.1\n")
    bad = (["--engine", "cpu", "--syndrome-noise", "0.1"],  # without min-sum
           base + ["--syndrome-noise", "1.5"], base + ["--syndrome-noise", "x"],
           base + ["--syndrome-noise", "0.1", "--syndrome-priors", str(table)],
           base + ["--syndrome-noise", "0.1", "--osd", "0"])
    for k, flags in enumerate(bad):
        d = tmp_path / ("bad%d" % k)
        d.mkdir()
        assert _cli(d, flags, path, "3 3 10 20 0.02").returncode == 2, flags
    d = tmp_path / "short"
    d.mkdir()
    assert _cli(d, base + ["--syndrome-priors", str(short)], path, "3 3 10 20 0.02").returncode == 1


# ---- the table of circulant block shapes (shared with tests/test_gpu_wave_soft_syndrome.py) ---------------------------
from test_circulant_shapes import KINDS, PS, groups, shape_id  # noqa: E402
from test_circulant_shapes import SHAPES as TABLE_SHAPES  # noqa: E402
from test_circulant_shapes import code_of as table_code_of  # noqa: E402
from test_circulant_shapes import inputs as table_syndromes  # noqa: E402
from test_wave_minsum import DECODE_CASES, SYN20, wave_mixes  # noqa: E402

_table_inputs, _table_cpu, _table_ref = {}, {}, {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("soft_syndrome")


def table_inputs(tmp, shape, P, kind="table"):
    """(sX, sZ, qX, qZ) of a table row: the batch of tests/test_circulant_shapes.py with its odd rows measured through the
    channel q."""
    key = (shape, P, kind)
    if key not in _table_inputs:
        code = table_code_of(tmp, shape, P)[0]
        qX, qZ = syndrome_priors(code.numEqsX, 100 + P), syndrome_priors(code.numEqsZ, 200 + P)
        sX, sZ = table_syndromes(tmp, shape, P, kind)
        fX, fZ = flipped(sX, qX, 300 + P), flipped(sZ, qZ, 400 + P)
        odd = (np.arange(len(sX)) % 2 == 1)[:, None]  # every other row as it was: rows that stop early stay among them
        out = (np.where(odd, fX, sX).astype(np.uint8), np.where(odd, fZ, sZ).astype(np.uint8), qX, qZ)
        for a in out:
            a.setflags(write=False)
        _table_inputs[key] = out
    return _table_inputs[key]


def table_reference(tmp, shape, P, case, kind="table", priors=None, schedule="flooding"):
    """The CPU engine's (eX, eZ, flags, iters, q_final, fX, fZ) of a decode case under syndrome priors, computed once.
    priors: None or a kind of test_priors.prior_vectors."""
    key = (shape, P, case, kind, priors, schedule)
    if key not in _table_ref:
        stop, p, N = case
        code = table_code_of(tmp, shape, P)[0]
        sX, sZ, qX, qZ = table_inputs(tmp, shape, P, kind)
        ck = (shape, P, schedule)
        if ck not in _table_cpu:
            _table_cpu[ck] = soft_cpu(code, qX, qZ, 160, None, schedule)
        dec = _table_cpu[ck]
        try:
            if priors is not None:
                dec.set_priors(*prior_vectors(code.n, priors))
            out = soft_decode(dec, sX, sZ, p, N, stop)
        finally:
            dec.set_priors(None, None)
        for a in out:
            a.setflags(write=False)
        _table_ref[key] = out
    return _table_ref[key]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("shape", TABLE_SHAPES, ids=shape_id)
def test_table_reference_is_not_vacuous(tmp, shape, schedule):
    """On the reference of every table row: finite messages, f bits set in both sectors, both outcomes of the syndrome
    stop, and with several groups per wave (G > 1) groups of one wave that stop at different iterations -- what the
    freeze of the wave kernels has to keep apart."""
    for P in PS:
        G = groups(P)
        syn = table_reference(tmp, shape, P, SYN20, "table", None, schedule)
        assert np.isfinite(syn[4]).all()
        assert syn[5].any() and syn[6].any(), (shape, P)
        seen = set(int(x) for x in syn[3].ravel())
        assert min(seen) < 20 and 20 in seen, (shape, P, seen)
        if G > 1:
            mixes = [wave_mixes(table_reference(tmp, shape, P, SYN20, kind, None, schedule)[3], G) for kind in KINDS]
            assert any(any(m) for m in mixes), (shape, P, mixes)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_table_reference_matches_the_yardstick(tmp, schedule):
    """The CPU engine on table codes against numpy (column weight 2 among them)."""
    for shape, P in (((2, 2, 4), 3), ((3, 3, 6), 9)):
        code = table_code_of(tmp, shape, P)[0]
        sX, sZ, qX, qZ = table_inputs(tmp, shape, P)
        for case in (("fixed", 0.03, 11), SYN20, ("ref", 0.005, 21)):
            stop, p, N = case
            want = soft_yardstick(code.pcm(0), code.pcm(1), sX, sZ, p, p, qX, qZ, 160, N, stop, schedule)
            assert_same_soft(table_reference(tmp, shape, P, case, "table", None, schedule), want, (shape, P, case))

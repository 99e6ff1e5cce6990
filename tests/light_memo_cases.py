"""Error sets for the light-sector table tests (QEC_OPT_LIGHT_MEMO) and the
numpy restatement of a sector's class key.  Not a test module."""
import numpy as np


def var_lane(E, P, l, j):
    """Variable-view lane mu of qubit (l, j): the kernels' lane relabelling takes C[l] = E[0][l]."""
    return (j - int(E[0][l])) % P


def checks_of(E, P, l, j):
    """The checks (r, c) of qubit (l, j): check (r, c) holds column (E[r][l] + c) mod P of block l."""
    return [(r, (j - int(E[r][l])) % P) for r in range(E.shape[0])]


def class_key(E, P, qubits):
    """The class of a one- or two-error set of one sector: (l,) or (l1, l2, d), invariant under a cyclic shift of
    every qubit's position: columns ascending, d the lane difference (second minus first) mod P; two errors of one
    column are the same set read from either end, so their d is the smaller of d and P - d."""
    v = sorted((l, var_lane(E, P, l, j)) for l, j in qubits)
    if len(v) == 1:
        return (v[0][0],)
    (l1, m1), (l2, m2) = v
    d = (m2 - m1) % P
    return (l1, l2, min(d, P - d) if l1 == l2 else d)


def lookup_key(E, P, qubits):
    """The table index the kernel forms: candidates in ascending (column, lane) order, d = second - first mod P."""
    v = sorted((l, var_lane(E, P, l, j)) for l, j in qubits)
    if len(v) == 1:
        return (v[0][0],)
    (l1, m1), (l2, m2) = v
    return (l1, l2, (m2 - m1) % P)


def representative(E, P, key):
    """The qubits of the table row of a lookup key: lane 0 of column l1 and lane d of column l2."""
    if len(key) == 1:
        return [(key[0], int(E[0][key[0]]) % P)]
    l1, l2, d = key
    return [(l1, int(E[0][l1]) % P), (l2, (d + int(E[0][l2])) % P)]


def shifted(P, qubits, k):
    return [(l, (j + k) % P) for l, j in qubits]


def vec(n, P, qubits):
    e = np.zeros(n, np.uint8)
    for l, j in qubits:
        e[l * P + j] ^= 1
    return e


def share_a_check(E, P, a, b):
    return bool(set(checks_of(E, P, *a)) & set(checks_of(E, P, *b)))


def pair_sets(E, P, L, count, seed):
    """`count` two-error sets of one sector: for every column pair the lane differences 1 and P - 1, same-column
    pairs, pairs that share a check, then random ones."""
    rng = np.random.default_rng(seed)
    R = E.shape[0]
    out = []
    for l1 in range(L):
        for l2 in range(l1, L):
            for d in (1, P - 1):
                j1 = int(rng.integers(P))
                m2 = (var_lane(E, P, l1, j1) + d) % P
                out.append([(l1, j1), (l2, (m2 + int(E[0][l2])) % P)])
    for l in range(L):  # one column, assorted distances
        j = int(rng.integers(P))
        out += [[(l, j), (l, (j + d) % P)] for d in (2, 30, 31, P - 2)]
    for r in range(R):  # two qubits of one check
        for _ in range(8):
            c = int(rng.integers(P))
            l1, l2 = (int(x) for x in rng.choice(L, 2, replace=False))
            pair = [(l1, (int(E[r][l1]) + c) % P), (l2, (int(E[r][l2]) + c) % P)]
            assert share_a_check(E, P, *pair)
            out.append(pair)
    while len(out) < count:
        a, b = (int(x) for x in rng.choice(L * P, 2, replace=False))
        out.append([(a // P, a % P), (b // P, b % P)])
    return out[:count]


def triple_sets_weight_2R(E, P, L, count, seed):
    """Three-error sets whose syndrome has weight 2R (R even): a chain a - b - c in which a, b share one check, b, c
    another and a, c none, so 3R - 4 = 2R needs R = 4; for other R the sets are three random qubits."""
    rng = np.random.default_rng(seed)
    R = E.shape[0]
    out = []
    while len(out) < count:
        if 3 * R - 4 != 2 * R:
            t = [int(x) for x in rng.choice(L * P, 3, replace=False)]
            out.append([(x // P, x % P) for x in t])
            continue
        r1, r2 = (int(x) for x in rng.choice(R, 2, replace=False))
        c1 = int(rng.integers(P))
        la, lb, lc = (int(x) for x in rng.choice(L, 3, replace=False))
        a = (la, (int(E[r1][la]) + c1) % P)
        b = (lb, (int(E[r1][lb]) + c1) % P)
        c2 = dict(checks_of(E, P, *b))[r2]
        c = (lc, (int(E[r2][lc]) + c2) % P)
        if share_a_check(E, P, a, c) or len({a, b, c}) < 3:
            continue
        if len(set(checks_of(E, P, *a)) ^ set(checks_of(E, P, *b)) ^ set(checks_of(E, P, *c))) != 2 * R:
            continue
        out.append([a, b, c])
    return out

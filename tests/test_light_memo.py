"""The light-sector table (QEC_OPT_LIGHT_MEMO) without a GPU: the class key of a
one- or two-error set of a P61 sector, restated in numpy, is the key of the set shifted by any number of lanes; the
table row the kernel would read holds a shift of the set; a shift of the error set shifts its syndrome block by
block; and the option is declared where the other exact shortcuts are."""
import numpy as np

import qec_ldpc_amd as q
from light_memo_cases import (checks_of, class_key, lookup_key, pair_sets, representative, share_a_check, shifted,
                              triple_sets_weight_2R, vec)
from qec_ldpc_amd.codes import P61, code_path

P, L = 61, 10


def p61():
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P61))
    return code, [np.asarray(code.exponents(sec)) for sec in (0, 1)]


def test_class_key_is_shift_invariant():
    _, Es = p61()
    for sec, E in enumerate(Es):
        sets = [[(l, j)] for l in range(L) for j in (0, 17, P - 1)] + pair_sets(E, P, L, 300, seed=5 + sec)
        keys = set()
        for s in sets:
            k0 = class_key(E, P, s)
            keys.add(k0)
            for k in range(P):
                t = shifted(P, s, k)
                assert class_key(E, P, t) == k0, (sec, s, k)
                # the row the kernel reads for the shifted set is some shift of the set
                rep = sorted(representative(E, P, lookup_key(E, P, t)))
                assert any(sorted(shifted(P, s, m)) == rep for m in range(P)), (sec, s, k)
        assert len(keys) > 200  # the sample spans many classes


def test_shifted_errors_shift_the_syndrome():
    """H is block-circulant: moving every error k positions along its block moves every block row of the syndrome
    k positions, which is what makes the decode of the shifted syndrome the shifted decode."""
    code, Es = p61()
    rng = np.random.default_rng(3)
    for sec, E in enumerate(Es):
        R = E.shape[0]
        for s in pair_sets(E, P, L, 40, seed=9 + sec):
            base = code.syndrome(sec, vec(code.n, P, s)[None])[0].reshape(R, P)
            k = int(rng.integers(1, P))
            moved = code.syndrome(sec, vec(code.n, P, shifted(P, s, k))[None])[0].reshape(R, P)
            assert np.array_equal(moved, np.roll(base, k, axis=1))
            want = 2 * R - 2 * len(set(checks_of(E, P, *s[0])) & set(checks_of(E, P, *s[1])))
            assert base.sum() == want and (want == 2 * R) == (not share_a_check(E, P, *s))


def test_three_error_look_alikes_exist_for_x_only():
    code, Es = p61()
    for sec, E in enumerate(Es):
        R = E.shape[0]
        for s in triple_sets_weight_2R(E, P, L, 10, seed=1):
            w = int(code.syndrome(sec, vec(code.n, P, s)[None]).sum())
            assert (w == 2 * R) == (R == 4), (sec, s, w)


def test_option_declared():
    assert q.OPTION["light_memo"] == 24 and q.lib().qec_abi_version() == 4
    code, _ = p61()
    dec = q.DecoderGPU(code, device=-1)  # the CPU engine keeps the value and decodes as ever
    assert dec.get_option("light_memo") == 1
    dec.set_option("light_memo", 0)
    assert dec.get_option("light_memo") == 0
    dec.set_option("light_memo", 7)
    assert dec.get_option("light_memo") == 1

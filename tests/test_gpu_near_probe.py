"""The near-hard probe (QEC_OPT_NEAR_PROBE) on the GPU, P61: with the probe on and
off the eight fixed- / reference-stop kernels (one launch, split waves, sector launches) give the same records,
flags and iteration counts byte for byte, and the CPU oracle's, at the iteration counts that put an exit next to
the first soft iteration and next to the reference stop's tests, from bit rows and byte rows, as records and byte
outputs, with the light-sector table on and off (off: the light sectors leave through the probe); also where the
probe passes and the syndrome half fails (an entry 2), far above the threshold (p = 0.2, 0.3), with final messages
requested, and on kernels compiled without the probe (P7, a runtime-shift code)."""
import functools

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import P7, P61, code_path
from qec_ldpc_amd.gather import pack_records
from qec_ldpc_amd.synthetic import depolarizing_errors
from test_circulant_shapes import write_file
from test_gpu_near_hard_jump import decode, with_options

pytestmark = pytest.mark.gpu

B = 383  # P61: 383 one-group waves, the shape of the near-hard tests
NS = (2, 3, 4, 11, 12, 21, 50)
FORMS = ("bytes", "rec_bytes", "rec_bits")


@functools.lru_cache(maxsize=None)
def setup(path):
    code = q.Quantum_LDPC_Code.createFromFile(path)
    return code, q.DecoderGPU(code, 0), OracleCode(path)


@functools.lru_cache(maxsize=None)
def syndromes(path, p, count=B):
    """count - 2 depolarising syndromes, an all-zero one and a single-bit one."""
    code = setup(path)[0]
    x, z = depolarizing_errors(code.n, 20253, count - 2, p)
    sX = np.concatenate([code.syndrome(0, x), np.zeros((2, code.numEqsX), np.uint8)])
    sZ = np.concatenate([code.syndrome(1, z), np.zeros((2, code.numEqsZ), np.uint8)])
    sX[-1, 3] = 1
    sZ[-1, 1] = 1
    return sX, sZ


@functools.lru_cache(maxsize=None)
def expected(path, p, N, stop, count=B):
    sX, sZ = syndromes(path, p, count)
    o = setup(path)[2].decode_batch(sX, sZ, p, N, stop)
    return pack_records(o[0], o[1], o[2]), o[3]


def on_off(dec, code, sX, sZ, p, N, stop, form, rec, its, what, **opts):
    got = {}
    for probe in (1, 0):
        with with_options(dec, near_probe=probe, **opts):
            got[probe] = decode(dec, code, sX, sZ, p, N, stop, form)
    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), ("on / off", what)
    assert np.array_equal(got[1][0], rec), ("records", what, np.flatnonzero((got[1][0] != rec).any(1))[:8])
    assert np.array_equal(got[1][1], its), ("iters", what, np.flatnonzero((got[1][1] != its).any(1))[:8])


@pytest.mark.parametrize("stop", ["fixed", "ref"])
@pytest.mark.parametrize("N", NS)
def test_probe_on_off_oracle(stop, N):
    path = code_path(P61)
    code, dec, _ = setup(path)
    assert dec.get_option("near_probe") == 1 and dec.get_option("near_hard") == 1
    sX, sZ = syndromes(path, 0.01)
    rec, its = expected(path, 0.01, N, stop)
    for split in (0, 2, 3):
        for memo in (0, 1):
            for form in FORMS:
                on_off(dec, code, sX, sZ, 0.01, N, stop, form, rec, its, (stop, N, split, memo, form),
                       sector_split=split, light_memo=memo)
    on_off(dec, code, sX[:1], sZ[:1], 0.01, N, stop, "rec_bits", rec[:1], its[:1], (stop, N, "one syndrome"))


def test_most_sectors_leave_at_the_first_soft_iteration():
    """What the probe is for: at p = 0.01 the fixed-stop count of nearly every sector is 50 with both flags clear
    (the oracle's word), i.e. the sectors the kernels end by the jump; the instrumented kernels, which carry no
    probe, count the same phases with the option on and off."""
    path = code_path(P61)
    code, dec, _ = setup(path)
    sX, sZ = syndromes(path, 0.01)
    w = {}
    for probe in (1, 0):
        with with_options(dec, near_probe=probe, phase_stats=1):
            w[probe] = decode(dec, code, sX, sZ, 0.01, 50, "fixed", "rec_bits")[1].astype(np.uint32)
    assert np.array_equal(w[1], w[0])
    jumped = (w[1] >> 24) > 0
    assert jumped.mean() > 0.5, jumped.mean()


def test_probe_passes_and_the_syndrome_half_fails():
    """Single-error syndromes with one set entry written as 2: every message settles on the sides of that error, so
    the fold test passes, but a sector with an entry other than 0 / 1 fails every syndrome test; the ordinary pass
    must run and the sector must not leave.  Byte rows (bit rows cannot hold the 2)."""
    path = code_path(P61)
    code, dec, orc = setup(path)
    n = 24
    x = np.zeros((n, code.n), np.uint8)
    z = np.zeros((n, code.n), np.uint8)
    rng = np.random.default_rng(5)
    x[np.arange(n), rng.integers(0, code.n, n)] = 1
    z[np.arange(n), rng.integers(0, code.n, n)] = 1
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    for i in range(0, n, 2):  # every other row; the rows between stay light
        sX[i, np.flatnonzero(sX[i])[i % 4]] = 2
        sZ[i, np.flatnonzero(sZ[i])[i % 5]] = 2
    for stop in ("fixed", "ref"):
        for N in (3, 12, 50):
            o = orc.decode_batch(sX, sZ, 0.01, N, stop)
            rec, its = pack_records(o[0], o[1], o[2]), o[3]
            assert (o[2][::2] & (q.SYNDROME_FAIL_X | q.SYNDROME_FAIL_Z)).all()
            for split in (0, 2, 3):
                for memo in (0, 1):
                    for form in ("bytes", "rec_bytes"):
                        on_off(dec, code, sX, sZ, 0.01, N, stop, form, rec, its, (stop, N, split, memo, form),
                               sector_split=split, light_memo=memo)


@pytest.mark.parametrize("p", [0.2, 0.3])
def test_high_p(p):
    """Far above the threshold few sectors ever come near a hard state (qec_near_hard_threshold still gives an eps0 for
    these p', 2^-8, so the probe runs and fails in nearly every pass): the ordinary pass behind a failed probe."""
    path = code_path(P61)
    code, dec, _ = setup(path)
    sX, sZ = syndromes(path, p, 64)
    for stop in ("fixed", "ref"):
        for N in (3, 12):
            rec, its = expected(path, p, N, stop, 64)
            for split in (0, 3):
                on_off(dec, code, sX, sZ, p, N, stop, "rec_bits", rec, its, (p, stop, N, split), sector_split=split)


def test_final_messages_requested():
    """A call that asks for the final messages never jumps, so never probes: messages equal bit for bit."""
    path = code_path(P61)
    code, dec, orc = setup(path)
    sX, sZ = syndromes(path, 0.01)
    sX, sZ = sX[-48:], sZ[-48:]
    for stop in ("fixed", "ref"):
        for N in (3, 12):
            o = orc.decode_batch(sX, sZ, 0.01, N, stop, want_q=True)
            got = {}
            for probe in (1, 0):
                with with_options(dec, near_probe=probe):
                    got[probe] = dec.decode_batch(sX, sZ, 0.01, N, stop, want_iters=True, want_q=True)
            for a, b, c in zip(got[1], got[0], o):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (stop, N, "on / off")
                # against the oracle a NaN matches a NaN (the single-bit row ends in 0 / 0; the sign of that NaN is
                # the divider's), every other message bit for bit
                nan = np.isnan(a) if a.dtype == np.float32 else np.zeros(a.shape, bool)
                assert np.array_equal(nan, np.isnan(c) if a.dtype == np.float32 else nan), (stop, N)
                assert np.array_equal(a[~nan].view(np.uint8), c[~nan].view(np.uint8)), (stop, N, "oracle")


def test_probe_needs_the_jump():
    """near_hard = 0 switches the probe off with the jump: the same outputs."""
    path = code_path(P61)
    code, dec, _ = setup(path)
    sX, sZ = syndromes(path, 0.01)
    rec, its = expected(path, 0.01, 12, "fixed")
    for opts in ({"near_hard": 0}, {"hard_paths": 0}, {"cycle_jump": 0}):
        on_off(dec, code, sX, sZ, 0.01, 12, "fixed", "rec_bits", rec, its, opts, **opts)


def test_kernels_without_the_probe(tmp_path):
    """P7 (nine groups per wave) and a runtime-shift code (J = 4, K = 5, L = 10 at P = 33) are compiled without the
    probe: the option changes nothing there."""
    for path, p in ((code_path(P7), 0.02), (write_file(tmp_path, (4, 5, 10), 33), 0.01)):
        code, dec, _ = setup(path)
        sX, sZ = syndromes(path, p, 200)
        for stop in ("fixed", "ref"):
            for N in (3, 12, 21):
                rec, its = expected(path, p, N, stop, 200)
                for form in ("bytes", "rec_bits"):
                    on_off(dec, code, sX, sZ, p, N, stop, form, rec, its, (path, stop, N, form))

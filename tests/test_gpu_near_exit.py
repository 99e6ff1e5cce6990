"""The near-hard exit straight to the outputs, and iteration 0 without the dead initialisation (DESIGN.md
section 4.1 item 15, section 7.1 "Near-hard exit"): a sector that leaves through the near-hard jump keeps its
soft registers and its outputs come from the fast branch (every live group of the wave near-exited) or the
general branch (a wave that also holds groups which stopped another way); the p' fill runs only when iteration
0 is not made by table.  Everything is held to the oracle: records and iteration counts over the exit paths,
a batch with many mixed waves, N = 1 .. 3 with and without the final messages, and the instrumented kernels'
phase counts against the ones recorded before the change (tests/golden/near_exit_phases.json)."""
import functools
import json
import os

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import P7, P61, code_path
from qec_ldpc_amd.gather import pack_records
from qec_ldpc_amd.synthetic import depolarizing_errors

pytestmark = pytest.mark.gpu

KEYS = {"P7": P7, "P61": P61}
B_RAGGED = 383  # P61: 383 one-group waves; P7: 42 waves of nine groups and one of five (idle lanes)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "near_exit_phases.json")


@functools.lru_cache(maxsize=None)
def setup(key):
    path = code_path(KEYS[key])
    code = q.Quantum_LDPC_Code.createFromFile(path)
    return code, q.DecoderGPU(code, 0), OracleCode(path)


@functools.lru_cache(maxsize=None)
def syndromes(key, p):
    """381 depolarising syndromes, an all-zero one and a single-bit one (the near-hard test's batch)."""
    code = setup(key)[0]
    x, z = depolarizing_errors(code.n, 20252, B_RAGGED - 2, p)
    sX = np.concatenate([code.syndrome(0, x), np.zeros((2, code.numEqsX), np.uint8)])
    sZ = np.concatenate([code.syndrome(1, z), np.zeros((2, code.numEqsZ), np.uint8)])
    sX[-1, 7] = 1
    sZ[-1, 0] = 1
    return sX, sZ


@functools.lru_cache(maxsize=None)
def expected(key, p, N, stop, want_q=False):
    """The oracle's records, iteration counts and (on request) final messages, computed once per point."""
    sX, sZ = syndromes(key, p)
    o = setup(key)[2].decode_batch(sX, sZ, p, N, stop, want_q=want_q)
    return pack_records(o[0], o[1], o[2]), o[3], o[4]


def bit_rows(s):
    import torch
    B, m = s.shape
    pk = np.packbits(s, axis=1, bitorder="little")
    pad = np.zeros((B, 4 * ((m + 31) // 32)), np.uint8)
    pad[:, :pk.shape[1]] = pk
    return torch.from_numpy(pad.view(np.int32).copy()).to("cuda:0")


def decode(dec, code, sX, sZ, p, N, stop, form):
    """One device-buffer decode -> (records, iters) as numpy; form: byte outputs, or records from bit rows."""
    import torch
    dev = torch.device("cuda", 0)
    B = len(sX)
    its = torch.empty((B, 2), dtype=torch.int32, device=dev)
    if form == "rec_bits":
        rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
        dec.decode_bits_packed_dev(bit_rows(sX), bit_rows(sZ), p, N, stop, rec, its)
        torch.cuda.synchronize()
        return rec.cpu().numpy(), its.cpu().numpy()
    assert form == "bytes"
    dX, dZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
    eX = torch.empty((B, code.n), dtype=torch.uint8, device=dev)
    eZ = torch.empty((B, code.n), dtype=torch.uint8, device=dev)
    fl = torch.empty((B,), dtype=torch.uint8, device=dev)
    dec.decode_batch_dev(dX, dZ, p, N, stop, eX, eZ, fl, its)
    torch.cuda.synchronize()
    return pack_records(eX.cpu().numpy(), eZ.cpu().numpy(), fl.cpu().numpy()), its.cpu().numpy()


class with_options:
    def __init__(self, dec, **opts):
        self.dec, self.opts = dec, opts

    def __enter__(self):
        self.old = {k: self.dec.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.dec.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.dec.set_option(k, v)


def phases(dec, code, sX, sZ, p, N, stop, **opts):
    """Per sector (soft, hard, agreed, jumped) iteration counts of the instrumented kernels: [B, sector, phase]."""
    with with_options(dec, phase_stats=1, **opts):
        w = decode(dec, code, sX, sZ, p, N, stop, "rec_bits")[1].astype(np.uint32)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24], -1)


@pytest.mark.parametrize("key", ["P7", "P61"])
@pytest.mark.parametrize("stop", ["fixed", "ref"])
@pytest.mark.parametrize("N", [3, 12, 50])
def test_exit_paths(key, stop, N):
    """N = 3: the only pass that may jump is n = 1, directly before the last pass; N = 12: the reference rule's
    cycle_end lands on n = 10.  One launch, split waves and sector launches; batch order and the automatic
    dispatch order; both output forms; a ragged batch and a single syndrome; the jump on and off."""
    code, dec, _ = setup(key)
    auto = dec.get_option("schedule")
    assert auto == 1 and dec.get_option("near_hard") == 1 and dec.get_option("hard_paths") == 1
    for p in (0.01, 0.05):
        sX, sZ = syndromes(key, p)
        rec, its, _ = expected(key, p, N, stop)
        for split in (0, 1, 3):
            for schedule in (0, auto):
                for near in (1, 0):
                    with with_options(dec, sector_split=split, schedule=schedule, near_hard=near):
                        for form in ("bytes", "rec_bits"):
                            for B in (B_RAGGED, 1):
                                g = decode(dec, code, sX[:B], sZ[:B], p, N, stop, form)
                                what = (p, split, schedule, near, form, B)
                                assert np.array_equal(g[0], rec[:B]), ("records", what)
                                assert np.array_equal(g[1], its[:B]), ("iters", what)


@pytest.mark.parametrize("p", [0.02, 0.05])
def test_mixed_waves(p):
    """P7 under the reference stop, batch order (a wave is nine consecutive syndromes): waves in which one
    sector left through a jump and another in-range sector stopped earlier without one take the general
    post-processing branch on the near-exited group's soft registers.  The batch holds at least 8 such waves
    (a condition on the inputs), and the whole batch equals the oracle in both output forms."""
    code, dec, _ = setup("P7")
    N = 50
    sX, sZ = syndromes("P7", p)
    ph = phases(dec, code, sX, sZ, p, N, "ref", schedule=0)
    total, jumped = ph.sum(-1), ph[..., 3]
    mixed = 0
    for w in range((B_RAGGED + 8) // 9):
        rows = slice(9 * w, min(9 * w + 9, B_RAGGED))
        mixed += any((jumped[rows, s] > 0).any() and ((jumped[rows, s] == 0) & (total[rows, s] < N)).any()
                     for s in (0, 1))
    print("p = %g: %d mixed waves of %d" % (p, mixed, (B_RAGGED + 8) // 9))
    assert mixed >= 8, mixed
    rec, its, _ = expected("P7", p, N, "ref")
    assert dec.get_option("phase_stats") == 0
    for split in (0, 1):
        with with_options(dec, schedule=0, sector_split=split):
            for form in ("bytes", "rec_bits"):
                g = decode(dec, code, sX, sZ, p, N, "ref", form)
                assert np.array_equal(g[0], rec), ("records", split, form)
                assert np.array_equal(g[1], its), ("iters", split, form)


@pytest.mark.parametrize("key", ["P7", "P61"])
@pytest.mark.parametrize("stop", ["fixed", "ref", "syndrome"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_initialisation(key, stop, N):
    """N = 1: no table, the p' fill is live; N = 2: the table, then the last pass; N = 3: one pass between.
    Records and counts equal the oracle's with the hard-message forms on and off, for a ragged batch and one
    syndrome; with the final messages requested (no jump: the fill or iteration 0 defined every register) q
    equals the oracle's bit for bit."""
    code, dec, _ = setup(key)
    p = 0.01
    sX, sZ = syndromes(key, p)
    rec, its, qo = expected(key, p, N, stop, True)
    for hp in (1, 0):
        with with_options(dec, hard_paths=hp):
            for B in (B_RAGGED, 1):
                for form in ("bytes", "rec_bits"):
                    g = decode(dec, code, sX[:B], sZ[:B], p, N, stop, form)
                    assert np.array_equal(g[0], rec[:B]), ("records", hp, B, form)
                    assert np.array_equal(g[1], its[:B]), ("iters", hp, B, form)
                eX, eZ, fl, it, qg = dec.decode_batch(sX[:B], sZ[:B], p, N, stop, want_iters=True, want_q=True)
                assert np.array_equal(pack_records(eX, eZ, fl), rec[:B]), ("records with q", hp, B)
                assert np.array_equal(it, its[:B]), ("iters with q", hp, B)
                assert np.array_equal(qg.view(np.uint32), qo[:B].view(np.uint32)), ("q", hp, B)


def test_phase_totals():
    """P61, p = 0.01, 50 fixed iterations: every sector's four counts sum to 50 with the jump on and off, and
    the counts with it on are those the instrumented kernel reported before the exit changed (same inputs)."""
    code, dec, _ = setup("P61")
    sX, sZ = syndromes("P61", 0.01)
    on = phases(dec, code, sX, sZ, 0.01, 50, "fixed", near_hard=1)
    off = phases(dec, code, sX, sZ, 0.01, 50, "fixed", near_hard=0)
    assert (on.sum(-1) == 50).all() and (off.sum(-1) == 50).all()
    with open(GOLDEN) as f:
        want = np.array(json.load(f), dtype=np.uint32).reshape(on.shape)
    assert np.array_equal(on, want), np.argwhere(on != want)[:8]

"""The near-hard jump (QEC_OPT_NEAR_HARD_JUMP) on the GPU: with the jump
on and off the wave-circulant kernels give the oracle's decisions, flags and iteration counts in every
output form (byte outputs, packed records from byte rows and from bit rows), as one launch and as
sector launches, for a ragged batch and a single syndrome; also with the hard-message forms or the cycle
jump off; and the instrumented kernels show the iterations it saves."""
import functools

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


@functools.lru_cache(maxsize=None)
def setup(key):
    path = code_path(KEYS[key])
    code = q.Quantum_LDPC_Code.createFromFile(path)
    return code, q.DecoderGPU(code, 0), OracleCode(path)


@functools.lru_cache(maxsize=None)
def syndromes(key, p):
    """381 depolarising syndromes, an all-zero one and a single-bit one."""
    code = setup(key)[0]
    x, z = depolarizing_errors(code.n, 20252, B_RAGGED - 2, p)
    sX = np.concatenate([code.syndrome(0, x), np.zeros((2, code.numEqsX), np.uint8)])
    sZ = np.concatenate([code.syndrome(1, z), np.zeros((2, code.numEqsZ), np.uint8)])
    sX[-1, 7] = 1
    sZ[-1, 0] = 1
    return sX, sZ


@functools.lru_cache(maxsize=None)
def expected(key, p, N, stop):
    """The oracle's records and iteration counts, computed once per point."""
    sX, sZ = syndromes(key, p)
    o = setup(key)[2].decode_batch(sX, sZ, p, N, stop)
    return pack_records(o[0], o[1], o[2]), o[3]


def bit_rows(s):
    import torch
    B, m = s.shape
    pk = np.packbits(s, axis=1, bitorder="little")
    pad = np.zeros((B, 4 * ((m + 31) // 32)), np.uint8)
    pad[:, :pk.shape[1]] = pk
    return torch.from_numpy(pad.view(np.int32).copy()).to("cuda:0")


def decode(dec, code, sX, sZ, p, N, stop, form):
    """One device-buffer decode -> (records, iters) as numpy; form: byte outputs, or records from byte / bit rows."""
    import torch
    dev = torch.device("cuda", 0)
    B = len(sX)
    its = torch.empty((B, 2), dtype=torch.int32, device=dev)
    rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    if form == "rec_bits":
        dec.decode_bits_packed_dev(bit_rows(sX), bit_rows(sZ), p, N, stop, rec, its)
    else:
        dX, dZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
        if form == "rec_bytes":
            dec.decode_batch_packed_dev(dX, dZ, p, N, stop, rec, its)
        else:
            eX = torch.empty((B, code.n), dtype=torch.uint8, device=dev)
            eZ = torch.empty((B, code.n), dtype=torch.uint8, device=dev)
            fl = torch.empty((B,), dtype=torch.uint8, device=dev)
            dec.decode_batch_dev(dX, dZ, p, N, stop, eX, eZ, fl, its)
            torch.cuda.synchronize()
            return pack_records(eX.cpu().numpy(), eZ.cpu().numpy(), fl.cpu().numpy()), its.cpu().numpy()
    torch.cuda.synchronize()
    return rec.cpu().numpy(), its.cpu().numpy()


def with_options(dec, **opts):
    class Ctx:
        def __enter__(self):
            self.old = {k: dec.get_option(k) for k in opts}
            for k, v in opts.items():
                dec.set_option(k, v)

        def __exit__(self, *a):
            for k, v in self.old.items():
                dec.set_option(k, v)
    return Ctx()


@pytest.mark.parametrize("key", ["P7", "P61"])
@pytest.mark.parametrize("p", [0.001, 0.01, 0.05, 0.1])
@pytest.mark.parametrize("stop", ["fixed", "ref"])
def test_jump_on_off_oracle(key, p, stop):
    code, dec, _ = setup(key)
    sX, sZ = syndromes(key, p)
    assert dec.get_option("near_hard") == 1 and dec.get_option("hard_paths") == 1
    for N in (2, 3, 4, 11, 12, 50):
        rec, its = expected(key, p, N, stop)
        for split in (0, 3):
            for near in (1, 0):
                with with_options(dec, sector_split=split, near_hard=near):
                    for form in ("bytes", "rec_bytes", "rec_bits"):
                        for B in (B_RAGGED, 1):
                            g = decode(dec, code, sX[:B], sZ[:B], p, N, stop, form)
                            what = (N, split, near, form, B)
                            assert np.array_equal(g[0], rec[:B]), ("records", what)
                            assert np.array_equal(g[1], its[:B]), ("iters", what)


@pytest.mark.parametrize("key", ["P7", "P61"])
@pytest.mark.parametrize("opts", [{"cycle_jump": 0}, {"hard_paths": 0}], ids=["no_cycle_jump", "no_hard_paths"])
def test_jump_with_other_shortcuts_off(key, opts):
    code, dec, _ = setup(key)
    for p in (0.01, 0.05):
        sX, sZ = syndromes(key, p)
        for stop in ("fixed", "ref"):
            for N in (12, 50):
                rec, its = expected(key, p, N, stop)
                with with_options(dec, near_hard=1, **opts):
                    g = decode(dec, code, sX, sZ, p, N, stop, "rec_bits")
                assert np.array_equal(g[0], rec) and np.array_equal(g[1], its), (p, stop, N)


def phases(dec, code, sX, sZ, p, N, **opts):
    """Per sector (soft, hard, agreed, jumped) iteration counts of the instrumented kernels."""
    with with_options(dec, phase_stats=1, **opts):
        w = decode(dec, code, sX, sZ, p, N, "fixed", "rec_bits")[1].astype(np.uint32)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24], -1)  # [B, sector, phase]


def test_phase_counts():
    """P61, p = 0.01, 50 fixed iterations: the phases sum to 50 per sector; the jump executes at least one
    iteration fewer per sector on average (a float32 CPU model of both updates gives 2.5 fewer for X and
    2.1 for Z; the margin is for the sample size); without the hard-message forms nothing is jumped."""
    code, dec, _ = setup("P61")
    sX, sZ = syndromes("P61", 0.01)
    on = phases(dec, code, sX, sZ, 0.01, 50, near_hard=1)
    off = phases(dec, code, sX, sZ, 0.01, 50, near_hard=0)
    full = phases(dec, code, sX, sZ, 0.01, 50, hard_paths=0)
    for ph in (on, off, full):
        assert (ph.sum(-1) == 50).all()
    executed_on, executed_off = on[..., :3].sum(-1).mean(0), off[..., :3].sum(-1).mean(0)
    print("executed iterations per sector (X, Z): jump on %s, off %s" % (executed_on, executed_off))
    assert (executed_on <= executed_off - 1.0).all(), (executed_on, executed_off)
    assert (full[..., 3] == 0).all() and (full[..., 0] == 50).all()

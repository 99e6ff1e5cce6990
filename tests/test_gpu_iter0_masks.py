"""Iteration 0 of the P61 fixed / reference-stop kernels: the syndrome bit of
each variable's checks reaches the variable through a ring rotation, by LDS or, in the form that section
records as tried, by a rotated wave lane mask.  Inputs that set every ring position of every row one at a
time, the positions where a rotation wraps, every table index, and the edge syndromes, against the oracle:
decisions, flags, iteration counts in every output form, and the final messages bit for bit after one and two
further iterations (each of the R L iteration-0 messages on its own edge).  The same inputs exercise the
syndrome loads and the table copy at the head of a wave (one launch, sector launches, a single syndrome)."""
import functools

import numpy as np
import pytest

import qec_ldpc_amd as q
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import P61, code_path
from qec_ldpc_amd.gather import pack_records
from qec_ldpc_amd.synthetic import depolarizing_errors

pytestmark = pytest.mark.gpu

P = 61
PROB = 0.01


@functools.lru_cache(maxsize=None)
def setup():
    path = code_path(P61)
    code = q.Quantum_LDPC_Code.createFromFile(path)
    return code, q.DecoderGPU(code, 0), OracleCode(path)


@functools.lru_cache(maxsize=None)
def syndromes():
    """441 syndromes (check (r, i) of a sector is entry r P + i):
    305 with exactly X check k and Z check k set (X is zero from k = 244 on, beside a live Z sector);
    per row r, ring positions {0, 60} and {29, 30, 31, 32} set in both sectors (row 4: Z only);
    64 of independent uniform bits (every table index; they run every iteration);
    all ones, all zero, and 60 depolarising ones at p = 0.01."""
    code = setup()[0]
    mX, mZ = code.numEqsX, code.numEqsZ
    assert (mX, mZ) == (4 * P, 5 * P)
    sx, sz = [], []
    for k in range(mZ):
        x, z = np.zeros(mX, np.uint8), np.zeros(mZ, np.uint8)
        if k < mX:
            x[k] = 1
        z[k] = 1
        sx.append(x)
        sz.append(z)
    for r in range(5):
        for pos in ((0, 60), (29, 30, 31, 32)):
            x, z = np.zeros(mX, np.uint8), np.zeros(mZ, np.uint8)
            for i in pos:
                if r < 4:
                    x[r * P + i] = 1
                z[r * P + i] = 1
            sx.append(x)
            sz.append(z)
    rng = np.random.default_rng(6161)
    sx += list(rng.integers(0, 2, (64, mX), dtype=np.uint8))
    sz += list(rng.integers(0, 2, (64, mZ), dtype=np.uint8))
    sx += [np.ones(mX, np.uint8), np.zeros(mX, np.uint8)]
    sz += [np.ones(mZ, np.uint8), np.zeros(mZ, np.uint8)]
    ex, ez = depolarizing_errors(code.n, 4242, 60, PROB)
    sX = np.concatenate([np.stack(sx), code.syndrome(0, ex)])
    sZ = np.concatenate([np.stack(sz), code.syndrome(1, ez)])
    assert len(sX) == len(sZ) == 441
    return sX, sZ


@functools.lru_cache(maxsize=None)
def expected(N, stop):
    """The oracle's outputs, once per (N, stop): (records, iters, final messages)."""
    sX, sZ = syndromes()
    o = setup()[2].decode_batch(sX, sZ, PROB, N, stop, want_q=N <= 3)
    return pack_records(o[0], o[1], o[2]), o[3], o[4]


def bit_rows(s):
    import torch
    B, m = s.shape
    pk = np.packbits(s, axis=1, bitorder="little")
    pad = np.zeros((B, 4 * ((m + 31) // 32)), np.uint8)
    pad[:, :pk.shape[1]] = pk
    return torch.from_numpy(pad.view(np.int32).copy()).to("cuda:0")


def decode(dec, code, sX, sZ, N, stop, form):
    """One device-buffer decode -> (records, iters); form: byte outputs, or records from byte / bit rows."""
    import torch
    dev = torch.device("cuda", 0)
    B = len(sX)
    its = torch.empty((B, 2), dtype=torch.int32, device=dev)
    rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    if form == "rec_bits":
        dec.decode_bits_packed_dev(bit_rows(sX), bit_rows(sZ), PROB, N, stop, rec, its)
    else:
        dX, dZ = torch.from_numpy(sX).to(dev), torch.from_numpy(sZ).to(dev)
        if form == "rec_bytes":
            dec.decode_batch_packed_dev(dX, dZ, PROB, N, stop, rec, its)
        else:
            eX = torch.empty((B, code.n), dtype=torch.uint8, device=dev)
            eZ = torch.empty((B, code.n), dtype=torch.uint8, device=dev)
            fl = torch.empty((B,), dtype=torch.uint8, device=dev)
            dec.decode_batch_dev(dX, dZ, PROB, N, stop, eX, eZ, fl, its)
            torch.cuda.synchronize()
            return pack_records(eX.cpu().numpy(), eZ.cpu().numpy(), fl.cpu().numpy()), its.cpu().numpy()
    torch.cuda.synchronize()
    return rec.cpu().numpy(), its.cpu().numpy()


class options:
    def __init__(self, dec, **opts):
        self.dec, self.opts = dec, opts

    def __enter__(self):
        self.old = {k: self.dec.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.dec.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.dec.set_option(k, v)


def same_floats(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn])


def assert_same(g, N, stop, B, what):
    rec, its, _ = expected(N, stop)
    bad = np.nonzero((g[0] != rec[:B]).any(1) | (g[1] != its[:B]).any(1))[0]
    assert bad.size == 0, (what, "syndromes", bad[:10])


@pytest.mark.parametrize("N", [2, 3, 50])
@pytest.mark.parametrize("B", [441, 1])
def test_fixed_bit_rows_every_launch(N, B):
    """The fixed stop with records from bit rows: one launch and sector launches, dispatch order off and
    on, hard-message forms off and on."""
    code, dec, _ = setup()
    sX, sZ = syndromes()
    for split in (0, 3):
        for schedule in (0, 1):
            for hp in (0, 1):
                with options(dec, sector_split=split, schedule=schedule, hard_paths=hp):
                    g = decode(dec, code, sX[:B], sZ[:B], N, "fixed", "rec_bits")
                assert_same(g, N, "fixed", B, (split, schedule, hp))


@pytest.mark.parametrize("stop", ["fixed", "ref"])
@pytest.mark.parametrize("N", [2, 3, 50])
def test_forms_and_reference_stop(stop, N):
    code, dec, _ = setup()
    sX, sZ = syndromes()
    for form in ("bytes", "rec_bytes", "rec_bits"):
        for split in (0, 3):
            with options(dec, sector_split=split):
                g = decode(dec, code, sX, sZ, N, stop, form)
            assert_same(g, N, stop, len(sX), (form, split))
    with options(dec, sector_split=3, schedule=0, hard_paths=0):
        g = decode(dec, code, sX[:1], sZ[:1], N, stop, "bytes")
    assert_same(g, N, stop, 1, "B = 1")


@pytest.mark.parametrize("stop", ["fixed", "ref"])
@pytest.mark.parametrize("N", [2, 3])
def test_final_messages(stop, N):
    """N = 2: iteration 0 and the peeled last iteration; N = 3: one loop iteration between them."""
    _, dec, _ = setup()
    sX, sZ = syndromes()
    rec, its, qo = expected(N, stop)
    for split in (0, 3):
        with options(dec, sector_split=split):
            g = dec.decode_batch(sX, sZ, PROB, N, stop, want_iters=True, want_q=True)
        assert np.array_equal(pack_records(g[0], g[1], g[2]), rec), split
        assert np.array_equal(g[3], its), split
        assert same_floats(g[4], qo), split


@pytest.mark.parametrize("stop", ["fixed", "ref"])
def test_non_binary_entry(stop):
    """Byte rows with an entry of 2: it decodes as 1 and fails the sector's syndrome test (the flag above
    the R syndrome bits must not reach a lane mask)."""
    code, dec, orc = setup()
    sX, sZ = (s[300:330].copy() for s in syndromes())
    sX[3, 2 * P + 60] = 2
    sZ[3, 4 * P] = 2
    sX[-1] = 0
    sX[-1, 0] = 2
    for N in (2, 50):
        o = orc.decode_batch(sX, sZ, PROB, N, stop)
        want = pack_records(o[0], o[1], o[2])
        for split in (0, 3):
            with options(dec, sector_split=split):
                for form in ("bytes", "rec_bytes"):
                    g = decode(dec, code, sX, sZ, N, stop, form)
                    assert np.array_equal(g[0], want) and np.array_equal(g[1], o[3]), (N, split, form)

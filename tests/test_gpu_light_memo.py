"""The light-sector table (QEC_OPT_LIGHT_MEMO) on the GPU, P61: with the option on
and off every output (decisions, flags, iteration counts) is byte-identical and equals the oracle's, under the
fixed and the reference stop, as one launch and as sector launches, from byte and bit rows, into byte outputs and
packed records, for one batch that holds every single error of both sectors, 2 000 pairs per sector (same column,
lane differences 1 and P - 1, pairs sharing a check), three-error sets whose X syndrome has weight 2R, random
p = 0.01 samples and a row with a non-binary syndrome byte, and for a batch of one; at keys where no class can
be memoised and back; with final messages requested; on a handle with priors; captured into a graph with a cold
key; and through the instrumented kernels."""
import functools

import numpy as np
import pytest

import qec_ldpc_amd as q
from light_memo_cases import pair_sets, triple_sets_weight_2R, vec
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import P61, code_path
from qec_ldpc_amd.gather import pack_records
from qec_ldpc_amd.synthetic import depolarizing_errors

pytestmark = pytest.mark.gpu

P, L = 61, 10
N_PAIRS, N_TRIPLES, N_RANDOM = 2000, 24, 300


@functools.lru_cache(maxsize=None)
def setup():
    path = code_path(P61)
    code = q.Quantum_LDPC_Code.createFromFile(path)
    return code, q.DecoderGPU(code, 0), OracleCode(path)


@functools.lru_cache(maxsize=None)
def batch():
    """(sX, sZ, first row of each part, the generating errors' records): singles | pairs | triples | random | one
    non-binary row (the last)."""
    code = setup()[0]
    n = code.n
    Es = [np.asarray(code.exponents(sec)) for sec in (0, 1)]
    errs = []
    for sec, E in enumerate(Es):
        sets = [[(j // P, j % P)] for j in range(n)]
        sets += pair_sets(E, P, L, N_PAIRS, seed=11 + sec)
        sets += triple_sets_weight_2R(E, P, L, N_TRIPLES, seed=21 + sec)
        errs.append(np.stack([vec(n, P, s) for s in sets]))
    x, z = depolarizing_errors(n, 4242, N_RANDOM, 0.01)
    ex = np.concatenate([errs[0], x, errs[0][5:6]])
    ez = np.concatenate([errs[1], z, errs[1][7:8]])
    sX, sZ = code.syndrome(0, ex), code.syndrome(1, ez)
    sX[-1][np.flatnonzero(sX[-1])[0]] = 2  # a one-error syndrome with a byte that is neither 0 nor 1
    parts = {"singles": 0, "pairs": n, "triples": n + N_PAIRS, "random": n + N_PAIRS + N_TRIPLES}
    assert len(sX) == n + N_PAIRS + N_TRIPLES + N_RANDOM + 1 and len(sX) % 2 == 1
    assert (sX[parts["triples"]:parts["random"]].sum(1) == 8).all()  # the X look-alikes: weight 2R
    return sX, sZ, parts, pack_records(ex, ez, np.zeros(len(ex), np.uint8))


@functools.lru_cache(maxsize=None)
def expected(p, N, stop, lo=0, hi=None):
    sX, sZ = batch()[:2]
    o = setup()[2].decode_batch(sX[lo:hi], sZ[lo:hi], p, N, stop)
    return pack_records(o[0], o[1], o[2]), o[3]


def bit_rows(s):
    import torch
    B, m = s.shape
    pk = np.packbits(s, axis=1, bitorder="little")
    pad = np.zeros((B, 4 * ((m + 31) // 32)), np.uint8)
    pad[:, :pk.shape[1]] = pk
    return torch.from_numpy(pad.view(np.int32).copy()).to("cuda:0")


def decode(dec, code, sX, sZ, p, N, stop, form):
    """One device-buffer decode -> (records, iters); form: byte outputs, or records from byte / bit rows."""
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


def check_on_off(dec, code, lo, hi, p, N, stop, splits=(0, 3), forms=("bytes", "rec_bytes", "rec_bits")):
    sX, sZ = batch()[:2]
    rec, its = expected(p, N, stop, lo, hi)
    for split in splits:
        for form in forms:
            # bit rows cannot hold the non-binary byte: that form decodes the batch without its last row
            cut = -1 if form == "rec_bits" and (hi is None or hi == len(sX)) else None
            got = {}
            for memo in (1, 0):
                with options(dec, sector_split=split, light_memo=memo):
                    got[memo] = decode(dec, code, sX[lo:hi][:cut], sZ[lo:hi][:cut], p, N, stop, form)
            what = (p, N, stop, split, form)
            assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), ("on / off", what)
            assert np.array_equal(got[1][0], rec[:cut]), ("records", what, np.flatnonzero((got[1][0] != rec[:cut]).any(1))[:8])
            assert np.array_equal(got[1][1], its[:cut]), ("iters", what, np.flatnonzero((got[1][1] != its[:cut]).any(1))[:8])


@pytest.mark.parametrize("stop", ["fixed", "ref"])
def test_on_off_oracle(stop):
    code, dec, _ = setup()
    assert dec.get_option("light_memo") == 1
    check_on_off(dec, code, 0, None, 0.01, 50, stop)
    check_on_off(dec, code, 0, 1, 0.01, 50, stop)  # a batch of one: a single error in both sectors


def test_every_single_and_clean_pair_is_memoisable_at_the_headline_key():
    """What makes the table pay: at (p = 0.01, N = 50) every single error, and every pair with disjoint checks, decodes
    to exactly its generating qubits with both flags clear (the oracle's word; the kernel's entry repeats it)."""
    sX, sZ, parts, gen = batch()
    rec, its = expected(0.01, 50, "fixed")
    hi = parts["triples"]
    clean = np.flatnonzero((sX[:hi].sum(1) % 4 == 0) & (sZ[:hi].sum(1) % 5 == 0))  # singles, pairs sharing no check
    assert len(clean) > parts["pairs"] + 1500  # random pairs share a check in 6-7 % of the sectors
    assert np.array_equal(rec[clean], gen[clean]) and (its[clean] == 50).all()


def test_keys_without_memoisable_classes_and_rekeying():
    """(p = 0.2, N = 2) and (p = 0.3, N = 50): no class decodes to its generating qubits, every entry is 0 and the
    sectors fall back to BP; then the headline key again on the same decoder."""
    code, dec, _ = setup()
    parts, gen = batch()[2:]
    lo = parts["pairs"] - 40  # the last singles, 200 pairs: two-column, one-column, sharing a check
    for p, N in ((0.2, 2), (0.3, 50)):
        check_on_off(dec, code, lo, lo + 240, p, N, "fixed", forms=("bytes", "rec_bits"))
        rec = expected(p, N, "fixed", lo, lo + 240)[0]
        assert (rec[:40] != gen[lo:lo + 40]).any(1).all()  # no single error comes back as itself
    check_on_off(dec, code, lo, lo + 240, 0.01, 50, "fixed", forms=("bytes", "rec_bits"))
    check_on_off(dec, code, lo, lo + 240, 0.01, 50, "ref", forms=("rec_bytes",))
    check_on_off(dec, code, lo, lo + 240, 0.01, 50, "fixed", forms=("rec_bytes",))


def test_final_messages_requested():
    code, dec, _ = setup()
    sX, sZ, parts = batch()[:3]
    lo = parts["pairs"] - 20
    rec, its = expected(0.01, 50, "fixed", lo, lo + 60)
    got = {}
    for memo in (1, 0):
        with options(dec, light_memo=memo):
            got[memo] = dec.decode_batch(sX[lo:lo + 60], sZ[lo:lo + 60], 0.01, 50, "fixed", want_iters=True, want_q=True)
    for a, b in zip(got[1], got[0]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(pack_records(*got[1][:3]), rec) and np.array_equal(got[1][3], its)


def test_priors_on_a_sparse_handle():
    """Per-qubit priors live on the sparse-graph engine, which has no table: the option changes nothing there."""
    code, _, _ = setup()
    sX, sZ, parts = batch()[:3]
    lo = parts["pairs"] - 20
    dec = q.DecoderGPU(code, 0, engine="sparse")
    rng = np.random.default_rng(8)
    dec.set_priors(rng.uniform(0.002, 0.02, code.n).astype(np.float32), rng.uniform(0.002, 0.02, code.n).astype(np.float32))
    got = {}
    for memo in (1, 0):
        dec.set_option("light_memo", memo)
        got[memo] = dec.decode_batch(sX[lo:lo + 60], sZ[lo:lo + 60], 0.01, 50, "fixed", want_iters=True)
    for a, b in zip(got[1], got[0]):
        assert np.array_equal(a, b)


def test_graph_captured_with_a_cold_key():
    """A capture with a cold key enqueues no fill and decodes without the table; after an eager call has warmed the
    key a second capture reads it.  Both replays give the eager records."""
    import torch
    code, _, _ = setup()
    sX, sZ, parts = batch()[:3]
    lo, B = parts["pairs"] - 100, 333
    dev = torch.device("cuda", 0)
    dec = q.DecoderGPU(code, 0, max_batch=B)
    tX, tZ = torch.from_numpy(sX[lo:lo + B]).to(dev), torch.from_numpy(sZ[lo:lo + B]).to(dev)
    want_rec, want_its = expected(0.01, 12, "fixed", lo, lo + B)
    for warm in (False, True):
        if warm:
            ref = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
            dec.decode_batch_packed_dev(tX, tZ, 0.01, 12, "fixed", ref)
            torch.cuda.synchronize()
            assert np.array_equal(ref.cpu().numpy(), want_rec)
        rec = torch.zeros((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
        its = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                dec.decode_batch_packed_dev(tX, tZ, 0.01, 12, "fixed", rec, its, stream=s)
        rec.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rec.cpu().numpy(), want_rec), warm
        assert np.array_equal(its.cpu().numpy(), want_its), warm


def test_instrumented_kernels_account_for_every_iteration():
    """The instrumented kernels decode every sector by BP (as they do zero syndromes): on the single-error batch the
    executed and the jumped iterations of each sector add up to the nominal 50."""
    code, dec, _ = setup()
    sX, sZ, parts = batch()[:3]
    with options(dec, phase_stats=1):
        w = decode(dec, code, sX[:parts["pairs"]], sZ[:parts["pairs"]], 0.01, 50, "fixed", "rec_bits")[1].astype(np.uint32)
    ph = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24], -1)
    assert (ph.sum(-1) == 50).all()

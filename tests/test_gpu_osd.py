"""BP + OSD-0 on the GPU (osd.hip): the elimination kernel through
qec_osd_dev, the synchronous calls and qec_monte_carlo with QEC_OPT_OSD on, and graph capture, against
the numpy yardstick of tests/test_osd_host.py (soft input and BP outputs from the oracle)."""
import numpy as np
import pytest
import torch

import qec_ldpc_amd as q
from qec_ldpc_amd.gather import pack_records
from test_osd_host import (FAIL, MAIN, check_main_conditions, env, forced_batch, inconsistent_syndrome,  # noqa: F401 (env: fixture)
                           main_case)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = [(k, e) for k in ("P7", "G13", "P61") for e in ("auto", "sparse")]


@pytest.fixture(scope="module")
def decoders(env):
    cache = {}

    def get(key, engine="auto", **kw):
        k = (key, engine, tuple(sorted(kw.items())))
        if k not in cache:
            cache[k] = q.DecoderGPU(env[key][0], 0, engine=engine, **kw)
        return cache[k]
    return get


_forced = {}


def forced_case(env, key):
    """The random-soft-input batch (every sector forced to fail) and the yardstick's repair of it."""
    if key not in _forced:
        code, _, _, ys = env[key]
        B = 64 if key == "P61" else 32  # P61: 128 sectors, each another random column order
        batch = forced_batch(code, np.random.default_rng(2024), B)
        want = ys.repair(*batch)
        assert want[3] == 2 * B
        _forced[key] = (batch, want)
    return _forced[key]


def guarded(a, pad_rows=1, offset=0):
    """The array on the device between guard rows of 0xA5 (offset: extra bytes in front, so a byte
    vector starts at an unaligned address) -> (whole tensor, the view the call gets)."""
    a = np.ascontiguousarray(a)
    flat = a.reshape(a.shape[0], -1)
    if a.ndim == 1:
        whole = torch.full((offset + a.shape[0] + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        view = whole[offset:offset + a.shape[0]]
        view.copy_(torch.from_numpy(a).to(DEV))
        return whole, view
    whole = torch.full((flat.shape[0] + 2 * pad_rows, flat.shape[1]), 0xA5, dtype=torch.uint8, device=DEV)
    view = whole[pad_rows:pad_rows + flat.shape[0]]
    view.copy_(torch.from_numpy(flat).to(DEV))
    return whole, view


def guards_intact(whole, view_rows, pad_rows=1, offset=0):
    w = whole.cpu().numpy()
    if w.ndim == 1:
        return (w[:offset] == 0xA5).all() and (w[offset + view_rows:] == 0xA5).all()
    return (w[:pad_rows] == 0xA5).all() and (w[pad_rows + view_rows:] == 0xA5).all()


@pytest.mark.parametrize("key,engine", CASES)
def test_osd_dev_matches_numpy_on_random_soft_input(env, decoders, key, engine):
    (sX, sZ, qf, eX, eZ, flags), (wX, wZ, wf, _) = forced_case(env, key)
    dec = decoders(key, engine)
    B = len(flags)
    tsX, tsZ = torch.from_numpy(sX).to(DEV), torch.from_numpy(sZ).to(DEV)
    tq = torch.from_numpy(qf).to(DEV)
    gX, vX = guarded(eX)
    gZ, vZ = guarded(eZ)
    gF, vF = guarded(flags, offset=5)
    s0, q0 = tsX.clone(), tq.clone()
    dec.osd_dev(tsX, tsZ, tq, vX, vZ, vF)
    torch.cuda.synchronize()
    assert np.array_equal(vF.cpu().numpy(), wf)
    assert np.array_equal(vX.cpu().numpy(), wX) and np.array_equal(vZ.cpu().numpy(), wZ)
    assert guards_intact(gX, B) and guards_intact(gZ, B) and guards_intact(gF, B, offset=5)
    assert torch.equal(tsX, s0) and torch.equal(tq.view(torch.int32), q0.view(torch.int32))
    for sweep in (1, 2):  # the kernel's two forms of the row update, forced: the same bits
        vX.copy_(torch.from_numpy(eX).to(DEV))
        vZ.copy_(torch.from_numpy(eZ).to(DEV))
        vF.copy_(torch.from_numpy(flags).to(DEV))
        dec.set_option("osd_sweep", sweep)
        try:
            dec.osd_dev(tsX, tsZ, tq, vX, vZ, vF)
        finally:
            dec.set_option("osd_sweep", 0)
        torch.cuda.synchronize()
        assert np.array_equal(vF.cpu().numpy(), wf), sweep
        assert np.array_equal(vX.cpu().numpy(), wX) and np.array_equal(vZ.cpu().numpy(), wZ), sweep
    # the host form of the same handle runs the kernel too
    hX, hZ, hf = dec.osd(sX, sZ, qf, eX, eZ, flags)
    assert np.array_equal(hX, wX) and np.array_equal(hZ, wZ) and np.array_equal(hf, wf)
    assert dec.get_option("osd_sectors") == 2 * B


@pytest.mark.parametrize("key,engine", CASES)
def test_decode_batch_with_osd(env, decoders, key, engine):
    code = env[key][0]
    dec = decoders(key, engine)
    p, N, B, _ = MAIN[key]
    sX, sZ, _, _, want = main_case(env, key)
    check_main_conditions(code, key, sX, sZ, want)
    eX, eZ, flags, cnt, iters, flags0 = want
    off = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
    path_off = dec.last_path()
    assert np.array_equal(off[2], flags0) and np.array_equal(off[3], iters) and "osd" not in path_off
    assert dec.get_option("osd_sectors") == 0
    rec_off, _ = dec.decode_batch_packed(sX, sZ, p, N, "syndrome")
    assert np.array_equal(rec_off, pack_records(off[0], off[1], off[2]))
    dec.set_option("osd", 1)
    try:
        g = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
        assert dec.last_path() == path_off | {"osd"}
        assert np.array_equal(g[2], flags) and np.array_equal(g[0], eX) and np.array_equal(g[1], eZ)
        assert np.array_equal(g[3], iters) and dec.get_option("osd_sectors") == cnt
        rec, its = dec.decode_batch_packed(sX, sZ, p, N, "syndrome", want_iters=True)
        assert "osd" in dec.last_path() and "records" in dec.last_path()
        assert np.array_equal(rec, pack_records(eX, eZ, flags)) and np.array_equal(its, iters)
        assert dec.get_option("osd_sectors") == cnt
    finally:
        dec.set_option("osd", 0)
    again = dec.decode_batch(sX, sZ, p, N, "syndrome")
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], off[:3])) and dec.last_path() == path_off


def unpack_errors(errp, n):
    nb = (n + 7) // 8
    bits = np.unpackbits(errp, axis=1, bitorder="little")
    return bits[:, :n].copy(), bits[:, 8 * nb:8 * nb + n].copy()


MC = {"G13": dict(count=4096, p=0.05, N=25, batch=1024), "P61": dict(count=512, p=0.06, N=50, batch=1024)}
_mc = {}


def mc_expected(env, dec, key):
    """Host counting over the device sampler's own samples, decoded and repaired by the yardstick."""
    if key not in _mc:
        code, _, orc, ys = env[key]
        m = MC[key]
        B = m["count"]
        sX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=DEV)
        sZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=DEV)
        errp = torch.empty((B, 2 * ((code.n + 7) // 8)), dtype=torch.uint8, device=DEV)
        dec.sample_syndrome_dev(0xD15EA5E, 3, m["p"], sX, sZ, errp)
        torch.cuda.synchronize()
        x, z = unpack_errors(errp.cpu().numpy(), code.n)
        sX, sZ = sX.cpu().numpy(), sZ.cpu().numpy()
        eX, eZ, flags, cnt, _, flags0 = ys.bp_osd(orc, sX, sZ, m["p"], m["N"], "syndrome")
        assert (flags0 & 3).any() and not (flags & 3).any()
        logical = code.check_logical(x ^ eX, z ^ eZ)
        _mc[key] = ({"withX": int(x.any(1).sum()), "withZ": int(z.any(1).sum()), "synX": 0, "synZ": 0,
                     "logical": int(logical.sum()), "corrected": int((~logical).sum()),
                     "convX": int(((flags & 4) != 0).sum()), "convZ": int(((flags & 8) != 0).sum())}, cnt)
    return _mc[key]


@pytest.mark.parametrize("key", ["G13", "P61"])
def test_monte_carlo_with_osd(env, decoders, key):
    code = env[key][0]
    dec = decoders(key)
    m = MC[key]
    exp, cnt = mc_expected(env, dec, key)
    run = lambda d: d.monte_carlo(0xD15EA5E, 3, m["count"], m["p"], m["N"], "syndrome", batch=m["batch"])  # noqa: E731
    off = run(dec)
    assert off["synX"] + off["synZ"] > 0 and "osd" not in dec.last_path() and dec.get_option("osd_sectors") == 0
    dec.set_option("osd", 1)
    try:
        on = run(dec)
        assert "osd" in dec.last_path() and dec.get_option("osd_sectors") == cnt
    finally:
        dec.set_option("osd", 0)
    assert {k: on[k] for k in q.MC_COUNTERS} == exp and on["tested"] == m["count"]
    assert (on["iterationsX"], on["iterationsZ"]) == (off["iterationsX"], off["iterationsZ"])
    assert on["corrected"] >= off["corrected"]
    two = q.DecoderGPU(code, devices=[0, 0])
    two.set_option("osd", 1)
    r2 = run(two)
    for k in q.MC_COUNTERS + ("tested", "iterationsX", "iterationsZ"):
        assert r2[k] == on[k], k
    assert two.get_option("osd_sectors") == cnt


def test_osd_dev_in_a_graph(env):
    """osd_dev allocates nothing and synchronises nothing: captured into a graph and replayed once it
    gives the eager call's output."""
    (sX, sZ, qf, eX, eZ, flags), (wX, wZ, wf, _) = forced_case(env, "G13")
    B = len(flags)
    dec = q.DecoderGPU(env["G13"][0], 0, max_batch=B)
    t = [torch.from_numpy(a).to(DEV) for a in (sX, sZ, qf)]
    oX, oZ, oF = (torch.from_numpy(a).to(DEV) for a in (eX, eZ, flags))
    cX, cZ, cF = oX.clone(), oZ.clone(), oF.clone()
    dec.osd_dev(*t, oX, oZ, oF)  # eager
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.osd_dev(*t, cX, cZ, cF, stream=s)
    cX.copy_(torch.from_numpy(eX).to(DEV))  # capture ran nothing; replay on fresh inputs
    cZ.copy_(torch.from_numpy(eZ).to(DEV))
    cF.copy_(torch.from_numpy(flags).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cX, oX) and torch.equal(cZ, oZ) and torch.equal(cF, oF)
    assert np.array_equal(cX.cpu().numpy(), wX) and np.array_equal(cF.cpu().numpy(), wf)


def osd_dev_on(dec, sX, sZ, qf, eX, eZ, flags):
    """osd_dev on guarded copies -> (eX, eZ, flags) as numpy, the guards checked."""
    B = len(flags)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (sX, sZ, qf)]
    gX, vX = guarded(eX)
    gZ, vZ = guarded(eZ)
    gF, vF = guarded(flags, offset=5)
    dec.osd_dev(*t, vX, vZ, vF)
    torch.cuda.synchronize()
    assert guards_intact(gX, B) and guards_intact(gZ, B) and guards_intact(gF, B, offset=5)
    return vX.cpu().numpy(), vZ.cpu().numpy(), vF.cpu().numpy()


@pytest.mark.parametrize("key", ["P7", "G13", "P61"])
def test_osd_dev_leaves_an_inconsistent_syndrome_alone(env, decoders, key):
    """The device twin of test_osd_host.test_inconsistent_syndrome_is_left_alone: the kernel returns before it
    writes, and the other sectors of the batch are repaired."""
    code, _, _, ys = env[key]
    rng = np.random.default_rng(5)
    sX, sZ, qf, eX, eZ, flags = forced_batch(code, rng, 4)
    deficient = [sec for sec in (0, 1) if ys.rank[sec] < ys.H[sec].shape[0]]
    assert deficient, "every shipped matrix is rank deficient"
    for sec in deficient:
        s = (sX, sZ)[sec]
        s[1] = inconsistent_syndrome(ys, sec, s[1], rng)
    wX, wZ, wf, cnt = ys.repair(sX, sZ, qf, eX, eZ, flags)
    assert cnt == 8 - len(deficient)
    dec = decoders(key)
    gX, gZ, gf = osd_dev_on(dec, sX, sZ, qf, eX, eZ, flags)
    assert np.array_equal(gX, wX) and np.array_equal(gZ, wZ) and np.array_equal(gf, wf)
    for sec in deficient:  # estimate and flag as BP left them
        assert gf[1] & FAIL[sec]
        assert np.array_equal((gX, gZ)[sec][1], (eX, eZ)[sec][1])
    hX, hZ, hf = dec.osd(sX, sZ, qf, eX, eZ, flags)
    assert np.array_equal(hX, wX) and np.array_equal(hZ, wZ) and np.array_equal(hf, wf)
    assert dec.get_option("osd_sectors") == cnt


@pytest.mark.parametrize("key", ["P7", "G13", "P61"])
def test_osd_dev_leaves_sectors_without_their_fail_bit_alone(env, decoders, key):
    """The device twin of the partial-flags half of test_osd_host.test_qec_osd_matches_numpy_on_random_soft_input."""
    (sX, sZ, qf, eX, eZ, flags), (wX, wZ, wf, _) = forced_case(env, key)
    part = flags.copy()
    part[::2] &= ~1 & 0xFF
    part[1::3] &= ~2 & 0xFF
    gX, gZ, gf = osd_dev_on(decoders(key), sX, sZ, qf, eX, eZ, part)
    keepX, keepZ = (part & 1) == 0, (part & 2) == 0
    assert keepX.any() and keepZ.any() and (~keepX).any() and (~keepZ).any()
    assert np.array_equal(gX[keepX], eX[keepX]) and np.array_equal(gZ[keepZ], eZ[keepZ])
    assert np.array_equal(gX[~keepX], wX[~keepX]) and np.array_equal(gZ[~keepZ], wZ[~keepZ])
    assert np.array_equal(gf, part & 12)

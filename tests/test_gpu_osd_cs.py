"""The combination sweep on the GPU (osd_kernel<true> in osd.hip): the
scoring stage through qec_osd_dev, the synchronous calls and qec_monte_carlo with QEC_OPT_OSD_ORDER
set, and graph capture, against the numpy yardstick of tests/test_osd_cs_host.py.

The forced batches are the smallest shapes at which the stage can go wrong: P7 (m = 14 / 21, f = 26:
less than one wave of columns, and lambda = 64 clamps to f), G13 (n = 78: a row crosses a word pair;
f = 41), P61 (305 rows: five row chunks and ten-word column vectors; f = 369 / 309: the column loop
runs several times; lambda = 64: 2 016 pairs)."""
import numpy as np
import pytest
import torch

import qec_ldpc_amd as q
from qec_ldpc_amd.gather import pack_records
from test_gpu_osd import MC, guarded, guards_intact, unpack_errors
from test_osd_cs_host import YardstickCS, check_forced_conditions, forced_cs, main_cs, osd_order
from test_osd_host import MAIN, env, main_case  # noqa: F401 (env: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = [(k, e) for k in ("P7", "G13", "P61") for e in ("auto", "sparse")]
MC_SEED = 0xD15EA5E


@pytest.fixture(scope="module")
def decoders(env):
    cache = {}

    def get(key, engine="auto"):
        if (key, engine) not in cache:
            cache[key, engine] = q.DecoderGPU(env[key][0], 0, engine=engine)
        return cache[key, engine]
    return get


@pytest.mark.parametrize("key,engine", CASES)
def test_osd_dev_matches_numpy_for_every_order(env, decoders, key, engine):
    (sX, sZ, qf, eX, eZ, flags), want = forced_cs(env, key)
    check_forced_conditions(env, key)
    dec = decoders(key, engine)
    B = len(flags)
    tsX, tsZ = torch.from_numpy(sX).to(DEV), torch.from_numpy(sZ).to(DEV)
    tq = torch.from_numpy(qf).to(DEV)
    gX, vX = guarded(eX)
    gZ, vZ = guarded(eZ)
    gF, vF = guarded(flags, offset=5)
    s0, z0, q0 = tsX.clone(), tsZ.clone(), tq.clone()
    for lam in (1, 2, 10, 64):
        wX, wZ, wf, cnt, swept = want[lam][:5]
        with osd_order(dec, lam):
            for sweep in (0, 1, 2):  # the elimination's forms of the row update: the same bits behind each
                vX.copy_(torch.from_numpy(eX).to(DEV))
                vZ.copy_(torch.from_numpy(eZ).to(DEV))
                vF.copy_(torch.from_numpy(flags).to(DEV))
                dec.set_option("osd_sweep", sweep)
                try:
                    dec.osd_dev(tsX, tsZ, tq, vX, vZ, vF)
                finally:
                    dec.set_option("osd_sweep", 0)
                torch.cuda.synchronize()
                assert np.array_equal(vF.cpu().numpy(), wf), (lam, sweep)
                assert np.array_equal(vX.cpu().numpy(), wX) and np.array_equal(vZ.cpu().numpy(), wZ), (lam, sweep)
                assert guards_intact(gX, B) and guards_intact(gZ, B) and guards_intact(gF, B, offset=5)
            # the host form of the same handle runs the kernel too, and counts
            hX, hZ, hf = dec.osd(sX, sZ, qf, eX, eZ, flags)
            assert np.array_equal(hX, wX) and np.array_equal(hZ, wZ) and np.array_equal(hf, wf), lam
            assert dec.get_option("osd_sectors") == cnt == 2 * B and dec.get_option("osd_cs_sectors") == swept, lam
    assert torch.equal(tsX, s0) and torch.equal(tsZ, z0) and torch.equal(tq.view(torch.int32), q0.view(torch.int32))
    # the order back at 0: OSD-0, and nothing swept
    hX, hZ, hf = dec.osd(sX, sZ, qf, eX, eZ, flags)
    assert np.array_equal(hX, want[0][0]) and np.array_equal(hZ, want[0][1]) and np.array_equal(hf, want[0][2])
    assert dec.get_option("osd_cs_sectors") == 0


@pytest.mark.parametrize("key,engine", CASES)
def test_decode_batch_with_osd_cs(env, decoders, key, engine):
    dec = decoders(key, engine)
    p, N, B, _ = MAIN[key]
    sX, sZ, _, _, zero = main_case(env, key)
    eX, eZ, flags, cnt, swept = main_cs(env, key)
    assert swept >= 1
    with osd_order(dec, 10, osd=1):
        g = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
        assert "osd" in dec.last_path()
        assert np.array_equal(g[2], flags) and np.array_equal(g[0], eX) and np.array_equal(g[1], eZ)
        assert np.array_equal(g[3], zero[4])
        assert dec.get_option("osd_sectors") == cnt and dec.get_option("osd_cs_sectors") == swept
        rec, its = dec.decode_batch_packed(sX, sZ, p, N, "syndrome", want_iters=True)
        assert "osd" in dec.last_path() and "records" in dec.last_path()
        assert np.array_equal(rec, pack_records(eX, eZ, flags)) and np.array_equal(its, zero[4])
        assert dec.get_option("osd_sectors") == cnt and dec.get_option("osd_cs_sectors") == swept
    dec.set_option("osd", 1)  # the order reset: the outputs of BP + OSD-0
    try:
        g = dec.decode_batch(sX, sZ, p, N, "syndrome")
        assert np.array_equal(g[0], zero[0]) and np.array_equal(g[1], zero[1]) and np.array_equal(g[2], zero[2])
        assert dec.get_option("osd_sectors") == zero[3] and dec.get_option("osd_cs_sectors") == 0
    finally:
        dec.set_option("osd", 0)


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
        dec.sample_syndrome_dev(MC_SEED, 3, m["p"], sX, sZ, errp)
        torch.cuda.synchronize()
        x, z = unpack_errors(errp.cpu().numpy(), code.n)
        sX, sZ = sX.cpu().numpy(), sZ.cpu().numpy()
        eX, eZ, flags, cnt, swept = YardstickCS(ys).bp_osd_cs(orc, sX, sZ, m["p"], m["N"], "syndrome", 10)
        assert cnt >= 1 and not (flags & 3).any()
        logical = code.check_logical(x ^ eX, z ^ eZ)
        _mc[key] = ({"withX": int(x.any(1).sum()), "withZ": int(z.any(1).sum()), "synX": 0, "synZ": 0,
                     "logical": int(logical.sum()), "corrected": int((~logical).sum()),
                     "convX": int(((flags & 4) != 0).sum()), "convZ": int(((flags & 8) != 0).sum())}, cnt, swept)
    return _mc[key]


@pytest.mark.parametrize("key", ["G13", "P61"])
def test_monte_carlo_with_osd_cs(env, decoders, key):
    code = env[key][0]
    dec = decoders(key)
    m = MC[key]
    exp, cnt, swept = mc_expected(env, dec, key)
    assert swept >= 1  # the sweep changes a winner in this run (checked on the CPU with oracle/philox.py first)
    run = lambda d: d.monte_carlo(MC_SEED, 3, m["count"], m["p"], m["N"], "syndrome", batch=m["batch"])  # noqa: E731
    with osd_order(dec, 10, osd=1):
        on = run(dec)
        assert "osd" in dec.last_path()
        assert dec.get_option("osd_sectors") == cnt and dec.get_option("osd_cs_sectors") == swept
    assert {k: on[k] for k in q.MC_COUNTERS} == exp and on["tested"] == m["count"]
    two = q.DecoderGPU(code, devices=[0, 0])
    two.set_option("osd", 1)
    two.set_option("osd_order", 10)
    assert two.get_option("osd_order") == 10
    r2 = run(two)
    for k in q.MC_COUNTERS + ("tested", "iterationsX", "iterationsZ"):
        assert r2[k] == on[k], k
    assert two.get_option("osd_sectors") == cnt and two.get_option("osd_cs_sectors") == swept


def test_osd_cs_dev_in_a_graph(env):
    """osd_dev at lambda = 10 allocates nothing and synchronises nothing: captured into a graph and
    replayed once it gives the eager call's output."""
    (sX, sZ, qf, eX, eZ, flags), want = forced_cs(env, "G13")
    wX, wZ, wf = want[10][:3]
    B = len(flags)
    dec = q.DecoderGPU(env["G13"][0], 0, max_batch=B)
    dec.set_option("osd_order", 10)
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
    assert np.array_equal(cX.cpu().numpy(), wX) and np.array_equal(cZ.cpu().numpy(), wZ)
    assert np.array_equal(cF.cpu().numpy(), wf)

"""The prior-weighted score of the combination sweep on the GPU (osd_kernel<true, true> in osd.hip; DESIGN.md
section 1.4): qec_osd_dev, the synchronous calls, qec_monte_carlo and graph capture with QEC_OPT_OSD_SCORE = 1,
against the numpy yardstick of tests/test_osd_weighted_host.py and the CPU engine.

The forced batches are the smallest shapes at which the stage can go wrong: surf3 (n = 13, one chunk of rows,
f < lambda clamps), hgp_ham (n = 58, the general BP kernel in front), G13 (n = 78: a row crosses a 64-bit
word), P61 (n = 610, 305 rows: five 64-row chunks, eleven-word bit-planes, the largest LDS image)."""
import numpy as np
import pytest
import torch

import qec_ldpc_amd as q
from qec_ldpc_amd.gather import pack_records
from test_gpu_general_code import count, logical_code
from test_gpu_osd import guarded, guards_intact
from test_osd_weighted_host import (FORCED_SMALL, FORCED_B, SAMPLED, forced, lds_words, osd_options, priors_of, sampled,
                                    want, weights_of, yardstick)
from test_priors import F32, code_of, matrices, prior_vectors

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LAMS = (1, 2, 10, 64)
_decoders = {}


def gpu(name):
    """One sparse-engine decoder per test code (priors and options are set by each test)."""
    if name not in _decoders:
        _decoders[name] = q.DecoderGPU(code_of(name), 0, engine="sparse")
    return _decoders[name]


def run_osd_dev(dec, data, lam, score):
    """osd_dev on fresh guarded copies of the batch -> (eX, eZ, flags) as numpy."""
    sX, sZ, qf, eX, eZ, flags = data
    B = len(flags)
    t = [torch.from_numpy(a).to(DEV) for a in (sX, sZ, qf)]
    gX, vX = guarded(eX)
    gZ, vZ = guarded(eZ)
    gF, vF = guarded(flags, offset=5)
    with osd_options(dec, lam, score):
        dec.osd_dev(*t, vX, vZ, vF)
        torch.cuda.synchronize()
    assert guards_intact(gX, B) and guards_intact(gZ, B) and guards_intact(gF, B, offset=5)
    assert np.array_equal(t[0].cpu().numpy(), sX) and np.array_equal(t[1].cpu().numpy(), sZ)  # the inputs are read only
    assert np.array_equal(t[2].cpu().numpy().view(np.uint32), np.ascontiguousarray(qf).view(np.uint32))
    return vX.cpu().numpy(), vZ.cpu().numpy(), vF.cpu().numpy()


# ---- 1. osd_dev = the yardstick = DecoderCPU.osd ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["surf3", "hgp_ham", "G13", "P61"])
@pytest.mark.parametrize("kind", ["random", "two"])
def test_osd_dev_matches_the_weighted_yardstick_and_the_cpu_engine(name, kind):
    code = code_of(name)
    data = forced(name)
    B = len(data[5])
    assert B == FORCED_SMALL.get(name, FORCED_B)
    exp = want(name, kind, "forced")
    dec, cpu = gpu(name), q.DecoderCPU(code)
    assert dec.describe().startswith("sparse-")
    pri = priors_of(code.n, kind)
    dec.set_priors(*pri)
    cpu.set_priors(*pri)
    assert all(np.array_equal(a, b) for a, b in zip(dec.osd_weights(), cpu.osd_weights()))
    if name == "surf3":
        assert max(yardstick(name).n - r for r in yardstick(name).rank) < 64  # f < lambda = 64: the clamp
    if kind == "two":  # candidates tied at the least score: the lowest index must win
        assert sum(s[3] > 1 for s in exp[10]["sectors"]) >= 1
    else:              # the rule changes a winner on this batch
        assert sum(s[0] != s[1] for s in exp[10]["sectors"]) >= 1
    for lam in LAMS:
        wX, wZ, wf, cnt, swept = exp[lam]["w"]
        assert cnt == 2 * B
        gX, gZ, gf = run_osd_dev(dec, data, lam, 1)
        assert np.array_equal(gf, wf), (lam, "flags")
        assert np.array_equal(gX, wX) and np.array_equal(gZ, wZ), (lam, "estimates")
        with osd_options(cpu, lam, 1):
            cX, cZ, cf = cpu.osd(*data)
        assert np.array_equal(gX, cX) and np.array_equal(gZ, cZ) and np.array_equal(gf, cf), (lam, "CPU engine")
        # the host form of the same handle runs the kernel too, and counts
        with osd_options(dec, lam, 1):
            hX, hZ, hf = dec.osd(*data)
            assert dec.get_option("osd_sectors") == cnt and dec.get_option("osd_cs_sectors") == swept, lam
        assert np.array_equal(hX, wX) and np.array_equal(hZ, wZ) and np.array_equal(hf, wf), lam
    # the rule back at 0 on the same handle: the Hamming kernel's result
    hX, hZ, hf = run_osd_dev(dec, data, 10, 0)
    assert np.array_equal(hX, exp[10]["h"][0]) and np.array_equal(hZ, exp[10]["h"][1]) and np.array_equal(hf, exp[10]["h"][2])


# ---- 2. uniform priors: the weighted kernel against the pinned Hamming kernel ---------------------------------------
@pytest.mark.parametrize("name", ["surf3", "hgp_ham", "G13", "P61"])
def test_uniform_priors_tie_the_weighted_kernel_to_the_hamming_kernel(name):
    code = code_of(name)
    data = forced(name)
    dec = gpu(name)
    dec.set_priors(*priors_of(code.n, "uniform"))
    wX, wZ = dec.osd_weights()
    assert len(set(wX.tolist()) | set(wZ.tolist())) == 1 and wX[0] > 0
    for lam in LAMS:
        a, b = run_osd_dev(dec, data, lam, 0), run_osd_dev(dec, data, lam, 1)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), lam
    # every weight zero: the OSD-0 estimate, nothing swept
    dec.set_priors(*priors_of(code.n, "half"))
    zero = run_osd_dev(dec, data, 0, 0)
    for lam in (10, 64):
        got = run_osd_dev(dec, data, lam, 1)
        assert all(np.array_equal(x, y) for x, y in zip(got, zero)), lam
    with osd_options(dec, 10, 1):
        dec.osd(*data)
        assert dec.get_option("osd_cs_sectors") == 0 and dec.get_option("osd_sectors") == 2 * len(data[5])
    # without priors the option has no effect
    dec.set_priors(None, None)
    a, b = run_osd_dev(dec, data, 10, 0), run_osd_dev(dec, data, 10, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 3. the synchronous calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hgp_ham", "G13"])
def test_synchronous_calls_equal_the_cpu_engine(name):
    p, N, _ = SAMPLED
    code = code_of(name)
    sX, sZ = sampled(name, "random")[:2]
    exp = want(name, "random", "sampled")[10]
    dec, cpu = gpu(name), q.DecoderCPU(code)
    pri = priors_of(code.n, "random")
    dec.set_priors(*pri)
    cpu.set_priors(*pri)
    for score, key in ((1, "w"), (0, "h")):
        with osd_options(cpu, 10, score, osd=1):
            c = cpu.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
            ccnt = (cpu.get_option("osd_sectors"), cpu.get_option("osd_cs_sectors"))
        assert ccnt == (exp[key][3], exp[key][4])
        assert all(np.array_equal(a, b) for a, b in zip(c[:3], exp[key][:3]))
        with osd_options(dec, 10, score, osd=1):
            g = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
            assert "osd" in dec.last_path()
            assert (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors")) == ccnt, score
            for a, b in zip(g[:4], c[:4]):
                assert np.array_equal(a, b), score
            rec, its = dec.decode_batch_packed(sX, sZ, p, N, "syndrome", want_iters=True)
            assert (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors")) == ccnt, score
            assert np.array_equal(rec, pack_records(c[0], c[1], c[2])) and np.array_equal(its, c[3])


# ---- 4. Monte-Carlo ----------------------------------------------------------------------------------------------------------
def test_monte_carlo_with_the_weighted_score():
    """4 096 samples over two calls: the counters equal a host recount from sample_independent_dev's errors and the
    CPU engine's decode of them under the same options, and the two rules sweep different numbers of sectors."""
    name, seed, total, half = "hgp_ham", 0xB1A5ED, 4096, 2048
    code = logical_code(name)
    HX, HZ = matrices(name)
    pX, pZ = prior_vectors(code.n, "random")
    dec, cpu = q.DecoderGPU(code, 0), q.DecoderCPU(code)
    for d in (dec, cpu):
        d.set_priors(pX, pZ)
    tx = torch.empty((total, code.n), dtype=torch.uint8, device=DEV)
    tz = torch.empty_like(tx)
    dec.sample_independent_dev(seed, 0, tx, tz)
    torch.cuda.synchronize()
    x, z = tx.cpu().numpy(), tz.cpu().numpy()
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    swept = {}
    for score in (1, 0):
        with osd_options(cpu, 10, score, osd=1):
            eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, 0.05, 20, "syndrome", want_iters=True)
            exp_cnt = (cpu.get_option("osd_sectors"), cpu.get_option("osd_cs_sectors"))
        exp = count(code, x, z, eX, eZ, fl, it)
        assert exp["synX"] == exp["synZ"] == 0 and exp_cnt[0] >= 100
        with osd_options(dec, 10, score, osd=1):
            got, cnt = {}, [0, 0]
            for start in (0, half):
                r = dec.monte_carlo(seed, start, half, 0.7, 20, "syndrome", batch=768)
                assert "osd" in dec.last_path()
                for k in exp:
                    got[k] = got.get(k, 0) + r[k]
                cnt[0] += dec.get_option("osd_sectors")
                cnt[1] += dec.get_option("osd_cs_sectors")
        assert got == exp, score
        assert tuple(cnt) == exp_cnt, score
        swept[score] = cnt[1]
    assert swept[0] != swept[1]


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------
def test_weighted_osd_dev_in_a_graph_follows_set_priors():
    """osd_dev with the weighted score allocates nothing and synchronises nothing: captured once (one kernel node),
    it replays to the eager result, and after a second set_priors to the result under the new tables."""
    name = "G13"
    code = code_of(name)
    sX, sZ, qf, eX, eZ, flags = data = forced(name)
    B = len(flags)
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    cpu = q.DecoderCPU(code)
    first, second = priors_of(code.n, "random"), priors_of(code.n, "two")
    dec.set_priors(*first)  # allocates the device tables before the capture
    dec.set_option("osd_order", 10)
    dec.set_option("osd_score", 1)
    t = [torch.from_numpy(a).to(DEV) for a in (sX, sZ, qf)]
    cX, cZ, cF = (torch.from_numpy(a).to(DEV) for a in (eX, eZ, flags))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.osd_dev(*t, cX, cZ, cF, stream=s)
    results = []
    for pri, kind in ((first, "random"), (second, "two")):
        dec.set_priors(*pri)  # rewrites the tables the captured kernel reads
        cpu.set_priors(*pri)
        oX, oZ, oF = (torch.from_numpy(a).to(DEV) for a in (eX, eZ, flags))
        dec.osd_dev(*t, oX, oZ, oF)  # eager
        cX.copy_(torch.from_numpy(eX).to(DEV))  # replay on fresh inputs
        cZ.copy_(torch.from_numpy(eZ).to(DEV))
        cF.copy_(torch.from_numpy(flags).to(DEV))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cX, oX) and torch.equal(cZ, oZ) and torch.equal(cF, oF), kind
        wX, wZ, wf = want(name, kind, "forced")[10]["w"][:3]
        assert np.array_equal(cX.cpu().numpy(), wX) and np.array_equal(cZ.cpu().numpy(), wZ), kind
        assert np.array_equal(cF.cpu().numpy(), wf), kind
        with osd_options(cpu, 10, 1):
            hX, hZ, hf = cpu.osd(*data)
        assert np.array_equal(hX, wX) and np.array_equal(hZ, wZ) and np.array_equal(hf, wf)
        results.append((wX, wZ))
    assert not (np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]))


# ---- 6. LDS refusal -----------------------------------------------------------------------------------------------------------
def test_lds_refusal_of_the_weighted_arrays():
    """HX = HZ = [I | I] with 460 checks on 920 qubits: the sweep at lambda = 64 fits one workgroup's 64 KiB under
    the Hamming score and not with the weighted score's arrays; whichever call would make the weighted sweep run
    is refused, and the text says which arrays do not fit."""
    m = 460
    n = 2 * m
    limit = 64 * 1024 // 4
    assert lds_words(m, n, 64, False) <= limit < lds_words(m, n, 64, True)
    assert lds_words(m, n, 10, True) <= limit
    H = np.concatenate([np.eye(m, dtype=np.uint8), np.eye(m, dtype=np.uint8)], axis=1)
    code = q.Quantum_LDPC_Code.createFromMatrices(H, H)
    pri = np.full(n, F32(0.01)), np.full(n, F32(0.02))

    def fresh():
        return q.DecoderGPU(code, 0, engine="sparse")

    dec = fresh()  # the option last
    dec.set_priors(*pri)
    dec.set_option("osd_order", 64)
    with pytest.raises(q.QecError, match=r"\(-4\).*weighted score"):  # QEC_ERR_UNSUPPORTED
        dec.set_option("osd_score", 1)
    assert dec.get_option("osd_score") == 0
    dec.set_option("osd_order", 10)
    dec.set_option("osd_score", 1)  # fits at lambda = 10
    with pytest.raises(q.QecError, match=r"\(-4\).*weighted score"):  # the order last
        dec.set_option("osd_order", 64)
    assert dec.get_option("osd_order") == 10
    dec = fresh()  # the priors last
    dec.set_option("osd_order", 64)
    dec.set_option("osd_score", 1)  # no priors: no effect, nothing to refuse
    with pytest.raises(q.QecError, match=r"\(-4\).*weighted score"):
        dec.set_priors(*pri)
    assert dec.get_priors() is None
    assert q.lib().qec_decoder_set_priors(dec._h, q._ptr(pri[0]), q._ptr(pri[1])) == -4  # QEC_ERR_UNSUPPORTED
    # under the Hamming score the same handle takes the priors and runs the sweep at lambda = 64
    dec.set_option("osd_score", 0)
    dec.set_priors(*pri)
    sX = np.zeros((2, m), dtype=np.uint8)
    sX[:, 3] = 1
    eX, eZ, fl = dec.osd(sX, sX, np.full((2, 4 * m), 0.25, dtype=F32), np.zeros((2, n), dtype=np.uint8),
                         np.zeros((2, n), dtype=np.uint8), np.full(2, 3, dtype=np.uint8))
    assert not fl.any() and np.array_equal((eX @ H.T) & 1, sX) and np.array_equal((eZ @ H.T) & 1, sX)

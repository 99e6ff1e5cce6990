"""Every instantiation of osd_kernel (osd.hip) on every row of the shape table of tests/test_osd_shapes.py, against
its numpy yardstick, bit for bit: estimates, flags, both counters, the inputs unchanged and the guard bytes around the
outputs intact.  The six instantiations are chosen by construction:

  osd0              osd_kernel<false>               bp_method 0, osd_order 0
  osd0-llr          osd_kernel<false, false, true>  bp_method 1, osd_order 0
  cs                osd_kernel<true>                bp_method 0, osd_order > 0, no priors
  cs-llr            osd_kernel<true, false, true>   bp_method 1, osd_order > 0, no priors
  cs-weighted       osd_kernel<true, true>          bp_method 0, osd_order > 0, priors and osd_score 1
  cs-weighted-llr   osd_kernel<true, true, true>    bp_method 1, osd_order > 0, priors and osd_score 1

so test_kernel_matches_the_yardstick[<shape>-<instantiation>] names what ran where.  A combination that the LDS plan
refuses (m2048: lambda = 64, and the weighted score at any lambda) is asserted as refused, with its text, in the same
test.  Then the flags byte at every offset in its aligned word, batches of one, two and three samples, the six
instantiations behind decode_batch on c128, qec_monte_carlo on w31 (n % 8 = 7: 4-byte halves of a record), and the
refusal of codes beyond 2048 qubits or checks."""
import numpy as np
import pytest
import torch

import qec_ldpc_amd as q
from oracle.philox import depolarizing
from test_gpu_general_code import count
from test_gpu_osd import guarded, guards_intact
from test_osd_shapes import (METHODS, ORDERS, OSD_SHAPES, OVERSIZE, SYNC, W31_MC, apply_rule, assert_same, batch, code_of, fits,
                             matrices, oversize_code, repair, sync_syndromes, want, weights_of, yardstick)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SWEEPS = (0, 1, 2)  # QEC_OPT_OSD_SWEEP: per chunk the cheaper form, the "words" form, the "rows" form
# name -> (bp_method, the sweep runs, the rules it runs under)
INSTANCES = {
    "osd0": (0, False, ("h",)),
    "osd0-llr": (1, False, ("h",)),
    "cs": (0, True, ("h",)),
    "cs-llr": (1, True, ("h",)),
    "cs-weighted": (0, True, ("random", "two")),
    "cs-weighted-llr": (1, True, ("random", "two")),
}
_decoders = {}


def gpu(name):
    """One sparse-engine decoder per shape; every test sets what it needs and resets it."""
    if name not in _decoders:
        _decoders[name] = q.DecoderGPU(code_of(name), 0, engine="sparse")
        assert _decoders[name].describe().startswith("sparse-")
    return _decoders[name]


class configured:
    """`with configured(dec, name, method, rule, lam, sweep)`: the options and priors that select an instantiation,
    set in the order in which each is checked against what is already there; all reset behind the block."""

    def __init__(self, dec, name, method, rule, lam, sweep=0, osd=0):
        self.args = (dec, name, method, rule, lam, sweep, osd)

    def __enter__(self):
        dec, name, method, rule, lam, sweep, osd = self.args
        dec.set_option("osd_order", 0)
        apply_rule(dec, name, rule)
        dec.set_option("bp_method", method)
        dec.set_option("osd_sweep", sweep)
        dec.set_option("osd_order", lam)
        dec.set_option("osd_score", int(rule != "h"))
        dec.set_option("osd", osd)
        # what chooses the kernel, read back from the handle
        assert dec.get_option("bp_method") == method and dec.get_option("osd_order") == lam
        assert dec.get_option("osd_score") == int(rule != "h") and (dec.osd_weights() is not None) == (rule != "h")
        if rule != "h":
            assert all(np.array_equal(a, b) for a, b in zip(dec.osd_weights(), weights_of(name, rule)))
        return dec

    def __exit__(self, *exc):
        dec = self.args[0]
        for option in ("osd", "osd_score", "osd_order", "osd_sweep", "bp_method"):
            dec.set_option(option, 0)
        dec.set_priors(None, None)


def run_osd_dev(dec, data, flags_offset=5):
    """osd_dev on fresh guarded copies of the batch -> (eX, eZ, flags) as numpy; the guards and the inputs checked."""
    sX, sZ, soft, eX, eZ, flags = data
    B = len(flags)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (sX, sZ, soft)]
    gX, vX = guarded(eX)
    gZ, vZ = guarded(eZ)
    gF, vF = guarded(flags, offset=flags_offset)
    assert gF.data_ptr() % 4 == 0 and vF.data_ptr() % 4 == flags_offset % 4
    dec.osd_dev(*t, vX, vZ, vF)
    torch.cuda.synchronize()
    assert guards_intact(gX, B) and guards_intact(gZ, B) and guards_intact(gF, B, offset=flags_offset)
    assert np.array_equal(t[0].cpu().numpy(), sX) and np.array_equal(t[1].cpu().numpy(), sZ)  # the inputs are read only
    assert np.array_equal(t[2].cpu().numpy().view(np.uint32), np.ascontiguousarray(soft).view(np.uint32))
    return vX.cpu().numpy(), vZ.cpu().numpy(), vF.cpu().numpy()


def assert_refused(dec, name, method, rule, lam):
    """The LDS plan's refusal of (lambda, score) on this shape: QEC_ERR_UNSUPPORTED with the text that says why, at
    the call that would make the kernel run, and the option as it was."""
    dec.set_option("osd_order", 0)
    apply_rule(dec, name, rule)
    dec.set_option("bp_method", method)
    try:
        if not fits(name, lam, False):  # not even under the Hamming score
            with pytest.raises(q.QecError, match=r"\(-4\).*augmented matrix and the sweep's column vectors need"):
                dec.set_option("osd_order", lam)
            assert dec.get_option("osd_order") == 0
        else:
            assert rule != "h"
            dec.set_option("osd_order", lam)
            with pytest.raises(q.QecError, match=r"\(-4\).*fits in LDS at QEC_OPT_OSD_ORDER = %d under the Hamming score, "
                                                 r"but not with the weighted score's arrays" % lam):
                dec.set_option("osd_score", 1)
            assert dec.get_option("osd_score") == 0
    finally:
        dec.set_option("osd_order", 0)
        dec.set_option("bp_method", 0)
        dec.set_priors(None, None)


# ---- 1. the six instantiations on the seven shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("inst", list(INSTANCES))
@pytest.mark.parametrize("name", list(OSD_SHAPES))
def test_kernel_matches_the_yardstick(name, inst):
    method, cs, rules = INSTANCES[inst]
    dec = gpu(name)
    data = batch(name, method)
    ran = refused = 0
    for rule in rules:
        for lam in (ORDERS[1:] if cs else (0,)):
            if not fits(name, lam, rule != "h"):
                assert_refused(dec, name, method, rule, lam)
                refused += 1
                continue
            expect = want(name, method)[0][lam, rule]
            for sweep in SWEEPS:
                with configured(dec, name, method, rule, lam, sweep):
                    got = run_osd_dev(dec, data)
                assert_same(got, expect[:3], (name, inst, rule, lam, sweep))
            with configured(dec, name, method, rule, lam):  # the host form runs the kernel too, and counts
                host = dec.osd(*data) + (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors"))
            assert_same(host, expect, (name, inst, rule, lam, "qec_osd"))
            ran += 1
    if name == "m2048":
        assert (ran, refused) == {(False, 1): (1, 0), (True, 1): (3, 1), (True, 2): (0, 8)}[cs, len(rules)]
    else:
        assert refused == 0 and ran == len(rules) * (4 if cs else 1)


# ---- 2. the flags byte in its aligned word -----------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_flags_at_every_offset_in_a_word(method):
    """w64, 9 samples, the flags vector 0, 1, 2 and 3 bytes behind a 4-byte boundary: the two sectors of a sample and
    up to four neighbouring samples share the word that atomicAnd works on, in every arrangement."""
    name, lam = "w64", 10
    data = batch(name, method, B=9)
    ys = yardstick(name, method)
    expect = repair(ys, data, {"h": None}, (lam,))[0][lam, "h"]
    assert expect[3] >= 9 and (expect[2] != data[5]).sum() >= 6
    dec = gpu(name)
    for offset in (0, 1, 2, 3):
        with configured(dec, name, method, "h", lam):
            got = run_osd_dev(dec, data, flags_offset=offset)
        assert_same(got, expect[:3], (method, offset))


# ---- 3. the smallest batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [slice(4, 5), slice(6, 8), slice(6, 9)], ids=["B1", "B2", "B3"])
@pytest.mark.parametrize("name", ["w31", "w64", "c128"])
def test_batches_of_one_two_and_three(name, rows):
    """Samples of the shape's batch whose two sectors both failed, as a batch of their own: a grid of 2, 4 and 6
    blocks (the last sample's index even, odd, even)."""
    for method in METHODS:
        data = tuple(np.ascontiguousarray(a[rows]) for a in batch(name, method))
        B = len(data[5])
        assert B == rows.stop - rows.start and ((data[5] & 3) == 3).all()
        for lam, rule in ((0, "h"), (10, "h"), (10, "random")):
            expect = tuple(a[rows] for a in want(name, method)[0][lam, rule][:3])
            assert not (expect[2] & 3).any()
            with configured(gpu(name), name, method, rule, lam):
                got = run_osd_dev(gpu(name), data, flags_offset=3)
            assert_same(got, expect, (name, method, lam, rule, B))


# ---- 4. the synchronous path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_decode_batch_with_osd_on_c128(inst):
    """decode_batch with osd = 1 under the syndrome stop: BP's own soft decode feeds the kernel; held to DecoderCPU
    on the same input, which tests/test_osd_shapes.py holds to the yardstick."""
    name = "c128"
    method, cs, rules = INSTANCES[inst]
    p, N = SYNC[:2]
    sX, sZ = sync_syndromes()
    dec, cpu = gpu(name), q.DecoderCPU(code_of(name))
    lam = 10 if cs else 0
    for rule in rules:
        with configured(cpu, name, method, rule, lam):
            bp = cpu.decode_batch(sX, sZ, p, N, "syndrome")[2]
        failed = int(((bp & 1) != 0).sum() + ((bp & 2) != 0).sum())
        assert failed >= 10, failed  # checked on the CPU first
        with configured(cpu, name, method, rule, lam, osd=1):
            c = cpu.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
            ccnt = (cpu.get_option("osd_sectors"), cpu.get_option("osd_cs_sectors"))
        assert ccnt[0] == failed and not (c[2] & 3).any()
        with configured(dec, name, method, rule, lam, osd=1):
            g = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
            gcnt = (dec.get_option("osd_sectors"), dec.get_option("osd_cs_sectors"))
            path = dec.last_path()
        assert "osd" in path and ("minsum" in path) == bool(method)
        for a, b, what in zip(g[:4], c[:4], ("eX", "eZ", "flags", "iters")):
            assert np.array_equal(a, b), (inst, rule, what)
        assert gcnt == ccnt, (inst, rule)


# ---- 5. Monte-Carlo on w31 -----------------------------------------------------------------------------------------------------
def test_w31_monte_carlo_counters():
    """n = 31: a record's halves are 4 bytes and the last byte of each holds 7 qubits (osd_scatter_kernel).  The
    matrices do not commute, so the check is the reference one.  Every counter equals a host recount from
    DecoderCPU's decode of the same samples."""
    p, N, B, seed = W31_MC
    code = code_of("w31").with_logical("reference")
    HX, HZ = matrices("w31")
    dec, cpu = q.DecoderGPU(code, 0, engine="sparse"), q.DecoderCPU(code)
    assert code.n % 8 == 7 and dec.record_bytes() == 9
    x, z = depolarizing(seed, 0, B, code.n, p)
    sX, sZ = ((x @ HX.T) & 1).astype(np.uint8), ((z @ HZ.T) & 1).astype(np.uint8)
    bp_only = cpu.decode_batch(sX, sZ, p, N, "syndrome")[2]
    assert ((bp_only & 1) != 0).sum() >= 100 and ((bp_only & 2) != 0).sum() >= 10  # BP leaves failures in both sectors
    for d in (dec, cpu):
        d.set_option("osd", 1)
        d.set_option("osd_order", 10)
    eX, eZ, fl, it, _ = cpu.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
    expect = count(code, x, z, eX, eZ, fl, it)
    assert expect["synX"] == expect["synZ"] == 0
    got = dec.monte_carlo(seed, 0, B, p, N, "syndrome", batch=1024)
    assert {k: got[k] for k in expect} == expect
    assert "osd" in dec.last_path()
    assert dec.get_option("osd_sectors") == cpu.get_option("osd_sectors") > 0
    assert dec.get_option("osd_cs_sectors") == cpu.get_option("osd_cs_sectors")


# ---- 6. beyond the kernel's sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OVERSIZE))
def test_oversize_codes_are_refused(name):
    """n = 2049 or 2049 checks: the decoder is created and decodes; whatever would run the OSD kernel answers
    QEC_ERR_UNSUPPORTED and says what the kernel takes.  (DecoderCPU repairs the same code: test_osd_shapes.py.)"""
    code = oversize_code(name)
    assert max(code.n, code.numEqsX, code.numEqsZ) == 2049
    dec = q.DecoderGPU(code, 0, engine="sparse")
    text = r"\(-4\).*OSD: n = %d, %d checks; the kernel takes up to 2048 of each" % (code.n, max(code.numEqsX, code.numEqsZ))
    with pytest.raises(q.QecError, match=text):
        dec.set_option("osd", 1)
    assert dec.get_option("osd") == 0
    B = 2
    qn = (code.numEqsX + code.numEqsZ) * code.stride
    sX, sZ = np.zeros((B, code.numEqsX), dtype=np.uint8), np.zeros((B, code.numEqsZ), dtype=np.uint8)
    soft = np.full((B, qn), 0.25, dtype=np.float32)
    eX, eZ = np.ones((B, code.n), dtype=np.uint8), np.ones((B, code.n), dtype=np.uint8)
    flags = np.full(B, 3, dtype=np.uint8)
    with pytest.raises(q.QecError, match=text):
        dec.osd(sX, sZ, soft, eX, eZ, flags)
    t = [torch.from_numpy(a).to(DEV) for a in (sX, sZ, soft, eX, eZ, flags)]
    with pytest.raises(q.QecError, match=text):
        dec.osd_dev(*t)
    torch.cuda.synchronize()
    for a, b in zip(t[3:], (eX, eZ, flags)):  # nothing ran
        assert np.array_equal(a.cpu().numpy(), b)
    # BP itself takes the code
    out = dec.decode_batch(sX, sZ, 0.05, 3, "syndrome")
    assert not out[0].any() and not out[1].any() and not (out[2] & 3).any()

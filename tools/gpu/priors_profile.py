"""Measurements of the per-qubit priors -> profiles/priors.json.

  scalar  the sparse engine WITHOUT priors on G13, P61 and hgp_ham: 2^16 syndromes, 50 fixed iterations, REPS
          timed decode_batch_dev calls between HIP events after a warm-up.  Uses nothing the commit before the
          priors lacks, so the same file runs there: run it from each tree in turn, several times, and compare
          the medians with the run-to-run spread of one tree.
  cost    the same batches with uniform priors against the scalar call, the two alternating in one process
          (outputs compared first: they must be equal).
  buys    hgp_ham, 2^20 samples drawn with piZ = 10 piX (mean 0.01), syndrome stop, cap 20, OSD-CS lambda 10
          composed on the device (decode, soft decode, osd_dev, records, per-sample outcome): logical errors
          when decoding with the true priors against the uniform prior of equal mean on the same samples.

Usage: python tools/gpu/priors_profile.py [scalar] [cost] [buys] --out profiles/priors.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import qec_ldpc_amd as q  # noqa: E402
from oracle.philox import depolarizing  # noqa: E402
from qec_ldpc_amd.codes import P61, code_path  # noqa: E402

REPS = 15
B, N = 1 << 16, 50
G13 = (3, 3, 6, 13, 3, 2)
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)
F32 = np.float32


def hgp(H1, H2):
    m1, n1 = H1.shape
    m2, n2 = H2.shape
    HX = np.concatenate([np.kron(H1, np.eye(n2, dtype=np.uint8)), np.kron(np.eye(m1, dtype=np.uint8), H2.T)], axis=1)
    HZ = np.concatenate([np.kron(np.eye(n1, dtype=np.uint8), H2), np.kron(H1.T, np.eye(m2, dtype=np.uint8))], axis=1)
    return np.ascontiguousarray(HX, dtype=np.uint8), np.ascontiguousarray(HZ, dtype=np.uint8)


def cases():
    return (("G13", q.QC_LDPC_CSS(*G13), 0.02), ("P61", q.Quantum_LDPC_Code.createFromFile(code_path(P61)), 0.01),
            ("hgp_ham", q.Quantum_LDPC_Code.createFromMatrices(*hgp(HAMMING, HAMMING)), 0.02))


def spread(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "all_ms": ms}


def setup(code, p):
    import torch
    dev = torch.device("cuda", 0)
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    x, z = depolarizing(0x51EC0DE, 0, B, code.n, p)
    tX = torch.from_numpy(code.syndrome(0, x)).to(dev)
    tZ = torch.from_numpy(code.syndrome(1, z)).to(dev)
    mk = lambda: (torch.empty((B, code.n), dtype=torch.uint8, device=dev),  # noqa: E731
                  torch.empty((B, code.n), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev))
    return dec, tX, tZ, mk


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def cmd_scalar():
    rows = []
    for label, code, p in cases():
        dec, tX, tZ, mk = setup(code, p)
        out = mk()
        run = lambda: dec.decode_batch_dev(tX, tZ, p, N, "fixed", *out)  # noqa: E731
        run()
        run()
        ms = [timed(run) for _ in range(REPS)]
        rows.append(dict(spread(ms), case=label, kernel=dec.describe(), B=B, iterations=N, p=p))
        print("scalar", label, "%.3f ms [%.3f, %.3f]" % (rows[-1]["median_ms"], rows[-1]["min_ms"], rows[-1]["max_ms"]), flush=True)
    return rows


def cmd_cost():
    import torch
    rows = []
    for label, code, p in cases():
        dec, tX, tZ, mk = setup(code, p)
        outs = {"scalar": mk(), "priors": mk()}
        uni = F32(2.0) / F32(3.0) * F32(p)

        def run(k):
            dec.set_priors(uni, uni) if k == "priors" else dec.set_priors(None, None)
            return lambda: dec.decode_batch_dev(tX, tZ, p, N, "fixed", *outs[k])

        for k in outs:
            f = run(k)
            f()
            f()
        torch.cuda.synchronize()
        if not all(torch.equal(a, b) for a, b in zip(outs["scalar"], outs["priors"])):
            raise SystemExit("%s: uniform priors differ from the scalar call" % label)
        ms = {k: [] for k in outs}
        for _ in range(REPS):
            for k in outs:  # alternating; set_priors is outside the timed region
                ms[k].append(timed(run(k)))
        r = {"case": label, "kernel": dec.describe(), "B": B, "iterations": N, "p": p,
             "scalar": spread(ms["scalar"]), "priors": spread(ms["priors"])}
        r["ratio_of_medians"] = r["priors"]["median_ms"] / r["scalar"]["median_ms"]
        print("cost", label, "scalar %.3f ms  priors %.3f ms  ratio %.4f" % (
            r["scalar"]["median_ms"], r["priors"]["median_ms"], r["ratio_of_medians"]), flush=True)
        rows.append(r)
    return rows


def cmd_buys():
    import torch
    dev = torch.device("cuda", 0)
    code = q.Quantum_LDPC_Code.createFromMatrices(*hgp(HAMMING, HAMMING)).with_logical("degenerate")
    n, CH, total, seed, lam, cap = code.n, 1 << 16, 1 << 20, 0x51EC0DE, 10, 20
    piX, piZ = F32(0.02 / 11.0), F32(0.2 / 11.0)
    true = (np.full(n, piX, dtype=F32), np.full(n, piZ, dtype=F32))
    mean = F32((float(piX) + float(piZ)) / 2)
    dec = q.DecoderGPU(code, 0, max_batch=CH)
    dec.set_option("osd_order", lam)
    u8 = torch.uint8
    sX = torch.empty((CH, code.numEqsX), dtype=u8, device=dev)
    sZ = torch.empty((CH, code.numEqsZ), dtype=u8, device=dev)
    errp = torch.empty((CH, 2 * ((n + 7) // 8)), dtype=u8, device=dev)
    eX, eZ = torch.empty((CH, n), dtype=u8, device=dev), torch.empty((CH, n), dtype=u8, device=dev)
    jX, jZ = torch.empty_like(eX), torch.empty_like(eX)
    fl, jf, outc = (torch.empty(CH, dtype=u8, device=dev) for _ in range(3))
    qf = torch.empty((CH, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    rec = torch.empty((CH, dec.record_bytes()), dtype=u8, device=dev)
    counts = {k: np.zeros(3, dtype=np.int64) for k in ("true_priors", "uniform_prior")}
    bp_failed = {k: 0 for k in counts}
    for lo in range(0, total, CH):
        dec.set_priors(*true)
        dec.sample_syndrome_dev(seed, lo, 0.0, sX, sZ, errp)  # the true channel's errors
        for k, pri in (("true_priors", true), ("uniform_prior", (mean, mean))):
            dec.set_priors(*pri)
            dec.decode_batch_dev(sX, sZ, 0.0, cap, "syndrome", eX, eZ, fl)
            bp_failed[k] += int(((fl & 3) != 0).sum().item())
            dec.decode_batch_dev(sX, sZ, 0.0, dec.get_option("osd_iterations"), "fixed", jX, jZ, jf, q=qf)
            dec.osd_dev(sX, sZ, qf, eX, eZ, fl)
            dec.pack_decisions_dev(eX, eZ, fl, rec)
            dec.logical_packed_dev(errp, rec, outc)
            counts[k] += np.bincount(outc.cpu().numpy(), minlength=3)[:3]
    # the library's own run under the true priors: the same samples, decode and OSD stage
    dec.set_priors(*true)
    dec.set_option("osd", 1)
    mc = dec.monte_carlo(seed, 0, total, 0.0, cap, "syndrome", batch=CH)
    rows = {"code": code.describe(), "kernel": dec.describe(), "samples": total, "stop": "syndrome", "cap": cap,
            "osd_order": lam, "piX": float(piX), "piZ": float(piZ), "uniform": float(mean),
            "monte_carlo_true_priors": {k: mc[k] for k in ("corrected", "logical", "synX", "synZ")}}
    for k in counts:
        rows[k] = {"corrected": int(counts[k][0]), "logical": int(counts[k][1]), "syndrome_failed": int(counts[k][2]),
                   "bp_left_unsatisfied": bp_failed[k]}
        print("buys", k, rows[k], flush=True)
    print("buys monte_carlo", rows["monte_carlo_true_priors"], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["scalar", "cost", "buys"])
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out = {"build_id": q.build_id(), "method": "HIP events around decode_batch_dev, %d repetitions after a warm-up" % REPS}
    for name, fn in (("scalar", cmd_scalar), ("cost", cmd_cost), ("buys", cmd_buys)):
        if name in a.what:
            out[name] = fn()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Measurements of min-sum under syndrome priors (qec_decoder_set_syndrome_priors)
-> profiles/soft_syndrome.json.

  cost     decode_batch_packed_dev at p = 0.02 (syndromes of the device sampler, unflipped), N = 20, the fixed and the
           syndrome stop, the wave kernels (minsum_wave = 1), flooding and layered, on P61 at 2^16 and 2^20 and on P7,
           QC_LDPC_CSS(3,3,6,13,3,2) and a (4,6,12) code at P = 64 at 2^16: one handle with syndrome priors set (q = 0:
           the same decode through the SOFT kernels) against the same handle with them cleared, alternating launches,
           REPS repetitions after a warm-up.  The fixed-stop ratio is the price of the extra input.
  parent   a handle without syndrome priors, the same rows, from this tree's package and from another tree's
           (--parent-root: the parent commit, built), in alternating child processes: what such a handle launches is
           what it launched before.
  buys     qec_monte_carlo, P61 and P7, p in {0.01, 0.02} x q in {0.01, 0.03}, 2^16 samples, syndrome stop, cap 20:
           with the syndrome priors; without them on the same flipped syndromes (a second handle flips, a handle without
           priors decodes); and the extended code [H | I] under per-column priors on the general sparse kernel, the
           workaround, for the same samples.  Corrected / logical / syndrome-failed, iterations, samples per second.

"differs" of a row: the medians differ by more than the sum of the two spreads (spread = max - min).

Each step runs in a child process of its own, under its own time limit; the first failure stops the tool.

Usage: python tools/gpu/soft_syndrome_profile.py --out profiles/soft_syndrome.json [--parent-root DIR]
       python tools/gpu/soft_syndrome_profile.py --step cost --out fragment.json
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wave_minsum_profile import CAP, REPS, SEED, code_of, spread, timed  # noqa: E402

P_COST = 0.02
# (label, log2 of the batch)
COST = (("P61", 16), ("P61", 20), ("P7", 16), ("G13", 16), ("r4-6-12-64", 16))
BUYS = ("P61", "P7")
BUY_PS, BUY_QS = (0.01, 0.02), (0.01, 0.03)
BUY_SAMPLES = 1 << 16
STEP_LIMIT = 540  # seconds per child


def handle(q, code, B, layered, wave=1, engine="sparse"):
    dec = q.DecoderGPU(code, 0, engine=engine, max_batch=B)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", wave)
    dec.set_option("minsum_schedule", layered)
    return dec


def differs(a, b):
    return bool(abs(a["median_ms"] - b["median_ms"]) > a["spread_ms"] + b["spread_ms"])


def syndromes(q, dec, code, B, p):
    import torch
    dev = torch.device("cuda", 0)
    tX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=dev)
    tZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=dev)
    dec.sample_syndrome_dev(SEED, 0, p, tX, tZ)
    torch.cuda.synchronize()
    return tX, tZ


def step_cost(q):
    import torch
    dev = torch.device("cuda", 0)
    rows = []
    for label, log2b in COST:
        B = 1 << log2b
        code = code_of(q, label)
        for layered in (0, 1):
            dec = handle(q, code, B, layered)
            tX, tZ = syndromes(q, dec, code, B, P_COST)
            dec.set_syndrome_priors(0.0, 0.0)  # allocates the device table once
            for stop in ("fixed", "syndrome"):
                recs = {k: torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev) for k in (0, 1)}
                its = {k: torch.zeros((B, 2), dtype=torch.int32, device=dev) for k in recs}

                def run(soft):
                    if soft:  # outside the timed region
                        dec.set_syndrome_priors(0.0, 0.0)
                    else:
                        dec.set_syndrome_priors(None, None)
                    return lambda: dec.decode_batch_packed_dev(tX, tZ, P_COST, CAP, stop, recs[soft], iters=its[soft])

                for soft in recs:
                    f = run(soft)
                    f()
                    f()
                    assert ("soft" in dec.last_path()) == bool(soft) and "wave" in dec.last_path()
                torch.cuda.synchronize()
                ms = {k: [] for k in recs}
                for _ in range(REPS):
                    for k in recs:  # alternating
                        ms[k].append(timed(run(k)))
                same = bool(torch.equal(recs[0], recs[1]) and torch.equal(its[0], its[1]))
                r = {"code": label, "describe": code.describe(), "kernel": dec.describe(), "layered": layered, "B": B,
                     "p": P_COST, "stop": stop, "N": CAP, "cleared": spread(ms[0]), "soft": spread(ms[1]),
                     "iterations": int(its[1].sum().item()), "same_records": same}
                r["ratio_of_medians"] = r["soft"]["median_ms"] / r["cleared"]["median_ms"]
                r["differs"] = differs(r["cleared"], r["soft"])
                print("cost %s B=2^%d layered=%d %s: cleared %.3f ms (spread %.3f)  soft %.3f ms (spread %.3f)  ratio %.4f  "
                      "differs %s  same records %s" % (label, log2b, layered, stop, r["cleared"]["median_ms"],
                                                       r["cleared"]["spread_ms"], r["soft"]["median_ms"], r["soft"]["spread_ms"],
                                                       r["ratio_of_medians"], r["differs"], same), flush=True)
                rows.append(r)
    return rows


def step_parent(q):
    """A handle without syndrome priors: nothing here that the parent commit lacks."""
    import torch
    dev = torch.device("cuda", 0)
    rows = []
    for label, log2b in COST:
        B = 1 << log2b
        code = code_of(q, label)
        for layered in (0, 1):
            dec = handle(q, code, B, layered)
            tX, tZ = syndromes(q, dec, code, B, P_COST)
            rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
            for stop in ("fixed", "syndrome"):
                run = lambda: dec.decode_batch_packed_dev(tX, tZ, P_COST, CAP, stop, rec)  # noqa: E731
                run()
                run()
                ms = [timed(run) for _ in range(REPS)]
                rows.append(dict(spread(ms), code=label, layered=layered, B=B, p=P_COST, stop=stop, cap=CAP,
                                 build_id=q.build_id()))
                print("parent %s B=2^%d layered=%d %s: %.3f ms (spread %.3f)"
                      % (label, log2b, layered, stop, rows[-1]["median_ms"], rows[-1]["spread_ms"]), flush=True)
    return rows


def extended_code(q, code):
    import numpy as np
    HX, HZ = code.pcm(0), code.pcm(1)
    mX, mZ = HX.shape[0], HZ.shape[0]
    EX = np.concatenate([HX, np.eye(mX, dtype=np.uint8), np.zeros((mX, mZ), dtype=np.uint8)], axis=1)
    EZ = np.concatenate([HZ, np.zeros((mZ, mX), dtype=np.uint8), np.eye(mZ, dtype=np.uint8)], axis=1)
    return q.Quantum_LDPC_Code.createFromMatrices(np.ascontiguousarray(EX), np.ascontiguousarray(EZ))


def step_buys(q):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    B = BUY_SAMPLES
    rows = []
    for label in BUYS:
        code = code_of(q, label)
        n, mX, mZ, nb = code.n, code.numEqsX, code.numEqsZ, (code.n + 7) // 8
        soft = handle(q, code, B, 0)   # with the syndrome priors: qec_monte_carlo, and the flipped syndromes of the others
        blind = handle(q, code, B, 0)  # without them
        ext = extended_code(q, code)
        wide = handle(q, ext, B, 0, wave=0)  # the workaround: the general sparse kernel
        nbe = (ext.n + 7) // 8
        tX = torch.empty((B, mX), dtype=torch.uint8, device=dev)
        tZ = torch.empty((B, mZ), dtype=torch.uint8, device=dev)
        errp = torch.empty((B, 2 * nb), dtype=torch.uint8, device=dev)
        rec = torch.empty((B, blind.record_bytes()), dtype=torch.uint8, device=dev)
        rece = torch.empty((B, wide.record_bytes()), dtype=torch.uint8, device=dev)
        its = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        keep = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        if n % 8:
            keep[-1] = (1 << (n % 8)) - 1
        for p in BUY_PS:
            for qs in BUY_QS:
                soft.set_syndrome_priors(qs, qs)
                pi = np.float32(2.0) / np.float32(3.0) * np.float32(p)
                half = np.full(mX + mZ, 0.5, dtype=np.float32)
                wide.set_priors(np.concatenate([np.full(n, pi, np.float32), np.full(mX, qs, np.float32), half[:mZ]]),
                                np.concatenate([np.full(n, pi, np.float32), half[:mX], np.full(mZ, qs, np.float32)]))
                soft.monte_carlo(SEED, 0, B, p, CAP, "syndrome", batch=B)  # warm-up
                secs, last = [], None
                for _ in range(REPS):
                    last = soft.monte_carlo(SEED, 0, B, p, CAP, "syndrome", batch=B)
                    secs.append(last["totalSeconds"] * 1e3)
                assert {"soft", "wave"} <= soft.last_path()
                out = [dict(spread(secs), decode="syndrome priors (wave SOFT kernels), qec_monte_carlo", corrected=last["corrected"],
                            logical=last["logical"], synX=last["synX"], synZ=last["synZ"],
                            iterations=last["iterationsX"] + last["iterationsZ"])]
                # the same samples through the channel, decoded without the priors and by the workaround
                soft.sample_syndrome_dev(SEED, 0, p, tX, tZ, errp)
                torch.cuda.synchronize()

                def count(records, iters):
                    cnt = torch.zeros(len(q.MC_COUNTERS_ALL), dtype=torch.int64, device=dev)
                    blind.statistics_packed_dev(errp, records, cnt, iters=iters)
                    torch.cuda.synchronize()
                    return dict(zip(q.MC_COUNTERS_ALL, (int(v) for v in cnt.cpu().numpy())))

                for name, dec, records in (("ignoring the syndrome noise (wave kernels), decode only", blind, rec),
                                           ("extended code [H | I] (general sparse kernel), decode only", wide, rece)):
                    run = lambda: dec.decode_batch_packed_dev(tX, tZ, p, CAP, "syndrome", records, iters=its)  # noqa: E731
                    run()
                    ms = [timed(run) for _ in range(REPS)]
                    if dec is wide:  # the data part of the extended records, as records of the base code
                        rec[:, :nb] = records[:, :nb] & keep
                        rec[:, nb:2 * nb] = records[:, nbe:nbe + nb] & keep
                        rec[:, 2 * nb] = records[:, 2 * nbe]
                    c = count(rec, its)
                    out.append(dict(spread(ms), decode=name, corrected=c["corrected"], logical=c["logical"], synX=c["synX"],
                                    synZ=c["synZ"], iterations=c["iterationsX"] + c["iterationsZ"]))
                for r in out:
                    r.update(code=label, p=p, q=qs, samples=B, cap=CAP, samples_per_s=B / (r["median_ms"] * 1e-3))
                    print("buys %s p=%g q=%g %s: corrected %d logical %d syndrome-failed %d / %d iterations %d  %.3f ms "
                          "(spread %.3f), %.2f M samples/s" % (label, p, qs, r["decode"], r["corrected"], r["logical"], r["synX"],
                                                               r["synZ"], r["iterations"], r["median_ms"], r["spread_ms"],
                                                               r["samples_per_s"] / 1e6), flush=True)
                rows += out
    return rows


STEPS = {"cost": step_cost, "parent": step_parent, "buys": step_buys}


def run_step(step, package_root, out):
    sys.path.insert(0, package_root)
    if package_root != ROOT:
        sys.path.insert(1, ROOT)
    import qec_ldpc_amd as q
    with open(out, "w") as f:
        json.dump({"build_id": q.build_id(), "rows": STEPS[step](q)}, f, indent=1)


def child(step, package_root, tmp, tag=""):
    """One step in a process of its own, under its own time limit."""
    frag = os.path.join(tmp, step + tag + ".json")
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--package-root", package_root, "--out", frag]
    subprocess.run(cmd, check=True, timeout=STEP_LIMIT)
    with open(frag) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--step", help="one step, in this process: cost, parent or buys")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose qec_ldpc_amd package (and library) is loaded")
    ap.add_argument("--parent-root", help="the parent commit's built tree, for the comparison without the feature")
    ap.add_argument("--rounds", type=int, default=2, help="back-to-back rounds of that comparison")
    ap.add_argument("--vgprs", help="a JSON file {kernel symbol: VGPRs} to carry along (tools/kbench/isa_diff.py's NEW lines)")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.package_root, a.out)
    tmp = tempfile.mkdtemp(prefix="soft_syndrome_fragments_")
    out = {"method": "HIP events around decode_batch_packed_dev, %d repetitions after a warm-up, syndrome priors set (q = 0) "
                     "and cleared alternating on one handle; qec_monte_carlo wall time, %d repetitions after a warm-up; "
                     "spread = max - min; each step in a process of its own" % (REPS, REPS),
           "cost": [], "parent": [], "buys": []}
    r = child("cost", ROOT, tmp)
    out["build_id"] = r["build_id"]
    out["cost"] = r["rows"]
    with open(a.out, "w") as f:  # what is measured so far survives a later step's failure
        json.dump(out, f, indent=1)
    out["buys"] = child("buys", ROOT, tmp)["rows"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if a.parent_root:
        for k in range(a.rounds):  # the two builds back to back, several times
            for tree, root in (("this", ROOT), ("parent", a.parent_root)):
                for row in child("parent", root, tmp, "_%s_%d" % (tree, k))["rows"]:
                    out["parent"].append(dict(row, tree=tree, round=k))
    if a.vgprs:
        with open(a.vgprs) as f:
            out["vgprs"] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

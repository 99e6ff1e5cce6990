"""Measurements of Relay-BP -> profiles/relay.json.

  buys     what qec_decoder_set_relay buys: qec_monte_carlo on hgp_ham, QC_LDPC_CSS(3,3,6,13,3,2) and P61 (sparse engine),
           degenerate logical check, p in {0.01, 0.02, 0.05}, syndrome stop, caps 20 / 25 / 50 per leg, the same samples
           under the product rule, min-sum alone (scale 160), the relay at L in {1, 5, 17} with S = 1 and at L = 17 with
           S = 5 (tables of q.relay_gammas, seed 1 for X and 2 for Z), each alone and followed by OSD-CS lambda = 10:
           failed samples (logical plus syndrome-failed X / Z), the iteration sums and samples per second.
  cost     the relay kernel at L = 1, gamma = 0 (every output bit the MINSUM kernel's) against the MINSUM kernel of the
           same build: decode_batch_packed_dev, 2^16 syndromes, fixed stop, N = 20, alternating in one process (HIP
           events, REPS repetitions after a warm-up), with both kernels' run-to-run spread.
  norelay  a handle without relay tables, with nothing the parent commit lacks, so the same step runs from another tree's
           package (--package-root): the configurations of the cost rows of profiles/minsum.json (method 0 and method 1,
           fixed stop N = 20 and syndrome stop at the cap, p in {0.01, 0.02, 0.05}).  Run from both trees in turn, several
           times, and compare the medians with the run-to-run spread of each tree.

Without --step the tool runs every step in a child process of its own, each under its own time limit, and stops at the
first one that fails; the children's results are merged into --out.

Usage: python tools/gpu/relay_profile.py --out profiles/relay.json [--parent-root DIR] [--samples N] [--codes a,b]
       python tools/gpu/relay_profile.py --step buys:hgp_ham --out fragment.json
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minsum_profile import B, CODES, PS, REPS, ROOT, SEED, code_of, decode_setup, spread, timed  # noqa: E402

STEP_LIMIT = 560  # seconds per child
# (label, QEC_OPT_BP_METHOD, legs, solutions)
CONFIGS = (("product", 0, 0, 0), ("minsum", 1, 0, 0), ("relay L=1", 1, 1, 1), ("relay L=5", 1, 5, 1), ("relay L=17", 1, 17, 1),
           ("relay L=17 S=5", 1, 17, 5))


def step_buys(q, label, samples_cap):
    cap, samples = CODES[label]
    samples = min(samples, samples_cap)
    code = code_of(q, label).with_logical("degenerate")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    what = {"code": label, "describe": code.describe(), "kernel": dec.describe()}
    rows = []
    for p in PS:
        for osd in (0, 1):
            dec.set_option("osd", osd)
            dec.set_option("osd_order", 10 if osd else 0)
            for name, method, legs, S in CONFIGS:
                dec.set_option("bp_method", method)
                if legs:
                    dec.set_relay(q.relay_gammas(code.n, legs, seed=1), q.relay_gammas(code.n, legs, seed=2), solutions=S)
                else:
                    dec.set_relay(None, None)
                dec.monte_carlo(SEED, 0, min(samples, B), p, cap, "syndrome", batch=B)  # warm-up
                r = dec.monte_carlo(SEED, 0, samples, p, cap, "syndrome", batch=B)
                row = dict(what, p=p, cap=cap, samples=samples, osd_order=10 if osd else None, config=name, bp_method=method,
                           legs=legs or None, solutions=S or None, corrected=r["corrected"], logical=r["logical"],
                           synX=r["synX"], synZ=r["synZ"], failed=samples - r["corrected"], iterationsX=r["iterationsX"],
                           iterationsZ=r["iterationsZ"], osd_sectors=dec.get_option("osd_sectors"),
                           seconds=r["totalSeconds"], samples_per_s=samples / r["totalSeconds"])
                print("buys", row, flush=True)
                rows.append(row)
    return rows


def step_cost(q, label, _):
    import numpy as np
    import torch
    rows = []
    for p in PS:
        code, dec, tX, tZ, mk = decode_setup(q, label, p)
        dec.set_option("bp_method", 1)
        zero = np.zeros((1, code.n), dtype=np.float32)
        recs = {"minsum": mk(), "relay": mk()}

        def run(which):
            if which == "relay":  # outside the timed region
                dec.set_relay(zero, zero)
            else:
                dec.set_relay(None, None)
            return lambda: dec.decode_batch_packed_dev(tX, tZ, p, 20, "fixed", recs[which])

        for which in recs:
            f = run(which)
            f()
            f()
        torch.cuda.synchronize()
        assert torch.equal(recs["minsum"], recs["relay"])  # gamma = 0: the same records
        ms = {k: [] for k in recs}
        for _ in range(REPS):
            for k in recs:  # alternating
                ms[k].append(timed(run(k)))
        r = {"code": label, "kernel": dec.describe(), "B": B, "p": p, "stop": "fixed", "N": 20,
             "minsum": spread(ms["minsum"]), "relay": spread(ms["relay"])}
        r["ratio_of_medians"] = r["relay"]["median_ms"] / r["minsum"]["median_ms"]
        print("cost", label, "p", p, "MINSUM %.3f ms [%.3f, %.3f]  RELAY L=1 gamma=0 %.3f ms [%.3f, %.3f]  ratio %.4f" % (
            r["minsum"]["median_ms"], r["minsum"]["min_ms"], r["minsum"]["max_ms"], r["relay"]["median_ms"],
            r["relay"]["min_ms"], r["relay"]["max_ms"], r["ratio_of_medians"]), flush=True)
        rows.append(r)
    return rows


def step_norelay(q, label, _):
    cap, _ = CODES[label]
    rows = []
    for p in PS:
        code, dec, tX, tZ, mk = decode_setup(q, label, p)
        rec = mk()
        for method in (0, 1):
            dec.set_option("bp_method", method)
            for stop, N in (("fixed", 20), ("syndrome", cap)):
                run = lambda: dec.decode_batch_packed_dev(tX, tZ, p, N, stop, rec)  # noqa: E731
                run()
                run()
                ms = [timed(run) for _ in range(REPS)]
                rows.append(dict(spread(ms), code=label, kernel=dec.describe(), B=B, p=p, bp_method=method, stop=stop, N=N,
                                 build_id=q.build_id()))
                print("norelay", label, p, method, stop, "%.3f ms [%.3f, %.3f]" % (
                    rows[-1]["median_ms"], rows[-1]["min_ms"], rows[-1]["max_ms"]), flush=True)
    return rows


STEPS = {"buys": step_buys, "cost": step_cost, "norelay": step_norelay}


def run_step(step, package_root, out, samples):
    sys.path.insert(0, package_root)
    if package_root != ROOT:
        sys.path.insert(1, ROOT)  # oracle/ (the Philox restatement) comes from this tree
    import qec_ldpc_amd as q
    kind, label = step.split(":")
    with open(out, "w") as f:
        json.dump({"build_id": q.build_id(), "rows": STEPS[kind](q, label, samples)}, f, indent=1)


def child(step, package_root, tmp, samples):
    """One step in a process of its own, under its own time limit."""
    frag = os.path.join(tmp, step.replace(":", "_") + ".json")
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--package-root", package_root, "--out", frag,
           "--samples", str(samples)]
    subprocess.run(cmd, check=True, timeout=STEP_LIMIT)
    with open(frag) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--step", help="one step, in this process: buys|cost|norelay:CODE")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose qec_ldpc_amd package (and library) is loaded")
    ap.add_argument("--parent-root", help="the parent commit's built tree, for the no-relay comparison")
    ap.add_argument("--rounds", type=int, default=3, help="back-to-back rounds of the no-relay comparison")
    ap.add_argument("--samples", type=int, default=1 << 20, help="at most this many Monte-Carlo samples per row")
    ap.add_argument("--codes", default=",".join(CODES), help="the codes to run, of " + ",".join(CODES))
    ap.add_argument("--kinds", default="buys,cost,norelay", help="the steps to run")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.package_root, a.out, a.samples)
    tmp = os.path.join(os.path.dirname(os.path.abspath(a.out)), ".relay_fragments")
    os.makedirs(tmp, exist_ok=True)
    codes, kinds = a.codes.split(","), a.kinds.split(",")
    out = {"method": "qec_monte_carlo counters and wall time (one warm-up batch before each run); HIP events around "
                     "decode_batch_packed_dev, %d repetitions after a warm-up; each step in a process of its own" % REPS,
           "buys": [], "cost": [], "norelay": []}
    if "buys" in kinds:
        for label in codes:
            r = child("buys:" + label, ROOT, tmp, a.samples)
            out["build_id"] = r["build_id"]
            out["buys"] += r["rows"]
    if "cost" in kinds:
        for label in codes:
            out["cost"] += child("cost:" + label, ROOT, tmp, a.samples)["rows"]
    if "norelay" in kinds and a.parent_root:
        for k in range(a.rounds):  # the two builds back to back, several times
            for tree, root in (("this", ROOT), ("parent", a.parent_root)):
                for label in codes:
                    for row in child("norelay:" + label, root, tmp, a.samples)["rows"]:
                        out["norelay"].append(dict(row, tree=tree, round=k))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()

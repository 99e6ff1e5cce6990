"""Measurements of layered min-sum (QEC_OPT_MINSUM_SCHEDULE) -> profiles/minsum_layered.json.

One sparse-engine handle per code under min-sum at scale 160, option 0 (flooding) against option 1 (layered),
alternating launches in one process; medians and each side's run-to-run spread (max - min over the repetitions).

  cost     decode_batch_packed_dev at p = 0.02 and 0.05 (syndromes of the device sampler), the fixed stop with N = 20 (the
           ratio is the cost of an iteration) and the syndrome stop with cap 20 (the ratio is the gain), on P61, P7,
           QC_LDPC_CSS(3,3,6,13,3,2) and a (4,6,12) code at P = 64: the wave kernels (minsum_wave = 1) at 2^16
           syndromes, P61 also at 2^20, and the sparse kernels (minsum_wave = 0) at 2^16.  HIP events, REPS repetitions
           after a warm-up.
  runs     qec_monte_carlo with its counters, syndrome stop with cap 20, 2^16 samples: P61 (wave kernels) at p = 0.01 /
           0.02 / 0.05, and hgp_ham (a general code: the sparse kernels) at p = 0.02 / 0.05.
  option0  option 0 alone, with nothing the parent commit lacks, so the same step runs from another tree's package
           (--parent-root): what a handle launches with the option at 0 is what it launched before.

"differs" of a row: the medians differ by more than the sum of the two spreads.

Each step runs in a child process of its own, under its own time limit; the first failure stops the tool.

Usage: python tools/gpu/minsum_layered_profile.py --out profiles/minsum_layered.json [--parent-root DIR]
       python tools/gpu/minsum_layered_profile.py --step cost:P61:16:1 --out fragment.json
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
from serial_profile import HAMMING, hgp  # noqa: E402
from wave_minsum_profile import CAP, REPS, SEED, code_of as wave_code_of, spread, timed  # noqa: E402

PS = (0.02, 0.05)
# (label, log2 of the batch, minsum_wave)
COST = (("P61", 16, 1), ("P61", 20, 1), ("P7", 16, 1), ("G13", 16, 1), ("r4-6-12-64", 16, 1),
        ("P61", 16, 0), ("P7", 16, 0), ("G13", 16, 0), ("r4-6-12-64", 16, 0))
RUNS = {"P61": (1, (0.01, 0.02, 0.05)), "hgp_ham": (0, (0.02, 0.05))}  # label -> minsum_wave, the p
RUN_SAMPLES = 1 << 16
STEP_LIMIT = 420  # seconds per child


def code_of(q, label):
    if label == "hgp_ham":
        return q.Quantum_LDPC_Code.createFromMatrices(*hgp(HAMMING, HAMMING)).with_logical("degenerate")
    return wave_code_of(q, label)


def handle(q, code, B, wave):
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_wave", wave)
    return dec


def differs(a, b):
    return bool(abs(a["median_ms"] - b["median_ms"]) > a["spread_ms"] + b["spread_ms"])


def step_cost(q, label, log2b, wave):
    import torch
    B, wave = 1 << int(log2b), int(wave)
    dev = torch.device("cuda", 0)
    code = code_of(q, label)
    dec = handle(q, code, B, wave)
    rows = []
    for p in PS:
        tX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=dev)
        tZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=dev)
        dec.sample_syndrome_dev(SEED, 0, p, tX, tZ)
        torch.cuda.synchronize()
        for stop in ("fixed", "syndrome"):
            recs = {k: torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev) for k in (0, 1)}
            its = {k: torch.zeros((B, 2), dtype=torch.int32, device=dev) for k in recs}

            def run(option):
                dec.set_option("minsum_schedule", option)  # outside the timed region
                return lambda: dec.decode_batch_packed_dev(tX, tZ, p, CAP, stop, recs[option], iters=its[option])

            for option in recs:
                f = run(option)
                f()
                f()
                assert ("serial" in dec.last_path()) == bool(option) and ("wave" in dec.last_path()) == bool(wave)
            torch.cuda.synchronize()
            ms = {k: [] for k in recs}
            for _ in range(REPS):
                for k in recs:  # alternating
                    ms[k].append(timed(run(k)))
            r = {"code": label, "describe": code.describe(), "kernel": dec.describe(), "minsum_wave": wave, "B": B, "p": p,
                 "stop": stop, "N": CAP, "option0": spread(ms[0]), "option1": spread(ms[1]),
                 "iterations0": int(its[0].sum().item()), "iterations1": int(its[1].sum().item()),
                 "failed0": int((recs[0][:, -1] & 3).ne(0).sum().item()), "failed1": int((recs[1][:, -1] & 3).ne(0).sum().item())}
            r["ratio_of_medians"] = r["option1"]["median_ms"] / r["option0"]["median_ms"]
            r["differs"] = differs(r["option0"], r["option1"])
            print("cost %s wave=%d B=2^%s p=%g %s: option 0 %.3f ms (spread %.3f)  option 1 %.3f ms (spread %.3f)  ratio %.4f  "
                  "differs %s  iterations %d / %d  failed %d / %d"
                  % (label, wave, log2b, p, stop, r["option0"]["median_ms"], r["option0"]["spread_ms"],
                     r["option1"]["median_ms"], r["option1"]["spread_ms"], r["ratio_of_medians"], r["differs"],
                     r["iterations0"], r["iterations1"], r["failed0"], r["failed1"]), flush=True)
            rows.append(r)
    return rows


def step_runs(q, label, *_):
    wave, ps = RUNS[label]
    code = code_of(q, label)
    B = RUN_SAMPLES
    dec = handle(q, code, B, wave)
    rows = []
    for p in ps:
        secs, last = {0: [], 1: []}, {}
        for option in secs:
            dec.set_option("minsum_schedule", option)
            dec.monte_carlo(SEED, 0, B, p, CAP, "syndrome", batch=B)  # warm-up
        for _ in range(REPS):
            for option in secs:  # alternating
                dec.set_option("minsum_schedule", option)
                last[option] = dec.monte_carlo(SEED, 0, B, p, CAP, "syndrome", batch=B)
                secs[option].append(last[option]["totalSeconds"] * 1e3)
        pair = []
        for option in secs:
            r = last[option]
            row = dict(spread(secs[option]), code=label, minsum_schedule=option, minsum_wave=wave, kernel=dec.describe(), p=p,
                       cap=CAP, samples=B, corrected=r["corrected"], logical=r["logical"], synX=r["synX"], synZ=r["synZ"],
                       iterationsX=r["iterationsX"], iterationsZ=r["iterationsZ"])
            row["samples_per_s"] = B / (row["median_ms"] * 1e-3)
            print("runs %s p=%g option %d: %.3f ms (spread %.3f), %.2f M samples/s, syndrome-failed sectors %d / %d, "
                  "iterations %d / %d, logical %d" % (label, p, option, row["median_ms"], row["spread_ms"],
                                                      row["samples_per_s"] / 1e6, row["synX"], row["synZ"], row["iterationsX"],
                                                      row["iterationsZ"], row["logical"]), flush=True)
            pair.append(row)
        for row in pair:
            row["differs"] = differs(pair[0], pair[1])
        rows += pair
    return rows


def step_option0(q, label, log2b, wave):
    import torch
    B, wave = 1 << int(log2b), int(wave)
    dev = torch.device("cuda", 0)
    code = code_of(q, label)
    dec = handle(q, code, B, wave)
    p = 0.02
    tX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=dev)
    tZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=dev)
    dec.sample_syndrome_dev(SEED, 0, p, tX, tZ)
    rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    rows = []
    for stop in ("syndrome", "fixed"):
        run = lambda: dec.decode_batch_packed_dev(tX, tZ, p, CAP, stop, rec)  # noqa: E731
        run()
        run()
        ms = [timed(run) for _ in range(REPS)]
        rows.append(dict(spread(ms), code=label, minsum_wave=wave, B=B, p=p, stop=stop, cap=CAP, build_id=q.build_id()))
        print("option0 %s wave=%d %s: %.3f ms (spread %.3f)" % (label, wave, stop, rows[-1]["median_ms"], rows[-1]["spread_ms"]),
              flush=True)
    return rows


STEPS = {"cost": step_cost, "runs": step_runs, "option0": step_option0}


def run_step(step, package_root, out):
    sys.path.insert(0, package_root)
    if package_root != ROOT:
        sys.path.insert(1, ROOT)
    import qec_ldpc_amd as q
    kind, *args = step.split(":")
    with open(out, "w") as f:
        json.dump({"build_id": q.build_id(), "rows": STEPS[kind](q, *args)}, f, indent=1)


def child(step, package_root, tmp):
    """One step in a process of its own, under its own time limit."""
    frag = os.path.join(tmp, step.replace(":", "_") + ".json")
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--package-root", package_root, "--out", frag]
    subprocess.run(cmd, check=True, timeout=STEP_LIMIT)
    with open(frag) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--step", help="one step, in this process: cost:CODE:LOG2B:WAVE, runs:CODE or option0:CODE:LOG2B:WAVE")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose qec_ldpc_amd package (and library) is loaded")
    ap.add_argument("--parent-root", help="the parent commit's built tree, for the option-0 comparison")
    ap.add_argument("--rounds", type=int, default=2, help="back-to-back rounds of the option-0 comparison")
    ap.add_argument("--vgprs", help="a JSON file {kernel symbol: VGPRs} to carry along (tools/kbench/isa_diff.py's NEW lines)")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.package_root, a.out)
    tmp = tempfile.mkdtemp(prefix="minsum_layered_fragments_")
    out = {"method": "HIP events around decode_batch_packed_dev, %d repetitions after a warm-up, option 0 and option 1 "
                     "alternating on one handle; qec_monte_carlo wall time, %d alternating repetitions after a warm-up; "
                     "spread = max - min; each step in a process of its own" % (REPS, REPS),
           "cost": [], "runs": [], "option0": []}
    for label, log2b, wave in COST:
        r = child("cost:%s:%d:%d" % (label, log2b, wave), ROOT, tmp)
        out["build_id"] = r["build_id"]
        out["cost"] += r["rows"]
        with open(a.out, "w") as f:  # what is measured so far survives a later step's failure
            json.dump(out, f, indent=1)
    for label in RUNS:
        out["runs"] += child("runs:" + label, ROOT, tmp)["rows"]
    if a.parent_root:
        for k in range(a.rounds):  # the two builds back to back, several times
            for tree, root in (("this", ROOT), ("parent", a.parent_root)):
                for label, log2b, wave in (("P61", 16, 1), ("P61", 16, 0)):
                    for row in child("option0:%s:%d:%d" % (label, log2b, wave), root, tmp)["rows"]:
                        out["option0"].append(dict(row, tree=tree, round=k))
    if a.vgprs:
        with open(a.vgprs) as f:
            out["vgprs"] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

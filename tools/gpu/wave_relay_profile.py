"""Measurements of the wave relay kernels (QEC_OPT_RELAY_WAVE) -> profiles/wave_relay.json.

One sparse-engine handle per code under min-sum at scale 160 with relay tables (relay_gammas, seed 1 for sector X and 2
for Z), option 0 (the sparse RELAY kernels, bp_sparse_kernel with BODY = kRelay) against option 1 (the wave kernels of
bp_wave_relay.hip),
alternating launches in one process; medians and each side's run-to-run spread (max - min over the repetitions).  The
baseline is always the option-0 run.

  cost   decode_batch_packed_dev at p = 0.02 (syndromes of the device sampler), N = 20 per leg, the fixed stop and the
         syndrome stop, under two tables -- L = 5 legs with S = 1, and L = 17 legs with S = 5 -- on P61, P7,
         QC_LDPC_CSS(3,3,6,13,3,2) and a (4,6,12) code at P = 64, 2^16 syndromes each; P61 also at 2^20.  HIP events,
         REPS repetitions after a warm-up; the outputs of the two options are compared before anything is timed.
  runs   qec_monte_carlo on P61 at p = 0.01 / 0.02 / 0.05, 2^16 samples, syndrome stop with cap 20, L = 5 and S = 1:
         option 0 and option 1, equal counters asserted.

"done" of a cost row: the option-1 median lies below the option-0 median by more than the sum of the two spreads.

Each step runs in a child process of its own, under its own time limit; the first failure stops the tool.

Usage: python tools/gpu/wave_relay_profile.py --out profiles/wave_relay.json
       python tools/gpu/wave_relay_profile.py --step cost:P61:16 --out fragment.json
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
from wave_minsum_profile import code_of, spread, timed  # noqa: E402  (the codes and the timing of section 7.15)

REPS = 15
SEED = 0x51EC0DE
P_COST = 0.02
CAP = 20
# label -> log2 of the batches
COST = {"P61": (16, 20), "P7": (16,), "G13": (16,), "r4-6-12-64": (16,)}
TABLES = ((5, 1), (17, 5))  # (legs, solutions)
RUN_PS = (0.01, 0.02, 0.05)
RUN_SAMPLES = 1 << 16
STEP_LIMIT = 420  # seconds per child


def relay_handle(q, code, B, legs, solutions):
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    dec.set_option("bp_method", 1)
    dec.set_relay(q.relay_gammas(code.n, legs, seed=1), q.relay_gammas(code.n, legs, seed=2), solutions=solutions)
    return dec


def step_cost(q, label, log2b):
    import torch
    B = 1 << int(log2b)
    dev = torch.device("cuda", 0)
    code = code_of(q, label)
    rows = []
    for legs, solutions in TABLES:
        dec = relay_handle(q, code, B, legs, solutions)
        tX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=dev)
        tZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=dev)
        dec.sample_syndrome_dev(SEED, 0, P_COST, tX, tZ)
        torch.cuda.synchronize()
        names = {}
        for option in (0, 1):
            dec.set_option("relay_wave", option)
            names[option] = dec.describe()
        for stop in ("fixed", "syndrome"):
            recs = {k: torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev) for k in (0, 1)}
            its = {k: torch.zeros((B, 2), dtype=torch.int32, device=dev) for k in recs}

            def run(option):
                dec.set_option("relay_wave", option)  # outside the timed region
                return lambda: dec.decode_batch_packed_dev(tX, tZ, P_COST, CAP, stop, recs[option], iters=its[option])

            for option in recs:
                f = run(option)
                f()
                f()
                assert ("wave" in dec.last_path()) == bool(option) and "relay" in dec.last_path()
            torch.cuda.synchronize()
            assert torch.equal(recs[0], recs[1]) and torch.equal(its[0], its[1])  # the same bits
            ms = {k: [] for k in recs}
            for _ in range(REPS):
                for k in recs:  # alternating
                    ms[k].append(timed(run(k)))
            r = {"code": label, "describe": code.describe(), "kernel0": names[0], "kernel1": names[1], "B": B, "p": P_COST,
                 "stop": stop, "N": CAP, "legs": legs, "solutions": solutions, "option0": spread(ms[0]),
                 "option1": spread(ms[1]), "iterations": int(its[1].sum().item()),
                 "failed": int((recs[1][:, -1] & 3).ne(0).sum().item())}
            r["ratio_of_medians"] = r["option1"]["median_ms"] / r["option0"]["median_ms"]
            r["done"] = bool(r["option1"]["median_ms"] <
                             r["option0"]["median_ms"] - (r["option0"]["spread_ms"] + r["option1"]["spread_ms"]))
            print("cost %s B=2^%s L=%d S=%d %s: option 0 %.3f ms (spread %.3f)  option 1 %.3f ms (spread %.3f)  ratio %.4f  "
                  "done %s" % (label, log2b, legs, solutions, stop, r["option0"]["median_ms"], r["option0"]["spread_ms"],
                               r["option1"]["median_ms"], r["option1"]["spread_ms"], r["ratio_of_medians"], r["done"]),
                  flush=True)
            rows.append(r)
        del dec
    return rows


def step_runs(q, label, _):
    code = code_of(q, label)
    B = RUN_SAMPLES
    legs, solutions = TABLES[0]
    rows = []
    handles = (("relay option 0", relay_handle(q, code, B, legs, solutions), 0),
               ("relay option 1", relay_handle(q, code, B, legs, solutions), 1))
    for _, dec, option in handles:
        dec.set_option("relay_wave", option)
    for p in RUN_PS:
        secs = {name: [] for name, _, _ in handles}
        last = {}
        for name, dec, _ in handles:
            dec.monte_carlo(SEED, 0, B, p, CAP, "syndrome", batch=B)  # warm-up
        for _ in range(REPS):
            for name, dec, _ in handles:  # alternating
                last[name] = dec.monte_carlo(SEED, 0, B, p, CAP, "syndrome", batch=B)
                secs[name].append(last[name]["totalSeconds"] * 1e3)
        for name, dec, option in handles:
            r = last[name]
            row = dict(spread(secs[name]), code=label, handle=name, kernel=dec.describe(), p=p, cap=CAP, samples=B,
                       legs=legs, solutions=solutions, corrected=r["corrected"], failed=B - r["corrected"], synX=r["synX"],
                       synZ=r["synZ"], iterationsX=r["iterationsX"], iterationsZ=r["iterationsZ"])
            row["samples_per_s"] = B / (row["median_ms"] * 1e-3)
            print("runs %s p=%g %s: %.3f ms (spread %.3f), %.1f M samples/s, failed %d"
                  % (label, p, name, row["median_ms"], row["spread_ms"], row["samples_per_s"] / 1e6, row["failed"]), flush=True)
            rows.append(row)
        a, b = last["relay option 0"], last["relay option 1"]
        assert all(a[k] == b[k] for k in a if not k.endswith("Seconds"))  # the same counters
    return rows


STEPS = {"cost": step_cost, "runs": step_runs}


def run_step(step, out):
    sys.path.insert(0, ROOT)
    import qec_ldpc_amd as q
    kind, label, arg = (step.split(":") + [""])[:3]
    with open(out, "w") as f:
        json.dump({"build_id": q.build_id(), "rows": STEPS[kind](q, label, arg)}, f, indent=1)


def child(step, tmp):
    """One step in a process of its own, under its own time limit."""
    frag = os.path.join(tmp, step.replace(":", "_") + ".json")
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--out", frag]
    subprocess.run(cmd, check=True, timeout=STEP_LIMIT)
    with open(frag) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--step", help="one step, in this process: cost:CODE:LOG2B or runs:CODE")
    ap.add_argument("--vgprs", help="a JSON file {kernel symbol: VGPRs} to carry along (tools/kbench/isa_diff.py's NEW lines)")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.out)
    tmp = tempfile.mkdtemp(prefix="wave_relay_fragments_")
    out = {"method": "HIP events around decode_batch_packed_dev, %d repetitions after a warm-up, option 0 and option 1 "
                     "alternating on one handle; qec_monte_carlo wall time, %d alternating repetitions after a warm-up; "
                     "spread = max - min; each step in a process of its own" % (REPS, REPS),
           "cost": [], "runs": []}
    for label, sizes in COST.items():
        for log2b in sizes:
            r = child("cost:%s:%d" % (label, log2b), tmp)
            out["build_id"] = r["build_id"]
            out["cost"] += r["rows"]
    out["runs"] += child("runs:P61", tmp)["rows"]
    p61 = [r for r in out["cost"] if r["code"] == "P61"]
    out["done"] = bool(p61) and all(r["done"] for r in p61)
    if a.vgprs:
        with open(a.vgprs) as f:
            out["vgprs"] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)
    print("done (P61, both stop rules, both batch sizes, both tables):", out["done"])


if __name__ == "__main__":
    main()

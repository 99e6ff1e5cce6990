"""Measurements of the prior-weighted OSD-CS score -> profiles/osd_weighted.json.

The channel: the [[58,16]] hypergraph product of two [7,4] Hamming codes with qubit-to-qubit priors, log-uniform in
[0.003, 0.25] (the draw of prior_vectors in tests/test_priors.py), errors drawn from the priors themselves; syndrome
stop, cap 20, OSD-CS at lambda = 10 and 60.

  mc      2^20 samples through monte_carlo under each rule: corrected, logical, repaired and swept sectors, and
          samples/s (wall clock around the call, REPS runs per rule, the rules alternating).
  kernel  the elimination kernel alone: one chunk of 2^16 samples decoded on the device, then osd_dev timed
          between HIP events under each rule on fresh copies of the estimates (REPS runs, alternating).

  run     one monte_carlo call of 2^20 samples at --order L --score R and nothing else, for a kernel trace:
            rocprofv3 --kernel-trace --stats --output-format csv -d DIR/o10_s1 -o run -- \
                python tools/gpu/osd_weighted_profile.py run --order 10 --score 1
  trace   --dir DIR: the *kernel_trace.csv files under DIR/o<L>_s<R>/ reduced to the time per kernel of each run.

A tree without the "osd_score" option (the commit before it) runs the Hamming half of both, so the same file
gives the parent's numbers: run it from each tree in turn and compare the Hamming rows with the run-to-run spread.

Usage: python tools/gpu/osd_weighted_profile.py [mc] [kernel] [trace --dir DIR] --out profiles/osd_weighted.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import qec_ldpc_amd as q  # noqa: E402

REPS = 5
TOTAL, CH, CAP, SEED = 1 << 20, 1 << 16, 20, 0x51EC0DE
LAMS = (10, 60)
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)
F32 = np.float32
RULES = (("hamming", 0), ("weighted", 1)) if "osd_score" in q.OPTION else (("hamming", 0),)


def hgp(H1, H2):
    m1, n1 = H1.shape
    m2, n2 = H2.shape
    HX = np.concatenate([np.kron(H1, np.eye(n2, dtype=np.uint8)), np.kron(np.eye(m1, dtype=np.uint8), H2.T)], axis=1)
    HZ = np.concatenate([np.kron(np.eye(n1, dtype=np.uint8), H2), np.kron(H1.T, np.eye(m2, dtype=np.uint8))], axis=1)
    return np.ascontiguousarray(HX, dtype=np.uint8), np.ascontiguousarray(HZ, dtype=np.uint8)


def random_priors(n, seed=20240611):
    """prior_vectors(n, "random") of tests/test_priors.py, draw for draw."""
    rng = np.random.default_rng(seed + n)
    out = []
    for _ in range(2):
        out.append(np.exp(rng.uniform(np.log(0.003), np.log(0.25), n)).astype(F32))
        rng.choice(n, 3, replace=False)
    return out[0], out[1]


def set_rule(dec, rule):
    if "osd_score" in q.OPTION:
        dec.set_option("osd_score", rule)


def spread(v):
    s = sorted(v)
    return {"median": statistics.median(s), "min": s[0], "max": s[-1], "all": v}


def make():
    code = q.Quantum_LDPC_Code.createFromMatrices(*hgp(HAMMING, HAMMING)).with_logical("degenerate")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=CH)
    dec.set_priors(*random_priors(code.n))
    return code, dec


def cmd_mc():
    import torch
    code, dec = make()
    dec.set_option("osd", 1)
    rows = []
    for lam in LAMS:
        dec.set_option("osd_order", lam)
        res = {name: {"samples_per_s": []} for name, _ in RULES}
        for rep in range(REPS + 1):  # the first run of each rule warms up
            for name, rule in RULES:
                set_rule(dec, rule)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mc = dec.monte_carlo(SEED, 0, TOTAL, 0.0, CAP, "syndrome", batch=CH)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    res[name]["samples_per_s"].append(TOTAL / dt)
                res[name].update({k: mc[k] for k in ("corrected", "logical", "synX", "synZ")},
                                 osd_sectors=dec.get_option("osd_sectors"), osd_cs_sectors=dec.get_option("osd_cs_sectors"))
        for name, _ in RULES:
            res[name]["samples_per_s"] = spread(res[name]["samples_per_s"])
            print("mc lambda", lam, name, {k: v for k, v in res[name].items() if k != "samples_per_s"},
                  "%.3g samples/s" % res[name]["samples_per_s"]["median"], flush=True)
        rows.append(dict(res, osd_order=lam))
    return {"code": code.describe(), "kernel": dec.describe(), "samples": TOTAL, "batch": CH, "stop": "syndrome",
            "cap": CAP, "priors": "log-uniform in [0.003, 0.25] per qubit and sector; errors drawn from them", "runs": rows}


def cmd_kernel():
    import torch
    dev = torch.device("cuda", 0)
    code, dec = make()
    n, u8 = code.n, torch.uint8
    sX = torch.empty((CH, code.numEqsX), dtype=u8, device=dev)
    sZ = torch.empty((CH, code.numEqsZ), dtype=u8, device=dev)
    errp = torch.empty((CH, 2 * ((n + 7) // 8)), dtype=u8, device=dev)
    eX, eZ = torch.empty((CH, n), dtype=u8, device=dev), torch.empty((CH, n), dtype=u8, device=dev)
    jX, jZ = torch.empty_like(eX), torch.empty_like(eX)
    fl, jf = torch.empty(CH, dtype=u8, device=dev), torch.empty(CH, dtype=u8, device=dev)
    qf = torch.empty((CH, (code.numEqsX + code.numEqsZ) * code.stride), dtype=torch.float32, device=dev)
    dec.sample_syndrome_dev(SEED, 0, 0.0, sX, sZ, errp)
    dec.decode_batch_dev(sX, sZ, 0.0, CAP, "syndrome", eX, eZ, fl)
    dec.decode_batch_dev(sX, sZ, 0.0, dec.get_option("osd_iterations"), "fixed", jX, jZ, jf, q=qf)
    torch.cuda.synchronize()
    failed = int(((fl & 1) != 0).sum().item() + ((fl & 2) != 0).sum().item())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    for lam in (0,) + LAMS:
        dec.set_option("osd_order", lam)
        ms = {name: [] for name, _ in RULES}
        for rep in range(REPS + 1):
            for name, rule in RULES:
                set_rule(dec, rule)
                cX, cZ, cf = eX.clone(), eZ.clone(), fl.clone()
                torch.cuda.synchronize()
                e0.record()
                dec.osd_dev(sX, sZ, qf, cX, cZ, cf)
                e1.record()
                e1.synchronize()
                if rep:
                    ms[name].append(e0.elapsed_time(e1))
        r = {"osd_order": lam, "failed_sectors": failed, "batch": CH}
        for name, _ in RULES:
            r[name + "_ms"] = spread(ms[name])
        if len(RULES) == 2:
            r["ratio_of_medians"] = r["weighted_ms"]["median"] / r["hamming_ms"]["median"]
        print("kernel lambda", lam, {k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()}, flush=True)
        rows.append(r)
    return rows


def cmd_run(order, score):
    import torch
    code, dec = make()
    dec.set_option("osd", 1)
    dec.set_option("osd_order", order)
    set_rule(dec, score)
    mc = dec.monte_carlo(SEED, 0, TOTAL, 0.0, CAP, "syndrome", batch=CH)
    torch.cuda.synchronize()
    print(json.dumps({"osd_order": order, "osd_score": score, "logical": mc["logical"],
                      "osd_cs_sectors": dec.get_option("osd_cs_sectors")}))


def cmd_trace(d):
    """Per run directory o<L>_s<R>: kernel -> [launches, total ms] of the one monte_carlo call."""
    out = {}
    for run in sorted(glob.glob(os.path.join(d, "o*_s*"))):
        durs = {}
        for f in glob.glob(os.path.join(run, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                k = row["Kernel_Name"].split("(")[0].split("::")[-1]
                k += "<" + row["Kernel_Name"].split("<", 1)[1].split(">")[0] + ">" if k.startswith("osd_kernel") else ""
                e = durs.setdefault(k, [0, 0.0])
                e[0] += 1
                e[1] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
        out[os.path.basename(run)] = dict(sorted(durs.items(), key=lambda kv: -kv[1][1]))
        out[os.path.basename(run)]["all_kernels_ms"] = sum(v[1] for v in durs.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["mc", "kernel"])
    ap.add_argument("--out")
    ap.add_argument("--dir")
    ap.add_argument("--order", type=int, default=10)
    ap.add_argument("--score", type=int, default=0)
    a = ap.parse_args()
    if a.what == ["run"]:
        return cmd_run(a.order, a.score)
    if not a.out:
        ap.error("--out is required")
    out = {"build_id": q.build_id(), "rules": [name for name, _ in RULES],
           "method": "wall clock around monte_carlo; HIP events around osd_dev; %d repetitions after a warm-up, "
                     "the rules alternating" % REPS}
    for name, fn in (("mc", cmd_mc), ("kernel", cmd_kernel)):
        if name in a.what:
            out[name] = fn()
    if "trace" in a.what:
        out["trace"] = cmd_trace(a.dir)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

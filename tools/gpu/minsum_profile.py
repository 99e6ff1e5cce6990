"""Measurements of scaled min-sum BP -> profiles/minsum.json.

  buys     what QEC_OPT_BP_METHOD = 1 buys: qec_monte_carlo on hgp_ham, QC_LDPC_CSS(3,3,6,13,3,2) and P61 (sparse
           engine), degenerate logical check, p in {0.01, 0.02, 0.05}, syndrome stop, caps 20 / 25 / 50, 2^20
           samples (P61: 2^16), the same samples under method 0 and under method 1 at scales 160 and 256, BP alone
           and with OSD-CS lambda = 10: corrected / logical / syndrome-failed X / Z, the iteration sums and samples
           per second.
  cost     what an iteration costs: decode_batch_packed_dev at 2^16 syndromes, method 1 (scale 160) against method 0
           alternating in one process (HIP events, REPS repetitions after a warm-up): the fixed stop with N = 20 for
           the cost of an iteration, the syndrome stop at the cap for the net effect.
  option0  method 0 alone, with nothing the parent commit lacks, so the same step runs from another tree's package
           (--package-root): run it from both trees in turn, several times, and compare the medians with the
           run-to-run spread of each tree.

Without --step the tool runs every step in a child process of its own, each under its own time limit, and stops at
the first one that fails; the children's results are merged into --out.

Usage: python tools/gpu/minsum_profile.py --out profiles/minsum.json [--parent-root DIR]
       python tools/gpu/minsum_profile.py --step buys:hgp_ham --out fragment.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 15
B = 1 << 16
G13 = (3, 3, 6, 13, 3, 2)
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)
PS = (0.01, 0.02, 0.05)
SEED = 0x51EC0DE
# code -> (iteration cap, Monte-Carlo samples)
CODES = {"hgp_ham": (20, 1 << 20), "G13": (25, 1 << 20), "P61": (50, 1 << 16)}
STEP_LIMIT = 420  # seconds per child


def hgp(H1, H2):
    m1, n1 = H1.shape
    m2, n2 = H2.shape
    HX = np.concatenate([np.kron(H1, np.eye(n2, dtype=np.uint8)), np.kron(np.eye(m1, dtype=np.uint8), H2.T)], axis=1)
    HZ = np.concatenate([np.kron(np.eye(n1, dtype=np.uint8), H2), np.kron(H1.T, np.eye(m2, dtype=np.uint8))], axis=1)
    return np.ascontiguousarray(HX, dtype=np.uint8), np.ascontiguousarray(HZ, dtype=np.uint8)


def code_of(q, label):
    from qec_ldpc_amd.codes import P61, code_path
    if label == "hgp_ham":
        return q.Quantum_LDPC_Code.createFromMatrices(*hgp(HAMMING, HAMMING))
    if label == "G13":
        return q.QC_LDPC_CSS(*G13)
    return q.Quantum_LDPC_Code.createFromFile(code_path(P61))


def spread(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "all_ms": ms}


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


# (QEC_OPT_BP_METHOD, QEC_OPT_MINSUM_SCALE)
CONFIGS = ((0, 160), (1, 160), (1, 256))


def step_buys(q, label):
    cap, samples = CODES[label]
    code = code_of(q, label).with_logical("degenerate")
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    what = {"code": label, "describe": code.describe(), "kernel": dec.describe()}
    rows = []
    for p in PS:
        for osd in (0, 1):
            dec.set_option("osd", osd)
            dec.set_option("osd_order", 10 if osd else 0)
            for method, scale in CONFIGS:
                dec.set_option("minsum_scale", scale)
                dec.set_option("bp_method", method)
                dec.monte_carlo(SEED, 0, min(samples, B), p, cap, "syndrome", batch=B)  # warm-up
                r = dec.monte_carlo(SEED, 0, samples, p, cap, "syndrome", batch=B)
                row = dict(what, p=p, cap=cap, samples=samples, osd_order=10 if osd else None, bp_method=method,
                           minsum_scale=scale if method else None,
                           corrected=r["corrected"], logical=r["logical"], synX=r["synX"], synZ=r["synZ"],
                           failed=samples - r["corrected"], iterationsX=r["iterationsX"], iterationsZ=r["iterationsZ"],
                           seconds=r["totalSeconds"], samples_per_s=samples / r["totalSeconds"])
                print("buys", row, flush=True)
                rows.append(row)
    return rows


def decode_setup(q, label, p):
    import torch
    from oracle.philox import depolarizing
    dev = torch.device("cuda", 0)
    code = code_of(q, label)
    dec = q.DecoderGPU(code, 0, engine="sparse", max_batch=B)
    x, z = depolarizing(SEED, 0, B, code.n, p)
    tX = torch.from_numpy(code.syndrome(0, x)).to(dev)
    tZ = torch.from_numpy(code.syndrome(1, z)).to(dev)
    mk = lambda: torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)  # noqa: E731
    return code, dec, tX, tZ, mk


def step_cost(q, label):
    import torch
    cap, _ = CODES[label]
    rows = []
    for p in PS:
        code, dec, tX, tZ, mk = decode_setup(q, label, p)
        for stop, N in (("fixed", 20), ("syndrome", cap)):
            recs = {0: mk(), 1: mk()}
            its = {k: torch.zeros((B, 2), dtype=torch.int32, device=tX.device) for k in recs}

            def run(option):
                dec.set_option("bp_method", option)  # outside the timed region
                return lambda: dec.decode_batch_packed_dev(tX, tZ, p, N, stop, recs[option], iters=its[option])

            for option in recs:
                f = run(option)
                f()
                f()
            torch.cuda.synchronize()
            ms = {k: [] for k in recs}
            for _ in range(REPS):
                for k in recs:  # alternating
                    ms[k].append(timed(run(k)))
            r = {"code": label, "kernel": dec.describe(), "B": B, "p": p, "stop": stop, "N": N,
                 "option0": spread(ms[0]), "option1": spread(ms[1]),
                 "iterations0": int(its[0].sum().item()), "iterations1": int(its[1].sum().item()),
                 "failed0": int((recs[0][:, -1] & 3).ne(0).sum().item()), "failed1": int((recs[1][:, -1] & 3).ne(0).sum().item())}
            r["ratio_of_medians"] = r["option1"]["median_ms"] / r["option0"]["median_ms"]
            print("cost", label, "p", p, stop, "option 0 %.3f ms  option 1 %.3f ms  ratio %.4f  iterations %d / %d  "
                  "syndrome-failed %d / %d" % (r["option0"]["median_ms"], r["option1"]["median_ms"], r["ratio_of_medians"],
                                               r["iterations0"], r["iterations1"], r["failed0"], r["failed1"]), flush=True)
            rows.append(r)
    return rows


def step_option0(q, label):
    cap, _ = CODES[label]
    p = 0.02
    rows = []
    code, dec, tX, tZ, mk = decode_setup(q, label, p)
    rec = mk()
    for stop in ("syndrome", "fixed"):
        run = lambda: dec.decode_batch_packed_dev(tX, tZ, p, cap, stop, rec)  # noqa: E731
        run()
        run()
        ms = [timed(run) for _ in range(REPS)]
        rows.append(dict(spread(ms), code=label, kernel=dec.describe(), B=B, p=p, stop=stop, cap=cap, build_id=q.build_id()))
        print("option0", label, stop, "%.3f ms [%.3f, %.3f]" % (rows[-1]["median_ms"], rows[-1]["min_ms"], rows[-1]["max_ms"]),
              flush=True)
    return rows


STEPS = {"buys": step_buys, "cost": step_cost, "option0": step_option0}


def run_step(step, package_root, out):
    sys.path.insert(0, package_root)
    if package_root != ROOT:
        sys.path.insert(1, ROOT)  # oracle/ (the Philox restatement) comes from this tree
    import qec_ldpc_amd as q
    kind, label = step.split(":")
    with open(out, "w") as f:
        json.dump({"build_id": q.build_id(), "rows": STEPS[kind](q, label)}, f, indent=1)


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
    ap.add_argument("--step", help="one step, in this process: buys|cost|option0:CODE")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose qec_ldpc_amd package (and library) is loaded")
    ap.add_argument("--parent-root", help="the parent commit's built tree, for the option-0 comparison")
    ap.add_argument("--rounds", type=int, default=3, help="back-to-back rounds of the option-0 comparison")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.package_root, a.out)
    tmp = os.path.join(os.path.dirname(os.path.abspath(a.out)), ".minsum_fragments")
    os.makedirs(tmp, exist_ok=True)
    out = {"method": "qec_monte_carlo counters and wall time (one warm-up batch before each run); HIP events around "
                     "decode_batch_packed_dev, %d repetitions after a warm-up; each step in a process of its own" % REPS,
           "buys": [], "cost": [], "option0": []}
    for label in CODES:
        r = child("buys:" + label, ROOT, tmp)
        out["build_id"] = r["build_id"]
        out["buys"] += r["rows"]
    for label in CODES:
        out["cost"] += child("cost:" + label, ROOT, tmp)["rows"]
    if a.parent_root:
        for k in range(a.rounds):  # the two builds back to back, several times
            for tree, root in (("this", ROOT), ("parent", a.parent_root)):
                for label in CODES:
                    for row in child("option0:" + label, root, tmp)["rows"]:
                        out["option0"].append(dict(row, tree=tree, round=k))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()

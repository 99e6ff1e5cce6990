"""Measurements of the sparse-general kernel (bp_sparse.hip, bp_sparse_kernel with GENERAL)
-> profiles/sparse_general.json.

  decode  the general kernel against the regular sparse kernel on the same regular code, the two sides
          alternating in one process: a warm-up of each, then REPS timed decode_batch_dev calls each between
          HIP events; median, minimum, maximum and quartiles per side.  The outputs of the two sides are
          compared first (they must be equal).
            (a) QC(3,3,6,13,3,2), B = 65 536, 20 fixed iterations, p = 0.02
            (a7) P7 (n = 42: 128 against 256 threads), B = 65 536, 20 fixed iterations, p = 0.02
            (b) P61, B = 8192, 50 fixed iterations, p = 0.01
  mc      hgp_ham and surf3 Monte-Carlo, 2^20 samples, syndrome stop 20, p = 0.01 / 0.05, BP alone and with
          osd = 1, osd_order = 10: samples/s and the counters (reported only)

Usage: python tools/gpu/general_profile.py [decode] [mc] --out profiles/sparse_general.json
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
from qec_ldpc_amd.codes import P7, P61, code_path  # noqa: E402

REPS = 25
G13 = (3, 3, 6, 13, 3, 2)
REP3 = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)


def hgp(H1, H2):
    """HX = [H1 (x) I | I (x) H2^T], HZ = [I (x) H2 | H1^T (x) I]."""
    m1, n1 = H1.shape
    m2, n2 = H2.shape
    HX = np.concatenate([np.kron(H1, np.eye(n2, dtype=np.uint8)), np.kron(np.eye(m1, dtype=np.uint8), H2.T)], axis=1)
    HZ = np.concatenate([np.kron(np.eye(n1, dtype=np.uint8), H2), np.kron(H1.T, np.eye(m2, dtype=np.uint8))], axis=1)
    return np.ascontiguousarray(HX, dtype=np.uint8), np.ascontiguousarray(HZ, dtype=np.uint8)


def spread(ms):
    s = sorted(ms)
    qs = statistics.quantiles(s, n=4)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "q1_ms": qs[0], "q3_ms": qs[2],
            "all_ms": ms}


def decode_case(label, code, B, N, p):
    import torch
    dev = torch.device("cuda", 0)
    gen = q.Quantum_LDPC_Code.createFromMatrices(code.pcm(0), code.pcm(1))
    sides = {"regular": q.DecoderGPU(code, 0, engine="sparse", max_batch=B), "general": q.DecoderGPU(gen, 0, max_batch=B)}
    x, z = depolarizing(0x51EC0DE, 0, B, code.n, p)
    tX = torch.from_numpy(code.syndrome(0, x)).to(dev)
    tZ = torch.from_numpy(code.syndrome(1, z)).to(dev)
    out = {k: (torch.empty((B, code.n), dtype=torch.uint8, device=dev), torch.empty((B, code.n), dtype=torch.uint8, device=dev),
               torch.empty(B, dtype=torch.uint8, device=dev)) for k in sides}

    def run(k):
        sides[k].decode_batch_dev(tX, tZ, p, N, "fixed", *out[k])

    for k in sides:  # warm-up: code objects, workspace
        run(k)
        run(k)
    torch.cuda.synchronize()
    if not all(torch.equal(a, b) for a, b in zip(out["regular"], out["general"])):
        raise SystemExit("%s: the two kernels disagree" % label)
    ms = {k: [] for k in sides}
    for _ in range(REPS):
        for k in sides:  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    r = {"case": label, "code": code.describe(), "B": B, "iterations": N, "stop": "fixed", "p": p, "reps": REPS,
         "regular": dict(spread(ms["regular"]), kernel=sides["regular"].describe()),
         "general": dict(spread(ms["general"]), kernel=sides["general"].describe())}
    r["ratio_of_medians"] = r["general"]["median_ms"] / r["regular"]["median_ms"]
    print(label, "regular %.3f ms [%.3f, %.3f]  general %.3f ms [%.3f, %.3f]  ratio %.3f" % (
        r["regular"]["median_ms"], r["regular"]["min_ms"], r["regular"]["max_ms"], r["general"]["median_ms"],
        r["general"]["min_ms"], r["general"]["max_ms"], r["ratio_of_medians"]), flush=True)
    return r


def cmd_decode():
    g13 = q.QC_LDPC_CSS(*G13)
    return [decode_case("a", g13, 65536, 20, 0.02),
            decode_case("a7", q.Quantum_LDPC_Code.createFromFile(code_path(P7)), 65536, 20, 0.02),
            decode_case("b", q.Quantum_LDPC_Code.createFromFile(code_path(P61)), 8192, 50, 0.01)]


def cmd_mc():
    rows = []
    count = 1 << 20
    for name, H in (("hgp_ham", hgp(HAMMING, HAMMING)), ("surf3", hgp(REP3, REP3))):
        code = q.Quantum_LDPC_Code.createFromMatrices(*H).with_logical("degenerate")
        dec = q.DecoderGPU(code, 0)
        for p in (0.01, 0.05):
            for osd in (0, 1):
                dec.set_option("osd", osd)
                dec.set_option("osd_order", 10 if osd else 0)
                dec.monte_carlo(0x51EC0DE, 0, count, p, 20, "syndrome")  # warm-up: workspace
                runs = [dec.monte_carlo(0x51EC0DE, 0, count, p, 20, "syndrome") for _ in range(3)]
                r = min(runs, key=lambda t: t["totalSeconds"])
                row = {"code": name, "describe": code.describe(), "kernel": dec.describe(), "p": p, "osd": osd,
                       "osd_order": 10 if osd else 0, "samples": count, "samples_per_s": count / r["totalSeconds"],
                       "all_seconds": [t["totalSeconds"] for t in runs], "corrected": r["corrected"],
                       "logical": r["logical"], "syndrome_failed": count - r["corrected"] - r["logical"],
                       "synX": r["synX"], "synZ": r["synZ"]}
                print(json.dumps({k: v for k, v in row.items() if k not in ("all_seconds", "kernel")}), flush=True)
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["decode", "mc"])
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out = {"build_id": q.build_id(), "method": "HIP events around decode_batch_dev, sides alternating in one process, "
                                               "%d repetitions after a warm-up" % REPS}
    if "decode" in a.what:
        out["decode"] = cmd_decode()
    if "mc" in a.what:
        out["monte_carlo"] = cmd_mc()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Measurements of the BP + OSD-0 stage (QEC_OPT_OSD) -> profiles/osd_p61.json.

  run    one qec_monte_carlo call with the option on (P61, 2^20 samples, syndrome stop, cap 50) at --p:
         the workload tools/gpu/run_osd_profile.sh puts under rocprofv3 --kernel-trace --stats
  rates  the Monte-Carlo rate with the option off and on at p = 0.05 and 0.1 in one session, and with
         each form of the kernel's row update (QEC_OPT_OSD_SWEEP)
  table  what the feature buys: corrected / logical / syndrome-fail counts with the option off and on
         for P61 and the generated n = 78 code (degenerate check) at p = 0.02, 0.05, 0.1, 2^16 samples,
         and QEC_OPT_OSD_ITERATIONS 1, 3, 5, 10 at p = 0.05
  reduce the kernel traces of `run` and the two JSON files above into one profile, stamped with the
         library's build id

Usage: python tools/gpu/osd_profile.py run --p 0.05 | rates --out F | table --out F |
       reduce --dir D --out profiles/osd_p61.json
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import qec_ldpc_amd as q  # noqa: E402
from qec_ldpc_amd.codes import P61, code_path  # noqa: E402

SEED, COUNT, CAP = 0x51EC0DE, 1 << 20, 50
G13 = (3, 3, 6, 13, 3, 2)
OSD_KERNELS = ("osd0_kernel", "osd_collect_kernel", "osd_gather_kernel", "osd_scatter_kernel")


def p61(degenerate=False):
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P61))
    return code.with_logical("degenerate") if degenerate else code


def mc(dec, p, count=COUNT, batch=COUNT, cap=CAP):
    return dec.monte_carlo(SEED, 0, count, p, cap, "syndrome", batch=batch)


def cmd_run(a):
    dec = q.DecoderGPU(p61(), 0)
    dec.set_option("osd", 1)
    r = mc(dec, a.p)
    r["osd_sectors"] = dec.get_option("osd_sectors")
    print(json.dumps({"p": a.p, **r}))


def best_rate(dec, p, reps=3):
    mc(dec, p)  # warm-up: workspace allocation
    runs = [mc(dec, p) for _ in range(reps)]
    r = min(runs, key=lambda x: x["totalSeconds"])
    return {"samples_per_s": COUNT / r["totalSeconds"], "seconds": r["totalSeconds"],
            "all_seconds": [x["totalSeconds"] for x in runs], "synX": r["synX"], "synZ": r["synZ"],
            "corrected": r["corrected"], "logical": r["logical"]}


def cmd_rates(a):
    dec = q.DecoderGPU(p61(), 0)
    out = {"samples": COUNT, "cap": CAP, "stop": "syndrome", "points": []}
    for p in (0.05, 0.1):
        pt = {"p": p, "off": best_rate(dec, p)}
        dec.set_option("osd", 1)
        for sweep, name in ((0, "on"), (1, "on_sweep_words"), (2, "on_sweep_rows")):
            dec.set_option("osd_sweep", sweep)
            pt[name] = best_rate(dec, p)
            pt[name]["osd_sectors"] = dec.get_option("osd_sectors")
        dec.set_option("osd_sweep", 0)
        dec.set_option("osd", 0)
        pt["ratio_on_over_off"] = pt["on"]["samples_per_s"] / pt["off"]["samples_per_s"]
        out["points"].append(pt)
        print(json.dumps(pt), flush=True)
    json.dump(out, open(a.out, "w"), indent=1)


def cmd_table(a):
    count = 1 << 16
    codes = {"P61": p61(True), "n78": q.QC_LDPC_CSS(*G13).with_logical("degenerate")}
    caps = {"P61": 50, "n78": 25}
    keep = ("corrected", "logical", "synX", "synZ")
    out = {"samples": count, "stop": "syndrome", "caps": caps, "rows": [], "iterations": []}
    for key, code in codes.items():
        dec = q.DecoderGPU(code, 0)
        for p in (0.02, 0.05, 0.1):
            row = {"code": key, "p": p}
            for name, on in (("off", 0), ("on", 1)):
                dec.set_option("osd", on)
                r = mc(dec, p, count, count, caps[key])
                row[name] = {k: r[k] for k in keep}
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        dec.set_option("osd", 1)
        for it in (1, 3, 5, 10):
            dec.set_option("osd_iterations", it)
            r = mc(dec, 0.05, count, count, caps[key])
            row = {"code": key, "p": 0.05, "osd_iterations": it, **{k: r[k] for k in keep}}
            out["iterations"].append(row)
            print(json.dumps(row), flush=True)
    json.dump(out, open(a.out, "w"), indent=1)


def short(name):
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*", "", re.sub(r"<.*", "", name)).split("::")[-1].strip()


def cmd_reduce(a):
    out = {"build_id": q.build_id(), "workload": "qec_monte_carlo, P61, 2^20 samples in one batch, syndrome stop, cap 50, "
           "QEC_OPT_OSD = 1, QEC_OPT_OSD_ITERATIONS = 3", "source": "tools/gpu/run_osd_profile.sh", "trace": []}
    for d in sorted(glob.glob(os.path.join(a.dir, "trace_p*"))):
        run = json.loads(open(os.path.join(d, "run.out")).read().strip().splitlines()[-1])
        durs, launches = {}, []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                k, t0, t1 = short(row["Kernel_Name"]), int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                durs.setdefault(k, []).append(t1 - t0)
                launches.append((t0, k, t1 - t0))
        total = sum(sum(v) for v in durs.values())
        osd0 = sum(durs.get("osd0_kernel", []))
        helpers = sum(sum(durs.get(k, [])) for k in OSD_KERNELS[1:])
        # the soft re-decode: what runs between the failure list and the statistics that is not an OSD kernel
        t_list = min([t for t, k, _ in launches if k == "osd_collect_kernel"], default=None)
        soft = sum(dt for t, k, dt in launches
                   if t_list is not None and t > t_list and k not in OSD_KERNELS and "statistics" not in k)
        kernels = {k: {"launches": len(v), "total_us": sum(v) / 1e3} for k, v in sorted(durs.items())}
        out["trace"].append({"p": run["p"], "osd_sectors": run["osd_sectors"], "counters": run,
                             "gpu_busy_us": total / 1e3, "osd0_total_us": osd0 / 1e3,
                             "osd0_us_per_sector": osd0 / 1e3 / max(run["osd_sectors"], 1),
                             "soft_decode_us": soft / 1e3, "collect_gather_scatter_us": helpers / 1e3,
                             "share_of_gpu_busy": {"osd0": osd0 / max(total, 1), "soft_decode": soft / max(total, 1),
                                                   "collect_gather_scatter": helpers / max(total, 1)},
                             "kernels": kernels})
    for name in ("rates", "table"):
        f = os.path.join(a.dir, name + ".json")
        if os.path.exists(f):
            out[name] = json.load(open(f))
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "rates", "table", "reduce"])
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--dir")
    ap.add_argument("--out")
    a = ap.parse_args()
    {"run": cmd_run, "rates": cmd_rates, "table": cmd_table, "reduce": cmd_reduce}[a.mode](a)


if __name__ == "__main__":
    main()

"""Measurements of the BP + OSD stage (QEC_OPT_OSD, QEC_OPT_OSD_ORDER; DESIGN.md sections 7.6, 7.7)
-> profiles/osd_p61.json (order 0) and profiles/osd_cs_p61.json (the combination sweep).

  run    one qec_monte_carlo call with the option on (P61, 2^20 samples, syndrome stop, cap 50) at --p:
         the workload tools/gpu/run_osd_profile.sh puts under rocprofv3 --kernel-trace --stats
  rates  the Monte-Carlo rate with the option off and on at p = 0.05 and 0.1 in one session, and with
         each form of the kernel's row update (QEC_OPT_OSD_SWEEP)
  table  what the feature buys: corrected / logical / syndrome-fail counts with the option off and on
         for P61 and the generated n = 78 code (degenerate check) at p = 0.02, 0.05, 0.1, 2^16 samples,
         and QEC_OPT_OSD_ITERATIONS 1, 3, 5, 10 at p = 0.05
  cs_rates  the Monte-Carlo rate at p = 0.05 and 0.1 with QEC_OPT_OSD_ORDER 0 / 10 / 60 alternating in
         one process (best of 3 after a warm-up)
  cs_table  what the sweep buys: BP, OSD-0 and OSD-CS (order 10; order 60 at p = 0.05) side by side on
         the rows of `table`, with QEC_OPT_OSD_CS_SECTORS
  rate0  the order-0 Monte-Carlo rate at --p, every repeat listed; --lib loads another build of the
         library (a parent commit's, to compare the two alternating in one session)
  reduce the kernel traces of `run` and the JSON files above into one profile, stamped with the
         library's build id

--order L (run, rates, table) sets QEC_OPT_OSD_ORDER and is written into the JSON.

Usage: python tools/gpu/osd_profile.py run --p 0.05 [--order L] | rates --out F | table --out F |
       cs_rates --out F | cs_table --out F | rate0 --p 0.05 [--lib SO] --out F |
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
OSD_KERNELS = ("osd0_kernel", "osd_cs_kernel", "osd_collect_kernel", "osd_gather_kernel", "osd_scatter_kernel")


def p61(degenerate=False):
    code = q.Quantum_LDPC_Code.createFromFile(code_path(P61))
    return code.with_logical("degenerate") if degenerate else code


def mc(dec, p, count=COUNT, batch=COUNT, cap=CAP):
    return dec.monte_carlo(SEED, 0, count, p, cap, "syndrome", batch=batch)


def cmd_run(a):
    dec = q.DecoderGPU(p61(), 0)
    dec.set_option("osd", 1)
    dec.set_option("osd_order", a.order)
    r = mc(dec, a.p)
    r["osd_sectors"] = dec.get_option("osd_sectors")
    r["osd_cs_sectors"] = dec.get_option("osd_cs_sectors")
    print(json.dumps({"p": a.p, "osd_order": a.order, **r}))


def best_rate(dec, p, reps=3):
    mc(dec, p)  # warm-up: workspace allocation
    runs = [mc(dec, p) for _ in range(reps)]
    r = min(runs, key=lambda x: x["totalSeconds"])
    return {"samples_per_s": COUNT / r["totalSeconds"], "seconds": r["totalSeconds"],
            "all_seconds": [x["totalSeconds"] for x in runs], "synX": r["synX"], "synZ": r["synZ"],
            "corrected": r["corrected"], "logical": r["logical"]}


def cmd_rates(a):
    dec = q.DecoderGPU(p61(), 0)
    dec.set_option("osd_order", a.order)
    out = {"samples": COUNT, "cap": CAP, "stop": "syndrome", "osd_order": a.order, "points": []}
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
    out = {"samples": count, "stop": "syndrome", "caps": caps, "osd_order": a.order, "rows": [], "iterations": []}
    for key, code in codes.items():
        dec = q.DecoderGPU(code, 0)
        dec.set_option("osd_order", a.order)
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


def cmd_cs_rates(a):
    dec = q.DecoderGPU(p61(), 0)
    dec.set_option("osd", 1)
    orders = (0, 10, 60)
    out = {"samples": COUNT, "cap": CAP, "stop": "syndrome", "orders": orders, "reps": 3, "points": []}
    for p in (0.05, 0.1):
        runs = {lam: [] for lam in orders}
        cs = {}
        mc(dec, p)  # warm-up: workspace allocation
        for _ in range(3):
            for lam in orders:
                dec.set_option("osd_order", lam)
                r = mc(dec, p)
                runs[lam].append(r["totalSeconds"])
                cs[lam] = {"osd_sectors": dec.get_option("osd_sectors"), "osd_cs_sectors": dec.get_option("osd_cs_sectors"),
                           "corrected": r["corrected"], "logical": r["logical"]}
        pt = {"p": p}
        for lam in orders:
            pt["order_%d" % lam] = {"samples_per_s": COUNT / min(runs[lam]), "all_seconds": runs[lam], **cs[lam]}
        for lam in orders[1:]:
            pt["ratio_order_%d_over_0" % lam] = min(runs[0]) / min(runs[lam])
        out["points"].append(pt)
        print(json.dumps(pt), flush=True)
    json.dump(out, open(a.out, "w"), indent=1)


def cmd_cs_table(a):
    count = 1 << 16
    codes = {"P61": p61(True), "n78": q.QC_LDPC_CSS(*G13).with_logical("degenerate")}
    caps = {"P61": 50, "n78": 25}
    keep = ("corrected", "logical", "synX", "synZ")
    out = {"samples": count, "stop": "syndrome", "caps": caps, "osd_iterations": 3, "rows": []}
    for key, code in codes.items():
        dec = q.DecoderGPU(code, 0)
        for p in (0.02, 0.05, 0.1):
            row = {"code": key, "p": p}
            for name, on, lam in (("bp", 0, 0), ("osd0", 1, 0), ("osd_cs_10", 1, 10)) + ((("osd_cs_60", 1, 60),) if p == 0.05 else ()):
                dec.set_option("osd", on)
                dec.set_option("osd_order", lam)
                r = mc(dec, p, count, count, caps[key])
                row[name] = {k: r[k] for k in keep}
                row[name]["osd_sectors"] = dec.get_option("osd_sectors")
                row[name]["osd_cs_sectors"] = dec.get_option("osd_cs_sectors")
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    json.dump(out, open(a.out, "w"), indent=1)


def cmd_rate0(a):
    dec = q.DecoderGPU(p61(), 0)
    dec.set_option("osd", 1)
    mc(dec, a.p)  # warm-up
    secs = [mc(dec, a.p)["totalSeconds"] for _ in range(3)]
    out = {"build_id": q.build_id(), "library": "the build given with --lib" if a.lib else "this tree's build", "p": a.p, "samples": COUNT, "all_seconds": secs,
           "samples_per_s": COUNT / min(secs), "spread": (max(secs) - min(secs)) / min(secs)}
    print(json.dumps(out), flush=True)
    json.dump(out, open(a.out, "w"), indent=1)


def short(name):
    # the elimination kernel is one template: order 0 and the sweep keep names of their own here
    name = name.replace("osd_kernel<false>", "osd0_kernel").replace("osd_kernel<true>", "osd_cs_kernel")
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*", "", re.sub(r"<.*", "", name)).split("::")[-1].strip()


def cmd_reduce(a):
    out = {"build_id": q.build_id(), "workload": "qec_monte_carlo, P61, 2^20 samples in one batch, syndrome stop, cap 50, "
           "QEC_OPT_OSD = 1, QEC_OPT_OSD_ITERATIONS = 3", "source": "tools/gpu/run_osd_profile.sh", "trace": []}
    for d in sorted(glob.glob(os.path.join(a.dir, "trace_*p*"))):
        run = json.loads(open(os.path.join(d, "run.out")).read().strip().splitlines()[-1])
        durs, launches = {}, []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                k, t0, t1 = short(row["Kernel_Name"]), int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                durs.setdefault(k, []).append(t1 - t0)
                launches.append((t0, k, t1 - t0))
        total = sum(sum(v) for v in durs.values())
        osd0 = sum(durs.get("osd0_kernel", [])) + sum(durs.get("osd_cs_kernel", []))  # one of the two runs
        helpers = sum(sum(durs.get(k, [])) for k in OSD_KERNELS[2:])
        # the soft re-decode: what runs between the failure list and the statistics that is not an OSD kernel
        t_list = min([t for t, k, _ in launches if k == "osd_collect_kernel"], default=None)
        soft = sum(dt for t, k, dt in launches
                   if t_list is not None and t > t_list and k not in OSD_KERNELS and "statistics" not in k)
        kernels = {k: {"launches": len(v), "total_us": sum(v) / 1e3} for k, v in sorted(durs.items())}
        out["trace"].append({"p": run["p"], "osd_order": run.get("osd_order", 0), "osd_sectors": run["osd_sectors"],
                             "osd_cs_sectors": run.get("osd_cs_sectors", 0), "counters": run,
                             "gpu_busy_us": total / 1e3, "osd0_total_us": osd0 / 1e3,
                             "osd0_us_per_sector": osd0 / 1e3 / max(run["osd_sectors"], 1),
                             "soft_decode_us": soft / 1e3, "collect_gather_scatter_us": helpers / 1e3,
                             "share_of_gpu_busy": {"osd0": osd0 / max(total, 1), "soft_decode": soft / max(total, 1),
                                                   "collect_gather_scatter": helpers / max(total, 1)},
                             "kernels": kernels})
    for name in ("rates", "table", "cs_rates", "cs_table"):
        f = os.path.join(a.dir, name + ".json")
        if os.path.exists(f):
            out[name] = json.load(open(f))
    rate0 = [json.load(open(f)) for f in sorted(glob.glob(os.path.join(a.dir, "rate0*.json")))]  # in run order
    if rate0:
        out["rate0"] = rate0
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "rates", "table", "cs_rates", "cs_table", "rate0", "reduce"])
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--order", type=int, default=0, help="QEC_OPT_OSD_ORDER (0 .. 64)")
    ap.add_argument("--lib", help="rate0: path of another build of libqecldpc.so")
    ap.add_argument("--dir")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.lib:
        q.LIB_PATH = os.path.abspath(a.lib)  # before the first call loads the library
    {"run": cmd_run, "rates": cmd_rates, "table": cmd_table, "cs_rates": cmd_cs_rates, "cs_table": cmd_cs_table,
     "rate0": cmd_rate0, "reduce": cmd_reduce}[a.mode](a)


if __name__ == "__main__":
    main()

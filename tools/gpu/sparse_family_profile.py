"""Times the sparse engine's min-sum family kernels of one built tree (--package-root): MINSUM, RELAY, LAYERED and the two
SOFT bodies, on hgp_ham (the smallest LDS code of tools/gpu/minsum_profile.py) and P61, 2^16 syndromes at p = 0.02, the
fixed stop with N = 20 and the syndrome stop at the code's cap; set-up and timing are minsum_profile's (HIP events, REPS
repetitions after two warm-up launches).  --rounds R --parent-root DIR: alternating child processes, new tree first."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minsum_profile import B, CODES, REPS, decode_setup, spread, timed  # noqa: E402

P = 0.02
FAMILIES = ("minsum", "relay", "layered", "soft_minsum", "soft_layered")


def configure(q, dec, code, family):
    dec.set_option("bp_method", 1)
    dec.set_option("minsum_scale", 160)
    dec.set_relay(None, None)
    dec.set_syndrome_priors(None, None)
    dec.set_option("minsum_schedule", 1 if family in ("layered", "soft_layered") else 0)
    if family == "relay":
        dec.set_relay(q.relay_gammas(code.n, 5, seed=1), q.relay_gammas(code.n, 5, seed=2), 1)
    if family.startswith("soft"):
        dec.set_syndrome_priors(0.01, 0.01)


def run_tree(package_root, out):
    sys.path.insert(0, package_root)
    if package_root != ROOT:
        sys.path.insert(1, ROOT)
    import qec_ldpc_amd as q
    assert os.path.dirname(os.path.dirname(os.path.abspath(q.__file__))) == os.path.abspath(package_root)
    rows = []
    for label in ("hgp_ham", "P61"):
        cap, _ = CODES[label]
        code, dec, tX, tZ, mk = decode_setup(q, label, P)
        rec = mk()
        for family in FAMILIES:
            configure(q, dec, code, family)
            for stop, N in (("fixed", 20), ("syndrome", cap)):
                run = lambda: dec.decode_batch_packed_dev(tX, tZ, P, N, stop, rec)  # noqa: E731
                run()
                run()
                path = " ".join(sorted(dec.last_path()))
                ms = [timed(run) for _ in range(REPS)]
                rows.append(dict(spread(ms), code=label, family=family, stop=stop, N=N, B=B, p=P, path=path,
                                 kernel=dec.describe(), build_id=q.build_id()))
                print("%s %s %s: %.3f ms [%.3f, %.3f] %s" % (label, family, stop, rows[-1]["median_ms"], rows[-1]["min_ms"],
                                                             rows[-1]["max_ms"], path), flush=True)
    with open(out, "w") as f:
        json.dump({"build_id": q.build_id(), "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--package-root")
    ap.add_argument("--parent-root")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.package_root:
        return run_tree(a.package_root, a.out)
    if not a.parent_root:
        ap.error("--parent-root (the parent commit's built tree) or --package-root (one tree, one run) is needed")
    merged = []
    for k in range(a.rounds):
        for tree, root in (("new", ROOT), ("parent", a.parent_root)):
            frag = a.out + ".%s%d" % (tree, k)
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", root, "--out", frag]
            subprocess.run(cmd, check=True, timeout=240)  # the first failure ends the job
            with open(frag) as f:
                d = json.load(f)
            os.remove(frag)
            merged += [dict({x: r[x] for x in r if x != "all_ms"}, tree=tree, round=k) for r in d["rows"]]
    with open(a.out, "w") as f:  # one row per line
        f.write('{"method": %s,\n "rows": [\n%s\n ]}\n' % (json.dumps(" ".join(__doc__.split())),
                                                         ",\n".join("  " + json.dumps(r) for r in merged)))


if __name__ == "__main__":
    main()

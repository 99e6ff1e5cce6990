"""Kernel-by-kernel comparison of two device-only assembly listings of one source file, e.g. bp_sparse.hip of the
parent commit and of this tree:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize \
        --cuda-device-only -S -o new.s qec_ldpc_amd/csrc/bp_sparse.hip      (and the same in a checkout of the parent)
  python tools/kbench/isa_diff.py parent.s new.s [pairs.txt]
For every kernel symbol of either listing: whether its instruction stream (the body between its label and its
.Lfunc_end, comments and local label numbers aside) is the same in both; for a pair that differs, whether the opcode
sequence (the first token of each instruction line) is the same, and the VGPR count, LDS bytes and scratch bytes of both
sides; and those figures for kernels that only the second listing has.  pairs.txt, lines of `old-symbol new-symbol`,
pairs kernels that were renamed between the listings.  Exit status 1 if a kernel of both listings differs."""
import re
import sys


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S+):\s*; @\1$", s, re.M):
        name = m.group(1)
        if ".amdhsa_kernel " + name not in s:
            continue
        body = s[m.end():s.index(".Lfunc_end", m.end())]
        lines = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if ln:
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        meta = s[s.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        get = lambda key: int(re.search(key + r" (\d+)", meta).group(1))  # noqa: E731
        out[name] = (lines, get(r"\.amdhsa_next_free_vgpr"), get(r"\.amdhsa_group_segment_fixed_size"),
                     get(r"\.amdhsa_private_segment_fixed_size"))
    return out


def opcodes(lines):
    return [ln.split()[0] for ln in lines if not ln.endswith(":")]


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    if len(sys.argv) > 3:  # renamed kernels: the first listing's kernels under their new names
        new_name = dict(ln.split() for ln in open(sys.argv[3]) if ln.strip())
        a = {new_name.get(k, k): v for k, v in a.items()}
    same = [k for k in a if k in b and a[k][0] == b[k][0]]
    differ = [k for k in a if k in b and a[k][0] != b[k][0]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print("kernels in both listings: %d, identical instruction streams: %d, different: %d, only in the first: %d, "
          "only in the second: %d" % (len(same) + len(differ), len(same), len(differ), len(gone), len(new)))
    for k in differ:
        print("DIFFERENT %s %d -> %d instructions, opcode sequence %s, VGPRs %d -> %d, static LDS %d -> %d B, "
              "scratch %d -> %d B" % (k, len(a[k][0]), len(b[k][0]),
                                      "same" if opcodes(a[k][0]) == opcodes(b[k][0]) else "differs",
                                      a[k][1], b[k][1], a[k][2], b[k][2], a[k][3], b[k][3]))
    for k in gone:
        print("GONE", k)
    for k in new:
        lines, vgpr, lds, scratch = b[k]
        print("NEW %s: %d instructions, %d VGPRs, %d B static LDS, %d B scratch" % (k, len(lines), vgpr, lds, scratch))
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())

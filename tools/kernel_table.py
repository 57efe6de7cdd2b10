"""One sorted row per kernel from `make -C fhe-fed_amd/csrc asm` output, for comparing two builds.

usage: python tools/kernel_table.py [--hist SUBSTRING] build/ntt.s build/encrypt.s ...
Reads the given .s files and every resource-usage*.txt beside them.  A row is the mangled name, the
resource fields (SGPRs, VGPRs, AGPRs, scratch bytes, SGPR / VGPR spills, occupancy, LDS bytes),
the instruction count and a digest of the opcode histogram (mnemonic -> count; comments, operands
and label numbers do not enter it).  `diff` of two tables shows every kernel that was lost, added
or compiled differently; a kernel emitted by two files is reported on stderr and fails the run.
--hist prints the full histogram of the kernels whose name contains SUBSTRING."""
import collections
import glob
import hashlib
import os
import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill",
          "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def resources(dirs):
    res, cur = {}, None
    for path in [p for d in sorted(dirs) for p in glob.glob(os.path.join(d, "resource-usage*.txt"))]:
        for line in open(path):
            m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = m.group(2)
    return res


def histograms(paths):
    """{kernel: (file, Counter of mnemonics)}; kernels are the names with an .amdhsa_kernel record."""
    out, dup = {}, []
    for path in paths:
        s = open(path).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, re.M):
            m = re.search(r"^%s:.*?$(.*?)^\.Lfunc_end\d+:" % re.escape(name), s, re.M | re.S)
            ops = collections.Counter(re.findall(r"^\s+([a-z][a-z0-9_]*)\b", m.group(1), re.M))
            if name in out:
                dup.append((name, out[name][0], path))
            out[name] = (os.path.basename(path), ops)
    return out, dup


def main():
    args = sys.argv[1:]
    hist = None
    if args[:1] == ["--hist"]:
        hist, args = args[1], args[2:]
    res = resources({os.path.dirname(p) or "." for p in args})
    kern, dup = histograms(args)
    for name in sorted(kern):
        ops = kern[name][1]
        if hist is not None:
            if hist in name:
                print(name)
                for op in sorted(ops):
                    print("  %-28s %d" % (op, ops[op]))
            continue
        digest = hashlib.md5(" ".join("%s:%d" % kv for kv in sorted(ops.items())).encode()).hexdigest()[:12]
        r = res.get(name, {})
        print(" ".join([name] + [r.get(f, "?") for f in FIELDS] + [str(sum(ops.values())), digest]))
    for name, a, b in dup:
        print("emitted twice: %s (%s, %s)" % (name, a, b), file=sys.stderr)
    sys.exit(1 if dup else 0)


if __name__ == "__main__":
    main()

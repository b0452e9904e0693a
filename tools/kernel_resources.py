"""Kernel resource tables from hipcc's -Rpass-analysis=kernel-resource-usage remarks, and their diff.

  hipcc --offload-arch=gfx950 <the Makefile's flags> -fno-slp-vectorize --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage -c mrt_kernels.hip -o /dev/null 2> new.log
  python tools/kernel_resources.py new.log            # one table
  python tools/kernel_resources.py parent.log new.log # both, and what changed

Kernels are matched by demangled name.  A kernel that gained a template parameter is matched to the
instantiation that has the parent's arguments as a prefix and false / 0 for the new ones, bool
arguments compared as 0 / 1 (a bool parameter that became an int: true -> 1).
"""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]")
HEAD = ("VGPR", "AGPR", "SGPR", "scratch", "waves", "Sspill", "Vspill", "LDS")


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name is not None and m.group(1) in FIELDS:
            out[name][m.group(1)] = m.group(2)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*$", "", d).replace("mrt::", "")
        d = re.sub(r"\((?:int|bool)\)", "", d)
        short[d] = out[n]
    return short


def key(name):
    m = re.match(r"(\w+)(?:<(.*)>)?$", name)
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
    return m.group(1), tuple({"false": "0", "true": "1"}.get(a, a) for a in args)


def table(t, names):
    w = max(len(n) for n in names)
    lines = ["%-*s " % (w, "kernel") + " ".join("%7s" % h for h in HEAD)]
    for n in names:
        lines.append("%-*s " % (w, n) + " ".join("%7s" % t[n].get(f, "?") for f in FIELDS))
    return "\n".join(lines)


def main():
    if len(sys.argv) == 2:
        t = parse(sys.argv[1])
        print(table(t, sorted(t)))
        return 0
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    newKeys = {key(n): n for n in new}
    pairs, matched = [], set()
    for o in sorted(old):
        base, args = key(o)
        cands = [n for (b, a), n in newKeys.items()
                 if b == base and a[:len(args)] == args and all(x == "0" for x in a[len(args):])]
        if len(cands) != 1:
            print("UNMATCHED parent kernel:", o, cands)
            return 1
        pairs.append((o, cands[0]))
        matched.add(cands[0])
    print("== parent: every kernel ==")
    print(table(old, sorted(old)))
    print("\n== this change: the instantiations the parent has ==")
    print(table(new, [n for _, n in pairs]))
    diff = [(o, n) for o, n in pairs if any(old[o].get(f) != new[n].get(f) for f in FIELDS)]
    print("\n== existing instantiations whose resources differ from the parent's: %d ==" % len(diff))
    for o, n in diff:
        print(" ", o, "->", n, {f: (old[o].get(f), new[n].get(f)) for f in FIELDS if old[o].get(f) != new[n].get(f)})
    added = sorted(n for n in new if n not in matched)
    print("\n== this change: new instantiations ==")
    print(table(new, added))
    spills = [n for n in added if new[n].get("ScratchSize [bytes/lane]") != "0" or new[n].get("VGPRs Spill") != "0"
              or new[n].get("SGPRs Spill") != "0"]
    print("\nnew instantiations with scratch or spills: %d %s" % (len(spills), spills))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())

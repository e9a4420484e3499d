#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code of two trees: has a refactor of device code changed what the compiler emits?

    python tools/isa_diff.py <parent tree> <new tree> vocoder.hip ar_xcd.hip ... [--keep DIR]

Each file (a name under vectorquantizedcpc_amd/csrc) is compiled in both trees with the Makefile's own flags plus --save-temps into a
scratch directory; the device .s is split by kernel symbol and compared as TEXT: instructions with labels, comments and directives
stripped (label numbers are renumbered per kernel, so a kernel that merely moved inside its file still compares equal), and the
.amdhsa_ lines of the kernel descriptor.  Per kernel: `identical`, or the instruction count parent -> new and the .amdhsa_ lines that
differ.  Exit status 1 if any kernel differs.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("vectorquantizedcpc_amd", "csrc")


def flags(tree):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*\??=\s*(.*)$", mk, re.M)}
    return re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["CXXFLAGS"]).split(), var["HIPCC"]


def compile_s(tree, name, out):
    os.makedirs(out, exist_ok=True)
    fl, hipcc = flags(tree)
    src = os.path.abspath(os.path.join(tree, CSRC, name))
    if not os.path.exists(src):                    # a unit that only one of the trees has: no kernels on this side
        return ""
    r = subprocess.run([hipcc, *fl, "--save-temps", "-c", src, "-o", "out.o"], cwd=out, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{src}: compile failed\n{r.stderr}")
    asm = [f for f in os.listdir(out) if f.endswith(".s") and "amdgcn" in f]
    return open(os.path.join(out, asm[0])).read()


def kernels(asm):
    """{symbol: (instructions, amdhsa lines)} of every kernel of a device .s"""
    body, desc, cur, kd = {}, {}, None, None
    for raw in asm.splitlines():
        line = raw.split(";")[0].strip()
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif line.startswith(".amdhsa_kernel"):
            kd = line.split()[1]
            desc[kd] = []
        elif line.startswith(".end_amdhsa_kernel"):
            kd = None
        elif kd and line.startswith(".amdhsa_"):
            desc[kd].append(line)
        elif cur and line and not line.endswith(":") and not line.startswith("."):
            body[cur].append(line)
    out = {}
    for k in desc:
        seen = {}
        renum = lambda m: ".L%d" % seen.setdefault(m.group(0), len(seen))
        out[k] = ([re.sub(r"\.L\w+", renum, i) for i in body.get(k, [])], desc[k])
    return out


def main():
    args = sys.argv[1:]
    keep = args.pop(args.index("--keep") + 1) if "--keep" in args else None
    args = [a for a in args if a != "--keep"]
    if len(args) < 3:
        sys.exit(__doc__)
    parent, new, files = args[0], args[1], args[2:]
    tmp = keep or tempfile.mkdtemp(prefix="isa_diff_")
    jobs = [(side, tree, f) for f in files for side, tree in (("parent", parent), ("new", new))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        asm = dict(zip(jobs, ex.map(lambda j: compile_s(j[1], j[2], os.path.join(tmp, j[0], j[2])), jobs)))
    differ = 0
    for f in files:
        a, b = kernels(asm[("parent", parent, f)]), kernels(asm[("new", new, f)])
        names = dict(zip(list(a) + list(b), subprocess.run(["c++filt", *a, *b], capture_output=True, text=True).stdout.splitlines()))
        print(f"== {f}: {len(a)} kernels in the parent, {len(b)} in the new tree")
        for k in sorted(set(a) | set(b), key=lambda s: names[s]):
            name = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", re.sub(r"^void ", "", names[k]))
            if k not in a or k not in b:
                print(f"  {name}: only in the {'parent' if k in a else 'new tree'}")
            elif a[k] == b[k]:
                print(f"  {name}: identical ({len(a[k][0])} instructions)")
                continue
            else:
                print(f"  {name}: instructions {len(a[k][0])} -> {len(b[k][0])}" + ("" if a[k][0] != b[k][0] else " (same text)"))
                for x, y in zip(a[k][1], b[k][1]):
                    if x != y:
                        print(f"      {x}  ->  {y.split()[-1]}")
            differ += 1
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

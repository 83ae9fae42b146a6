"""Static comparison of the gfx950 kernels of two source trees, no GPU needed: registers, scratch, LDS, instruction count and
lane-spill traffic (v_readlane + v_writelane) of every kernel, before and after a change.

    python tools/kernel_static_table.py OLD_CSRC NEW_CSRC rollout mlp_fused greedy_tail env loss > profiles/NAME.md

Each file is compiled to device assembly with its own tree's flags: the files a tree's csrc/Makefile names in a `FAST_TU :=` line
(trees from before the sequence kernels' FMAs were written out) get -ffp-contract=fast, a tree without that line has one flag set.
OLD_EXTRA_FLAGS in the environment is appended for the first tree only: with the same tree given twice, a what-if build against
the real one (`OLD_EXTRA_FLAGS=-ffp-contract=fast ... NEW_CSRC NEW_CSRC lstm wgrad`: what is left to contract).  The kernels of all
named files are collected per tree -- a file that a tree does not have is skipped -- and matched by kernel name, so a kernel
that moved between files is followed (`... OLD_CSRC NEW_CSRC mlp_fused mlp_rollout mlp_update`).  A template kernel whose
argument list gained a trailing `false` (a new defaulted bool) is matched with its old name; a kernel only one tree has is listed
with its own figures.  The stream column says
"same" when the instruction stream is identical after block labels are renumbered, "same opcodes" when the instruction count
and the multiset of opcodes are equal but the stream is reordered or uses other registers, else "differs".  A record for a
refactor, not a gate.
"""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def fast_tu(csrc):
    """the files of this tree that its Makefile builds with -ffp-contract=fast: none unless it has a FAST_TU line"""
    m = re.search(r"^FAST_TU\s*:?=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split() if m else []


def kernels(csrc, tu, what_if=()):
    """{demangled kernel name: dict(tu, vgpr, sgpr, scratch, lds, insts, lanes, sha, ops)} of csrc/tu.hip"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, tu + ".s")
        extra = (["-ffp-contract=fast"] if tu in fast_tu(csrc) else []) + list(what_if)
        subprocess.run([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(csrc, tu + ".hip"), "-o", out], check=True)
        txt = open(out).read()
    res = {}
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S)}
    for name, block in meta.items():
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s+\.amdhsa_kernel " % re.escape(name), txt, re.S | re.M).group(1)
        ins = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.startswith(".LBB"):
                continue
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        code = [i for i in ins if not i.endswith(":")]
        info = txt[txt.index("\t.size\t%s," % name):][:3000]                  # the "; Kernel info:" comment block behind the function
        stat = lambda key, src: int(re.search(r"%s[:, ]+(\d+)" % key, src).group(1))                 # noqa: E731
        nice = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        nice = re.sub(r"^void |\(.*$", "", nice.replace("(anonymous namespace)::", ""))
        res[nice] = dict(tu=tu + ".hip", ops=collections.Counter(i.split()[0] for i in code), vgpr=stat(r"; NumVgprs", info), sgpr=stat(r"; TotalNumSgprs", info), scratch=stat(r"; ScratchSize", info),
                         lds=stat(r"\.amdhsa_group_segment_fixed_size", block),
                         insts=len(code), lanes=sum(i.startswith(("v_readlane", "v_writelane")) for i in code),
                         sha=hashlib.sha256("\n".join(ins).encode()).hexdigest())
    return res


def tree(csrc, tus, what_if=()):
    """the kernels of every file of `tus` that the tree has, by kernel name"""
    res = {}
    for tu in tus:
        if os.path.exists(os.path.join(csrc, tu + ".hip")):
            res.update(kernels(csrc, tu, what_if))
    return res


def main():
    old, new, tus = sys.argv[1], sys.argv[2], sys.argv[3:]
    print("| file | kernel | VGPR | SGPR | scratch B | static LDS B | instructions | v_readlane + v_writelane | stream |")
    print("|---|---|---|---|---|---|---|---|---|")
    cell = lambda a, b: str(a) if a == b else f"{a} -> {b}"                                         # noqa: E731
    a, b = tree(old, tus, os.environ.get("OLD_EXTRA_FLAGS", "").split()), tree(new, tus)
    # a template that gained a defaulted trailing bool: old `name<args>` is new `name<args, false>`, listed under the new name
    for k in [k for k in a if k not in b and k.endswith(">") and k[:-1] + ", false>" in b]:
        a[k[:-1] + ", false>"] = a.pop(k)
    for k in sorted(set(a) | set(b), key=lambda k: ((a.get(k) or b[k])["tu"], k)):
        if k not in a or k not in b:
            x = a.get(k) or b[k]
            print(f"| {x['tu']} | `{k}` | " + " | ".join(str(x[f]) for f in ("vgpr", "sgpr", "scratch", "lds", "insts", "lanes")) +
                  f" | {'only old' if k in a else 'only new'} |")
            continue
        x, y = a[k], b[k]
        stream = "same" if x["sha"] == y["sha"] else ("same opcodes" if x["ops"] == y["ops"] else "differs")
        print(f"| {cell(x['tu'], y['tu'])} | `{k}` | " + " | ".join(cell(x[f], y[f]) for f in ("vgpr", "sgpr", "scratch", "lds", "insts", "lanes")) +
              f" | {stream} |")


if __name__ == "__main__":
    main()

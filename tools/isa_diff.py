"""Compare the gfx950 instruction streams of selected kernels in two builds of libuavppo.so (no GPU needed).

    python tools/isa_diff.py OLD.so NEW.so [--kernels REGEX] [--show]

Every device code object is extracted from both libraries (llvm-objdump --offloading), disassembled, and cut into kernels
by symbol.  A kernel's stream is its instructions with operands; the address / encoding comment of each line is dropped, and
a symbol in a branch target keeps only its offset.  Kernels are matched by mangled name; a kernel of the OLD library whose
name is absent from the NEW one is also looked up with trailing `Lb0E` template arguments appended (a template that gained
defaulted `bool = false` parameters mangles them).  Prints one line per kernel and exits non-zero when a stream differs
or a kernel is missing.  Default selection: the fused rollout kernels.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
DEFAULT = r"rollout_(lstm|mlp|tail)_kernel"


def kernels(lib):
    """{mangled name: [instruction lines]} over all gfx950 code objects of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        os.symlink(os.path.abspath(lib), local)
        subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f], cwd=tmp, check=True, capture_output=True,
                                 text=True).stdout
            name = None
            for line in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1)
                    out[name] = []
                    continue
                if name is None or not line.startswith("\t"):
                    continue
                ins = line.split("//")[0].strip()
                ins = re.sub(r"<[^>+]+(\+0x[0-9a-f]+)?>", lambda k: k.group(1) or "+0x0", ins)
                if ins:
                    out[name].append(ins)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--kernels", default=DEFAULT)
    ap.add_argument("--show", action="store_true", help="print the first differing lines")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    pat = re.compile(a.kernels)
    bad = 0
    for name in sorted(n for n in old if pat.search(n)):
        cand = None
        for extra in range(0, 3):                                # I...E -> I...Lb0EE for each defaulted bool that was added
            n2 = name if extra == 0 else re.sub(r"(I(?:L[a-z][0-9n]+E)+)E", lambda k: k.group(1) + "Lb0E" * extra + "E", name, count=1)
            if n2 in new:
                cand = n2
                break
        if cand is None:
            print(f"MISSING  {name}")
            bad += 1
            continue
        a_, b_ = old[name], new[cand]
        if a_ == b_:
            print(f"same     {len(a_):6d} instructions  {name}" + ("" if cand == name else f"  (now {cand})"))
            continue
        bad += 1
        print(f"DIFFERS  {len(a_)} -> {len(b_)} instructions  {name}  (now {cand})")
        if a.show:
            for i, (x, y) in enumerate(zip(a_, b_)):
                if x != y:
                    print(f"    first difference at instruction {i}:\n      - {x}\n      + {y}")
                    break
    print(f"{len([n for n in old if pat.search(n)])} kernels compared, {bad} differ or are missing; "
          f"{len([n for n in new if pat.search(n)])} match the pattern in the new library")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

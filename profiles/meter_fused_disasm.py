#!/usr/bin/env python3
"""Compare the device code of the conversion and level units with a parent
commit's, kernel by kernel: the kernels that existed before the level meter
moved into the conversion's pass (planar_kernel, interleaved_kernel,
level_kernel, squelch_kernel, last_kernel) must have the same instructions.

    python profiles/meter_fused_disasm.py [PARENT_REV] > profiles/meter_fused_disasm.txt

Both trees' units are compiled device-only with the library's own compile
command (make kcmd) and disassembled with llvm-objdump -d; per kernel the
instruction text is compared with addresses and encodings dropped, so a kernel
that merely moved compares equal ("labels apart").  Needs no GPU.  Exit status
1 if a kernel of the parent is missing or differs.
"""
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlecarrier_amd", "csrc")
UNITS = ("qpsk_input.hip", "qpsk_level.hip")
OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def kernels(tree: str, unit: str, cmd: list, tmp: str, tag: str) -> dict:
    """{demangled kernel name: [instruction text]} of one unit of a tree"""
    co = os.path.join(tmp, f"{tag}_{unit}.co")
    run(cmd + ["-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "singlecarrier_amd", "csrc"),
               "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", co,
               os.path.join(tree, "singlecarrier_amd", "csrc", unit)])
    out, name = {}, None
    for line in run([OBJDUMP, "-d", "-C", co]).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.startswith("\t"):
            text = line.split("//")[0].strip()
            if text:
                out[name].append(re.sub(r"\s+", " ", text))
    # the padding behind a kernel's last instruction is not part of it: s_nop,
    # s_code_end, and "..." for a run of zeros
    for v in out.values():
        while v and (v[-1] == "..." or v[-1].startswith(("s_nop", "s_code_end"))):
            v.pop()
    # by the kernel's name and template arguments: the argument types moved
    # between namespaces (LevelWords), which changes no instruction
    named = {}
    for k, v in out.items():
        m = re.search(r"(\w+_kernel(<[^>]*>)?)\(", k)
        if m:
            key = m.group(1)
            while key in named:   # (the same name with other argument types: a new overload)
                key += "'"
            named[key] = v
    return named


def main() -> int:
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    cmd = shlex.split(run(["make", "-s", "--no-print-directory", "-C", CSRC, "kcmd"]))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        parent = os.path.join(tmp, "parent")
        os.makedirs(parent)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "include", "singlecarrier_amd/csrc"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", parent], input=tar, check=True)
        print(f"parent: {run(['git', '-C', ROOT, 'rev-parse', '--short', rev]).strip()}")
        print(f"command: {' '.join(cmd)} --cuda-device-only -c")
        for unit in UNITS:
            old, new = kernels(parent, unit, cmd, tmp, "old"), kernels(ROOT, unit, cmd, tmp, "new")
            print(f"\n{unit}: {len(old)} kernels in the parent, {len(new)} now")
            for k in sorted(old):
                if k not in new:
                    verdict = "MISSING"
                elif old[k] == new[k]:
                    verdict = "identical"
                else:
                    verdict = f"DIFFERS ({len(old[k])} -> {len(new[k])} instructions)"
                bad += verdict != "identical"
                print(f"  {verdict:10s} {len(old[k]):5d} instructions  {k}")
            for k in sorted(set(new) - set(old)):
                print(f"  {'new':10s} {len(new[k]):5d} instructions  {k}")
    print(f"\n{'all kernels of the parent are identical' if not bad else str(bad) + ' kernels differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

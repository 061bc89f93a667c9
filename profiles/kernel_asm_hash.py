"""Per-kernel hash of a device assembly listing (make -C singlecarrier_amd/csrc
asm -> build/qpsk_rx.s): for every function, the sha256 (first 16 hex digits) of
its instructions from its label to its .Lfunc_end, so that two trees can be
compared kernel by kernel.  Comment lines are dropped (they carry source line
numbers), nothing else.
  python profiles/kernel_asm_hash.py file.s             one line per kernel
  python profiles/kernel_asm_hash.py before.s after.s   same / CHANGED per kernel
"""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = hashlib.sha256("".join(body).encode()).hexdigest()[:16]
            name = None
            continue
        s = line.strip()
        if s and not s.startswith(";"):
            body.append(s.split(";")[0].rstrip() + "\n")
    return out


def short(name):
    try:
        d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        d = name
    return re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", ""))


if __name__ == "__main__":
    a = kernels(sys.argv[1])
    if len(sys.argv) == 2:
        for k, v in a.items():
            print(v, short(k))
    else:
        b = kernels(sys.argv[2])
        for k in sorted(set(a) | set(b), key=short):
            same = a.get(k) == b.get(k)
            print("same   " if same else "CHANGED", a.get(k, "-" * 16), b.get(k, "-" * 16), short(k))

#!/bin/bash
# Instruction mix of the C3 (4x2) kernel's loops for a variant's -D flags
# (device assembly only, no GPU):  bash profiles/asmcount.sh [-DKNOB=..]
set -eu
cd "$(dirname "$0")/../singlecarrier_amd/csrc"
KNOBS=; [ $# -eq 0 ] || KNOBS=$(printf '%q ' "$@")
make -s asm KUNIT=_asmcount QPSK_VARIANT="$KNOBS"
python3 ../../profiles/loopstat.py build/_asmcount.s "${KERN:-rx_kernelILi4ELi2ELi0ELb0ELi64ELb0ELb0E}" | awk '$4 > 800'
rm -f build/_asmcount.s

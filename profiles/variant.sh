#!/bin/bash
# Build a variant of the receive library from another qpsk_rx.hip source (A/B
# experiments only; the product is singlecarrier_amd/libqpsk_hip.so).
#   bash profiles/variant.sh NAME path/to/qpsk_rx.hip [extra hipcc flags]
# The other objects are the product's (the Makefile's list, `make restobj`); a
# source from before the split of qpsk_rx.hip carries the host side itself and
# is linked without the product's qpsk_rx_host.o.
set -euo pipefail
SCHED=${SCHED-iterative-ilp}   # machine scheduler; SCHED= for the default one
NAME=$1; SRC=$(realpath $2); shift 2
cd "$(dirname "$0")/../singlecarrier_amd/csrc"
OBJ=$(make -s --no-print-directory restobj)
make -s $OBJ
if grep -q 'qpsk_rx_create_mode' "$SRC"; then OBJ=${OBJ/build\/qpsk_rx_host.o/}; fi
cp "$SRC" build/_variant_$NAME.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off \
  -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -fno-fast-math \
  -I../../include -I. ${SCHED:+-mllvm -amdgpu-sched-strategy=$SCHED} "$@" \
  -c -o build/_variant_$NAME.o build/_variant_$NAME.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/lib_$NAME.so build/_variant_$NAME.o \
  $OBJ -lm -lpthread
echo singlecarrier_amd/csrc/build/lib_$NAME.so

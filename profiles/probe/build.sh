#!/bin/bash
# Builds the round-4 probes (run from anywhere; outputs next to this script):
#   simd_probe      which SIMD each wave of a workgroup lands on (HW_ID)
#   fir_probe       fir_dec / fir_head issue rates at 1..4 waves per SIMD, the
#                   product source's FIRs as they are
set -eu
cd "$(dirname "$0")"
H=/opt/rocm/bin/hipcc
F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero \
 -I../../include -I../../singlecarrier_amd/csrc -mllvm -amdgpu-sched-strategy=iterative-ilp"
$H --offload-arch=gfx950 -O2 -o simd_probe simd_probe.hip
$H $F -c -o /tmp/fir_probe.o fir_probe.hip
# fir_probe.hip includes qpsk_rx.hip, the kernels' translation unit, which needs
# no other object of the library
$H --offload-arch=gfx950 -o fir_probe /tmp/fir_probe.o -lm -lpthread

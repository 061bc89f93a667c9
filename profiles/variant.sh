#!/bin/bash
# Build a variant of the receive library from another qpsk_rx.hip source (A/B
# experiments only; the product is singlecarrier_amd/libqpsk_hip.so).
#   bash profiles/variant.sh NAME path/to/qpsk_rx.hip [extra hipcc flags]
# build_variant.sh under its older command line (SCHED as there).
set -euo pipefail
echo singlecarrier_amd/csrc/$(bash "$(dirname "$0")/build_variant.sh" "$@")

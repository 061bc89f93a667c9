#!/bin/bash
# Build an A/B variant of libqpsk_hip.so whose receive kernels come from another
# revision of qpsk_rx.hip (or extra -D knobs), next to the product library.
# The build is the product's Makefile with the variant as its kernel unit:
# every other object is the product's, and the kernel headers the variant
# includes are the working tree's.  A revision from before the split of
# qpsk_rx.hip carries the host side itself: it is linked without the product's
# qpsk_rx_host.o.  The variant carries its own kernel hash ("variant-<name>"),
# never the product's (bench.pmc_record drops its counters).
#   bash profiles/build_variant.sh NAME REV [-DKNOB=..]
#   REV: a git revision, "work" or a file;  SCHED=NAME or SCHED= in the
#   environment: another machine scheduler, or the compiler's default one
# Output: singlecarrier_amd/csrc/build/lib_NAME.so
set -eu
NAME=$1; REV=$2; shift 2
if [ -f "$REV" ]; then REV=$(realpath "$REV"); fi
cd "$(dirname "$0")/../singlecarrier_amd/csrc"
make -s >/dev/null
SRC=build/_variant_$NAME.hip
if [ "$REV" = work ]; then cp qpsk_rx.hip $SRC
elif [ -f "$REV" ]; then cp "$REV" $SRC
else git show "$REV:singlecarrier_amd/csrc/qpsk_rx.hip" > $SRC; fi
REST=$(make -s --no-print-directory restobj)
KNOBS=; [ $# -eq 0 ] || KNOBS=$(printf '%q ' "$@")
if grep -q 'qpsk_rx_create_mode' $SRC; then REST=${REST/build\/qpsk_rx_host.o/}; fi
make -s KUNIT=_variant_$NAME KUNIT_SRC=$SRC HASHSTR=variant-$NAME LIB=build/lib_$NAME.so REST="$REST" \
  QPSK_VARIANT="$KNOBS" ${SCHED+"SCHED=${SCHED:+-mllvm -amdgpu-sched-strategy=$SCHED}"} >/dev/null
echo "build/lib_$NAME.so"

#!/usr/bin/env python3
"""Compare the device code of the transmitter's units with a parent commit's,
kernel by kernel: the kernels of a uniform context (tx_batch_kernel's three
instantiations, tx_state_kernel) and the output conversions must have the same
instructions as before the per-channel packet index (tx_plan_kernel,
tx_seed_kernel, tx_mask_kernel are new).

    python profiles/tx_mask_disasm.py [PARENT_REV] > profiles/tx_mask_disasm.txt

The comparison is meter_fused_disasm.py's (same compile command, llvm-objdump
-d per kernel, addresses and encodings dropped) over other units.  Needs no
GPU.  Exit status 1 if a kernel of the parent is missing or differs.
"""
import sys

import meter_fused_disasm as m

m.UNITS = ("qpsk_tx.hip", "qpsk_output.hip")

if __name__ == "__main__":
    sys.exit(m.main())

# The flags every HIP translation unit of the project is compiled with, written
# once: the library (Makefile) and the test helpers (tests/kernels/Makefile)
# include this file; the ThreadSanitizer and variant builds go through the
# Makefile.  Variables only.
ROCM  ?= /opt/rocm
HIPCC := $(ROCM)/bin/hipcc
ARCH  ?= gfx950
# Bit-exactness contract: no FP contraction anywhere, correctly rounded fp32
# division/sqrt, denormals kept (HIP defaults, restated so they cannot drift).
EXACT   := -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero \
           -fno-fast-math
HIPBASE := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC $(EXACT)
# the library's machine scheduler (one unit of it is built without: Makefile)
SCHED   := -mllvm -amdgpu-sched-strategy=iterative-ilp

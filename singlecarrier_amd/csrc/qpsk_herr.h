// qpsk_herr.h -- a HIP error as a QPSK_* status and the check that returns it,
// defined once for csrc/.  The kernels' unit uses them (qpsk_rx_shared.h), so
// this file is part of the kernel hash; qpsk_hip_host.h has the rest.
#pragma once

#include <hip/hip_runtime.h>

#include "qpsk_batch.h"

static inline int herr(hipError_t e) { return e == hipSuccess ? QPSK_OK : QPSK_EHIP - (int)e; }
#define HCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return herr(e_); } while (0)

"""A bounded delay on a GPU stream, for tests of stream order
(tests/test_gpu_async.py): work enqueued behind it on the same stream is still
pending when the host has finished enqueueing, which is the regime every
device entry point's `stream` argument is about.

The delay is one wave of tests/kernels/spin_delay.hip that waits on the
device's wall clock (the constant-rate counter, 100 MHz on an MI355X) and
gives up after a capped number of iterations, so it cannot run unbounded.
torch.cuda._sleep was tried first and is not used: it counts shader cycles,
and the shader clock moves with the device's power state, so a delay sized
from one calibration is short whenever the clock is faster than it was at the
calibration (2.4 GHz idle against 1.8 GHz under load on one card).  The wall
clock needs no calibration: its rate is a device attribute.

Plain module: torch is imported when a function is called, never at import.

put(stream, ms)   enqueue a delay of `ms` on `stream` (a torch stream), between
                  two events; returns a Delay.  Refuses more than MAX_MS.
Delay.running()   the delay has not ended yet (a query, no wait).
Delay.ms()        how long it lasted by the events (waits for its end).
"""
import ctypes as C
import functools
import os
import subprocess

MAX_MS = 1000.0     # put() refuses a longer delay
# An iteration of the kernel's loop sleeps 2,048 shader cycles and reads the
# clock: 0.9 us at 2.4 GHz, more at any lower clock.  1,500 iterations per
# millisecond asked are therefore never reached before the wall clock ends the
# loop, and end it after a few times the delay if the wall clock stood still.
CAP_PER_MS = 1500

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels")


@functools.lru_cache(maxsize=None)
def _lib():
    path = os.path.join(HERE, "libspin_delay.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", HERE], check=True)
    import torch  # noqa: F401  (one HIP runtime in the process)
    lib = C.CDLL(path)
    lib.spin_delay_clock_khz.restype = C.c_longlong
    lib.spin_delay_clock_khz.argtypes = [C.c_int]
    lib.spin_delay.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong]
    return lib


@functools.lru_cache(maxsize=None)
def clock_khz(device=0):
    """The rate of the device's wall clock, in kHz."""
    khz = int(_lib().spin_delay_clock_khz(device))
    if khz <= 0:
        raise RuntimeError(f"no wall clock rate for device {device}: {khz}")
    return khz


class Delay:
    def __init__(self, e0, e1, asked_ms):
        self._e0, self._e1, self.asked_ms = e0, e1, asked_ms

    def running(self):
        return not self._e1.query()

    def ms(self):
        self._e1.synchronize()
        return self._e0.elapsed_time(self._e1)


def put(stream, ms):
    """A delay of `ms` milliseconds on `stream` (a torch stream)."""
    if not 0 < ms <= MAX_MS:
        raise ValueError(f"a delay of {ms} ms: this helper gives at most {MAX_MS} ms")
    import torch
    ticks = int(round(ms * clock_khz(stream.device.index or 0)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        rc = _lib().spin_delay(C.c_void_p(stream.cuda_stream), ticks, int(ms * CAP_PER_MS) + 1)
        e1.record()
    if rc != 0:
        raise RuntimeError(f"spin_delay: HIP error {rc}")
    return Delay(e0, e1, ms)

"""singlecarrier_amd -- MI355X receive path of the SingleCarrier QPSK modem.

Python mirror of the C-ABI in ``include/qpsk_internal.h`` (the reference's
``headers/qpsk_internal.h:79-84`` surface) and ``include/qpsk_batch.h`` (the
batched, multi-channel receiver), ``include/qpsk_tx.h`` (the batched
transmitter), ``include/qpsk_input.h`` (G.711 and timeslot-interleaved
input), ``include/qpsk_output.h`` (the same formats as output),
``include/qpsk_compact.h`` (the receive output as records of the valid frames)
and ``include/qpsk_level.h`` (the input level meter and the squelch),
over ``singlecarrier_amd/libqpsk_hip.so``.

There is no CPU fallback: if the HIP library is missing or no GPU is present,
the receive functions raise.  (The CPU restatement in ``oracle/`` is test
infrastructure, never called from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# QPSK_LIB overrides the library path (A/B experiments with variant builds only)
LIB_PATH = os.environ.get("QPSK_LIB") or os.path.join(HERE, "libqpsk_hip.so")

FRAME_SIZE = 1880        # headers/qpsk_internal.h:45
DATA_SYMBOLS = 31        # headers/qpsk_internal.h:37
PREAMBLE_LENGTH = 128    # headers/qpsk_internal.h:50
BITS_PER_FRAME = 496     # headers/qpsk_internal.h:48 (record size of the RX driver)
NBITS = 62               # bits written per valid frame (src/qpsk.c:206-215)
CYCLES = 5

_lib = None


class _CF(C.Structure):
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


class QpskError(RuntimeError):
    """A negative QPSK_E* code from the library (``.code``)."""
    code = 0


# error codes (include/qpsk_batch.h, qpsk_stream.h)
QPSK_EINVAL, QPSK_ENOMEM, QPSK_ENODEV, QPSK_EBUSY, QPSK_ESTALL = -1, -2, -3, -4, -5


def build(verbose: bool = False) -> str:
    """Compile libqpsk_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", os.path.join(HERE, "csrc")], capture_output=True,
                         text=True)
    if out.returncode != 0:
        raise QpskError("build failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])
    if verbose:
        print(out.stdout)
    return LIB_PATH


# the receive kernels' sources, in the order the Makefile's KSRC hashes them
# (csrc/Makefile: qpsk_kernel_hash())
KERNEL_SOURCES = ("qpsk_rx.hip", "qpsk_cmul.h", "qpsk_rx_shared.h", "qpsk_herr.h", "qpsk_rx_dev.h", "qpsk_rx_front.h",
                  "qpsk_rx_back.h", "qpsk_rx_quad.h", "qpsk_hunt.h", "qpsk_rcp.h", "qpsk_consts.h",
                  "qpsk_fft_dev.h", "qpsk_split.h")


def kernel_source_hash(csrc: str = None) -> str:
    """The hash the Makefile compiles into the library (KERNEL_SOURCES, the
    C-ABI headers they include, the kernel unit's compile command and the
    compiler's version),
    for the sources in `csrc` (default: this package's csrc/).  The Makefile is
    the one definition: this asks it (make khash)."""
    csrc = csrc or os.path.join(HERE, "csrc")
    inc = os.path.join(os.path.dirname(HERE), "include")
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, "khash", f"INCDIR={inc}"],
                         capture_output=True, text=True)
    if out.returncode != 0:
        raise QpskError("make khash failed:\n" + out.stderr[-2000:])
    return out.stdout.strip()


def kernel_hash() -> str:
    """qpsk_kernel_hash() of the loaded library (no GPU needed)."""
    return lib().qpsk_kernel_hash().decode()


def lib():
    """Load the HIP library (fails loudly when it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QpskError(f"{LIB_PATH} not built: run singlecarrier_amd.build() "
                            "or make -C singlecarrier_amd/csrc")
        try:  # share torch's HIP runtime when torch is in use (same soname)
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
        L.qpsk_rx_create.restype = vp
        L.qpsk_rx_create.argtypes = [i32, i32, C.POINTER(C.c_int)]
        L.qpsk_rx_create_mode.restype = vp
        L.qpsk_rx_create_mode.argtypes = [i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_rx_mode.argtypes = [vp]
        L.qpsk_rx_destroy.argtypes = [vp]
        L.qpsk_rx_reset.argtypes = [vp]
        L.qpsk_rx_channels.argtypes = [vp]
        L.qpsk_rx_frames.restype = u64
        L.qpsk_rx_frames.argtypes = [vp]
        L.qpsk_rx_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.qpsk_rx_batch_device.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
        L.qpsk_strerror.restype = C.c_char_p
        L.qpsk_strerror.argtypes = [i32]
        L.qpsk_kernel_hash.restype = C.c_char_p
        L.qpsk_kernel_hash.argtypes = []
        L.qpsk_rx_frame.argtypes = [vp, vp]
        L.qpsk_tx_frame.argtypes = [vp, vp, i32, C.c_bool]
        L.qpsk_surface_error.restype = i32
        L.qpsk_rx_timing_enable.argtypes = [vp, i32]
        L.qpsk_rx_sync.argtypes = [vp]
        L.qpsk_rx_timing_collect.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.qpsk_rx_timing_split.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                           C.POINTER(C.c_int)]
        L.qpsk_synth_batch.restype = None
        L.qpsk_synth_batch.argtypes = [u64, C.c_uint32, i32, C.c_double, vp, C.c_long, i32]
        L.qpsk_synth_device.argtypes = [u64, C.c_uint32, i32, C.c_double, vp, C.c_long, vp]
        L.qpsk_tx_phase_table.restype = None
        L.qpsk_tx_phase_table.argtypes = [vp, C.c_long]
        L.qpsk_stream_create.restype = vp
        L.qpsk_stream_create.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_stream_create_mode.restype = vp
        L.qpsk_stream_create_mode.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_stream_destroy.argtypes = [vp]
        L.qpsk_stream_acquire.restype = vp
        L.qpsk_stream_acquire.argtypes = [vp, C.POINTER(C.c_int)]
        L.qpsk_stream_submit.argtypes = [vp]
        L.qpsk_stream_pending.argtypes = [vp]
        L.qpsk_stream_retrieve.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.qpsk_stream_ctx.restype = vp
        L.qpsk_stream_ctx.argtypes = [vp]
        L.qpsk_records.restype = C.c_size_t
        L.qpsk_records.argtypes = [vp, vp, i32, vp]
        L.qpsk_fft_alloc.restype = vp
        L.qpsk_fft_alloc.argtypes = [i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_fft_free.argtypes = [vp]
        L.qpsk_fft_device.argtypes = [vp, vp, vp, i32, vp]
        L.qpsk_fft.argtypes = [vp, vp, vp, i32]
        L.qpsk_fft_twiddle_table.restype = None
        L.qpsk_fft_twiddle_table.argtypes = [i32, i32, vp]
        L.qpsk_fft_perm_table.argtypes = [i32, vp]
        L.qpsk_rx_state_size.restype = C.c_size_t
        L.qpsk_rx_state_size.argtypes = [i32]
        L.qpsk_rx_state_save.argtypes = [vp, i32, i32, vp, C.c_size_t]
        L.qpsk_rx_state_load.argtypes = [vp, i32, i32, vp, C.c_size_t]
        L.qpsk_rx_state_join.argtypes = [vp, i32, i32, vp, C.c_size_t]
        L.qpsk_rx_reset_channels.argtypes = [vp, i32, i32]
        L.qpsk_rx_channel_frames.argtypes = [vp, i32, i32, vp]
        L.qpsk_tx_create.restype = vp
        L.qpsk_tx_create.argtypes = [i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_tx_destroy.restype = None
        L.qpsk_tx_destroy.argtypes = [vp]
        L.qpsk_tx_reset.argtypes = [vp]
        L.qpsk_tx_channels.argtypes = [vp]
        L.qpsk_tx_gap.argtypes = [vp]
        L.qpsk_tx_packets.restype = u64
        L.qpsk_tx_packets.argtypes = [vp]
        L.qpsk_tx_batch.argtypes = [vp, vp, i32, vp, C.c_long]
        L.qpsk_tx_batch_device.argtypes = [vp, vp, i32, vp, C.c_long, vp]
        L.qpsk_tx_sync.argtypes = [vp]
        L.qpsk_tx_batch_host.argtypes = [vp, i32, vp, i32, i32, vp, C.c_long, i32]
        L.qpsk_tx_state_init.restype = None
        L.qpsk_tx_state_init.argtypes = [vp]
        L.qpsk_tx_batch_masked.argtypes = [vp, vp, vp, i32, vp, C.c_long]
        L.qpsk_tx_batch_masked_device.argtypes = [vp, vp, vp, i32, vp, C.c_long, vp]
        L.qpsk_tx_batch_masked_host.argtypes = [vp, i32, vp, vp, i32, i32, vp, C.c_long, i32]
        L.qpsk_tx_reset_channels.argtypes = [vp, i32, i32]
        L.qpsk_tx_channel_packets.argtypes = [vp, i32, i32, vp]
        L.qpsk_tx_state_size.restype = C.c_size_t
        L.qpsk_tx_state_size.argtypes = [i32]
        L.qpsk_tx_state_save.argtypes = [vp, i32, i32, vp, C.c_size_t]
        L.qpsk_tx_state_load.argtypes = [vp, i32, i32, vp, C.c_size_t]
        L.qpsk_tx_batch_masked_fmt.argtypes = [vp, vp, vp, i32, vp, i32, C.c_long]
        L.qpsk_tx_batch_masked_device_fmt.argtypes = [vp, vp, vp, i32, vp, i32, C.c_long, vp]
        L.qpsk_input_bytes.restype = C.c_size_t
        L.qpsk_input_bytes.argtypes = [i32, i32, i32, C.c_long]
        L.qpsk_input_convert_host.argtypes = [i32, vp, C.c_long, i32, i32, vp, i32]
        L.qpsk_input_convert_device.argtypes = [i32, vp, C.c_long, i32, i32, vp, vp]
        L.qpsk_input_convert_device_dec.argtypes = [i32, vp, C.c_long, i32, i32, vp, vp, i32]
        L.qpsk_input_load_width.argtypes = [vp, C.c_long, i32]
        L.qpsk_rx_batch_fmt.argtypes = [vp, vp, i32, C.c_long, i32, vp, vp, vp, vp]
        L.qpsk_rx_batch_device_fmt.argtypes = [vp, vp, i32, C.c_long, i32, vp, vp, vp, vp, vp]
        L.qpsk_stream_create_fmt.restype = vp
        L.qpsk_stream_create_fmt.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_stream_acquire_raw.restype = vp
        L.qpsk_stream_acquire_raw.argtypes = [vp, C.POINTER(C.c_int)]
        L.qpsk_output_bytes.restype = C.c_size_t
        L.qpsk_output_bytes.argtypes = [i32, i32, C.c_long, C.c_long]
        L.qpsk_output_convert_host.argtypes = [i32, vp, C.c_long, i32, C.c_long, vp, C.c_long, i32]
        L.qpsk_output_convert_device.argtypes = [i32, vp, C.c_long, i32, C.c_long, vp, C.c_long, vp]
        L.qpsk_output_convert_device_w.argtypes = [i32, vp, C.c_long, i32, C.c_long, vp, C.c_long, vp,
                                                   C.POINTER(C.c_int)]
        L.qpsk_output_store_width.argtypes = [vp, C.c_long, i32]
        L.qpsk_tx_batch_fmt.argtypes = [vp, vp, i32, vp, i32, C.c_long]
        L.qpsk_tx_batch_device_fmt.argtypes = [vp, vp, i32, vp, i32, C.c_long, vp]
        L.qpsk_tx_batch_device_fmt_path.argtypes = [vp, vp, i32, vp, i32, C.c_long, vp, i32]
        sz, u32p = C.c_size_t, C.POINTER(C.c_uint32)
        L.qpsk_bits_pack_host.argtypes = [vp, sz, vp]
        L.qpsk_bits_unpack_host.argtypes = [vp, sz, vp]
        L.qpsk_bits_pack_device.argtypes = [vp, sz, vp, vp]
        L.qpsk_compact_host.argtypes = [vp, vp, vp, vp, i32, i32, i32, sz, vp, vp, vp, vp, vp]
        L.qpsk_compact_work_bytes.restype = sz
        L.qpsk_compact_work_bytes.argtypes = [i32, i32]
        L.qpsk_compact_tiling.restype = None
        L.qpsk_compact_tiling.argtypes = [C.POINTER(C.c_int)] * 3
        L.qpsk_compact_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, sz, vp, vp, vp, vp, vp, vp, sz, vp]
        L.qpsk_rx_batch_records.argtypes = [vp, vp, i32, i32, sz, vp, vp, vp, vp, vp]
        L.qpsk_rx_batch_records_fmt.argtypes = [vp, vp, i32, C.c_long, i32, i32, sz, vp, vp, vp, vp, vp]
        L.qpsk_rx_batch_records_device.argtypes = [vp, vp, i32, i32, sz, vp, vp, vp, vp, vp, vp]
        L.qpsk_stream_create_records.restype = vp
        L.qpsk_stream_create_records.argtypes = [i32, i32, i32, i32, i32, i32, i32, sz, C.POINTER(C.c_int)]
        L.qpsk_stream_retrieve_records.argtypes = [vp, C.POINTER(C.c_void_p), u32p, C.POINTER(C.c_void_p)]
        L.qpsk_level_host.argtypes = [vp, sz, vp]
        L.qpsk_level_device.argtypes = [vp, sz, vp, vp]
        L.qpsk_level_tiling.restype = None
        L.qpsk_level_tiling.argtypes = [C.POINTER(C.c_int)]
        L.qpsk_level_dbfs.restype = C.c_double
        L.qpsk_level_dbfs.argtypes = [vp]
        L.qpsk_level_sumsq_of_dbfs.restype = u64
        L.qpsk_level_sumsq_of_dbfs.argtypes = [C.c_double]
        L.qpsk_squelch_host.argtypes = [vp, vp, i32, i32, u64, vp, vp, vp, vp, vp]
        L.qpsk_squelch_device.argtypes = [vp, vp, i32, i32, u64, vp, vp, vp, vp, vp, vp]
        L.qpsk_rx_batch_records_squelch.argtypes = [vp, vp, i32, u64, vp, i32, sz, vp, vp, vp, vp, vp, vp]
        L.qpsk_rx_batch_records_squelch_device.argtypes = [vp, vp, i32, u64, vp, i32, sz, vp, vp, vp, vp, vp, vp, vp]
        L.qpsk_input_level_work_bytes.restype = sz
        L.qpsk_input_level_work_bytes.argtypes = [i32, i32, i32, C.c_long]
        L.qpsk_input_convert_level_host.argtypes = [i32, vp, C.c_long, i32, i32, vp, vp, i32]
        L.qpsk_input_convert_level_device.argtypes = [i32, vp, C.c_long, i32, i32, vp, vp, vp, sz, vp]
        L.qpsk_input_convert_level_device_grid.argtypes = [i32, vp, C.c_long, i32, i32, vp, vp, vp, sz, vp, i32,
                                                           C.c_uint]
        L.qpsk_rx_batch_records_squelch_fmt.argtypes = [vp, vp, i32, C.c_long, i32, u64, vp, i32, sz, vp, vp, vp, vp,
                                                        vp, vp]
        L.qpsk_rx_batch_records_squelch_device_fmt.argtypes = [vp, vp, i32, C.c_long, i32, u64, vp, i32, sz, vp, vp,
                                                               vp, vp, vp, vp, vp]
        L.qpsk_stream_create_records_squelch.restype = vp
        L.qpsk_stream_create_records_squelch.argtypes = [i32, i32, i32, i32, i32, i32, i32, sz, u64,
                                                         C.POINTER(C.c_int)]
        L.qpsk_stream_retrieve_records_squelch.argtypes = [vp, C.POINTER(C.c_void_p), u32p, C.POINTER(C.c_void_p),
                                                           C.POINTER(C.c_void_p)]
        L.cnormf.restype = C.c_float
        L.cnormf.argtypes = [_CF]   # _Complex float == {float, float} in one SSE reg (SysV)
        _lib = L
    return _lib


SYMBOLS = ["qpsk_rx_create", "qpsk_rx_create_mode", "qpsk_rx_mode", "qpsk_rx_destroy", "qpsk_rx_reset", "qpsk_rx_channels",
           "qpsk_rx_frames", "qpsk_rx_batch", "qpsk_rx_batch_device", "qpsk_rx_sync", "qpsk_strerror",
           "qpsk_kernel_hash",
           "cnormf", "qpsk_mod", "qpsk_demod", "qpsk_rx_frame", "qpsk_tx_frame",
           "qpsk_rx_init", "qpsk_tx_init", "qpsk_surface_error", "qpsk_tx_state_init",
           "qpsk_tx_frame_state", "qpsk_synth_batch", "qpsk_rx_timing_enable",
           "qpsk_rx_timing_collect", "qpsk_rx_timing_split", "qpsk_synth_device",
           "qpsk_tx_phase_table", "qpsk_stream_create", "qpsk_stream_create_mode", "qpsk_stream_destroy",
           "qpsk_stream_acquire", "qpsk_stream_submit", "qpsk_stream_pending",
           "qpsk_stream_retrieve", "qpsk_stream_ctx", "qpsk_records", "qpsk_fft_alloc",
           "qpsk_fft_free", "qpsk_fft_device", "qpsk_fft", "qpsk_rx_state_size",
           "qpsk_rx_state_save", "qpsk_rx_state_load",
           "qpsk_rx_state_join", "qpsk_rx_reset_channels", "qpsk_rx_channel_frames",
           "qpsk_tx_create", "qpsk_tx_destroy", "qpsk_tx_reset", "qpsk_tx_channels", "qpsk_tx_gap",
           "qpsk_tx_packets", "qpsk_tx_batch", "qpsk_tx_batch_device", "qpsk_tx_sync",
           "qpsk_tx_batch_host",
           "qpsk_tx_batch_masked", "qpsk_tx_batch_masked_device", "qpsk_tx_batch_masked_host",
           "qpsk_tx_reset_channels", "qpsk_tx_channel_packets", "qpsk_tx_state_size", "qpsk_tx_state_save",
           "qpsk_tx_state_load", "qpsk_tx_batch_masked_fmt", "qpsk_tx_batch_masked_device_fmt",
           "qpsk_input_bytes", "qpsk_input_convert_host", "qpsk_input_convert_device",
           "qpsk_rx_batch_fmt", "qpsk_rx_batch_device_fmt", "qpsk_stream_create_fmt",
           "qpsk_stream_acquire_raw",
           "qpsk_output_bytes", "qpsk_output_convert_host", "qpsk_output_convert_device",
           "qpsk_tx_batch_fmt", "qpsk_tx_batch_device_fmt",
           "qpsk_bits_pack_host", "qpsk_bits_unpack_host", "qpsk_bits_pack_device", "qpsk_compact_host",
           "qpsk_compact_work_bytes", "qpsk_compact_tiling", "qpsk_compact_device", "qpsk_rx_batch_records",
           "qpsk_rx_batch_records_fmt", "qpsk_rx_batch_records_device", "qpsk_stream_create_records",
           "qpsk_stream_retrieve_records",
           "qpsk_level_host", "qpsk_level_device", "qpsk_level_tiling", "qpsk_level_dbfs",
           "qpsk_level_sumsq_of_dbfs", "qpsk_squelch_host", "qpsk_squelch_device",
           "qpsk_rx_batch_records_squelch", "qpsk_rx_batch_records_squelch_device",
           "qpsk_input_level_work_bytes", "qpsk_input_convert_level_host", "qpsk_input_convert_level_device",
           "qpsk_rx_batch_records_squelch_fmt", "qpsk_rx_batch_records_squelch_device_fmt",
           "qpsk_stream_create_records_squelch", "qpsk_stream_retrieve_records_squelch"]


def _check(rc: int) -> None:
    if rc != 0:
        e = QpskError(f"qpsk error {rc}: {lib().qpsk_strerror(rc).decode()}")
        e.code = rc
        raise e


def _ptr(a) -> int | None:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor (device memory)


# receiver semantics (include/qpsk_batch.h QPSK_MODE_*)
MODE_REFERENCE = 0   # bit-identical to the reference as built
MODE_DEC752 = 1      # decimated_frame[752] ("intended semantics"), NOT reference parity
MODE_FFT_HUNT = 2    # flag: preamble hunt through the reference's kiss_fft (src/fft.c)


# input formats (include/qpsk_input.h): a format word is encoding | layout
IN_S16, IN_ALAW, IN_ULAW = 0, 1, 2
IN_PLANAR, IN_INTERLEAVED = 0, 0x10


def _enc(fmt: int) -> int:      # IN_S16, IN_ALAW, IN_ULAW
    return fmt & 0x0f


def _layout(fmt: int) -> int:   # IN_PLANAR, IN_INTERLEAVED
    return fmt & ~0x0f


def _in_dtype(fmt: int):
    return np.int16 if _enc(fmt) == IN_S16 else np.uint8


def _threads(threads: int) -> int:
    """Host threads of a call: the caller's, or by default up to 16."""
    return threads or min(16, os.cpu_count() or 1)


def _stream(stream, device):
    """The hipStream_t of ``stream`` (default: torch's current stream on `device`)."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return C.c_void_p(stream.cuda_stream)


def _on(stream, device):
    """The torch stream context of a device call: ``stream``, or torch's current
    stream on `device`.  A wrapper allocates the tensors it makes inside it, so
    their memory belongs to the stream the call is enqueued on."""
    import torch
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device))


def _fmt_check(fmt: int, nch: int) -> None:
    """QPSK_EINVAL for an unknown format word or nch < 1 (the library's own
    check: a call of no frames)."""
    _check(lib().qpsk_input_convert_host(fmt, None, nch, nch, 0, None, 1))


def _in_block(x, fmt: int, nch: int, what: str = "x"):
    """(nframes, ld) of a source block in format `fmt`: planar [nch][T],
    interleaved [T][ld] with ld >= nch (a 2-D array or tensor whose rows are
    ld elements apart and whose elements along a row are adjacent; the columns
    past nch need not belong to it), T = nframes * 1880.  Works on numpy
    arrays and torch tensors alike."""
    shape = tuple(x.shape)
    if _layout(fmt) == IN_INTERLEAVED:
        if len(shape) != 2 or shape[1] != nch or shape[0] % FRAME_SIZE:
            raise ValueError(f"{what} must be [nframes * {FRAME_SIZE}][{nch}], got {shape}")
        return shape[0] // FRAME_SIZE, None
    n = 1
    for d in shape[1:]:
        n *= d
    if len(shape) < 2 or shape[0] != nch or n % FRAME_SIZE:
        raise ValueError(f"{what} must be [{nch}][nframes * {FRAME_SIZE}], got {shape}")
    return n // FRAME_SIZE, 0


def _np_block(x, fmt: int, nch: int):
    """A numpy source block as (array that owns the memory, nframes, ld).  An
    interleaved block may be a column range of a wider array (ld = its row
    length) and may start at any element; anything else is made contiguous."""
    x = np.asarray(x)
    if x.dtype != _in_dtype(fmt):
        raise ValueError(f"format {fmt:#x} takes {np.dtype(_in_dtype(fmt)).name} input, got {x.dtype}")
    nf, ld = _in_block(x, fmt, nch)
    if ld is None:
        es = x.itemsize
        if x.shape[0] > 1 and (x.strides[1] != es or x.strides[0] % es or x.strides[0] < nch * es):
            x = np.ascontiguousarray(x)
        elif x.shape[0] <= 1 and x.strides[1] != es:
            x = np.ascontiguousarray(x)
        ld = x.strides[0] // es if x.shape[0] > 1 else nch
    elif not x.flags.c_contiguous:
        x = np.ascontiguousarray(x)
    return x, nf, ld


def input_bytes(fmt: int, nch: int, nframes: int, ld: int = 0) -> int:
    """qpsk_input_bytes: bytes of a source block from its first element to its
    last (0 for arguments the conversions refuse)."""
    return int(lib().qpsk_input_bytes(fmt, nch, nframes, ld))


def input_convert_host(x, fmt: int, nch: int, threads: int = 0) -> np.ndarray:
    """qpsk_input_convert_host: a source block in format `fmt` (planar
    [nch][T] or interleaved [T][nch], possibly a column range of a wider
    array) -> int16 [nch][nframes][1880], on the host."""
    _fmt_check(fmt, nch)
    x, nf, ld = _np_block(x, fmt, nch)
    out = np.empty((nch, nf, FRAME_SIZE), np.int16)
    _check(lib().qpsk_input_convert_host(fmt, _ptr(x), ld, nch, nf, _ptr(out), _threads(threads)))
    return out


def _torch_block(x, fmt: int, nch: int):
    """(nframes, ld) of a cuda tensor in format `fmt`; an interleaved block may
    be a column range of a wider tensor."""
    import torch
    want = torch.int16 if _enc(fmt) == IN_S16 else torch.uint8
    if not x.is_cuda or x.dtype != want:
        raise ValueError(f"format {fmt:#x} takes a cuda {want} tensor")
    nf, ld = _in_block(x, fmt, nch)
    if ld is None:
        if (x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < nch)) or \
                (x.shape[0] <= 1 and nch > 1 and x.stride(1) != 1):
            raise ValueError("an interleaved block must have unit stride along a row and rows >= nch apart")
        ld = x.stride(0) if x.shape[0] > 1 else nch
    elif not x.is_contiguous():
        raise ValueError("a planar block must be contiguous")
    return nf, ld


def input_convert_device(x, fmt: int, nch: int, out=None, stream=None):
    """qpsk_input_convert_device: a cuda tensor in format `fmt` -> a torch int16
    tensor [nch][nframes][1880] on the same device; enqueued on ``stream``
    (default: torch's current stream)."""
    import torch
    _fmt_check(fmt, nch)
    nf, ld = _torch_block(x, fmt, nch)
    if out is not None and (out.dtype != torch.int16 or tuple(out.shape) != (nch, nf, FRAME_SIZE)
                            or not out.is_contiguous() or not out.is_cuda):
        raise ValueError(f"out must be a contiguous cuda int16 [{nch}][{nf}][{FRAME_SIZE}] tensor")
    with torch.cuda.device(x.device), _on(stream, x.device):
        if out is None:
            out = torch.empty((nch, nf, FRAME_SIZE), dtype=torch.int16, device=x.device)
        _check(lib().qpsk_input_convert_device(fmt, x.data_ptr(), ld, nch, nf, out.data_ptr(),
                                               _stream(stream, x.device)))
    return out


# output formats (include/qpsk_output.h): the same words as the input's
OUT_S16, OUT_ALAW, OUT_ULAW = IN_S16, IN_ALAW, IN_ULAW
OUT_PLANAR, OUT_INTERLEAVED = IN_PLANAR, IN_INTERLEAVED


def _out_shape(fmt: int, nch: int, n: int, ld):
    """(rows, ld) of a block's array in format `fmt`: planar [nch][ld >= n],
    interleaved [n][ld >= nch]; ld None = the minimum."""
    inter = _layout(fmt) == OUT_INTERLEAVED
    least = nch if inter else n
    ld = least if ld is None else int(ld)
    _check(lib().qpsk_output_convert_host(fmt, None, n, nch, 0, None, ld, 1))   # the format word, nch
    if ld < least:
        _check(QPSK_EINVAL)
    return (n if inter else nch), ld


def _out_array(out, fmt: int, rows: int, ld: int) -> np.ndarray:
    """The [rows][ld] array a host call writes its block into: ``out``, checked, or zeros."""
    if out is None:
        return np.zeros((rows, ld), _in_dtype(fmt))
    if out.dtype != _in_dtype(fmt) or out.shape != (rows, ld) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a contiguous {np.dtype(_in_dtype(fmt)).name} [{rows}][{ld}] array")
    return out


def output_bytes(fmt: int, nch: int, n: int, ld: int) -> int:
    """qpsk_output_bytes: bytes of a block of nch channels x n samples from its
    first element to its last (0 for arguments the conversions refuse)."""
    return int(lib().qpsk_output_bytes(fmt, nch, n, ld))


def output_convert_host(x, fmt: int, ld: int | None = None, out=None, threads: int = 0) -> np.ndarray:
    """qpsk_output_convert_host: int16 [nch][n] (rows may be further apart:
    any array with unit stride along a row) -> the block in format `fmt`, as
    an array [nch][ld] (planar) or [n][ld] (interleaved) of int16 or uint8.
    Only the block's elements are written: with ``out`` given, the rest of it
    keeps its contents; otherwise the rest is zero."""
    x = np.asarray(x)
    if x.dtype != np.int16 or x.ndim != 2:
        raise ValueError(f"expected int16 [nch][n], got {x.dtype} {x.shape}")
    nch, n = x.shape
    if n > 1 and x.strides[1] != 2 or nch > 1 and (x.strides[0] % 2 or x.strides[0] < 2 * n):
        x = np.ascontiguousarray(x)
    src_ld = x.strides[0] // 2 if nch > 1 else n
    rows, ld = _out_shape(fmt, nch, n, ld)
    out = _out_array(out, fmt, rows, ld)
    _check(lib().qpsk_output_convert_host(fmt, _ptr(x), src_ld, nch, n, _ptr(out), ld, _threads(threads)))
    return out


def _torch_out(t, fmt: int, nch: int, n: int, what: str = "out") -> int:
    """ld of a cuda tensor that holds a block in format `fmt`: [nch][>= n]
    planar, [n][>= nch] interleaved, unit stride along a row, rows ld apart (a
    column range of a wider tensor is such a block)."""
    import torch
    want = torch.int16 if _enc(fmt) == OUT_S16 else torch.uint8
    inter = _layout(fmt) == OUT_INTERLEAVED
    rows, cols = (n, nch) if inter else (nch, n)
    if not t.is_cuda or t.dtype != want or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols \
            or (t.shape[1] > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < cols):
        raise ValueError(f"{what} must be a cuda {want} [{rows}][>= {cols}] tensor with unit stride along a row")
    return t.stride(0) if rows > 1 else max(t.stride(0), cols)


def output_convert_device(x, fmt: int, out, stream=None) -> None:
    """qpsk_output_convert_device: a cuda int16 tensor [nch][n] (unit stride
    along a row) into ``out``, a cuda tensor that holds the block in format
    `fmt` ([nch][>= n] planar, [n][>= nch] interleaved, possibly a column range
    of a wider tensor); enqueued on ``stream`` (default: torch's current
    stream).  Only the block's elements are written."""
    import torch
    if not x.is_cuda or x.dtype != torch.int16 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("x must be a cuda int16 [nch][n] tensor with unit stride along a row")
    nch, n = x.shape
    src_ld = x.stride(0) if nch > 1 else max(x.stride(0), n)
    _out_shape(fmt, nch, n, None)
    ld = _torch_out(out, fmt, nch, n)
    with torch.cuda.device(x.device):
        _check(lib().qpsk_output_convert_device(fmt, x.data_ptr(), src_ld, nch, n, out.data_ptr(), ld,
                                                _stream(stream, x.device)))


def _rx_arrays(nch: int, nf: int, trace: bool, soft: bool) -> dict:
    """The host arrays a receive call of nf frames fills."""
    out = {"bits": np.zeros((nch, nf, NBITS), np.uint8),
           "valid": np.zeros((nch, nf), np.uint8)}
    if trace:
        out["trace"] = np.zeros((nch, nf, 4), np.int32)
    if soft:
        out["soft"] = np.zeros((nch, nf, DATA_SYMBOLS, 2), np.float32)
    return out


def _rx_tensors_check(nch: int, nf: int, bits, valid, trace, soft) -> None:
    """The output tensors of a device receive call of nf frames."""
    for name, t, shape in (("bits", bits, (nch, nf, NBITS)),
                           ("valid", valid, (nch, nf)),
                           ("trace", trace, (nch, nf, 4)),
                           ("soft", soft, (nch, nf, DATA_SYMBOLS, 2))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"{name} must be a contiguous cuda tensor of shape {shape}")


# --- the receive output as records (include/qpsk_compact.h) ---

REC_BY_CHANNEL, REC_BY_FRAME = 0, 1
# qpsk_frame_rec: 16 bytes, little endian
REC_DTYPE = np.dtype([("channel", "<u4"), ("frame", "<u4"), ("bits", "<u8")])


def compact_tiling() -> dict:
    """qpsk_compact_tiling: the device compaction's tiling -- the items one
    wave ranks (``run_items``), those of one workgroup (``block_items``) and
    the counts the scan's workgroup takes per trip (``scan_trip``)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().qpsk_compact_tiling(C.byref(a), C.byref(b), C.byref(c))
    return {"run_items": a.value, "block_items": b.value, "scan_trip": c.value}


def compact_work_bytes(nch: int, nframes: int) -> int:
    """qpsk_compact_work_bytes: bytes of compact_device's work area."""
    return int(lib().qpsk_compact_work_bytes(nch, nframes))


def pack_bits(bits) -> np.ndarray:
    """qpsk_bits_pack_host: uint8 [..., 62] -> uint64 [...], bit i set iff
    bits[..., i] == 1."""
    bits = np.ascontiguousarray(bits, np.uint8)
    if bits.ndim < 1 or bits.shape[-1] != NBITS:
        raise ValueError(f"expected uint8 [...][{NBITS}], got {bits.shape}")
    out = np.zeros(bits.shape[:-1], np.uint64)
    _check(lib().qpsk_bits_pack_host(_ptr(bits), out.size, _ptr(out)))
    return out


def unpack_bits(words) -> np.ndarray:
    """qpsk_bits_unpack_host: uint64 [...] -> uint8 [..., 62] of 0/1."""
    words = np.ascontiguousarray(words, np.uint64)
    out = np.zeros(words.shape + (NBITS,), np.uint8)
    _check(lib().qpsk_bits_unpack_host(_ptr(words), words.size, _ptr(out)))
    return out


def pack_bits_device(bits, out=None, stream=None):
    """qpsk_bits_pack_device: a contiguous cuda uint8 tensor [..., 62] -> an
    int64 tensor [...] holding the words; enqueued on ``stream``."""
    import torch
    if not bits.is_cuda or bits.dtype != torch.uint8 or bits.shape[-1] != NBITS or not bits.is_contiguous():
        raise ValueError(f"bits must be a contiguous cuda uint8 [...][{NBITS}] tensor")
    with torch.cuda.device(bits.device), _on(stream, bits.device):
        if out is None:
            out = torch.empty(tuple(bits.shape[:-1]), dtype=torch.int64, device=bits.device)
        _check(lib().qpsk_bits_pack_device(bits.data_ptr(), out.numel(), out.data_ptr(),
                                           _stream(stream, bits.device)))
    return out


def _groups_of(order: int, nch: int, nf: int) -> int:
    return nf if order == REC_BY_FRAME else nch


def _rec_arrays(cap: int, trace: bool, soft: bool, ngroups: int) -> dict:
    """The host arrays a record call of at most cap records fills."""
    o = {"rec": np.zeros(cap, REC_DTYPE), "groups": np.zeros(max(ngroups, 0) + 1, np.uint32)}
    if trace:
        o["trace"] = np.zeros((cap, 4), np.int32)
    if soft:
        o["soft"] = np.zeros((cap, DATA_SYMBOLS, 2), np.float32)
    return o


def _rec_trim(o: dict, count: int, cap: int) -> dict:
    m = min(count, cap)
    r = {k: (v if k == "groups" else v[:m]) for k, v in o.items()}
    r["count"] = count
    return r


def compact_host(bits, valid, trace=None, soft=None, order: int = REC_BY_CHANNEL, cap: int | None = None,
                 out: dict | None = None) -> dict:
    """qpsk_compact_host: the dense outputs of a receive call (bits
    [nch][nframes][62], valid [nch][nframes], optionally trace and soft) ->
    {"rec" (REC_DTYPE), "count", "groups"} (+ "trace", "soft" rows), trimmed to
    min(count, cap) rows; cap None = every frame.  ``out``: the arrays to write
    into ("rec", "trace", "soft" of cap rows, "groups"; a missing one is not
    made), returned untrimmed with "count"."""
    valid = np.ascontiguousarray(valid, np.uint8)
    if valid.ndim != 2:
        raise ValueError(f"valid must be [nch][nframes], got {valid.shape}")
    nch, nf = valid.shape
    bits = np.ascontiguousarray(bits, np.uint8)
    if bits.shape != (nch, nf, NBITS):
        raise ValueError(f"bits must be [{nch}][{nf}][{NBITS}], got {bits.shape}")
    if trace is not None:
        trace = np.ascontiguousarray(trace, np.int32).reshape(nch, nf, 4)
    if soft is not None:
        soft = np.ascontiguousarray(soft, np.float32).reshape(nch, nf, DATA_SYMBOLS, 2)
    cap = nch * nf if cap is None else int(cap)
    o = out if out is not None else _rec_arrays(cap, trace is not None, soft is not None,
                                                _groups_of(order, nch, nf))
    count = C.c_uint32(0)
    _check(lib().qpsk_compact_host(_ptr(bits), _ptr(valid), _ptr(trace), _ptr(soft), nch, nf, order, cap,
                                   _ptr(o.get("rec")), _ptr(o.get("trace")), _ptr(o.get("soft")),
                                   _ptr(o.get("groups")), C.addressof(count)))
    return dict(o, count=int(count.value)) if out is not None else _rec_trim(o, int(count.value), cap)


def compact_device(bits, valid, trace=None, soft=None, order: int = REC_BY_CHANNEL, cap: int | None = None,
                   rec=None, rec_trace=None, rec_soft=None, groups=None, count=None, work=None, stream=None) -> dict:
    """qpsk_compact_device on cuda tensors: bits uint8 [nch][nframes][62], valid
    uint8 [nch][nframes] (+ trace int32 [..][4], soft float32 [..][31][2]).
    Outputs (made when None): rec int64 [cap][2] (rec_from_tensor gives
    REC_DTYPE on the host), rec_trace int32 [cap][4], rec_soft float32
    [cap][31][2], groups and count int32 (holding the uint32 values), work
    uint8 [compact_work_bytes].  Enqueued on ``stream``; returns the tensors
    untrimmed."""
    import torch
    nch, nf = tuple(valid.shape)
    dev = valid.device
    cap = nch * nf if cap is None else int(cap)
    with torch.cuda.device(dev), _on(stream, dev):
        if rec is None and cap > 0:
            rec = torch.empty((cap, 2), dtype=torch.int64, device=dev)
        if rec_trace is None and trace is not None:
            rec_trace = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        if rec_soft is None and soft is not None:
            rec_soft = torch.empty((cap, DATA_SYMBOLS, 2), dtype=torch.float32, device=dev)
        if groups is None:
            groups = torch.empty(_groups_of(order, nch, nf) + 1, dtype=torch.int32, device=dev)
        if count is None:
            count = torch.empty(1, dtype=torch.int32, device=dev)
        if work is None:
            work = torch.empty(compact_work_bytes(nch, nf), dtype=torch.uint8, device=dev)
        _check(lib().qpsk_compact_device(_ptr(bits), _ptr(valid), _ptr(trace), _ptr(soft), nch, nf, order, cap,
                                         _ptr(rec), _ptr(rec_trace), _ptr(rec_soft), _ptr(groups), _ptr(count),
                                         _ptr(work), work.numel(), _stream(stream, dev)))
    return {"rec": rec, "trace": rec_trace, "soft": rec_soft, "groups": groups, "count": count, "work": work}


def rec_from_tensor(rec, m: int | None = None) -> np.ndarray:
    """A device record tensor (int64 [cap][2]) as a REC_DTYPE array on the host
    (its first m rows)."""
    a = rec.cpu().numpy() if m is None else rec[:m].cpu().numpy()
    return np.ascontiguousarray(a).view(REC_DTYPE).reshape(-1)


# --- the input level meter and the squelch (include/qpsk_level.h) ---

# qpsk_frame_level: 16 bytes, little endian
LEVEL_DTYPE = np.dtype([("sumsq", "<u8"), ("sum", "<i4"), ("peak", "<u2"), ("clipped", "<u2")])
FULL_SUMSQ = FRAME_SIZE << 30   # sumsq of a frame of -32768: 0 dBFS


def level_tiling() -> dict:
    """qpsk_level_tiling: the rows (frames) one workgroup of the device meter
    takes (``rows_per_block``)."""
    r = C.c_int(0)
    lib().qpsk_level_tiling(C.byref(r))
    return {"rows_per_block": r.value}


def level_host(x) -> np.ndarray:
    """qpsk_level_host: int16 [..., 1880] -> LEVEL_DTYPE [...], the level of
    every frame."""
    x = np.ascontiguousarray(x, np.int16)
    if x.ndim < 1 or x.shape[-1] != FRAME_SIZE:
        raise ValueError(f"expected int16 [...][{FRAME_SIZE}], got {x.shape}")
    out = np.zeros(x.shape[:-1], LEVEL_DTYPE)
    _check(lib().qpsk_level_host(_ptr(x), out.size, _ptr(out)))
    return out


def level_device(x, out=None, stream=None):
    """qpsk_level_device: a contiguous cuda int16 tensor [..., 1880] -> an int64
    tensor [..., 2] holding the levels (level_from_tensor gives LEVEL_DTYPE on
    the host); enqueued on ``stream``."""
    import torch
    if not x.is_cuda or x.dtype != torch.int16 or x.dim() < 1 or x.shape[-1] != FRAME_SIZE or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous cuda int16 [...][{FRAME_SIZE}] tensor")
    with torch.cuda.device(x.device), _on(stream, x.device):
        if out is None:
            out = torch.empty(tuple(x.shape[:-1]) + (2,), dtype=torch.int64, device=x.device)
        _check(lib().qpsk_level_device(x.data_ptr(), x.numel() // FRAME_SIZE, out.data_ptr(),
                                       _stream(stream, x.device)))
    return out


def level_from_tensor(level) -> np.ndarray:
    """A device level tensor (int64 [..., 2]) as a LEVEL_DTYPE array [...] on the host."""
    a = np.ascontiguousarray(level.cpu().numpy())
    return a.view(LEVEL_DTYPE).reshape(a.shape[:-1])


def level_dbfs(level) -> np.ndarray:
    """qpsk_level_dbfs of every element of a LEVEL_DTYPE array (or of sumsq
    values): float64, -inf for sumsq == 0."""
    level = np.asarray(level)
    if level.dtype != LEVEL_DTYPE:
        q = np.zeros(level.shape, LEVEL_DTYPE)
        q["sumsq"] = level
        level = q
    level = np.ascontiguousarray(level)
    out = np.zeros(level.shape, np.float64)
    flat, o = level.reshape(-1), out.reshape(-1)
    for i in range(flat.size):
        o[i] = lib().qpsk_level_dbfs(flat[i:i + 1].ctypes.data)
    return out


def sumsq_of_dbfs(db: float) -> int:
    """qpsk_level_sumsq_of_dbfs: the smallest sumsq whose level is at least
    ``db`` dBFS -- the ``min_sumsq`` of a squelch at that level."""
    return int(lib().qpsk_level_sumsq_of_dbfs(float(db)))


def _levels(a, n: int, what: str):
    """A LEVEL_DTYPE array of n elements (or None)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, LEVEL_DTYPE)
    if a.size != n:
        raise ValueError(f"{what} must have {n} levels, got {a.shape}")
    return a


def squelch_host(level, valid, min_sumsq: int, prev=None, bits=None, soft=None, valid_out=None, last=None) -> dict:
    """qpsk_squelch_host: level LEVEL_DTYPE [nch][nframes] and valid uint8
    [nch][nframes] -> {"valid" (the squelched flags), "last" (LEVEL_DTYPE
    [nch], the levels the next call takes as ``prev``)}.  ``bits`` / ``soft``
    (the dense arrays, C-contiguous) are written in place: the rows of frames
    that were valid and are squelched become zero.  ``valid_out`` may be
    ``valid`` itself and ``last`` may be ``prev``."""
    # (an array that is contiguous and of the right type already is passed on
    # as it is, so valid_out = valid and last = prev reach the library as one array)
    valid = np.ascontiguousarray(valid, np.uint8)
    if valid.ndim != 2:
        raise ValueError(f"valid must be [nch][nframes], got {valid.shape}")
    nch, nf = valid.shape
    level = _levels(level, nch * nf, "level")
    prev = _levels(prev, nch, "prev")
    if valid_out is None:
        valid_out = np.zeros((nch, nf), np.uint8)
    if last is None:
        last = np.zeros(nch, LEVEL_DTYPE)
    for name, a, dt, shape in (("bits", bits, np.uint8, (nch, nf, NBITS)),
                               ("soft", soft, np.float32, (nch, nf, DATA_SYMBOLS, 2)),
                               ("valid_out", valid_out, np.uint8, (nch, nf)), ("last", last, LEVEL_DTYPE, (nch,))):
        if a is not None and (a.dtype != dt or a.shape != shape or not a.flags.c_contiguous):
            raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
    _check(lib().qpsk_squelch_host(_ptr(level), _ptr(prev), nch, nf, int(min_sumsq), _ptr(valid), _ptr(valid_out),
                                   _ptr(bits), _ptr(soft), _ptr(last)))
    return {"valid": valid_out, "last": last}


def squelch_device(level, valid, min_sumsq: int, prev=None, bits=None, soft=None, valid_out=None, last=None,
                   stream=None) -> dict:
    """qpsk_squelch_device on cuda tensors: level int64 [nch][nframes][2] (as
    level_device gives it), valid uint8 [nch][nframes], prev / last int64
    [nch][2], bits uint8 [nch][nframes][62] and soft float32
    [nch][nframes][31][2] (written in place).  valid_out and last are made
    when None; enqueued on ``stream``."""
    import torch
    nch, nf = tuple(valid.shape)
    dev = valid.device
    with torch.cuda.device(dev), _on(stream, dev):
        if valid_out is None:
            valid_out = torch.empty((nch, nf), dtype=torch.uint8, device=dev)
        if last is None:
            last = torch.empty((nch, 2), dtype=torch.int64, device=dev)
        _check(lib().qpsk_squelch_device(_ptr(level), _ptr(prev), nch, nf, int(min_sumsq), _ptr(valid),
                                         _ptr(valid_out), _ptr(bits), _ptr(soft), _ptr(last), _stream(stream, dev)))
    return {"valid": valid_out, "last": last}


def input_level_work_bytes(fmt: int, nch: int, nframes: int, ld: int = 0) -> int:
    """qpsk_input_level_work_bytes: bytes of input_convert_level_device's work
    area (0 for a planar block, for no frames and for refused arguments)."""
    return int(lib().qpsk_input_level_work_bytes(fmt, nch, nframes, ld))


def input_convert_level_host(x, fmt: int, nch: int, threads: int = 0):
    """qpsk_input_convert_level_host: input_convert_host and level_host of its
    output, as (int16 [nch][nframes][1880], LEVEL_DTYPE [nch][nframes])."""
    _fmt_check(fmt, nch)
    x, nf, ld = _np_block(x, fmt, nch)
    out = np.empty((nch, nf, FRAME_SIZE), np.int16)
    level = np.zeros((nch, nf), LEVEL_DTYPE)
    _check(lib().qpsk_input_convert_level_host(fmt, _ptr(x), ld, nch, nf, _ptr(out), _ptr(level), _threads(threads)))
    return out, level


def input_convert_level_device(x, fmt: int, nch: int, out=None, level=None, work=None, stream=None):
    """qpsk_input_convert_level_device: input_convert_device that also takes
    the level of every frame in the same pass.  Returns (out, level): int16
    [nch][nframes][1880] and int64 [nch][nframes][2] (see level_from_tensor)
    on the source's device.  ``work`` (a cuda uint8 tensor of at least
    input_level_work_bytes) is made when None; enqueued on ``stream``."""
    import torch
    _fmt_check(fmt, nch)
    nf, ld = _torch_block(x, fmt, nch)
    dev = x.device
    if out is not None and (out.dtype != torch.int16 or tuple(out.shape) != (nch, nf, FRAME_SIZE)
                            or not out.is_contiguous() or not out.is_cuda):
        raise ValueError(f"out must be a contiguous cuda int16 [{nch}][{nf}][{FRAME_SIZE}] tensor")
    if level is not None and (level.dtype != torch.int64 or tuple(level.shape) != (nch, nf, 2)
                              or not level.is_contiguous() or not level.is_cuda):
        raise ValueError(f"level must be a contiguous cuda int64 [{nch}][{nf}][2] tensor")
    need = input_level_work_bytes(fmt, nch, nf, ld)
    with torch.cuda.device(dev), _on(stream, dev):
        if out is None:
            out = torch.empty((nch, nf, FRAME_SIZE), dtype=torch.int16, device=dev)
        if level is None:
            level = torch.empty((nch, nf, 2), dtype=torch.int64, device=dev)
        if work is None and need:
            work = torch.empty(need, dtype=torch.uint8, device=dev)
        _check(lib().qpsk_input_convert_level_device(fmt, x.data_ptr(), ld, nch, nf, out.data_ptr(), level.data_ptr(),
                                                     _ptr(work), work.numel() if work is not None else 0,
                                                     _stream(stream, dev)))
    return out, level


class Receiver:
    """A batch of ``nch`` independent receivers on one GPU (``qpsk_ctx``).

    Each channel behaves like the reference receiver fed that channel's stream
    from a fresh start (src/qpsk.c:427-458); state persists across calls.
    ``mode`` selects the receiver semantics (MODE_REFERENCE or MODE_DEC752).
    """

    def __init__(self, nch: int, device: int = 0, mode: int = MODE_REFERENCE):
        err = C.c_int(0)
        self._h = lib().qpsk_rx_create_mode(device, nch, mode, C.byref(err))
        if not self._h:
            _check(err.value or -3)
        self.nch = nch
        self.device = device
        self.mode = int(lib().qpsk_rx_mode(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().qpsk_rx_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self) -> None:
        _check(lib().qpsk_rx_reset(self._h))

    @property
    def frames(self) -> int:
        return int(lib().qpsk_rx_frames(self._h))

    def state_save(self, c0: int = 0, n: int | None = None) -> bytes:
        """Snapshot of channels [c0, c0 + n) (qpsk_rx_state_save): the carried
        per-channel state and the frame index, as bytes."""
        n = self.nch - c0 if n is None else n
        buf = np.zeros(int(lib().qpsk_rx_state_size(n)), np.uint8)
        _check(lib().qpsk_rx_state_save(self._h, c0, n, _ptr(buf), buf.size))
        return buf.tobytes()

    @staticmethod
    def _snapshot(snap: bytes, n):
        """(buffer, n) of a snapshot: length and magic checked before its header is read."""
        buf = np.frombuffer(snap, np.uint8)
        if len(snap) < 64 or bytes(snap[:8]) != b"QPSKSTA1":   # StateHdr: 64 bytes, magic first
            _check(QPSK_EINVAL)
        if n is None:
            n = int(np.frombuffer(snap[20:24], np.int32)[0])   # StateHdr.n
        return buf, n

    def state_load(self, snap: bytes, c0: int = 0, n: int | None = None) -> None:
        """Load a snapshot of n channels into channels [c0, c0 + n)
        (qpsk_rx_state_load)."""
        buf, n = self._snapshot(snap, n)
        _check(lib().qpsk_rx_state_load(self._h, c0, n, _ptr(buf), buf.size))

    def state_join(self, snap: bytes, c0: int = 0, n: int | None = None) -> None:
        """Load a snapshot of n channels, taken at any frame index, into
        channels [c0, c0 + n) while the others go on: the joined channels
        continue at the snapshot's index (qpsk_rx_state_join)."""
        buf, n = self._snapshot(snap, n)
        _check(lib().qpsk_rx_state_join(self._h, c0, n, _ptr(buf), buf.size))

    def reset_channels(self, c0: int, n: int = 1) -> None:
        """Channels [c0, c0 + n) back to their initial state, at own frame index
        0; every other channel is untouched (qpsk_rx_reset_channels)."""
        _check(lib().qpsk_rx_reset_channels(self._h, c0, n))

    def channel_frames(self, c0: int = 0, n: int | None = None) -> np.ndarray:
        """The own frame index of channels [c0, c0 + n), uint64 [n]
        (qpsk_rx_channel_frames); ``frames`` stays the context's."""
        n = self.nch - c0 if n is None else n
        out = np.zeros(max(n, 0), np.uint64)
        _check(lib().qpsk_rx_channel_frames(self._h, c0, n, _ptr(out)))
        return out

    def timing(self, on: bool = True) -> None:
        """Enable per-call step-kernel span events (see qpsk_rx_timing_collect)."""
        _check(lib().qpsk_rx_timing_enable(self._h, int(on)))

    def collect_timing(self):
        """(summed kernel span in ms, frames) since the last collect."""
        ms, n = C.c_float(0), C.c_int(0)
        _check(lib().qpsk_rx_timing_collect(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def collect_timing_split(self):
        """(rx_kernel ms, rx_data_kernel ms, frames) since the last collect."""
        a, b, n = C.c_float(0), C.c_float(0), C.c_int(0)
        _check(lib().qpsk_rx_timing_split(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return float(a.value), float(b.value), int(n.value)

    def demod(self, x, trace: bool = False, soft: bool = False):
        """Host arrays: x int16 [nch][nframes][1880] -> dict of numpy arrays
        bits [nch][nframes][62], valid [nch][nframes] (+ trace [..][4], soft [..][31][2])."""
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 3 or x.shape[0] != self.nch or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"expected int16 [{self.nch}][nframes][{FRAME_SIZE}], got {x.shape}")
        nf = x.shape[1]
        out = _rx_arrays(self.nch, nf, trace, soft)
        _check(lib().qpsk_rx_batch(self._h, _ptr(x), nf, _ptr(out["bits"]), _ptr(out["valid"]),
                                   _ptr(out.get("trace")), _ptr(out.get("soft"))))
        return out

    def demod_fmt(self, x, fmt: int, trace: bool = False, soft: bool = False):
        """``demod`` for a host source block in format ``fmt`` (IN_*): planar
        [nch][nframes * 1880] or interleaved [nframes * 1880][nch] (possibly a
        column range of a wider array: ld is its row length), int16 or uint8
        G.711 codes.  The block crosses PCIe as it is and is converted on the
        GPU (qpsk_rx_batch_fmt)."""
        _fmt_check(fmt, self.nch)
        x, nf, ld = _np_block(x, fmt, self.nch)
        out = _rx_arrays(self.nch, nf, trace, soft)
        _check(lib().qpsk_rx_batch_fmt(self._h, _ptr(x), fmt, ld, nf, _ptr(out["bits"]),
                                       _ptr(out["valid"]), _ptr(out.get("trace")), _ptr(out.get("soft"))))
        return out

    def demod_device_fmt(self, x, fmt: int, bits, valid, trace=None, soft=None, stream=None) -> None:
        """``demod_device`` for a cuda source block in format ``fmt`` (layouts
        as demod_fmt): conversion and receive are enqueued on ``stream``
        (qpsk_rx_batch_device_fmt)."""
        _fmt_check(fmt, self.nch)
        nf, ld = _torch_block(x, fmt, self.nch)
        _rx_tensors_check(self.nch, nf, bits, valid, trace, soft)
        _check(lib().qpsk_rx_batch_device_fmt(self._h, x.data_ptr(), fmt, ld, nf, _ptr(bits), _ptr(valid),
                                              _ptr(trace), _ptr(soft), _stream(stream, x.device)))

    def demod_records(self, x, order: int = REC_BY_CHANNEL, cap: int | None = None, trace: bool = False,
                      soft: bool = False) -> dict:
        """``demod`` whose output is the list of the valid frames
        (qpsk_rx_batch_records): {"rec" (REC_DTYPE: channel, frame, bits),
        "count", "groups"} (+ "trace", "soft" rows), in ``order``, trimmed to
        min(count, cap) rows.  The dense outputs never leave the device."""
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 3 or x.shape[0] != self.nch or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"expected int16 [{self.nch}][nframes][{FRAME_SIZE}], got {x.shape}")
        nf = x.shape[1]
        cap = self.nch * nf if cap is None else int(cap)
        o = _rec_arrays(cap, trace, soft, _groups_of(order, self.nch, nf))
        count = C.c_uint32(0)
        _check(lib().qpsk_rx_batch_records(self._h, _ptr(x), nf, order, cap, _ptr(o["rec"]), _ptr(o.get("trace")),
                                           _ptr(o.get("soft")), _ptr(o["groups"]), C.addressof(count)))
        return _rec_trim(o, int(count.value), cap)

    def demod_records_fmt(self, x, fmt: int, order: int = REC_BY_CHANNEL, cap: int | None = None,
                          trace: bool = False, soft: bool = False) -> dict:
        """``demod_records`` for a host source block in format ``fmt`` (as
        demod_fmt takes it; qpsk_rx_batch_records_fmt)."""
        _fmt_check(fmt, self.nch)
        x, nf, ld = _np_block(x, fmt, self.nch)
        cap = self.nch * nf if cap is None else int(cap)
        o = _rec_arrays(cap, trace, soft, _groups_of(order, self.nch, nf))
        count = C.c_uint32(0)
        _check(lib().qpsk_rx_batch_records_fmt(self._h, _ptr(x), fmt, ld, nf, order, cap, _ptr(o["rec"]),
                                               _ptr(o.get("trace")), _ptr(o.get("soft")), _ptr(o["groups"]),
                                               C.addressof(count)))
        return _rec_trim(o, int(count.value), cap)

    def demod_records_device(self, x, order: int = REC_BY_CHANNEL, cap: int | None = None, trace: bool = False,
                             soft: bool = False, stream=None) -> dict:
        """``demod_device`` whose output is records, all on the device and
        asynchronous on ``stream`` (qpsk_rx_batch_records_device): returns the
        tensors of compact_device, untrimmed; check with ``sync``."""
        import torch
        if x.dtype != torch.int16 or x.dim() != 3 or x.shape[0] != self.nch \
                or x.shape[2] != FRAME_SIZE or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("x must be a contiguous cuda int16 [nch][nframes][1880] tensor")
        nf = x.shape[1]
        cap = self.nch * nf if cap is None else int(cap)
        dev = x.device
        with torch.cuda.device(dev), _on(stream, dev):
            rec = torch.empty((cap, 2), dtype=torch.int64, device=dev) if cap > 0 else None
            rtr = torch.empty((cap, 4), dtype=torch.int32, device=dev) if trace else None
            rso = torch.empty((cap, DATA_SYMBOLS, 2), dtype=torch.float32, device=dev) if soft else None
            groups = torch.empty(_groups_of(order, self.nch, nf) + 1, dtype=torch.int32, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            _check(lib().qpsk_rx_batch_records_device(self._h, _ptr(x), nf, order, cap, _ptr(rec), _ptr(rtr),
                                                      _ptr(rso), _ptr(groups), _ptr(count), _stream(stream, dev)))
        return {"rec": rec, "trace": rtr, "soft": rso, "groups": groups, "count": count}

    def demod_records_squelch(self, x, min_sumsq: int, prev=None, order: int = REC_BY_CHANNEL,
                              cap: int | None = None, trace: bool = False, soft: bool = False) -> dict:
        """``demod_records`` behind the level meter and the squelch
        (qpsk_rx_batch_records_squelch): frames whose own level and the level
        of the frame in front of them are both below ``min_sumsq`` (see
        sumsq_of_dbfs) give no record.  ``prev``: the ``"prev"`` of the
        previous call on this stream of frames (LEVEL_DTYPE [nch]; None at its
        start; not changed).  Returns what demod_records returns plus
        ``"level"`` (LEVEL_DTYPE [nch][nframes]) and the new ``"prev"``."""
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 3 or x.shape[0] != self.nch or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"expected int16 [{self.nch}][nframes][{FRAME_SIZE}], got {x.shape}")
        nf = x.shape[1]
        cap = self.nch * nf if cap is None else int(cap)
        o = _rec_arrays(cap, trace, soft, _groups_of(order, self.nch, nf))
        level = np.zeros((self.nch, nf), LEVEL_DTYPE)
        # (a prev of zeros is what NULL means)
        prev = np.zeros(self.nch, LEVEL_DTYPE) if prev is None else _levels(prev, self.nch, "prev").copy()
        count = C.c_uint32(0)
        _check(lib().qpsk_rx_batch_records_squelch(self._h, _ptr(x), nf, int(min_sumsq), _ptr(prev), order, cap,
                                                   _ptr(o["rec"]), _ptr(o.get("trace")), _ptr(o.get("soft")),
                                                   _ptr(o["groups"]), C.addressof(count), _ptr(level)))
        r = _rec_trim(o, int(count.value), cap)
        r["level"], r["prev"] = level, prev
        return r

    def demod_records_squelch_device(self, x, min_sumsq: int, prev=None, order: int = REC_BY_CHANNEL,
                                     cap: int | None = None, trace: bool = False, soft: bool = False,
                                     level: bool = True, stream=None) -> dict:
        """``demod_records_device`` behind the meter and the squelch, all on the
        device and asynchronous on ``stream``
        (qpsk_rx_batch_records_squelch_device).  ``prev``: a cuda int64 [nch][2]
        tensor that is read and then overwritten in stream order (None: the
        start of a stream, and nothing is carried).  Returns the tensors of
        demod_records_device plus ``"level"`` (int64 [nch][nframes][2], see
        level_from_tensor; None with level=False) and ``"prev"``."""
        import torch
        if x.dtype != torch.int16 or x.dim() != 3 or x.shape[0] != self.nch \
                or x.shape[2] != FRAME_SIZE or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("x must be a contiguous cuda int16 [nch][nframes][1880] tensor")
        if prev is not None and (prev.dtype != torch.int64 or tuple(prev.shape) != (self.nch, 2)
                                 or not prev.is_contiguous() or not prev.is_cuda):
            raise ValueError("prev must be a contiguous cuda int64 [nch][2] tensor")
        nf = x.shape[1]
        cap = self.nch * nf if cap is None else int(cap)
        dev = x.device
        with torch.cuda.device(dev), _on(stream, dev):
            rec = torch.empty((cap, 2), dtype=torch.int64, device=dev) if cap > 0 else None
            rtr = torch.empty((cap, 4), dtype=torch.int32, device=dev) if trace else None
            rso = torch.empty((cap, DATA_SYMBOLS, 2), dtype=torch.float32, device=dev) if soft else None
            groups = torch.empty(_groups_of(order, self.nch, nf) + 1, dtype=torch.int32, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            lvl = torch.empty((self.nch, nf, 2), dtype=torch.int64, device=dev) if level else None
            _check(lib().qpsk_rx_batch_records_squelch_device(self._h, _ptr(x), nf, int(min_sumsq), _ptr(prev), order,
                                                              cap, _ptr(rec), _ptr(rtr), _ptr(rso), _ptr(groups),
                                                              _ptr(count), _ptr(lvl), _stream(stream, dev)))
        return {"rec": rec, "trace": rtr, "soft": rso, "groups": groups, "count": count, "level": lvl, "prev": prev}

    def demod_records_squelch_fmt(self, x, fmt: int, min_sumsq: int, prev=None, order: int = REC_BY_CHANNEL,
                                  cap: int | None = None, trace: bool = False, soft: bool = False) -> dict:
        """``demod_records_squelch`` for a host source block in format ``fmt``
        (as demod_fmt takes it; qpsk_rx_batch_records_squelch_fmt).  The block
        crosses PCIe as it is; ``"level"`` is the level of the decoded samples,
        taken by the conversion's own pass."""
        _fmt_check(fmt, self.nch)
        x, nf, ld = _np_block(x, fmt, self.nch)
        cap = self.nch * nf if cap is None else int(cap)
        o = _rec_arrays(cap, trace, soft, _groups_of(order, self.nch, nf))
        level = np.zeros((self.nch, nf), LEVEL_DTYPE)
        prev = np.zeros(self.nch, LEVEL_DTYPE) if prev is None else _levels(prev, self.nch, "prev").copy()
        count = C.c_uint32(0)
        _check(lib().qpsk_rx_batch_records_squelch_fmt(self._h, _ptr(x), fmt, ld, nf, int(min_sumsq), _ptr(prev),
                                                       order, cap, _ptr(o["rec"]), _ptr(o.get("trace")),
                                                       _ptr(o.get("soft")), _ptr(o["groups"]), C.addressof(count),
                                                       _ptr(level)))
        r = _rec_trim(o, int(count.value), cap)
        r["level"], r["prev"] = level, prev
        return r

    def demod_records_squelch_device_fmt(self, x, fmt: int, min_sumsq: int, prev=None, order: int = REC_BY_CHANNEL,
                                         cap: int | None = None, trace: bool = False, soft: bool = False,
                                         level: bool = True, stream=None) -> dict:
        """``demod_records_squelch_device`` for a cuda source block in format
        ``fmt`` (layouts as demod_fmt; qpsk_rx_batch_records_squelch_device_fmt)."""
        import torch
        _fmt_check(fmt, self.nch)
        nf, ld = _torch_block(x, fmt, self.nch)
        if prev is not None and (prev.dtype != torch.int64 or tuple(prev.shape) != (self.nch, 2)
                                 or not prev.is_contiguous() or not prev.is_cuda):
            raise ValueError("prev must be a contiguous cuda int64 [nch][2] tensor")
        cap = self.nch * nf if cap is None else int(cap)
        dev = x.device
        with torch.cuda.device(dev), _on(stream, dev):
            rec = torch.empty((cap, 2), dtype=torch.int64, device=dev) if cap > 0 else None
            rtr = torch.empty((cap, 4), dtype=torch.int32, device=dev) if trace else None
            rso = torch.empty((cap, DATA_SYMBOLS, 2), dtype=torch.float32, device=dev) if soft else None
            groups = torch.empty(_groups_of(order, self.nch, nf) + 1, dtype=torch.int32, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            lvl = torch.empty((self.nch, nf, 2), dtype=torch.int64, device=dev) if level else None
            _check(lib().qpsk_rx_batch_records_squelch_device_fmt(self._h, x.data_ptr(), fmt, ld, nf, int(min_sumsq),
                                                                  _ptr(prev), order, cap, _ptr(rec), _ptr(rtr),
                                                                  _ptr(rso), _ptr(groups), _ptr(count), _ptr(lvl),
                                                                  _stream(stream, dev)))
        return {"rec": rec, "trace": rtr, "soft": rso, "groups": groups, "count": count, "level": lvl, "prev": prev}

    def sync(self) -> None:
        """Wait for the latest demod_device call; raise QpskError (QPSK_ESTALL)
        if any call since the previous check failed on the device."""
        _check(lib().qpsk_rx_sync(self._h))

    def demod_device(self, x, bits, valid, trace=None, soft=None, stream=None) -> None:
        """Device tensors (torch, on this device): enqueue on ``stream``
        (default: torch's current stream) and return without synchronising."""
        import torch
        if x.dtype != torch.int16 or x.dim() != 3 or x.shape[0] != self.nch \
                or x.shape[2] != FRAME_SIZE or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("x must be a contiguous cuda int16 [nch][nframes][1880] tensor")
        nf = x.shape[1]
        _rx_tensors_check(self.nch, nf, bits, valid, trace, soft)
        _check(lib().qpsk_rx_batch_device(self._h, _ptr(x), nf, _ptr(bits), _ptr(valid),
                                          _ptr(trace), _ptr(soft), _stream(stream, x.device)))


TX_PACKET = 1880         # transmitted samples per packet: 5 * (128 + 8 * 31)
PACKET_BITS = 8 * NBITS  # payload bytes per packet, uint8 [8][62]
TX_STATE_SIZE = (49 * 2 + 2) * 4   # sizeof(qpsk_tx_state), include/qpsk_synth.h


def _tx_bits(bits, nch=None):
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    if bits.ndim != 4 or bits.shape[2:] != (8, NBITS) or (nch is not None and bits.shape[0] != nch):
        raise ValueError(f"expected uint8 [{nch or 'nch'}][npackets][8][{NBITS}], got {bits.shape}")
    return bits


def _tx_bits_tensor(bits, nch: int) -> int:
    """npackets of a device call's payload tensor."""
    import torch
    if bits.dtype != torch.uint8 or bits.dim() != 4 or bits.shape[0] != nch \
            or tuple(bits.shape[2:]) != (8, NBITS) or not bits.is_contiguous() or not bits.is_cuda:
        raise ValueError("bits must be a contiguous cuda uint8 [nch][npackets][8][62] tensor")
    return bits.shape[1]


def _tx_mask(active, nch: int, npk: int):
    """A host call's mask: None, or uint8 [nch][npackets] (nonzero = the
    channel sends in that slot; any other dtype is compared with 0)."""
    if active is None:
        return None
    active = np.asarray(active)
    if active.dtype != np.uint8:
        active = active != 0
    active = np.ascontiguousarray(active, dtype=np.uint8)
    if active.shape != (nch, npk):
        raise ValueError(f"active must be [{nch}][{npk}], got {active.shape}")
    return active


def _tx_mask_tensor(active, nch: int, npk: int):
    """A device call's mask: None, or a contiguous cuda uint8 / bool tensor
    [nch][npackets] (any address)."""
    import torch
    if active is None:
        return None
    if active.dtype not in (torch.uint8, torch.bool) or tuple(active.shape) != (nch, npk) \
            or not active.is_contiguous() or not active.is_cuda:
        raise ValueError(f"active must be a contiguous cuda uint8 or bool [{nch}][{npk}] tensor")
    return active.view(torch.uint8)


class Transmitter:
    """A batch of ``nch`` independent transmitters on one GPU (``qpsk_tx_ctx``,
    include/qpsk_tx.h).

    Each channel is the reference transmitter in the packet order of its
    main() (src/qpsk.c:380-413) with the caller's payload bits; ``gap`` zero
    samples follow every packet.  State persists across calls.  Like
    ``Receiver`` there is no CPU fallback: without a GPU the constructor raises
    (``tx_batch_host`` is the explicit host path).

    Channels may come and go (include/qpsk_tx.h "Channels that come and go"):
    every ``modulate*`` takes ``active``, [nch][npackets], nonzero where the
    channel sends in that slot (None: every slot); an idle slot is 1880 + gap
    zeros and leaves the channel's state alone.  ``reset_channels`` starts
    channels afresh, ``state_save`` / ``state_load`` move them to another
    transmitter, ``channel_packets`` reads their own packet indices.
    """

    def __init__(self, nch: int, device: int = 0, gap: int = 903):
        err = C.c_int(0)
        self._h = lib().qpsk_tx_create(device, nch, gap, C.byref(err))
        if not self._h:
            _check(err.value or -3)
        self.nch, self.device, self.gap = nch, device, gap

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().qpsk_tx_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self) -> None:
        _check(lib().qpsk_tx_reset(self._h))

    def sync(self) -> None:
        _check(lib().qpsk_tx_sync(self._h))

    def packets(self) -> int:
        return int(lib().qpsk_tx_packets(self._h))

    def reset_channels(self, c0: int, n: int = 1) -> None:
        """Channels [c0, c0 + n) back to the start state, at own packet index
        0; every other channel is untouched (qpsk_tx_reset_channels)."""
        _check(lib().qpsk_tx_reset_channels(self._h, c0, n))

    def channel_packets(self, c0: int = 0, n: int | None = None) -> np.ndarray:
        """The own packet index of channels [c0, c0 + n), uint64 [n]
        (qpsk_tx_channel_packets); ``packets`` stays the context's."""
        n = self.nch - c0 if n is None else n
        out = np.zeros(max(n, 0), np.uint64)
        _check(lib().qpsk_tx_channel_packets(self._h, c0, n, _ptr(out)))
        return out

    def state_save(self, c0: int = 0, n: int | None = None) -> bytes:
        """Snapshot of channels [c0, c0 + n) (qpsk_tx_state_save): their own
        packet indices and last 9 dibits, as bytes."""
        n = self.nch - c0 if n is None else n
        buf = np.zeros(int(lib().qpsk_tx_state_size(n)), np.uint8)
        _check(lib().qpsk_tx_state_save(self._h, c0, n, _ptr(buf), buf.size))
        return buf.tobytes()

    def state_load(self, snap: bytes, c0: int = 0, n: int | None = None) -> None:
        """Load a snapshot of n channels (default: as many as it holds), taken
        at any packet index and gap, into channels [c0, c0 + n) while the
        others go on (qpsk_tx_state_load)."""
        buf = np.frombuffer(snap, np.uint8)
        if n is None:
            if len(snap) < 16:
                _check(QPSK_EINVAL)
            n = int(np.frombuffer(snap[8:12], "<u4")[0])
        _check(lib().qpsk_tx_state_load(self._h, c0, n, _ptr(buf), buf.size))

    def modulate(self, bits, active=None) -> np.ndarray:
        """Host arrays: bits uint8 [nch][npackets][8][62] -> int16
        [nch][npackets * (1880 + gap)]; ``active`` [nch][npackets] marks the
        slots a channel sends in (qpsk_tx_batch_masked)."""
        bits = _tx_bits(bits, self.nch)
        npk = bits.shape[1]
        active = _tx_mask(active, self.nch, npk)
        out = np.zeros((self.nch, npk * (TX_PACKET + self.gap)), np.int16)
        _check(lib().qpsk_tx_batch_masked(self._h, _ptr(bits), _ptr(active), npk, _ptr(out), out.shape[1]))
        return out

    def modulate_device(self, bits, out, stream=None, active=None) -> None:
        """Device tensors (torch, on this device): bits uint8 [nch][npackets][8][62]
        contiguous, out int16 [nch][>= npackets * (1880 + gap)] with unit stride
        along a row and ld = out.stride(0).  Enqueues on ``stream`` (default:
        torch's current stream) and returns without synchronising.  ``active``
        is a cuda uint8 or bool tensor [nch][npackets], read in stream order
        (qpsk_tx_batch_masked_device)."""
        import torch
        npk = _tx_bits_tensor(bits, self.nch)
        active = _tx_mask_tensor(active, self.nch, npk)
        if out.dtype != torch.int16 or out.dim() != 2 or out.shape[0] != self.nch or not out.is_cuda \
                or out.shape[1] < npk * (TX_PACKET + self.gap) \
                or (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError("out must be a cuda int16 [nch][>= npackets * (1880 + gap)] tensor "
                             "with unit stride along a row")
        ld = out.stride(0) if self.nch > 1 else max(out.stride(0), out.shape[1])
        _check(lib().qpsk_tx_batch_masked_device(self._h, _ptr(bits), _ptr(active), npk, _ptr(out), ld,
                                                 _stream(stream, out.device)))

    def modulate_fmt(self, bits, fmt: int, ld: int | None = None, out=None, active=None) -> np.ndarray:
        """``modulate`` with the block in format ``fmt`` (OUT_*): uint8 G.711
        codes or int16, planar [nch][ld >= n] or interleaved [n][ld >= nch],
        n = npackets * (1880 + gap); ld None = the minimum.  Only the block's
        bytes cross PCIe and are written (qpsk_tx_batch_fmt): with ``out``
        given, a contiguous array of that shape, its row tails and foreign
        columns keep their contents; otherwise they are zero.  ``active`` as
        in ``modulate`` (qpsk_tx_batch_masked_fmt)."""
        bits = _tx_bits(bits, self.nch)
        npk = bits.shape[1]
        active = _tx_mask(active, self.nch, npk)
        rows, ld = _out_shape(fmt, self.nch, npk * (TX_PACKET + self.gap), ld)
        out = _out_array(out, fmt, rows, ld)
        _check(lib().qpsk_tx_batch_masked_fmt(self._h, _ptr(bits), _ptr(active), npk, _ptr(out), fmt, ld))
        return out

    def modulate_device_fmt(self, bits, out, fmt: int, ld: int | None = None, stream=None, active=None) -> None:
        """``modulate_device`` with the block in format ``fmt`` (OUT_*): ``out``
        is a cuda tensor [nch][>= n] (planar) or [n][>= nch] (interleaved) of
        uint8 codes or int16, unit stride along a row; ``ld`` defaults to its
        row stride.  The conversion follows the modulator on ``stream``.
        ``active`` as in ``modulate_device`` (qpsk_tx_batch_masked_device_fmt)."""
        npk = _tx_bits_tensor(bits, self.nch)
        active = _tx_mask_tensor(active, self.nch, npk)
        _out_shape(fmt, self.nch, npk * (TX_PACKET + self.gap), None)
        row = _torch_out(out, fmt, self.nch, npk * (TX_PACKET + self.gap))
        ld = row if ld is None else int(ld)
        _check(lib().qpsk_tx_batch_masked_device_fmt(self._h, _ptr(bits), _ptr(active), npk, _ptr(out), fmt, ld,
                                                     _stream(stream, out.device)))


def tx_states(nch: int) -> np.ndarray:
    """nch transmitter states (qpsk_tx_state) in main()'s start state, as uint8
    [nch][TX_STATE_SIZE]."""
    st = np.zeros((nch, TX_STATE_SIZE), np.uint8)
    for c in range(nch):
        lib().qpsk_tx_state_init(st[c].ctypes.data)
    return st


def tx_batch_host(bits, gap: int = 903, states=None, threads: int = 0, active=None) -> np.ndarray:
    """qpsk_tx_batch_host: the batched transmitter's contract on the host.
    bits uint8 [nch][npackets][8][62] -> int16 [nch][npackets * (1880 + gap)].
    ``states`` (tx_states(nch)) is advanced in place, so a stream may continue
    over calls; None starts every channel fresh.  ``active`` [nch][npackets]
    marks the slots a channel sends in (qpsk_tx_batch_masked_host): an idle
    slot is zeros and leaves the channel's state alone."""
    bits = _tx_bits(bits)
    nch, npk = bits.shape[:2]
    active = _tx_mask(active, nch, npk)
    if states is None:
        states = tx_states(nch)
    if states.dtype != np.uint8 or states.shape != (nch, TX_STATE_SIZE) or not states.flags.c_contiguous:
        raise ValueError(f"states must be tx_states({nch})")
    if gap < 0:
        _check(QPSK_EINVAL)
    out = np.zeros((nch, npk * (TX_PACKET + gap)), np.int16)
    _check(lib().qpsk_tx_batch_masked_host(_ptr(states), nch, _ptr(bits), _ptr(active), npk, gap, _ptr(out),
                                           out.shape[1], _threads(threads)))
    return out


# --- the reference's single-channel surface (headers/qpsk_internal.h:79-84) ---

class Stream:
    """Streaming ingest over pinned chunk slots (include/qpsk_stream.h): fill
    ``acquire()`` in place, ``submit()``, later ``retrieve()`` the oldest chunk.
    Every channel's state carries across chunks.  With ``fmt`` other than
    planar int16 (IN_*) the chunks are source blocks in that format, filled
    through ``acquire_raw()`` and converted on the GPU.  With ``records=True``
    the chunks come back through ``retrieve_records()`` as the list of their
    valid frames in ``order``, at most ``cap`` a chunk (include/qpsk_compact.h).
    With ``min_sumsq`` (and ``records=True``) the records pass the level meter
    and the squelch (include/qpsk_level.h): the stream carries each channel's
    last level from chunk to chunk, from zero at its start, and
    ``retrieve_records(levels=True)`` also gives the chunk's levels."""

    def __init__(self, nch: int, frames: int, nslot: int = 3, device: int = 0,
                 mode: int = MODE_REFERENCE, fmt: int = IN_S16 | IN_PLANAR, records: bool = False,
                 order: int = REC_BY_CHANNEL, cap: int | None = None, min_sumsq: int | None = None):
        err = C.c_int(0)
        self.records, self.order = bool(records), order
        self.cap = min(nch * frames, nch * frames if cap is None else int(cap))
        self.squelch = min_sumsq is not None
        if self.squelch and not records:
            raise ValueError("min_sumsq needs records=True")
        if self.squelch:
            self._h = lib().qpsk_stream_create_records_squelch(device, nch, frames, nslot, mode, fmt, order, self.cap,
                                                               int(min_sumsq), C.byref(err))
        elif records:
            self._h = lib().qpsk_stream_create_records(device, nch, frames, nslot, mode, fmt, order, self.cap,
                                                       C.byref(err))
        elif fmt == IN_S16 | IN_PLANAR:
            self._h = lib().qpsk_stream_create_mode(device, nch, frames, nslot, mode, C.byref(err))
        else:
            self._h = lib().qpsk_stream_create_fmt(device, nch, frames, nslot, mode, fmt, C.byref(err))
        if not self._h:
            _check(err.value or -3)
        self.nch, self.frames, self.nslot, self.fmt = nch, frames, nslot, fmt

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().qpsk_stream_destroy(self._h)
            self._h = None

    __del__ = close

    def acquire(self) -> np.ndarray:
        """The next chunk's pinned input buffer as int16 [nch][frames][1880]."""
        err = C.c_int(0)
        p = lib().qpsk_stream_acquire(self._h, C.byref(err))
        if not p:
            _check(err.value or -1)
        n = self.nch * self.frames * FRAME_SIZE
        buf = (C.c_int16 * n).from_address(p)
        return np.frombuffer(buf, np.int16).reshape(self.nch, self.frames, FRAME_SIZE)

    def acquire_raw(self) -> np.ndarray:
        """The next chunk's pinned source block in the stream's format: planar
        [nch][frames * 1880], interleaved [frames * 1880][nch]; int16 or uint8."""
        err = C.c_int(0)
        p = lib().qpsk_stream_acquire_raw(self._h, C.byref(err))
        if not p:
            _check(err.value or -1)
        dt = _in_dtype(self.fmt)
        n = self.nch * self.frames * FRAME_SIZE
        buf = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(p)
        a = np.frombuffer(buf, dt)
        if _layout(self.fmt) == IN_INTERLEAVED:
            return a.reshape(self.frames * FRAME_SIZE, self.nch)
        return a.reshape(self.nch, self.frames * FRAME_SIZE)

    def submit(self) -> None:
        _check(lib().qpsk_stream_submit(self._h))

    @property
    def pending(self) -> int:
        return int(lib().qpsk_stream_pending(self._h))

    def retrieve(self, copy: bool = True):
        """(bits [nch][frames][62], valid [nch][frames]) of the oldest chunk."""
        b, v = C.c_void_p(), C.c_void_p()
        _check(lib().qpsk_stream_retrieve(self._h, C.byref(b), C.byref(v)))
        cf = self.nch * self.frames
        bits = np.frombuffer((C.c_uint8 * (cf * NBITS)).from_address(b.value), np.uint8)
        valid = np.frombuffer((C.c_uint8 * cf).from_address(v.value), np.uint8)
        bits = bits.reshape(self.nch, self.frames, NBITS)
        valid = valid.reshape(self.nch, self.frames)
        return (bits.copy(), valid.copy()) if copy else (bits, valid)

    def retrieve_records(self, copy: bool = True, levels: bool = False) -> dict:
        """{"rec" (REC_DTYPE, min(count, cap) of them), "count", "groups"} of
        the oldest chunk of a ``records=True`` stream; with ``levels=True`` (a
        stream with ``min_sumsq``) also ``"level"``, LEVEL_DTYPE [nch][frames]."""
        r, g, count, lv = C.c_void_p(), C.c_void_p(), C.c_uint32(0), C.c_void_p()
        if levels:
            _check(lib().qpsk_stream_retrieve_records_squelch(self._h, C.byref(r), C.byref(count), C.byref(g),
                                                              C.byref(lv)))
        else:
            _check(lib().qpsk_stream_retrieve_records(self._h, C.byref(r), C.byref(count), C.byref(g)))
        m = min(int(count.value), self.cap)
        ng = _groups_of(self.order, self.nch, self.frames) + 1
        rec = np.frombuffer((C.c_uint8 * (16 * m)).from_address(r.value), REC_DTYPE) if m else np.zeros(0, REC_DTYPE)
        groups = np.frombuffer((C.c_uint32 * ng).from_address(g.value), np.uint32)
        out = {"rec": rec.copy() if copy else rec, "count": int(count.value),
               "groups": groups.copy() if copy else groups}
        if levels:
            cf = self.nch * self.frames
            level = np.frombuffer((C.c_uint8 * (16 * cf)).from_address(lv.value), LEVEL_DTYPE)
            level = level.reshape(self.nch, self.frames)
            out["level"] = level.copy() if copy else level
        return out


def cnormf(val: complex) -> float:
    """|val|^2 as the reference computes it (src/qpsk.c:75-80)."""
    return float(lib().cnormf(_CF(val.real, val.imag)))


def qpsk_mod(bits, index: int) -> complex:
    """Gray map: I = bits[index+1], Q = bits[index] (src/qpsk.c:251-256)."""
    i = -1.0 if bits[index + 1] == 1 else 1.0
    q = -1.0 if bits[index] == 1 else 1.0
    return complex(i, q)


def qpsk_demod(symbol: complex) -> list:
    """[Q, I] hard decisions, bits[1] = Re<0, bits[0] = Im<0 (src/qpsk.c:268-271)."""
    return [int(np.float32(symbol.imag) < 0), int(np.float32(symbol.real) < 0)]


def qpsk_rx_init() -> None:
    lib().qpsk_rx_init()
    _check(lib().qpsk_surface_error())


def qpsk_rx_frame(frame, bits=None):
    """One 1880-sample frame through the one-channel GPU receiver (src/qpsk.c:133).
    Returns 1 and fills bits[0..61] on a valid frame, else 0."""
    fr = np.ascontiguousarray(frame, dtype=np.int16)
    if fr.shape != (FRAME_SIZE,):
        raise ValueError("frame must be 1880 int16 samples")
    b = np.zeros(NBITS, np.uint8)
    v = lib().qpsk_rx_frame(_ptr(fr), _ptr(b))
    _check(lib().qpsk_surface_error())
    if v and bits is not None:
        bits[:NBITS] = b
    return v, b


def qpsk_tx_init() -> None:
    lib().qpsk_tx_init()


def qpsk_tx_frame(symbols, preamble: bool) -> np.ndarray:
    """Host TX of the reference (src/qpsk.c:278-322): len(symbols) complex
    symbols -> 5*len int16 samples."""
    s = np.ascontiguousarray(np.asarray(symbols, np.complex64))
    out = np.zeros(s.size * CYCLES, np.int16)
    n = lib().qpsk_tx_frame(_ptr(out), _ptr(s), s.size, bool(preamble))
    return out[:n]


def synth(seed: int, nch: int, nframes: int, ebn0_db: float = 1000.0, c0: int = 0,
          threads: int = 0) -> np.ndarray:
    """Synthetic channel streams int16 [nch][nframes][1880] (include/qpsk_synth.h)."""
    out = np.empty((nch, nframes, FRAME_SIZE), np.int16)
    lib().qpsk_synth_batch(seed, c0, nch, float(ebn0_db), _ptr(out), nframes * FRAME_SIZE,
                           _threads(threads))
    return out


def synth_device(seed: int, nch: int, nframes: int, ebn0_db: float = 1000.0, c0: int = 0,
                 device: int | None = None, out=None):
    """The same streams as synth(), generated on the GPU: a torch int16 tensor
    [nch][nframes][1880] on `device` (qpsk_synth_device)."""
    import torch
    if out is None:
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        out = torch.empty((nch, nframes, FRAME_SIZE), dtype=torch.int16, device=dev)
    with torch.cuda.device(out.device):
        stream = torch.cuda.current_stream().cuda_stream
        _check(lib().qpsk_synth_device(seed, c0, nch, float(ebn0_db), out.data_ptr(),
                                       nframes * FRAME_SIZE, stream))
    return out


def tx_phase_table(ntx: int) -> np.ndarray:
    """Carrier phase of the first ntx transmitted samples, float32 [ntx][2]."""
    out = np.empty((ntx, 2), np.float32)
    lib().qpsk_tx_phase_table(_ptr(out), ntx)
    return out


def read_raw(path: str) -> np.ndarray:
    """A reference .raw capture as frames [nframes][1880]; the short tail is
    dropped like the reference driver (src/qpsk.c:442-445)."""
    raw = np.fromfile(path, np.int16)
    nf = raw.size // FRAME_SIZE
    return raw[: nf * FRAME_SIZE].reshape(nf, FRAME_SIZE)


def records(bits: np.ndarray, valid: np.ndarray) -> bytes:
    """The reference driver's output file (src/qpsk.c:455-457): one 496-byte
    record per valid frame, bits in bytes 0..61, the rest zero (qpsk_records,
    host code)."""
    bits = np.ascontiguousarray(bits, np.uint8)
    valid = np.ascontiguousarray(valid, np.uint8)
    nf = valid.shape[0]
    out = np.empty(max(nf, 1) * BITS_PER_FRAME, np.uint8)
    n = lib().qpsk_records(_ptr(bits), _ptr(valid), nf, _ptr(out))
    return out[:n].tobytes()


class FftPlan:
    """The reference's kiss_fft on the GPU (include/qpsk_fft.h): fft_alloc(nfft,
    inverse) + batched fft(), bit-identical to src/fft.c.  nfft: a power of two
    in [4, 4096]."""

    def __init__(self, nfft: int, inverse: bool = False, device: int = 0):
        err = C.c_int(0)
        self._h = lib().qpsk_fft_alloc(device, nfft, int(inverse), C.byref(err))
        if not self._h:
            _check(err.value or -3)
        self.nfft, self.inverse, self.device = nfft, bool(inverse), device

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().qpsk_fft_free(self._h)
            self._h = None

    __del__ = close

    def __call__(self, x) -> np.ndarray:
        """complex64 [..., nfft] host array -> its transform (host)."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.shape[-1] != self.nfft:
            raise ValueError(f"last axis must be {self.nfft}")
        out = np.empty_like(x)
        _check(lib().qpsk_fft(self._h, _ptr(x), _ptr(out), x.size // self.nfft))
        return out

    def run_device(self, x, out=None, stream=None):
        """torch complex64 (or float32 [..., nfft, 2]) cuda tensors; enqueued."""
        import torch
        n = x.numel() // (self.nfft * (1 if x.is_complex() else 2))
        with torch.cuda.device(x.device), _on(stream, x.device):
            if out is None:
                out = torch.empty_like(x)
            _check(lib().qpsk_fft_device(self._h, x.data_ptr(), out.data_ptr(), n, _stream(stream, x.device)))
        return out


def fft_twiddle_table(nfft: int, inverse: bool = False) -> np.ndarray:
    """The product's host twiddle table (qpsk_fft_host.c), for tests."""
    tw = np.empty(nfft, np.complex64)
    lib().qpsk_fft_twiddle_table(nfft, int(inverse), _ptr(tw))
    return tw

"""ctypes binding of libjpeg_amd/libmijpeg.so (include/mijpeg.h) for tests and bench.py.

This is plumbing above the C ABI: it mirrors the decode half of the reference's `class JPEG`
(interface/jpeg.hpp:185-252): Read -> `Decoder.read`, GetInformation -> `Decoder.info`,
DisplayRectangle -> `Decoder.reconstruct` / `reconstruct_rect`, LastError -> `MijpegError`.
The product path has no CPU fallback: if the shared library (HIP kernels inside) is missing, `lib()`
fails loudly; if no GPU is present, every reconstruct call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIJPEG_LIBRARY") or os.path.join(HERE, "libmijpeg.so")  # MIJPEG_LIBRARY: another build of the same library (kernel experiments)

FLAG_NO_COLOR_TRANSFORM = 1
FLAG_FORCE_GENERIC = 2
FLAG_FORCE_SAFE = 4
FLAG_DEVICE_OUTPUT = 8
FLAG_NO_UPSAMPLING = 16
FLAG_SPECULATIVE = 32
FLAG_FORCE_DOT2 = 64  # (testing) the packed 4:2:0 kernel's 16-bit second pass whatever the range check says

ERR_DEVICE = -8191
ERR_NOT_AVAILABLE = -1029
ERR_INVALID_PARAMETER = -1024
ERR_OVERFLOW_PARAMETER = -1028
ERR_NOT_IMPLEMENTED = -1034  # MIJPEG_ERR_NOT_IMPLEMENTED (= MIJPEG_ERR_OPERATION_UNIMPLEMENTED)


class MijpegInfo(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("precision", C.c_int32),
        ("hsamp", C.c_int32 * 4), ("vsamp", C.c_int32 * 4), ("subx", C.c_int32 * 4), ("suby", C.c_int32 * 4),
        ("quant_index", C.c_int32 * 4), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32),
        ("blocks_w", C.c_int32 * 4), ("blocks_h", C.c_int32 * 4), ("restart_interval", C.c_int32),
        ("ycbcr", C.c_int32), ("fast_arith", C.c_int32), ("coef_offset", C.c_int64 * 4),
        ("coef_count", C.c_int64), ("quant", (C.c_uint16 * 64) * 4), ("range_max", C.c_int32 * 4),
        ("sample_bytes", C.c_int32), ("xt", C.c_int32), ("is_float", C.c_int32), ("progressive", C.c_int32),
        ("coef_wide", C.c_int32), ("dnl", C.c_int32), ("rows", C.c_int32 * 4),
    ]


class MijpegXtParams(C.Structure):
    _fields_ = [
        ("residual", MijpegInfo), ("ltable", (C.c_int32 * 4096) * 3), ("ltable_entries", C.c_int32), ("hidden_bits", C.c_int32),
        ("residual_hidden_bits", C.c_int32), ("residual_wide", C.c_int32), ("ltrafo_ycbcr", C.c_int32), ("rtrafo_ycbcr", C.c_int32),
        ("out_max", C.c_int32), ("out_shift", C.c_int32), ("is_float", C.c_int32), ("clamp", C.c_int32),
        ("general", C.c_int32), ("lmat", C.c_int32 * 9), ("rmat", C.c_int32 * 9), ("cmat", C.c_int32 * 9),
        ("rdct_bypass", C.c_int32), ("noise_shaping", C.c_int32), ("qtable_entries", C.c_int32),
        ("qtable", C.c_void_p * 3), ("r2table", C.c_void_p * 3), ("no_residual", C.c_int32), ("ltrafo_standard", C.c_int32), ("rct", C.c_int32), ("rbits", C.c_int32),
    ]


class MijpegBatch(C.Structure):
    _fields_ = [
        ("info", MijpegInfo), ("coef_dev", C.c_void_p), ("coef_frame_stride", C.c_int64),
        ("quant_dev", C.c_void_p), ("out_dev", C.c_void_p), ("out_frame_stride", C.c_int64),
        ("out_row_stride", C.c_int64), ("frames", C.c_int32), ("flags", C.c_uint32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("xt", C.POINTER(MijpegXtParams)),
    ]


class MijpegForwardBatch(C.Structure):
    _fields_ = [
        ("info", MijpegInfo), ("pixels_dev", C.c_void_p), ("pixel_frame_stride", C.c_int64), ("pixel_row_stride", C.c_int64),
        ("coef_dev", C.c_void_p), ("coef_frame_stride", C.c_int64), ("frames", C.c_int32), ("flags", C.c_uint32),
    ]


class MijpegBitmap(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes_per_pixel", C.c_int32), ("bytes_per_row", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32)]


class MijpegRaggedStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("images", "ragged", "fallbacks", "errors", "entropy_launches", "walk_launches", "recon_launches", "recon_single")]


class MijpegPlanarStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("images", "fused", "two_pass", "fused_launches", "two_pass_launches")]


class MijpegRect(C.Structure):
    """mijpeg_rect: a crop window on a picture's canvas, inclusive."""
    _fields_ = [(k, C.c_int32) for k in ("min_x", "min_y", "max_x", "max_y")]


class MijpegRaggedRectStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("images", "fused", "copied", "launches")] + [("workgroups", C.c_int64), ("workgroups_full", C.c_int64)]


class MijpegRaggedResizedStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("images", "resampled", "refused", "window_launches", "resample_launches", "reserved")] + [("arena_bytes", C.c_int64)]


SAMPLE_U8, SAMPLE_F32, SAMPLE_F16, SAMPLE_BF16 = 0, 1, 2, 3  # MIJPEG_SAMPLE_*
SAMPLE_BYTES = {SAMPLE_U8: 1, SAMPLE_F32: 4, SAMPLE_F16: 2, SAMPLE_BF16: 2}


class MijpegBatchFormat(C.Structure):
    """mijpeg_batch_format: what the normalised resized call stores per sample, and which pictures it mirrors."""
    _fields_ = [("sample", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3), ("mirror", C.c_void_p)]


class MijpegRaggedNormalizedStats(C.Structure):
    _fields_ = [("sample", C.c_int32), ("mirrored", C.c_int32), ("reserved", C.c_int32 * 2)]


class MijpegRaggedFrame(C.Structure):
    _fields_ = [("coef_base", C.c_int64), ("off_y", C.c_int64), ("off_cb", C.c_int64), ("off_cr", C.c_int64)] + \
               [(k, C.c_int32) for k in ("first_workgroup", "tiles_x", "tiles_y", "width", "height", "bw_y", "bh_y", "bw_c", "bh_c", "cw", "ch", "reserved")]


RAGGED_GROUPS = ("420", "422", "444", "grey")  # MIJPEG_RAGGED_420 ...
RAGGED_GROUPS16 = RAGGED_GROUPS + ("420_12", "422_12", "444_12", "grey_12")  # ... MIJPEG_RAGGED_420_12 ...: the ...16 calls


class MijpegEncodeFrame(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("row_stride", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32),
                ("hsamp", C.c_int32 * 4), ("vsamp", C.c_int32 * 4), ("quality", C.c_int32), ("restart_interval", C.c_int32)]


class MijpegEncodeRaggedItem(C.Structure):
    _fields_ = [("info", MijpegInfo), ("coef_base", C.c_int64), ("blocks", C.c_uint32), ("intervals", C.c_uint32), ("first_block", C.c_uint32),
                ("first_interval", C.c_uint32), ("pass_", C.c_int32), ("reserved", C.c_int32)]


class MijpegEncodeRaggedTotals(C.Structure):
    _fields_ = [("coef_count", C.c_int64), ("blocks", C.c_uint64), ("intervals", C.c_uint64), ("passes", C.c_int32), ("reserved", C.c_int32)]


class MijpegEncodeRaggedStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("pictures", "passes", "forward_launches", "coder_launches", "host_syncs", "reserved")] + [("bytes_downloaded", C.c_int64)]


class MijpegEncodePlanarStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("pictures", "fused", "two_pass", "own_plane", "interleave_launches", "reserved")]


class MijpegTranscodeSpec(C.Structure):
    _fields_ = [("quality", C.c_int32), ("restart_interval", C.c_int32)]


class MijpegTranscodeRaggedStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("pictures", "served", "kept", "refused", "children", "passes", "requant_launches", "coder_launches", "host_syncs",
                                         "child_uploads")] + [("bytes_downloaded", C.c_int64)]


TRANSCODE_KEEP, TRANSCODE_SKIP = 0, -1  # mijpeg_transcode_spec.quality: the source's tables; no stream for this picture


class MijpegTranscodeTransformStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("transformed", "trimmed", "geometry_refusals", "transform_launches")]


# MIJPEG_TRANSFORM_*: jpegtran's JXFORM_CODE, and the bit that trims partial MCUs of a mirrored axis
(TRANSFORM_NONE, TRANSFORM_FLIP_H, TRANSFORM_FLIP_V, TRANSFORM_TRANSPOSE, TRANSFORM_TRANSVERSE, TRANSFORM_ROT_90, TRANSFORM_ROT_180,
 TRANSFORM_ROT_270) = range(8)
TRANSFORM_TRIM = 0x100


# sampling factors (hsamp, vsamp) per component of the layouts the encoder takes by name
ENCODE_LAYOUTS = {"444": ((1, 1, 1), (1, 1, 1)), "420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "440": ((1, 1, 1), (2, 1, 1)),
                  "411": ((4, 1, 1), (1, 1, 1))}


def encode_frame(width: int, height: int, components: int, quality: int = 85, subsampling="444", restart_mcus: int = 0, pixels: int = 0,
                 row_stride: int | None = None) -> MijpegEncodeFrame:
    """A mijpeg_encode_frame.  subsampling: a name of ENCODE_LAYOUTS or (hsamp, vsamp) tuples; pixels: address (device or host)."""
    hs, vs = ENCODE_LAYOUTS[subsampling] if isinstance(subsampling, str) else subsampling
    e = MijpegEncodeFrame()
    e.pixels, e.row_stride = pixels or None, width * components if row_stride is None else row_stride
    e.width, e.height, e.components, e.quality, e.restart_interval = int(width), int(height), int(components), int(quality), int(restart_mcus)
    for c in range(min(4, len(hs))):
        e.hsamp[c], e.vsamp[c] = hs[c], vs[c]
    return e


class MijpegError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"mijpeg error {code}: {message}")
        self.code = code
        self.message = message


def build(force: bool = False) -> str:
    """Compile libmijpeg.so in-tree (hipcc --offload-arch=gfx950); cross-compiles without a GPU."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(HERE, "csrc")], check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the reconstruction path)")
        # When PyTorch is used in the same process (tests and bench.py use it for device buffers, streams and
        # torch.distributed) its bundled HIP runtime must be the one this library binds to: two HIP runtimes in
        # one process do not see each other's device state.  Importing torch first makes the dynamic linker
        # resolve libamdhip64 to the copy that is already loaded.  Without torch the system ROCm runtime is used.
        try:
            if not os.environ.get("MIJPEG_NO_TORCH"):  # (host-only helper processes have no use for it)
                import torch  # noqa: F401
        except Exception:  # torch is plumbing, not a dependency of the C ABI
            pass
        L = C.CDLL(LIB_PATH)
        P = C.POINTER
        L.mijpeg_version.restype = C.c_char_p
        L.mijpeg_create.argtypes = [P(C.c_void_p), C.c_int]
        L.mijpeg_destroy.argtypes = [C.c_void_p]
        L.mijpeg_destroy.restype = None
        L.mijpeg_set_input.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.mijpeg_read_header.argtypes = [C.c_void_p, P(MijpegInfo)]
        L.mijpeg_get_info.argtypes = [C.c_void_p, P(MijpegInfo)]
        L.mijpeg_get_xt_params.argtypes = [C.c_void_p, P(MijpegXtParams)]
        L.mijpeg_decode_coefficients.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_decode_coefficients_device.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_decode_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int]
        L.mijpeg_submit_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int]
        L.mijpeg_finish_batch_device.argtypes = [C.c_void_p]
        L.mijpeg_batch_speculation.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mijpeg_reconstruct_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_int]
        L.mijpeg_decode_ragged_device.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_int32)]
        L.mijpeg_ragged_info.argtypes = [C.c_void_p, C.c_int, P(MijpegInfo)]
        L.mijpeg_ragged_warning.argtypes = [C.c_void_p, C.c_int, P(C.c_char_p)]
        L.mijpeg_ragged_route.argtypes = [C.c_void_p, C.c_int, P(C.c_char_p)]
        L.mijpeg_reconstruct_ragged_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int]
        L.mijpeg_ragged_get_stats.argtypes = [C.c_void_p, P(MijpegRaggedStats)]
        L.mijpeg_reconstruct_planar_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.c_uint32, C.c_int]
        L.mijpeg_reconstruct_batch_planar_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_int]
        L.mijpeg_reconstruct_ragged_planar_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int]
        L.mijpeg_planar_stats_get.argtypes = [C.c_void_p, P(MijpegPlanarStats)]
        L.mijpeg_reconstruct_ragged_rect_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int]
        L.mijpeg_reconstruct_ragged_rect_planar_device.argtypes = L.mijpeg_reconstruct_ragged_rect_device.argtypes
        L.mijpeg_ragged_rect_stats_get.argtypes = [C.c_void_p, P(MijpegRaggedRectStats)]
        L.mijpeg_ragged_rect_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mijpeg_reconstruct_ragged_resized_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                               C.c_uint32, C.POINTER(C.c_int32), C.c_int]
        L.mijpeg_ragged_resized_stats_get.argtypes = [C.c_void_p, P(MijpegRaggedResizedStats)]
        L.mijpeg_reconstruct_ragged_normalized_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, P(MijpegBatchFormat), C.c_void_p, C.c_int64,
                                                                  C.c_int64, C.c_int64, C.c_uint32, C.POINTER(C.c_int32), C.c_int]
        L.mijpeg_ragged_normalized_stats_get.argtypes = [C.c_void_p, P(MijpegRaggedNormalizedStats)]
        L.mijpeg_resample_taps.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.mijpeg_resample_taps.restype = C.c_int32
        L.mijpeg_deinterleave_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int64]
        L.mijpeg_ragged_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mijpeg_ragged_plan16.argtypes = L.mijpeg_ragged_plan.argtypes
        L.mijpeg_decode_ragged_device16.argtypes = L.mijpeg_decode_ragged_device.argtypes
        L.mijpeg_encode_ragged_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged_get_stats.argtypes = [C.c_void_p, P(MijpegEncodeRaggedStats)]
        L.mijpeg_encode_ragged_plan16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged_device16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged_planar_device16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_planar_stats_get.argtypes = [C.c_void_p, P(MijpegEncodePlanarStats)]
        L.mijpeg_interleave_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int]
        if hasattr(L, "mijpeg_transcode_ragged_device"):  # (MIJPEG_LIBRARY may name a build from before the ragged transcode: its calls then fail by name)
            L.mijpeg_transcode_ragged_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.mijpeg_transcode_ragged_stats_get.argtypes = [C.c_void_p, P(MijpegTranscodeRaggedStats)]
            L.mijpeg_transcode_plan.argtypes = [P(MijpegInfo), P(MijpegTranscodeSpec), P(MijpegInfo), P(C.c_int32), P(C.c_int32)]
            L.mijpeg_requantize.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
            L.mijpeg_requantize.restype = C.c_int64
        if hasattr(L, "mijpeg_transcode_ragged_transformed_device"):  # (as above: a build from before the transforms fails by name)
            L.mijpeg_transcode_ragged_transformed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.mijpeg_transcode_transform_stats_get.argtypes = [C.c_void_p, P(MijpegTranscodeTransformStats)]
            L.mijpeg_transcode_plan_transformed.argtypes = [P(MijpegInfo), P(MijpegTranscodeSpec), C.c_int32, P(MijpegInfo), P(C.c_int32), P(C.c_int32)]
            L.mijpeg_transform_blocks.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
            L.mijpeg_transform_blocks.restype = C.c_int64
        L.mijpeg_free.argtypes = [C.c_void_p]
        L.mijpeg_free.restype = None
        L.mijpeg_set_device_markers.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_device_markers_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mijpeg_batch_pipeline_device_markers.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_device_markers_staging.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
        L.mijpeg_device_markers_staging.restype = C.c_void_p
        L.mijpeg_device_marker_search.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.mijpeg_device_marker_search.restype = C.c_int64
        L.mijpeg_device_walk_rounds.argtypes = [C.c_void_p]
        L.mijpeg_device_walk_rounds.restype = C.c_int
        L.mijpeg_speculative_scans.argtypes = [C.POINTER(C.c_int64)]
        L.mijpeg_speculative_scans.restype = C.c_int64
        L.mijpeg_coefficients.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_coefficients.restype = C.c_void_p
        L.mijpeg_coefficients32.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_coefficients32.restype = C.c_void_p
        L.mijpeg_device_coefficients.argtypes = [C.c_void_p]
        L.mijpeg_device_coefficients.restype = C.c_void_p
        L.mijpeg_reconstruct_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_int]
        L.mijpeg_reconstruct_rect.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_uint32, P(C.c_void_p), P(C.c_int32), P(C.c_int32)]
        L.mijpeg_reconstruct_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32]
        L.mijpeg_display_rect.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_uint32, P(MijpegBitmap)]
        L.mijpeg_display_plan.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_uint32, P(C.c_uint32), P(C.c_int32)]
        L.mijpeg_display_cursor.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_host_alloc.argtypes = [C.c_size_t]
        L.mijpeg_host_alloc.restype = C.c_void_p
        L.mijpeg_host_free.argtypes = [C.c_void_p]
        L.mijpeg_host_free.restype = None
        L.mijpeg_last_error.argtypes = [C.c_void_p, P(C.c_char_p)]
        L.mijpeg_alpha_channel.argtypes = [C.c_void_p]
        L.mijpeg_alpha_channel.restype = C.c_void_p
        L.mijpeg_has_alpha.argtypes = [C.c_void_p]
        L.mijpeg_batch_pipeline_create.argtypes = [P(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]
        L.mijpeg_batch_pipeline_destroy.argtypes = [C.c_void_p]
        L.mijpeg_batch_pipeline_destroy.restype = None
        L.mijpeg_batch_pipeline_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.mijpeg_batch_pipeline_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.mijpeg_batch_pipeline_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mijpeg_batch_pipeline_last_error.argtypes = [C.c_void_p, P(C.c_char_p)]
        L.mijpeg_batch_pipeline_speculation.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_batch_pipeline_decoder.argtypes = [C.c_void_p, C.c_int]
        L.mijpeg_batch_pipeline_decoder.restype = C.c_void_p
        L.mijpeg_alpha_info.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int32)]
        L.mijpeg_last_timing.argtypes = [C.c_void_p, P(C.c_double)]
        L.mijpeg_launch_reconstruct.argtypes = [P(MijpegBatch), C.c_void_p]
        L.mijpeg_kernel_name.argtypes = [P(MijpegBatch)]
        L.mijpeg_kernel_name.restype = C.c_char_p
        L.mijpeg_workspace_bytes.argtypes = [P(MijpegBatch)]
        L.mijpeg_workspace_bytes.restype = C.c_size_t
        _lib = L
    return _lib


def _foreign_work_done() -> None:
    """The decoder object works on a stream of its own (non-blocking): device buffers handed to it must not have work
    pending on other streams -- a torch fill queued a moment ago, say (include/mijpeg.h states the requirement).  These
    bindings are the tests' and bench.py's: they simply wait for torch's streams."""
    t = sys.modules.get("torch")
    if t is not None and t.cuda.is_available():
        t.cuda.synchronize()


class Decoder:
    """One image at a time.  device=None -> host-only object (parsing + Huffman decoding)."""

    def __init__(self, device: int | None = 0):
        self._h = C.c_void_p()
        rc = lib().mijpeg_create(C.byref(self._h), -1 if device is None else int(device))
        if rc:
            raise MijpegError(rc, "mijpeg_create failed (no usable HIP device?)")
        self._data = None
        self.info: MijpegInfo | None = None

    def close(self):
        # the alpha decoders handed out are owned by this object's handle: they die with it
        for ref in getattr(self, "_children", ()):
            child = ref()
            if child is not None:
                child._h = C.c_void_p()
        self._children = []
        if self._h:
            if not getattr(self, "_borrowed", False):
                lib().mijpeg_destroy(self._h)
            self._h = C.c_void_p()

    def alpha_channel(self) -> "Decoder | None":
        """The decoder object of the file's alpha channel (JPEG XT ALFA box), owned by this one and valid until it reads again; None
        when the decoded file has none.  Its `info` is the alpha image's (one component)."""
        h = lib().mijpeg_alpha_channel(self._h)
        if not h:
            return None
        a = Decoder.__new__(Decoder)
        a._h = C.c_void_p(h)
        a._borrowed = True
        a._data = None
        a._owner = self  # keep the owning object alive
        if not hasattr(self, "_children"):
            self._children = []
        self._children.append(weakref.ref(a))
        a.info = MijpegInfo()
        a._check(lib().mijpeg_get_info(a._h, C.byref(a.info)))
        return a

    def alpha_info(self):
        """-> (mode, (r, g, b)): compositing method and matte colour of the alpha merging specification's AMUL box (mode -1: none)."""
        mode = C.c_int32(-1)
        matte = (C.c_int32 * 3)()
        self._check(lib().mijpeg_alpha_info(self._h, C.byref(mode), matte))
        return mode.value, tuple(matte)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            if not self._h:
                raise MijpegError(rc, "the decoder object is closed")
            msg = C.c_char_p()
            lib().mijpeg_last_error(self._h, C.byref(msg))
            raise MijpegError(rc, (msg.value or b"").decode())

    def _stats(self, struct, getter, leave_out=()) -> dict:
        """A statistics struct filled by its getter, as a dict of its integer fields without those in leave_out."""
        st = struct()
        self._check(getter(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in struct._fields_ if k not in leave_out}

    def _ragged_lengths(self, destinations, row_strides, rects=None) -> int:
        """The list calls' length check: one destination and row stride (and crop) per image of the ragged batch -> that many."""
        n, images = len(destinations), getattr(self, "ragged_images", -1)
        if n != images or len(row_strides) != n or (rects is not None and len(rects) != n):
            crops = f"{len(rects)} crops, " if rects is not None else ""
            raise ValueError(f"{crops}{n} destinations and {len(row_strides)} row strides for the {max(images, 0)} images of the ragged batch")
        return n

    @staticmethod
    def _pointer_table(ptrs, planar: bool):
        """The flat c_void_p array of a list call: one pointer per picture, or -- planar -- its plane pointers padded to 4; 0 / None /
        empty: skipped."""
        if not planar:
            return (C.c_void_p * len(ptrs))(*[p or None for p in ptrs])
        flat = []
        for p in ptrs:
            p = list(p or [])
            flat += [q or None for q in p] + [None] * (4 - len(p))
        return (C.c_void_p * (4 * len(ptrs)))(*flat)

    def _ragged_call(self, fn, rects, ptrs, planar: bool, row_strides, flags: int, sync: bool, wait_foreign: bool) -> None:
        """A list reconstruction call of the library: fn(handle, [crops,] destinations, row strides, flags, sync)."""
        n = self._ragged_lengths(ptrs, row_strides, rects)
        if wait_foreign:
            _foreign_work_done()
        crops = () if rects is None else (rect_array(rects),)
        self._check(fn(self._h, *crops, self._pointer_table(ptrs, planar), (C.c_int64 * n)(*row_strides), flags, 1 if sync else 0))

    def read_header(self, data: bytes) -> MijpegInfo:
        """Tables + frame header (JPEG::Read up to the first scan, then JPEG::GetInformation)."""
        self._data = data  # keep alive: the library borrows the bytes
        self._check(lib().mijpeg_set_input(self._h, data, len(data)))
        info = MijpegInfo()
        self._check(lib().mijpeg_read_header(self._h, C.byref(info)))
        self.info = info
        return info

    def read(self, data: bytes, threads: int = 0, entropy: str = "host") -> MijpegInfo:
        """JPEG::Read: parse everything and entropy-decode all scans (uploads when a device is attached).
        entropy = "host" (restart-interval parallel on the CPU), "gpu" (on the device, error if the stream does not
        qualify), "auto" (device when it qualifies and has enough restart intervals to occupy it) or "prefer-gpu" (device
        whenever it qualifies, however small; host otherwise -- damaged streams always end up there)."""
        self._data = data
        self._check(lib().mijpeg_set_input(self._h, data, len(data)))
        self.entropy_used = "host"
        if entropy in ("gpu", "auto", "prefer-gpu"):
            rc = lib().mijpeg_decode_coefficients_device(self._h, 0 if entropy == "auto" else 1)
            if rc == 0:
                self.entropy_used = "gpu"
            elif rc != ERR_NOT_AVAILABLE or entropy == "gpu":
                self._check(rc)
                raise MijpegError(rc, "stream does not qualify for on-device entropy decoding")
        if self.entropy_used == "host":
            self._check(lib().mijpeg_decode_coefficients(self._h, threads))
        info = MijpegInfo()
        self._check(lib().mijpeg_get_info(self._h, C.byref(info)))
        self.info = info
        return info

    def device_walk_rounds(self) -> int:
        """Rounds the on-device self-synchronising walk took in the last device entropy decode (0 = none needed)."""
        return int(lib().mijpeg_device_walk_rounds(self._h))

    def encode(self, img: np.ndarray, quality: int = 85, subsampling: str = "444", restart_mcus: int = 0, optimize: bool = False,
               coder: str = "gpu") -> bytes:
        """mijpeg_encode_image_ex: (H, W, 3) RGB or (H, W) grey uint8 picture -> baseline JPEG; forward transform on the device,
        entropy coder on the device (coder="gpu") or on the host cores (coder="host").  A uint16 picture (samples 0..4095) goes
        through mijpeg_encode_image16 -> extended sequential 12-bit JPEG; its Huffman tables are always the picture's own."""
        if np.asarray(img).dtype == np.uint16:
            return self._encode16(np.ascontiguousarray(img), quality, subsampling, restart_mcus, coder)
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        nc = 1 if img.ndim == 2 else img.shape[2]
        hs, vs = {"444": ((1, 1, 1), (1, 1, 1)), "420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "440": ((1, 1, 1), (2, 1, 1)),
                  "411": ((4, 1, 1), (1, 1, 1))}[subsampling]
        L = lib()
        L.mijpeg_encode_image_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mijpeg_free.argtypes = [C.c_void_p]
        p, n = C.c_void_p(), C.c_size_t()
        self._check(L.mijpeg_encode_image_ex(self._h, img.ctypes.data, w, h, nc, w * nc, quality, (C.c_int32 * 4)(*hs, 1), (C.c_int32 * 4)(*vs, 1),
                                             restart_mcus, 1 if optimize else 0, 1 if coder == "host" else 0, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            L.mijpeg_free(p)

    def _encode16(self, img: np.ndarray, quality: int, subsampling: str, restart_mcus: int, coder: str, precision: int = 12) -> bytes:
        h, w = img.shape[:2]
        nc = 1 if img.ndim == 2 else img.shape[2]
        hs, vs = ENCODE_LAYOUTS[subsampling] if isinstance(subsampling, str) else subsampling
        L = lib()
        L.mijpeg_encode_image16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mijpeg_free.argtypes = [C.c_void_p]
        p, n = C.c_void_p(), C.c_size_t()
        self._check(L.mijpeg_encode_image16(self._h, img.ctypes.data, w, h, nc, w * nc * 2, precision, quality, (C.c_int32 * 4)(*hs, 1), (C.c_int32 * 4)(*vs, 1),
                                            restart_mcus, 1 if coder == "host" else 0, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            L.mijpeg_free(p)

    def encode_batch_device(self, info: MijpegInfo, pixels_dev: int, coef_dev: int, frames: int, pixel_row_stride: int, pixel_frame_stride: int,
                            restart_mcus: int = 0, optimize: bool = False):
        """mijpeg_encode_batch_device: frames resident in HBM -> list of baseline JPEG streams (forward kernels + device entropy coder).
        info.precision == 12 (frame_layout(..., precision=12)): pixels_dev holds uint16 samples, the streams are extended sequential."""
        _foreign_work_done()
        b = MijpegForwardBatch()
        C.memmove(C.byref(b.info), C.byref(info), C.sizeof(MijpegInfo))
        b.pixels_dev, b.pixel_frame_stride, b.pixel_row_stride = pixels_dev, pixel_frame_stride, pixel_row_stride
        b.coef_dev, b.coef_frame_stride, b.frames = coef_dev, info.coef_count, frames
        L = lib()
        L.mijpeg_encode_batch_device.argtypes = [C.c_void_p, C.POINTER(MijpegForwardBatch), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mijpeg_free.argtypes = [C.c_void_p]
        ptrs, sizes = (C.c_void_p * frames)(), (C.c_size_t * frames)()
        self._check(L.mijpeg_encode_batch_device(self._h, C.byref(b), restart_mcus, 1 if optimize else 0, ptrs, sizes))
        out = []
        for f in range(frames):
            out.append(C.string_at(ptrs[f], sizes[f]))
            L.mijpeg_free(ptrs[f])
        return out

    def encode_coefficients_device(self, info: MijpegInfo, coef_dev: int, restart_interval: int = 0, optimize: bool = False) -> bytes:
        """mijpeg_encode_coefficients_device: quantised coefficient planes resident in HBM (int16, the layout of `info`: what
        device_coefficients() returns after a device entropy decode) -> the stream encode_coefficients writes for the same planes."""
        _foreign_work_done()
        L = lib()
        L.mijpeg_encode_coefficients_device.argtypes = [C.c_void_p, C.POINTER(MijpegInfo), C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                                        C.POINTER(C.c_size_t)]
        L.mijpeg_free.argtypes = [C.c_void_p]
        p, n = C.c_void_p(), C.c_size_t()
        self._check(L.mijpeg_encode_coefficients_device(self._h, C.byref(info), coef_dev, restart_interval, 1 if optimize else 0, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            L.mijpeg_free(p)

    def _encode_ragged(self, fn, frames, optimize: bool, flags: int = 0, precision=None):
        """fn: one of the ragged encode entry points; with `precision` (8 or 12 per picture) its ...16 flavour."""
        n = len(frames)
        arr = (MijpegEncodeFrame * max(n, 1))(*frames)
        ptrs, sizes = (C.c_void_p * max(n, 1))(), (C.c_size_t * max(n, 1))()
        if precision is None:
            self._check(fn(self._h, arr, n, 1 if optimize else 0, flags, ptrs, sizes))
        else:
            self._check(fn(self._h, arr, _precision_array(precision, n), n, 1 if optimize else 0, flags, ptrs, sizes))
        out = []
        for i in range(n):
            out.append(C.string_at(ptrs[i], sizes[i]))
            lib().mijpeg_free(ptrs[i])
        return out

    def encode_ragged_device(self, frames, optimize: bool = False, precision=None):
        """mijpeg_encode_ragged_device: MijpegEncodeFrame descriptions (api.encode_frame) of pictures resident in HBM -> list of
        baseline JPEG streams, each what `encode` writes for that picture; launches and host waits do not grow with the list.
        precision: 8 or 12 per picture (mijpeg_encode_ragged_device16: a 12-bit picture's pixels are uint16 samples, its row stride
        counts bytes, its stream is extended sequential and its Huffman tables are its own whatever `optimize` says)."""
        _foreign_work_done()
        if precision is None:
            return self._encode_ragged(lib().mijpeg_encode_ragged_device, frames, optimize)
        return self._encode_ragged(lib().mijpeg_encode_ragged_device16, frames, optimize, precision=precision)

    def encode_ragged_planar_device(self, frames, planes, optimize: bool = False, precision=None):
        """mijpeg_encode_ragged_planar_device16: encode_ragged_device for pictures that lie in HBM as component planes.  planes[i]:
        the device addresses of picture i's planes (one for grey, three for colour, anywhere); frames[i].row_stride: the line pitch
        in bytes of every plane of picture i; frames[i].pixels is ignored.  Stream i is what encode_ragged_device writes for the
        interleaved picture with the same samples."""
        _foreign_work_done()
        n = len(frames)
        if len(planes) != n:
            raise ValueError(f"{len(planes)} plane lists for {n} pictures")
        flat = []
        for p in planes:
            p = list(p or [])
            flat += [q or None for q in p[:4]] + [None] * (4 - len(p))
        table = (C.c_void_p * (4 * max(n, 1)))(*flat)
        fn = lambda h, arr, prec, *rest: lib().mijpeg_encode_ragged_planar_device16(h, arr, table, prec, *rest)
        return self._encode_ragged(fn, frames, optimize, precision=precision if precision is not None else [8] * n)

    def encode_planar_stats(self) -> dict:
        """What the object's last planar encode did (mijpeg_encode_planar_stats)."""
        return self._stats(MijpegEncodePlanarStats, lib().mijpeg_encode_planar_stats_get, {"reserved"})

    def interleave_device(self, plane_ptrs, plane_row_stride: int, width: int, height: int, components: int, sample_bytes: int, dst_ptr: int,
                          dst_row_stride: int, sync: bool = True):
        """mijpeg_interleave_device: planes in device memory -> an interleaved picture, on the object's stream."""
        ptrs = list(plane_ptrs) + [None] * (4 - len(plane_ptrs))
        src = (C.c_void_p * 4)(*[p or None for p in ptrs])
        self._check(lib().mijpeg_interleave_device(self._h, src, plane_row_stride, width, height, components, sample_bytes, dst_ptr, dst_row_stride,
                                                   1 if sync else 0))

    def encode_ragged(self, images, quality=85, subsampling="444", restart_mcus=0, optimize: bool = False):
        """mijpeg_encode_ragged16: (H, W, 3) / (H, W) arrays in host memory -> list of JPEG streams.  uint16 arrays are 12-bit
        pictures (samples 0..4095 -> extended sequential streams), everything else is taken as uint8 (-> baseline streams); both
        may appear in one list.  quality, subsampling (a name of ENCODE_LAYOUTS) and restart_mcus: one value for all or a list
        with one per picture."""
        imgs = [np.ascontiguousarray(im, np.uint16 if np.asarray(im).dtype == np.uint16 else np.uint8) for im in images]
        per = lambda v, i: v[i] if isinstance(v, (list, tuple)) else v
        frames = []
        for i, im in enumerate(imgs):
            nc = 1 if im.ndim == 2 or im.shape[2] == 1 else im.shape[2]
            frames.append(encode_frame(im.shape[1], im.shape[0], nc, per(quality, i), per(subsampling, i), per(restart_mcus, i), im.ctypes.data,
                                       im.shape[1] * nc * im.itemsize))
        return self._encode_ragged(lib().mijpeg_encode_ragged16, frames, optimize, precision=[12 if im.itemsize == 2 else 8 for im in imgs])

    def encode_ragged_stats(self) -> dict:
        return self._stats(MijpegEncodeRaggedStats, lib().mijpeg_encode_ragged_get_stats, {"reserved"})

    def transcode_ragged_device(self, specs=None, optimize: bool = False, transforms=None):
        """mijpeg_transcode_ragged_device: the pictures of the last decode_ragged_device call coded again from their quantised planes in
        HBM.  specs: None (keep every picture's tables and restart interval) or one (quality, restart_interval) per
        picture -- quality 1..100, TRANSCODE_KEEP or TRANSCODE_SKIP; restart_interval 0..65535 or -1 for the source's.
        transforms: None, or one TRANSFORM_* code per picture, TRANSFORM_TRIM OR-ed in where partial MCUs of a mirrored axis are to be
        dropped (mijpeg_transcode_ragged_transformed_device).
        -> (streams, status): bytes or None per picture, and its status code (0 with None: skipped)."""
        n = getattr(self, "ragged_images", 0)
        arr = None
        if transforms is not None:
            transforms = [int(t) for t in transforms]
            if len(transforms) != n:
                raise ValueError(f"{len(transforms)} transforms for the {n} images of the ragged batch")
        if specs is not None:
            specs = list(specs)
            if len(specs) != n:
                raise ValueError(f"{len(specs)} specs for the {n} images of the ragged batch")
            arr = (MijpegTranscodeSpec * max(n, 1))(*[MijpegTranscodeSpec(int(q), int(r)) for q, r in specs])
        ptrs, sizes, status = (C.c_void_p * max(n, 1))(), (C.c_size_t * max(n, 1))(), (C.c_int32 * max(n, 1))()
        if transforms is None:
            self._check(lib().mijpeg_transcode_ragged_device(self._h, arr, 1 if optimize else 0, 0, ptrs, sizes, status))
        else:
            codes = (C.c_int32 * max(n, 1))(*transforms)
            self._check(lib().mijpeg_transcode_ragged_transformed_device(self._h, arr, codes, 1 if optimize else 0, 0, ptrs, sizes, status))
        out = []
        for i in range(n):
            out.append(C.string_at(ptrs[i], sizes[i]) if ptrs[i] else None)
            lib().mijpeg_free(ptrs[i])
        return out, list(status)[:n]

    def transcode_ragged_stats(self) -> dict:
        """What the object's last transcode call did (mijpeg_transcode_ragged_stats)."""
        return self._stats(MijpegTranscodeRaggedStats, lib().mijpeg_transcode_ragged_stats_get)

    def transcode_transform_stats(self) -> dict:
        """What the transforms of the object's last transcode call did (mijpeg_transcode_transform_stats)."""
        return self._stats(MijpegTranscodeTransformStats, lib().mijpeg_transcode_transform_stats_get)

    def xt_params(self) -> MijpegXtParams:
        xt = MijpegXtParams()
        self._check(lib().mijpeg_get_xt_params(self._h, C.byref(xt)))
        return xt

    def coefficients(self, comp: int) -> np.ndarray:
        f = self.info
        wide = bool(f.coef_wide)  # a damaged stream whose coefficients left the 16-bit range: int32 planes
        p = (lib().mijpeg_coefficients32 if wide else lib().mijpeg_coefficients)(self._h, comp)
        if not p:
            raise MijpegError(-1031, "no decoded coefficients")
        n = f.blocks_w[comp] * f.blocks_h[comp] * 64
        arr = np.ctypeslib.as_array(((C.c_int32 if wide else C.c_int16) * n).from_address(p))
        return arr.reshape(f.blocks_h[comp], f.blocks_w[comp], 64).copy()

    def residual_coefficients(self, comp: int) -> np.ndarray:
        """JPEG XT: the residual codestream's planes, which follow the legacy ones in the same coefficient buffer
        (mijpeg_xt_params.residual.coef_offset, in int16 units): int32 when the residual frame has hidden bits."""
        x = self.xt_params()
        base = lib().mijpeg_coefficients(self._h, 0)
        if not base or not self.info.xt:
            raise MijpegError(-1031, "no decoded residual coefficients")
        r = x.residual
        wide = bool(x.residual_wide)
        n = r.blocks_w[comp] * r.blocks_h[comp] * 64
        addr = base + 2 * int(r.coef_offset[comp])
        arr = np.ctypeslib.as_array(((C.c_int32 if wide else C.c_int16) * n).from_address(addr))
        return arr.reshape(r.blocks_h[comp], r.blocks_w[comp], 64).copy()

    def device_coefficients(self) -> int:
        return lib().mijpeg_device_coefficients(self._h) or 0

    def reconstruct(self, flags: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """JPEG::DisplayRectangle over the whole canvas -> (H, W, C) uint8 in host memory."""
        f = self.info
        return self.reconstruct_rect(0, 0, f.width - 1, f.height - 1, flags=flags, out=out)

    def reconstruct_rect(self, x0, y0, x1, y1, comp0=0, comp1=None, flags: int = 0,
                         out: np.ndarray | None = None) -> np.ndarray:
        f = self.info
        nc = f.components
        sb = max(1, f.sample_bytes)  # 2: precision 12 or JPEG XT (16-bit codes)
        comp1 = nc - 1 if comp1 is None else comp1
        if out is None:
            out = np.zeros((f.height, f.width, nc), np.uint8 if sb == 1 else np.uint16)
        base = out.ctypes.data
        dst = (C.c_void_p * 4)(*[base + c * sb if c < nc else None for c in range(4)])
        bpp = (C.c_int32 * 4)(*([nc * sb] * 4))
        bpr = (C.c_int32 * 4)(*([out.strides[0]] * 4))
        self._check(lib().mijpeg_reconstruct_rect(self._h, x0, y0, x1, y1, comp0, comp1, flags, dst, bpp, bpr))
        return out

    def display_rect(self, canvas: np.ndarray, x0, y0, x1, y1, comp0=0, comp1=None, flags: int = 0, bm_height: int | None = None,
                     bm_width=None, device_ptrs=None) -> None:
        """mijpeg_display_rect: one JPEG::DisplayRectangle call of a sequence (the object keeps the reference's state between
        calls).  canvas: (ncomp, H, W) planar uint8 / uint16, written in place; bm_height: BIO_HEIGHT the hook would report;
        bm_width: BIO_WIDTH, one value or one per component (default: the canvas's width).  device_ptrs: per component the device
        address of pixel (0, 0) of a plane laid out like canvas[c] -- the bitmaps live in device memory (MIJPEG_FLAG_DEVICE_OUTPUT)
        and `canvas` only describes them."""
        f = self.info
        nc = f.components
        comp1 = nc - 1 if comp1 is None else comp1
        sb = canvas.dtype.itemsize
        H, W = canvas.shape[1:]
        widths = [W] * nc if bm_width is None else list(bm_width) if np.ndim(bm_width) else [bm_width] * nc
        if device_ptrs is not None:
            _foreign_work_done()
            flags |= FLAG_DEVICE_OUTPUT
        maps = (MijpegBitmap * 4)()
        for c in range(nc):
            maps[c].data = canvas[c].ctypes.data if device_ptrs is None else device_ptrs[c]
            maps[c].bytes_per_pixel = sb
            maps[c].bytes_per_row = canvas.strides[1]
            maps[c].width = widths[c]
            maps[c].height = H if bm_height is None else bm_height
        self._check(lib().mijpeg_display_rect(self._h, x0, y0, x1, y1, comp0, comp1, flags, maps))

    def reconstruct_cli(self, flags: int = 0) -> np.ndarray:
        """What the reference's command line shows of the image (cmd/reconstruct.cpp:272-342 with upsampling): frames of one
        or three components are requested in stripes over all components -- the plain picture --, frames of two or four
        component by component (PGX), where the state JPEG::DisplayRectangle keeps between calls shows (mijpeg_display_rect).
        -> (H, W, C).  Like the reference's loop it can run once per decoded image."""
        f = self.info
        if f.components in (1, 3):
            return self.reconstruct(flags)
        canvas = np.zeros((f.components, f.height, f.width), np.uint8 if max(1, f.sample_bytes) == 1 else np.uint16)
        for c in range(f.components):
            for y in range(0, f.height, 8):
                self.display_rect(canvas, 0, y, f.width - 1, min(y + 7, f.height - 1), c, c, flags, bm_height=y + 8)
        return np.ascontiguousarray(np.moveaxis(canvas, 0, -1))

    def display_plan(self, x0, y0, x1, y1, comp0, comp1, flags: int, bm_height: int):
        """mijpeg_display_plan (no device needed): advance the request state, return the plan as a dict."""
        out = (C.c_int32 * 32)()
        hh = (C.c_uint32 * 4)(bm_height, bm_height, bm_height, bm_height)
        self._check(lib().mijpeg_display_plan(self._h, x0, y0, x1, y1, comp0, comp1, flags, hh, out))
        o = list(out)
        return dict(nothing=o[0], plain=o[1], ycc=o[2], view=o[3], region=tuple(o[4:8]),
                    comps=[dict(cursor=o[8 + 6 * c], g0=o[9 + 6 * c], g1=o[10 + 6 * c], wstart=o[11 + 6 * c], wlimit=o[12 + 6 * c],
                                zeros=o[13 + 6 * c]) for c in range(4)])

    def display_cursor(self, component: int) -> int:
        """mijpeg_display_cursor: the row the cursor of `component` stands at (JPEG XT: 4 + c = the residual image's)."""
        return int(lib().mijpeg_display_cursor(self._h, component))

    def decode_batch_device(self, streams, min_intervals: int = 0) -> MijpegInfo:
        """mijpeg_decode_batch_device: n streams of one shape -> n coefficient stores in HBM with one Huffman kernel launch."""
        n = len(streams)
        self._batch = list(streams)  # keep the bytes alive during the call
        arr = (C.c_char_p * n)(*self._batch)
        sizes = (C.c_size_t * n)(*[len(s) for s in self._batch])
        self._check(lib().mijpeg_decode_batch_device(self._h, arr, sizes, n, min_intervals))
        info = MijpegInfo()
        self._check(lib().mijpeg_get_info(self._h, C.byref(info)))
        self.info = info
        self.batch_frames = n
        return info

    def prepare_batch_host(self, streams) -> None:
        """mijpeg_prepare_batch_host: the host half of a batch submit alone (no device needed)."""
        n = len(streams)
        arr = (C.c_char_p * n)(*streams)
        sizes = (C.c_size_t * n)(*[len(s) for s in streams])
        L = lib()
        L.mijpeg_prepare_batch_host.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int]
        self._check(L.mijpeg_prepare_batch_host(self._h, arr, sizes, n))

    def set_device_markers(self, on) -> None:
        """mijpeg_set_device_markers: restart marker search and unstuffing of qualifying device decodes on the device (opt-in)."""
        self._check(lib().mijpeg_set_device_markers(self._h, int(on)))

    def device_markers_stats(self):
        """mijpeg_device_markers_stats -> (searched, declined): images of this object that went through the device search, images
        of calls that took the ordinary route although the option was on."""
        a, b = C.c_int64(), C.c_int64()
        self._check(lib().mijpeg_device_markers_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def device_markers_staging(self, image: int):
        """mijpeg_device_markers_staging: the raw segment of image `image` as the last batch call with the option on staged it
        (bytes), or None when that call took the ordinary route."""
        n = C.c_size_t()
        p = lib().mijpeg_device_markers_staging(self._h, image, C.byref(n))
        return C.string_at(p, n.value) if p else None

    def device_marker_search(self, segment: bytes, expect: int, capacity: int | None = None):
        """mijpeg_device_marker_search (diagnostics) -> dict(total, dst, begin, end, term, flags): the search kernels on one raw
        segment; dst holds `capacity` bytes (default: the segment's size + 256)."""
        capacity = len(segment) + 256 if capacity is None else capacity
        dst = np.zeros(capacity, np.uint8)
        begin, end = np.zeros(expect, np.uint32), np.zeros(expect, np.uint32)
        term, flags = C.c_uint32(), C.c_uint32()
        total = lib().mijpeg_device_marker_search(self._h, segment, len(segment), expect, dst.ctypes.data, capacity, begin.ctypes.data, end.ctypes.data,
                                                  C.byref(term), C.byref(flags))
        if total < 0:
            self._check(int(total))
        return dict(total=int(total), dst=dst, begin=begin, end=end, term=term.value, flags=flags.value)

    @staticmethod
    def stream_arrays(streams):
        """(pointer array, size array, list that keeps the bytes alive) for the batch calls: a pipeline builds them once per chunk
        instead of once per call (a hundred microseconds of ctypes per 24 streams, on the thread that feeds the link)."""
        keep = list(streams)
        n = len(keep)
        return (C.c_char_p * n)(*keep), (C.c_size_t * n)(*[len(s) for s in keep]), keep

    def submit_batch_device(self, streams, min_intervals: int = 0, arrays=None) -> None:
        """mijpeg_submit_batch_device: parse, gather, enqueue upload + Huffman kernel; returns without waiting for the device.
        arrays: what stream_arrays(streams) returned (optional)."""
        arr, sizes, self._batch = arrays if arrays is not None else self.stream_arrays(streams)
        n = len(self._batch)
        self._check(lib().mijpeg_submit_batch_device(self._h, arr, sizes, n, min_intervals))
        self.batch_frames = n

    def finish_batch_device(self) -> MijpegInfo:
        """mijpeg_finish_batch_device: wait for a submitted batch, raise what its decode reported."""
        self._check(lib().mijpeg_finish_batch_device(self._h))
        info = MijpegInfo()
        self._check(lib().mijpeg_get_info(self._h, C.byref(info)))
        self.info = info
        return info

    def batch_speculation(self):
        """-> (last validation had to reconstruct again, speculative launches of this object, of them redone): MIJPEG_FLAG_SPECULATIVE"""
        launched, redone = C.c_int64(0), C.c_int64(0)
        again = lib().mijpeg_batch_speculation(self._h, C.byref(launched), C.byref(redone))
        return bool(again == 1), launched.value, redone.value

    def reconstruct_batch_device(self, dst_ptr: int, frame_stride: int, row_stride: int, flags: int = 0, sync: bool = True,
                                 wait_foreign: bool = True):
        """wait_foreign=False: the caller vouches that nothing is pending on other streams for the destination (pipelines that
        must not stall the device between their stages)."""
        if wait_foreign:
            _foreign_work_done()
        self._check(lib().mijpeg_reconstruct_batch_device(self._h, dst_ptr, frame_stride, row_stride, flags, 1 if sync else 0))

    def decode_ragged_device(self, streams, min_intervals: int = 0, with_12bit: bool = False) -> list[int]:
        """mijpeg_decode_ragged_device: n streams of any shapes -> coefficient stores in HBM, one Huffman launch per layout group;
        what the batch kernels do not cover takes the single-image route inside the call.  -> status code per stream (0 = decoded).
        with_12bit: mijpeg_decode_ragged_device16 -- plain 12-bit frames have layout groups of their own instead of taking that route."""
        n = len(streams)
        self._batch = list(streams)
        arr = (C.c_char_p * n)(*self._batch)
        sizes = (C.c_size_t * n)(*[len(s) for s in self._batch])
        status = (C.c_int32 * n)()
        fn = lib().mijpeg_decode_ragged_device16 if with_12bit else lib().mijpeg_decode_ragged_device
        self._check(fn(self._h, arr, sizes, n, min_intervals, status))
        self.ragged_images = n
        return list(status)

    def ragged_info(self, i: int) -> MijpegInfo:
        """Geometry and range check of image i of the last ragged decode (raises the stream's error for one that has none)."""
        info = MijpegInfo()
        self._check(lib().mijpeg_ragged_info(self._h, i, C.byref(info)))
        return info

    def ragged_warning(self, i: int):
        """-> (code, message) the single-image route left for image i, or (0, None)."""
        msg = C.c_char_p()
        code = lib().mijpeg_ragged_warning(self._h, i, C.byref(msg))
        return code, (msg.value.decode() if msg.value else None)

    def ragged_route(self, i: int):
        """-> (True, None) when image i was decoded by its layout group's launch, (False, reason) for the single-image route."""
        why = C.c_char_p()
        rc = lib().mijpeg_ragged_route(self._h, i, C.byref(why))
        if rc < 0:
            self._check(rc)
        return rc == 0, (why.value.decode() if why.value else None)

    def reconstruct_ragged_device(self, dst_ptrs, row_strides, flags: int = 0, sync: bool = True, wait_foreign: bool = True):
        """mijpeg_reconstruct_ragged_device: image i -> dst_ptrs[i] (0 / None: skipped) with row_strides[i] bytes per line; one entry
        per stream of the decode call (the library walks that many)."""
        self._ragged_call(lib().mijpeg_reconstruct_ragged_device, None, dst_ptrs, False, row_strides, flags, sync, wait_foreign)

    def ragged_stats(self) -> dict:
        return self._stats(MijpegRaggedStats, lib().mijpeg_ragged_get_stats)

    # ---- planar output: component planes instead of interleaved pixels (include/mijpeg.h)
    def reconstruct_planar_device(self, plane_ptrs, row_stride: int, flags: int = 0, sync: bool = True):
        """mijpeg_reconstruct_planar_device: component c of the decoded picture -> plane_ptrs[c], row_stride bytes per plane line."""
        _foreign_work_done()
        ptrs = list(plane_ptrs) + [None] * (4 - len(plane_ptrs))
        dst = (C.c_void_p * 4)(*[p or None for p in ptrs])
        self._check(lib().mijpeg_reconstruct_planar_device(self._h, dst, row_stride, flags, 1 if sync else 0))

    def reconstruct_batch_planar_device(self, dst_ptr: int, frame_stride: int, plane_stride: int, row_stride: int, flags: int = 0,
                                        sync: bool = True, wait_foreign: bool = True):
        """mijpeg_reconstruct_batch_planar_device: the decoded uniform batch as (N, C, H, W) with the given strides in bytes."""
        if wait_foreign:
            _foreign_work_done()
        self._check(lib().mijpeg_reconstruct_batch_planar_device(self._h, dst_ptr, frame_stride, plane_stride, row_stride, flags, 1 if sync else 0))

    def reconstruct_ragged_planar_device(self, plane_ptrs, row_strides, flags: int = 0, sync: bool = True, wait_foreign: bool = True):
        """mijpeg_reconstruct_ragged_planar_device: plane_ptrs[i] = the plane addresses of image i (None / empty: skipped), one entry
        per stream of the decode call; row_strides[i] bytes per line of its planes."""
        self._ragged_call(lib().mijpeg_reconstruct_ragged_planar_device, None, plane_ptrs, True, row_strides, flags, sync, wait_foreign)

    # ---- crop windows of a ragged batch (include/mijpeg.h)
    def reconstruct_ragged_rect_device(self, rects, dst_ptrs, row_strides, flags: int = 0, sync: bool = True, wait_foreign: bool = True):
        """mijpeg_reconstruct_ragged_rect_device: pixel (min_x, min_y) of image i -> dst_ptrs[i] (0 / None: skipped), row_strides[i] bytes
        per line of the crop.  rects[i]: (min_x, min_y, max_x, max_y), inclusive; max beyond the picture is clipped (RECT_TO_EDGE)."""
        self._ragged_call(lib().mijpeg_reconstruct_ragged_rect_device, rects, dst_ptrs, False, row_strides, flags, sync, wait_foreign)

    def reconstruct_ragged_rect_planar_device(self, rects, plane_ptrs, row_strides, flags: int = 0, sync: bool = True, wait_foreign: bool = True):
        """mijpeg_reconstruct_ragged_rect_planar_device: sample (min_x, min_y) of component c of image i -> plane_ptrs[i][c] (None /
        empty: the image is skipped), row_strides[i] bytes per line of every plane of the crop."""
        self._ragged_call(lib().mijpeg_reconstruct_ragged_rect_planar_device, rects, plane_ptrs, True, row_strides, flags, sync, wait_foreign)

    def ragged_rect_stats(self) -> dict:
        """What the object's last crop call did (mijpeg_ragged_rect_stats)."""
        return self._stats(MijpegRaggedRectStats, lib().mijpeg_ragged_rect_stats_get)

    # ---- crops resized into one batch tensor (include/mijpeg.h)
    def reconstruct_ragged_resized_device(self, rects, out_width: int, out_height: int, channels: int, dst_ptr: int, image_stride: int, plane_stride: int,
                                          row_stride: int, flags: int = 0, sync: bool = True, wait_foreign: bool = True) -> list[int]:
        """mijpeg_reconstruct_ragged_resized_device: the crop rects[i] (None: whole pictures; (min_x, min_y, max_x, max_y), inclusive) of
        picture i of the last ragged decode, resized to out_width x out_height, into slot i at dst_ptr + i * image_stride; planar with
        plane_stride != 0, interleaved with 0.  -> status per picture: 0 = served, its decode status, or ERR_NOT_IMPLEMENTED."""
        n = getattr(self, "ragged_images", 0)
        if rects is not None and len(rects) != n:
            raise ValueError(f"{len(rects)} crops for the {n} images of the ragged batch")
        if wait_foreign:
            _foreign_work_done()
        status = (C.c_int32 * max(1, n))()
        self._check(lib().mijpeg_reconstruct_ragged_resized_device(self._h, rect_array(rects) if rects is not None else None, out_width, out_height, channels,
                                                                   dst_ptr or None, image_stride, plane_stride, row_stride, flags, status, 1 if sync else 0))
        return list(status)[:n]

    def ragged_resized_stats(self) -> dict:
        """What the object's last resized call did (mijpeg_ragged_resized_stats)."""
        return self._stats(MijpegRaggedResizedStats, lib().mijpeg_ragged_resized_stats_get, {"reserved"})

    # ---- ... as a normalised float batch, mirrored per picture (include/mijpeg.h)
    def reconstruct_ragged_normalized_device(self, rects, out_width: int, out_height: int, channels: int, sample: int, scale, bias, mirror, dst_ptr: int,
                                             image_stride: int, plane_stride: int, row_stride: int, flags: int = 0, sync: bool = True,
                                             wait_foreign: bool = True) -> list[int]:
        """mijpeg_reconstruct_ragged_normalized_device: the resized call with `sample` (SAMPLE_U8 / F32 / F16 / BF16) elements; a float
        element of channel c is fl32(fl32(v * scale[c]) + bias[c]) of the 8-bit sample v the resized call writes (scale, bias: up to three
        numbers, or None with SAMPLE_U8).  mirror: None or one truth value per picture of the ragged batch -- that slot's lines reversed.
        Strides are in BYTES and multiples of the element size.  -> status per picture, as the resized call gives it."""
        n = getattr(self, "ragged_images", 0)
        if rects is not None and len(rects) != n:
            raise ValueError(f"{len(rects)} crops for the {n} images of the ragged batch")
        if mirror is not None and len(mirror) != n:
            raise ValueError(f"{len(mirror)} mirror flags for the {n} images of the ragged batch")
        fmt = MijpegBatchFormat()
        fmt.sample = int(sample)
        for k, v in enumerate(list(scale or ())[:3]):
            fmt.scale[k] = v
        for k, v in enumerate(list(bias or ())[:3]):
            fmt.bias[k] = v
        flags_array = (C.c_uint8 * max(1, n))(*[1 if m else 0 for m in mirror]) if mirror is not None else None  # (alive until the call returns)
        fmt.mirror = C.cast(flags_array, C.c_void_p) if flags_array is not None else None
        if wait_foreign:
            _foreign_work_done()
        status = (C.c_int32 * max(1, n))()
        self._check(lib().mijpeg_reconstruct_ragged_normalized_device(self._h, rect_array(rects) if rects is not None else None, out_width, out_height, channels,
                                                                      C.byref(fmt), dst_ptr or None, image_stride, plane_stride, row_stride, flags, status,
                                                                      1 if sync else 0))
        return list(status)[:n]

    def ragged_normalized_stats(self) -> dict:
        """Sample type and mirrored pictures of the object's last resized or normalised call (mijpeg_ragged_normalized_stats)."""
        return self._stats(MijpegRaggedNormalizedStats, lib().mijpeg_ragged_normalized_stats_get, {"reserved"})

    def deinterleave_device(self, src_ptr: int, src_row_stride: int, width: int, height: int, components: int, sample_bytes: int, plane_ptrs,
                            row_stride: int):
        """mijpeg_deinterleave_device: an interleaved picture in device memory -> its planes, on the object's stream (no wait)."""
        ptrs = list(plane_ptrs) + [None] * (4 - len(plane_ptrs))
        dst = (C.c_void_p * 4)(*[p or None for p in ptrs])
        self._check(lib().mijpeg_deinterleave_device(self._h, src_ptr, src_row_stride, width, height, components, sample_bytes, dst, row_stride))

    def planar_stats(self) -> dict:
        """What the object's last planar call did (mijpeg_planar_stats)."""
        return self._stats(MijpegPlanarStats, lib().mijpeg_planar_stats_get)

    def reconstruct_unsampled(self, comp: int, flags: int = 0) -> np.ndarray:
        """JPGTAG_DECODER_UPSAMPLE = false: component `comp` on its own sample grid, no colour transformation
        (what the reference CLI's -U writes into out_<comp>.raw)."""
        f = self.info
        sb = max(1, f.sample_bytes)
        w, h = -(-f.width // f.subx[comp]), -(-f.height // f.suby[comp])
        out = np.zeros((h, w), np.uint8 if sb == 1 else np.uint16)
        dst = (C.c_void_p * 4)(*[out.ctypes.data if c == comp else None for c in range(4)])
        bpp = (C.c_int32 * 4)(*([sb] * 4))
        bpr = (C.c_int32 * 4)(*([out.strides[0]] * 4))
        self._check(lib().mijpeg_reconstruct_rect(self._h, 0, 0, f.width - 1, f.height - 1, comp, comp,
                                                  flags | FLAG_NO_UPSAMPLING, dst, bpp, bpr))
        return out

    def reconstruct_rect_device(self, x0, y0, x1, y1, ptrs, bytes_per_pixel, bytes_per_row, comp0=0, comp1=None,
                                flags: int = 0):
        """mijpeg_reconstruct_rect with MIJPEG_FLAG_DEVICE_OUTPUT: `ptrs[c]` is the device address of canvas pixel
        (0,0) of component c (0/None = component not wanted), strides in bytes as in the reference's ImageBitMap."""
        _foreign_work_done()
        nc = self.info.components
        comp1 = nc - 1 if comp1 is None else comp1
        ptrs = list(ptrs) + [None] * (4 - len(ptrs))
        dst = (C.c_void_p * 4)(*[p or None for p in ptrs])
        bpp = (C.c_int32 * 4)(*(list(bytes_per_pixel) + [0] * (4 - len(bytes_per_pixel))))
        bpr = (C.c_int32 * 4)(*(list(bytes_per_row) + [0] * (4 - len(bytes_per_row))))
        self._check(lib().mijpeg_reconstruct_rect(self._h, x0, y0, x1, y1, comp0, comp1, flags | FLAG_DEVICE_OUTPUT,
                                                  dst, bpp, bpr))

    def reconstruct_into(self, out: np.ndarray, flags: int = 0) -> np.ndarray:
        """Whole frame with the device-to-host copy landing directly in `out` (fast when `out` is pinned, see
        pinned_frame()); `out` is (H, W, C) with contiguous pixels, any row stride."""
        self._check(lib().mijpeg_reconstruct_host(self._h, out.ctypes.data, out.strides[0], flags))
        return out

    def reconstruct_device(self, dst_ptr: int, row_stride: int, flags: int = 0, sync: bool = True):
        _foreign_work_done()
        self._check(lib().mijpeg_reconstruct_device(self._h, dst_ptr, row_stride, flags, 1 if sync else 0))

    def last_warning(self):
        """JPEG::LastWarning: (code, message) -- (0, None) when the reference would not warn."""
        L = lib()
        L.mijpeg_last_warning.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
        msg = C.c_char_p()
        code = L.mijpeg_last_warning(self._h, C.byref(msg))
        return code, (msg.value.decode() if msg.value else None)

    def synchronize(self):
        """Wait for everything this object has enqueued on its stream (mijpeg_finish_batch_device is the batch flavour;
        a reconstruction launched with sync=False is waited for by the next synchronous call on the object: this one)."""
        L = lib()
        L.mijpeg_synchronize.argtypes = [C.c_void_p]
        self._check(L.mijpeg_synchronize(self._h))

    def stream_wait(self, client_stream: int = 0):
        """Everything this object has enqueued so far happens before what the caller enqueues on `client_stream` (a hipStream_t as
        an integer, e.g. torch.cuda.Stream().cuda_stream) from now on; the host does not block (mijpeg_stream_wait)."""
        L = lib()
        L.mijpeg_stream_wait.argtypes = [C.c_void_p, C.c_void_p]
        self._check(L.mijpeg_stream_wait(self._h, C.c_void_p(client_stream)))

    def timing(self):
        t = (C.c_double * 4)()
        lib().mijpeg_last_timing(self._h, t)
        return dict(huffman=t[0], h2d_wait=t[1], kernel=t[2], d2h=t[3])


class PinnedFrame:
    """(H, W, C) frame buffer in pinned host memory (mijpeg_host_alloc); .array is the numpy view."""

    def __init__(self, height: int, width: int, channels: int, dtype=np.uint8):
        line = (width * channels * np.dtype(dtype).itemsize + 7) & ~7
        self._bytes = line * height
        self._p = lib().mijpeg_host_alloc(self._bytes)
        if not self._p:
            raise MemoryError("mijpeg_host_alloc failed")
        raw = np.ctypeslib.as_array((C.c_uint8 * self._bytes).from_address(self._p)).reshape(height, line)
        self.array = raw[:, :width * channels * np.dtype(dtype).itemsize].view(dtype).reshape(height, width, channels)

    def close(self):
        if self._p:
            self.array = None
            lib().mijpeg_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def speculative_scans():
    """(scans, pieces) decoded by the host's self-synchronising parallel path since the library was loaded."""
    p = C.c_int64(0)
    n = lib().mijpeg_speculative_scans(C.byref(p))
    return int(n), int(p.value)


def trim_cache() -> int:
    """Free the buffers destroyed decoder objects left in the process-wide cache; returns the bytes freed."""
    L = lib()
    L.mijpeg_trim_cache.restype = C.c_size_t
    return int(L.mijpeg_trim_cache())


def default_threads() -> int:
    L = lib()
    L.mijpeg_default_threads.restype = C.c_int
    return int(L.mijpeg_default_threads())


def decode(data: bytes, device: int = 0, threads: int = 0, flags: int = 0) -> np.ndarray:
    """`jpeg in.jpg out.ppm` in one call: bytes -> (H, W, C) uint8."""
    d = Decoder(device)
    try:
        d.read(data, threads)
        return d.reconstruct(flags)
    finally:
        d.close()


def launch_reconstruct(info: MijpegInfo, coef_dev: int, out_dev: int, frames: int, out_row_stride: int,
                       out_frame_stride: int, coef_frame_stride: int | None = None, flags: int = 0,
                       workspace: int = 0, workspace_bytes: int = 0, stream: int = 0, xt: MijpegXtParams | None = None,
                       quant_dev: int = 0) -> None:
    """Stateless batch launch (device-resident coefficients -> device pixels), asynchronous.  quant_dev: device address of
    per-frame tables, u16 [frames][4][64] (component, natural order); info.quant then holds the batch-wide maxima."""
    b = MijpegBatch()
    C.memmove(C.byref(b.info), C.byref(info), C.sizeof(MijpegInfo))
    b.coef_dev = coef_dev
    b.coef_frame_stride = info.coef_count if coef_frame_stride is None else coef_frame_stride
    b.out_dev = out_dev
    b.out_frame_stride = out_frame_stride
    b.out_row_stride = out_row_stride
    b.frames = frames
    b.flags = flags
    b.workspace = workspace
    b.workspace_bytes = workspace_bytes
    b.quant_dev = quant_dev or None
    if xt is not None:
        b.xt = C.pointer(xt)
    rc = lib().mijpeg_launch_reconstruct(C.byref(b), stream)
    if rc:
        raise MijpegError(rc, "mijpeg_launch_reconstruct failed")


def frame_layout(width: int, height: int, components: int, hsamp, vsamp, quant, quant_index=None, ycbcr: int = 1, precision: int = 8) -> MijpegInfo:
    """mijpeg_frame_layout: geometry of a frame to be coded (encoder direction).  quant: up to four tables of 64 deltas,
    natural order; quant_index[c]: table of component c (default 0 for the first, 1 for the others)."""
    f = MijpegInfo()
    f.width, f.height, f.components, f.precision, f.ycbcr = width, height, components, precision, ycbcr
    for c in range(components):
        f.hsamp[c], f.vsamp[c] = hsamp[c], vsamp[c]
        f.quant_index[c] = (0 if c == 0 else min(1, len(quant) - 1)) if quant_index is None else quant_index[c]
    for t, tab in enumerate(quant):
        for i in range(64):
            f.quant[t][i] = int(tab[i])
    L = lib()
    L.mijpeg_frame_layout.argtypes = [C.POINTER(MijpegInfo)]
    rc = L.mijpeg_frame_layout(C.byref(f))
    if rc:
        raise MijpegError(rc, "mijpeg_frame_layout failed")
    return f


def launch_forward(info: MijpegInfo, pixels_dev: int, coef_dev: int, frames: int, pixel_row_stride: int, pixel_frame_stride: int,
                   coef_frame_stride: int | None = None, stream: int = 0) -> None:
    """Encoder direction, stateless: device-resident interleaved pixels -> quantised coefficient planes in HBM (asynchronous)."""
    b = MijpegForwardBatch()
    C.memmove(C.byref(b.info), C.byref(info), C.sizeof(MijpegInfo))
    b.pixels_dev = pixels_dev
    b.pixel_frame_stride = pixel_frame_stride
    b.pixel_row_stride = pixel_row_stride
    b.coef_dev = coef_dev
    b.coef_frame_stride = info.coef_count if coef_frame_stride is None else coef_frame_stride
    b.frames = frames
    L = lib()
    L.mijpeg_launch_forward.argtypes = [C.POINTER(MijpegForwardBatch), C.c_void_p]
    rc = L.mijpeg_launch_forward(C.byref(b), stream)
    if rc:
        raise MijpegError(rc, "mijpeg_launch_forward failed")


def encode_coefficients(info: MijpegInfo, coef: np.ndarray, restart_interval: int = 0, optimize: bool = False, threads: int = 0) -> bytes:
    """mijpeg_encode_coefficients: quantised coefficient planes (host int16, info.coef_count of them) -> baseline JPEG stream."""
    coef = np.ascontiguousarray(coef, np.int16).reshape(-1)
    assert coef.size == info.coef_count
    L = lib()
    L.mijpeg_encode_coefficients.argtypes = [C.POINTER(MijpegInfo), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mijpeg_free.argtypes = [C.c_void_p]
    p, n = C.c_void_p(), C.c_size_t()
    rc = L.mijpeg_encode_coefficients(C.byref(info), coef.ctypes.data, restart_interval, 1 if optimize else 0, threads, C.byref(p), C.byref(n))
    if rc:
        raise MijpegError(rc, "mijpeg_encode_coefficients failed")
    try:
        return C.string_at(p, n.value)
    finally:
        L.mijpeg_free(p)


def transcode_plan(source: MijpegInfo, quality: int = TRANSCODE_KEEP, restart_interval: int = -1):
    """mijpeg_transcode_plan (no device): a decoded picture's frame + spec -> (status, output MijpegInfo, restart interval, kept).
    status is the picture's refusal or 0; the output frame is zeroed on a refusal and for TRANSCODE_SKIP."""
    spec, out, ri, kept = MijpegTranscodeSpec(int(quality), int(restart_interval)), MijpegInfo(), C.c_int32(), C.c_int32()
    rc = lib().mijpeg_transcode_plan(C.byref(source), C.byref(spec), C.byref(out), C.byref(ri), C.byref(kept))
    return rc, out, ri.value, bool(kept.value)


def transcode_plan_transformed(source: MijpegInfo, quality: int = TRANSCODE_KEEP, restart_interval: int = -1, transform: int = TRANSFORM_NONE):
    """mijpeg_transcode_plan_transformed (no device): transcode_plan under a TRANSFORM_* code (TRANSFORM_TRIM may be OR-ed in)."""
    spec, out, ri, kept = MijpegTranscodeSpec(int(quality), int(restart_interval)), MijpegInfo(), C.c_int32(), C.c_int32()
    rc = lib().mijpeg_transcode_plan_transformed(C.byref(source), C.byref(spec), int(transform), C.byref(out), C.byref(ri), C.byref(kept))
    return rc, out, ri.value, bool(kept.value)


def transform_blocks(plane: np.ndarray, dst_bh: int, dst_bw: int, transform: int, q_old, q_new, precision: int = 8):
    """mijpeg_transform_blocks, the host twin of transform_list_kernel: one component's plane (blocks_h, blocks_w, 64) int16 under
    table q_old (the source's order) -> ((dst_bh, dst_bw, 64) under q_new (the destination's order), how many values were clamped)."""
    src = np.ascontiguousarray(plane, np.int16)
    dst = np.empty((int(dst_bh), int(dst_bw), 64), np.int16)
    a, b = np.ascontiguousarray(q_old, np.uint16).reshape(64), np.ascontiguousarray(q_new, np.uint16).reshape(64)
    clamped = lib().mijpeg_transform_blocks(src.ctypes.data, src.shape[1], src.shape[0], dst.ctypes.data, int(dst_bw), int(dst_bh), int(transform), a.ctypes.data,
                                            b.ctypes.data, int(precision))
    if clamped < 0:
        raise MijpegError(int(clamped), "mijpeg_transform_blocks failed")
    return dst, int(clamped)


def requantize(blocks: np.ndarray, q_old, q_new, precision: int = 8):
    """mijpeg_requantize, the host twin of requant_list_kernel: (n, 64) int16 coefficients (natural order) under table q_old ->
    (the values under q_new, clamped into the coding range of `precision`; how many were clamped)."""
    src = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64)
    dst = np.empty_like(src)
    a, b = np.ascontiguousarray(q_old, np.uint16).reshape(64), np.ascontiguousarray(q_new, np.uint16).reshape(64)
    clamped = lib().mijpeg_requantize(src.ctypes.data, dst.ctypes.data, src.shape[0], a.ctypes.data, b.ctypes.data, int(precision))
    if clamped < 0:
        raise MijpegError(int(clamped), "mijpeg_requantize failed")
    return dst, int(clamped)


RECT_TO_EDGE = 2**31 - 1  # max_x / max_y of a crop: "to the picture's edge"


def rect_array(rects):
    """(min_x, min_y, max_x, max_y) tuples or MijpegRect -> the array the crop calls take (an array made here passes through: a caller
    that repeats a call converts once -- the conversion of 256 rectangles costs about as much host time as the launch they describe,
    profiles/ragged_rect.txt)."""
    if isinstance(rects, C.Array):
        return rects
    import array
    import itertools

    try:
        flat = array.array("i", itertools.chain.from_iterable((r.min_x, r.min_y, r.max_x, r.max_y) if isinstance(r, MijpegRect) else r for r in rects))
    except (OverflowError, TypeError) as e:
        raise ValueError(f"crop rectangles are four 32-bit integers each: {e}") from None
    if flat.itemsize != 4 or len(flat) != 4 * len(rects):
        raise ValueError("crop rectangles are (min_x, min_y, max_x, max_y)")
    if not rects:
        flat = array.array("i", [0] * 4)
    return (MijpegRect * (len(flat) // 4)).from_buffer(flat)


def resample_taps(n: int, m: int):
    """mijpeg_resample_taps (no device needed): the integer triangle filter's taps for one axis of n source and m output samples ->
    (first, count, weights): int32 arrays of m entries and an int16 array (m, maximal count), zero behind an output's count."""
    cap = lib().mijpeg_resample_taps(n, m, None, None, None, 0)
    if cap < 1:
        raise MijpegError(ERR_INVALID_PARAMETER, f"mijpeg_resample_taps: no taps for {n} -> {m} samples (1 .. 65535 each)")
    first, count, weights = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, cap), np.int16)
    if lib().mijpeg_resample_taps(n, m, first.ctypes.data, count.ctypes.data, weights.ctypes.data, cap) != cap:
        raise MijpegError(ERR_INVALID_PARAMETER, "mijpeg_resample_taps failed")
    return first, count, weights


def ragged_rect_plan(infos, rects):
    """mijpeg_ragged_rect_plan (no device needed): per picture the clipped window in 128 x 128 tiles -> lists tile_x0, tile_y0, tiles_x,
    tiles_y; picture i runs tiles_x[i] * tiles_y[i] workgroups.  Raises MijpegError for a rectangle the crop calls refuse."""
    n = len(infos)
    arr = (MijpegInfo * max(n, 1))()
    for i, f in enumerate(infos):
        C.memmove(C.byref(arr[i]), C.byref(f), C.sizeof(MijpegInfo))
    out = [(C.c_int32 * max(n, 1))() for _ in range(4)]
    rc = lib().mijpeg_ragged_rect_plan(arr, rect_array(rects), n, *out)
    if rc:
        raise MijpegError(rc, "mijpeg_ragged_rect_plan failed")
    return tuple(list(o)[:n] for o in out)


def ragged_plan(infos):
    """mijpeg_ragged_plan (no device needed): frame descriptions -> (group per frame, -1 = single-image route; MijpegRaggedFrame per
    frame; grid of the four layout groups; size of the packed coefficient store)."""
    return _ragged_plan(infos, "mijpeg_ragged_plan", RAGGED_GROUPS)


def ragged_plan16(infos):
    """mijpeg_ragged_plan16: ragged_plan with the 12-bit layout groups (RAGGED_GROUPS16: eight grids)."""
    return _ragged_plan(infos, "mijpeg_ragged_plan16", RAGGED_GROUPS16)


def _ragged_plan(infos, call, groups):
    n = len(infos)
    arr = (MijpegInfo * max(n, 1))()
    for i, f in enumerate(infos):
        C.memmove(C.byref(arr[i]), C.byref(f), C.sizeof(MijpegInfo))
    group = (C.c_int32 * max(n, 1))()
    frames = (MijpegRaggedFrame * max(n, 1))()
    grids = (C.c_int32 * len(groups))()
    total = C.c_int64()
    rc = getattr(lib(), call)(arr, n, group, frames, grids, C.byref(total))
    if rc:
        raise MijpegError(rc, call + " failed")
    return list(group), list(frames), list(grids), total.value


def _precision_array(precision, n: int):
    """The parallel precision array of the ...16 ragged encode calls: one value for all pictures or one per picture."""
    values = [int(precision)] * n if np.ndim(precision) == 0 else [int(p) for p in precision]
    if len(values) != n:
        raise ValueError(f"{len(values)} precisions for {n} pictures")
    return (C.c_int32 * max(n, 1))(*values)


def interleave_device(decoder: "Decoder", plane_ptrs, plane_row_stride: int, width: int, height: int, components: int, sample_bytes: int, dst_ptr: int,
                      dst_row_stride: int, sync: bool = True) -> None:
    """mijpeg_interleave_device on `decoder`'s stream: `components` planes in device memory -> an interleaved picture, the kernel of
    the planar encode's two-pass route on its own (Decoder.interleave_device)."""
    _foreign_work_done()
    decoder.interleave_device(plane_ptrs, plane_row_stride, width, height, components, sample_bytes, dst_ptr, dst_row_stride, sync)


def encode_ragged_plan(frames, pass_blocks: int = 0, precision=None):
    """mijpeg_encode_ragged_plan (no device needed): MijpegEncodeFrame descriptions -> (MijpegEncodeRaggedItem per picture, totals).
    precision: 8 or 12 per picture (mijpeg_encode_ragged_plan16); None: 8-bit pictures."""
    n = len(frames)
    arr = (MijpegEncodeFrame * max(n, 1))(*frames)
    items = (MijpegEncodeRaggedItem * max(n, 1))()
    totals = MijpegEncodeRaggedTotals()
    if precision is None:
        rc = lib().mijpeg_encode_ragged_plan(arr, n, pass_blocks, items, C.byref(totals))
    else:
        rc = lib().mijpeg_encode_ragged_plan16(arr, _precision_array(precision, n), n, pass_blocks, items, C.byref(totals))
    if rc:
        raise MijpegError(rc, "mijpeg_encode_ragged_plan failed")
    return list(items)[:n], totals


def workspace_bytes(info: MijpegInfo, frames: int, flags: int = 0, own_tables: bool = False, xt: "MijpegXtParams | None" = None) -> int:
    b = MijpegBatch()
    C.memmove(C.byref(b.info), C.byref(info), C.sizeof(MijpegInfo))
    b.frames = frames
    b.flags = flags
    if xt is not None:
        b.xt = C.pointer(xt)
    if own_tables:  # only asked whether it is set
        b.quant_dev = 16
    return int(lib().mijpeg_workspace_bytes(C.byref(b)))


def kernel_name(info: MijpegInfo, flags: int = 0, xt: "MijpegXtParams | None" = None) -> str:
    b = MijpegBatch()
    C.memmove(C.byref(b.info), C.byref(info), C.sizeof(MijpegInfo))
    b.flags = flags
    if xt is not None:
        b.xt = C.pointer(xt)
    return lib().mijpeg_kernel_name(C.byref(b)).decode()

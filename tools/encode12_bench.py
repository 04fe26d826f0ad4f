#!/usr/bin/env python3
"""Measurements of the 12-bit encoder direction (profiles/encode12.txt): 8 frames of 8K resident in HBM,

  forward   the forward kernels alone (mijpeg_launch_forward), device events around `--inner` launches
  stream    pixels in HBM -> finished streams in host memory (mijpeg_encode_batch_device), host clock around the call

for 12-bit 4:2:0 and 4:4:4, each against its 8-bit twin of the same build (same picture content scaled, same quantiser tables,
restart interval 8; the 8-bit twin with optimised Huffman tables too, as the 12-bit frames always have them), and -- with --parent
PATH, another build of libmijpeg.so, e.g. of the parent commit -- the 8-bit measurements of this build against that build's.

    python tools/encode12_bench.py [--reps 9] [--frames 8] [--inner 5] [--layouts 420,444] [--parent other/libmijpeg.so]

A and B alternate in one process, `--reps` samples each after a warm-up of both; every figure is the median with minimum and maximum
beside it, one JSON line per pair, the streams' size beside the stream timings (12-bit samples quantised with the tables of the 8-bit
twin leave far more and wider coefficients: the coder's work is the stream's size, not the picture's).  GB/s is algorithmic: the samples read plus the int16 coefficients written (12-bit 4:2:0: 6 + 3
bytes per pixel) over the forward kernels' time; `of_8TBs` is that over 8 TB/s.  There is no CPU fallback: without a device the tool
fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libjpeg_amd import api, synth  # noqa: E402

W, H = 7680, 4320
LAYOUTS = {"420": ((2, 1, 1), (2, 1, 1)), "444": ((1, 1, 1), (1, 1, 1))}
PEAK_BYTES_PER_S = 8e12


class Build:
    """One build of libmijpeg.so, loaded beside any other: the three calls the measurements need."""

    def __init__(self, path):
        import torch  # noqa: F401  (its HIP runtime is the one every build binds to, see api.lib)

        self.path = path
        L = self.L = C.CDLL(path)
        L.mijpeg_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.mijpeg_destroy.argtypes = [C.c_void_p]
        L.mijpeg_destroy.restype = None
        L.mijpeg_free.argtypes = [C.c_void_p]
        L.mijpeg_free.restype = None
        L.mijpeg_launch_forward.argtypes = [C.POINTER(api.MijpegForwardBatch), C.c_void_p]
        L.mijpeg_encode_batch_device.argtypes = [C.c_void_p, C.POINTER(api.MijpegForwardBatch), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        self.h = C.c_void_p()
        if L.mijpeg_create(C.byref(self.h), 0):
            raise SystemExit(f"{path}: mijpeg_create failed (no usable device?)")

    def forward(self, batch, stream):
        if self.L.mijpeg_launch_forward(C.byref(batch), stream):
            raise SystemExit(f"{self.path}: mijpeg_launch_forward failed")

    def streams(self, batch, ri, optimize):
        n = batch.frames
        ptrs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
        if self.L.mijpeg_encode_batch_device(self.h, C.byref(batch), ri, optimize, ptrs, sizes):
            raise SystemExit(f"{self.path}: mijpeg_encode_batch_device failed")
        total = sum(sizes)
        for p in ptrs:
            self.L.mijpeg_free(p)
        return total

    def close(self):
        self.L.mijpeg_destroy(self.h)


def quality_tables(q):
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.mijpeg_quality_tables.restype = None
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    L.mijpeg_quality_tables(q, luma.ctypes.data, chroma.ctypes.data)
    return [luma, chroma]  # (quality 85 has no entry above 255: the 12-bit tables of -q 85 are the same)


def alternate(a, b, reps):
    """a and b in turn, `reps` samples each after one warm-up of both; a sample is what the callable returns (ms)."""
    a(), b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(a())
        tb.append(b())
    return ta, tb


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def inside(x, other):
    return other["min_ms"] <= x["median_ms"] <= other["max_ms"]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--layouts", default="420,444")
    ap.add_argument("--parent", default=None, help="another build of libmijpeg.so to alternate the 8-bit measurements with")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no device: nothing is measured without one")
    F, RI = args.frames, 8
    this = Build(api.LIB_PATH)
    parent = Build(args.parent) if args.parent else None
    quant = quality_tables(85)
    img8 = synth.synth_image(W, H, 1234)
    rng = np.random.default_rng(1234)
    img12 = (img8.astype(np.uint16) << 4) | rng.integers(0, 16, img8.shape, dtype=np.uint16)  # the picture with four more bits of texture
    px8 = torch.from_numpy(img8).cuda().unsqueeze(0).repeat(F, 1, 1, 1).contiguous()
    px12 = torch.from_numpy(img12.view(np.int16)).cuda().unsqueeze(0).repeat(F, 1, 1, 1).contiguous()
    stream = torch.cuda.current_stream()
    for lay in args.layouts.split(","):
        hs, vs = LAYOUTS[lay]
        batches = {}
        for prec, px in ((8, px8), (12, px12)):
            info = api.frame_layout(W, H, 3, hs, vs, quant, quant_index=[0, 0, 0], precision=prec)
            coef = torch.empty((F, int(info.coef_count)), dtype=torch.int16, device="cuda")
            b = api.MijpegForwardBatch()
            C.memmove(C.byref(b.info), C.byref(info), C.sizeof(api.MijpegInfo))
            sb = 2 if prec == 12 else 1  # bytes per sample
            b.pixels_dev, b.pixel_row_stride, b.pixel_frame_stride = px.data_ptr(), W * 3 * sb, H * W * 3 * sb
            b.coef_dev, b.coef_frame_stride, b.frames = coef.data_ptr(), info.coef_count, F
            bpp = 3 * sb + 2.0 * int(info.coef_count) / (W * H)
            batches[prec] = (b, coef, bpp)
        torch.cuda.synchronize()

        def forward_ms(build, prec):
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.inner):
                    build.forward(batches[prec][0], stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / args.inner
            return run

        stream_bytes = {}  # (precision, optimize) -> bytes of the F streams of the last call

        def stream_ms(build, prec, optimize):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stream_bytes[prec, optimize] = build.streams(batches[prec][0], RI, optimize)
                return (time.perf_counter() - t0) * 1e3
            return run

        def report(what, name_a, ta, name_b, tb, bpp_a=None, bpp_b=None, mb_a=None, mb_b=None):
            a, b = summary(ta), summary(tb)
            for s, mb in ((a, mb_a), (b, mb_b)):
                if mb:
                    s["stream_MB_per_frame"] = round(mb / F / 1e6, 2)
            for s, bpp in ((a, bpp_a), (b, bpp_b)):
                if bpp:
                    s["GBs"] = round(W * H * F * bpp / s["median_ms"] / 1e6, 1)
                    s["of_8TBs"] = round(W * H * F * bpp / (s["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 3)
                    s["bytes_per_pixel"] = round(bpp, 2)
            print(json.dumps({"measurement": what, "layout": lay, "frames": F, "reps": args.reps, name_a: a, name_b: b,
                              "ratio": round(b["median_ms"] / a["median_ms"], 3),
                              "each_median_inside_the_others_range": bool(inside(a, b) and inside(b, a))}), flush=True)

        # 12 bits against the 8-bit twin of this build
        ta, tb = alternate(forward_ms(this, 8), forward_ms(this, 12), args.reps)
        report("forward", "p8", ta, "p12", tb, batches[8][2], batches[12][2])
        ta, tb = alternate(stream_ms(this, 8, 1), stream_ms(this, 12, 1), args.reps)
        report("stream, optimised tables", "p8", ta, "p12", tb, mb_a=stream_bytes[8, 1], mb_b=stream_bytes[12, 1])
        # the 8-bit kernels of this build against another build's
        if parent:
            ta, tb = alternate(forward_ms(parent, 8), forward_ms(this, 8), args.reps)
            report("forward, 8 bits", "parent", ta, "this", tb, batches[8][2], batches[8][2])
            ta, tb = alternate(stream_ms(parent, 8, 0), stream_ms(this, 8, 0), args.reps)
            report("stream, 8 bits, Annex K tables", "parent", ta, "this", tb, mb_a=stream_bytes[8, 0], mb_b=stream_bytes[8, 0])
        del batches
    this.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()

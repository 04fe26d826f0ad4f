#!/usr/bin/env python3
"""Measurements of the ragged encode with a precision per picture (profiles/ragged_encode12.txt).  One process, one device.

  a   256 12-bit pictures of 64..1024 pixels a side, 4:2:0, quality 85, with restart interval 4 and without restart markers:
      mijpeg_encode_ragged_device16 (pixels in HBM) and mijpeg_encode_ragged16 (pixels in host memory) against a loop of
      mijpeg_encode_image16 over the same pictures (pixels in host memory: the loop has no other way in)
  b   the same list with the even pictures 8-bit (the loop: mijpeg_encode_image_ex for those)
  c   with --parent PATH, another build of libmijpeg.so (of the parent commit): what existed before, this build against that one --
      the 8-bit list of profiles/ragged_encode.txt (a) through mijpeg_encode_ragged_device, and the uniform forward launches
      (mijpeg_launch_forward, `--frames` frames of 3840 x 2160, 4:2:0) at 8 and at 12 bits, device events around `--inner` launches

    python tools/ragged_encode12_bench.py [--sections a,b,c] [--reps 9] [--pictures 256] [--parent other/libmijpeg.so]

The candidates of a comparison alternate, `--reps` samples each after a warm-up of all; every figure is the median with minimum and
maximum beside it, one JSON line per comparison.  Call times are host clock around a call that ends synchronised.  The streams of the
ragged calls are compared with the loop's before anything is timed.  There is no CPU fallback: without a device the tool fails.
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

from libjpeg_amd import api  # noqa: E402

HS, VS = (2, 1, 1), (2, 1, 1)
QUALITY = 85


class Build:
    """One build of libmijpeg.so, loaded beside any other: the calls the measurements need."""

    def __init__(self, path, new_calls=True):
        import torch  # noqa: F401  (its HIP runtime is the one every build binds to, see api.lib)

        self.path = path
        L = self.L = C.CDLL(path)
        L.mijpeg_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.mijpeg_destroy.argtypes = [C.c_void_p]
        L.mijpeg_destroy.restype = None
        L.mijpeg_free.argtypes = [C.c_void_p]
        L.mijpeg_free.restype = None
        L.mijpeg_launch_forward.argtypes = [C.POINTER(api.MijpegForwardBatch), C.c_void_p]
        L.mijpeg_encode_ragged_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mijpeg_encode_ragged_get_stats.argtypes = [C.c_void_p, C.POINTER(api.MijpegEncodeRaggedStats)]
        L.mijpeg_encode_image_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mijpeg_encode_image16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        if new_calls:
            for fn in (L.mijpeg_encode_ragged_device16, L.mijpeg_encode_ragged16):
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        self.h = C.c_void_p()
        if L.mijpeg_create(C.byref(self.h), 0):
            raise SystemExit(f"{path}: mijpeg_create failed (no usable device?)")

    def _collect(self, ptrs, sizes, keep):
        out = [C.string_at(p, s) for p, s in zip(ptrs, sizes)] if keep else sum(sizes)
        for p in ptrs:
            self.L.mijpeg_free(p)
        return out

    def ragged(self, fn, frames, precision, keep=False):
        """fn: a ragged encode entry point; precision None: one of the 8-bit ones.  Streams (keep) or their total size."""
        n = len(frames)
        ptrs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
        rc = fn(self.h, frames, n, 0, 0, ptrs, sizes) if precision is None else fn(self.h, frames, precision, n, 0, 0, ptrs, sizes)
        if rc:
            raise SystemExit(f"{self.path}: ragged encode failed ({rc})")
        return self._collect(ptrs, sizes, keep)

    def stats(self):
        st = api.MijpegEncodeRaggedStats()
        self.L.mijpeg_encode_ragged_get_stats(self.h, C.byref(st))
        return {k: int(getattr(st, k)) for k in ("passes", "forward_launches", "coder_launches", "host_syncs", "bytes_downloaded")}

    def loop(self, imgs, ri, keep=False):
        """One single-image call per picture: mijpeg_encode_image16 for uint16 samples, mijpeg_encode_image_ex otherwise; flags 0."""
        hs, vs = (C.c_int32 * 4)(*HS, 1), (C.c_int32 * 4)(*VS, 1)
        n = len(imgs)
        ptrs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
        for i, im in enumerate(imgs):
            h, w = im.shape[:2]
            p, s = C.c_void_p(), C.c_size_t()
            if im.dtype == np.uint16:
                rc = self.L.mijpeg_encode_image16(self.h, im.ctypes.data, w, h, 3, w * 6, 12, QUALITY, hs, vs, ri, 0, C.byref(p), C.byref(s))
            else:
                rc = self.L.mijpeg_encode_image_ex(self.h, im.ctypes.data, w, h, 3, w * 3, QUALITY, hs, vs, ri, 0, 0, C.byref(p), C.byref(s))
            if rc:
                raise SystemExit(f"{self.path}: single-image encode failed ({rc})")
            ptrs[i], sizes[i] = p.value, s.value
        return self._collect(ptrs, sizes, keep)

    def forward(self, batch, stream):
        if self.L.mijpeg_launch_forward(C.byref(batch), stream):
            raise SystemExit(f"{self.path}: mijpeg_launch_forward failed")

    def close(self):
        self.L.mijpeg_destroy(self.h)


def pictures(n, seed):
    """n seeded 12-bit pictures of 64..1024 pixels a side in HBM, (h, w, 3) int16 tensors holding 0..4095: smooth content plus
    texture, made on the device."""
    import torch

    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = []
    for _ in range(n):
        w, h = int(rng.integers(64, 1025)), int(rng.integers(64, 1025))
        y = torch.arange(h, device="cuda", dtype=torch.float32)[:, None, None]
        x = torch.arange(w, device="cuda", dtype=torch.float32)[None, :, None]
        fx = torch.tensor(rng.uniform(0.02, 0.25, 3), device="cuda", dtype=torch.float32)
        fy = torch.tensor(rng.uniform(0.02, 0.25, 3), device="cuda", dtype=torch.float32)
        img = 2048 + 1500 * torch.sin(fx * x + fy * y) + 180 * torch.randn((h, w, 3), device="cuda", generator=g)
        out.append(img.round().clamp(0, 4095).to(torch.int16).contiguous())
    return out


def alternate(fns, reps):
    """The callables in turn, `reps` samples each after one warm-up of all; a sample is what the callable returns (ms)."""
    for f in fns:
        f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t[k].append(f())
    return t


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def inside(x, other):
    return other["min_ms"] <= x["median_ms"] <= other["max_ms"]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="a,b,c")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--parent", default=None, help="another build of libmijpeg.so (section c)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no device: nothing is measured without one")
    sections = args.sections.split(",")
    this = Build(api.LIB_PATH)
    n = args.pictures
    dev12 = pictures(n, 2026)
    dev8 = [(t >> 4).to(torch.uint8).contiguous() for t in dev12]
    host12 = [t.cpu().numpy().view(np.uint16) for t in dev12]
    host8 = [t.cpu().numpy() for t in dev8]
    mpix = sum(t.shape[0] * t.shape[1] for t in dev12) / 1e6

    def frame_array(tensors_or_arrays, ri, device):
        fr = []
        for t in tensors_or_arrays:
            h, w = t.shape[:2]
            sb = t.element_size() if device else t.itemsize  # bytes per sample
            fr.append(api.encode_frame(w, h, 3, QUALITY, (HS, VS), ri, t.data_ptr() if device else t.ctypes.data, w * 3 * sb))
        return (api.MijpegEncodeFrame * len(fr))(*fr)

    def timed(call):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3  # (every call returns with its streams downloaded: synchronised)
        return run

    def list_section(name, dev, host, precision):
        parr = (C.c_int32 * n)(*precision)
        for ri in (4, 0):
            fdev, fhost = frame_array(dev, ri, True), frame_array(host, ri, False)
            expected = this.loop(host, ri, keep=True)
            if this.ragged(this.L.mijpeg_encode_ragged_device16, fdev, parr, keep=True) != expected:
                raise SystemExit("mijpeg_encode_ragged_device16 does not write the single-image encoders' bytes")
            st = this.stats()
            if this.ragged(this.L.mijpeg_encode_ragged16, fhost, parr, keep=True) != expected:
                raise SystemExit("mijpeg_encode_ragged16 does not write the single-image encoders' bytes")
            t = alternate([timed(lambda: this.loop(host, ri)), timed(lambda: this.ragged(this.L.mijpeg_encode_ragged_device16, fdev, parr)),
                           timed(lambda: this.ragged(this.L.mijpeg_encode_ragged16, fhost, parr))], args.reps)
            print(json.dumps({"section": name, "pictures": n, "megapixels": round(mpix, 1), "restart_interval": ri, "reps": args.reps,
                              "stream_MB": round(sum(len(e) for e in expected) / 1e6, 2), "loop_of_single_image_calls": summary(t[0]),
                              "ragged_device16": summary(t[1]), "ragged16_host_pixels": summary(t[2]), "ragged_stats": st,
                              "streams_equal_the_loops": True}), flush=True)

    if "a" in sections:
        list_section("a: all 12-bit", dev12, host12, [12] * n)
    if "b" in sections:
        mixed_dev = [dev8[i] if i % 2 == 0 else dev12[i] for i in range(n)]
        mixed_host = [host8[i] if i % 2 == 0 else host12[i] for i in range(n)]
        list_section("b: 8-bit and 12-bit alternating", mixed_dev, mixed_host, [8 if i % 2 == 0 else 12 for i in range(n)])
    if "c" in sections and args.parent:
        parent = Build(args.parent, new_calls=False)
        f8 = frame_array(dev8, 0, True)
        if parent.ragged(parent.L.mijpeg_encode_ragged_device, f8, None, keep=True) != this.ragged(this.L.mijpeg_encode_ragged_device, f8, None, keep=True):
            raise SystemExit("the 8-bit ragged list: this build's streams differ from the parent's")
        st = {"parent": parent.stats(), "this": this.stats()}
        t = alternate([timed(lambda: parent.ragged(parent.L.mijpeg_encode_ragged_device, f8, None)),
                       timed(lambda: this.ragged(this.L.mijpeg_encode_ragged_device, f8, None))], args.reps)
        a, b = summary(t[0]), summary(t[1])
        print(json.dumps({"section": "c: 8-bit ragged list, mijpeg_encode_ragged_device", "pictures": n, "megapixels": round(mpix, 1), "reps": args.reps,
                          "parent": a, "this": b, "stats": st, "each_median_inside_the_others_range": bool(inside(a, b) and inside(b, a))}), flush=True)
        # uniform forward launches
        W, H, F = 3840, 2160, args.frames
        stream = torch.cuda.current_stream()
        L = api.lib()
        L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.mijpeg_quality_tables.restype = None
        luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
        L.mijpeg_quality_tables(QUALITY, luma.ctypes.data, chroma.ctypes.data)
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        px12 = torch.randint(0, 4096, (F, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
        px8 = (px12 >> 4).to(torch.uint8)
        for prec, px in ((8, px8), (12, px12)):
            info = api.frame_layout(W, H, 3, HS, VS, [luma, chroma], quant_index=[0, 0, 0], precision=prec)
            coef = torch.empty((F, int(info.coef_count)), dtype=torch.int16, device="cuda")
            bt = api.MijpegForwardBatch()
            C.memmove(C.byref(bt.info), C.byref(info), C.sizeof(api.MijpegInfo))
            sb = 2 if prec == 12 else 1
            bt.pixels_dev, bt.pixel_row_stride, bt.pixel_frame_stride = px.data_ptr(), W * 3 * sb, H * W * 3 * sb
            bt.coef_dev, bt.coef_frame_stride, bt.frames = coef.data_ptr(), info.coef_count, F

            def forward_ms(build):
                def run():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.inner):
                        build.forward(bt, stream.cuda_stream)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1) / args.inner
                return run

            t = alternate([forward_ms(parent), forward_ms(this)], args.reps)
            a, b = summary(t[0]), summary(t[1])
            print(json.dumps({"section": f"c: uniform forward launch, {prec} bits", "frames": F, "width": W, "height": H, "reps": args.reps, "parent": a, "this": b,
                              "each_median_inside_the_others_range": bool(inside(a, b) and inside(b, a))}), flush=True)
        parent.close()
    this.close()


if __name__ == "__main__":
    main()

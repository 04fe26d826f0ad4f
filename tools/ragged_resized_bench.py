"""Measurements of the resized call (profiles/ragged_resized.txt): compressed pictures in host memory -> one (N, 3, 224, 224)
batch tensor in HBM.

    python tools/ragged_resized_bench.py [--pictures 256] [--reps 9] [--inner 3] [--size 224] [--only A,B,S1,S12]

The pictures are workload b of tools/ragged_bench.py (the list of DESIGN 4.1e: sides 64..1024 around 4:3, 4:2:0, quality 75..95, DRI =
4); every picture gets a seeded random crop of 8 % .. 100 % of its area with an aspect ratio of 3/4 .. 4/3 (RandomResizedCrop).
  A    what a caller does today: batch.decode_mixed(crops=..., layout="chw"), then per picture
       torch.nn.functional.interpolate(mode="bilinear", antialias=True) on the float picture, then torch.stack (float32 result)
  B    batch.decode_resized(..., layout="chw"): the same decode, the crop launches into the object's arena, ONE resample launch (uint8)
and, from coefficients that are already in HBM (one decode, not timed), the two stages of B:
  S1   mijpeg_reconstruct_ragged_rect_device into crop-size tensors: what stage 1 runs
  S12  mijpeg_reconstruct_ragged_resized_device: stage 1 + the table upload + the resample launch
The routes alternate in one process after a warm-up of each; a repetition times `--inner` calls between two device synchronisations
with the host clock and reports the time per call.  One JSON line: medians of `--reps` with [min .. max]; the bytes the resample
launch moves (crops read, tap tables read, batch written), computed from the shapes; how far A (rounded) and B are apart.
Kernel times come from a trace of a run of its own (rocprofv3 --kernel-trace --stats -- python tools/ragged_resized_bench.py --only S12).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libjpeg_amd import api, batch  # noqa: E402
from ragged_bench import pictures  # noqa: E402


def random_crops(sizes):
    """(x, y, w, h) per picture: area 8 % .. 100 %, aspect ratio log-uniform in 3/4 .. 4/3, clipped to the picture"""
    rng = np.random.default_rng(224)
    out = []
    for w, h in sizes:
        area = float(rng.uniform(0.08, 1.0)) * w * h
        ratio = math.exp(float(rng.uniform(math.log(3 / 4), math.log(4 / 3))))
        cw = max(1, min(w, int(round(math.sqrt(area * ratio)))))
        ch = max(1, min(h, int(round(math.sqrt(area / ratio)))))
        out.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    import torch
    import torch.nn.functional as F

    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--only", default="A,B,S1,S12", help="the routes to run (a kernel trace wants S12 alone)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    side = args.size
    streams = pictures(args.pictures, 4)
    n = len(streams)
    d = api.Decoder(0)
    assert not any(d.decode_ragged_device(streams))
    infos = [d.ragged_info(i) for i in range(n)]
    crops = random_crops([(f.width, f.height) for f in infos])
    rects = [(x, y, x + w - 1, y + h - 1) for x, y, w, h in crops]
    rects_c = api.rect_array(rects)
    crop_tensors = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for _, _, w, h in crops]
    crop_ptrs, crop_rows = [t.data_ptr() for t in crop_tensors], [t.shape[1] * 3 for t in crop_tensors]
    dst = torch.zeros((n, 3, side, side), dtype=torch.uint8, device="cuda")
    result = {}

    def a():
        parts = batch.decode_mixed(streams, 0, decoder=d, layout="chw", crops=crops)
        result["A"] = torch.stack([F.interpolate(t[None].float(), size=(side, side), mode="bilinear", antialias=True)[0] for t in parts])

    def b():
        result["B"], errors = batch.decode_resized(streams, (side, side), crops=crops, layout="chw", decoder=d)
        assert not any(errors)

    def s1():
        d.reconstruct_ragged_rect_device(rects_c, crop_ptrs, crop_rows, wait_foreign=False)

    def s12():
        d.reconstruct_ragged_resized_device(rects_c, side, side, 3, dst.data_ptr(), 3 * side * side, side * side, side, wait_foreign=False)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    routes = {k: fn for k, fn in (("A", a), ("B", b), ("S1", s1), ("S12", s12)) if k in args.only.split(",")}
    for fn in routes.values():  # warm-up of every route (S1 and S12 follow a decode of the same list: A's, B's or the one above)
        timed(fn)
    ms = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    out = {"pictures": n, "size": side, "reps": args.reps, "inner": args.inner, **{k: summary(v) for k, v in ms.items()}}
    if "S12" in routes or "B" in routes:
        st = d.ragged_resized_stats()
        tables = 0
        for _, _, w, h in crops:
            for src in (w, h):
                tables += side * 8 + side * api.resample_taps(src, side)[2].shape[1] * 2
        out["stats"] = st
        out["resample_bytes"] = {"crops_read": st["arena_bytes"], "tables_read": tables, "batch_written": n * 3 * side * side}
    if "A" in result and "B" in result:
        diff = (result["A"].round().clamp(0, 255) - result["B"].float()).abs()
        out["A_rounded_minus_B"] = {"max": float(diff.max()), "share_differing": round(float((diff > 0).float().mean()), 4)}
        out["B_faster_beyond_both_ranges"] = out["B"]["max_ms"] < out["A"]["min_ms"]
    print(json.dumps(out), flush=True)
    d.close()


if __name__ == "__main__":
    main()

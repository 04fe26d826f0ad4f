"""Measurements of the crop calls (profiles/ragged_rect.txt): coefficients in HBM -> a crop of every picture in HBM.

    python tools/ragged_rect_bench.py [--pictures 256] [--reps 9] [--inner 5] [--planar] [--sets whole]

The pictures are workload b of tools/ragged_bench.py (sides 64..1024 around 4:3, 4:2:0, quality 75..95, DRI = 4), decoded ONCE by
mijpeg_decode_ragged_device; what is timed is the way from the coefficient stores to the crops, for three crop sets:
  random224  a 224 x 224 window per picture at a seeded random corner (clipped where the picture is smaller)
  centre78   the centre window of 7/8 of each side
  whole      the whole picture
  A  what a caller does today: mijpeg_reconstruct_ragged_device into full-size tensors, then every slice made contiguous
  B  mijpeg_reconstruct_ragged_rect_device into crop-size tensors
  E  (whole only) the existing call alone, without the slices: B runs the same tiles
A and B (and E) alternate in one process after a warm-up of each; a repetition times `--inner` calls between two device
synchronisations with the host clock and reports the time per call.  Per set one JSON line: medians of `--reps` with [min .. max],
the tiles run and the tiles the pictures have, destination bytes of A (full pictures + crops) and of B (crops).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libjpeg_amd import api  # noqa: E402
from ragged_bench import pictures  # noqa: E402


def crop_sets(infos):
    rng = np.random.default_rng(224)
    sets = {"random224": [], "centre78": [], "whole": []}
    for f in infos:
        w, h = f.width, f.height
        cw, ch = min(224, w), min(224, h)
        x, y = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
        sets["random224"].append((x, y, x + cw - 1, y + ch - 1))
        cw, ch = max(1, w * 7 // 8), max(1, h * 7 // 8)
        x, y = (w - cw) // 2, (h - ch) // 2
        sets["centre78"].append((x, y, x + cw - 1, y + ch - 1))
        sets["whole"].append((0, 0, w - 1, h - 1))
    return sets


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--planar", action="store_true", help="the planar twins: (C, H, W) tensors")
    ap.add_argument("--sets", default="random224,centre78,whole", help="the crop sets to run (a kernel trace wants one at a time)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    planar = args.planar
    streams = pictures(args.pictures, 4)
    d = api.Decoder(0)
    assert not any(d.decode_ragged_device(streams))
    n = len(streams)
    infos = [d.ragged_info(i) for i in range(n)]
    shape = (lambda h, w, c: (c, h, w)) if planar else (lambda h, w, c: (h, w, c))
    full = [torch.zeros(shape(f.height, f.width, f.components), dtype=torch.uint8, device="cuda") for f in infos]
    full_bytes = sum(t.numel() for t in full)

    def ptrs_of(ts):
        return [[t[c].data_ptr() for c in range(t.shape[0])] for t in ts] if planar else [t.data_ptr() for t in ts]

    def rows_of(ts):
        return [t.shape[2] if planar else t.shape[1] * t.shape[2] for t in ts]

    full_ptrs, full_rows = ptrs_of(full), rows_of(full)

    def existing():
        if planar:
            d.reconstruct_ragged_planar_device(full_ptrs, full_rows, wait_foreign=False)
        else:
            d.reconstruct_ragged_device(full_ptrs, full_rows, wait_foreign=False)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    for name, rects in crop_sets(infos).items():
        if name not in args.sets.split(","):
            continue
        crops = [torch.zeros(shape(r[3] - r[1] + 1, r[2] - r[0] + 1, f.components), dtype=torch.uint8, device="cuda") for r, f in zip(rects, infos)]
        crop_ptrs, crop_rows = ptrs_of(crops), rows_of(crops)
        sliced = [None] * n
        rects_c = api.rect_array(rects)  # (converted once, as the destinations' addresses are)

        def a():
            existing()
            for i, (t, r) in enumerate(zip(full, rects)):
                s = t[:, r[1]:r[3] + 1, r[0]:r[2] + 1] if planar else t[r[1]:r[3] + 1, r[0]:r[2] + 1]
                sliced[i] = s.contiguous()

        def b():
            if planar:
                d.reconstruct_ragged_rect_planar_device(rects_c, crop_ptrs, crop_rows, wait_foreign=False)
            else:
                d.reconstruct_ragged_rect_device(rects_c, crop_ptrs, crop_rows, wait_foreign=False)

        routes = {"A": a, "B": b}
        if name == "whole":
            routes["E"] = existing
        for fn in routes.values():  # warm-up of every route
            timed(fn)
        assert all(torch.equal(x, y) for x, y in zip(sliced, crops)), name  # the routes agree on every byte
        ms = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, fn in routes.items():
                ms[k].append(timed(fn))
        st = d.ragged_rect_stats()
        crop_bytes = sum(t.numel() for t in crops)
        out = {"set": name, "planar": planar, "pictures": n, "reps": args.reps, "inner": args.inner, **{k: summary(v) for k, v in ms.items()},
               "stats": st, "workgroups": st["workgroups"], "workgroups_full": st["workgroups_full"],
               "dest_bytes_A": full_bytes + crop_bytes, "dest_bytes_B": crop_bytes}
        a_, b_ = out["A"], out["B"]
        out["B_faster_beyond_both_ranges"] = b_["max_ms"] < a_["min_ms"]
        print(json.dumps(out), flush=True)
    d.close()


if __name__ == "__main__":
    main()

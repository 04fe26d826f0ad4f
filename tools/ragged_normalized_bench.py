"""Measurements of the normalised resized call (profiles/ragged_normalized.txt): compressed pictures in host memory -> one
(N, 3, 224, 224) float batch in HBM, a random half of the pictures mirrored, ImageNet's mean and deviation applied.

    python tools/ragged_normalized_bench.py [--pictures 256] [--reps 9] [--inner 3] [--size 224] [--only A,B,S12u,S12f16,S12f32]

The pictures and crops are those of tools/ragged_resized_bench.py (the list of DESIGN 4.1f).
  A       what a training step does today: batch.decode_resized (uint8), then in torch the per-picture flip of the flagged slots,
          float(), * scale + bias, the cast to float16
  B       batch.decode_resized(dtype=torch.float16, mean=..., std=..., mirror=...): the same decode and crop launches, ONE resample launch
and, from coefficients that are already in HBM (one decode, not timed):
  S12u    mijpeg_reconstruct_ragged_resized_device: the uint8 call
  S12f16  mijpeg_reconstruct_ragged_normalized_device with float16 samples and the mirror flags
  S12f32  ... with float32 samples (four times the bytes written)
The routes alternate in one process after a warm-up of each; a repetition times `--inner` calls between two device synchronisations
with the host clock and reports the time per call.  One JSON line: medians of `--reps` with [min .. max], the statistics of the last
call, and whether A and B hold the same bits.
Kernel times come from a trace of a run of its own (rocprofv3 --kernel-trace --stats -- python tools/ragged_normalized_bench.py --only
S12u,S12f16,S12f32).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libjpeg_amd import api, batch  # noqa: E402
from ragged_bench import pictures  # noqa: E402
from ragged_resized_bench import random_crops, summary  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--only", default="A,B,S12u,S12f16,S12f32", help="the routes to run (a kernel trace wants the S12 routes alone)")
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
    rects_c = api.rect_array([(x, y, x + w - 1, y + h - 1) for x, y, w, h in crops])
    mirror = [bool(v) for v in np.random.default_rng(225).integers(0, 2, n)]
    flagged = torch.tensor([i for i, m in enumerate(mirror) if m], device="cuda")
    scale, bias = batch._normalize_constants(MEAN, STD, 3)
    scale_t = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    bias_t = torch.tensor(bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    dst = {1: torch.zeros((n, 3, side, side), dtype=torch.uint8, device="cuda"), 2: torch.zeros((n, 3, side, side), dtype=torch.float16, device="cuda"),
           4: torch.zeros((n, 3, side, side), dtype=torch.float32, device="cuda")}
    result = {}

    def a():
        u8, errors = batch.decode_resized(streams, (side, side), crops=crops, layout="chw", decoder=d)
        assert not any(errors)
        u8[flagged] = u8[flagged].flip(3)
        result["A"] = (u8.float() * scale_t + bias_t).to(torch.float16)

    def b():
        result["B"], errors = batch.decode_resized(streams, (side, side), crops=crops, layout="chw", decoder=d, dtype=torch.float16, mean=MEAN, std=STD, mirror=mirror)
        assert not any(errors)

    def s12u():
        d.reconstruct_ragged_resized_device(rects_c, side, side, 3, dst[1].data_ptr(), 3 * side * side, side * side, side, wait_foreign=False)

    def s12f(sample, es):
        def call():
            d.reconstruct_ragged_normalized_device(rects_c, side, side, 3, sample, scale, bias, mirror, dst[es].data_ptr(), 3 * side * side * es, side * side * es,
                                                   side * es, wait_foreign=False)
        return call

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    every = (("A", a), ("B", b), ("S12u", s12u), ("S12f16", s12f(api.SAMPLE_F16, 2)), ("S12f32", s12f(api.SAMPLE_F32, 4)))
    routes = {k: fn for k, fn in every if k in args.only.split(",")}
    for fn in routes.values():  # warm-up of every route (the S12 routes follow a decode of the same list: A's, B's or the one above)
        timed(fn)
    ms = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    out = {"pictures": n, "size": side, "reps": args.reps, "inner": args.inner, "mirrored": sum(mirror), **{k: summary(v) for k, v in ms.items()}}
    out["stats"] = {**d.ragged_resized_stats(), **d.ragged_normalized_stats()}
    out["batch_written_bytes"] = {"uint8": n * 3 * side * side, "float16": 2 * n * 3 * side * side, "float32": 4 * n * 3 * side * side}
    if "A" in result and "B" in result:
        out["A_and_B_same_bits"] = bool(torch.equal(result["A"].view(torch.int16), result["B"].view(torch.int16)))
        out["B_faster_beyond_both_ranges"] = out["B"]["max_ms"] < out["A"]["min_ms"]
    print(json.dumps(out), flush=True)
    d.close()


if __name__ == "__main__":
    main()

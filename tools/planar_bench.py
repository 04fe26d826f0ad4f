"""Measurements of planar output (profiles/planar_output.txt): component planes written by the fused kernels themselves
against the interleaved launch, and against the interleaved launch followed by deinterleave_kernel -- the route they replace.

    python tools/planar_bench.py [--workloads k,e] [--reps 9] [--frames 8] [--size 7680x4320] [--pictures 256]

  k  kernel level: `--frames` resident frames of `--size` per layout (4:2:0, 4:2:2, 4:4:4; two pictures, repeated), decoded once;
     timed are the reconstruction calls alone, three candidates alternating in one process:
       a  mijpeg_reconstruct_ragged_device                        (the interleaved ragged launch)
       b  mijpeg_reconstruct_ragged_planar_device                 (the fused planar launch)
       c  a into a staging area + mijpeg_deinterleave_device per frame   (the two-pass route's kernels)
     A timed sample is a burst of `--burst` asynchronous calls between two synchronisations of the object's stream, per call.
  e  end to end: `--pictures` pictures of 64..1024 pixels a side (tools/ragged_bench.py's list a), bytes in host memory ->
     tensors in HBM: batch.decode_mixed(layout="chw") against batch.decode_mixed() + permute(2, 0, 1).contiguous() per tensor.
Every figure: median of `--reps` samples with [min .. max]; the device is warmed on every shape and settled (150 ms of launches)
before the first sample.  One JSON line per layout / workload.  b as a fraction of 8 TB/s counts the kernel's algorithmic bytes:
coefficients in (2 B each: 3, 4 or 6 B per pixel) + 3 B per pixel out.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libjpeg_amd import api, batch, synth  # noqa: E402

PEAK_BYTES_PER_S = 8e12
BYTES_PER_PIXEL = {"420": 6, "422": 7, "444": 9}


def figure(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def spread(f):
    return f["max_ms"] - f["min_ms"]


def kernel_level(layout, w, h, frames, reps, burst):
    import torch

    with ThreadPoolExecutor(2) as ex:
        two = list(ex.map(lambda i: synth.synth_jpeg(w, h, 7100 + i, 85, layout, 8), range(2)))
    streams = [two[i % 2] for i in range(frames)]
    d = api.Decoder(0)
    assert not any(d.decode_ragged_device(streams))
    inter = torch.empty((frames, h, w * 3), dtype=torch.uint8, device="cuda")
    planar = torch.empty((frames, 3, h, w), dtype=torch.uint8, device="cuda")
    planar_c = torch.empty((frames, 3, h, w), dtype=torch.uint8, device="cuda")
    iptrs, irows = [inter[i].data_ptr() for i in range(frames)], [w * 3] * frames
    pptrs = [[planar[i, c].data_ptr() for c in range(3)] for i in range(frames)]
    cptrs = [[planar_c[i, c].data_ptr() for c in range(3)] for i in range(frames)]

    def a():
        d.reconstruct_ragged_device(iptrs, irows, sync=False, wait_foreign=False)

    def b():
        d.reconstruct_ragged_planar_device(pptrs, [w] * frames, sync=False, wait_foreign=False)

    def c():
        a()
        for i in range(frames):
            d.deinterleave_device(iptrs[i], w * 3, w, h, 3, 1, cptrs[i], w)

    cands = {"a_interleaved": a, "b_fused_planar": b, "c_interleaved_then_deinterleave": c}
    for fn in cands.values():  # every shape once: buffers grow, code objects load
        fn()
    d.synchronize()
    st = d.planar_stats()
    assert st["fused"] == frames and st["two_pass"] == 0, st
    want = inter.view(frames, h, w, 3).permute(0, 3, 1, 2)
    assert torch.equal(planar, want) and torch.equal(planar_c, want)  # the three candidates agree on every sample
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) < 0.15:  # settle the clocks
        b()
        d.synchronize()
    ms = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            d.synchronize()
            t0 = time.perf_counter()
            for _ in range(burst):
                fn()
            d.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / burst)
    d.close()
    res = {"workload": "kernel", "layout": layout, "frames": frames, "width": w, "height": h, "burst": burst, "reps": reps}
    for k in cands:
        res[k] = figure(ms[k])
    fa, fb, fc = (res[k] for k in cands)
    pixels = frames * w * h
    res["b_fraction_of_8TBps"] = round(pixels * BYTES_PER_PIXEL[layout] / (fb["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
    res["b_gpixels_per_s"] = round(pixels / (fb["median_ms"] * 1e-3) / 1e9, 1)
    res["b_over_a"] = round(fb["median_ms"] / fa["median_ms"], 4)
    res["b_over_c"] = round(fb["median_ms"] / fc["median_ms"], 4)
    res["b_clears_the_bar"] = fc["median_ms"] - fb["median_ms"] > max(spread(fb), spread(fc))  # faster than c by more than the spread of either
    return res


def end_to_end(pictures, reps):
    import torch

    import ragged_bench

    streams = ragged_bench.pictures(pictures, 0)
    d = api.Decoder(0)

    def chw():
        return batch.decode_mixed(streams, 0, decoder=d, layout="chw")

    def hwc_then_permute():
        return [t.permute(2, 0, 1).contiguous() for t in batch.decode_mixed(streams, 0, decoder=d)]

    cands = {"decode_mixed_chw": chw, "decode_mixed_then_permute": hwc_then_permute}
    x, y = chw(), hwc_then_permute()
    torch.cuda.synchronize()
    st = d.planar_stats()
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    del x, y
    ms = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            del out
    d.close()
    res = {"workload": "end_to_end", "pictures": len(streams), "compressed_MB": round(sum(map(len, streams)) / 1e6, 2), "planar_stats": st, "reps": reps}
    for k in cands:
        res[k] = figure(ms[k])
    res["gain_ms"] = round(res["decode_mixed_then_permute"]["median_ms"] - res["decode_mixed_chw"]["median_ms"], 3)
    res["faster_beyond_both_spreads"] = res["gain_ms"] > max(spread(res["decode_mixed_chw"]), spread(res["decode_mixed_then_permute"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="k,e")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="7680x4320")
    ap.add_argument("--burst", type=int, default=8)
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--layouts", default="420,422,444")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    print(json.dumps({"library": api.LIB_PATH}), flush=True)
    for wl in args.workloads.split(","):
        if wl == "k":
            for layout in args.layouts.split(","):
                print(json.dumps(kernel_level(layout, w, h, args.frames, args.reps, args.burst)), flush=True)
        elif wl == "e":
            print(json.dumps(end_to_end(args.pictures, args.reps)), flush=True)


if __name__ == "__main__":
    main()

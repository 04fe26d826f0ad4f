"""Measurements of planar input for the ragged encode (profiles/planar_encode.txt): the planar-input flavours of the
ragged forward kernels against the interleaved flavours, and against interleave_kernel followed by the interleaved flavours -- the
route they replace.

    python tools/planar_encode_bench.py [--workloads k,e] [--reps 9] [--frames 8] [--size 7680x4320] [--pictures 256]

  k  forward stage alone: `--frames` resident frames of `--size` per layout (4:2:0, 4:2:2, 4:4:4), quality 85; three candidates
     alternating in one process, each a whole ragged encode call of which only the forward stage is timed -- the device time
     between an event in front of the first thing the pass enqueues and an event behind its forward launches
     (MIJPEG_ENCODE_RAGGED_TIME_FORWARD, mijpeg_last_timing [1]; the ~10 us upload of the descriptors is inside for all three):
       a  mijpeg_encode_ragged_device on HWC data                  (the interleaved ragged forward launches)
       b  mijpeg_encode_ragged_planar_device16 on CHW data         (the planar-input launches)
       c  b with MIJPEG_ENCODE_PLANAR_TWO_PASS: interleave_kernel per frame into scratch, then a's launches
  e  end to end: `--pictures` pictures of 64..1024 pixels a side resident in HBM as (3, H, W) tensors, 4:2:0, quality 85:
     batch.encode_mixed(layout="chw") against permute(1, 2, 0).contiguous() on every picture + batch.encode_mixed().
Every figure: median of `--reps` samples with [min .. max]; every shape runs once before the first sample.  One JSON line per
layout / workload."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from libjpeg_amd import api, batch  # noqa: E402


def figure(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def outside_both_ranges(fast, slow):
    return fast["max_ms"] < slow["min_ms"]


def content(w, h, seed):
    """(3, h, w) uint8: smooth colour fields plus noise, planes that differ (the kernels' time does not depend on it; the coder's does)."""
    rng = np.random.default_rng(seed)
    x = np.arange(w, dtype=np.float32)[None, :]
    y = np.arange(h, dtype=np.float32)[:, None]
    out = np.empty((3, h, w), np.uint8)
    for c, (fx, fy) in enumerate(((37.0, 53.0), (91.0, 67.0), (17.0, 29.0))):
        out[c] = np.clip(128 + 90 * np.sin(x / fx + c) * np.cos(y / fy) + rng.normal(0, 4, (h, w)), 0, 255).astype(np.uint8)
    return out


_TWO = {}  # the two pictures of a size, made once


def kernel_level(layout, w, h, frames, reps):
    import torch

    os.environ["MIJPEG_ENCODE_RAGGED_TIME_FORWARD"] = "1"
    if (w, h) not in _TWO:
        _TWO[(w, h)] = [content(w, h, 7100 + i) for i in range(2)]
    two = [torch.from_numpy(p).cuda() for p in _TWO[(w, h)]]
    chw = torch.stack([two[i % 2] for i in range(frames)])  # (frames, 3, h, w)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    del two
    d = api.Decoder(0)
    iframes = [api.encode_frame(w, h, 3, 85, layout, 0, hwc[i].data_ptr(), w * 3) for i in range(frames)]
    pframes = [api.encode_frame(w, h, 3, 85, layout, 0, 0, w) for i in range(frames)]
    planes = [[chw[i, c].data_ptr() for c in range(3)] for i in range(frames)]
    out = {}

    def a():
        out["a"] = d.encode_ragged_device(iframes, False)
        return d.timing()["h2d_wait"] * 1e3

    def b():
        out["b"] = d.encode_ragged_planar_device(pframes, planes, False)
        return d.timing()["h2d_wait"] * 1e3

    def c():
        os.environ["MIJPEG_ENCODE_PLANAR_TWO_PASS"] = "1"
        try:
            out["c"] = d.encode_ragged_planar_device(pframes, planes, False)
        finally:
            del os.environ["MIJPEG_ENCODE_PLANAR_TWO_PASS"]
        return d.timing()["h2d_wait"] * 1e3

    cands = {"a_interleaved": a, "b_planar_input": b, "c_interleave_then_a": c}
    routes = {}
    for k, fn in cands.items():  # every shape once: buffers grow, code objects load
        fn()
        routes[k] = dict(d.encode_ragged_stats(), **(d.encode_planar_stats() if k != "a_interleaved" else {}))
    assert out["a"] == out["b"] == out["c"]  # the three candidates write the same streams
    assert routes["b_planar_input"]["fused"] == frames and routes["c_interleave_then_a"]["two_pass"] == frames
    ms = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            ms[k].append(fn())
    d.close()
    res = {"workload": "forward_stage", "layout": layout, "frames": frames, "width": w, "height": h, "reps": reps,
           "forward_launches": {k: routes[k]["forward_launches"] for k in cands}, "stream_bytes": sum(map(len, out["a"]))}
    for k in cands:
        res[k] = figure(ms[k])
    fa, fb, fc = (res[k] for k in cands)
    res["b_over_a"] = round(fb["median_ms"] / fa["median_ms"], 4)
    res["b_over_c"] = round(fb["median_ms"] / fc["median_ms"], 4)
    res["b_gpixels_per_s"] = round(frames * w * h / (fb["median_ms"] * 1e-3) / 1e9, 1)
    res["b_beats_c_outside_both_ranges"] = outside_both_ranges(fb, fc)
    del os.environ["MIJPEG_ENCODE_RAGGED_TIME_FORWARD"]
    return res


def end_to_end(pictures, reps):
    import torch

    rng = np.random.default_rng(20261020)
    sizes = [(int(rng.integers(64, 1025)), int(rng.integers(64, 1025))) for _ in range(pictures)]
    base = torch.from_numpy(content(1024, 1024, 5)).cuda()
    chw = [base[:, :h, :w].contiguous() for w, h in sizes]
    d = api.Decoder(0)

    def planar():
        return batch.encode_mixed(chw, 85, "420", 0, decoder=d, layout="chw")

    def permute_then_interleaved():
        return batch.encode_mixed([t.permute(1, 2, 0).contiguous() for t in chw], 85, "420", 0, decoder=d)

    cands = {"encode_mixed_chw": planar, "permute_then_encode_mixed": permute_then_interleaved}
    x, y = planar(), permute_then_interleaved()
    st = d.encode_planar_stats()
    assert x == y
    ms = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    d.close()
    pixel_bytes = sum(3 * w * h for w, h in sizes)
    res = {"workload": "end_to_end", "pictures": pictures, "pixel_MB": round(pixel_bytes / 1e6, 1), "stream_MB": round(sum(map(len, x)) / 1e6, 2),
           "planar_stats": st, "reps": reps, "destination_bytes_saved": pixel_bytes, "permute_kernels_saved": pictures}
    for k in cands:
        res[k] = figure(ms[k])
    fp, fi = res["encode_mixed_chw"], res["permute_then_encode_mixed"]
    res["gain_ms"] = round(fi["median_ms"] - fp["median_ms"], 3)
    res["faster_outside_both_ranges"] = outside_both_ranges(fp, fi)
    return res


def registers():
    """VGPRs (AGPRs included) of the six planar-input kernels beside their interleaved ragged twins', from the library's metadata."""
    from test_ragged_batch import LIB, _kernel_metadata

    meta = _kernel_metadata(LIB)
    out = {}
    for name, k in sorted(meta.items()):
        if "planar_in" not in name:
            continue
        twin = meta[name.replace("_ZN3mij9planar_in", "_ZN3mij").replace("NS0_10KernelArgs", "NS_10KernelArgs")]
        short = name.split("planar_in", 1)[1].split("EEv")[0].lstrip("0123456789")
        regs = lambda m: int(m["vgpr_count"]) + int(m.get("agpr_count", 0))
        out[short] = {"planar_vgprs": regs(k), "twin_vgprs": regs(twin), "planar_sgprs": int(k["sgpr_count"]), "twin_sgprs": int(twin["sgpr_count"]),
                      "scratch": int(k["private_segment_fixed_size"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="r,k,e")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="7680x4320")
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--layouts", default="420,422,444")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    print(json.dumps({"library": os.path.relpath(api.LIB_PATH, ROOT)}), flush=True)
    for wl in args.workloads.split(","):
        if wl == "r":
            print(json.dumps({"workload": "registers", "kernels": registers()}), flush=True)
        elif wl == "k":
            for layout in args.layouts.split(","):
                print(json.dumps(kernel_level(layout, w, h, args.frames, args.reps)), flush=True)
        elif wl == "e":
            print(json.dumps(end_to_end(args.pictures, args.reps)), flush=True)


if __name__ == "__main__":
    main()

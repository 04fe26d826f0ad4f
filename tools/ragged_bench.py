"""Measurements of the ragged batch path (profiles/ragged_batch.txt): bytes in host memory -> pixels in HBM.

    python tools/ragged_bench.py [--workloads a,b,c,s,u] [--reps 9] [--pictures 256] [--frames 64]

Workloads, generated from seeds:
  a  `--pictures` pictures, sides drawn uniformly from 64..1024 around a 4:3 aspect, 4:2:0, quality 75..95, optimised tables, no DRI
  b  the same pictures with DRI = 4
  c  `--frames` x 3840 x 2160, 4:2:0, quality 85, DRI = 8
  s  `--pictures` pictures of 64..240 pixels a side (fewer than 256 MCUs each), 4:2:0, without restart markers -- every one of them
     ONE interval decoded by one lane -- and the same pictures with DRI = 1, through the ragged calls: what the one-lane route costs
  u  32 x 3840 x 2160 through mijpeg_decode_batch_device alone (the uniform device Huffman decode; runs on trees without the
     ragged calls as well: the non-regression comparison)
For a and b: the ragged calls against the two single-image routes, one decoder object, same process:
  loop-device  mijpeg_decode_coefficients_device (prefer-gpu: min_intervals = 1), host decoder where that declines, + mijpeg_reconstruct_device
  loop-host    mijpeg_decode_coefficients + mijpeg_reconstruct_device
For c: the ragged calls against mijpeg_decode_batch_device + mijpeg_reconstruct_batch_device.
Every figure: median over `--reps` repetitions of the timed call and the spread (max - min) beside it, one JSON line per workload.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libjpeg_amd import api, synth  # noqa: E402


def pictures(n, dri, largest=1024):
    rng = np.random.default_rng(4242)
    jobs = []
    for i in range(n):
        side = int(rng.integers(64, largest + 1))
        aspect = (4 / 3) * float(rng.uniform(0.85, 1.15))
        if rng.random() < 0.5:
            w, h = side, max(64, min(largest, int(round(side / aspect))))
        else:
            h, w = side, max(64, min(largest, int(round(side / aspect))))
        jobs.append((w, h, 9000 + i, int(rng.integers(75, 96))))
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda j: synth.encode_jpeg(synth.synth_image(j[0], j[1], j[2]), j[3], "420", dri, optimize=True), jobs))


def frames_4k(n):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda i: synth.synth_jpeg(3840, 2160, 1000 + i, 85, "420", 8), range(n)))


def timed(fn, reps):
    import torch

    fn()  # warm-up: buffers grow, tables are built
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "reps": reps}


def destinations(streams):
    import torch

    hd = api.Decoder(None)
    out = []
    for s in streams:
        f = hd.read_header(s)
        out.append(torch.zeros((f.height, f.width * f.components), dtype=torch.uint8, device="cuda"))
    hd.close()
    return out


def compare_routes(streams, reps):
    import torch

    L = api.lib()
    d = api.Decoder(0)
    dst = destinations(streams)
    ptrs, rows = [t.data_ptr() for t in dst], [t.shape[1] for t in dst]
    res = {"pictures": len(streams), "compressed_MB": round(sum(map(len, streams)) / 1e6, 2), "megapixels": round(sum(t.shape[0] * t.shape[1] // 3 for t in dst) / 1e6, 2)}

    def ragged():
        assert not any(d.decode_ragged_device(streams))
        d.reconstruct_ragged_device(ptrs, rows, wait_foreign=False)

    res["ragged"] = timed(ragged, reps)
    res["ragged_stats"] = d.ragged_stats()
    want = [t.clone() for t in dst]

    def loop(device_first):
        def run():
            for s, p, r in zip(streams, ptrs, rows):
                rc = L.mijpeg_set_input(d._h, s, len(s))
                rc = rc or (L.mijpeg_decode_coefficients_device(d._h, 1) if device_first else api.ERR_NOT_AVAILABLE)
                if rc == api.ERR_NOT_AVAILABLE:
                    rc = L.mijpeg_decode_coefficients(d._h, 0)
                rc = rc or L.mijpeg_reconstruct_device(d._h, p, r, 0, 0)
                assert rc == 0, rc
            d.synchronize()
        return run

    for name, device_first in (("loop_device", True), ("loop_host", False)):
        for t in dst:
            t.zero_()
        res[name] = timed(loop(device_first), reps)
        assert all(torch.equal(a, b) for a, b in zip(dst, want)), name  # the routes agree on every pixel
    base = min(res["loop_device"], res["loop_host"], key=lambda r: r["median_ms"])
    res["baseline"] = "loop_device" if base is res["loop_device"] else "loop_host"
    res["gain_ms"] = round(base["median_ms"] - res["ragged"]["median_ms"], 3)
    res["faster_beyond_both_spreads"] = res["gain_ms"] > base["spread_ms"] + res["ragged"]["spread_ms"]
    d.close()
    return res


def compare_uniform(streams, reps):
    import torch

    d = api.Decoder(0)
    n, row = len(streams), 3840 * 3
    out = torch.zeros((n, 2160, row), dtype=torch.uint8, device="cuda")
    ptrs = [out[i].data_ptr() for i in range(n)]

    def uniform():
        d.decode_batch_device(streams, 1)
        d.reconstruct_batch_device(out.data_ptr(), 2160 * row, row, wait_foreign=False)

    def ragged():
        assert not any(d.decode_ragged_device(streams))
        d.reconstruct_ragged_device(ptrs, [row] * n, wait_foreign=False)

    res = {"frames": n, "uniform_batch": timed(uniform, reps)}
    want = out.clone()
    out.zero_()
    res["ragged"] = timed(ragged, reps)
    assert torch.equal(out, want)
    res["ragged_stats"] = d.ragged_stats()
    d.close()
    return res


def one_lane_cost(n, reps):
    d = api.Decoder(0)
    res = {"pictures": n}
    for name, dri in (("no_restart_markers_one_lane_each", 0), ("dri_1", 1)):
        streams = pictures(n, dri, largest=240)
        dst = destinations(streams)
        ptrs, rows = [t.data_ptr() for t in dst], [t.shape[1] for t in dst]

        def decode():
            assert not any(d.decode_ragged_device(streams))

        def both():
            decode()
            d.reconstruct_ragged_device(ptrs, rows, wait_foreign=False)

        res[name] = {"decode": timed(decode, reps), "decode_and_reconstruct": timed(both, reps), "stats": d.ragged_stats(),
                     "compressed_MB": round(sum(map(len, streams)) / 1e6, 2)}
    d.close()
    return res


def uniform_huffman(reps):
    d = api.Decoder(0)
    streams = frames_4k(32)
    res = {"frames": 32, "decode_batch_device": timed(lambda: d.decode_batch_device(streams, 1), reps)}
    d.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,c,u")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    assert args.reps >= 7
    for w in args.workloads.split(","):
        if w in ("a", "b"):
            r = compare_routes(pictures(args.pictures, 0 if w == "a" else 4), args.reps)
        elif w == "c":
            r = compare_uniform(frames_4k(args.frames), args.reps)
        elif w == "s":
            r = one_lane_cost(args.pictures, args.reps)
        else:
            r = uniform_huffman(args.reps)
        print(json.dumps({"workload": w, **r}), flush=True)


if __name__ == "__main__":
    main()

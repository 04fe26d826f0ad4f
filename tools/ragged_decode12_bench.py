"""Measurements of the ragged decode with 12-bit layout groups (profiles/ragged_decode12.txt): bytes in host memory -> pixels in HBM.

    python tools/ragged_decode12_bench.py [--workloads a0,a4,b0,b4] [--reps 9] [--pictures 256]

Workloads, generated from seeds (the picture list of tools/ragged_bench.py: sides 64..1024 around 4:3, 4:2:0, quality 75..95):
  a0 / a4  every picture 12 bit (synth.to_12bit(.., 16)), without restart markers / with DRI = 4
  b0 / b4  the same list with every other picture left 8 bit
Candidates, alternating repetition by repetition on one decoder object in one process:
  old  mijpeg_decode_ragged_device   + mijpeg_reconstruct_ragged_device  (every 12-bit picture on the single-image route: today's
       route for such a list)
  new  mijpeg_decode_ragged_device16 + mijpeg_reconstruct_ragged_device  (12-bit layout groups)
Every figure: median over `--reps` repetitions with minimum and maximum, one JSON line per workload; the two calls' pictures are
compared byte for byte before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libjpeg_amd import api, synth  # noqa: E402
from ragged_bench import pictures  # noqa: E402


def destinations(streams):
    import torch

    hd = api.Decoder(None)
    out = []
    for s in streams:
        f = hd.read_header(s)
        out.append(torch.zeros((f.height, f.width * f.components * (2 if f.precision > 8 else 1)), dtype=torch.uint8, device="cuda"))
    hd.close()
    return out


def compare(streams, reps):
    import torch

    d = api.Decoder(0)
    dst = destinations(streams)
    ptrs, rows = [t.data_ptr() for t in dst], [t.shape[1] for t in dst]
    res = {"pictures": len(streams), "compressed_MB": round(sum(map(len, streams)) / 1e6, 2)}

    def run(with_12bit):
        assert not any(d.decode_ragged_device(streams, with_12bit=with_12bit))
        d.reconstruct_ragged_device(ptrs, rows, wait_foreign=False)

    pixels = {}
    for name, flag in (("old", False), ("new", True)):  # warm-up, statistics, the pictures
        for t in dst:
            t.zero_()
        run(flag)
        res[name + "_stats"] = d.ragged_stats()
        pixels[name] = [t.clone() for t in dst]
    assert all(torch.equal(a, b) for a, b in zip(pixels["old"], pixels["new"])), "the two calls disagree on a picture"
    ms = {"old": [], "new": []}
    for _ in range(reps):
        for name, flag in (("old", False), ("new", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(flag)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in ms.items():
        res[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "reps": reps}
    res["ranges_disjoint"] = res["new"]["max_ms"] < res["old"]["min_ms"] or res["old"]["max_ms"] < res["new"]["min_ms"]
    d.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a0,a4,b0,b4")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pictures", type=int, default=256)
    args = ap.parse_args()
    assert args.reps >= 7
    for w in args.workloads.split(","):
        eight = pictures(args.pictures, 4 if w[1] == "4" else 0)
        streams = [s if (w[0] == "b" and i % 2 == 0) else synth.to_12bit(s, 16) for i, s in enumerate(eight)]
        print(json.dumps({"workload": w, **compare(streams, args.reps)}), flush=True)


if __name__ == "__main__":
    main()

"""Measurements of the ragged encode (profiles/ragged_encode.txt): pixels resident in HBM -> finished streams in host memory.

    python tools/ragged_encode_bench.py [--workloads a,ao,ar,c] [--reps 9] [--pictures 256] [--frames 64] [--old-only]

Workloads, generated from seeds:
  a   `--pictures` pictures, sides drawn uniformly from 64..1024 around a 4:3 aspect, 4:2:0, quality 85, no restart markers
  ao  the same with optimised Huffman tables
  ar  the same with a restart interval of 4 MCUs
  c   `--frames` x 3840 x 2160 of one geometry, 4:2:0, quality 85, restart interval 8
Old and new route alternate in one process, on one decoder object:
  a*  mijpeg_encode_ragged_device for the whole list against the only route there was for such a list: a loop of
      mijpeg_encode_batch_device with frames = 1, one call per picture
  c   mijpeg_encode_ragged_device against ONE mijpeg_encode_batch_device call for all frames
The clock starts with the pictures in device memory and stops when the last stream is complete in host memory.  Every figure:
median over `--reps` repetitions after a warm-up and the spread (max - min) beside it, one JSON line per workload.  The streams
of the two routes are compared once, outside the timed region.  --old-only times the old route alone: it runs on a build without
the ragged encode as well (MIJPEG_LIBRARY), which is how the uniform call is compared between two builds.
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

HS, VS = (2, 1, 1), (2, 1, 1)


def picture_sizes(n, largest=1024):
    rng = np.random.default_rng(4242)
    out = []
    for _ in range(n):
        side = int(rng.integers(64, largest + 1))
        aspect = (4 / 3) * float(rng.uniform(0.85, 1.15))
        other = max(64, min(largest, int(round(side / aspect))))
        out.append((side, other) if rng.random() < 0.5 else (other, side))
    return out


def quality_tables(q):
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.mijpeg_quality_tables.restype = None
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    L.mijpeg_quality_tables(q, luma.ctypes.data, chroma.ctypes.data)
    return [luma, chroma]


def alternate(old, new, reps):
    """old and new in turn, `reps` times each after one warm-up of both; -> (median ms, spread ms) of each."""
    old(), new()
    t_old, t_new = [], []
    for _ in range(reps):
        for fn, ms in ((old, t_old), (new, t_new)):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(t_old), max(t_old) - min(t_old)), (statistics.median(t_new), max(t_new) - min(t_new))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,ao,ar,c")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--old-only", action="store_true")
    args = ap.parse_args()
    dec = api.Decoder(0)
    quant = quality_tables(85)
    for wl in args.workloads.split(","):
        if wl in ("a", "ao", "ar"):
            sizes = picture_sizes(args.pictures)
            ri, opt = (4 if wl == "ar" else 0), wl == "ao"
            tensors = [torch.from_numpy(synth.synth_image(w, h, 9000 + i)).cuda() for i, (w, h) in enumerate(sizes)]
            infos = [api.frame_layout(w, h, 3, HS, VS, quant, quant_index=[0, 0, 0]) for w, h in sizes]
            coef = torch.empty(max(int(f.coef_count) for f in infos), dtype=torch.int16, device="cuda")
            frames = [api.encode_frame(w, h, 3, 85, "420", ri, t.data_ptr()) for (w, h), t in zip(sizes, tensors)]
            count = len(sizes)
            torch.cuda.synchronize()
            keep = {}

            def old():
                keep["old"] = [dec.encode_batch_device(f, t.data_ptr(), coef.data_ptr(), 1, w * 3, w * h * 3, ri, opt)[0]
                               for f, t, (w, h) in zip(infos, tensors, sizes)]

            def new():
                keep["new"] = dec.encode_ragged_device(frames, opt)

            mpix = sum(w * h for w, h in sizes) / 1e6
        elif wl == "c":
            w, h, n = 3840, 2160, args.frames
            ri, opt = 8, False
            px = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
            for i in range(n):
                px[i] = torch.from_numpy(synth.synth_image(w, h, 1000 + i)).cuda()
            info = api.frame_layout(w, h, 3, HS, VS, quant, quant_index=[0, 0, 0])
            coef = torch.empty((n, int(info.coef_count)), dtype=torch.int16, device="cuda")
            frames = [api.encode_frame(w, h, 3, 85, "420", ri, px[i].data_ptr()) for i in range(n)]
            count = n
            torch.cuda.synchronize()
            keep = {}

            def old():
                keep["old"] = dec.encode_batch_device(info, px.data_ptr(), coef.data_ptr(), n, w * 3, w * h * 3, ri, opt)

            def new():
                keep["new"] = dec.encode_ragged_device(frames, opt)

            mpix = n * w * h / 1e6
        else:
            raise SystemExit(f"unknown workload {wl}")
        if args.old_only:
            (m_old, s_old), _ = alternate(old, lambda: None, args.reps)
            print(json.dumps(dict(workload=wl, pictures=count, megapixels=round(mpix, 1), restart_interval=ri, optimize=opt, reps=args.reps,
                                  old_ms=round(m_old, 3), old_spread_ms=round(s_old, 3))), flush=True)
            continue
        (m_old, s_old), (m_new, s_new) = alternate(old, new, args.reps)
        st = dec.encode_ragged_stats()
        print(json.dumps(dict(workload=wl, pictures=count, megapixels=round(mpix, 1), restart_interval=ri, optimize=opt, reps=args.reps,
                              old_ms=round(m_old, 3), old_spread_ms=round(s_old, 3), new_ms=round(m_new, 3), new_spread_ms=round(s_new, 3),
                              speedup=round(m_old / m_new, 2), beyond_noise=bool(abs(m_old - m_new) > s_old + s_new),
                              same_bytes=keep["old"] == keep["new"], stats=st)), flush=True)
        del keep
    dec.close()


if __name__ == "__main__":
    main()

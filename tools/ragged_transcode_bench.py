"""Measurements of the ragged transcode (profiles/ragged_transcode.txt): compressed pictures in host memory -> recoded
streams in host memory.

    python tools/ragged_transcode_bench.py [--pictures 256] [--reps 9] [--only A,B] [--quality 75]

The pictures are workload b of tools/ragged_bench.py (sides 64..1024 around 4:3, 4:2:0, quality 75..95, DRI = 4).
  A    kept tables.  old: what there was for such a list -- per picture Decoder.read(entropy="gpu") + encode_coefficients_device;
       new: decode_ragged_device + transcode_ragged_device(None).  The streams of the two are compared once, outside the clock
  B    another quality.  pixels: batch.decode_mixed + batch.encode_mixed at `--quality` (a second generation of DCT loss, 4:2:0 again);
       new: decode_ragged_device + transcode_ragged_device at `--quality`.  Context only: the outputs differ by construction
  K    decode once, then `--reps` transcode calls at `--quality` alone: the run a kernel trace wants
       (rocprofv3 --kernel-trace --stats -- python tools/ragged_transcode_bench.py --only K), with the bytes requant_list_kernel moves
The candidates of a section alternate in one process after a warm-up of each, host clock around calls that wait; medians of `--reps`
with [min .. max].  One JSON line.
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

from libjpeg_amd import api, batch  # noqa: E402
from ragged_bench import pictures  # noqa: E402


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def alternate(routes, reps):
    for fn in routes.values():
        fn()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summary(v) for k, v in ms.items()}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--only", default="A,B")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    streams = pictures(args.pictures, 4)
    n = len(streams)
    d, one = api.Decoder(0), api.Decoder(0)
    out = {"pictures": n, "reps": args.reps, "quality": args.quality, "source_bytes": sum(len(s) for s in streams)}
    keep = {}
    only = args.only.split(",")

    def loop():
        got = []
        for s in streams:
            info = one.read(s, entropy="gpu")
            got.append(one.encode_coefficients_device(info, one.device_coefficients(), info.restart_interval, False))
        keep["loop"] = got

    def list_kept():
        assert not any(d.decode_ragged_device(streams))
        keep["kept"], status = d.transcode_ragged_device(None, False)
        assert not any(status)

    def list_quality():
        assert not any(d.decode_ragged_device(streams))
        keep["quality"], status = d.transcode_ragged_device([(args.quality, -1)] * n, False)
        assert not any(status)

    def through_pixels():
        tensors = batch.decode_mixed(streams, 0, decoder=d)
        keep["pixels"] = batch.encode_mixed(tensors, args.quality, "420", 4, decoder=d)

    if "A" in only:
        out["A"] = alternate({"loop": loop, "list": list_kept}, args.reps)
        out["A"]["same_bytes"] = keep["loop"] == keep["kept"]
        out["A"]["stats"] = d.transcode_ragged_stats()
        out["A"]["list_faster_beyond_both_ranges"] = out["A"]["list"]["max_ms"] < out["A"]["loop"]["min_ms"]
    if "B" in only:
        out["B"] = alternate({"pixels": through_pixels, "list": list_quality}, args.reps)
        out["B"]["stats"] = d.transcode_ragged_stats()
        out["B"]["bytes"] = {"pixels": sum(len(s) for s in keep["pixels"]), "list": sum(len(s) for s in keep["quality"])}
    if "K" in only:
        assert not any(d.decode_ragged_device(streams))
        coefficients = sum(int(d.ragged_info(i).coef_count) for i in range(n))
        plain = torch.zeros((2, coefficients), dtype=torch.int16, device="cuda")
        for _ in range(args.reps + 1):
            got, status = d.transcode_ragged_device([(args.quality, -1)] * n, False)
            assert not any(status)
            plain[1].copy_(plain[0])  # (a plain device copy of the same size, for the trace to set beside the kernel)
        torch.cuda.synchronize()
        out["K"] = {"calls": args.reps + 1, "requant_bytes_read": coefficients * 2, "requant_bytes_written": coefficients * 2, "descriptor_bytes": n * 2208,
                    "stats": d.transcode_ragged_stats()}
    print(json.dumps(out), flush=True)
    d.close()
    one.close()


if __name__ == "__main__":
    main()

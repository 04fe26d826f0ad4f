"""Measurements of the ragged transcode's transforms (profiles/ragged_transform.txt).

    python tools/ragged_transform_bench.py [--pictures 256] [--reps 9] [--only C]

The pictures are the 256-picture list of tools/ragged_transcode_bench.py (workload b of tools/ragged_bench.py: sides 64..1024 around
4:3, 4:2:0, quality 75..95, DRI = 4).  Mirrored axes are trimmed to whole MCUs (MIJPEG_TRANSFORM_TRIM): the list's sizes are any.
  C    the whole call, kept tables: decode_ragged_device + transcode_ragged_device(None) without a transform -- the call as it was --
       against the same with rot90 for every picture.  The candidates alternate in one process after a warm-up of each, host clock
       around calls that wait; medians of `--reps` with [min .. max]
  K    decode once, then `--reps` + 1 kept transcode calls each without a transform (requant_list_kernel, the yardstick: the same
       bytes with the same ownership), with flip_h and with rot90 (transform_list_kernel), in turn: the run a kernel trace wants
       (rocprofv3 --kernel-trace --stats -- python tools/ragged_transform_bench.py --only K), with the bytes each launch moves.
       K_FLIP / K_ROT / K_NONE run one of the three alone, so that a trace's per-kernel statistics speak of one transform
The other way to transpose a block (eight strided 2-byte loads instead of the exchange through LDS) is tools/microbench/
transpose_variants.hip, a program of its own.  One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libjpeg_amd import api  # noqa: E402
from ragged_bench import pictures  # noqa: E402
from ragged_transcode_bench import alternate  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="C")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    streams = pictures(args.pictures, 4)
    n = len(streams)
    d = api.Decoder(0)
    out = {"pictures": n, "reps": args.reps, "source_bytes": sum(len(s) for s in streams)}
    only = args.only.split(",")
    codes = {"none": None, "flip_h": [api.TRANSFORM_FLIP_H | api.TRANSFORM_TRIM] * n, "rot90": [api.TRANSFORM_ROT_90 | api.TRANSFORM_TRIM] * n}
    keep = {}

    def call(name):
        def run():
            assert not any(d.decode_ragged_device(streams))
            keep[name], status = d.transcode_ragged_device(None, False, codes[name])
            assert not any(status), status
            keep[name + "_stats"] = dict(d.transcode_ragged_stats(), **d.transcode_transform_stats())
        return run

    if "C" in only:
        out["C"] = alternate({"kept": call("none"), "kept_rot90": call("rot90")}, args.reps)
        out["C"]["stats"] = {"kept": keep["none_stats"], "kept_rot90": keep["rot90_stats"]}
        out["C"]["bytes_out"] = {"kept": sum(len(s) for s in keep["none"]), "kept_rot90": sum(len(s) for s in keep["rot90"])}
    traced = [k for k in ("none", "flip_h", "rot90") if "K" in only or {"none": "K_NONE", "flip_h": "K_FLIP", "rot90": "K_ROT"}[k] in only]
    if traced:
        assert not any(d.decode_ragged_device(streams))
        read = sum(int(d.ragged_info(i).coef_count) for i in range(n)) * 2
        out["K"] = {"calls_each": args.reps + 1, "source_plane_bytes": read, "descriptor_bytes": n * 2208}
        for _ in range(args.reps + 1):
            for name in traced:
                got, status = d.transcode_ragged_device(None, False, codes[name])
                assert not any(status)
                st = dict(d.transcode_ragged_stats(), **d.transcode_transform_stats())
                plan = [api.transcode_plan_transformed(d.ragged_info(i), api.TRANSCODE_KEEP, -1, codes[name][i] if codes[name] else 0)[1] for i in range(n)]
                out["K"][name] = {"bytes_written": sum(int(f.coef_count) for f in plan) * 2, "requant_launches": st["requant_launches"],
                                  "transform_launches": st["transform_launches"], "trimmed": st["trimmed"]}
        torch.cuda.synchronize()
    print(json.dumps(out), flush=True)
    d.close()


if __name__ == "__main__":
    main()

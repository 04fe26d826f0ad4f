#!/usr/bin/env python3
"""Restart marker search and unstuffing on the device (mijpeg_set_device_markers) against the host's, option off
and on alternating in one process, medians of --reps with [min .. max]:

  --part a   mijpeg_prepare_batch_host -- the host half of a batch submit -- over 32 4K 4:2:0 Q85 DRI 8 streams with one worker
             (MIJPEG_THREADS=1 unless the environment says otherwise), ms per stream.  Needs no GPU.
  --part b   the pipeline (libjpeg_amd.batch.BatchShard, chunks of 32, two decoder objects) over 256 such streams, ms per batch,
             with the worker pool the environment gives (MIJPEG_THREADS).
  --part c   the option-on pipeline alone, a few times -- the run to put under a kernel-trace-only profiler for the search
             launches' times (marker_count_kernel, marker_write_kernel, the scans between them).

  Streams WITHOUT restart markers (4K 4:2:0 Q85, DRI 0: searched with one expected interval, fitted, walked on the device):
  --part na  (a) for them, and for the DRI 8 streams in the same run (one worker).  Needs no GPU.
  --part nb  mijpeg_decode_batch_device over 32 of them, bytes -> coefficients in HBM, ms per batch.
  --part nc  batch.decode_mixed over 64 pictures of 64 .. 1024 pixels a side (half of them without restart markers), ms per list.

    python tools/device_markers_bench.py --part a|b|c|na|nb|nc [--reps 9] [--streams 32] [--batch 256] [--out FILE]   (--out appends)

(d), bench.py on the parent build and on this one, is two runs of bench.py and not part of this script.
"""
import argparse
import os
import statistics
import sys
import time

if "--part=a" in sys.argv or "--part=na" in sys.argv or ("--part" in sys.argv[:-1] and sys.argv[sys.argv.index("--part") + 1] in ("a", "na")):  # (the pool is sized when the library loads)
    os.environ.setdefault("MIJPEG_THREADS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libjpeg_amd import api, batch, synth  # noqa: E402


def med(xs):
    return f"{statistics.median(xs):8.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def alternate(fa, fb, reps):
    a, b = [], []
    fa(), fb()  # warm: buffers grown, pages touched
    for _ in range(reps):
        a.append(fa())
        b.append(fb())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--part", required=True, choices=["a", "b", "c", "na", "nb", "nc"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.part in ("na", "nb", "nc"):
        return no_restart_markers(args, say, lines)
    distinct = [synth.synth_jpeg(3840, 2160, 500 + i, 85, "420", 8) for i in range(4)]
    streams = [distinct[i % 4] for i in range(args.streams)]
    say(f"streams: 4K 4:2:0 Q85 DRI 8, {sum(map(len, streams)) / len(streams) / 1e6:.2f} MB each; MIJPEG_THREADS={os.environ.get('MIJPEG_THREADS', 'unset')}, "
        f"{api.lib().mijpeg_default_threads()} workers")

    if args.part == "a":
        off, on = api.Decoder(None), api.Decoder(None)
        on.set_device_markers(1)

        def host_half(d):
            def run():
                t0 = time.perf_counter()
                d.prepare_batch_host(streams)
                return (time.perf_counter() - t0) * 1e3 / len(streams)
            return run

        a, b = alternate(host_half(off), host_half(on), args.reps)
        assert on.device_markers_stats()[1] == 0, "the option-on half declined"
        say(f"(a) mijpeg_prepare_batch_host over {args.streams} streams, ms per stream")
        say(f"    option off  {med(a)}")
        say(f"    option on   {med(b)}")
        off.close()
        on.close()
        return finish(args, lines)

    import torch

    many = [distinct[i % 4] for i in range(args.batch)]

    def pipeline(shard):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            shard.run()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return run

    s_on = batch.BatchShard(many, 0, chunk=32, depth=2, device_markers=True)
    if args.part == "c":
        for _ in range(3):
            pipeline(s_on)()
        assert s_on.fallbacks == 0
        s_on.close()
        return 0
    s_off = batch.BatchShard(many, 0, chunk=32, depth=2)
    a, b = alternate(pipeline(s_off), pipeline(s_on), args.reps)
    assert s_on.fallbacks == 0 and sum(d.device_markers_stats()[1] for d in s_on.decoders) == 0, "the option-on pipeline declined"
    assert bool((s_off.out == s_on.out).all()), "pixels differ"
    say(f"(b) pipeline over {args.batch} streams (chunks of 32, two decoder objects), ms per batch")
    say(f"    option off  {med(a)}")
    say(f"    option on   {med(b)}")
    s_off.close()
    s_on.close()
    return finish(args, lines)


def no_restart_markers(args, say, lines):
    """Parts na, nb, nc: streams without restart markers, option off against on."""
    import numpy as np

    def timed(f, per=1):
        def run():
            t0 = time.perf_counter()
            f()
            return (time.perf_counter() - t0) * 1e3 / per
        return run

    if args.part == "nc":
        rng = np.random.default_rng(64)
        sides = [(int(rng.integers(64, 1025)), int(rng.integers(64, 1025))) for _ in range(64)]
        pics = [synth.synth_jpeg(w, h, 700 + i, 85, ("420", "422", "444")[i % 3], 0 if i % 2 else 4) for i, (w, h) in enumerate(sides)]
        off, on = api.Decoder(0), api.Decoder(0)
        a, b = alternate(timed(lambda: batch.decode_mixed(pics, 0, decoder=off)), timed(lambda: batch.decode_mixed(pics, 0, decoder=on, device_markers=True)), args.reps)
        say(f"(c) decode_mixed over 64 pictures of 64 .. 1024 pixels a side, {sum(map(len, pics)) / 1e6:.2f} MB, ms per list; {api.lib().mijpeg_default_threads()} workers")
        say(f"    option off  {med(a)}")
        say(f"    option on   {med(b)}   searched, declined: {on.device_markers_stats()}; launches {off.ragged_stats()['entropy_launches']} / {on.ragged_stats()['entropy_launches']}")
        off.close()
        on.close()
        return finish(args, lines)
    kinds = {dri: [synth.synth_jpeg(3840, 2160, 500 + i, 85, "420", dri) for i in range(4)] for dri in ((0, 8) if args.part == "na" else (0,))}
    for dri, distinct in kinds.items():
        streams = [distinct[i % 4] for i in range(args.streams)]
        dev = None if args.part == "na" else 0
        off, on = api.Decoder(dev), api.Decoder(dev)
        on.set_device_markers(1)
        if args.part == "na":
            a, b = alternate(timed(lambda: off.prepare_batch_host(streams), len(streams)), timed(lambda: on.prepare_batch_host(streams), len(streams)), args.reps)
            say(f"(a) mijpeg_prepare_batch_host over {args.streams} 4K 4:2:0 Q85 DRI {dri} streams of {len(streams[0]) / 1e6:.2f} MB, ms per stream; "
                f"{api.lib().mijpeg_default_threads()} workers")
        else:
            a, b = alternate(timed(lambda: off.decode_batch_device(streams, 1)), timed(lambda: on.decode_batch_device(streams, 1)), args.reps)
            say(f"(b) mijpeg_decode_batch_device over {args.streams} 4K 4:2:0 Q85 DRI {dri} streams, bytes -> coefficients, ms per batch; "
                f"{api.lib().mijpeg_default_threads()} workers, walk rounds {off.device_walk_rounds()} / {on.device_walk_rounds()}")
        assert on.device_markers_stats()[1] == 0, "the option-on call declined"
        say(f"    option off  {med(a)}")
        say(f"    option on   {med(b)}")
        off.close()
        on.close()
    return finish(args, lines)


def finish(args, lines):
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X JPEG block-decode path (BASELINE.json metric).

A "step" is one pass of the hot path (fused dequant + IDCT + chroma upsample + YCbCr->RGB kernel) over one
batch of F synthetic 8K (7680x4320) 4:2:0 baseline frames whose int16 coefficient planes are already
resident in HBM; pixels are written to HBM.  value = decoded Mpixels/s over all ranks.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--frames F] [--size 8k|4k] [--dump-outputs DIR] [--full [--workload both|headline|batch4k]]

A plain run sets up, warms up, times the K steps and prints the line; nothing else.  --dump-outputs DIR then writes what the last
timed step computed as DIR/pixels.npy (float32, a fixed seeded sample of the output bytes; the inputs are seeded too, so two builds
can be compared output for output).  --full adds everything else: the check against the oracle, the side measurements below,
the CPU baselines and the profiler passes.

N > 1: one rank per GPU, RCCL barriers and scalar reductions only (frames are independent, nothing is exchanged).  Started
either by the driver through torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the environment) or plainly as
`python bench.py --gpus N`: without WORLD_SIZE the script starts its N ranks itself through
`torch.distributed.run --standalone` (`--launcher always` does that for N = 1 too: world 1 over RCCL).  More ranks asked
for than devices visible, or a WORLD_SIZE that contradicts --gpus, is an error -- never a silent run on fewer GPUs.
Rank 0 prints ONE JSON line.

With --full, beside the headline the same line carries
  "batch4k"        BASELINE config 4 as written: 256 distinct 4K 4:2:0 Q85 DRI=8 streams in host memory, image-sharded
                   over the ranks (strong scaling), bytes -> pixels in HBM, each rank on its share of the host cores;
  "roofline_dense" the headline launch on content that defeats the sparse shortcuts (every coefficient non-zero) and on
                   content beyond the 16-bit chroma gate (32-bit kernel flavour);
  roofline.traffic HBM bytes per launch from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over a child of this script
                   (null when rocprofv3 is not usable, e.g. when this process is itself being profiled).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# the ranks of one node share its cores: each rank's host pool (header parsing, marker search, host Huffman decoding) gets
# cores / world of them.  Must be in the environment before libmijpeg.so is loaded.
_WORLD = int(os.environ.get("WORLD_SIZE", "1"))
if _WORLD > 1:
    os.environ.setdefault("MIJPEG_THREADS", str(max(1, min(64, (os.cpu_count() or 1) // _WORLD))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from libjpeg_amd import api, sharding, synth  # noqa: E402

SIZES = {"8k": (7680, 4320), "4k": (3840, 2160)}
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
BYTES_PER_PIXEL_420 = 6.0  # int16 coefficients in (3 B/px) + interleaved RGB out (3 B/px)


def verify_against_oracle(frames):
    """The checker, AFTER a timed region: frames = [(device tensor of one frame's pixels, its JPEG stream)] -> True when every frame
    the timed launches wrote equals oracle.decode() of its stream, byte for byte (the oracle is never on the measured path)."""
    from oracle import oracle as O

    cache = {}
    ok = True
    for px, data in frames:
        key = id(data)
        if key not in cache:
            cache[key] = O.decode(data)
        exp = cache[key]
        got = px.cpu().numpy().reshape(-1)
        ok = ok and got.size == exp.size and bool(np.array_equal(got, exp.reshape(-1)))
    return ok


DUMP_SAMPLES = 8 << 20  # float32 values: 32 MB, under the 64 MB an output dump may take
DUMP_SEED = 5150


def dump_outputs(out, directory):
    """--dump-outputs: `out` (the device tensor the last timed step wrote) -> directory/pixels.npy, float32 values of its bytes at
    DUMP_SAMPLES positions drawn with DUMP_SEED, in ascending order (every byte when they fit): the same positions for the same
    arguments, so that the files of two builds compare element for element."""
    flat = out.reshape(-1)
    n = flat.numel()
    if n > DUMP_SAMPLES:
        idx = torch.randint(0, n, (DUMP_SAMPLES,), generator=torch.Generator().manual_seed(DUMP_SEED)).sort().values
        flat = flat[idx.to(flat.device)]
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "pixels.npy"), flat.to(torch.float32).cpu().numpy())


def cpu_baseline(jpeg_bytes, width, height):
    """Reference CPU path timed on this box's host cores (rank 0, N=1 only).  Uses oracle/_ref/jpeg (the
    real reference binary, kind 'reference') if it was built, else the oracle's C restatement ('port')."""
    from oracle import oracle as O

    mpix = width * height / 1e6
    if O.have_reference():
        tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
        with tempfile.TemporaryDirectory(dir=tmpdir) as d:
            src, dst = os.path.join(d, "in.jpg"), os.path.join(d, "out.ppm")
            with open(src, "wb") as f:
                f.write(jpeg_bytes)
            ts = []
            for _ in range(5):
                t = time.perf_counter()
                subprocess.run([O.REF_BIN, src, dst], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                ts.append(time.perf_counter() - t)
        best = sorted(ts)[len(ts) // 2]
        return dict(value=round(mpix / best, 2), unit="Mpixels/s", cores=1, kind="reference",
                    sample=f"5 whole-process decodes of one {width}x{height} 4:2:0 Q85 DRI=8 frame by oracle/_ref/jpeg "
                           f"(file in /dev/shm -> PPM in /dev/shm), median {best * 1e3:.0f} ms")
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        O.decode(jpeg_bytes)
        ts.append(time.perf_counter() - t)
    best = sorted(ts)[len(ts) // 2]
    return dict(value=round(mpix / best, 2), unit="Mpixels/s", cores=1, kind="port",
                sample=f"5 in-memory decodes of one {width}x{height} 4:2:0 frame by oracle/liboracle.so, median {best * 1e3:.0f} ms")


def drop_in_client(binary, jpeg_bytes, reps):
    """tools/cxx/stripe_loop.cpp: a C++ client of class JPEG decodes the frame from memory with ONE DisplayRectangle request and
    with the eight-line stripe loop of cmd/reconstruct.cpp (bitmap in host memory).  `binary` is that source linked with
    libmijpeg.so (libjpeg_amd/bin/stripe_loop) or with the reference library (oracle/_ref/stripe_loop_ref, cpu_baseline only)."""
    import re
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmpdir) as d:
        src = os.path.join(d, "in.jpg")
        with open(src, "wb") as f:
            f.write(jpeg_bytes)
        out = subprocess.run([binary, src, str(reps)], check=True, capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"Read ([0-9.]+) ms; whole frame in one request ([0-9.]+) ms.*stripe loop ([0-9.]+) ms.*first stripe ([0-9.]+) ms after Read.*\((equal|DIFFERENT)\)", out)
    if not m:
        return {"error": out[-300:]}
    return {"read_ms": float(m.group(1)), "whole_frame_request_ms": float(m.group(2)), "stripe_loop_ms": float(m.group(3)),
            "first_stripe_after_read_ms": float(m.group(4)), "both_ways_same_pixels": m.group(5) == "equal", "repetitions": reps,
            "note": "bytes in host memory -> Construct + Read + DisplayRectangle(s) + Destruct -> interleaved RGB in host memory, best of the "
                    "repetitions; stripe loop = 8 lines per request, the hook reports BIO_HEIGHT = miny + 8 (cmd/reconstruct.cpp, cmd/bitmaphook.cpp)"}


def cpu_baseline_all_cores(streams, width, height):
    """The reference on ALL host cores: `nproc` concurrent whole-process decodes of distinct frames (one process per core;
    the reference is single-threaded), aggregate Mpixels/s.  Output goes to /dev/null (writing the PPMs of hundreds of
    concurrent processes into /dev/shm would measure the page allocator); bounded by the memory the box has free."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import oracle as O

    if not O.have_reference():
        return None
    nproc = os.cpu_count() or 1
    try:
        with open("/proc/meminfo") as f:
            avail_kb = next(int(line.split()[1]) for line in f if line.startswith("MemAvailable"))
        per_proc = (width * height * 3 // 2) * 4 * 2 + width * height * 4  # LONG coefficient store + line buffers, generous
        nproc = max(1, min(nproc, int(avail_kb * 1024 * 0.5 / per_proc)))
    except (OSError, StopIteration, ValueError):
        pass
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmpdir) as d:
        files = []
        for i in range(nproc):
            fn = os.path.join(d, f"in{i}.jpg")
            with open(fn, "wb") as f:
                f.write(streams[i % len(streams)])
            files.append(fn)

        def one(fn):
            subprocess.run([O.REF_BIN, fn, "/dev/null"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

        # every core the box gives us, not only the socket this rank's threads were bound to: the launcher threads are created
        # by this thread and inherit its affinity, the reference processes inherit theirs
        bound = os.sched_getaffinity(0)
        os.sched_setaffinity(0, FULL_AFFINITY)
        try:
            best = None
            for _ in range(2):
                t = time.perf_counter()
                with ThreadPoolExecutor(nproc) as ex:
                    list(ex.map(one, files))
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
        finally:
            os.sched_setaffinity(0, bound)
    quota = cpu_quota_cpus()
    return dict(value=round(nproc * width * height / best / 1e6, 1), unit="Mpixels/s", cores=nproc, kind="reference", cpu_quota_cpus=quota,
                sample=f"{nproc} concurrent whole-process decodes of {min(nproc, len(streams))} distinct {width}x{height} 4:2:0 Q85 DRI=8 frames by "
                       f"oracle/_ref/jpeg (files in /dev/shm -> /dev/null), best of 2 rounds: {best * 1e3:.0f} ms; host has {os.cpu_count()} logical cores"
                       + (f", but the container's CPU quota (cgroup cpu.max) is {quota:g} CPUs' worth of time: that, not the core count, bounds this figure" if quota else ""))


def cpu_quota_cpus():
    """CPUs' worth of time per period the container may spend (cgroup v2 cpu.max, v1 cfs quota), None when unlimited / unknown."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else round(int(q) / int(p), 2)
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else round(q / p, 2)
    except (OSError, ValueError):
        return None


# ---- HBM traffic of the headline launch, measured where it is reported ------------------------------------------------
TRAFFIC_FRAMES = 8


def traffic_child(path):
    """Child process of measure_traffic(): 3 launches of the headline kernel on TRAFFIC_FRAMES frames whose coefficient planes
    the parent left in `path` -- nothing else, so that the rocprofv3 pass around it is short."""
    blob = np.load(path, allow_pickle=False)
    info = api.MijpegInfo.from_buffer_copy(blob["info"].tobytes())
    planes = torch.from_numpy(blob["planes"]).cuda()
    W, H, n = info.width, info.height, int(info.coef_count)
    coef = torch.empty((TRAFFIC_FRAMES, n), dtype=torch.int16, device="cuda")
    for f in range(TRAFFIC_FRAMES):
        coef[f].copy_(planes[f % planes.shape[0]])
    row = W * 3
    out = torch.empty((TRAFFIC_FRAMES, H, row), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), TRAFFIC_FRAMES, row, H * row, n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def measure_traffic(info, host_planes, kernel, frames):
    """roofline.traffic: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE: they do not fit one pass, MI355X_MICROARCH.md) over
    a child of this script, counters of `kernel` per launch, FETCH_SIZE doubled per the guide's gfx950 correction (wide
    coalesced reads are tallied at half their bytes), KB -> bytes, scaled from the child's TRAFFIC_FRAMES frames per launch
    to `frames`.  -> (bytes or None, note)."""
    import csv
    import glob
    import shutil

    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rocprof is None:
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCP_")) for k in os.environ):
        return None, "this process runs under rocprofv3 itself: no nested counter pass"
    try:
        tmp = tempfile.mkdtemp(prefix="mijpeg_traffic_", dir="/tmp" if os.path.isdir("/tmp") else None)
    except OSError as e:
        return None, f"no scratch directory for the counter passes: {e!r}"
    try:
        path = os.path.join(tmp, "planes.npz")
        np.savez(path, info=np.frombuffer(bytes(info), np.uint8), planes=np.stack(host_planes))
        vals = {}
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            outdir = os.path.join(tmp, ctr)
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
                env.pop(k, None)
            r = subprocess.run([rocprof, "--pmc", ctr, "--output-format", "csv", "-d", outdir, "-o", "t", "--", sys.executable,
                                os.path.abspath(__file__), "--traffic-child", path], cwd=tmp, env=env, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=240)
            got = []
            for fn in glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"), recursive=True):
                with open(fn) as fh:
                    for rowd in csv.DictReader(fh):
                        if kernel in rowd["Kernel_Name"] and rowd["Counter_Name"] == ctr:
                            got.append(float(rowd["Counter_Value"]))
            if not got:
                return None, f"rocprofv3 --pmc {ctr} produced no rows for {kernel} (exit {r.returncode})"
            vals[ctr] = sum(got) / len(got)
        per_launch = (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0
        note = (f"rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes run by this process over a child doing 3 launches of {TRAFFIC_FRAMES} "
                f"frames (FETCH_SIZE {vals['FETCH_SIZE']:.0f} KB doubled per the gfx950 correction, WRITE_SIZE {vals['WRITE_SIZE']:.0f} KB), "
                f"scaled x{frames}/{TRAFFIC_FRAMES}")
        return int(per_launch * frames / TRAFFIC_FRAMES), note
    except Exception as e:  # noqa: BLE001 -- the counters are a report, never a reason to lose the benchmark
        return None, f"traffic pass failed: {e!r}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- the headline launch on other content ------------------------------------------------------------------------------
def dense_roofline(info0, F, W, H, stream, steps):
    """The same launch (F frames, one kernel) on coefficient planes made on the device:
       "dense"       every one of the 64 coefficients of every block non-zero (+-1, +-2): no zero rows, no zero columns, nothing
                     for the sparse shortcuts of the transform, yet inside the 16-bit gates (same kernel as the headline);
       "beyond_gate" chroma amplitudes past the packed 16-bit gate (sum |c| q >= 2047 per block, what saturated graphics and
                     low-Q tables produce): the 32-bit flavour runs.
    fast_arith / range_max are computed from the planes exactly as the decoder computes them (max over the blocks of a
    component of sum_k |c_k| q_k), so the kernel selection is the one a stream with these coefficients would get."""
    res = {}
    n = int(info0.coef_count)
    row = W * 3
    out = torch.empty((F, H, row), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    # magnitudes (luma, chroma) and DC amplitude: with the Q85 tables (sum of the chroma deltas 1666) "dense" stays below the
    # packed-chroma gate of 2047, "beyond_gate" lands between 2047 and the 16384 of the fast arithmetic
    for name, hi_luma, hi_chroma, dc_amp in (("dense", 2, 1, 60), ("beyond_gate", 3, 3, 200)):
        info = api.MijpegInfo.from_buffer_copy(bytes(info0))
        one = torch.empty((2, n), dtype=torch.int16, device="cuda")
        for c in range(info.components):
            nb = info.blocks_w[c] * info.blocks_h[c]
            q = torch.tensor(list(info.quant[info.quant_index[c]]), dtype=torch.int32, device="cuda")
            mag = torch.randint(1, (hi_luma if c == 0 else hi_chroma) + 1, (2, nb, 64), generator=g, device="cuda", dtype=torch.int32)
            sgn = torch.randint(0, 2, (2, nb, 64), generator=g, device="cuda", dtype=torch.int32) * 2 - 1
            blk = mag * sgn
            blk[:, :, 0] = torch.randint(-dc_amp, dc_amp + 1, (2, nb), generator=g, device="cuda", dtype=torch.int32)
            info.range_max[c] = int((blk.abs() * q).sum(dim=2).max())
            off = int(info.coef_offset[c])
            one[:, off:off + nb * 64] = blk.reshape(2, -1).to(torch.int16)
        info.fast_arith = 1 if max(info.range_max[c] for c in range(info.components)) < 16384 else 0
        coef = torch.empty((F, n), dtype=torch.int16, device="cuda")
        for f in range(F):
            coef[f].copy_(one[f % 2])
        del one
        for _ in range(6):
            api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), F, row, H * row, n, stream=stream.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), F, row, H * row, n, stream=stream.cuda_stream)
        e1.record(stream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        alg = W * H * F * BYTES_PER_PIXEL_420
        ach = alg / (ms * 1e-3) / 1e9
        res[name] = {"kernel": api.kernel_name(info), "kernel_ms": round(ms, 4), "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(ach / HBM_PEAK_GBPS, 4), "value_Mpixels_s": round(W * H * F / ms / 1e3, 1),
                     "range_max": [int(info.range_max[c]) for c in range(info.components)], "fast_arith": int(info.fast_arith)}
        del coef
    res["note"] = ("same launch shape as the headline (frames, geometry, quantiser tables), coefficient planes synthesised on the device: "
                   "'dense' = all 64 coefficients of every block non-zero; 'beyond_gate' = chroma sum|c|q past 2047")
    return res


# ---- the headline launch on streams the REFERENCE encoder wrote --------------------------------------------------------
def reference_encoded_roofline(dec, F, W, H, stream, steps, seed):
    """SURVEY 8(d) wants the reference-encoded twin beside the Pillow streams: `jpeg -bl -q 85 -s 1x1,2x2,2x2 -z 8` of the same
    picture (the reference encoder quantises every component with table 0 and writes its own Huffman tables, so chroma
    range_max -- and possibly the kernel flavour -- differ).  oracle/_ref/jpeg only PREPARES the input here (untimed)."""
    from oracle import oracle as O

    if not O.have_reference():
        return {"skipped": "oracle/_ref/jpeg (the reference encoder) is not built on this box"}
    planes, info, sizes = [], None, []
    for i in range(2):
        data = O.reference_encode(synth.synth_image(W, H, seed + i), ["-bl", "-q", "85", "-s", "1x1,2x2,2x2", "-z", "8"])
        sizes.append(len(data))
        info = dec.read(data)
        planes.append(np.concatenate([dec.coefficients(c).reshape(-1) for c in range(info.components)]))
    n = int(info.coef_count)
    coef = torch.empty((F, n), dtype=torch.int16, device="cuda")
    for f in range(F):
        if f < 2:
            coef[f].copy_(torch.from_numpy(planes[f]))
        else:
            coef[f].copy_(coef[f % 2])
    row = W * 3
    out = torch.empty((F, H, row), dtype=torch.uint8, device="cuda")
    for _ in range(6):
        api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), F, row, H * row, n, stream=stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), F, row, H * row, n, stream=stream.cuda_stream)
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    ach = W * H * F * BYTES_PER_PIXEL_420 / (ms * 1e-3) / 1e9
    return {"encoder": "oracle/_ref/jpeg -bl -q 85 -s 1x1,2x2,2x2 -z 8 (input preparation only)", "stream_bytes": sizes,
            "kernel": api.kernel_name(info), "kernel_ms": round(ms, 4), "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(ach / HBM_PEAK_GBPS, 4), "value_Mpixels_s": round(W * H * F / ms / 1e3, 1),
            "range_max": [int(info.range_max[c]) for c in range(info.components)], "fast_arith": int(info.fast_arith),
            "quant_index": [int(info.quant_index[c]) for c in range(info.components)]}


# ---- BASELINE config 5: JPEG XT profile C, 4K HDR ----------------------------------------------------------------------
XT_ARGS = ["-r", "-q", "85", "-Q", "90", "-h", "-profile", "c", "-r12", "-s", "1x1,2x2,2x2"]


def xt_profile_c(local_rank, stream, with_cpu, frames=8, steps=10):
    """3840x2160 HDR (seed 99) coded by the reference encoder as JPEG XT profile C -- `-r -q 85 -Q 90 -h
    -profile c -r12`, and the same with four hidden residual bits (`-rR 4`: RFIN refinement scans, 16-bit residual samples).
    The reference encoder (oracle/_ref/jpeg) only PREPARES the input here, untimed; it is timed as cpu_baseline on the same
    stream.  Per variant: the reconstruction launch on `frames` device-resident frames (HIP events), bytes -> half-float codes
    in HBM, bytes -> float32 samples in host memory (what the reference's PFM writer gets), the entropy decode alone."""
    from oracle import oracle as O

    if not O.have_reference():
        return {"skipped": "oracle/_ref/jpeg (the reference encoder that writes the config 5 input) is not built on this box"}
    import ctypes as C

    W, H = SIZES["4k"]
    hdr = synth.synth_hdr(W, H, 99)
    res = {"input": f"{W}x{H} HDR, seed 99 (libjpeg_amd/synth.py synth_hdr = SURVEY 8d recipe), reference encoder `jpeg {' '.join(XT_ARGS)}` [+ -rR 4]"}
    hip = C.CDLL("libamdhip64.so")
    dec = api.Decoder(local_rank)
    # (-z 8: with restart intervals every hidden refinement scan decodes interval-parallel on the host instead of as one chain)
    for name, extra in (("r12", []), ("r12_rR4", ["-rR", "4"]), ("r12_rR4_z8", ["-rR", "4", "-z", "8"])):
        t = time.perf_counter()
        data = O.reference_encode_hdr(hdr, XT_ARGS + extra)
        enc_s = time.perf_counter() - t
        reads = {}
        for mode in ("host", "prefer-gpu"):
            ts = []
            for _ in range(4):
                t = time.perf_counter()
                dec.read(data, entropy=mode)
                ts.append(time.perf_counter() - t)
            reads[mode] = (min(ts) * 1e3, dec.entropy_used)
        info = dec.read(data, entropy="host")
        phases = {k: round(v * 1e3, 2) for k, v in dec.timing().items()}
        xt = dec.xt_params()
        n = int(info.coef_count)
        wide = bool(xt.residual_wide)
        F = frames
        coef = torch.empty((F, n), dtype=torch.int16, device="cuda")
        src = dec.device_coefficients()
        dec.synchronize()
        torch.cuda.synchronize()
        for f in range(F):
            assert hip.hipMemcpy(C.c_void_p(coef[f].data_ptr()), C.c_void_p(src), C.c_size_t(n * 2), 3) == 0
        row = W * 3 * 2
        out = torch.empty((F, H, row), dtype=torch.uint8, device="cuda")
        wsb = api.workspace_bytes(info, F, xt=xt)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")

        def step():
            api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), F, row, H * row, n, workspace=ws.data_ptr(), workspace_bytes=wsb,
                                   stream=stream.cuda_stream, xt=xt)

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:  # clocks
            step()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            step()
        e1.record(stream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        # algorithmic bytes per pixel: legacy 4:2:0 int16 coefficients 3 B + residual 4:4:4 coefficients (int16: 6 B; with hidden
        # bits they are 16-bit-precision samples' coefficients kept as int32: 12 B) + three half-float codes out 6 B.
        # SURVEY 8(d) prices config 5 at 21 B/px because it assumes the reference's int32 residual store; without hidden bits this
        # design stores the residual as int16 and is priced on what it moves (15): the smaller figure, i.e. the lower fraction.
        bpp = 3 + (12 if wide else 6) + 6
        ach = W * H * F * bpp / (ms * 1e-3) / 1e9
        kname = api.kernel_name(info, xt=xt)
        try:  # what the timed launches wrote (every frame is a copy of the same picture) against the oracle's half-float codes
            codes, _ = O.decode_xt(data)
            verified = all(bool(np.array_equal(out[i].cpu().numpy().view(np.uint16).reshape(codes.shape), codes)) for i in sorted({0, F // 2, F - 1}))
        except Exception as e:  # noqa: BLE001
            verified = repr(e)
        del coef, ws
        # bytes -> half codes left in HBM, bytes -> float32 in host memory
        dev_out = out[0]
        th, tf = [], []
        for _ in range(4):
            t = time.perf_counter()
            dec.read(data, entropy="prefer-gpu")
            dec.reconstruct_device(dev_out.data_ptr(), row)
            th.append(time.perf_counter() - t)
        host_f32 = torch.empty((H, W * 3), dtype=torch.float32).pin_memory()
        for _ in range(3):
            t = time.perf_counter()
            dec.read(data, entropy="prefer-gpu")
            dec.reconstruct_device(dev_out.data_ptr(), row)
            # half codes -> float32 is exact (every half is a float; the reference's client does it per sample, cmd/iohelpers.hpp:60-77);
            # here the expansion runs on the device (torch: plumbing) and 4 bytes per sample come down
            host_f32.copy_(dev_out.view(torch.float16).to(torch.float32), non_blocking=True)
            torch.cuda.synchronize()
            tf.append(time.perf_counter() - t)
        del out, host_f32
        ent = {"variant": "jpeg " + " ".join(XT_ARGS + extra), "stream_bytes": len(data), "reference_encode_s": round(enc_s, 1),
               "kernel": kname, "frames": F, "kernel_ms": round(ms, 4), "value": round(W * H * F / ms / 1e3, 1), "unit": "Mpixels/s",
               "verified": verified,
               "roofline": {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBPS, 4),
                            "bytes_per_pixel": bpp, "residual_coefficients": "int32" if wide else "int16"},
               "residual_hidden_bits": int(xt.residual_hidden_bits), "legacy_hidden_bits": int(xt.hidden_bits),
               "entropy_decode_ms": {"host": round(reads["host"][0], 2), "host_phases_ms": phases, "host_threads": api.default_threads(),
                                     "prefer_gpu": round(reads["prefer-gpu"][0], 2), "prefer_gpu_ran_on": reads["prefer-gpu"][1]},
               "bytes_to_half_codes_in_hbm": {"ms": round(min(th) * 1e3, 2), "value": round(W * H / min(th) / 1e6, 1), "unit": "Mpixels/s"},
               "bytes_to_float32_in_host_memory": {"ms": round(min(tf) * 1e3, 2), "value": round(W * H / min(tf) / 1e6, 1), "unit": "Mpixels/s",
                                                   "note": "read + kernels + half -> float32 expansion on the device + D2H of 4 bytes per sample into pinned host memory"}}
        if with_cpu:
            tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
            with tempfile.TemporaryDirectory(dir=tmpdir) as dd:
                srcf, dstf = os.path.join(dd, "in.jpg"), os.path.join(dd, "out.pfm")
                with open(srcf, "wb") as fh:
                    fh.write(data)
                ts = []
                for _ in range(3):
                    t = time.perf_counter()
                    subprocess.run([O.REF_BIN, srcf, dstf], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                    ts.append(time.perf_counter() - t)
            med = sorted(ts)[1]
            ent["cpu_baseline"] = {"value": round(W * H / med / 1e6, 2), "unit": "Mpixels/s", "cores": 1, "kind": "reference",
                                   "sample": f"3 whole-process decodes of this stream by oracle/_ref/jpeg (/dev/shm -> PFM in /dev/shm), median {med * 1e3:.0f} ms"}
        res[name] = ent
    # the refinement scans of the -rR variant are decoded by the host (codestream/refinementscan.cpp:584-700: 49 % of the reference's
    # XT decode); what they cost here = host entropy decode with them minus without
    res["host_refinement_decode_ms"] = round(res["r12_rR4"]["entropy_decode_ms"]["host"] - res["r12"]["entropy_decode_ms"]["host"], 2)
    dec.close()
    return res


# ---- config 4 as one rank of an N-rank job would see it, on one GPU -----------------------------------------------------
def emulate_world_child(n_world, stream_dir, frames_total, steps):
    """Runs in a child of bench.py whose environment carries MIJPEG_THREADS = cores / n_world: rank 0's REAL share of the batch
    (frames 0, N, 2N, ...: bytes -> pixels in HBM on this GPU, its host pool cut to a rank's share, bound to the GPU's NUMA
    node) while N - 1 host-only neighbours (libjpeg_amd/batch.py host_load_worker) keep doing their ranks' host work on the
    remaining cores -- ranks 1 .. N/2 - 1 on this socket, the others on the rest, as on an 8-GPU node with four GPUs per socket."""
    from libjpeg_amd import batch

    torch.cuda.set_device(0)
    full = sorted(int(c) for c in os.environ["MIJPEG_EMU_ALL_CPUS"].split(",")) if os.environ.get("MIJPEG_EMU_ALL_CPUS") else sorted(os.sched_getaffinity(0))
    binding = None if os.environ.get("MIJPEG_BENCH_NO_NUMA") else sharding.bind_to_gpu_node(0)
    near = sorted(os.sched_getaffinity(0)) # (the parent may have bound itself -- and so this child -- already)
    far = [c for c in full if c not in set(near)] or near
    mine = sharding.frames_of_rank(frames_total, 0, n_world)
    streams = {}
    for i in mine:
        with open(os.path.join(stream_dir, f"{i}.jpg"), "rb") as f:
            streams[i] = f.read()
    env = dict(os.environ, MIJPEG_NO_TORCH="1")
    procs = []
    seconds = 12.0
    for r in range(1, n_world):
        cpus = near if r < max(1, n_world // 2) else far
        procs.append(subprocess.Popen([sys.executable, "-m", "libjpeg_amd.batch", "--host-load", stream_dir, str(r), str(n_world), str(frames_total),
                                       str(seconds), ",".join(map(str, cpus))], env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True))
    time.sleep(2.5)  # the neighbours are loaded and looping
    best, tried = None, []
    t_begin = time.perf_counter()
    for chunk, depth, ramp in ((8, 4, False), (11, 3, False), (16, 3, False), (16, 2, False)):
        if time.perf_counter() - t_begin > seconds - 5.0:
            break
        r = batch.run_sharded(streams, frames_total, 0, n_world, 0, None, steps=steps, warmup=3, chunk=chunk, depth=depth, ramp=ramp)
        r["shard"].close()
        ms = r["seconds"] * 1e3 / steps
        tried.append({"chunk_frames": chunk, "decoder_objects": depth, "ramp": ramp, "ms": round(ms, 3)})
        if best is None or ms < best:
            best = ms
    loaded_until = time.perf_counter() - t_begin
    passes = []
    for p in procs:
        out, _ = p.communicate(timeout=60)
        passes.append(int(out.strip().splitlines()[-1]) if out.strip() else -1)
    W, H = SIZES["4k"]
    print(json.dumps({"world": n_world, "rank0_frames": len(mine), "rank0_ms": round(best, 3), "settings_tried": tried,
                      "projected_value": round(frames_total * W * H / (best * 1e-3) / 1e6, 1), "unit": "Mpixels/s",
                      "host_threads": api.default_threads(), "numa_binding": binding or {"inherited_cpus": len(near)},
                      "neighbours_on_this_socket": max(1, n_world // 2) - 1, "neighbours_elsewhere_cpus": len(far) if far is not near else 0,
                      "neighbour_passes": passes,
                      "measured_while_neighbours_ran": bool(loaded_until < seconds - 2.5)}))


def emulate_world(n_world, streams, frames_total, steps):
    """Parent side: the batch's streams go to /dev/shm, the child (own MIJPEG_THREADS, own HIP context) does the rest."""
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmpdir, prefix="mijpeg_emu_") as d:
        for i, data in streams.items():
            with open(os.path.join(d, f"{i}.jpg"), "wb") as f:
                f.write(data)
        env = dict(os.environ, MIJPEG_THREADS=str(max(1, min(64, (os.cpu_count() or 1) // n_world))),
                   MIJPEG_EMU_ALL_CPUS=",".join(map(str, sorted(FULL_AFFINITY))))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emulate-world-child", str(n_world), "--emulate-dir", d,
                            "--batch-frames", str(frames_total), "--batch-steps", str(steps)], env=env, capture_output=True, text=True, timeout=180)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": (r.stderr or r.stdout)[-400:]}
    res = json.loads(lines[-1])
    res["note"] = (f"PROJECTED, not measured on {n_world} GPUs: one GPU runs rank 0's share of the {frames_total}-frame batch with a rank's share of the host "
                   f"(cores / {n_world} pool threads, NUMA-bound) while {n_world - 1} host-only processes do the other ranks' parsing / marker search / "
                   "gathering on the remaining cores; projected_value = all frames / rank 0's time (ranks are symmetric, no data-path collective)")
    return res


# ---- BASELINE config 4 ----------------------------------------------------------------------------------------------------
NUMA_BINDING = None  # what sharding.bind_to_gpu_node did for this rank (main() sets it)
FULL_AFFINITY = os.sched_getaffinity(0)  # before any binding: the CPU baselines run on all of it


def batch4k(rank, world, local_rank, dist, steps, frames_total, with_cpu, emulate_n=0):
    """256 x 4K 4:2:0 Q85 DRI=8 (seeds 1000..1255), image-sharded, bytes in host memory -> pixels in HBM; strong scaling."""
    from libjpeg_amd import batch

    cfg = dict(batch.CONFIG4, frames=frames_total)
    mine = sharding.frames_of_rank(frames_total, rank, world)
    t = time.perf_counter()
    streams = batch.make_streams(mine, cfg, workers=max(1, min(64, (os.cpu_count() or 1) // (2 * world))))
    gen_s = time.perf_counter() - t
    best = None
    tried = []
    # (the clock governor needs ~100 ms of load to settle, DESIGN 5: the first setting warms up for that long, untimed)
    # (pipeline settings worth trying depend on how many frames a rank has: with 256 / 8 = 32 of them, chunks of 16 would leave
    # the pipeline two stages deep)
    # (chunk frames, decoder objects, ramped schedule: small chunks at both ends of the batch -- libjpeg_amd/batch.py)
    settings = (((24, 4, False), (28, 4, True), (32, 4, True), (24, 4, True), (32, 4, False)) if len(mine) >= 128 else
                # (no setting with two objects: the upload engine then idles whenever the host's one wait per chunk returns late, and on
                # most boxes that is the case for the first hundred chunks of a shard -- profiles/r05/batch4k_stall.txt)
                ((8, 4, True), (8, 4, False), (11, 3, False), (16, 3, False), (4, 8, False), (max(1, len(mine)), 1, False)))
    for ci, (chunk, depth, ramp) in enumerate(settings):
        r = batch.run_sharded(streams, frames_total, rank, world, local_rank, dist, steps=steps, warmup=10 if ci == 0 else 2, chunk=chunk, depth=depth,
                              ramp=ramp)
        if ci + 1 < len(settings):
            r["shard"].close()
            r.pop("shard")
        r.update(chunk=chunk, depth=depth, ramp=ramp)
        sm = sorted(r["step_ms"])
        r["median_ms"] = sm[len(sm) // 2]
        tried.append({"chunk_frames": chunk, "decoder_objects": depth, "ramp": ramp, "ms_per_batch": round(r["seconds"] * 1e3 / steps, 2),
                      "median_ms": round(r["median_ms"], 2), "step_ms": [round(x, 2) for x in r["step_ms"]]})
        # (the setting is chosen by its median step: one pass in twenty takes 6-8 ms longer on some boxes -- same device work, host
        # side, profiles/r05/batch4k_stall.txt -- and with five steps a mean would pick the setting that happened not to meet one)
        if best is None or r["median_ms"] < best["median_ms"]:
            best = r
    last_shard = r.pop("shard")
    verified = None
    try:  # three frames of what the last timed batch left in HBM, against the oracle
        o = last_shard.out
        verified = verify_against_oracle([(o[i], streams[mine[i]]) for i in sorted({0, 1, len(mine) - 1})])
    except Exception as e:  # noqa: BLE001
        verified = repr(e)
    W, H = cfg["width"], cfg["height"]
    ms = best["seconds"] * 1e3 / steps
    rank_ms = [best["rank_ms"]]
    rank_threads = [api.default_threads()]
    rank_verified = [verified is True]
    if dist is not None:
        # per rank: its milliseconds, the size of its host pool, and whether ITS frames equal the oracle's (a rank that decoded
        # something else fails the whole line)
        tt = torch.zeros((3, world), dtype=torch.float64, device="cuda")
        tt[0, rank] = best["rank_ms"]
        tt[1, rank] = api.default_threads()
        tt[2, rank] = 1.0 if verified is True else 0.0
        dist.all_reduce(tt)
        rank_ms = [float(x) for x in tt[0]]
        rank_threads = [int(x) for x in tt[1]]
        rank_verified = [bool(x > 0.5) for x in tt[2]]
        if verified is True and not all(rank_verified):
            verified = f"frames differ from the oracle on rank(s) {[r for r, ok in enumerate(rank_verified) if not ok]}"
    quota = cpu_quota_cpus()
    res = {"metric": "decoded Mpixels/s, 256 x 4K 4:2:0 Q85 DRI=8 streams in host memory -> pixels in HBM (BASELINE configs[3])",
           "value": round(best["total_pixels"] / best["seconds"] / 1e6, 1), "unit": "Mpixels/s", "scaling": "strong", "n_gpus": world,
           "frames": frames_total, "frames_per_rank": len(mine), "ms_per_batch": round(ms, 2), "ms_per_frame": round(ms / frames_total, 4),
           "median_ms_per_batch": round(best["median_ms"], 2), "step_ms": [round(x, 2) for x in best["step_ms"]],
           "verified": verified,
           "per_rank_ms": [round(x, 2) for x in rank_ms], "steps": steps, "chunk_frames": best["chunk"], "decoder_objects": best["depth"],
           "ramped_schedule": best["ramp"],
           "per_rank_verified": rank_verified, "per_rank_host_threads": rank_threads,
           "host_threads_per_rank": api.default_threads(), "host_cores": os.cpu_count(), "cpu_quota_cpus": quota,
           "cpu_quota_cpus_per_rank": None if quota is None else round(quota / world, 2),
           "stream_bytes_total": int(sum(len(v) for v in streams.values())) if world == 1 else None,
           "generation_s": round(gen_s, 1), "settings_tried": tried, "numa_binding": NUMA_BINDING,
           "note": "per rank: `decoder_objects` decoder objects driven round-robin by one thread, `chunk_frames` frames each: parallel header parse + "
                   "restart marker search + gather into pinned memory (host pool = cores / ranks) while the previous chunks' H2D of the compressed "
                   "bytes, huffman_scan_kernel and fused kernel run on their streams; pixels stay in HBM; RCCL barriers around the timed "
                   "region only; max over ranks"}
    # the other end of config 4: the tag / hook API's consumer is HOST memory.  The decoded frames of the last shard go back
    # over PCIe in slabs of 32 into one pinned buffer a client would recycle; not overlapped with the decode (the download is
    # more than ten times the decode, so an overlapped pipeline would be bound by it just the same).
    try:
        out = last_shard.out
        slab = min(32, out.shape[0])
        pinned = torch.empty((slab,) + tuple(out.shape[1:]), dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        best_dl = None
        for _ in range(2):
            t = time.perf_counter()
            for a in range(0, out.shape[0], slab):
                b = min(out.shape[0], a + slab)
                pinned[:b - a].copy_(out[a:b], non_blocking=True)
                torch.cuda.synchronize()
            dt = time.perf_counter() - t
            best_dl = dt if best_dl is None else min(best_dl, dt)
        nbytes = out.numel()
        per_rank_decode_s = best["seconds"] / steps
        res["pixels_to_host"] = {"download_ms": round(best_dl * 1e3, 2), "download_GBps": round(nbytes / best_dl / 1e9, 1),
                                 "bytes": int(nbytes), "frames": int(out.shape[0]),
                                 "value": round(out.shape[0] * W * H / (per_rank_decode_s + best_dl) / 1e6, 1), "unit": "Mpixels/s",
                                 "note": "this rank's frames: bytes -> pixels in HBM (above) + D2H of the interleaved RGB frames into pinned host memory, "
                                         "32 frames at a time, decode and download not overlapped; the link carries 18 x more bytes down than up"}
        del pinned
        # ... and with both directions of the link in use: every chunk's pixels go down behind its reconstruction kernel while
        # the later chunks' bytes go up (BatchShard.run(download_to=...), mijpeg_stream_wait)
        full = torch.empty(tuple(out.shape), dtype=torch.uint8).pin_memory()
        best_fd = None
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            last_shard.run(download_to=full)
            dt = time.perf_counter() - t
            best_fd = dt if best_fd is None else min(best_fd, dt)
        ok = bool(torch.equal(full[-1], out[-1].cpu()) and torch.equal(full[0], out[0].cpu()))
        res["pixels_to_host"]["full_duplex"] = {
            "ms": round(best_fd * 1e3, 2), "value": round(out.shape[0] * W * H / best_fd / 1e6, 1), "unit": "Mpixels/s",
            "of_download_alone": round(best_fd / best_dl, 3), "chunk_frames": last_shard.chunk, "decoder_objects": last_shard.depth,
            "host_copy_equals_device": ok,
            "note": "bytes in host memory -> pixels in pinned host memory, one pass: the download of chunk i runs under the upload, the "
                    "Huffman kernel and the reconstruction of chunks i+1.. (a download stream waits for the decoder object's stream, "
                    "not the host); the batch takes the download's time instead of decode + download"}
        del full
    except Exception as e:  # noqa: BLE001
        res["pixels_to_host"] = {"error": repr(e)}
    last_shard.close()
    if emulate_n > 1 and rank == 0 and world == 1 and frames_total % emulate_n == 0:
        try:
            res[f"emulated_world{emulate_n}"] = emulate_world(emulate_n, streams, frames_total, steps)
        except Exception as e:  # noqa: BLE001
            res[f"emulated_world{emulate_n}"] = {"error": repr(e)}
    if with_cpu and rank == 0 and world == 1:
        try:
            some = [streams[i] for i in mine[:min(len(mine), os.cpu_count() or 1)]]
            res["cpu_baseline"] = cpu_baseline_all_cores(some, W, H)
        except Exception as e:  # noqa: BLE001
            res["cpu_baseline"] = {"value": None, "error": repr(e)}
    return res


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: become one.  N ranks of this very command line through
    torch.distributed.run --standalone on 127.0.0.1 (the container's hostname may not resolve); returns its exit code."""
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n:
        raise SystemExit(f"bench.py: --gpus {n} but {have} device(s) visible: not running on fewer GPUs than asked for")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: what RCCL needs on these hosts)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={n}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64, help="frames per step (= one kernel launch) and rank, device resident")
    ap.add_argument("--settle-ms", type=float, default=150.0,
                    help="untimed launches before the warmup steps: MI355X power management needs ~50 ms of sustained load "
                         "before the clock settles (profiles/r01/step_times.txt); 0 disables")
    ap.add_argument("--size", default="8k", choices=sorted(SIZES))
    ap.add_argument("--subsampling", default="420", choices=["420", "444"], help="420 = the BASELINE workload; 444 for side measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--no-traffic", action="store_true", help="skip the rocprofv3 --pmc child passes (roofline.traffic = null)")
    ap.add_argument("--no-dense", action="store_true", help="skip roofline_dense")
    ap.add_argument("--no-xt", action="store_true", help="skip xt_profile_c (BASELINE config 5)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the check against the oracle, the side measurements, the CPU baselines and the profiler passes "
                         "(the --no-* switches and --workload select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last one computed to DIR/pixels.npy (float32, a fixed seeded sample)")
    ap.add_argument("--workload", default="both", choices=["both", "headline", "batch4k"],
                    help="with --full: headline = the 8K kernel benchmark only; batch4k adds BASELINE config 4 (256 x 4K streams -> pixels, sharded)")
    ap.add_argument("--batch-frames", type=int, default=256, help="frames of the config 4 batch (256 as written)")
    ap.add_argument("--batch-steps", type=int, default=5)
    ap.add_argument("--traffic-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--emulate-world", type=int, default=8,
                    help="with N = 1: also run rank 0's share of config 4 as one rank of this many would see it (host-only neighbours load the "
                         "other cores) and report the PROJECTED aggregate; 0 disables")
    ap.add_argument("--emulate-world-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--emulate-dir", default="", help=argparse.SUPPRESS)
    ap.add_argument("--launcher", default="auto", choices=["auto", "always", "never"],
                    help="auto: with --gpus N > 1 and no WORLD_SIZE in the environment, start the N ranks through torch.distributed.run "
                         "--standalone; always: also for N = 1 (one rank over RCCL); never: run as the single process this is")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be at least 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be at least 1 and --warmup at least 0")
    launched = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if not launched and not args.traffic_child and not args.emulate_world_child and \
            (args.launcher == "always" or (args.launcher == "auto" and args.gpus > 1)):
        sys.exit(launch_ranks(args.gpus))
    if launched and int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks")
    if not launched and args.gpus > 1:
        raise SystemExit(f"bench.py: --gpus {args.gpus} with --launcher never and no WORLD_SIZE: refusing to report {args.gpus} GPUs from one process")
    if args.traffic_child:
        traffic_child(args.traffic_child)
        return
    if args.emulate_world_child:
        emulate_world_child(args.emulate_world_child, args.emulate_dir, args.batch_frames, args.batch_steps)
        return

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the reconstruction path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    # one process per GPU, on the socket its GPU hangs off (before the library creates its worker pool); MIJPEG_BENCH_NO_NUMA=1: as is
    global NUMA_BINDING
    NUMA_BINDING = None if os.environ.get("MIJPEG_BENCH_NO_NUMA") else sharding.bind_to_gpu_node(local_rank)
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants device {local_rank}, {torch.cuda.device_count()} visible")
    dist = None
    if world > 1 or launched:  # (a launched world of one still runs its barriers and reductions over RCCL)
        import torch.distributed as dist_

        dist = dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    W, H = SIZES[args.size]
    F = args.frames
    # ---- workload: F frames per rank, two distinct pictures per rank, coefficient planes in HBM ----------
    dec = api.Decoder(local_rank)
    host_planes, jpegs = [], []
    info = None
    for i in range(2):
        data = synth.synth_jpeg(W, H, seed=1234 + 17 * rank + i, quality=85, subsampling=args.subsampling, restart_mcus=8)
        jpegs.append(data)
        info = dec.read(data)
        host_planes.append(np.concatenate([dec.coefficients(c).reshape(-1) for c in range(info.components)]))
    n = int(info.coef_count)
    coef = torch.empty((F, n), dtype=torch.int16, device="cuda")
    for f in range(F):
        if f < 2:
            coef[f].copy_(torch.from_numpy(host_planes[f]))
        else:
            coef[f].copy_(coef[f % 2])
    row = W * 3
    out = torch.empty((F, H, row), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()

    def step():
        api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), F, row, H * row, n, stream=stream.cuda_stream)

    # bring the device to its steady-state clock (untimed, disclosed in config.settle_launches)
    settle_launches = 0
    if args.settle_ms > 0:
        torch.cuda.synchronize()
        t_settle = time.perf_counter()
        while (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
            for _ in range(4):
                step()
            settle_launches += 4
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed_steps():
        ev0.record(stream)
        for _ in range(args.steps):
            step()
        ev1.record(stream)
        return W * H * F * args.steps

    # barrier + torch.cuda.synchronize() on both sides, MAX over ranks of the elapsed time (libjpeg_amd/sharding.py)
    wall, pixels = sharding.timed_region(timed_steps, dist)
    kernel_ms = ev0.elapsed_time(ev1) / args.steps  # HIP events on the launch stream: one kernel per step
    total_pixels, wall = sharding.reduce_result(pixels, wall, dist)
    if dist:
        t = torch.tensor([kernel_ms], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        kernel_ms = float(t[0])
    assert total_pixels == W * H * F * args.steps * world

    if rank == 0 and args.dump_outputs:
        dump_outputs(out, args.dump_outputs)
    # what the timed launches wrote, against the oracle (rank 0's frames; after the timed region, never part of it)
    verified = None
    if rank == 0 and args.full:
        try:
            verified = verify_against_oracle([(out[i], jpegs[i % 2]) for i in sorted({0, 1, F - 1})])
        except Exception as e:  # noqa: BLE001 -- reported, never hidden
            verified = repr(e)
    pixels_per_step = W * H * F * world
    ms_per_step = wall * 1e3 / args.steps
    value = pixels_per_step / (ms_per_step * 1e-3) / 1e6
    bpp = BYTES_PER_PIXEL_420 if args.subsampling == "420" else 9.0  # 4:4:4: 3 x 2 B in + 3 B out
    alg_bytes = W * H * F * bpp  # per launch (one rank)
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9

    result = {
        "metric": "decoded Mpixels/s, 8K 4:2:0 baseline (fused IDCT+upsample+YCbCr kernel, coefficients resident in HBM)",
        "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "int32 (int16 coefficients in, u8 pixels out)", "data": "synthetic",
        "config": {"workload": f"{F} x {W}x{H} {args.subsampling[0]}:{args.subsampling[1]}:{args.subsampling[2]} Q85 DRI=8 baseline frames per GPU per step (BASELINE configs[2] frame shape, "
                               f"device-resident coefficient planes; 2 distinct pictures per rank repeated over the {F} frames: {F * n * 2 >> 20} MiB in + "
                               f"{F * H * row >> 20} MiB out per launch, far beyond the 256 MiB Infinity Cache)", "frames_per_gpu": F, "kernel": api.kernel_name(info), "settle_launches": settle_launches,
                   "fast_arith": int(info.fast_arith), "parallelism": f"image-sharded x{world}, no data-path collective",
                   "verified": verified},
        "verified": verified,
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None,
                     "kernel_ms": round(kernel_ms, 4), "algorithmic_bytes_per_launch": int(alg_bytes), "verified": verified},
    }
    result["launch"] = {"launched_by": "torch.distributed.run" if launched else "single process", "world": world,
                        "collectives": dist.get_backend() if dist else None, "visible_devices": torch.cuda.device_count()}
    result["verified_note"] = ("frames 0, 1 and F-1 of the output the timed launches wrote, downloaded after the timed region and compared byte for byte "
                               "with oracle.decode() of their streams (oracle/: the checker, never on the measured path)" if args.full else
                               "not checked: the check against the oracle runs with --full")

    if args.full and rank == 0 and world == 1 and not args.no_traffic:
        tb, tnote = measure_traffic(info, host_planes, api.kernel_name(info), F)
        result["roofline"]["traffic"] = tb
        result["roofline"]["traffic_note"] = tnote
    else:
        result["roofline"]["traffic_note"] = "not measured in this run (N > 1, --no-traffic or no --full)"
    # what HBM gives this launch's traffic without the arithmetic (a side measurement: never fails the line)
    mb = os.path.join(ROOT, "tools", "microbench", "stream_ceiling")
    if args.full and rank == 0 and world == 1 and not args.no_traffic and args.subsampling == "420" and os.path.exists(mb):
        try:
            torch.cuda.synchronize()
            t = json.loads(subprocess.run([mb, "--brief"], capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
            result["roofline"]["traffic_only"] = {
                "pattern_ms_per_8_frames": t["pattern_ms"], "pattern_frac": t["pattern_frac"], "copy_ms_per_8_frames": t["copy_ms"], "copy_frac": t["copy_frac"],
                "kernel_ms_per_8_frames": round(kernel_ms * 8 / F, 4), "pieces_frac": t.get("pieces_frac"),
                "note": "tools/microbench/stream_ceiling --brief on the same GPU right after the timed steps: 'pattern' = the fused kernel's loads and stores (tile shape, "
                        "tile order, halo re-reads, a line's pixels through LDS and out as 16 contiguous non-temporal bytes per lane) with no arithmetic between them; "
                        "'pieces' = the same with the 24-byte line pieces the kernel stored until the end of round 6; 'copy' = the best of three grid sizes of a plain "
                        "16-byte-per-lane copy of the same 3 + 3 bytes per pixel; fractions of the same 8 TB/s"}
        except Exception as e:  # noqa: BLE001
            result["roofline"]["traffic_only"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_dense and args.subsampling == "420":
        try:
            result["roofline_dense"] = dense_roofline(info, F, W, H, stream, max(5, args.steps // 2))
        except Exception as e:  # noqa: BLE001
            result["roofline_dense"] = {"error": repr(e)}
        try:
            result["roofline_reference_encoded"] = reference_encoded_roofline(dec, F, W, H, stream, max(5, args.steps // 2), 1234 + 17 * rank)
        except Exception as e:  # noqa: BLE001
            result["roofline_reference_encoded"] = {"error": repr(e)}

    # config 4 comes before the single-rank side measurements: with N > 1 every rank takes part in it, and nobody waits for rank 0
    if args.full and args.workload in ("both", "batch4k"):
        del coef, out
        torch.cuda.empty_cache()
        try:
            b4 = batch4k(rank, world, local_rank, dist, args.batch_steps, args.batch_frames, not args.no_cpu_baseline, args.emulate_world)
            result["batch4k"] = b4
        except Exception as e:  # noqa: BLE001 -- all ranks take the same path: a failure here is symmetric
            result["batch4k"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_end_to_end:
        # whole decode of one frame through the decoder object: host Huffman (all cores) + streaming H2D +
        # kernel + D2H into host memory.  PCIe/host inclusive -- reported beside, never as `value`.
        user = np.empty((H, W, 3), np.uint8)
        user[:] = 0  # touch the pages once: a real client reuses its frame buffer
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            dec.read(jpegs[0])
            dec.reconstruct(out=user)
            ts.append(time.perf_counter() - t)
        tm = dec.timing()
        best = min(ts)
        result["end_to_end"] = {"value": round(W * H / best / 1e6, 1), "unit": "Mpixels/s", "ms": round(best * 1e3, 2),
                                "host_threads": api.default_threads(), "host_cores": os.cpu_count(), "cpu_quota_cpus": cpu_quota_cpus(),
                                "phases_ms": {k: round(v * 1e3, 2) for k, v in tm.items()},
                                "note": "one frame, PCIe and host inclusive: bytes -> host Huffman (restart-interval parallel) -> "
                                        "pinned H2D (streamed) -> kernel -> D2H -> copy into the caller's interleaved bitmap"}
    if args.full and rank == 0 and world == 1 and not args.no_end_to_end:
        # the drop-in boundary from a client's seat: class JPEG through its hooks, one request and the reference CLI's stripe loop
        client = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libjpeg_amd", "bin", "stripe_loop")
        try:
            result["end_to_end"]["drop_in_client"] = drop_in_client(client, jpegs[0], 6) if os.path.exists(client) else {"skipped": "libjpeg_amd/bin/stripe_loop is not built"}
        except Exception as e:  # noqa: BLE001 -- a side measurement never costs the headline number
            result["end_to_end"]["drop_in_client"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_end_to_end:
        # the same, pipelined over a batch of frames (config 4's end-to-end shape): two decoder objects / streams
        from libjpeg_amd import pipeline

        nb = 24
        pipe = pipeline.FramePipeline(local_rank, depth=2, entropy="host")
        pipe.run([jpegs[i % 2] for i in range(4)])  # warm: pinned buffers, worker threads
        t = time.perf_counter()
        pipe.run([jpegs[i % 2] for i in range(nb)])
        dt = time.perf_counter() - t
        pipe.close()
        result["end_to_end"]["pipelined"] = {"value": round(W * H * nb / dt / 1e6, 1), "unit": "Mpixels/s", "frames": nb,
                                             "ms_per_frame": round(dt / nb * 1e3, 2), "depth": 2,
                                             "note": "two decoder objects / streams, D2H straight into pinned frames; bound by the ~200 MB per 8K frame that cross PCIe"}
    if args.full and rank == 0 and world == 1 and not args.no_end_to_end:
        # the same with the entropy decoding on the device (restart intervals in parallel, csrc/huffman.hip): only the
        # compressed bytes go up.  One frame to host memory, one frame left in HBM, and the two-deep pipeline.
        ts, tr = [], []
        for _ in range(5):
            t = time.perf_counter()
            dec.read(jpegs[0], entropy="gpu")
            t1 = time.perf_counter()
            dec.reconstruct(out=user)
            ts.append(time.perf_counter() - t)
            tr.append(t1 - t)
        dev_out = torch.empty((H, row), dtype=torch.uint8, device="cuda")
        th = []
        for _ in range(5):
            t = time.perf_counter()
            dec.read(jpegs[0], entropy="gpu")
            dec.reconstruct_device(dev_out.data_ptr(), row)
            th.append(time.perf_counter() - t)
        best_dt, best_depth = None, 0
        for depth in (2, 3):
            pipe = pipeline.FramePipeline(local_rank, depth=depth, entropy="gpu")
            pipe.run([jpegs[i % 2] for i in range(4)])
            t = time.perf_counter()
            pipe.run([jpegs[i % 2] for i in range(nb)])
            dt = time.perf_counter() - t
            pipe.close()
            if best_dt is None or dt < best_dt:
                best_dt, best_depth = dt, depth
        dt = best_dt
        # batch of frames: one Huffman launch + one reconstruction launch, pixels left in HBM (mijpeg_decode_batch_device)
        nbatch = 32
        bdec = api.Decoder(local_rank)
        bout = torch.empty((nbatch, H, row), dtype=torch.uint8, device="cuda")
        tb = []
        for _ in range(4):
            t = time.perf_counter()
            bdec.decode_batch_device([jpegs[i % 2] for i in range(nbatch)])
            bdec.reconstruct_batch_device(bout.data_ptr(), H * row, row)
            tb.append(time.perf_counter() - t)
        # ... and the same 32 frames through the software pipeline of the batch path (libjpeg_amd/batch.py: several decoder
        # objects driven round-robin, submit / finish halves of the batch entry points)
        del bout
        from libjpeg_amd import batch as batch_mod
        tp_best, tp_cfg = None, None
        for chunk, depth in ((8, 4), (8, 3), (4, 4), (16, 2)):
            sh = batch_mod.BatchShard([jpegs[i % 2] for i in range(nbatch)], local_rank, chunk, depth)
            sh.run()
            for _ in range(3):
                t = time.perf_counter()
                sh.run()
                dtp = time.perf_counter() - t
                if tp_best is None or dtp < tp_best:
                    tp_best, tp_cfg = dtp, (chunk, depth)
            sh.close()
        bout = torch.empty((nbatch, H, row), dtype=torch.uint8, device="cuda")
        # the same streams without restart markers: the device finds virtual restart points itself (huffman_walk_kernel)
        plain = [synth.synth_jpeg(W, H, seed=1234 + 17 * rank + i, quality=85, subsampling=args.subsampling, restart_mcus=0) for i in range(2)]
        tn = []
        for _ in range(5):
            t = time.perf_counter()
            dec.read(plain[0], entropy="gpu")
            dec.reconstruct_device(dev_out.data_ptr(), row)
            tn.append(time.perf_counter() - t)
        walk_rounds = dec.device_walk_rounds()
        nplain = 16
        tnb = []
        for _ in range(3):
            t = time.perf_counter()
            bdec.decode_batch_device([plain[i % 2] for i in range(nplain)])
            bdec.reconstruct_batch_device(bout.data_ptr(), H * row, row)
            tnb.append(time.perf_counter() - t)
        bdec.close()
        del bout
        result["end_to_end"]["device_entropy_no_restart_markers"] = {
            "pixels_left_in_hbm_ms": round(min(tn) * 1e3, 2), "value": round(W * H / min(tn) / 1e6, 1), "unit": "Mpixels/s", "walk_rounds": walk_rounds,
            "batch": {"frames": nplain, "ms_per_frame": round(min(tnb) / nplain * 1e3, 3), "value": round(W * H * nplain / min(tnb) / 1e6, 1), "unit": "Mpixels/s"},
            "stream_bytes": len(plain[0]),
            "note": "no DRI: huffman_walk_kernel rounds to a fixed point of the subsequence hand-over states, prefix sums, virtual restart "
                    "intervals emitted on the device, then huffman_scan_kernel and the fused kernel; no host thread decodes"}
        result["end_to_end"]["device_entropy"] = {
            "batch": {"frames": nbatch, "ms_per_frame": round(min(tb) / nbatch * 1e3, 3), "value": round(W * H * nbatch / min(tb) / 1e6, 1),
                      "unit": "Mpixels/s", "note": "32 streams in host memory -> parallel header parse -> H2D of the compressed bytes -> "
                                                   "huffman_scan_kernel launches -> one fused kernel launch, pixels left in HBM (one synchronous call)",
                      "pipelined": {"ms_per_frame": round(tp_best / nbatch * 1e3, 3), "value": round(W * H * nbatch / tp_best / 1e6, 1), "unit": "Mpixels/s",
                                    "chunk_frames": tp_cfg[0], "decoder_objects": tp_cfg[1],
                                    "note": "the same 32 streams through libjpeg_amd/batch.py: chunks on several decoder objects, host work of one chunk "
                                            "under the upload and the kernels of the others"}},
            "value": round(W * H / min(ts) / 1e6, 1), "unit": "Mpixels/s", "ms": round(min(ts) * 1e3, 2),
            "read_ms": round(min(tr) * 1e3, 2), "pixels_left_in_hbm_ms": round(min(th) * 1e3, 2),
            "pipelined_ms_per_frame": round(dt / nb * 1e3, 2), "pipelined_value": round(W * H * nb / dt / 1e6, 1),
            "pipelined_depth": best_depth,
            "restart_interval_mcus": 8, "stream_bytes": len(jpegs[0]),
            "note": "bytes -> header parse + restart marker search on the host -> H2D of the compressed stream -> "
                    "huffman_scan_kernel (one lane per restart interval) -> fused kernel -> D2H of the pixels"}
    if args.full and rank == 0 and world == 1 and not args.no_end_to_end:
        # progressive frames with restart markers: every scan on the device since round 6 (huffman_prog_kernel), host decoder beside it
        try:
            pdata = synth.synth_jpeg(W, H, seed=1234 + 17 * rank, quality=85, subsampling=args.subsampling, restart_mcus=8, progressive=True)
            pr = {}
            for mode in ("host", "prefer-gpu"):
                ts = []
                for _ in range(4):
                    t = time.perf_counter()
                    dec.read(pdata, entropy=mode)
                    ts.append(time.perf_counter() - t)
                pr[mode] = (min(ts), dec.entropy_used)
            dec.read(pdata, entropy="prefer-gpu")
            dev_px = torch.empty((H, row), dtype=torch.uint8, device="cuda")
            dec.reconstruct_device(dev_px.data_ptr(), row)
            ok = verify_against_oracle([(dev_px, pdata)])
            del dev_px
            result["end_to_end"]["progressive"] = {
                "stream_bytes": len(pdata), "read_ms_host": round(pr["host"][0] * 1e3, 2), "read_ms_prefer_gpu": round(pr["prefer-gpu"][0] * 1e3, 2),
                "prefer_gpu_ran_on": pr["prefer-gpu"][1], "verified": ok,
                "note": "one 8K 4:2:0 Q85 progressive frame (Pillow's scan script, DRI = 8): bytes -> coefficients in HBM; device = header parse + "
                        "marker search on the host, every scan one restart interval per lane (DC / AC first passes with EOB runs, refinement passes)"}
        except Exception as e:  # noqa: BLE001 -- a side measurement never costs the headline number
            result["end_to_end"]["progressive"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_end_to_end:
        # encoder direction of the block pipeline: forward kernels on frames resident in HBM, and one picture
        # from host memory to a baseline stream (upload, kernels, download of the coefficients, entropy coder on the host)
        try:
            img = synth.synth_image(W, H, 1234 + 17 * rank)
            fi = api.frame_layout(W, H, 3, (2, 1, 1), (2, 1, 1), [list(info.quant[t]) for t in range(4)], quant_index=list(info.quant_index)[:3])
            FE = 8
            px = torch.from_numpy(img).cuda().unsqueeze(0).repeat(FE, 1, 1, 1).contiguous()
            fcoef = torch.empty((FE, int(fi.coef_count)), dtype=torch.int16, device="cuda")
            for _ in range(150):  # settles the clocks like the main measurement does
                api.launch_forward(fi, px.data_ptr(), fcoef.data_ptr(), FE, W * 3, H * W * 3, stream=stream.cuda_stream)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(20):
                api.launch_forward(fi, px.data_ptr(), fcoef.data_ptr(), FE, W * 3, H * W * 3, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            fms = e0.elapsed_time(e1) / 20
            # the frames stay where they are: forward kernels for all of them, device entropy coder frame by frame
            dec.encode_batch_device(fi, px.data_ptr(), fcoef.data_ptr(), 2, W * 3, H * W * 3, 8, False)
            tb = []
            for _ in range(3):
                streams = dec.encode_batch_device(fi, px.data_ptr(), fcoef.data_ptr(), FE, W * 3, H * W * 3, 8, False)
                tb.append(list(dec.timing().values())[0])  # the C call (the Python wrapper copies the streams once more)
            del px, fcoef
            dec.encode(img, 85, "420", 8, False)
            te = []
            for _ in range(4):
                t = time.perf_counter()
                stream_bytes = dec.encode(img, 85, "420", 8, False)
                te.append(time.perf_counter() - t)
            result["end_to_end"]["encoder_direction"] = {
                "forward_kernels": {"value": round(W * H * FE / fms / 1e3, 1), "unit": "Mpixels/s", "ms": round(fms, 3), "frames": FE,
                                    "algorithmic_GBps": round(W * H * FE * 6 / fms / 1e6, 1),
                                    "note": "RGB in HBM -> YCbCr 4:2:0 -> FDCT -> quantiser -> int16 planes in HBM (fdct420_tile_kernel + fdct_blocks_kernel for the edges)"},
                "encode_frames_in_hbm": {"value": round(W * H * FE / min(tb) / 1e6, 1), "unit": "Mpixels/s", "ms_per_frame": round(min(tb) / FE * 1e3, 3), "frames": FE,
                                         "stream_bytes": len(streams[0]),
                                         "note": "frames resident in HBM -> baseline JPEG streams in host memory: forward kernels + on-device entropy "
                                                 "coder (mijpeg_encode_batch_device); only the streams cross PCIe"},
                "encode_picture": {"value": round(W * H / min(te) / 1e6, 1), "unit": "Mpixels/s", "ms": round(min(te) * 1e3, 2), "stream_bytes": len(stream_bytes),
                                   "note": "one 8K picture in host memory -> baseline JPEG, restart interval 8, Annex K tables: the reference "
                                           "encoder's tables and coefficients (mijpeg_encode_image)"}}
        except Exception as e:  # a side measurement never costs the headline number
            result["end_to_end"]["encoder_direction"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_xt:
        try:
            result["xt_profile_c"] = xt_profile_c(local_rank, stream, not args.no_cpu_baseline)
        except Exception as e:  # noqa: BLE001 -- a side measurement never costs the headline number
            result["xt_profile_c"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            result["cpu_baseline"] = cpu_baseline(jpegs[0], W, H)
            if isinstance(result.get("batch4k"), dict) and result["batch4k"].get("cpu_baseline"):
                result["cpu_baseline"]["all_cores"] = result["batch4k"]["cpu_baseline"]
            ref_client = os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "_ref", "stripe_loop_ref")
            if os.path.exists(ref_client):  # the reference library under the same client as end_to_end.drop_in_client (one core)
                result["cpu_baseline"]["drop_in_client"] = drop_in_client(ref_client, jpegs[0], 2)
        except Exception as e:  # the baseline is a report, never a reason to lose the GPU number
            result["cpu_baseline"] = {"value": None, "error": repr(e)}
    dec.close()
    if rank == 0:
        # the side measurements in a few scalars: inside `config` (the driver's record keeps the scalars of the contract's keys) and once
        # more as the LAST key of the line (what a tail of the output still shows)
        def pick(d, *path):
            for k in path:
                d = d.get(k) if isinstance(d, dict) else None
            return d

        summary = {"verified": result.get("verified"), "kernel_frac": pick(result, "roofline", "frac"),
                   "batch4k_ms": pick(result, "batch4k", "ms_per_batch"), "batch4k_median_ms": pick(result, "batch4k", "median_ms_per_batch"),
                   "batch4k_mpix": pick(result, "batch4k", "value"),
                   "batch4k_verified": pick(result, "batch4k", "verified"),
                   "xt_r12_kernel_ms": pick(result, "xt_profile_c", "r12", "kernel_ms"), "xt_r12_frac": pick(result, "xt_profile_c", "r12", "roofline", "frac"),
                   "xt_r12_verified": pick(result, "xt_profile_c", "r12", "verified"),
                   "xt_rR4_kernel_ms": pick(result, "xt_profile_c", "r12_rR4", "kernel_ms"), "xt_rR4_frac": pick(result, "xt_profile_c", "r12_rR4", "roofline", "frac"),
                   "xt_rR4_bytes_to_codes_ms": pick(result, "xt_profile_c", "r12_rR4", "bytes_to_half_codes_in_hbm", "ms"),
                   "xt_rR4_verified": pick(result, "xt_profile_c", "r12_rR4", "verified"),
                   "xt_rR4_z8_bytes_to_codes_ms": pick(result, "xt_profile_c", "r12_rR4_z8", "bytes_to_half_codes_in_hbm", "ms"),
                   "xt_rR4_z8_verified": pick(result, "xt_profile_c", "r12_rR4_z8", "verified"),
                   "e2e_ms": pick(result, "end_to_end", "ms"), "e2e_device_entropy_ms": pick(result, "end_to_end", "device_entropy", "ms"),
                   "progressive_read_ms_host": pick(result, "end_to_end", "progressive", "read_ms_host"),
                   "progressive_read_ms_device": pick(result, "end_to_end", "progressive", "read_ms_prefer_gpu"),
                   "dense_frac": pick(result, "roofline_dense", "dense", "frac"), "reference_encoded_frac": pick(result, "roofline_reference_encoded", "frac")}
        if args.full:
            for k, v in summary.items():
                if k != "verified":
                    result["config"]["side_" + k] = v
            result["summary"] = summary
        print(json.dumps(result))
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

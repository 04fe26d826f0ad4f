"""The host decoder's results, recorded: every stream under tests/golden and three damaged variants of each, read by the host
decoder at 1, 2, 5 and 16 threads, against the digests tests/golden/host_decode_digests.json holds.  The digests were recorded
from the decoder as it stood before HostDecoder::decode_t was broken into named stages; a restructuring of the host decoder
that changes what any of these reads leaves -- coefficients, range maxima, flags, the error code -- shows here, on the CPU.

Per read: the error code, or the first 12 hex digits of a SHA-256 over the whole coefficient store (residual planes included),
range_max of the frame's components, fast_arith, coef_wide and, for JPEG XT frames, the residual frame's range_max.

    python tests/test_host_decode_pinned.py --record     writes the fixture from the library as built
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "host_decode_digests.json")
THREADS = (1, 2, 5, 16)

# (a process of its own per environment: the switches are read once per process)
CHILD = r"""
import sys, os, glob, json, hashlib, ctypes as C
os.environ["MIJPEG_NO_TORCH"] = "1"
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import damage
from libjpeg_amd import api
L = api.lib()
L.mijpeg_coefficients.restype = C.c_void_p
L.mijpeg_coefficients32.restype = C.c_void_p
L.mijpeg_coefficients32.argtypes = [C.c_void_p, C.c_int]
golden, every = sys.argv[1], int(sys.argv[2])
files = sorted(glob.glob(os.path.join(golden, "**", "*.jpg"), recursive=True))
out = {}
for index, path in enumerate(files):
    if index %% every:
        continue
    data = open(path, "rb").read()
    blobs = [data] + [blob for _, blob in damage.cases(data, 3, 9000 + index, "entropy")]
    entries = []
    for blob in blobs:
        for thr in %(threads)r:
            d = api.Decoder(None)
            try:
                f = d.read(blob, thr)
            except api.MijpegError as e:
                entries.append(int(e.code))
                d.close()
                continue
            # the store begins coef_offset[0] int16 slots in front of the first plane; coef_count counts int16 slots, of which a
            # coefficient of a wide frame takes two (include/mijpeg.h)
            first = (L.mijpeg_coefficients32 if f.coef_wide else L.mijpeg_coefficients)(d._h, 0)
            base = first - int(f.coef_offset[0]) * 2
            n = int(f.coef_count) * 2
            h = hashlib.sha256(bytes((C.c_uint8 * n).from_address(base)))
            rr = list(d.xt_params().residual.range_max)[:3] if f.xt else []
            h.update(repr((list(f.range_max)[:f.components], int(f.fast_arith), int(f.coef_wide), rr)).encode())
            entries.append(h.hexdigest()[:12])
            d.close()
    out[os.path.relpath(path, golden).replace(os.sep, "/")] = entries
json.dump(out, sys.stdout)
""" % {"root": ROOT, "threads": THREADS}


def _start(extra, every=1):
    return subprocess.Popen([sys.executable, "-c", CHILD, GOLDEN, str(every)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            env=dict(os.environ, **extra))


def _finish(proc):
    out, err = proc.communicate()
    assert proc.returncode == 0, err[-2000:]
    return json.loads(out)


def _differences(got, pinned):
    diffs = []
    for path in sorted(set(got) | set(pinned)):
        a, b = got.get(path), pinned.get(path)
        if a == b:
            continue
        if a is None or b is None or len(a) != len(b):
            diffs.append("%s: %s" % (path, "not decoded here" if a is None else "not in the fixture" if b is None else "another number of reads"))
            continue
        for k, (x, y) in enumerate(zip(a, b)):
            if x != y:
                diffs.append("%s, %s, %d threads: %r, recorded %r" % (path, "as it is" if k < 4 else "damaged variant %d" % (k // 4), THREADS[k % 4], x, y))
    return diffs


ENVIRONMENTS = ({}, {"MIJPEG_NO_SCAN_PIPELINE": "1", "MIJPEG_NO_FRAME_OVERLAP": "1"}, {"MIJPEG_NO_DEFERRED_REFINE": "1"})


def test_host_reads_leave_what_was_recorded():
    """Every golden stream and its damaged variants at 1, 2, 5 and 16 threads: the recorded digest or error code -- with the scan
    pipeline and the overlap of the two frames, without them (scan after scan, frame after frame), and with the coefficient
    blocks instead of bit masks between the scans of a refinement chain."""
    with open(FIXTURE) as f:
        pinned = json.load(f)
    assert len(pinned) >= 500 and all(len(v) == 4 * len(THREADS) for v in pinned.values())
    procs = [_start(extra) for extra in ENVIRONMENTS]  # (side by side: the three take the time of one)
    results = [_finish(p) for p in procs]
    for extra, got in zip(ENVIRONMENTS, results):
        diffs = _differences(got, pinned)
        assert not diffs, "%s: %d reads differ:\n%s" % (extra or "default environment", len(diffs), "\n".join(diffs[:40]))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    recorded = _finish(_start({}))
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(recorded[k])) for k in sorted(recorded)) + "\n}\n")  # a line per stream
    print("%d files, %d reads, %d of them errors" % (len(recorded), sum(len(v) for v in recorded.values()),
                                                     sum(isinstance(e, int) for v in recorded.values() for e in v)))

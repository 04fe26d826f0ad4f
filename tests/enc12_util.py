"""Shared pieces of the 12-bit encoder tests (test_encode12_cpu.py, test_encode12.py) and of tests/golden/enc12/generate.py:
the seeded 12-bit test pictures, the list of golden cases, 16-bit PNM I/O, and a numpy restatement of what the reference does in
front of its block transform at 12 bits -- forward L transformation (colortrafo/ycbcrtrafo.cpp:85-242 with m_lDCShift = 2048, clamp
to (4096 << 4) - 1) and box downsampling (upsampling/downsampler.cpp:70-139, downsamplerbase.cpp:124-155) -- whose output goes
through the oracle's oj_fdct_block(..., 12).  The restatement is validated against every golden by test_encode12_cpu.py; the GPU
tests use it for shapes that have no golden.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "enc12")

# layout name -> (hsamp, vsamp) per component, and the reference CLI's -s argument (SUBSAMPLING factors per component)
LAYOUTS = {
    "444": (((1, 1, 1), (1, 1, 1)), None),
    "420": (((2, 1, 1), (2, 1, 1)), "1x1,2x2,2x2"),
    "422": (((2, 1, 1), (1, 1, 1)), "1x1,2x1,2x1"),
    "440": (((1, 1, 1), (2, 1, 1)), "1x1,1x2,1x2"),
    "411": (((4, 1, 1), (1, 1, 1)), "1x1,4x1,4x1"),
    "3x3": (((3, 1, 1), (3, 1, 1)), "1x1,3x3,3x3"),
    "grey": (((1,), (1,)), None),
}

# key: (width, height, layout, content, seed, quality, extra switches of the reference CLI)
CASES = {
    "420_80x48": (80, 48, "420", "synth", 1, 85, []),
    "422_100x9": (100, 9, "422", "synth", 2, 85, []),
    "440_97x61": (97, 61, "440", "synth", 3, 85, []),
    "444_97x61": (97, 61, "444", "synth", 4, 85, []),
    "3x3_97x61": (97, 61, "3x3", "synth", 5, 85, []),
    "411_33x17": (33, 17, "411", "synth", 6, 85, []),
    "grey_70x50": (70, 50, "grey", "synth", 7, 85, []),
    "420_64x40_q2": (64, 40, "420", "synth", 8, 2, []),
    "420_64x40_q30": (64, 40, "420", "synth", 12, 30, []),
    "420_64x40_q100": (64, 40, "420", "synth", 9, 100, []),
    "444_64x40_q100_pixel_checker": (64, 40, "444", "pixel_checker", 0, 100, []),
    "444_64x40_q100_block_checker": (64, 40, "444", "block_checker", 0, 100, []),
    "420_272x144_z4": (272, 144, "420", "synth", 10, 85, ["-z", "4"]),
    "444_41x23_identity": (41, 23, "444", "synth", 11, 85, ["-c"]),
}


def synth12(w: int, h: int, seed: int, channels: int = 3) -> np.ndarray:
    """Seeded 12-bit picture, (h, w, channels) uint16 in 0..4095: smooth content plus texture, a region pinned at 0 and one at 4095."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, channels), np.float64)
    for c in range(channels):
        fx, fy, ph = rng.uniform(0.02, 0.25), rng.uniform(0.02, 0.25), rng.uniform(0, 6.28)
        img[..., c] = 2048 + 1500 * np.sin(fx * x + fy * y + ph) + 400 * np.cos(0.9 * x - 0.7 * y + c)
    img += rng.normal(0, 180, img.shape)
    img = np.clip(np.rint(img), 0, 4095).astype(np.uint16)
    img[: max(1, h // 5), : max(1, w // 4)] = 0
    img[h - max(1, h // 4):, w - max(1, w // 5):] = 4095
    return img


def pixel_checker(w: int, h: int, channels: int = 3) -> np.ndarray:
    """0 / 4095 checkerboard of single pixels: the widest AC coefficients."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 4095).astype(np.uint16)[..., None], channels, axis=2)


def block_checker(w: int, h: int, channels: int = 3) -> np.ndarray:
    """0 / 4095 checkerboard of 8 x 8 blocks: DC differences of category 15 at quality 100."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((((x >> 3) + (y >> 3)) & 1) * 4095).astype(np.uint16)[..., None], channels, axis=2)


def case_image(key: str) -> np.ndarray:
    w, h, layout, content, seed, _, _ = CASES[key]
    nc = 1 if layout == "grey" else 3
    if content == "pixel_checker":
        return pixel_checker(w, h, nc)
    if content == "block_checker":
        return block_checker(w, h, nc)
    return synth12(w, h, seed, nc)


def case_args(key: str):
    """The reference CLI's switches of a case."""
    _, _, layout, _, _, q, extra = CASES[key]
    sub = LAYOUTS[layout][1]
    return ["-q", str(q)] + (["-s", sub] if sub else []) + list(extra)


def case_restart(key: str) -> int:
    extra = CASES[key][6]
    return int(extra[extra.index("-z") + 1]) if "-z" in extra else 0


def golden_stream(key: str) -> bytes:
    with open(os.path.join(GOLDEN_DIR, key + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def golden_coefficients(key: str):
    """(oracle info, [int32 (bh, bw, 64)] per component) of a golden -- computed once, shared, not to be written to."""
    info, planes = O.decode_coefficients(golden_stream(key))
    for p in planes:
        p.setflags(write=False)
    return info, planes


def manifest() -> dict:
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as f:
        return json.load(f)


def write_pnm16(path: str, img: np.ndarray, maxval: int = 4095) -> None:
    """P5 / P6 with big-endian 16-bit samples."""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 or img.shape[2] == 1 else 3
    with open(path, "wb") as f:
        f.write(b"P%d\n%d %d\n%d\n" % (6 if ch == 3 else 5, w, h, maxval))
        f.write(np.ascontiguousarray(img, np.uint16).astype(">u2").tobytes())


def reference_encode12(img: np.ndarray, args):
    """The reference CLI on a 16-bit PNM of `img`: (return code, stream or None, stderr)."""
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmpdir) as d:
        src, dst = os.path.join(d, "in.ppm"), os.path.join(d, "out.jpg")
        write_pnm16(src, img)
        r = subprocess.run([O.REF_BIN, *args, src, dst], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        data = None
        if os.path.exists(dst):
            with open(dst, "rb") as f:
                data = f.read()
        return r.returncode, data, r.stderr.decode(errors="replace")


# ---- numpy restatement of colour transformation + downsampling at 12 bits -------------------------------------------------
def ycc12(img: np.ndarray) -> np.ndarray:
    """(h, w, 3) samples -> (3, h, w) int64 Y, Cb, Cr with COLOR_BITS = 4 fractional bits: FIX_TO_COLOR at FIX_BITS 13, the 12-bit DC
    offset 2048 << 13 on the chroma rows, clamp to 0 .. (4096 << 4) - 1 (ycbcrtrafo.cpp:176-199; matrix
    colortransformerfactory.cpp:177-183)."""
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    dc = (2048 << 13) + 256
    y = (r * 2449 + g * 4809 + b * 934 + 256) >> 9
    cb = (r * -1382 + g * -2714 + b * 4096 + dc) >> 9
    cr = (r * 4096 + g * -3430 + b * -666 + dc) >> 9
    return np.clip(np.stack([y, cb, cr]), 0, (4096 << 4) - 1)


def component_samples(img: np.ndarray, ycbcr: bool) -> np.ndarray:
    """(ncomp, h, w) int64 samples with 4 fractional bits in front of the downsampler."""
    if img.ndim == 2:
        img = img[..., None]
    if img.shape[2] == 3 and ycbcr:
        return ycc12(img)
    return np.moveaxis(img.astype(np.int64) << 4, 2, 0)  # INT_TO_COLOR


def block_samples(s: np.ndarray, sx: int, sy: int) -> np.ndarray:
    """One component's full-resolution samples (h, w) -> the samples of its blocks that cover samples (nby * 8, nbx * 8).
    1 x 1: partial blocks pre-filled with the level shift (ycbcrtrafo.cpp:100-113).  Otherwise the box filter over the lines that
    exist, the line beyond the right edge mirrored (downsamplerbase.cpp:141-145), a row without any line zero
    (downsampler.cpp:92-95)."""
    h, w = s.shape
    nbx, nby = ((w + sx - 1) // sx + 7) >> 3, ((h + sy - 1) // sy + 7) >> 3
    if sx == 1 and sy == 1:
        out = np.full((nby * 8, nbx * 8), 2048 << 4, np.int64)
        out[:h, :w] = s
        return out
    x = np.arange(nbx * 8 * sx)
    m = x - w
    xi = np.where(x < w, x, np.where(w > m, w - 1 - m, 0))
    out = np.zeros((nby * 8, nbx * 8), np.int64)
    for r in range(nby * 8):
        lines = [y for y in range(r * sy, r * sy + sy) if y < h]
        if not lines:
            continue
        acc = s[lines][:, xi].sum(axis=0).reshape(nbx * 8, sx).sum(axis=1)
        norm = len(lines) * sx
        out[r] = acc // norm if norm > 1 else acc
    return out


def fdct_blocks(samples: np.ndarray, quant, bw: int, bh: int) -> np.ndarray:
    """Block samples (nby * 8, nbx * 8) -> (bh, bw, 64) int32 coefficients through oj_fdct_block(..., 12); MCU padding blocks zero."""
    L = O.lib()
    nby, nbx = samples.shape[0] // 8, samples.shape[1] // 8
    out = np.zeros((bh, bw, 64), np.int32)
    q = np.ascontiguousarray(quant, np.uint16)
    blk = np.empty(64, np.int32)
    res = np.empty(64, np.int32)
    for by in range(nby):
        for bx in range(nbx):
            blk[:] = samples[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64)
            L.oj_fdct_block(res.ctypes.data, blk.ctypes.data, q.ctypes.data, 12)
            out[by, bx] = res
    return out


def forward12(img: np.ndarray, hsamp, vsamp, quants, ycbcr: bool = True):
    """The coefficient planes of a 12-bit picture: [int32 (bh, bw, 64)] per component.  quants[c]: component c's 64 deltas, natural
    order."""
    h, w = img.shape[:2]
    comps = component_samples(img, ycbcr)
    nc = comps.shape[0]
    hmax, vmax = max(hsamp[:nc]), max(vsamp[:nc])
    mx, my = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    planes = []
    for c in range(nc):
        sx, sy = hmax // hsamp[c], vmax // vsamp[c]
        planes.append(fdct_blocks(block_samples(comps[c], sx, sy), quants[c], mx * hsamp[c], my * vsamp[c]))
    return planes


def covered_blocks(w: int, h: int, sx: int, sy: int):
    """(nbx, nby): the blocks of a component that cover samples."""
    return ((w + sx - 1) // sx + 7) >> 3, ((h + sy - 1) // sy + 7) >> 3


def oracle_quant(info, c: int) -> np.ndarray:
    return np.array(info.quant[info.tq[c]][:], np.uint16)


assert C.sizeof(C.c_int32) == 4

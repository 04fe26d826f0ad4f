"""Cases for the forward (encoder direction) kernels at their partition edges, pitches and ties (tests/test_forward_gates_cpu.py,
tests/test_forward_gates.py).

Three things live here.  The REFERENCE MODEL, expected(): oracle.forward at 8 bits (the C restatement pinned against the reference
encoder's coefficients) and enc12_util.forward12 at 12; nothing in it calls the library's forward path.  The PARTITION RESTATEMENT,
owners(): which kernel owns each block of a component, restated from the rule in forward.hpp / encode_list.hpp::forward_args_of; it
lets the tests state and assert what a case reaches and never produces an expected value.  The CORPUS: the smallest shapes that
still cross each boundary, content with saturated samples and exact quantiser halves, and four sets of quantiser tables.

block_samples() and pre_quantiser() restate in numpy what the model feeds its block transform and what the transform hands the
quantiser; they exist to FIND and COUNT quantiser ties and to hold the model against a float64 DCT, and the CPU tests hold them
against the model first."""
import functools

import numpy as np

import enc12_util as U
from oracle import oracle as O

# layout name -> (hsamp, vsamp) per component
LAYOUTS = {"444": ((1, 1, 1), (1, 1, 1)), "420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "440": ((1, 1, 1), (2, 1, 1)),
           "411": ((4, 1, 1), (1, 1, 1)), "3x3": ((3, 1, 1), (3, 1, 1)), "4x2": ((4, 1, 1), (2, 1, 1)), "mixed": ((2, 1, 2), (2, 2, 1)),
           "grey": ((1,), (1,)), "rgb": ((1, 1, 1), (1, 1, 1))}  # rgb: three components, no colour transformation (ycbcr = 0)

TILES_420 = [(128, 128), (129, 129), (144, 136), (255, 257), (256, 128)]  # whole tiles; all but the first with strips beside them
NO_TILES_420 = [(127, 300), (136, 127)]  # one side below a tile: interior and per-block kernels only
SMALL = [(7, 7), (8, 8), (9, 17), (17, 9), (16, 16), (24, 33), (33, 24), (32, 32), (31, 15), (15, 31)]  # 444 / 422 / 440 (and 420)
SUB_BLOCK = [(1, 1), (2, 3), (3, 2), (5, 1), (7, 2), (9, 5), (33, 17)]  # 411, 3x3, 4x2, mixed
PLAIN = [(9, 7), (70, 50)]  # grey, rgb

# (width, height, layout) of every case
SHAPES = ([(w, h, "420") for w, h in TILES_420 + NO_TILES_420] + [(w, h, lay) for lay in ("444", "422", "440", "420") for w, h in SMALL] +
          [(w, h, lay) for lay in ("411", "3x3", "4x2", "mixed") for w, h in SUB_BLOCK] + [(w, h, lay) for lay in ("grey", "rgb") for w, h in PLAIN])
CONTENTS = ("noise", "saturated", "pixel_checker", "block_checker", "ties")
TABLES = ("ones", "max", "pow2", "random")
PRECISIONS = (8, 12)


def components_of(layout: str) -> int:
    return len(LAYOUTS[layout][0])


def ycbcr_of(layout: str) -> bool:
    return layout not in ("grey", "rgb")


# ---- geometry and the partition restatement ---------------------------------------------------------------------------------------
def geometry(w: int, h: int, layout: str):
    """Per component (subx, suby, bw, bh, nbx, nby): subsampling factors, plane size in blocks (MCU padded), blocks that cover samples."""
    hs, vs = LAYOUTS[layout]
    hmax, vmax = max(hs), max(vs)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    out = []
    for c in range(len(hs)):
        sx, sy = hmax // hs[c], vmax // vs[c]
        out.append((sx, sy, mx * hs[c], my * vs[c], (-(-w // sx) + 7) >> 3, (-(-h // sy) + 7) >> 3))
    return out


def coef_layout(w: int, h: int, layout: str):
    """(plane offsets in int16 units, coefficient count) of the decoder's layout: planes one behind the other."""
    offs, at = [], 0
    for _, _, bw, bh, _, _ in geometry(w, h, layout):
        offs.append(at)
        at += bw * bh * 64
    return offs, at


PAD, TILE, INTERIOR, EDGE = 0, 1, 2, 3


def dword_lines(base: int, row_stride: int, frame_stride: int = 0) -> bool:
    """forward_args_of's gate of the tile and interior kernels: every line starts on a dword boundary."""
    return ((base | row_stride | frame_stride) & 3) == 0


def fast_components(layout: str, dword: bool = True, slow: bool = False):
    """Per component: the interior kernels take its whole blocks (three components under RGB -> YCbCr, factors 1 or 2, dword lines,
    no MIJPEG_FORWARD_SLOW)."""
    hs, vs = LAYOUTS[layout]
    hmax, vmax = max(hs), max(vs)
    ok = dword and len(hs) == 3 and ycbcr_of(layout) and not slow
    return [ok and hmax // hs[c] <= 2 and vmax // vs[c] <= 2 for c in range(len(hs))]


def tiled(w: int, h: int, layout: str, dword: bool = True, slow: bool = False, no_tiles: bool = False) -> bool:
    return layout == "420" and all(fast_components("420", dword, slow)) and w >= 128 and h >= 128 and not no_tiles


def owners(w: int, h: int, layout: str, dword: bool = True, slow: bool = False, no_tiles: bool = False):
    """Per component a (bh, bw) array of PAD / TILE / INTERIOR / EDGE: who writes the block."""
    fast = fast_components(layout, dword, slow)
    is_tiled = tiled(w, h, layout, dword, slow, no_tiles)
    out = []
    for c, (sx, sy, bw, bh, nbx, nby) in enumerate(geometry(w, h, layout)):
        by, bx = np.mgrid[0:bh, 0:bw]
        own = np.full((bh, bw), EDGE, np.int8)
        if fast[c]:
            own[(bx < w // (8 * sx)) & (by < h // (8 * sy))] = INTERIOR
        if is_tiled:
            per_tile = 16 // sx
            own[(bx < (w >> 7) * per_tile) & (by < (h >> 7) * (16 // sy))] = TILE
        own[(bx >= nbx) | (by >= nby)] = PAD
        out.append(own)
    return out


def interior_kernel(layout: str, c: int):
    """(SX, SY) of fdct_interior_kernel<SX, SY> for component c."""
    hs, vs = LAYOUTS[layout]
    return max(hs) // hs[c], max(vs) // vs[c]


def mirror_clamps(w: int, sx: int) -> bool:
    """The mirror of the right edge reaches its `W > m ? W - 1 - m : 0` clamp: some x of the last block column lies W or more beyond W."""
    nbx = (-(-w // sx) + 7) >> 3
    return sx > 1 and nbx * 8 * sx - 1 - w >= w


def rows_without_lines(h: int, sy: int) -> bool:
    """Some row of a block that covers samples has no line of the picture under it."""
    nby = (-(-h // sy) + 7) >> 3
    return sy > 1 and (nby * 8 - 1) * sy >= h


# ---- quantiser tables -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(kind: str, nc: int):
    if kind == "ones":
        t = [np.ones(64, np.uint16) for _ in range(nc)]
    elif kind == "max":
        t = [np.full(64, 255, np.uint16) for _ in range(nc)]
    elif kind == "pow2":  # 1 .. 128 in turn, another phase per component; the DC delta of every component is 16
        t = []
        for c in range(nc):
            q = (1 << ((np.arange(64) + 3 * c) % 8)).astype(np.uint16)
            q[0] = 16
            t.append(q)
    else:
        rng = np.random.default_rng(2025)
        t = [rng.integers(1, 256, 64).astype(np.uint16) for _ in range(nc)]
    for q in t:
        q.setflags(write=False)
    return tuple(t)


def tables(kind: str, nc: int):
    """nc tables of 64 deltas, natural order, one per component."""
    return list(_tables(kind, nc))


def invq(delta) -> np.ndarray:
    """The quantiser multipliers as forward_args_of computes them: LONG(FLOAT(1 << 30) / delta + 0.5), a single precision quotient."""
    q = np.float32(1 << 30) / np.asarray(delta).astype(np.float32)
    return np.floor(q.astype(np.float64) + 0.5).astype(np.int64)


# ---- numpy restatement of the model's inner values --------------------------------------------------------------------------------
def _ycc8(img: np.ndarray) -> np.ndarray:
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    dc = (128 << 13) + 256
    y = (r * 2449 + g * 4809 + b * 934 + 256) >> 9
    cb = (r * -1382 + g * -2714 + b * 4096 + dc) >> 9
    cr = (r * 4096 + g * -3430 + b * -666 + dc) >> 9
    return np.clip(np.stack([y, cb, cr]), 0, (256 << 4) - 1)


def block_samples(img: np.ndarray, layout: str, precision: int):
    """Per component the samples (4 fractional bits) of its blocks that cover samples, (nby * 8, nbx * 8) int64: what the model feeds
    its block transform.  12 bits: enc12_util's; 8 bits: the same steps with the level shift 128."""
    if img.ndim == 2:
        img = img[..., None]
    ycc = ycbcr_of(layout)
    if precision == 12:
        comps = U.component_samples(img, ycc)
    else:
        comps = _ycc8(img) if ycc else np.moveaxis(img.astype(np.int64) << 4, 2, 0)
    out = []
    for c, (sx, sy, _, _, _, _) in enumerate(geometry(img.shape[1], img.shape[0], layout)):
        s = U.block_samples(comps[c], sx, sy)
        if precision == 8 and sx == 1 and sy == 1:  # (enc12_util pre-fills partial blocks with 2048: here the level shift is 128)
            h, w = comps[c].shape
            s[:] = 128 << 4
            s[:h, :w] = comps[c]
        out.append(s)
    return out


def _w(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # wrap to int32, as the reference's LONG does


def _f9(x: float) -> int:
    return int(x * 512.0 + 0.5)


def _fdct_1d(s):
    """One 8-point pass over eight int64 arrays: outputs before any shift (0 and 4 plain sums, the others scaled by 2^9)."""
    t0, t1, t2, t3 = _w(s[0] + s[7]), _w(s[1] + s[6]), _w(s[2] + s[5]), _w(s[3] + s[4])
    t10, t12, t11, t13 = _w(t0 + t3), _w(t0 - t3), _w(t1 + t2), _w(t1 - t2)
    o = [None] * 8
    o[0], o[4] = _w(t10 + t11), _w(t10 - t11)
    z1 = _w((t12 + t13) * _f9(0.541196100))
    o[2] = _w(z1 + t12 * _f9(0.765366865))
    o[6] = _w(z1 - t13 * _f9(1.847759065))
    t0, t1, t2, t3 = _w(s[0] - s[7]), _w(s[1] - s[6]), _w(s[2] - s[5]), _w(s[3] - s[4])
    t10, t11, t12, t13 = _w(t0 + t3), _w(t1 + t2), _w(t0 + t2), _w(t1 + t3)
    z1 = _w((t12 + t13) * _f9(1.175875602))
    tt12, tt13 = t12 * -_f9(0.390180644) + z1, t13 * -_f9(1.961570560) + z1
    o[1] = _w(t0 * _f9(1.501321110) - t10 * _f9(0.899976223) + tt12)
    o[3] = _w(t1 * _f9(3.072711026) - t11 * _f9(2.562915447) + tt13)
    o[5] = _w(t2 * _f9(2.053119869) - t11 * _f9(2.562915447) + tt12)
    o[7] = _w(t3 * _f9(0.298631336) - t10 * _f9(0.899976223) + tt13)
    return o


def pre_quantiser(samples: np.ndarray, precision: int) -> np.ndarray:
    """Block samples (nby * 8, nbx * 8) -> (nby, nbx, 64) int64: the value n of every coefficient that the quantiser
    (n * invq + (n > 0) + 2^45) >> 46 is given."""
    nby, nbx = samples.shape[0] // 8, samples.shape[1] // 8
    b = samples.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3).astype(np.int64)  # (nby, nbx, row, column)
    o = _fdct_1d([b[:, :, k, :] for k in range(8)])  # o[k]: frequency k of every column
    t = [o[k] if k in (0, 4) else _w(o[k] + 256) >> 9 for k in range(8)]
    out = np.empty((nby, nbx, 8, 8), np.int64)
    for r in range(8):
        o = _fdct_1d([t[r][..., i] for i in range(8)])
        o[0] = _w((o[0] - (((1 << (precision - 1)) << 10) if r == 0 else 0)) << 9)
        o[4] = _w(o[4] << 9)
        for k in range(8):
            out[:, :, r, k] = o[k]
    return out.reshape(nby, nbx, 64)


def quantise(n: np.ndarray, delta) -> np.ndarray:
    return (n * invq(delta) + (n > 0) + (1 << 45)) >> 46


def is_tie(n: np.ndarray, delta) -> np.ndarray:
    """The quantiser's argument is an exact half: n * invq + 2^45 = 0 (mod 2^46)."""
    return ((n * invq(delta) + (1 << 45)) & ((1 << 46) - 1)) == 0


# ---- content ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_blocks(precision: int):
    """Grey 8 x 8 blocks (a grey pixel's Y, and component 0 without a transformation, is the value itself) for the `pow2` tables of
    component 0: (DC+, DC-, AC+, AC-).  DC: flat blocks of 2^(P-1) +- an odd number, whose DC is an odd number of halves under the DC
    delta 16.  AC: a seeded search for blocks with an exact half at one AC position or more and none at DC, by the sign of the first."""
    top, shift = (1 << precision) - 1, 1 << (precision - 1)
    q = tables("pow2", 1)[0]
    dc = [[np.full((8, 8), shift + d, np.int64) for d in ds] for ds in ((1, 3, 77, shift - 1), (-1, -5, -101, -(shift - 1)))]
    rng = np.random.default_rng(1000 + precision)
    ac = [[], []]
    while min(len(ac[0]), len(ac[1])) < 4:
        amp = int(rng.integers(2, shift))
        cand = np.clip(shift + rng.integers(-amp, amp + 1, (8, 512 * 8)), 0, top).astype(np.int64)
        n = pre_quantiser(cand << 4, precision)[0]
        tie = is_tie(n, q)
        for k in np.flatnonzero(tie[:, 1:].any(axis=1) & ~tie[:, 0]):
            sign = 0 if n[k, 1 + int(np.argmax(tie[k, 1:]))] > 0 else 1
            if len(ac[sign]) < 4:
                ac[sign].append(cand[:, k * 8:k * 8 + 8])
    return dc[0], dc[1], ac[0], ac[1]


def picture(w: int, h: int, layout: str, precision: int, content: str, seed: int = 0) -> np.ndarray:
    """(h, w, 3) or -- grey -- (h, w) samples, uint8 or uint16 below 2^precision."""
    nc = components_of(layout)
    top = (1 << precision) - 1
    rng = np.random.default_rng([w, h, precision, CONTENTS.index(content), seed])
    y, x = np.mgrid[0:h, 0:w]
    if content == "noise":
        img = rng.integers(0, top + 1, (h, w, nc))
    elif content == "saturated":
        img = rng.integers(0, 2, (h, w, nc)) * top
    elif content == "pixel_checker":  # (another phase in the second channel: chroma sees it too)
        img = np.stack([((x + y + (c == 1)) & 1) * top for c in range(nc)], axis=2)
    elif content == "block_checker":
        img = np.stack([(((x >> 3) + (y >> 3) + (c == 1)) & 1) * top for c in range(nc)], axis=2)
    else:  # ties: block (bx, by) is of kind (bx & 1) + 2 * (by & 1) -- DC+, DC-, AC+, AC- --, the kind's blocks in turn
        kinds = _tie_blocks(precision)
        img = np.empty((((h + 7) >> 3) * 8, ((w + 7) >> 3) * 8), np.int64)
        for by in range(img.shape[0] >> 3):
            for bx in range(img.shape[1] >> 3):
                blocks = kinds[(bx & 1) + 2 * (by & 1)]
                img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blocks[((bx >> 1) + (by >> 1) + seed) % len(blocks)]
        img = np.repeat(img[:h, :w, None], nc, axis=2)
    img = np.ascontiguousarray(img.astype(np.uint8 if precision == 8 else np.uint16))
    return img[..., 0] if nc == 1 else img


def count_ties(img: np.ndarray, layout: str, precision: int, quants):
    """(DC+, DC-, AC+, AC-): exact halves of component 0 under quants[0], counted on the model's pre-quantiser values."""
    n = pre_quantiser(block_samples(img, layout, precision)[0], precision)
    tie = is_tie(n, quants[0])
    return (int((tie[..., 0] & (n[..., 0] > 0)).sum()), int((tie[..., 0] & (n[..., 0] < 0)).sum()),
            int((tie[..., 1:] & (n[..., 1:] > 0)).sum()), int((tie[..., 1:] & (n[..., 1:] < 0)).sum()))


# ---- the reference model ----------------------------------------------------------------------------------------------------------------
def expected(img: np.ndarray, hs, vs, quants, precision: int, ycbcr: bool):
    """The coefficient planes [int32 (bh, bw, 64)] of a picture: oracle.forward at 8 bits, enc12_util.forward12 at 12.  quants[c]:
    component c's 64 deltas, natural order."""
    if precision == 12:
        return U.forward12(img, hs, vs, quants, ycbcr)
    h, w = img.shape[:2]
    nc = 1 if img.ndim == 2 else img.shape[2]
    hmax, vmax = max(hs[:nc]), max(vs[:nc])
    oi = O.OjInfo()
    oi.width, oi.height, oi.precision, oi.ncomp = w, h, 8, nc
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    for c in range(nc):
        oi.hs[c], oi.vs[c], oi.tq[c] = hs[c], vs[c], c
        oi.subx[c], oi.suby[c] = hmax // hs[c], vmax // vs[c]
        oi.bw[c], oi.bh[c] = mx * hs[c], my * vs[c]
        oi.cw[c], oi.ch[c] = -(-w // oi.subx[c]), -(-h // oi.suby[c])
        for i in range(64):
            oi.quant[c][i] = int(quants[c][i])
    return O.forward(oi, img if img.ndim == 3 else img[..., None], 1 if ycbcr else 0)


@functools.lru_cache(maxsize=None)
def case(w: int, h: int, layout: str, precision: int, content: str, table: str):
    """(picture, expected planes) of a corpus case, computed once, shared, not to be written to."""
    img = picture(w, h, layout, precision, content)
    hs, vs = LAYOUTS[layout]
    planes = expected(img, hs, vs, tables(table, components_of(layout)), precision, ycbcr_of(layout))
    img.setflags(write=False)
    for p in planes:
        p.setflags(write=False)
    return img, planes


def coefficient_store(planes, w: int, h: int, layout: str) -> np.ndarray:
    """Expected planes -> the frame's coefficient store as the kernels leave it (int16, coef_count elements): the blocks that cover
    samples, the MCU padding blocks zero."""
    offs, count = coef_layout(w, h, layout)
    out = np.zeros(count, np.int16)
    for c, (_, _, bw, bh, nbx, nby) in enumerate(geometry(w, h, layout)):
        p = np.zeros((bh, bw, 64), np.int32)
        p[:nby, :nbx] = planes[c][:nby, :nbx]
        assert np.abs(p).max(initial=0) < 32768
        out[offs[c]:offs[c] + bw * bh * 64] = p.reshape(-1)
    return out

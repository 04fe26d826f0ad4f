"""The ragged transcode's transforms (include/mijpeg.h) restated in numpy on block planes, for the tests of
mijpeg_transform_blocks, mijpeg_transcode_plan_transformed, transform_list_kernel and the transformed list call.  Each of the eight
transforms is "transpose first (T), then mirror horizontally (MH) and / or vertically (MV)"; per component, blocks in natural order,
block[v, u] with u the horizontal frequency:

    T    the block grid and every block are transposed; sampling factors, width and height swap; tables are transposed
    MH   the block columns are reversed over the destination's width in blocks, odd u are negated
    MV   the block rows are reversed over the destination's height in blocks, odd v are negated

A mirrored axis must be a whole number of MCUs of the frame after T: the picture is refused, or (TRIM) the partial MCU at the far
edge is dropped.  Requantisation (tests/requant_model.py) composes with the transposed source table.  Nothing here is taken from the
library; test_ragged_transform_cpu.py pins the model itself by a float64 inverse DCT."""
import numpy as np

import requant_model as R

NONE, FLIP_H, FLIP_V, TRANSPOSE, TRANSVERSE, ROT_90, ROT_180, ROT_270 = range(8)
TRIM = 0x100
NAMES = ["none", "flip_h", "flip_v", "transpose", "transverse", "rot90", "rot180", "rot270"]
# (T, MH, MV)
BITS = {NONE: (0, 0, 0), FLIP_H: (0, 1, 0), FLIP_V: (0, 0, 1), TRANSPOSE: (1, 0, 0), TRANSVERSE: (1, 1, 1), ROT_90: (1, 1, 0), ROT_180: (0, 1, 1), ROT_270: (1, 0, 1)}


def table(q, code):
    """a quantiser table (64, natural order) as the destination sees it"""
    q = np.asarray(q).reshape(8, 8)
    return (q.T if BITS[code & 7][0] else q).reshape(64).copy()


def frame(width, height, samp, code):
    """samp: [(h, v)] per component -> (refused, width, height, samp, trimmed) of the output; a single component is 1 x 1"""
    t, mh, mv = BITS[code & 7]
    samp = [(1, 1)] if len(samp) == 1 else [tuple(s) for s in samp]
    if t:
        width, height, samp = height, width, [(v, h) for h, v in samp]
    mcu_w, mcu_h = 8 * max(h for h, _ in samp), 8 * max(v for _, v in samp)
    refused = trimmed = False
    if mh and width % mcu_w:
        if code & TRIM and width > mcu_w:
            width, trimmed = width - width % mcu_w, True
        else:
            refused = True
    if mv and height % mcu_h:
        if code & TRIM and height > mcu_h:
            height, trimmed = height - height % mcu_h, True
        else:
            refused = True
    return refused, width, height, samp, trimmed


def blocks_of(width, height, samp):
    """[(blocks_h, blocks_w)] per component of a frame"""
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return [(my * v, mx * h) for h, v in samp]


def permute(plane, dst_bh, dst_bw, code):
    """one component's plane (blocks_h, blocks_w, 64) -> the destination's (dst_bh, dst_bw, 64) in int64, not requantised"""
    t, mh, mv = BITS[code & 7]
    p = np.asarray(plane, np.int64)
    p = p.reshape(p.shape[0], p.shape[1], 8, 8)
    if t:
        p = p.transpose(1, 0, 3, 2)
    canvas = np.zeros((max(dst_bh, p.shape[0]), max(dst_bw, p.shape[1]), 8, 8), np.int64)
    canvas[:p.shape[0], :p.shape[1]] = p
    d = canvas[:dst_bh, :dst_bw].copy()  # (what lies beyond the destination at the far edge is dropped)
    if mh:
        d = d[:, ::-1].copy()
        d[..., :, 1::2] *= -1
    if mv:
        d = d[::-1].copy()
        d[..., 1::2, :] *= -1
    return d.reshape(dst_bh, dst_bw, 64)


def transform_blocks(plane, dst_bh, dst_bw, code, q_old, q_new, precision=8):
    """-> (the destination plane in int16 under q_new, clamped; how many values were clamped).  q_old in the source's order."""
    return R.requant_blocks(permute(plane, dst_bh, dst_bw, code), table(q_old, code), q_new, precision)


def apply(pic, code):
    """pic: (width, height, samp, tables, planes) with a table and a plane per component -> the same of the kept output, or None
    where the picture is refused"""
    width, height, samp, tables, planes = pic
    refused, w, h, s, _ = frame(width, height, samp, code)
    if refused:
        return None
    out_tables = [table(q, code) for q in tables]
    out = [transform_blocks(planes[c], bh, bw, code, tables[c], out_tables[c], 16)[0] for c, (bh, bw) in enumerate(blocks_of(w, h, s))]
    return w, h, s, out_tables, out


def samp_of(info):
    return [(info.hsamp[c], info.vsamp[c]) for c in range(info.components)]


def transcode_planes(info, planes, out_info, code):
    """planes[c]: (blocks_h, blocks_w, 64) of the source frame `info` -> (the flat int16 planes of the output frame out_info of
    api.transcode_plan_transformed as the host coder takes them, coefficients that were clamped)"""
    flat = np.zeros(out_info.coef_count, np.int16)
    beyond = 0
    for c in range(out_info.components):
        src = np.asarray(planes[c]).reshape(info.blocks_h[c], info.blocks_w[c], 64)
        dst, n = transform_blocks(src, out_info.blocks_h[c], out_info.blocks_w[c], code, R.table(info, c), R.table(out_info, c), out_info.precision)
        beyond += n
        flat[out_info.coef_offset[c]:out_info.coef_offset[c] + dst.size] = dst.reshape(-1)
    return flat, beyond

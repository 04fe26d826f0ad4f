#!/usr/bin/env python3
"""Regenerate tests/golden/kernel_selection.json: what mijpeg_kernel_name and mijpeg_workspace_bytes answer for a fixed
list of batch descriptions.

Run against a build of the library (no device needed):   python tests/golden/make_kernel_selection.py

The cases cover every sampling layout the kernels know (4:2:0, 4:2:2, 4:4:0, 4:1:1, 4:4:4, one component, others, CMYK,
RGB stored as such) at 8 and 12 bit, each range gate of the selection from both sides, delta bounds, the caller's flags,
per-frame tables, int32 coefficients, DNL frames, strides and frames at the 32-bit offset limit, and JPEG XT frames read
from the golden streams plus variations of their parameter blocks.  Stored: the distinct outcomes (kernel name index,
workspace bytes), two characters per case that pick one, and a hash of the case list (tests/test_kernel_selection.py
rebuilds the list and requires the same answers).
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from libjpeg_amd import api  # noqa: E402

GOLDEN = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(GOLDEN, "kernel_selection.json")

# upper bounds on mijpeg_info::range_max the selection compares against
GATES = [1477, 2047, 7600, 8190, 16384, 45056, 49152, 65536]
FLAGS = [0, api.FLAG_FORCE_SAFE, api.FLAG_FORCE_GENERIC, api.FLAG_NO_COLOR_TRANSFORM, api.FLAG_FORCE_DOT2]
FRAMES = 3

# name: components, hsamp, vsamp, ycbcr
LAYOUTS = {
    "420": (3, [2, 1, 1], [2, 1, 1], 1),
    "422": (3, [2, 1, 1], [1, 1, 1], 1),
    "440": (3, [1, 1, 1], [2, 1, 1], 1),
    "411": (3, [4, 1, 1], [1, 1, 1], 1),
    "444": (3, [1, 1, 1], [1, 1, 1], 1),
    "grey": (1, [1], [1], 0),
    "grey2x2": (1, [2], [2], 0),
    "lumasub": (3, [1, 2, 2], [1, 2, 2], 1),
    "1x2": (3, [1, 1, 1], [2, 1, 1], 0),
    "mixed": (3, [2, 1, 2], [2, 1, 1], 1),
    "all2x2": (3, [2, 2, 2], [2, 2, 2], 1),
    "rgb": (3, [1, 1, 1], [1, 1, 1], 0),
    "rgb420": (3, [2, 1, 1], [2, 1, 1], 0),
    "cmyk": (4, [1, 1, 1, 1], [1, 1, 1, 1], 0),
    "ycck420": (4, [2, 1, 1, 2], [2, 1, 1, 2], 0),
    "two": (2, [2, 1], [2, 1], 0),
}

# layouts the range sweep leaves to the other cases
SWEEP_SKIPS = {"grey2x2", "two", "1x2", "mixed"}

# the XT golden streams whose parameter blocks seed the JPEG XT cases; the first ones' are varied as well
XT_VARIED = ["xt_129x71_420", "xt_200x120_420_rR4", "xt_int16/w420_r12", "xt_grey/ghdr"]
XT_STREAMS = XT_VARIED + [
    "xt_129x71_420_R2_rR3_dri3", "xt_33x17_422", "xt_64x48_444", "xt_general/a_q_and_r2", "xt_general/b_q_and_r2",
    "xt_general/enc_xyz", "xt_int8/enc_c", "xt_grey/g8", "xt_lonly/hdr_R1_420", "xt_lonly/g16_R1_seq",
]


def _quant(luma_max=30, chroma_max=40):
    """Two tables of small deltas; the largest entry of each is luma_max / chroma_max."""
    y = [1 + i % 20 for i in range(64)]
    c = [2 + i % 25 for i in range(64)]
    y[63], c[40] = luma_max, chroma_max
    return [y, c]


def _frame(layout, precision=8, width=97, height=61, luma_max=30, chroma_max=40):
    n, hs, vs, ycc = LAYOUTS[layout]
    f = api.frame_layout(width, height, n, hs, vs, _quant(luma_max, chroma_max), ycbcr=ycc)
    f.precision = precision
    f.fast_arith = 1
    return f


def _batch(info, flags=0, xt=None, frames=FRAMES, quant_dev=False, row_stride=0):
    b = api.MijpegBatch()
    C.memmove(C.byref(b.info), C.byref(info), C.sizeof(api.MijpegInfo))
    b.flags, b.frames, b.out_row_stride = flags, frames, row_stride
    b.quant_dev = 16 if quant_dev else None  # (only asked whether it is set)
    if xt is not None:
        b.xt = C.pointer(xt)
    return b


def _ranges():
    """(luma, chroma) range_max pairs: every gate from both sides, on all components, on luma alone and on chroma alone,
    and a few pairs around the 12-bit one-sum colour bound"""
    out = [(0, 0), (100, 100), (0, 100)]
    for g in GATES:
        for r in (g - 1, g):
            out += [(r, r), (r, 100), (100, r)]
    out += [(20000, 40000), (40000, 30000), (48000, 44000), (45000, 20000), (30000, 45055)]
    return out


def _set_ranges(f, luma, chroma):
    for c in range(f.components):
        f.range_max[c] = luma if c == 0 else chroma


def _plain_cases():
    for lay in LAYOUTS:
        for prec in (8, 12):
            for luma, chroma in [] if lay in SWEEP_SKIPS else _ranges():
                for flags in FLAGS:
                    f = _frame(lay, prec)
                    _set_ranges(f, luma, chroma)
                    yield f"{lay}/{prec}/r{luma},{chroma}/f{flags}", _batch(f, flags)
            for flags in FLAGS:
                base = f"{lay}/{prec}/f{flags}"
                for luma_max, chroma_max in ((2047, 40), (2048, 40), (30, 2047), (30, 2048)):
                    f = _frame(lay, prec, luma_max=luma_max, chroma_max=chroma_max)
                    _set_ranges(f, 100, 100)
                    yield f"{base}/delta{luma_max},{chroma_max}", _batch(f, flags)
                f = _frame(lay, prec)
                _set_ranges(f, 100, 100)
                f.fast_arith = 0
                yield f"{base}/slow", _batch(f, flags)
                for luma, chroma in ((100, 100), (100, 3000), (30000, 30000)):
                    f = _frame(lay, prec)
                    _set_ranges(f, luma, chroma)
                    yield f"{base}/own_tables/r{luma},{chroma}", _batch(f, flags, quant_dev=True)
                    yield f"{base}/one_frame/r{luma},{chroma}", _batch(f, flags, frames=1)
                    g = _frame(lay, prec)
                    _set_ranges(g, luma, chroma)
                    g.coef_wide = 1
                    yield f"{base}/coef_wide/r{luma},{chroma}", _batch(g, flags)
                # DNL: height 32 ends on a block row of the 2x subsampled planes; rows[c] says how many block rows exist
                for rows in (2, 3):
                    f = _frame(lay, prec, height=32)
                    _set_ranges(f, 100, 100)
                    f.dnl = 1
                    for c in range(f.components):
                        f.rows[c] = f.blocks_h[c] if f.suby[c] == 1 else rows
                    yield f"{base}/dnl_rows{rows}", _batch(f, flags)
                f = _frame(lay, prec, width=64, height=64)
                _set_ranges(f, 100, 100)
                line = 64 * f.components * (2 if prec > 8 else 1)
                yield f"{base}/negative_stride", _batch(f, flags, row_stride=-line)
                # 32-bit offsets: height * row_stride + line <= 2^32 - 1 holds for the first stride and not for the second
                last = (2**32 - 1 - line) // 64
                for rs in (last, last + 1):
                    yield f"{base}/row_stride{rs}", _batch(f, flags, row_stride=rs)
                big = _frame(lay, prec, width=65535, height=65535)
                _set_ranges(big, 100, 100)
                yield f"{base}/65535x65535", _batch(big, flags)


def _read_xt(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as fh:
        data = fh.read()
    d = api.Decoder(None)
    try:
        f = d.read(data)
        x = d.xt_params()
    finally:
        d.close()
    info = api.MijpegInfo()
    C.memmove(C.byref(info), C.byref(f), C.sizeof(api.MijpegInfo))
    for c in range(3):  # the decoder's table copies are gone with it; the selection only asks whether they exist
        x.qtable[c] = 1 if x.qtable[c] else None
        x.r2table[c] = 1 if x.r2table[c] else None
    return info, x


def _copy_xt(x):
    y = api.MijpegXtParams()
    C.memmove(C.byref(y), C.byref(x), C.sizeof(api.MijpegXtParams))
    return y


def _xt_variants(stream, x):
    """the parameter block as read, and the shapes the fused JPEG XT kernels do or do not cover"""
    yield "as_read", x
    if stream not in XT_VARIED:
        return
    edits = {
        "general": lambda y: setattr(y, "general", 1),
        "legacy_hidden1": lambda y: setattr(y, "hidden_bits", 1),
        "residual_hidden1": lambda y: (setattr(y, "residual_hidden_bits", 1), setattr(y, "residual_wide", 1)),
        "residual_hidden4": lambda y: (setattr(y, "residual_hidden_bits", 4), setattr(y, "residual_wide", 1)),
        "residual_hidden5": lambda y: (setattr(y, "residual_hidden_bits", 5), setattr(y, "residual_wide", 1)),
        "residual_wide_only": lambda y: setattr(y, "residual_wide", 1),
        "no_residual": lambda y: setattr(y, "no_residual", 1),
        "ltrafo_off": lambda y: setattr(y, "ltrafo_ycbcr", 0),
        "ltrafo_not_standard": lambda y: setattr(y, "ltrafo_standard", 0),
        "out_max255": lambda y: setattr(y, "out_max", 255),
        "ltable512": lambda y: setattr(y, "ltable_entries", 512),
        "residual_range65535": lambda y: [y.residual.range_max.__setitem__(c, 65535) for c in range(3)],
        "residual_range65536": lambda y: y.residual.range_max.__setitem__(2, 65536),
        "residual_delta2047": lambda y: y.residual.quant[y.residual.quant_index[1]].__setitem__(5, 2047),
        "residual_delta2048": lambda y: y.residual.quant[y.residual.quant_index[1]].__setitem__(5, 2048),
        "residual_narrower": lambda y: setattr(y.residual, "width", y.residual.width - 1),
        "residual_precision8": lambda y: setattr(y.residual, "precision", 8),
    }
    for name, edit in edits.items():
        y = _copy_xt(x)
        edit(y)
        yield name, y


def _xt_cases():
    for stream in XT_STREAMS:
        info0, x0 = _read_xt(stream)
        for vname, x in _xt_variants(stream, x0):
            # (the legacy frame's gates of the XT paths on every variant, the others on the block as read)
            gates = GATES if vname == "as_read" else [7600, 16384]
            for flags in FLAGS:
                base = f"xt/{stream}/{vname}/f{flags}"
                yield f"{base}/as_read", _batch(info0, flags, x)
                for g in gates:
                    for r in (g - 1, g):
                        f = api.MijpegInfo()
                        C.memmove(C.byref(f), C.byref(info0), C.sizeof(api.MijpegInfo))
                        _set_ranges(f, r, r)
                        yield f"{base}/r{r}", _batch(f, flags, x)
        for flags in FLAGS:
            base = f"xt/{stream}/f{flags}"
            yield f"{base}/no_params", _batch(info0, flags)  # (mijpeg_kernel_name asked without the parameter block)
            f = api.MijpegInfo()
            C.memmove(C.byref(f), C.byref(info0), C.sizeof(api.MijpegInfo))
            f.coef_wide = 1
            yield f"{base}/coef_wide", _batch(f, flags, x0)
            yield f"{base}/negative_stride", _batch(info0, flags, x0, row_stride=-4096)
            yield f"{base}/one_frame", _batch(info0, flags, x0, frames=1)
            for q in (2047, 2048):
                f = api.MijpegInfo()
                C.memmove(C.byref(f), C.byref(info0), C.sizeof(api.MijpegInfo))
                f.quant[f.quant_index[0]][9] = q
                yield f"{base}/delta{q}", _batch(f, flags, x0)


def cases():
    """[(label, MijpegBatch)]: the batch descriptions, in a fixed order"""
    return list(_plain_cases()) + list(_xt_cases())


def case_hash(cs) -> str:
    """sha256 over everything a case hands the library"""
    h = hashlib.sha256()
    for label, b in cs:
        h.update(label.encode())
        h.update(bytes(b.info))
        h.update(repr((b.quant_dev or 0, b.out_row_stride, b.frames, b.flags)).encode())
        if b.xt:
            h.update(bytes(b.xt.contents))
    return h.hexdigest()


# a case's answer as two characters: base 62 index into the table of (kernel name index, workspace bytes) pairs
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def decode(table):
    """[(kernel name, workspace bytes)] per case of a stored table"""
    codes = table["results"]
    out = []
    for i in range(0, len(codes), 2):
        k, w = table["outcomes"][DIGITS.index(codes[i]) * len(DIGITS) + DIGITS.index(codes[i + 1])]
        out.append((table["kernel_names"][k], w))
    return out


def answers(cs):
    """[(kernel name, workspace bytes)] per case"""
    L = api.lib()
    return [(L.mijpeg_kernel_name(C.byref(b)).decode(), int(L.mijpeg_workspace_bytes(C.byref(b)))) for _, b in cs]


def main():
    cs = cases()
    res = answers(cs)
    names = sorted({k for k, _ in res})
    outcomes = sorted({(names.index(k), w) for k, w in res})
    assert len(outcomes) <= len(DIGITS) ** 2
    index = {o: i for i, o in enumerate(outcomes)}
    codes = [index[(names.index(k), w)] for k, w in res]
    table = {
        "cases": len(cs),
        "case_sha256": case_hash(cs),
        "kernel_names": names,
        "outcomes": [list(o) for o in outcomes],
        "results": "".join(DIGITS[c // len(DIGITS)] + DIGITS[c % len(DIGITS)] for c in codes),
    }
    assert decode(table) == res
    with open(OUT, "w") as fh:
        json.dump(table, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(cs)} cases, {len(names)} kernel names, {len(outcomes)} outcomes -> {os.path.relpath(OUT, ROOT)} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()

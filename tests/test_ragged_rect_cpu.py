"""Crop windows of a ragged batch without a device: the planner of the window launches (mijpeg_ragged_rect_plan: clipping,
refusals, the tiles a window touches) against a brute-force tile count, the host half of the window launches' tables under the
sanitizers (tests/cxx/fused_window_tables.cpp around fused_list.hpp), and the machine code: the window instantiations exist in
namespaces of their own and use no scratch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libjpeg_amd import api
from test_isa_guard import LIB
from test_ragged_batch import READELF, _kernel_metadata
from test_ragged_twin_cpu import _run_under_sanitizers

EDGE = 2**31 - 1


def _info(w, h):
    f = api.MijpegInfo()
    f.width, f.height = w, h
    return f


def _brute_tiles(w, h, rect):
    """The 128 x 128 tiles of a w x h picture that hold a pixel of the rectangle, from a pixel mask: -> (set of (tx, ty))"""
    x0, y0, x1, y1 = rect
    xs = np.arange(w)
    ys = np.arange(h)
    cols = np.unique(xs[(xs >= x0) & (xs <= x1)] // 128)
    rows = np.unique(ys[(ys >= y0) & (ys <= y1)] // 128)
    return {(int(tx), int(ty)) for tx in cols for ty in rows}


def _seeded_pairs(n):
    """(w, h, rect): sizes 1..1100 (up to 9 x 9 tiles), rects of every kind -- random, single pixels, touching each edge, on tile seams,
    reaching beyond the picture, INT32_MAX."""
    rng = np.random.default_rng(20261020)
    out = []
    for k in range(n):
        w, h = int(rng.integers(1, 1101)), int(rng.integers(1, 1101))
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        kind = k % 8
        if kind == 0:
            x1, y1 = int(rng.integers(x0, w)), int(rng.integers(y0, h))
        elif kind == 1:
            x1, y1 = x0, y0  # one pixel
        elif kind == 2:
            x0, y0, x1, y1 = 0, 0, int(rng.integers(0, w)), int(rng.integers(0, h))  # the left and the top edge
        elif kind == 3:
            x1, y1 = w - 1, h - 1  # the right and the bottom edge
        elif kind == 4:
            x1, y1 = x0 + int(rng.integers(0, 3000)), y0 + int(rng.integers(0, 3000))  # beyond the picture: clipped
        elif kind == 5:
            x1, y1 = EDGE, EDGE
        elif kind == 6:  # on the seams: 127 / 128 on either side
            x0, y0 = min(w - 1, 128 * int(rng.integers(0, 9)) + int(rng.integers(0, 2)) * 127), min(h - 1, 128 * int(rng.integers(0, 9)) + int(rng.integers(0, 2)) * 127)
            x1, y1 = min(w - 1, x0 + int(rng.integers(0, 3))), min(h - 1, y0 + int(rng.integers(0, 3)))
        else:
            x0, y0, x1, y1 = 0, 0, w - 1, h - 1  # the whole picture
        out.append((w, h, (x0, y0, x1, y1)))
    return out


def test_planner_against_brute_force():
    pairs = _seeded_pairs(4000)
    tx0, ty0, ntx, nty = api.ragged_rect_plan([_info(w, h) for w, h, _ in pairs], [r for _, _, r in pairs])
    assert len(tx0) == len(pairs)
    for k, (w, h, r) in enumerate(pairs):
        clipped = (r[0], r[1], min(r[2], w - 1), min(r[3], h - 1))
        want = _brute_tiles(w, h, clipped)
        got = {(tx0[k] + i, ty0[k] + j) for i in range(ntx[k]) for j in range(nty[k])}
        assert got == want, (w, h, r)
        assert ntx[k] * nty[k] == len(want)
        assert (tx0[k], ty0[k]) == (r[0] >> 7, r[1] >> 7)
    # every tile count from one tile to the whole 9 x 9 was seen, and windows that leave tile column / row 0 out
    assert {1, 2, 4, 81} <= {a * b for a, b in zip(ntx, nty)}
    assert any(x > 0 for x in tx0) and any(y > 0 for y in ty0)


def test_planner_clipping_and_refusals():
    f = [_info(300, 270)]
    assert api.ragged_rect_plan(f, [(0, 0, 299, 269)]) == ([0], [0], [3], [3])
    assert api.ragged_rect_plan(f, [(0, 0, EDGE, EDGE)]) == ([0], [0], [3], [3])
    assert api.ragged_rect_plan(f, [(130, 129, 5000, 269)]) == ([1], [1], [2], [2])
    assert api.ragged_rect_plan(f, [(299, 269, 299, 269)]) == ([2], [2], [1], [1])
    assert api.ragged_rect_plan(f, [(127, 127, 128, 128)]) == ([0], [0], [2], [2])
    refused = [(-1, 0, 5, 5), (0, -1, 5, 5), (300, 0, 305, 5), (0, 270, 5, 275), (6, 0, 5, 5), (0, 6, 5, 5), (0, 0, -1, 5), (EDGE, EDGE, EDGE, EDGE),
               (-2**31, 0, 5, 5)]
    for r in refused:
        with pytest.raises(api.MijpegError) as e:
            api.ragged_rect_plan(f, [r])
        assert e.value.code == api.ERR_INVALID_PARAMETER, r
        with pytest.raises(api.MijpegError):  # one bad rectangle refuses the list
            api.ragged_rect_plan(f * 3, [(0, 0, 5, 5), r, (0, 0, 5, 5)])
    for w, h in ((0, 10), (10, 0), (-5, 10)):  # no picture, no window
        with pytest.raises(api.MijpegError):
            api.ragged_rect_plan([_info(w, h)], [(0, 0, 0, 0)])
    # argument errors
    L = api.lib()
    arr, rects = (api.MijpegInfo * 1)(f[0]), api.rect_array([(0, 0, 5, 5)])
    outs = [(C.c_int32 * 1)() for _ in range(4)]
    assert L.mijpeg_ragged_rect_plan(arr, rects, 1, *outs) == 0
    assert L.mijpeg_ragged_rect_plan(arr, rects, 0, *outs) == api.ERR_INVALID_PARAMETER
    for k in range(6):
        args = [arr, rects, 1] + outs
        args[k if k < 2 else k + 1] = None
        assert L.mijpeg_ragged_rect_plan(*args) == api.ERR_INVALID_PARAMETER, k


def test_crop_calls_argument_errors_without_a_device():
    """NULL lists and an object without a device or without a ragged batch are told so before anything else happens."""
    L = api.lib()
    d = api.Decoder(None)
    rects, dst, rows = api.rect_array([(0, 0, 5, 5)]), (C.c_void_p * 4)(), (C.c_int64 * 1)(64)
    st = api.MijpegRaggedRectStats()
    for fn in (L.mijpeg_reconstruct_ragged_rect_device, L.mijpeg_reconstruct_ragged_rect_planar_device):
        assert fn(None, rects, dst, rows, 0, 1) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, None, dst, rows, 0, 1) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, rects, None, rows, 0, 1) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, rects, dst, None, 0, 1) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, rects, dst, rows, 0, 1) == api.ERR_NOT_AVAILABLE  # created without a device
    assert L.mijpeg_ragged_rect_stats_get(d._h, None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_ragged_rect_stats_get(None, C.byref(st)) == api.ERR_INVALID_PARAMETER
    assert d.ragged_rect_stats() == dict(images=0, fused=0, copied=0, launches=0, workgroups=0, workgroups_full=0)
    with pytest.raises(ValueError):  # one crop, one destination and one stride per stream of the decode call
        d.reconstruct_ragged_rect_device([(0, 0, 1, 1)], [0], [0])
    d.close()


def test_decode_mixed_refuses_bad_crops_without_a_device():
    """decode_mixed(crops=...) raises ValueError before any device work: here there is no device to work on."""
    from libjpeg_amd import batch, synth

    streams = [synth.synth_jpeg(40, 30, 1, 85, "420", 0), synth.synth_jpeg(24, 16, 2, 85, "444", 0)]
    for bad in [(0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (40, 0, 5, 5), (0, 30, 5, 5), (1, 2, 3), (1, 2, 3, 4, 5), "abcd", 7, (1, 0, 2**31, 1)]:
        with pytest.raises(ValueError):
            batch.decode_mixed(streams, device=None, crops=[bad, None])
    with pytest.raises(ValueError):
        batch.decode_mixed(streams, device=None, crops=[None])  # one entry per stream
    # a rank is answerable for its own pictures' crops only (the other rank raises for this one)
    assert batch._checked_crops([(99, 0, 5, 5), (0, 0, 5, 5)], streams, [1]) == [None, (0, 0, 5, 5)]
    with pytest.raises(ValueError):
        batch._checked_crops([(99, 0, 5, 5), (0, 0, 5, 5)], streams, [0])


def test_fused_window_tables_under_sanitizers(tmp_path):
    """tests/cxx/fused_window_tables.cpp, a program of its own around fused_list.hpp: the window launches' tables in a heap buffer of
    exactly the layout's size -- offsets and alignment, first[] as the prefix of window tiles, every listed tile against its rectangle
    by brute force, the biased base -- under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "fused_window_tables")


# The window instantiations: the seven 8-bit ragged flavours in mij::window, the six with planes out in mij::window::planar
WINDOW_KERNELS = sorted(["fused420p_kernel", "fused420_kernel", "fused420_kernel", "fused422_kernel", "fused422_kernel", "fused444_kernel", "fused1_kernel"])
WINDOW_PLANAR_KERNELS = sorted(["fused420p_kernel", "fused420_kernel", "fused420_kernel", "fused422_kernel", "fused422_kernel", "fused444_kernel"])


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_window_instantiations_exist_and_use_no_scratch():
    meta = _kernel_metadata(LIB)
    pat = re.compile(r"^_ZN3mij6window(6planar)?\d+(fused(?:420p|420|422|444|1)_kernel)I((?:L[bi]\d+E)+)EEvNS_12Fused420ArgsE$")
    seen = {False: [], True: []}
    for name, k in meta.items():
        m = pat.match(name)
        if not m:
            assert "6window" not in name, f"a kernel of mij::window that is none of the fused texts: {name}"
            continue
        args = tuple(int(x) for x in re.findall(r"L[bi](\d+)E", m.group(3)))
        assert args[-1] == 1, f"{name}: a window flavour that is not ragged"  # RAGGED is the last template parameter of all five
        seen[bool(m.group(1))].append(m.group(2))
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
    assert sorted(seen[False]) == WINDOW_KERNELS and sorted(seen[True]) == WINDOW_PLANAR_KERNELS, seen

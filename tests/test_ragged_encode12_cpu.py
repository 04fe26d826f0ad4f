"""Ragged encode of lists that mix 8-bit and 12-bit pictures, the part that needs no device (mijpeg_encode_ragged_plan16 and the
argument checks of mijpeg_encode_ragged_device16 / mijpeg_encode_ragged16): the planner against mijpeg_frame_layout at
either precision, against the all-8-bit planner and against the quantiser tables in the streams the reference encoder wrote
(tests/golden/enc12); its argument errors; the device entry points on an object without a device; the machine code of the six ragged
12-bit forward kernels.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import enc12_util as U
from libjpeg_amd import api
from test_isa_guard import LIB
from test_ragged_batch import READELF, _kernel_metadata

SIDES = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 1000)
QUALITIES = (2, 30, 85, 100)


def _frame(w, h, layout, q=85, ri=0, pixels=0, row_stride=None):
    hs, vs = U.LAYOUTS[layout][0]
    return api.encode_frame(w, h, len(hs), q, (hs, vs), ri, pixels, row_stride)


def _quality_tables8(q):
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.mijpeg_quality_tables.restype = None
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    L.mijpeg_quality_tables(q, luma.ctypes.data, chroma.ctypes.data)
    return luma, chroma


def _planner_list():
    """77 descriptions: every side of SIDES as a width and as a height, every layout of enc12_util.LAYOUTS, the four qualities, restart
    intervals 0, 1, 3 and one beyond the MCU count; precisions alternate along the list."""
    names = list(U.LAYOUTS)
    out = []
    for i, w in enumerate(SIDES):
        for j in range(7):
            h = SIDES[(i * 3 + j * 5) % len(SIDES)]
            out.append((w, h, names[(i + j) % 7], QUALITIES[(i + j) % 4], (0, 1, 3, 65000)[(i + 2 * j) % 4]))
    return out, [12 if k % 2 else 8 for k in range(len(out))]


def test_planner_completes_every_frame_at_its_precision():
    cases, prec = _planner_list()
    assert {c[0] for c in cases} == set(SIDES) and {c[1] for c in cases} == set(SIDES) and {c[2] for c in cases} == set(U.LAYOUTS)
    assert {(c[2], p) for c, p in zip(cases, prec)} == {(lay, p) for lay in U.LAYOUTS for p in (8, 12)}
    frames = [_frame(*c) for c in cases]
    items, totals = api.encode_ragged_plan(frames, precision=prec)
    old_items, old_totals = api.encode_ragged_plan(frames)  # the same list, all 8-bit, through the old entry point
    assert len(items) == len(cases)
    for (w, h, lay, q, ri), p, it, old in zip(cases, prec, items, old_items):
        hs, vs = U.LAYOUTS[lay][0]
        nc = len(hs)
        got = it.info
        ref = api.frame_layout(w, h, nc, hs, vs, [np.array(got.quant[0][:]), np.array(got.quant[1][:])], quant_index=[0] * nc, ycbcr=1 if nc == 3 else 0,
                               precision=p)
        for k in ("width", "height", "components", "precision", "ycbcr", "mcus_x", "mcus_y", "coef_count", "sample_bytes"):
            assert getattr(got, k) == getattr(ref, k), (w, h, lay, p, k)
        assert (got.precision, got.sample_bytes) == (p, 2 if p == 12 else 1)
        for c in range(nc):
            for k in ("hsamp", "vsamp", "subx", "suby", "blocks_w", "blocks_h", "coef_offset", "quant_index"):
                assert getattr(got, k)[c] == getattr(ref, k)[c], (w, h, lay, p, k, c)
        # the tables of `quality`: mijpeg_quality_tables' at 8 bits; at 12 bits the same rule without the limit of 255 (the exact
        # values are pinned against the reference's streams in the next test)
        luma, chroma = _quality_tables8(q)
        t0, t1 = np.array(got.quant[0][:]), np.array(got.quant[1][:])
        if p == 8:
            assert np.array_equal(t0, luma) and np.array_equal(t1, chroma)
        else:
            assert np.array_equal(np.minimum(t0, 255), luma) and np.array_equal(np.minimum(t1, 255), chroma) and t0.max() <= 32767
        # nothing else depends on the precision
        for k in ("blocks", "intervals", "first_block", "first_interval", "coef_base", "pass_"):
            assert getattr(it, k) == getattr(old, k), (w, h, lay, p, k)
    assert bytes(totals) == bytes(old_totals)
    # ... with passes cut as well
    items, totals = api.encode_ragged_plan(frames, 4096, precision=prec)
    old_items, old_totals = api.encode_ragged_plan(frames, 4096)
    assert totals.passes > 3 and bytes(totals) == bytes(old_totals)
    for it, old in zip(items, old_items):
        assert (it.blocks, it.intervals, it.first_block, it.first_interval, it.coef_base, it.pass_) == \
               (old.blocks, old.intervals, old.first_block, old.first_interval, old.coef_base, old.pass_)


def test_quantiser_tables_are_the_reference_encoders(oracle):
    keys = sorted(U.CASES)
    assert {U.CASES[k][5] for k in keys} == set(QUALITIES)
    frames = [_frame(U.CASES[k][0], U.CASES[k][1], U.CASES[k][2], U.CASES[k][5], U.case_restart(k)) for k in keys]
    items, _ = api.encode_ragged_plan(frames, precision=[12] * len(keys))
    for k, it in zip(keys, items):
        gold, _ = U.golden_coefficients(k)
        assert list(gold.tq[:gold.ncomp]) == [0] * gold.ncomp
        assert list(it.info.quant_index[:gold.ncomp]) == [0] * gold.ncomp
        assert np.array_equal(np.array(it.info.quant[0][:], np.uint16), U.oracle_quant(gold, 0)), k
        assert (it.info.precision, it.info.sample_bytes) == (12, 2)
    q2 = items[keys.index("420_64x40_q2")].info
    assert max(q2.quant[0]) > 255 and max(q2.quant[1]) > 255  # 16-bit DQT entries
    # the 8-bit planner limits the same tables to 255
    old, _ = api.encode_ragged_plan([frames[keys.index("420_64x40_q2")]])
    assert max(old[0].info.quant[0]) == 255


def test_without_precisions_the_planner_is_the_old_one():
    cases, _ = _planner_list()
    frames = [_frame(*c) for c in cases]
    for pass_blocks in (0, 4096):
        old_items, old_totals = api.encode_ragged_plan(frames, pass_blocks)
        for prec in (None, [8] * len(frames)):
            n = len(frames)
            arr = (api.MijpegEncodeFrame * n)(*frames)
            items, totals = (api.MijpegEncodeRaggedItem * n)(), api.MijpegEncodeRaggedTotals()
            parr = None if prec is None else (C.c_int32 * n)(*prec)
            assert api.lib().mijpeg_encode_ragged_plan16(arr, parr, n, pass_blocks, items, C.byref(totals)) == 0
            assert bytes(totals) == bytes(old_totals)
            assert all(bytes(a) == bytes(b) for a, b in zip(items, old_items))


def test_planner_argument_errors():
    L = api.lib()
    good8, good12 = _frame(64, 48, "420", 85, 2), _frame(33, 17, "411", 30, 0)
    items, totals = (api.MijpegEncodeRaggedItem * 3)(), api.MijpegEncodeRaggedTotals()

    def plan(frame_list, prec, n=None, it=items, tot=totals):
        arr = (api.MijpegEncodeFrame * max(1, len(frame_list)))(*frame_list)
        parr = None if prec is None else (C.c_int32 * max(1, len(prec)))(*prec)
        return L.mijpeg_encode_ragged_plan16(arr, parr, len(frame_list) if n is None else n, 0, it, C.byref(tot) if tot is not None else None)

    assert plan([good8, good12], [8, 12]) == 0
    assert plan([good8, good12], [12, 8]) == 0
    assert plan([good8, good12], None) == 0
    for p in (0, 10, 16, -12, 9):
        assert plan([good12], [p]) == api.ERR_INVALID_PARAMETER, p
        assert plan([good8, good12, good8], [8, 12, p]) == api.ERR_INVALID_PARAMETER, p  # anywhere in the list
        assert plan([good8, good12, good8], [p, 12, 8]) == api.ERR_INVALID_PARAMETER, p
    assert plan([good12], [12], n=0) == api.ERR_INVALID_PARAMETER
    assert plan([good12], [12], n=-1) == api.ERR_INVALID_PARAMETER
    assert plan([good12], [12], it=None) == api.ERR_INVALID_PARAMETER
    assert plan([good12], [12], tot=None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_encode_ragged_plan16(None, (C.c_int32 * 1)(12), 1, 0, items, C.byref(totals)) == api.ERR_INVALID_PARAMETER

    def bad(**kw):
        f = _frame(64, 48, "420", 85, 2)
        for k, v in kw.items():
            if isinstance(v, tuple):
                for c, x in enumerate(v):
                    getattr(f, k)[c] = x
            else:
                setattr(f, k, v)
        return f

    # one picture of a mixed list spoilt, at either precision, as test_ragged_encode.py::test_planner_argument_errors spoils it
    for kw in (dict(components=0), dict(components=2), dict(components=4), dict(hsamp=(0, 1, 1)), dict(hsamp=(5, 1, 1)), dict(vsamp=(2, 0, 1)),
               dict(vsamp=(1, 1, 5)), dict(hsamp=(3, 2, 1)), dict(restart_interval=-1), dict(restart_interval=65536), dict(width=0),
               dict(width=65536), dict(height=0), dict(height=65536), dict(height=-3)):
        for p in (8, 12):
            assert plan([bad(**kw)], [p]) == api.ERR_INVALID_PARAMETER, (kw, p)
            assert plan([good8, bad(**kw), good12], [8, p, 12]) == api.ERR_INVALID_PARAMETER, (kw, p)
    for kw in (dict(restart_interval=65535), dict(width=65535, height=1), dict(hsamp=(4, 2, 1), vsamp=(4, 1, 2))):
        assert plan([good8, bad(**kw)], [8, 12]) == 0, kw
    with pytest.raises(api.MijpegError) as e:
        api.encode_ragged_plan([good8, good12], precision=[8, 10])
    assert e.value.code == api.ERR_INVALID_PARAMETER
    with pytest.raises(ValueError):
        api.encode_ragged_plan([good8, good12], precision=[8])


def test_device_entry_points_without_a_device():
    """What the old entry points return on such an object (test_ragged_encode.py), with the outputs cleared."""
    L = api.lib()
    d = api.Decoder(None)
    img16 = U.synth12(24, 16, 1)
    img8 = (img16 >> 4).astype(np.uint8)
    frames = [_frame(24, 16, "420", pixels=img16.ctypes.data, row_stride=24 * 6), _frame(24, 16, "420", pixels=img8.ctypes.data)]
    arr = (api.MijpegEncodeFrame * 2)(*frames)
    prec = (C.c_int32 * 2)(12, 8)
    for fn, old in ((L.mijpeg_encode_ragged_device16, L.mijpeg_encode_ragged_device), (L.mijpeg_encode_ragged16, L.mijpeg_encode_ragged)):
        for p in (prec, None):
            ptrs, sizes = (C.c_void_p * 2)(0xdead0, 0xdead0), (C.c_size_t * 2)(77, 77)
            rc = fn(d._h, arr, p, 2, 0, 0, ptrs, sizes)
            assert rc == api.ERR_NOT_AVAILABLE == old(d._h, arr, 2, 0, 0, (C.c_void_p * 2)(), (C.c_size_t * 2)())
            assert not ptrs[0] and not ptrs[1] and sizes[0] == 0 and sizes[1] == 0
            msg = C.c_char_p()
            assert L.mijpeg_last_error(d._h, C.byref(msg)) == api.ERR_NOT_AVAILABLE and b"device" in msg.value
        # argument checks come first and need no device either
        ptrs, sizes = (C.c_void_p * 2)(), (C.c_size_t * 2)()
        assert fn(d._h, arr, prec, 0, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, None, prec, 2, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, arr, prec, 2, 0, 0, None, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, arr, prec, 2, 0, 0, ptrs, None) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, arr, prec, 2, 0, 0x80, ptrs, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(None, arr, prec, 2, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER
    # the Python front ends: uint16 pictures are no longer narrowed, they reach the same refusal
    for call in (lambda: d.encode_ragged([img16, img8], 85, "420"), lambda: d.encode_ragged_device(frames, precision=[12, 8])):
        with pytest.raises(api.MijpegError) as e:
            call()
        assert e.value.code == api.ERR_NOT_AVAILABLE and "device" in e.value.message
    d.close()


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_ragged_12_bit_forward_kernels_exist_and_spill_nothing():
    meta = _kernel_metadata(LIB)
    ragged = re.compile(r"^_ZN3mij8ragged12\d+(fdct\w+_kernel)I((?:L[bi]\d+E)+)E")
    uniform = re.compile(r"^_ZN3mij\d+(fdct\w+_kernel)I((?:L[bi]\d+E)+)E")
    args_of = lambda m: tuple(int(x) for x in re.findall(r"L[bi](\d+)E", m.group(2)))
    twins = {}  # (kernel, template arguments in front of RAGGED) -> metadata of the uniform 12-bit flavour
    for name, k in meta.items():
        m = uniform.match(name)
        if m and args_of(m)[-2:] == (0, 12):
            twins[(m.group(1), args_of(m)[:-2])] = k
    seen = {}
    for name, k in meta.items():
        m = ragged.match(name)
        if not m:
            continue
        args = args_of(m)
        assert args[-2:] == (1, 12), f"{name}: only the ragged 12-bit flavours live in mij::ragged12"
        key = (m.group(1), args[:-2])
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k["vgpr_count"]) <= int(twins[key]["vgpr_count"]), f"{name}: more VGPRs than its uniform twin"
        seen[key] = k
    assert set(seen) == {("fdct420_tile_kernel", ()), ("fdct_interior_kernel", (1, 1)), ("fdct_interior_kernel", (2, 2)), ("fdct_interior_kernel", (2, 1)),
                         ("fdct_interior_kernel", (1, 2)), ("fdct_blocks_kernel", ())}
    # the tile kernel declares two workgroups per CU; at 128 registers a lane there is room for four of its waves on a SIMD
    assert int(seen[("fdct420_tile_kernel", ())]["vgpr_count"]) + int(seen[("fdct420_tile_kernel", ())].get("agpr_count", 0)) <= 128

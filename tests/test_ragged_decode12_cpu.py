"""Ragged decode of lists that mix 8-bit and 12-bit pictures (mijpeg_ragged_plan16, mijpeg_decode_ragged_device16),
the part that needs no device: the planner with the 12-bit layout groups, and a guard on the machine code of the seven ragged
instantiations of the 12-bit fused kernels -- no scratch, no spills, no more registers than the uniform per-frame-table twin, whose
count is read from the same library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import enc12_util as U
from libjpeg_amd import api
from test_isa_guard import LIB
from test_ragged_batch import LAYOUTS, READELF, _kernel_metadata, _layout

NAMES = list(LAYOUTS)  # 420, 422, 444, grey: the order of the group ids


def _layout12(w, h, hs, vs):
    f = _layout(w, h, hs, vs)
    f.precision = 12
    f.sample_bytes = 2
    return f


def _planner_list16():
    """400 frame descriptions, seeded: sizes 1..4100, the four layouts at both precisions, every ninth one something no group takes
    -- 8-bit and 12-bit 4:4:0 and 4:1:1, a 12-bit progressive frame, a 12-bit JPEG XT frame.  -> (infos, (layout, precision) or None)."""
    rng = np.random.default_rng(20261019)
    infos, eligible = [], []
    for i in range(400):
        w, h = int(rng.integers(1, 4101)), int(rng.integers(1, 4101))
        if i % 9 == 4:
            kind = (i // 9) % 6
            make = _layout if kind < 2 else _layout12
            if kind in (0, 2):
                f = make(w, h, (1, 1, 1), (2, 1, 1))  # 4:4:0
            elif kind in (1, 3):
                f = make(w, h, (4, 1, 1), (1, 1, 1))  # 4:1:1
            else:
                f = make(w, h, (2, 1, 1), (2, 1, 1))
                if kind == 4:
                    f.progressive = 1
                else:
                    f.xt = 1
            eligible.append(None)
        else:
            name, p12 = NAMES[int(rng.integers(0, 4))], bool(rng.integers(0, 2))
            f = (_layout12 if p12 else _layout)(w, h, *LAYOUTS[name])
            eligible.append((name, 12 if p12 else 8))
        infos.append(f)
    return infos, eligible


GEOMETRY = ("first_workgroup", "tiles_x", "tiles_y", "width", "height", "bw_y", "bh_y", "bw_c", "bh_c", "cw", "ch", "off_y", "off_cb", "off_cr")


def test_planner16_groups_ranges_and_bases():
    infos, eligible = _planner_list16()
    assert {e for e in eligible if e} == {(n, p) for n in NAMES for p in (8, 12)}
    group, frames, grids, total = api.ragged_plan16(infos)
    old_group, old_frames, old_grids, _ = api.ragged_plan(infos)
    assert len(grids) == 8 and api.RAGGED_GROUPS16[:4] == api.RAGGED_GROUPS and len(api.RAGGED_GROUPS16) == 8
    for i, e in enumerate(eligible):
        want = -1 if e is None else NAMES.index(e[0]) + (4 if e[1] == 12 else 0)
        assert group[i] == want, (i, e, group[i])
        if e is None or e[1] == 12:
            assert old_group[i] == -1  # (the old planner keeps every 12-bit frame out)
        else:  # an 8-bit entry: what mijpeg_ragged_plan gives -- group, workgroup range, geometry (the store lies elsewhere: below)
            assert old_group[i] == group[i]
            assert [getattr(frames[i], k) for k in GEOMETRY] == [getattr(old_frames[i], k) for k in GEOMETRY], i
    assert list(grids[:4]) == list(old_grids)
    # workgroup ranges: per group disjoint, in list order, exactly tiles_x * tiles_y per frame (128 x 128 tiles), no padding
    for g in range(8):
        at = 0
        for i, f in enumerate(infos):
            if group[i] != g:
                continue
            fr = frames[i]
            assert (fr.tiles_x, fr.tiles_y) == ((f.width + 127) // 128, (f.height + 127) // 128)
            assert fr.first_workgroup == at, (g, i)
            at += fr.tiles_x * fr.tiles_y
            assert (fr.width, fr.height, fr.bw_y, fr.bh_y) == (f.width, f.height, f.blocks_w[0], f.blocks_h[0])
            assert fr.cw == (f.width + 1) // 2 and fr.ch == (f.height if g % 4 == NAMES.index("422") else (f.height + 1) // 2)
            if f.components == 3:
                assert (fr.bw_c, fr.bh_c, fr.off_cb, fr.off_cr) == (f.blocks_w[1], f.blocks_h[1], f.coef_offset[1], f.coef_offset[2])
        assert grids[g] == at
    assert all(grids[g] > 0 for g in range(8)), list(grids)
    # coefficient stores: back to back in LIST order across both precisions, coef_count each
    at = 0
    for i, f in enumerate(infos):
        if group[i] < 0:
            continue
        assert frames[i].coef_base == at and f.coef_count > 0, i
        at += f.coef_count
    assert total == at


def test_planner16_on_the_reference_written_streams():
    """Headers as the parser fills them: the 14 streams the reference's 12-bit encoder wrote."""
    d = api.Decoder(None)
    keys = sorted(U.CASES)
    infos = [d.read_header(U.golden_stream(k)) for k in keys]
    d.close()
    assert all(f.precision == 12 for f in infos)
    group, frames, grids, total = api.ragged_plan16(infos)
    for k, g in zip(keys, group):
        layout = U.CASES[k][2]
        assert g == (4 + NAMES.index(layout) if layout in NAMES else -1), (k, g)
    assert api.ragged_plan(infos)[0] == [-1] * len(keys)
    assert total == sum(f.coef_count for f, g in zip(infos, group) if g >= 0)


def test_planner16_argument_errors():
    L = api.lib()
    f = _layout12(64, 64, *LAYOUTS["420"])
    group, frames, grids, total = (C.c_int32 * 1)(), (api.MijpegRaggedFrame * 1)(), (C.c_int32 * 8)(), C.c_int64()
    ok = (C.byref(f), 1, group, frames, grids, C.byref(total))
    assert L.mijpeg_ragged_plan16(*ok) == 0 and group[0] == 4 and list(grids) == [0, 0, 0, 0, 1, 0, 0, 0]
    assert L.mijpeg_ragged_plan16(C.byref(f), 0, group, frames, grids, C.byref(total)) == api.ERR_INVALID_PARAMETER
    for k in (0, 2, 3, 4, 5):
        args = list(ok)
        args[k] = None
        assert L.mijpeg_ragged_plan16(*args) == api.ERR_INVALID_PARAMETER, k
    # the decoder-object call: NULL lists, n = 0, an object without a device
    d = api.Decoder(None)
    status = (C.c_int32 * 1)()
    arr, sizes = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    assert L.mijpeg_decode_ragged_device16(d._h, arr, sizes, 0, 0, status) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_decode_ragged_device16(d._h, None, sizes, 1, 0, status) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_decode_ragged_device16(d._h, arr, sizes, 1, 0, None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_decode_ragged_device16(d._h, arr, sizes, 1, 0, status) == api.ERR_NOT_AVAILABLE
    d.close()


# ------------------------------------------------------------------------------------------------ machine code
# the seven ragged instantiations -> the uniform per-frame-table (QDEV) instantiation of the same kernel and flavour
RAGGED12 = {
    "_ZN3mij8ragged1215fused420_kernelILb1ELi2ELb1ELi12ELb0ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij15fused420_kernelILb1ELi2ELb1ELi12ELb0ELb0EEEvNS_12Fused420ArgsE",
    "_ZN3mij8ragged1215fused420_kernelILb1ELi2ELb1ELi12ELb1ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij15fused420_kernelILb1ELi2ELb1ELi12ELb1ELb0EEEvNS_12Fused420ArgsE",
    "_ZN3mij18fused422_12_kernelILb1ELb0ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij18fused422_12_kernelILb1ELb0ELb0EEEvNS_12Fused420ArgsE",
    "_ZN3mij18fused422_12_kernelILb1ELb1ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij18fused422_12_kernelILb1ELb1ELb0EEEvNS_12Fused420ArgsE",
    "_ZN3mij18fused444_12_kernelILb1ELb0ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij18fused444_12_kernelILb1ELb0ELb0EEEvNS_12Fused420ArgsE",
    "_ZN3mij18fused444_12_kernelILb1ELb1ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij18fused444_12_kernelILb1ELb1ELb0EEEvNS_12Fused420ArgsE",
    "_ZN3mij8ragged1213fused1_kernelILb1ELi12ELb1EEEvNS_12Fused420ArgsE": "_ZN3mij13fused1_kernelILb1ELi12ELb0EEEvNS_12Fused420ArgsE",
}


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_ragged_12bit_flavours_fit_their_twins_registers():
    meta = _kernel_metadata(LIB)
    for name, twin in RAGGED12.items():
        assert name in meta, f"ragged instantiation missing: {name}"
        assert twin in meta, f"uniform twin missing: {twin}"
        k, t = meta[name], meta[twin]
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, f"{name}: spills"
        assert int(k["vgpr_count"]) + int(k.get("agpr_count", 0)) <= int(t["vgpr_count"]) + int(t.get("agpr_count", 0)), \
            f"{name}: {k['vgpr_count']} VGPRs, the uniform twin has {t['vgpr_count']}"
        assert int(k["group_segment_fixed_size"]) == int(t["group_segment_fixed_size"]), name  # (the same LDS: the same workgroups per CU)
    # ... and these seven are all: no other ragged instantiation of a 12-bit kernel, inside mij::ragged12 or outside
    pat = re.compile(r"^_ZN3mij(?:8ragged12)?\d+fused(?:420|1|422_12|444_12)_kernelI((?:L[bi]\d+E)+)EEvNS_12Fused420ArgsE$")
    found = {n for n in meta if pat.match(n) and n.endswith("Lb1EEEvNS_12Fused420ArgsE") and ("Li12E" in n or "_12_kernel" in n)}
    assert found == set(RAGGED12), sorted(found ^ set(RAGGED12))

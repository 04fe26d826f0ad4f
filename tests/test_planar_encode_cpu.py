"""Planar (CHW) input for the ragged encode (include/mijpeg.h: mijpeg_encode_ragged_planar_device16, mijpeg_encode_planar_stats_get,
mijpeg_interleave_device) without a GPU: the planner, routing and tables of a planar pass as a program of its own under
the sanitizers, what the entry points answer before a device is touched, what the built library's code objects say about the
planar-input forward kernels, and the content the GPU tests rest on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import planar_encode_util as PU
from libjpeg_amd import api
from test_planar_cpu import _waves_per_simd
from test_ragged_batch import LIB, READELF, _kernel_metadata
from test_ragged_twin_cpu import _run_under_sanitizers


def test_planar_lists_under_sanitizers(tmp_path):
    """tests/cxx/encode_list_planar_tables.cpp around encode_list.hpp and encoder.cpp: planar lists of every routing, both precisions,
    with and without own tables, cut into passes -- a planar picture gets exactly the work items of its interleaved twin, on the planar
    lists; one off its dword boundaries the per-block list only; every plane-table entry, prefix table and work list read back from
    buffers of exactly the arenas' sizes -- under AddressSanitizer and UBSan.  Host code only."""
    _run_under_sanitizers(tmp_path, "encode_list_planar_tables", "encoder.cpp")


def _call(L, d, frames, planes, precision, n=None, streams=True, sizes=True, flags=0):
    n = len(frames) if n is None else n
    arr = (api.MijpegEncodeFrame * max(1, len(frames)))(*frames)
    flat = []
    for p in planes:
        flat += [q or None for q in p] + [None] * (4 - len(p))
    table = (C.c_void_p * max(4, len(flat)))(*flat)
    ptrs, sz = (C.c_void_p * max(1, n))(*([0xdead0] * max(1, n))), (C.c_size_t * max(1, n))(*([77] * max(1, n)))
    prec = None if precision is None else (C.c_int32 * max(1, n))(*precision)
    rc = L.mijpeg_encode_ragged_planar_device16(d, arr, table, prec, n, 0, flags, ptrs if streams else None, sz if sizes else None)
    return rc, [ptrs[i] for i in range(n)], [sz[i] for i in range(n)]


def test_entry_points_without_a_device():
    L = api.lib()
    some = 4096  # (never dereferenced)
    d = api.Decoder(None)
    colour = api.encode_frame(20, 10, 3, 85, "420", 0, 0, 20)
    grey = api.encode_frame(20, 10, 1, 85, "444", 0, 0, 20)
    good = ([colour, grey], [[some, some + 1, some + 2], [some]])

    def cleared(r):
        return all(not p for p in r[1]) and all(s == 0 for s in r[2])

    # NULL lists, n < 1, flags
    assert L.mijpeg_encode_ragged_planar_device16(None, None, None, None, 1, 0, 0, None, None) == api.ERR_INVALID_PARAMETER
    assert _call(L, None, *good, None)[0] == api.ERR_INVALID_PARAMETER
    assert _call(L, d._h, *good, None, streams=False)[0] == api.ERR_INVALID_PARAMETER
    assert _call(L, d._h, *good, None, sizes=False)[0] == api.ERR_INVALID_PARAMETER
    arr = (api.MijpegEncodeFrame * 2)(*good[0])
    ptrs, sz = (C.c_void_p * 2)(1, 1), (C.c_size_t * 2)(5, 5)
    assert L.mijpeg_encode_ragged_planar_device16(d._h, arr, None, None, 2, 0, 0, ptrs, sz) == api.ERR_INVALID_PARAMETER
    assert not ptrs[0] and not ptrs[1] and sz[0] == sz[1] == 0
    assert L.mijpeg_encode_ragged_planar_device16(d._h, None, (C.c_void_p * 8)(), None, 2, 0, 0, ptrs, sz) == api.ERR_INVALID_PARAMETER
    r = _call(L, d._h, *good, None, flags=1)
    assert r[0] == api.ERR_INVALID_PARAMETER and cleared(r)
    assert _call(L, d._h, [], [], None, n=0)[0] == api.ERR_INVALID_PARAMETER
    # a picture's own faults are INVALID_PARAMETER whether or not there is a device: they are looked at first
    short = api.encode_frame(20, 10, 3, 85, "420", 0, 0, 19)
    short12 = api.encode_frame(20, 10, 3, 85, "420", 0, 0, 39)
    odd12 = api.encode_frame(20, 10, 3, 85, "420", 0, 0, 41)
    ok12 = api.encode_frame(20, 10, 3, 85, "420", 0, 0, 40)
    grey12 = api.encode_frame(20, 10, 1, 85, "444", 0, 0, 40)
    for frames, planes, precision in (([colour, grey], [[some, None, some], [some]], None),  # a NULL plane the picture needs
                                      ([colour, grey], [[some, some, some], [None]], None),
                                      ([colour, grey], [[some, some], [some]], None),
                                      ([short, grey], good[1], None),  # a pitch below one line
                                      ([short12, grey], good[1], [12, 8]),
                                      ([odd12, grey], [[some, some, some], [some]], [12, 8]),  # an odd pitch at 12 bit
                                      ([ok12, grey], [[some, some + 1, some], [some]], [12, 8]),  # an odd address at 12 bit
                                      ([grey12, ok12], [[some + 1], [some, some, some]], [12, 12]),
                                      ([colour, grey], good[1], [8, 10]),  # a precision other than 8 or 12
                                      ([colour, grey], good[1], [16, 8]),
                                      ([api.encode_frame(20, 10, 2, 85, "444", 0, 0, 20), grey], good[1], None),  # two components
                                      ([api.encode_frame(0, 10, 3, 85, "444", 0, 0, 20), grey], good[1], None)):
        r = _call(L, d._h, frames, planes, precision)
        assert r[0] == api.ERR_INVALID_PARAMETER and cleared(r), (planes, precision)
    # what the interleaved call takes is taken: odd addresses and an odd pitch at 8 bit, even ones at 12 -- and then the object has no device
    for frames, planes, precision in ((good[0], good[1], None), (good[0], good[1], [8, 8]), ([ok12, grey12], [[some, some + 2, some + 6], [some]], [12, 12]),
                                      ([api.encode_frame(20, 10, 3, 85, "411", 0, 0, 21), grey], good[1], [8, 8])):
        r = _call(L, d._h, frames, planes, precision)
        assert r[0] == api.ERR_NOT_AVAILABLE and cleared(r), (planes, precision)
    # statistics
    st = api.MijpegEncodePlanarStats()
    assert L.mijpeg_encode_planar_stats_get(None, C.byref(st)) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_encode_planar_stats_get(d._h, None) == api.ERR_INVALID_PARAMETER
    assert d.encode_planar_stats() == dict(pictures=0, fused=0, two_pass=0, own_plane=0, interleave_launches=0)
    assert d.encode_ragged_stats()["pictures"] == 0
    with pytest.raises(api.MijpegError):
        d.encode_ragged_planar_device(good[0], good[1])
    with pytest.raises(ValueError):
        d.encode_ragged_planar_device(good[0], good[1][:1])
    # mijpeg_interleave_device
    src = (C.c_void_p * 4)(some, some, some, None)
    f = L.mijpeg_interleave_device
    assert f(None, src, 20, 20, 10, 3, 1, some, 60, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, None, 20, 20, 10, 3, 1, some, 60, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 20, 20, 10, 3, 1, None, 60, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 19, 20, 10, 3, 1, some, 60, 1) == api.ERR_INVALID_PARAMETER  # a plane pitch below a line
    assert f(d._h, src, 20, 20, 10, 3, 1, some, 59, 1) == api.ERR_INVALID_PARAMETER  # a destination pitch below a line
    assert f(d._h, src, 40, 20, 10, 3, 2, some, 119, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 20, 20, 10, 4, 1, some, 80, 1) == api.ERR_INVALID_PARAMETER  # a fourth plane that is not there
    assert f(d._h, src, 20, 20, 10, 0, 1, some, 60, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 20, 20, 10, 5, 1, some, 100, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 20, 20, 10, 3, 3, some, 180, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 20, 0, 10, 3, 1, some, 60, 1) == api.ERR_INVALID_PARAMETER
    assert f(d._h, src, 20, 20, 10, 3, 1, some, 60, 1) == api.ERR_NOT_AVAILABLE
    d.close()


FAMILIES = ["fdct420_tile_kernelILb1ELi8E", "fdct_blocks_kernelILb1ELi8E", "fdct_interior_kernelILi1ELi1ELb1ELi8E", "fdct_interior_kernelILi1ELi2ELb1ELi8E",
            "fdct_interior_kernelILi2ELi1ELb1ELi8E", "fdct_interior_kernelILi2ELi2ELb1ELi8E"]


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_the_planar_input_kernels_in_the_code_objects():
    """The six mij::planar_in instantiations exist, no others are in that namespace, none has scratch or spills at the launch bounds of
    its interleaved ragged twin (same workgroup size, no occupancy step lower); the eight interleave kernels likewise."""
    meta = _kernel_metadata(LIB)
    mine = {n: k for n, k in meta.items() if "planar_in" in n}
    found = []
    for name, k in mine.items():
        m = re.match(r"^_ZN3mij9planar_in\d+(fdct\w+?I(?:L[bi]\d+E)+)EEvNS0_10KernelArgsIXT\d?_EE4typeEi?$", name)
        assert m, name
        found.append(m.group(1))
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
        twin = name.replace("_ZN3mij9planar_in", "_ZN3mij").replace("NS0_10KernelArgs", "NS_10KernelArgs")
        assert twin in meta, f"{name}: no interleaved twin"
        t = meta[twin]
        assert int(t["private_segment_fixed_size"]) == 0 and k["max_flat_workgroup_size"] == t["max_flat_workgroup_size"] == "256"
        v, tv = int(k["vgpr_count"]) + int(k.get("agpr_count", 0)), int(t["vgpr_count"]) + int(t.get("agpr_count", 0))
        print(f"{m.group(1)}: {v} VGPRs (AGPRs included), the interleaved twin {tv}")
        assert _waves_per_simd(v) >= _waves_per_simd(tv), f"{name}: {v} registers, its twin {tv}: an occupancy step lower"
    assert sorted(found) == sorted(FAMILIES), sorted(found)
    inter = {n: k for n, k in meta.items() if re.match(r"^_ZN3mij\d+interleave_kernelILi[1-4]ELi[12]EEEvNS_14InterleaveArgsE$", n)}
    assert len(inter) == 8, sorted(inter)  # 1..4 components x 1 or 2 sample bytes
    for name, k in inter.items():
        assert int(k["private_segment_fixed_size"]) == 0 and int(k.get("vgpr_spill_count", 0)) == 0, f"{name}: scratch"


def test_content_tells_planes_and_positions_apart():
    for w, h in ((128, 128), (130, 200), (256, 144), (64, 64), (24, 40), (48, 24), (97, 61), (17, 15), (7, 9)):
        for bits in (8, 12):
            p = PU.planes(w, h, 11, 3, bits)
            assert p.shape == (3, h, w) and p.dtype == (np.uint8 if bits == 8 else np.uint16) and int(p.max()) < (1 << bits)
            assert PU.tells_planes_and_positions_apart(p) and PU.shifted_differs(p), (w, h, bits)
            assert not np.array_equal(p, PU.planes(w, h, 12, 3, bits))
    # ... and the checks are not beside the point
    flat = np.full((3, 8, 8), 7, np.uint8)
    assert not PU.tells_planes_and_positions_apart(flat)
    same = PU.planes(16, 16, 3)
    same[2] = same[0]
    assert not PU.tells_planes_and_positions_apart(same)
    stripes = np.broadcast_to(np.arange(16, dtype=np.uint8)[None, None, :] * np.array([1, 2, 3], np.uint8)[:, None, None], (3, 16, 16))
    assert not PU.tells_planes_and_positions_apart(stripes)  # constant along y
    assert PU.tells_planes_and_positions_apart(PU.planes(1, 1, 5))

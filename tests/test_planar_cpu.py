"""Planar output (include/mijpeg.h: mijpeg_reconstruct_planar_device and its batch and ragged forms) without a GPU:
what the calls answer before a device is touched, and what the built library's code objects say about the planar kernels."""
import ctypes as C
import os
import re

import pytest

from conftest import golden_jpeg
from libjpeg_amd import api
from test_ragged_batch import LIB, READELF, _kernel_metadata


def _planes(*ptrs):
    return (C.c_void_p * 4)(*[p or None for p in ptrs])


def test_arguments_are_checked_before_a_device_is_touched():
    L = api.lib()
    some = 4096  # (never dereferenced: every call below is answered from its arguments and the object's state)
    good = _planes(some, some, some)
    d = api.Decoder(None)
    # null pointers
    assert L.mijpeg_reconstruct_planar_device(None, good, 64, 0, 1) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_reconstruct_planar_device(d._h, None, 64, 0, 1) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_reconstruct_batch_planar_device(None, some, 0, 0, 0, 0, 1) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_reconstruct_batch_planar_device(d._h, None, 0, 0, 0, 0, 1) == api.ERR_INVALID_PARAMETER
    rows = (C.c_int64 * 1)(64)
    assert L.mijpeg_reconstruct_ragged_planar_device(None, good, rows, 0, 1) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_reconstruct_ragged_planar_device(d._h, None, rows, 0, 1) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_reconstruct_ragged_planar_device(d._h, good, None, 0, 1) == api.ERR_INVALID_PARAMETER
    st = api.MijpegPlanarStats()
    assert L.mijpeg_planar_stats_get(None, C.byref(st)) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_planar_stats_get(d._h, None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_planar_stats_get(d._h, C.byref(st)) == 0 and st.images == 0
    # a decoded picture (200 x 120, three components), no device: its destination is checked first ...
    f = d.read(golden_jpeg("pil_200x120_420_dri8"))
    assert (f.width, f.components) == (200, 3)
    assert L.mijpeg_reconstruct_planar_device(d._h, good, 199, 0, 1) == api.ERR_INVALID_PARAMETER  # short stride
    assert L.mijpeg_reconstruct_planar_device(d._h, _planes(some, None, some), 200, 0, 1) == api.ERR_INVALID_PARAMETER  # missing plane
    assert L.mijpeg_reconstruct_planar_device(d._h, _planes(some, some), 200, 0, 1) == api.ERR_INVALID_PARAMETER
    # ... and a good one gets the interleaved twin's answer for an object without a device
    twin = L.mijpeg_reconstruct_device(d._h, some, 600, 0, 1)
    assert twin != 0 and L.mijpeg_reconstruct_planar_device(d._h, good, 200, 0, 1) == twin
    twin = L.mijpeg_reconstruct_batch_device(d._h, some, 600 * 120, 600, 0, 1)
    assert twin != 0 and L.mijpeg_reconstruct_batch_planar_device(d._h, some, 3 * 200 * 120, 200 * 120, 200, 0, 1) == twin
    dst = (C.c_void_p * 1)(some)
    twin = L.mijpeg_reconstruct_ragged_device(d._h, dst, rows, 0, 1)
    assert twin != 0 and L.mijpeg_reconstruct_ragged_planar_device(d._h, good, rows, 0, 1) == twin
    d.close()


def _waves_per_simd(vgprs):
    """Waves a SIMD of gfx950 holds at this many VGPRs (512 per lane, allocated in eights): the occupancy step."""
    return min(8, 512 // (-(-max(1, vgprs) // 8) * 8))


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_the_planar_kernels_in_the_code_objects():
    meta = _kernel_metadata(LIB)
    pat = re.compile(r"^_ZN3mij6planar\d+(fused(?:420p|420|422|444)_kernel)I((?:L[bi]\d+E)+)EEvNS_12Fused420ArgsE$")
    found = []
    for name, k in meta.items():
        m = pat.match(name)
        if not m:
            continue
        found.append(m.group(1))
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
        twin = name.replace("_ZN3mij6planar", "_ZN3mij")  # the interleaved ragged instantiation with the same template arguments
        assert twin in meta, f"{name}: no interleaved twin"
        v, tv = int(k["vgpr_count"]), int(meta[twin]["vgpr_count"])
        print(f"{m.group(1)}<{m.group(2)}>: {v} VGPRs, the interleaved twin {tv}")
        assert _waves_per_simd(v) >= _waves_per_simd(tv), f"{name}: {v} VGPRs, its twin {tv}: an occupancy step lower"
    # packed 4:2:0; 4:2:0 fast and safe; 4:2:2 packed and wide; 4:4:4
    assert sorted(found) == sorted(["fused420p_kernel", "fused420_kernel", "fused420_kernel", "fused422_kernel", "fused422_kernel", "fused444_kernel"])
    deint = {n: k for n, k in meta.items() if re.match(r"^_ZN3mij\d+deinterleave_kernelILi[1-4]ELi[12]EEEvNS_16DeinterleaveArgsE$", n)}
    assert len(deint) == 8, sorted(deint)  # 1..4 components x 1 or 2 sample bytes
    for name, k in deint.items():
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"

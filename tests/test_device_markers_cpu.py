"""Device marker search (mijpeg_set_device_markers), the part that needs no GPU: the reference model of the
primitive's contract is pinned to the host's own search (mijpeg_unstuffed_scan), the host half of the opt-in route stages the
raw segment, the setter's argument errors, and a guard on the search kernels' machine code (no scratch, no spills).
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import markers_model as M
from libjpeg_amd import api, synth
from test_isa_guard import LIB, gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
LAYOUTS = [("420", 160, 120), ("444", 127, 129), ("grey", 333, 200)]


def layout_stream(name, w, h, dri, quality, seed=7):
    if name == "grey":
        return synth.encode_jpeg(synth.synth_image(w, h, seed, channels=1), quality, restart_mcus=dri)
    return synth.synth_jpeg(w, h, seed, quality, name, dri)


def host_search(d, data):
    """(bytes, begin[], intervals) of the host's search for the parsed stream of decoder d (mijpeg_unstuffed_scan)."""
    L = api.lib()
    L.mijpeg_unstuffed_scan.restype = C.c_int64
    L.mijpeg_unstuffed_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32)]
    nint = C.c_int32()
    total = L.mijpeg_unstuffed_scan(d._h, None, 0, None, 0, 0, C.byref(nint))
    assert total >= 0
    buf, begin = (C.c_uint8 * max(1, total))(), (C.c_uint32 * nint.value)()
    assert L.mijpeg_unstuffed_scan(d._h, buf, total, begin, nint.value, 0, None) == total
    return bytes(buf[:total]), list(begin), nint.value


@pytest.mark.parametrize("name,w,h", LAYOUTS)
def test_model_is_the_hosts_search(name, w, h):
    d = api.Decoder(None)
    for dri in (1, 4, 7):
        for quality in (50, 99):
            data = layout_stream(name, w, h, dri, quality)
            d.read(data)
            kept, begin, nint = host_search(d, data)
            seg = data[M.ecs_offset(data):]
            m = M.search(seg, nint)
            assert m["flags"] == 0 and m["term"] == len(seg) - 2, (dri, quality, m["flags"])
            assert m["markers"] + 1 == nint
            assert m["kept"] == kept and m["begin"] == begin, (dri, quality)
    d.close()


def test_model_flags():
    s = M.search
    assert s(b"", 1) == dict(flags=M.NO_END, term=0, total=0, kept=b"", markers=0, begin=[0], end=[0])
    assert s(b"\xff", 1)["flags"] == M.NO_END and s(b"\xff", 1)["term"] == 1
    assert s(b"ab\xff\x00c\xff\xd9", 1)["kept"] == b"ab\xffc" and s(b"ab\xff\x00c\xff\xd9", 1)["term"] == 5
    assert s(b"a\xff\xd0b\xff\xd9", 2)["flags"] == 0 and s(b"a\xff\xd0b\xff\xd9", 2)["begin"] == [0, 1]
    assert s(b"a\xff\xd1b\xff\xd9", 2)["flags"] == M.SEQUENCE
    assert s(b"a\xff\xd0b\xff\xd9", 3)["flags"] == M.COUNT and s(b"a\xff\xd0b\xff\xd9", 1)["flags"] == M.COUNT
    assert s(b"a\xff\xff\xd0b\xff\xd9", 2)["flags"] == M.FILL
    assert s(b"a\xff\xd9\xff\xd0\xff\xff\xff\x00", 1)["flags"] == 0  # nothing behind the terminator counts


def test_host_half_stages_the_raw_segment():
    streams = [layout_stream("420", 160, 120, 4, q, seed) for q, seed in ((50, 1), (85, 2), (99, 3))]
    d = api.Decoder(None)
    d.set_device_markers(1)
    d.prepare_batch_host(streams)
    for i, s in enumerate(streams):
        assert d.device_markers_staging(i) == s[M.ecs_offset(s):], i
    assert d.device_markers_staging(len(streams)) is None
    assert d.device_markers_stats() == (3, 0)
    # one stream that does not qualify (no restart markers): the whole call takes the ordinary route, which still succeeds
    d.prepare_batch_host(streams[:2] + [layout_stream("420", 160, 120, 0, 85)])
    assert d.device_markers_staging(0) is None
    assert d.device_markers_stats() == (3, 3)
    # bytes behind EOI: not the plain case either
    d.prepare_batch_host([streams[0] + b"\x00"])
    assert d.device_markers_stats() == (3, 4)
    # errors are the ordinary route's
    with pytest.raises(api.MijpegError):
        d.prepare_batch_host([streams[0], b"\xff\xd8 not a jpeg at all"])
    d.set_device_markers(0)
    d.prepare_batch_host(streams)
    assert d.device_markers_staging(0) is None and d.device_markers_stats() == (3, 6)
    d.close()


def test_setter_argument_errors():
    L = api.lib()
    d = api.Decoder(None)
    assert L.mijpeg_set_device_markers(None, 1) == api.ERR_INVALID_PARAMETER
    for bad in (-1, 2, 7):
        assert L.mijpeg_set_device_markers(d._h, bad) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_set_device_markers(d._h, 1) == 0 and L.mijpeg_set_device_markers(d._h, 0) == 0
    assert L.mijpeg_device_markers_stats(None, None, None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_device_markers_stats(d._h, None, None) == 0
    assert L.mijpeg_batch_pipeline_device_markers(None, 1) == api.ERR_INVALID_PARAMETER
    term, flags = C.c_uint32(), C.c_uint32()
    ok = [d._h, b"ab", 2, 1, None, 0, None, None, C.byref(term), C.byref(flags)]
    assert L.mijpeg_device_marker_search(None, *ok[1:]) == api.ERR_INVALID_PARAMETER
    for k, v in ((3, 0), (8, None), (9, None), (1, None)):
        args = list(ok)
        args[k] = v
        assert L.mijpeg_device_marker_search(*args) == api.ERR_INVALID_PARAMETER, k
    assert L.mijpeg_device_marker_search(*ok) == api.ERR_NOT_AVAILABLE  # created without a device
    d.close()


def _kernel_metadata(path):
    """{mangled name: {field: value}} of the gfx950 code objects' AMDGPU metadata notes."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(gfx950_code_objects(path)):
            f = os.path.join(tmp, f"k{i}.co")
            with open(f, "wb") as fh:
                fh.write(co)
            txt = subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout
            cur = None
            for ln in txt.splitlines():
                head = re.match(r"^  - \.(\w+):\s*(.*)", ln)
                field = head or re.match(r"^    \.(\w+):\s*(.*)", ln)
                if head:
                    cur = {}
                if field and cur is not None:
                    cur[field.group(1)] = field.group(2).strip()
                    if field.group(1) == "name":
                        out[cur["name"]] = cur
    return out


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_search_kernels_use_no_scratch():
    meta = _kernel_metadata(LIB)
    found = {n: k for n, k in meta.items() if re.search(r"marker_(count|write)_kernel", n)}
    assert len(found) == 2, sorted(found)
    for name, k in found.items():
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name

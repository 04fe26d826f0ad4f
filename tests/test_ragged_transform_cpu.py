"""The transforms of the ragged transcode, without a device: the numpy model (tests/transform_model.py) pinned by a float64
inverse DCT and by the group's laws, the host twin of the kernel (mijpeg_transform_blocks) against the model at tolerance 0, the plan of
a picture (mijpeg_transcode_plan_transformed), the EXIF parser of batch.transcode_mixed, the plan, layout and both work lists of a
pass under the sanitizers as a program of its own, and the kernel's figures in the built code object."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import requant_model as R
import transform_model as M
from conftest import ROOT, golden_jpeg
from libjpeg_amd import api, batch
from test_ragged_batch import LIB, READELF, _kernel_metadata

# (width, height, [(h, v)]) on frames of whole MCUs
CASES = {"420": (48, 32, [(2, 2), (1, 1), (1, 1)]), "422": (32, 16, [(2, 1), (1, 1), (1, 1)]), "444": (24, 40, [(1, 1)] * 3), "grey": (8, 24, [(1, 1)]),
         "411": (32, 8, [(4, 1), (1, 1), (1, 1)])}
NUMPY_OPS = {M.NONE: lambda a: a, M.FLIP_H: np.fliplr, M.FLIP_V: np.flipud, M.TRANSPOSE: lambda a: a.T, M.TRANSVERSE: lambda a: np.rot90(a.T, 2),
             M.ROT_90: lambda a: np.rot90(a, -1), M.ROT_180: lambda a: np.rot90(a, 2), M.ROT_270: lambda a: np.rot90(a, 1)}


def _picture(name, seed=0, amplitude=200):
    """-> (width, height, samp, tables, planes): random planes, a table without symmetry per component"""
    w, h, samp = CASES[name]
    rng = np.random.default_rng(4350 + seed + sum(map(ord, name)))
    tables = [rng.permutation(np.arange(1, 65)) + 3 * c for c in range(len(samp))]
    planes = [rng.integers(-amplitude, amplitude + 1, (bh, bw, 64)).astype(np.int16) for bh, bw in M.blocks_of(w, h, samp)]
    return w, h, samp, tables, planes


def _info(pic, precision=8, tables=None):
    """the frame a decoder reports for a picture of the model: component c on table c"""
    w, h, samp, own, _ = pic
    return api.frame_layout(w, h, len(samp), [s[0] for s in samp], [s[1] for s in samp], tables or [list(t) for t in own], quant_index=list(range(len(samp))),
                            ycbcr=int(len(samp) == 3), precision=precision)


# ------------------------------------------------------------------------------------------------ the model is pinned by mathematics
_k = np.arange(8)
_BASIS = np.sqrt(np.where(_k == 0, 1 / 8, 2 / 8))[:, None] * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)  # [frequency, sample]


def _samples(plane, q):
    """the float64 inverse DCT of the dequantised plane (blocks_h, blocks_w, 64) at the component's own resolution"""
    bh, bw, _ = plane.shape
    f = (np.asarray(plane, np.float64) * np.asarray(q, np.float64)).reshape(bh, bw, 8, 8)
    return np.einsum("vy,hwvu,ux->hywx", _BASIS, f, _BASIS).reshape(bh * 8, bw * 8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_is_the_numpy_operation_on_the_samples(name):
    pic = _picture(name)
    _, _, samp, tables, planes = pic
    for code in range(8):
        out = M.apply(pic, code)
        assert out is not None, (name, code)
        w, h, s, out_tables, out_planes = out
        assert (w, h) == ((pic[1], pic[0]) if M.BITS[code][0] else (pic[0], pic[1]))
        assert s == ([(v, hh) for hh, v in samp] if M.BITS[code][0] else samp)
        for c in range(len(samp)):
            want = NUMPY_OPS[code](_samples(planes[c], tables[c]))
            got = _samples(out_planes[c], out_tables[c])
            assert got.shape == want.shape, (name, code, c)
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (name, M.NAMES[code], c)


def _same(a, b):
    return a[:3] == b[:3] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_group_laws_on_the_model(name):
    pic = _picture(name, 1)
    pic = (pic[0], pic[1], [(1, 1)] if len(pic[2]) == 1 else pic[2], pic[3], pic[4])

    def chain(*codes):
        p = pic
        for code in codes:
            p = M.apply(p, code)
        return p

    for code in (M.FLIP_H, M.FLIP_V, M.TRANSPOSE, M.TRANSVERSE, M.ROT_180):
        assert _same(chain(code, code), pic), M.NAMES[code]
    assert _same(chain(M.ROT_90, M.ROT_90, M.ROT_90, M.ROT_90), pic)
    assert _same(chain(M.ROT_90, M.ROT_270), pic) and _same(chain(M.ROT_270, M.ROT_90), pic)
    assert _same(chain(M.FLIP_H, M.TRANSPOSE), chain(M.ROT_270)) and _same(chain(M.TRANSPOSE, M.FLIP_H), chain(M.ROT_90))
    assert _same(chain(M.ROT_90, M.ROT_90), chain(M.ROT_180)) and _same(chain(M.NONE), pic)
    assert not _same(chain(M.ROT_90), chain(M.ROT_270))


# ------------------------------------------------------------------------------------------------ the host twin
def _quality_table(quality):
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    luma, chroma = (C.c_uint16 * 64)(), (C.c_uint16 * 64)()
    L.mijpeg_quality_tables(quality, luma, chroma)
    return np.array(luma[:], np.int64)


@pytest.mark.parametrize("precision", [8, 12])
def test_host_twin_equals_the_model(precision):
    rng = np.random.default_rng(4351 + precision)
    dc_min, dc_max, ac_max = R.coding_range(precision)
    q_old = rng.permutation(np.arange(1, 65))
    noise = rng.integers(-ac_max // 64, ac_max // 64 + 1, (5, 3, 64)).astype(np.int16)
    edges = np.resize(np.array([ac_max, -ac_max, ac_max + 1, -ac_max - 1, 1, -1, 0, ac_max - 1, 32767, -32768, -32767]), (5, 3, 64)).astype(np.int16)
    edges[..., 0] = np.resize(np.array([dc_min, dc_max, dc_min - 1, dc_max + 1, 0]), (5, 3))
    clamps = 0
    for code in range(8):
        t = M.BITS[code][0]
        for plane in (noise, edges):
            for dbh, dbw in {(3, 5) if t else (5, 3), (2, 2), (6, 6)}:  # the source's own extent, a trimmed one, one with blocks without a source
                for q_new in (M.table(q_old, code), _quality_table(30), _quality_table(95), np.ones(64, np.int64)):
                    got, n = api.transform_blocks(plane, dbh, dbw, code, q_old, q_new, precision)
                    want, m = M.transform_blocks(plane, dbh, dbw, code, q_old, q_new, precision)
                    assert np.array_equal(got, want) and n == m, (precision, M.NAMES[code], dbh, dbw)
                    clamps += n
    assert clamps > 0
    # kept tables and values inside the range: the permutation alone, and NONE is mijpeg_requantize
    got, n = api.transform_blocks(noise, 3, 5, M.ROT_90, q_old, M.table(q_old, M.ROT_90), precision)
    assert n == 0 and np.array_equal(got, M.permute(noise, 3, 5, M.ROT_90))
    got, n = api.transform_blocks(edges, 5, 3, M.NONE, q_old, _quality_table(95), precision)
    want, m = api.requantize(edges.reshape(-1, 64), q_old, _quality_table(95), precision)
    assert np.array_equal(got.reshape(-1, 64), want) and n == m
    L = api.lib()
    one, zero, buf, dst = np.ones(64, np.uint16), np.zeros(64, np.uint16), np.zeros(64, np.int16), np.zeros(64, np.int16)
    args = lambda **kw: [kw.get("src", buf.ctypes.data), kw.get("sbw", 1), 1, kw.get("dst", dst.ctypes.data), 1, 1, kw.get("code", 0), one.ctypes.data,
                         kw.get("q", one.ctypes.data), kw.get("precision", 8)]
    assert L.mijpeg_transform_blocks(*args()) == 0
    for bad in (dict(src=None), dict(dst=None), dict(dst=buf.ctypes.data), dict(sbw=0), dict(code=8), dict(code=-1), dict(q=zero.ctypes.data), dict(precision=10)):
        assert L.mijpeg_transform_blocks(*args(**bad)) == api.ERR_INVALID_PARAMETER, bad


# ------------------------------------------------------------------------------------------------ the plan
def _check_plan(f, samp, code, quality, want_size):
    """the plan of frame f under `code` against the model's frame; want_size: (w, h) or None for the geometry's refusal"""
    rc, out, ri, kept = api.transcode_plan_transformed(f, api.TRANSCODE_KEEP if quality is None else quality, -1, code)
    refused, w, h, s, _ = M.frame(f.width, f.height, samp, code)
    if want_size is None:
        assert refused and rc == api.ERR_NOT_AVAILABLE and not bytes(out).strip(b"\0") and ri == 0 and not kept, (code, rc)
        return None
    assert not refused and rc == 0 and (out.width, out.height) == (w, h) == want_size, (code, rc, out.width, out.height)
    nc = len(s)
    assert [(out.hsamp[c], out.vsamp[c]) for c in range(nc)] == s and out.components == nc and out.precision == f.precision
    assert [(out.blocks_h[c], out.blocks_w[c]) for c in range(nc)] == M.blocks_of(w, h, s)
    if quality is None:
        assert kept and [out.quant_index[c] for c in range(nc)] == [f.quant_index[c] for c in range(nc)]
        assert all(list(out.quant[t]) == list(M.table(f.quant[t][:], code)) for t in range(4))
    else:  # the tables of the quality as the untransformed plan writes them: the target is not transposed
        plain = api.transcode_plan(f, quality)[1]
        assert not kept and [out.quant_index[c] for c in range(nc)] == [0] * nc and all(list(out.quant[t]) == list(plain.quant[t]) for t in range(4))
    want = api.frame_layout(w, h, nc, [x[0] for x in s], [x[1] for x in s], [list(out.quant[t]) for t in range(4)], quant_index=[out.quant_index[c] for c in range(nc)],
                            ycbcr=int(nc == 3), precision=f.precision)
    assert bytes(out) == bytes(want)
    return out


def test_plan_transformed():
    for name in CASES:
        pic = _picture(name)
        for precision in (8, 12):
            f = _info(pic, precision)
            for code in range(8):
                for quality in (None, 75):
                    t = M.BITS[code][0]
                    _check_plan(f, pic[2], code, quality, (pic[1], pic[0]) if t else (pic[0], pic[1]))
                    _check_plan(f, pic[2], code | M.TRIM, quality, (pic[1], pic[0]) if t else (pic[0], pic[1]))
    # NONE is the plan without a transform
    f = _info(_picture("422"))
    assert bytes(api.transcode_plan_transformed(f, 50, 3, M.NONE)[1]) == bytes(api.transcode_plan(f, 50, 3)[1])
    # partial MCUs: a mirrored axis is refused or trimmed, the others keep theirs
    samp = [(2, 2), (1, 1), (1, 1)]
    tabs = [list(range(1, 65)), list(range(2, 66))]
    f = api.frame_layout(50, 35, 3, [2, 1, 1], [2, 1, 1], tabs)
    for code, size in ((M.FLIP_H, None), (M.FLIP_H | M.TRIM, (48, 35)), (M.FLIP_V | M.TRIM, (50, 32)), (M.FLIP_V, None), (M.TRANSPOSE, (35, 50)), (M.ROT_90, None),
                       (M.ROT_90 | M.TRIM, (32, 50)), (M.ROT_270, None), (M.ROT_270 | M.TRIM, (35, 48)), (M.ROT_180 | M.TRIM, (48, 32)), (M.TRANSVERSE | M.TRIM, (32, 48)),
                       (M.NONE | M.TRIM, (50, 35))):
        for quality in (None, 30):
            _check_plan(f, samp, code, quality, size)
    f = api.frame_layout(15, 40, 3, [2, 1, 1], [2, 1, 1], tabs)
    _check_plan(f, samp, M.FLIP_H | M.TRIM, None, None)  # (nothing left)
    _check_plan(f, samp, M.FLIP_V | M.TRIM, None, (15, 32))
    g = api.frame_layout(13, 9, 1, [1], [1], tabs, ycbcr=0)
    _check_plan(g, [(1, 1)], M.FLIP_H | M.TRIM, None, (8, 9))
    _check_plan(g, [(1, 1)], M.FLIP_H, None, None)
    _check_plan(g, [(1, 1)], M.ROT_180 | M.TRIM, 50, (8, 8))
    # a one-component output is 1 x 1 whatever the header said: its MCU is one block
    g.hsamp[0], g.vsamp[0] = 2, 2
    _check_plan(g, [(2, 2)], M.FLIP_H | M.TRIM, None, (8, 9))


def test_plan_refusals_are_unchanged_under_a_transform():
    def header(name):
        d = api.Decoder(None)
        try:
            return d.read_header(golden_jpeg(name))
        finally:
            d.close()

    def copy(f):
        g = api.MijpegInfo()
        C.memmove(C.byref(g), C.byref(f), C.sizeof(api.MijpegInfo))
        return g

    xt, cmyk, tall = (header(n) for n in ("xt_64x48_444", "pil_90x60_cmyk", "ref_64x64_2x4"))
    wide, zero, big = copy(tall), copy(tall), _info(_picture("420"))
    wide.coef_wide = 1
    zero.quant[0][10] = 0
    big.quant[1][63] = 256  # (a kept 8-bit picture with an entry no baseline DQT holds)
    for code in list(range(8)) + [M.ROT_90 | M.TRIM]:
        for quality in (api.TRANSCODE_KEEP, 50):
            for f in (xt, cmyk, wide, zero):  # (also where the geometry would refuse as well: the existing refusal comes first)
                rc, out, ri, kept = api.transcode_plan_transformed(f, quality, -1, code)
                assert rc == api.ERR_NOT_IMPLEMENTED == api.transcode_plan(f, quality)[0] and not bytes(out).strip(b"\0") and ri == 0 and not kept
        assert api.transcode_plan_transformed(big, api.TRANSCODE_KEEP, -1, code)[0] == api.ERR_NOT_IMPLEMENTED
        assert api.transcode_plan_transformed(big, 50, -1, code)[0] == 0
        rc, out, ri, kept = api.transcode_plan_transformed(tall, api.TRANSCODE_SKIP, 3, code)
        assert rc == 0 and not bytes(out).strip(b"\0") and ri == 0 and not kept
        for quality, interval in ((101, 0), (-2, 0), (50, 65536), (50, -2)):
            assert api.transcode_plan_transformed(tall, quality, interval, code)[0] == api.ERR_INVALID_PARAMETER
    for code in (8, -1, 9 | M.TRIM, 0x200, 0x101 + 0x100):
        rc, out, ri, kept = api.transcode_plan_transformed(tall, 50, -1, code)
        assert rc == api.ERR_INVALID_PARAMETER and not bytes(out).strip(b"\0"), code
    L = api.lib()
    spec, out, r, k = api.MijpegTranscodeSpec(0, -1), api.MijpegInfo(), C.c_int32(), C.c_int32()
    assert L.mijpeg_transcode_plan_transformed(None, C.byref(spec), 1, C.byref(out), C.byref(r), C.byref(k)) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_transcode_plan_transformed(C.byref(tall), C.byref(spec), 1, None, C.byref(r), C.byref(k)) == api.ERR_INVALID_PARAMETER


def test_list_call_checks_its_transforms_before_any_device():
    L = api.lib()
    d = api.Decoder(None)
    try:
        ptrs, sizes, status = (C.c_void_p * 2)(), (C.c_size_t * 2)(), (C.c_int32 * 2)()
        codes = (C.c_int32 * 2)(M.ROT_90, M.FLIP_H | M.TRIM)
        fn = L.mijpeg_transcode_ragged_transformed_device
        assert fn(d._h, None, codes, 0, 0, ptrs, sizes, status) == api.ERR_NOT_AVAILABLE == fn(d._h, None, None, 0, 0, ptrs, sizes, status)
        assert fn(d._h, None, codes, 0, 1, ptrs, sizes, status) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, None, codes, 0, 0, None, sizes, status) == api.ERR_INVALID_PARAMETER
        assert fn(None, None, codes, 0, 0, ptrs, sizes, status) == api.ERR_INVALID_PARAMETER
        assert d.transcode_transform_stats() == dict(transformed=0, trimmed=0, geometry_refusals=0, transform_launches=0)
        with pytest.raises(ValueError):
            d.transcode_ragged_device(None, False, [M.ROT_90])  # (no decoded batch: no transform is one too many)
    finally:
        d.close()
    data = golden_jpeg("pil_9x9_420")
    for kw in (dict(transform="rot45"), dict(transform=["rot90"]), dict(transform=["rot90", "exif", None]), dict(transform=[5, 5])):
        with pytest.raises(ValueError):
            batch.transcode_mixed([data, data], device=None, **kw)
    assert batch.transcode_mixed([data, data], rank=2, world=3, device=None, transform="exif", trim=True) == [None, None]


def test_exports_and_struct_sizes(tmp_path):
    L = api.lib()
    for name in ("mijpeg_transcode_ragged_transformed_device", "mijpeg_transcode_plan_transformed", "mijpeg_transform_blocks", "mijpeg_transcode_transform_stats_get"):
        assert hasattr(L, name), name
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mijpeg.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d %d %d\\n", sizeof(mijpeg_transcode_transform_stats), '
                   'offsetof(mijpeg_transcode_transform_stats, transform_launches), sizeof(mijpeg_transcode_ragged_stats), sizeof(mijpeg_transcode_spec), '
                   'MIJPEG_TRANSFORM_FLIP_H, MIJPEG_TRANSFORM_TRANSVERSE, MIJPEG_TRANSFORM_ROT_270, MIJPEG_TRANSFORM_TRIM); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(C.sizeof(api.MijpegTranscodeTransformStats)), str(api.MijpegTranscodeTransformStats.transform_launches.offset), "48", "8", str(api.TRANSFORM_FLIP_H),
                   str(api.TRANSFORM_TRANSVERSE), str(api.TRANSFORM_ROT_270), str(api.TRANSFORM_TRIM)] == ["16", "12", "48", "8", "1", "4", "7", "256"], out
    assert [getattr(api, "TRANSFORM_" + n.upper().replace("ROT", "ROT_")) for n in M.NAMES] == list(range(8))


# ------------------------------------------------------------------------------------------------ EXIF
def _app1(orientation, order, entries_before=1, value_type=3, count=1, ifd_at=8):
    e = "<" if order == "II" else ">"
    ifd = struct.pack(e + "H", entries_before + 1)
    for k in range(entries_before):
        ifd += struct.pack(e + "HHII", 0x010F + k, 2, 1, 0)
    ifd += struct.pack(e + "HHIHH", 0x0112, value_type, count, orientation, 0) + struct.pack(e + "I", 0)
    tiff = order.encode() + struct.pack(e + "HI", 42, ifd_at) + b"\0" * (ifd_at - 8) + ifd
    body = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


def _with_segments(data, *segments):
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"".join(segments) + data[2:]


def test_exif_orientation():
    data = golden_jpeg("pil_9x9_420")
    com = b"\xff\xfe" + struct.pack(">H", 7) + b"hello"
    assert batch.exif_orientation(data) == 1  # (no APP1)
    for order in ("II", "MM"):
        for value in range(1, 9):
            assert batch.exif_orientation(_with_segments(data, _app1(value, order))) == value, (order, value)
            assert batch.exif_orientation(_with_segments(data, com, _app1(value, order, entries_before=3, ifd_at=12))) == value
        for value in (0, 9, 0x0600, 65535):
            assert batch.exif_orientation(_with_segments(data, _app1(value, order))) == 1
        assert batch.exif_orientation(_with_segments(data, _app1(6, order, value_type=4))) == 1  # (not a SHORT)
        assert batch.exif_orientation(_with_segments(data, _app1(6, order, count=2))) == 1
        whole = _app1(6, order)
        for cut in range(5, len(whole) - 4):  # a truncated IFD: the segment ends before the entry does (its last 4 bytes: the next IFD)
            seg = b"\xff\xe1" + struct.pack(">H", cut - 2) + whole[4:cut]
            assert batch.exif_orientation(_with_segments(data, seg)) == 1, (order, cut)
        e = "<" if order == "II" else ">"
        far = b"Exif\0\0" + order.encode() + struct.pack(e + "HI", 42, 4000)  # an offset past the segment
        assert batch.exif_orientation(_with_segments(data, b"\xff\xe1" + struct.pack(">H", len(far) + 2) + far)) == 1
        assert batch.exif_orientation(_with_segments(data, _app1(6, order).replace(b"Exif", b"Exxf"))) == 1
    # garbage never raises
    rng = np.random.default_rng(4352)
    for n in (0, 1, 2, 3, 4, 7, 64, 500):
        for head in (b"", b"\xff\xd8", b"\xff\xd8\xff\xe1", b"\xff\xd8\xff\xe1\x00\x40Exif\0\0II*\0\x08\0\0\0", b"\xff\xd8\xff\xe1\x00\x40Exif\0\0MM\0*\0\0\0\x08\xff\xff"):
            assert batch.exif_orientation(head + rng.integers(0, 256, n, dtype=np.uint8).tobytes()) in range(1, 9)
    assert batch.exif_orientation(None) == 1 and batch.exif_orientation(b"\xff\xd8\xff\xe1\xff\xff") == 1 and batch.exif_orientation(memoryview(data)) == 1


# ------------------------------------------------------------------------------------------------ the program under the sanitizers
def _run_under_sanitizers(tmp_path, name, *more_sources):
    """tests/cxx/<name>.cpp (and library sources that need no device) as a program of its own under AddressSanitizer and UBSan."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"  # (ROCm's host clang++: a plain host compile, no device code)
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "libjpeg_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include", "-I", csrc,
                    os.path.join(ROOT, "tests", "cxx", name + ".cpp"), *[os.path.join(csrc, s) for s in more_sources], "-pthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])


def test_transform_tables_under_sanitizers(tmp_path):
    """tests/cxx/transform_tables.cpp, a program of its own around transform.hpp, encode_list.hpp and encoder.cpp: lists of transformed
    and untransformed pictures through the real plan, pass layout and fill into heap buffers of exactly the arenas' sizes, both work
    lists walked lane by lane as the two kernels address them over sources of exactly their frames' sizes, and the layout of a pass
    without transforms against the one the old signatures give -- under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "transform_tables", "encoder.cpp")


# ------------------------------------------------------------------------------------------------ the code object
@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_transform_kernel_has_no_scratch_and_spills_nothing():
    meta = _kernel_metadata(LIB)
    mine = {name: k for name, k in meta.items() if "transform_list_kernel" in name}
    assert len(mine) == 1, sorted(mine)
    (name, k), = mine.items()
    assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
    assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
    assert int(k["group_segment_fixed_size"]) == 32 * 40 * 4 and int(k["max_flat_workgroup_size"]) == 256  # (a padded 8 x 8 exchange per block)
    assert int(k["vgpr_count"]) <= 64, f"{name}: {k['vgpr_count']} VGPRs, below eight waves a SIMD"

"""The ragged transcode's device-free half, without a device: the numpy model of the rule (tests/requant_model.py) against
exact rationals, the host twin of the kernel (mijpeg_requantize) against the model at tolerance 0, the plan of a picture
(mijpeg_transcode_plan) against the frame and tables the encoder calls write, the argument checks of the list call, the plan, descriptors,
work list and pass layout under the sanitizers as a program of its own, and the kernel's figures in the built code object."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import requant_model as M
from conftest import ROOT, golden_jpeg
from libjpeg_amd import api
from test_ragged_batch import LIB, READELF, _kernel_metadata

TABLE_ENTRIES = [1, 2, 3, 255, 256, 32767, 65535]
SOURCE_ENTRIES = [1, 255, 65535]
COEFFICIENTS = [1, -1, 1023, -1023, -1024, 16383, -16383, -16384, 32767, -32767, -32768]


def _exact(c, a, b):
    """The rule in rationals: to nearest, halves away from zero."""
    v = Fraction(c * a, b)
    q = int(abs(v) + Fraction(1, 2))  # (floor of |v| + 1/2)
    return q if v >= 0 else -q


def _header(name):
    d = api.Decoder(None)
    try:
        return d.read_header(golden_jpeg(name))
    finally:
        d.close()


def _decoded(name):
    """-> (info, planes) of a golden from the host decoder"""
    d = api.Decoder(None)
    try:
        f = d.read(golden_jpeg(name))
        return f, [d.coefficients(c).copy() for c in range(f.components)]
    finally:
        d.close()


def _copy(f):
    g = api.MijpegInfo()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(api.MijpegInfo))
    return g


# ------------------------------------------------------------------------------------------------ the rule
def test_model_against_exact_rationals():
    rng = np.random.default_rng(4301)
    triples = [(int(c), int(a), int(b)) for c, a, b in zip(rng.integers(-32768, 32768, 3000), rng.integers(1, 65536, 3000), rng.integers(1, 65536, 3000))]
    triples += [(c, a, b) for c in COEFFICIENTS for a in SOURCE_ENTRIES for b in TABLE_ENTRIES]
    triples += [(s * (k * b + b // 2 + d), 1, b) for b in (2, 4, 16, 256, 3, 255) for k in range(4) for d in (-1, 0, 1) for s in (1, -1)]
    c, a, b = (np.array(x, np.int64) for x in zip(*triples))
    got = M.requant(c, a, b)
    assert [int(x) for x in got] == [_exact(*t) for t in triples]
    assert np.array_equal(M.requant(c, a, a), c)  # the identity


def _twin(c, a, b, precision):
    """coefficients c (any shape) at EVERY position of a block under uniform tables a, b -> mijpeg_requantize's values and count"""
    blocks = np.repeat(np.asarray(c, np.int16).reshape(-1, 1), 64, axis=1)
    return api.requantize(blocks, np.full(64, a), np.full(64, b), precision)


def test_host_twin_equals_the_model():
    for precision in (8, 12):
        # the edges: every coefficient against every pair of entries, at the DC position and at the AC positions
        for a in SOURCE_ENTRIES:
            for b in TABLE_ENTRIES + [a]:
                got, clamped = _twin(COEFFICIENTS, a, b, precision)
                want, n = M.requant_blocks(np.repeat(np.array(COEFFICIENTS).reshape(-1, 1), 64, axis=1), np.full(64, a), np.full(64, b), precision)
                assert np.array_equal(got, want) and clamped == n, (precision, a, b)
                if b == a:  # the identity holds wherever the value is inside the range
                    dc_min, dc_max, ac_max = M.coding_range(precision)
                    inside = [c for c in COEFFICIENTS if -ac_max <= c <= ac_max]
                    assert np.array_equal(_twin(inside, a, a, precision)[0][:, 1], np.array(inside, np.int16))
        # exact halves of both signs at even b, one below and above them; odd b
        for b in (2, 4, 16, 256, 3, 5, 255):
            c = [s * (k * b + b // 2 + d) for k in range(5) for d in (-1, 0, 1) for s in (1, -1)]
            got, clamped = _twin(c, 1, b, precision)
            assert np.array_equal(got[:, 5], M.requant(c, 1, b).astype(np.int16)) and clamped == 0, (precision, b)
            if b % 2 == 0:
                assert _twin([b // 2, -(b // 2)], 1, b, precision)[0][:, 7].tolist() == [1, -1]  # away from zero
        # seeded noise under random tables, whole blocks
        rng = np.random.default_rng(4302 + precision)
        blocks = rng.integers(-32768, 32768, (500, 64)).astype(np.int16)
        qa, qb = rng.integers(1, 65536, 64), rng.integers(1, 65536, 64)
        got, clamped = api.requantize(blocks, qa, qb, precision)
        want, n = M.requant_blocks(blocks, qa, qb, precision)
        assert np.array_equal(got, want) and clamped == n and n > 0


def test_host_twin_clamps_and_counts_at_the_range_edges():
    for precision in (8, 12):
        dc_min, dc_max, ac_max = M.coding_range(precision)
        assert (dc_min, dc_max, ac_max) == ((-1024, 1023, 1023) if precision == 8 else (-16384, 16383, 16383))
        one = np.ones(64, int)
        for value, at, want, count in ((dc_max, 0, dc_max, 0), (dc_max + 1, 0, dc_max, 1), (dc_min, 0, dc_min, 0), (dc_min - 1, 0, dc_min, 1),
                                       (ac_max, 1, ac_max, 0), (ac_max + 1, 1, ac_max, 1), (-ac_max, 63, -ac_max, 0), (-ac_max - 1, 63, -ac_max, 1)):
            block = np.zeros((1, 64), np.int16)
            block[0, at] = value
            got, clamped = api.requantize(block, one, one, precision)
            assert got[0, at] == want and clamped == count and not np.delete(got[0], at).any(), (precision, value, at)
            assert M.requant_blocks(block, one, one, precision)[1] == count
        # the issue's refusal: an AC value of 1000 under an entry of 16 at quality 100 (entry 1) is 16000
        block = np.zeros((1, 64), np.int16)
        block[0, 9] = 1000
        got, clamped = api.requantize(block, np.full(64, 16), one, precision)
        assert (got[0, 9], clamped) == ((1023, 1) if precision == 8 else (16000, 0))
    L = api.lib()
    buf = np.zeros(64, np.int16)
    q, zero = np.ones(64, np.uint16), np.zeros(64, np.uint16)
    assert L.mijpeg_requantize(None, buf.ctypes.data, 1, q.ctypes.data, q.ctypes.data, 8) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_requantize(buf.ctypes.data, buf.ctypes.data, 1, q.ctypes.data, zero.ctypes.data, 8) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_requantize(buf.ctypes.data, buf.ctypes.data, 1, q.ctypes.data, q.ctypes.data, 10) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_requantize(buf.ctypes.data, buf.ctypes.data, 1, q.ctypes.data, q.ctypes.data, 8) == 0  # (in place)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_at_a_quality_is_the_encoders_frame():
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    for name in ("pilprog_75x45_420", "ref_64x64_2x4", "ref_23x50_lumasub", "pil_70x40_gray", "ref_97x61_420_dnl", "p12_120x90_420_dri3"):
        f = _header(name)
        for quality in (1, 30, 75, 100):
            rc, out, ri, kept = M.plan(f, quality)
            assert rc == 0 and not kept and ri == f.restart_interval, name
            nc = f.components
            hs, vs = ([f.hsamp[c] for c in range(nc)], [f.vsamp[c] for c in range(nc)]) if nc == 3 else ([1], [1])
            luma, chroma = (C.c_uint16 * 64)(), (C.c_uint16 * 64)()
            L.mijpeg_quality_tables(quality, luma, chroma)
            if f.precision == 8:  # (mijpeg_quality_tables speaks of 8-bit frames: entries to 255)
                assert list(out.quant[0]) == list(luma) and list(out.quant[1]) == list(chroma), (name, quality)
            want = api.frame_layout(f.width, f.height, nc, hs, vs, [list(out.quant[0]), list(out.quant[1])], quant_index=[0] * nc, ycbcr=int(nc == 3), precision=f.precision)
            assert bytes(out) == bytes(want), (name, quality)
            assert not out.dnl and not out.progressive and out.precision == f.precision
        assert M.plan(f, 50, 0)[2] == 0 and M.plan(f, 50, 65535)[2] == 65535 and M.plan(f, None, 7)[2] == 7


def test_plan_kept_keeps_tables_and_their_indices():
    for name in ("pilprog_75x45_420", "ref_64x64_2x4", "pil_131x77_422", "enc12/420_64x40_q2"):
        f = _header(name)
        rc, out, ri, kept = M.plan(f)
        assert rc == 0 and kept and ri == f.restart_interval
        assert [out.quant_index[c] for c in range(3)] == [f.quant_index[c] for c in range(3)]
        assert all(list(out.quant[t]) == list(f.quant[t]) for t in range(4))
        assert (out.width, out.height, out.precision, list(out.hsamp), list(out.vsamp)) == (f.width, f.height, f.precision, list(f.hsamp), list(f.vsamp))
        assert bytes(out) == bytes(api.frame_layout(f.width, f.height, 3, list(f.hsamp), list(f.vsamp), [list(f.quant[t]) for t in range(4)],
                                                    quant_index=list(f.quant_index), precision=f.precision))
    # a one-component output is 1 x 1 whatever the header said: its scan is not interleaved
    g = _copy(_header("pil_70x40_gray"))
    g.hsamp[0], g.vsamp[0], g.blocks_w[0], g.blocks_h[0] = 2, 2, 10, 6
    out = M.plan(g)[1]
    assert (out.hsamp[0], out.vsamp[0], out.blocks_w[0], out.blocks_h[0], out.mcus_x, out.mcus_y) == (1, 1, 9, 5, 9, 5)


def test_plan_refusals_and_spec_checks():
    xt, cmyk, prog, tall = (_header(n) for n in ("xt_64x48_444", "pil_90x60_cmyk", "pilprog_75x45_420", "ref_64x64_2x4"))
    assert xt.xt and cmyk.components == 4 and prog.progressive
    for quality in (None, 50):
        assert M.plan(xt, quality)[0] == api.ERR_NOT_IMPLEMENTED and M.plan(cmyk, quality)[0] == api.ERR_NOT_IMPLEMENTED
        two = _copy(prog)
        two.components = 2
        wide = _copy(tall)
        wide.coef_wide = 1
        zero = _copy(tall)
        zero.quant[0][10] = 0
        for f in (two, wide, zero):
            rc, out, ri, kept = M.plan(f, quality)
            assert rc == api.ERR_NOT_IMPLEMENTED and not bytes(out).strip(b"\0") and ri == 0 and not kept
    # a kept 8-bit picture with an entry no baseline DQT holds; at a quality, and at 12 bits, it is served
    big = _copy(prog)
    big.quant[1][63] = 256
    assert M.plan(big)[0] == api.ERR_NOT_IMPLEMENTED and M.plan(big, 50)[0] == 0
    big.quant[1][63] = 255
    assert M.plan(big)[0] == 0
    p12 = _copy(_header("enc12/420_64x40_q2"))
    assert max(p12.quant[0]) > 255 and M.plan(p12)[0] == 0
    # SKIP is no refusal; a spec outside its ranges is the caller's error, with the outputs cleared
    rc, out, ri, kept = api.transcode_plan(prog, api.TRANSCODE_SKIP, 3)
    assert rc == 0 and not bytes(out).strip(b"\0") and ri == 0 and not kept
    for quality, ri in ((101, 0), (-2, 0), (50, 65536), (50, -2)):
        rc, out, r, kept = api.transcode_plan(prog, quality, ri)
        assert rc == api.ERR_INVALID_PARAMETER and not bytes(out).strip(b"\0") and r == 0 and not kept
    L = api.lib()
    spec, out, r, k = api.MijpegTranscodeSpec(0, -1), api.MijpegInfo(), C.c_int32(), C.c_int32()
    assert L.mijpeg_transcode_plan(None, C.byref(spec), C.byref(out), C.byref(r), C.byref(k)) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_transcode_plan(C.byref(prog), None, C.byref(out), C.byref(r), C.byref(k)) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_transcode_plan(C.byref(prog), C.byref(spec), None, C.byref(r), C.byref(k)) == api.ERR_INVALID_PARAMETER


def test_goldens_are_inside_the_coding_range_at_every_quality(oracle):
    """The refusals of the device tests come from crafted inputs alone: the goldens they recode are out of range nowhere."""
    for name in ("pil_131x77_422", "pil_80x48_444", "pil_70x40_gray", "pil_9x9_420", "pil_1x1_444", "p12_120x90_420_dri3", "p12_64x48_444", "pilprog_75x45_420",
                 "refprog_64x64_444_dri5", "ref_97x61_440", "ref_97x61_411", "ref_64x64_2x4", "ref_23x50_lumasub", "ref_97x61_420_dnl", "ref_120x88_sof1_420",
                 "pil_200x120_420_dri8", "ref_33x17_420_dri1", "ref_100x9_422", "ref_64x40_q2", "ref_64x40_q100", "enc12/422_100x9"):
        f, planes = _decoded(name)
        for quality in (None, 30, 75, 95, 100):
            rc, out, _, _ = M.plan(f, quality)
            assert rc == 0 and M.transcode_planes(f, planes, out)[1] == 0, (name, quality)
    # enc12/420_272x144_z4, which the device tests recode with its own tables, is inside the range as it is.  Its black blocks are
    # not at quality 100: their DC of -3277 under an entry of 5 is -16385, one below what a 12-bit frame codes (the forward rounding
    # of -16384 / 5, taken back at entry 1) -- 24 values, a refusal by range that no crafting made and the rule's to give
    f, planes = _decoded("enc12/420_272x144_z4")
    assert M.transcode_planes(f, planes, M.plan(f)[1])[1] == 0 and M.transcode_planes(f, planes, M.plan(f, 100)[1])[1] == 24


# ------------------------------------------------------------------------------------------------ the list call's arguments
def test_list_call_checks_its_arguments_before_any_device():
    L = api.lib()
    d = api.Decoder(None)
    try:
        ptrs, sizes, status = (C.c_void_p * 2)(), (C.c_size_t * 2)(), (C.c_int32 * 2)()
        specs = (api.MijpegTranscodeSpec * 2)()
        fn = L.mijpeg_transcode_ragged_device
        assert fn(d._h, specs, 0, 0, ptrs, sizes, status) == api.ERR_NOT_AVAILABLE == fn(d._h, None, 1, 0, ptrs, sizes, status)
        msg = C.c_char_p()
        assert L.mijpeg_last_error(d._h, C.byref(msg)) == api.ERR_NOT_AVAILABLE and b"device" in msg.value
        assert fn(d._h, specs, 0, 0, None, sizes, status) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, specs, 0, 0, ptrs, None, status) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, specs, 0, 0, ptrs, sizes, None) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, specs, 0, 1, ptrs, sizes, status) == api.ERR_INVALID_PARAMETER
        assert fn(None, specs, 0, 0, ptrs, sizes, status) == api.ERR_INVALID_PARAMETER
        with pytest.raises(api.MijpegError) as e:
            d.transcode_ragged_device()
        assert e.value.code == api.ERR_NOT_AVAILABLE
        assert d.transcode_ragged_stats() == dict(pictures=0, served=0, kept=0, refused=0, children=0, passes=0, requant_launches=0, coder_launches=0,
                                                  host_syncs=0, child_uploads=0, bytes_downloaded=0)
    finally:
        d.close()


def test_exports_and_struct_sizes(tmp_path):
    L = api.lib()
    for name in ("mijpeg_transcode_ragged_device", "mijpeg_transcode_ragged_stats_get", "mijpeg_transcode_plan", "mijpeg_requantize"):
        assert hasattr(L, name), name
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mijpeg.h"\nint main(void) { printf("%zu %zu %zu %d %d\\n", sizeof(mijpeg_transcode_ragged_stats), '
                   'offsetof(mijpeg_transcode_ragged_stats, bytes_downloaded), sizeof(mijpeg_transcode_spec), MIJPEG_TRANSCODE_KEEP, MIJPEG_TRANSCODE_SKIP); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(C.sizeof(api.MijpegTranscodeRaggedStats)), str(api.MijpegTranscodeRaggedStats.bytes_downloaded.offset), str(C.sizeof(api.MijpegTranscodeSpec)),
                   str(api.TRANSCODE_KEEP), str(api.TRANSCODE_SKIP)] == ["48", "40", "8", "0", "-1"], out


def test_transcode_mixed_checks_its_arguments_without_a_device():
    from libjpeg_amd import batch

    data = golden_jpeg("pil_9x9_420")
    for kw in (dict(quality=[50]), dict(quality=101), dict(quality=0), dict(quality=[50, 200]), dict(restart_mcus=[1, 2, 3]), dict(restart_mcus=65536), dict(restart_mcus=-1)):
        with pytest.raises(ValueError):
            batch.transcode_mixed([data, data], device=None, **kw)
    assert batch.transcode_mixed([], device=None) == []
    assert batch.transcode_mixed([data, data], rank=2, world=3, device=None) == [None, None]  # (a rank without pictures touches nothing)


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


def test_transcode_tables_under_sanitizers(tmp_path):
    """tests/cxx/transcode_tables.cpp, a program of its own around requant.hpp, encode_list.hpp and encoder.cpp: the rule against
    64-bit arithmetic; plan, descriptors, work list and pass layout for lists with group members and children, both precisions, with
    and without own tables, cut into passes, into heap buffers of exactly the arenas' sizes, the work list walked as the kernel
    addresses it -- under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "transcode_tables", "encoder.cpp")


# ------------------------------------------------------------------------------------------------ the code object
@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_requant_kernel_has_no_scratch_and_spills_nothing():
    meta = _kernel_metadata(LIB)
    mine = {name: k for name, k in meta.items() if "requant_list_kernel" in name}
    assert len(mine) == 1, sorted(mine)
    (name, k), = mine.items()
    assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
    assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
    assert int(k["group_segment_fixed_size"]) == 0 and int(k["max_flat_workgroup_size"]) == 256
    assert int(k["vgpr_count"]) <= 64, f"{name}: {k['vgpr_count']} VGPRs, below eight waves a SIMD"

"""12-bit encoder direction, the part that needs no device: the host entropy coder on crafted precision-12 coefficient planes
(extended sequential, SOF1 / P = 12, DC categories to 15 and AC categories to 14), the argument checks of the new entry points, the
numpy restatement of the 12-bit colour transformation and downsampling (tests/enc12_util.py) against every golden the reference
encoder wrote (tests/golden/enc12), and a guard on the machine code of the forward kernels and the device coder."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import enc12_util as U
from libjpeg_amd import api
from test_isa_guard import LIB
from test_ragged_batch import READELF, _kernel_metadata

ERR_OVERFLOW_PARAMETER = -1028
ERR_OPERATION_UNIMPLEMENTED = -1034


def _grey12(blocks_x: int, blocks_y: int):
    return api.frame_layout(blocks_x * 8, blocks_y * 8, 1, (1,), (1,), [np.ones(64, int)], ycbcr=0, precision=12)


def _crafted_planes():
    """(info, int16 coefficients): 32 blocks whose DC differences run through the smallest and the largest value of every category
    0..15 and whose AC coefficients through those of every category 1..14, both signs, with zero runs beyond 15 in between."""
    info = _grey12(8, 4)
    coef = np.zeros((32, 64), np.int16)
    dc = [0, 0]  # (difference 0: category 0)
    for k in range(1, 16):
        for d in (1 << (k - 1), (1 << k) - 1):
            dc.append(dc[-1] - d if dc[-1] > 0 else dc[-1] + d)
    assert len(dc) == 32 and max(abs(v) for v in dc) <= 32767
    coef[:, 0] = dc
    rng = np.random.default_rng(12)
    mags = [m for k in range(1, 15) for m in (1 << (k - 1), (1 << k) - 1)]
    for b in range(32):
        pos = np.sort(rng.choice(np.arange(1, 64), size=4 if b % 3 else 2, replace=False))  # (two of 63: runs beyond 15)
        for j, p in enumerate(pos):
            m = mags[(b * 4 + j) % len(mags)]
            coef[b, p] = m if (b + j) & 1 else -m
    assert int(np.abs(coef[:, 1:]).max()) == 16383 and {int(abs(v)).bit_length() for v in coef[:, 1:].reshape(-1) if v} == set(range(1, 15))
    diffs = np.diff(np.concatenate([[0], coef[:, 0].astype(int)]))
    assert {int(abs(v)).bit_length() for v in diffs} == set(range(0, 16))
    return info, coef


def _sof(data: bytes):
    """(marker, precision) of the frame header."""
    i = 2
    while i < len(data):
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m, data[i + 4]
        i += 2 + n
    raise AssertionError("no frame header")


@pytest.mark.parametrize("ri", [0, 1, 5])
def test_host_coder_codes_every_12_bit_category(oracle, ri):
    info, coef = _crafted_planes()
    data = api.encode_coefficients(info, coef, ri, optimize=False)  # (optimize is ignored at precision 12: no Annex K codes up there)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    assert _sof(data) == (0xC1, 12)
    assert api.encode_coefficients(info, coef, ri, optimize=True) == data
    for th in (1, 3):
        assert api.encode_coefficients(info, coef, ri, threads=th) == data
    oi, back = oracle.decode_coefficients(data)
    assert (oi.width, oi.height, oi.precision, oi.restart_interval) == (64, 32, 12, ri)
    assert np.array_equal(back[0].reshape(32, 64), coef)
    d = api.Decoder(None)
    f = d.read(data, threads=2)
    assert f.precision == 12
    assert np.array_equal(np.asarray(d.coefficients(0)).reshape(32, 64), coef)
    d.close()
    if oracle.have_reference():
        px, err = oracle.reference_decode_status(data)
        assert err == 0 and px.shape[:2] == (32, 64)


def test_one_value_beyond_either_limit_is_refused():
    info, coef = _crafted_planes()
    for opt in (False, True):
        bad = coef.copy()
        bad[3, 9] = 16384  # AC category 15
        with pytest.raises(api.MijpegError) as e:
            api.encode_coefficients(info, bad, 0, opt)
        assert e.value.code == ERR_OVERFLOW_PARAMETER
        bad = coef.copy()
        bad[4, 0], bad[5, 0] = -20000, 20000  # DC difference of category 16
        with pytest.raises(api.MijpegError) as e:
            api.encode_coefficients(info, bad, 0, opt)
        assert e.value.code == ERR_OVERFLOW_PARAMETER
    ok = coef.copy()
    ok[3, 9] = -16383
    assert _sof(api.encode_coefficients(info, ok)) == (0xC1, 12)


def test_8_bit_frames_keep_their_limits_and_their_header():
    """What test_encoder.py::test_coefficients_outside_the_8_bit_range_are_refused pins, beside a precision-12 frame of the same planes."""
    info8 = api.frame_layout(16, 16, 1, (1,), (1,), [np.ones(64, int)], ycbcr=0)
    info12 = _grey12(2, 2)
    coef = np.zeros(int(info8.coef_count), np.int16)
    coef[5] = 1024
    with pytest.raises(api.MijpegError) as e:
        api.encode_coefficients(info8, coef)
    assert e.value.code == ERR_OVERFLOW_PARAMETER
    assert _sof(api.encode_coefficients(info12, coef)) == (0xC1, 12)
    coef[5] = 1023
    coef[0] = 2047
    assert _sof(api.encode_coefficients(info8, coef)) == (0xC0, 8)
    coef[0] = 2048
    with pytest.raises(api.MijpegError):
        api.encode_coefficients(info8, coef, optimize=True)
    info8.precision = 16
    with pytest.raises(api.MijpegError) as e:
        api.encode_coefficients(info8, coef)
    assert e.value.code == ERR_OPERATION_UNIMPLEMENTED


def test_frame_layout_takes_precision_8_and_12_only():
    q = [np.ones(64, int)]
    for p in (8, 12):
        f = api.frame_layout(33, 17, 3, (2, 1, 1), (2, 1, 1), q, precision=p)
        assert (f.precision, f.sample_bytes, f.mcus_x, f.mcus_y) == (p, 2 if p == 12 else 1, 3, 2)
    for p in (9, 16, 0):
        with pytest.raises(api.MijpegError) as e:
            api.frame_layout(33, 17, 3, (2, 1, 1), (2, 1, 1), q, precision=p)
        assert e.value.code == api.ERR_INVALID_PARAMETER


def test_encode_image16_rejects_bad_arguments_without_a_device():
    L = api.lib()
    L.mijpeg_encode_image16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    d = api.Decoder(None)
    img = np.zeros((16, 16, 3), np.uint16)
    p, n = C.c_void_p(), C.c_size_t()

    def call(handle=None, pixels=img.ctypes.data, w=16, h=16, nc=3, stride=96, precision=12, flags=0, out=C.byref(p)):
        return L.mijpeg_encode_image16(d._h if handle is None else handle, pixels, w, h, nc, stride, precision, 85, None, None, 0, flags, out, C.byref(n))

    for kw in ({"precision": 8}, {"precision": 16}, {"precision": 0}, {"stride": 95}, {"stride": 94}, {"pixels": None}, {"nc": 2}, {"flags": 2},
               {"pixels": img.ctypes.data + 1}, {"out": None}):
        assert call(**kw) == api.ERR_INVALID_PARAMETER, kw
    assert call() == api.ERR_NOT_AVAILABLE  # everything in order but the device
    with pytest.raises(api.MijpegError) as e:
        d.encode(img, 85, "420")  # uint16 input goes to the same entry point
    assert e.value.code == api.ERR_NOT_AVAILABLE
    d.close()


@pytest.mark.parametrize("key", sorted(U.CASES))
def test_restatement_gives_the_coefficients_of_every_golden(oracle, key):
    """enc12_util.forward12 (numpy colour transformation and downsampling, the oracle's block transform) against the coefficients in
    the stream the reference encoder wrote -- on the blocks that cover samples; the MCU padding blocks are the encoder's own."""
    w, h, layout, _, _, q, extra = U.CASES[key]
    data = U.golden_stream(key)
    assert _sof(data) == (0xC1, 12)
    assert U.manifest()[key]["switches"] == U.case_args(key)
    info, planes = U.golden_coefficients(key)
    assert (info.width, info.height, info.restart_interval) == (w, h, U.case_restart(key))
    assert list(info.tq[:info.ncomp]) == [0] * info.ncomp
    hs, vs = U.LAYOUTS[layout][0]
    img = U.case_image(key)
    mine = U.forward12(img, hs, vs, [U.oracle_quant(info, c) for c in range(info.ncomp)], ycbcr="-c" not in extra)
    for c in range(info.ncomp):
        nbx, nby = U.covered_blocks(w, h, info.subx[c], info.suby[c])
        assert mine[c].shape == planes[c].shape
        assert np.array_equal(mine[c][:nby, :nbx], planes[c][:nby, :nbx]), (key, c)


def test_goldens_reach_the_widest_categories():
    _, planes = U.golden_coefficients("444_64x40_q100_pixel_checker")
    assert int(np.abs(planes[0][..., 1:]).max()).bit_length() == 14
    _, planes = U.golden_coefficients("444_64x40_q100_block_checker")
    assert int(np.abs(np.diff(planes[0][..., 0].reshape(-1))).max()).bit_length() == 15
    assert max(U.golden_coefficients("420_64x40_q2")[0].quant[0]) > 255  # 16-bit DQT entries


# VGPRs of the forward kernels' 8-bit instantiations in a build of the parent commit a6954f6 ("Split capi.cpp: reconstruction,
# ragged decode and encoder get own files"), same compiler (hipcc --offload-arch=gfx950 -O3); key: kernel, template arguments as
# mangled, without the precision this change appends.
PARENT_FORWARD_VGPRS = {
    ("fdct_blocks_kernel", (0,)): 101, ("fdct_blocks_kernel", (1,)): 90,
    ("fdct420_tile_kernel", (0,)): 197, ("fdct420_tile_kernel", (1,)): 197,
    ("fdct_interior_kernel", (1, 1, 0)): 81, ("fdct_interior_kernel", (1, 1, 1)): 82,
    ("fdct_interior_kernel", (1, 2, 0)): 134, ("fdct_interior_kernel", (1, 2, 1)): 135,
    ("fdct_interior_kernel", (2, 1, 0)): 134, ("fdct_interior_kernel", (2, 1, 1)): 134,
    ("fdct_interior_kernel", (2, 2, 0)): 256, ("fdct_interior_kernel", (2, 2, 1)): 264,
}


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_12_bit_kernels_spill_nothing_and_cost_the_8_bit_ones_nothing():
    meta = _kernel_metadata(LIB)
    pat = re.compile(r"^_ZN3mij\d+(fdct\w+_kernel)I((?:L[bi]\d+E)+)E")
    seen8, seen12 = set(), set()
    for name, k in meta.items():
        m = pat.match(name)
        if not m:
            continue
        args = tuple(int(x) for x in re.findall(r"L[bi](\d+)E", m.group(2)))
        key = (m.group(1), args[:-1])
        if args[-1] == 12:  # the precision is the last template parameter of all three
            assert not args[-2], f"{name}: there is no ragged 12-bit flavour"
            assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
            assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
            seen12.add(key)
        else:
            assert args[-1] == 8 and key in PARENT_FORWARD_VGPRS, f"instantiation the parent did not have: {name}"
            assert int(k["vgpr_count"]) == PARENT_FORWARD_VGPRS[key], f"{name}: {k['vgpr_count']} VGPRs, the parent's build had {PARENT_FORWARD_VGPRS[key]}"
            seen8.add(key)
    assert seen8 == set(PARENT_FORWARD_VGPRS)
    assert seen12 == {k for k in PARENT_FORWARD_VGPRS if not k[1][-1]}  # the uniform flavour of every family
    # the device coder has no instantiation of its own for 12 bits (its tables index 16 DC categories and 256 AC symbols, code word
    # and value bits are put separately): the kernels that code 12-bit frames are the ones that code 8-bit frames
    coder = [k for n, k in meta.items() if re.search(r"henc_\w+_kernel|scan_(apply|tile_sums)_kernel", n)]
    assert len(coder) >= 14
    for k in coder:
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0 and int(k["private_segment_fixed_size"]) == 0, k["name"]

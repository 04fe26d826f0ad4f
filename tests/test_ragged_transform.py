"""mijpeg_transcode_ragged_transformed_device on the device: the pictures of a decoded ragged batch flipped, transposed or
rotated on their way through the transcode pass.  Everything is equality at tolerance 0.  The references:

  the model        tests/transform_model.py (pinned by a float64 inverse DCT in test_ragged_transform_cpu.py) over the source's planes,
                   laid out in the output frame of mijpeg_transcode_plan_transformed
  host coder       api.encode_coefficients(output frame, model planes, restart interval, optimize, threads=1): every served stream
                   equals it byte for byte, headers included -- so transform_list_kernel equals the model and the passes' coder the host's
  oracle decoder   oracle.decode_coefficients(output) returns the model's planes on the blocks that cover samples
  numpy            the pixels of a transformed picture of DC coefficients alone are the numpy operation on the source's pixels

Crafted sources are written by the host coder (api.encode_coefficients takes any tables), the rest are committed goldens."""
import struct

import numpy as np
import pytest

import requant_model as R
import transform_model as M
from conftest import golden_jpeg
from libjpeg_amd import api, batch
from test_ragged_transcode import _check_against_oracle, _crafted_one
from test_ragged_transcode_cpu import _decoded
from test_ragged_transform_cpu import _app1, _with_segments

pytestmark = pytest.mark.gpu

SAMP = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": [(1, 1)] * 3, "grey": [(1, 1)]}
HWC_OPS = {M.NONE: lambda a: a, M.FLIP_H: lambda a: a[:, ::-1], M.FLIP_V: lambda a: a[::-1], M.TRANSPOSE: lambda a: a.transpose(1, 0, 2),
           M.TRANSVERSE: lambda a: np.rot90(a.transpose(1, 0, 2), 2), M.ROT_90: lambda a: np.rot90(a, -1), M.ROT_180: lambda a: np.rot90(a, 2),
           M.ROT_270: lambda a: np.rot90(a, 1)}
EXIF_CODES = {1: M.NONE, 2: M.FLIP_H, 3: M.ROT_180, 4: M.FLIP_V, 5: M.TRANSPOSE, 6: M.ROT_90, 7: M.TRANSVERSE, 8: M.ROT_270}


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ helpers
def _craft(rng, w, h, layout, precision=8, ri=0, fill=None, amplitude=None):
    """-> (info, planes, stream): noise inside the coding range at every position under tables without symmetry (|c| <= range // entry,
    so that no quality takes a value out of it); amplitude: a bound on |c| as well, and only a block's first 16 positions are filled"""
    samp = SAMP[layout]
    tabs = [rng.integers(1, 256, 64), rng.integers(1, 256, 64)]
    f = api.frame_layout(w, h, len(samp), [s[0] for s in samp], [s[1] for s in samp], tabs, ycbcr=int(len(samp) == 3), precision=precision)
    f.restart_interval = ri
    ac_max = R.coding_range(precision)[2]

    def noise(c):
        amp = ac_max // np.array(f.quant[f.quant_index[c]][:])
        if amplitude:
            amp = np.where(np.arange(64) < 16, np.minimum(amp, amplitude), 0)
        return rng.integers(-amp, amp + 1, (f.blocks_h[c], f.blocks_w[c], 64)).astype(np.int16)

    planes = [fill(c, f) if fill else noise(c) for c in range(f.components)]
    return f, planes, api.encode_coefficients(f, np.concatenate([p.reshape(-1) for p in planes]).astype(np.int16), ri, False, threads=1)


def _expected(f, planes, quality, code, optimize=False):
    """what the call owes for a decoded picture: (status, stream or None, output frame, model planes, restart interval)"""
    rc, out, ri, kept = api.transcode_plan_transformed(f, api.TRANSCODE_KEEP if quality is None else quality, -1, code)
    if rc:
        return rc, None, None, None, 0
    flat, beyond = M.transcode_planes(f, planes, out, code)
    if beyond:
        return api.ERR_OVERFLOW_PARAMETER, None, out, flat, ri
    return 0, api.encode_coefficients(out, flat, ri, optimize, threads=1), out, flat, ri


@pytest.fixture(scope="module")
def crafted_list():
    """[(name, planes, stream, trim)]; the single-image route's picture is a progressive golden"""
    rng = np.random.default_rng(4360)
    out = []
    for name, w, h, layout, precision, ri, trim in (("420", 48, 32, "420", 8, 0, 0), ("422", 32, 16, "422", 8, 2, 0), ("444_63_blocks", 72, 56, "444", 8, 0, 0),
                                                    ("grey", 8, 24, "grey", 8, 1, 0), ("420_trimmed", 50, 35, "420", 8, 0, M.TRIM), ("420_12bit", 32, 32, "420", 12, 3, 0)):
        f, planes, stream = _craft(rng, w, h, layout, precision, ri)
        out.append((name, planes, stream, trim))
    f, planes = _decoded("refprog_64x64_444_dri5")
    out.append(("progressive", planes, golden_jpeg("refprog_64x64_444_dri5"), 0))
    f, planes, stream = _craft(rng, 40, 24, "422")
    out.append(("untransformed", planes, stream, None))
    f, planes, stream = _craft(rng, 64, 16, "420")
    out.append(("420_last", planes, stream, 0))
    return out


# ------------------------------------------------------------------------------------------------ 1. kernel and coder
@pytest.mark.parametrize("code", range(8))
def test_kernel_is_the_model_and_the_coder_is_the_host_coder(dec, oracle, crafted_list, code):
    n = len(crafted_list)
    assert dec.decode_ragged_device([s for _, _, s, _ in crafted_list], with_12bit=True) == [0] * n
    route = [dec.ragged_route(i)[0] for i in range(n)]
    assert not route[6]  # (the progressive picture is the single-image route's)
    infos = [dec.ragged_info(i) for i in range(n)]
    codes = [M.NONE if trim is None else code | (trim if code else 0) for _, _, _, trim in crafted_list]
    for quality in (None, 75):
        for optimize in (False, True):
            got, status = dec.transcode_ragged_device([(api.TRANSCODE_KEEP if quality is None else quality, -1)] * n, optimize, codes)
            stats, tstats = dec.transcode_ragged_stats(), dec.transcode_transform_stats()
            for i, (name, planes, _, _) in enumerate(crafted_list):
                rc, want, out, flat, ri = _expected(infos[i], planes, quality, codes[i], optimize)
                what = (M.NAMES[code], name, quality, optimize)
                assert rc == 0 and status[i] == 0, (what, status[i], rc)
                assert got[i] == want, (what, len(got[i] or b""), len(want))
                if not optimize:
                    _check_against_oracle(oracle, got[i], out, flat, ri, what)
            assert (stats["served"], stats["refused"], stats["passes"]) == (n, 0, 1) and stats["children"] >= 1
            assert stats["requant_launches"] == 1 and tstats["transform_launches"] == (1 if code else 0)
            assert (tstats["transformed"], tstats["geometry_refusals"]) == ((n - 1, 0) if code else (0, 0))
            assert tstats["trimmed"] == (1 if M.BITS[code][1] or M.BITS[code][2] else 0)


# ------------------------------------------------------------------------------------------------ 2. through the product
def test_rotations_and_flips_compose_to_the_kept_transcode(dec):
    rng = np.random.default_rng(4361)
    streams = [_craft(rng, 48, 32, "420", ri=3)[2], _craft(rng, 32, 16, "422")[2], _craft(rng, 24, 40, "444", ri=1)[2], _craft(rng, 8, 24, "grey")[2],
               _craft(rng, 32, 32, "420", 12)[2]]
    kept = batch.transcode_mixed(streams, decoder=dec)
    assert all(isinstance(s, bytes) for s in kept)
    turned = streams
    for k in range(4):
        turned = batch.transcode_mixed(turned, transform="rot90", decoder=dec)
        assert all(isinstance(s, bytes) for s in turned), k
        assert (turned == kept) == (k == 3)
    flipped = batch.transcode_mixed(streams, transform="flip_h", decoder=dec)
    assert flipped != kept and batch.transcode_mixed(flipped, transform="flip_h", decoder=dec) == kept
    assert batch.transcode_mixed(batch.transcode_mixed(streams, transform="rot270", decoder=dec), transform=["rot90"] * 5, decoder=dec) == kept
    once = batch.transcode_mixed(streams, transform="rot90", decoder=dec)
    assert batch.transcode_mixed(batch.transcode_mixed(streams, transform="transpose", decoder=dec), transform="flip_h", decoder=dec) == once


# ------------------------------------------------------------------------------------------------ 3. pixels
def _dc_only(rng, w, h, layout):
    def fill(c, f):  # (DC values that stay inside the sample range under the picture's table)
        amp = 900 // f.quant[f.quant_index[c]][0]
        p = np.zeros((f.blocks_h[c], f.blocks_w[c], 64), np.int16)
        p[..., 0] = rng.integers(-amp, amp + 1, (f.blocks_h[c], f.blocks_w[c]))
        return p

    return _craft(rng, w, h, layout, fill=fill)[2]


def _pixels(dec, streams):
    out = batch.decode_mixed(streams, decoder=dec)
    assert not any(isinstance(t, api.MijpegError) for t in out), out
    return [t.cpu().numpy().reshape(t.shape[0], t.shape[1], -1) for t in out]


def test_dc_only_pictures_are_the_numpy_operation_on_the_pixels(dec):
    """(The reconstruction is constant on a block of a DC coefficient alone, so the comparison is with the source's own pixels.)"""
    rng = np.random.default_rng(4362)
    sources = [_dc_only(rng, 24, 16, "444"), _dc_only(rng, 16, 40, "grey")]
    before = _pixels(dec, sources)
    assert all(len(np.unique(p[:8, :8, 0])) == 1 for p in before) and all(len(np.unique(p[..., 0])) > 1 for p in before)
    for code in range(1, 8):
        got = _pixels(dec, batch.transcode_mixed(sources, transform=M.NAMES[code], decoder=dec))
        for g, b in zip(got, before):
            assert np.array_equal(g, HWC_OPS[code](b)), M.NAMES[code]


# ------------------------------------------------------------------------------------------------ 4. refusals serve their neighbours
def test_refusals_serve_their_neighbours(dec, oracle):
    rng = np.random.default_rng(4363)
    a, odd, b = _craft(rng, 48, 32, "420"), _craft(rng, 50, 35, "420"), _craft(rng, 16, 8, "grey")
    assert dec.decode_ragged_device([a[2], odd[2], b[2]]) == [0, 0, 0]
    infos = [dec.ragged_info(i) for i in range(3)]
    got, status = dec.transcode_ragged_device(None, False, [M.FLIP_H] * 3)
    assert status == [0, api.ERR_NOT_AVAILABLE, 0] and got[1] is None
    assert got[0] == _expected(infos[0], a[1], None, M.FLIP_H)[1] and got[2] == _expected(infos[2], b[1], None, M.FLIP_H)[1]
    st, ts = dec.transcode_ragged_stats(), dec.transcode_transform_stats()
    assert (st["served"], st["refused"]) == (2, 1) and ts == dict(transformed=2, trimmed=0, geometry_refusals=1, transform_launches=1)
    got, status = dec.transcode_ragged_device(None, False, [M.FLIP_H | M.TRIM] * 3)
    assert status == [0, 0, 0] and got[1] == _expected(infos[1], odd[1], None, M.FLIP_H | M.TRIM)[1]
    assert dec.transcode_transform_stats() == dict(transformed=3, trimmed=1, geometry_refusals=0, transform_launches=1)
    mixed = batch.transcode_mixed([a[2], odd[2], b[2]], transform=["flip_h", "rot90", None], decoder=dec)
    assert isinstance(mixed[1], api.MijpegError) and mixed[1].code == api.ERR_NOT_AVAILABLE and isinstance(mixed[0], bytes) and isinstance(mixed[2], bytes)
    assert "width of 35" in str(mixed[1]) and "16 x 16" in str(mixed[1]) and "trim=True" in str(mixed[1]), str(mixed[1])
    assert batch.transcode_mixed([odd[2]], transform="rot90", trim=True, decoder=dec)[0] == _expected(infos[1], odd[1], None, M.ROT_90 | M.TRIM)[1]
    # a value out of range after requantisation, under rot180: an AC value of 1000 under an entry of 16 is 16000 at quality 100
    f, planes, bad = _crafted_one(9, 1000, 16)
    assert dec.decode_ragged_device([a[2], bad, b[2]]) == [0, 0, 0]
    got, status = dec.transcode_ragged_device([(100, -1)] * 3, False, [M.ROT_180] * 3)
    assert status == [0, api.ERR_OVERFLOW_PARAMETER, 0] and got[1] is None
    assert got[0] == _expected(infos[0], a[1], 100, M.ROT_180)[1] and got[2] == _expected(infos[2], b[1], 100, M.ROT_180)[1]
    got, status = dec.transcode_ragged_device(None, False, [M.ROT_180] * 3)  # (kept, 1000 is inside the range)
    assert status == [0, 0, 0] and got[1] == _expected(f, planes, None, M.ROT_180)[1]
    _, back = oracle.decode_coefficients(got[1])
    assert back[1][0, 0].reshape(-1)[9] == 1000  # (block (2, 1) of 3 x 2 becomes block (0, 0); position 9 is u = v = 1: negated once per axis)
    # the call's own argument check, with a decoded batch on the object
    for code in (8, -1, 0x200, 9 | M.TRIM):
        with pytest.raises(api.MijpegError) as e:
            dec.transcode_ragged_device(None, False, [code, 0, 0])
        assert e.value.code == api.ERR_INVALID_PARAMETER


# ------------------------------------------------------------------------------------------------ 5. launches do not grow
def test_launches_and_waits_do_not_grow_and_untransformed_lists_are_the_parents(dec):
    # (the coder's scans are one launch up to 1023 elements and three beyond, whatever the first stage: as in the untransformed
    # call's test the 32 pictures' streams stay below 1024 chunks of 64 bytes, so the counts compare the passes and not the scans)
    rng = np.random.default_rng(4364)
    four = [_craft(rng, 48, 32, "420", amplitude=3)[2], _craft(rng, 32, 16, "422", amplitude=3)[2], _craft(rng, 72, 56, "444", amplitude=3)[2],
            _craft(rng, 8, 24, "grey", amplitude=3)[2]]
    stats = {}
    for times in (1, 8):
        n = 4 * times
        assert dec.decode_ragged_device(four * times) == [0] * n
        for optimize in (False, True):
            got, status = dec.transcode_ragged_device([(75, 0)] * n, optimize, [M.ROT_90] * n)
            assert status == [0] * n and got[:4] * times == got
            stats[(times, optimize)] = dict(dec.transcode_ragged_stats(), **dec.transcode_transform_stats())
            assert stats[(times, optimize)]["bytes_downloaded"] < 1024 * 64
    for optimize in (False, True):
        a, b = stats[(1, optimize)], stats[(8, optimize)]
        assert (a["transformed"], b["transformed"]) == (4, 32) and b["bytes_downloaded"] > a["bytes_downloaded"]
        for k in ("requant_launches", "transform_launches", "coder_launches", "host_syncs", "passes"):
            assert a[k] == b[k], (k, optimize, a, b)
        assert a["requant_launches"] == 0 and a["transform_launches"] == a["passes"] == 1 and a["host_syncs"] == (4 if optimize else 3)
    # a list without transforms: the existing call's streams and statistics, whichever entry point takes it
    want, status = dec.transcode_ragged_device([(75, 0)] * 32, True)
    parent = dec.transcode_ragged_stats()
    assert dec.transcode_transform_stats() == dict(transformed=0, trimmed=0, geometry_refusals=0, transform_launches=0)
    got, status2 = dec.transcode_ragged_device([(75, 0)] * 32, True, [M.NONE, M.NONE | M.TRIM] * 16)
    assert got == want and status2 == status and dec.transcode_ragged_stats() == parent and parent["requant_launches"] == 1
    assert dec.transcode_transform_stats() == dict(transformed=0, trimmed=0, geometry_refusals=0, transform_launches=0)
    assert parent["host_syncs"] == stats[(8, True)]["host_syncs"]


# ------------------------------------------------------------------------------------------------ 6. the stores survive
def test_the_decodes_stores_survive(dec):
    import torch

    names = ["pil_131x77_422", "pil_70x40_gray", "pilprog_75x45_420", "ref_97x61_440", "pil_9x9_420"]
    streams = [golden_jpeg(n) for n in names]
    codes = [M.ROT_90 | M.TRIM, M.FLIP_V | M.TRIM, M.TRANSVERSE | M.TRIM, M.TRANSPOSE, M.NONE]

    def pixels():
        infos = [dec.ragged_info(i) for i in range(len(names))]
        tensors = [torch.zeros((f.height, f.width * f.components), dtype=torch.uint8, device="cuda:0") for f in infos]
        dec.reconstruct_ragged_device([t.data_ptr() for t in tensors], [f.width * f.components for f in infos])
        return [t.cpu().numpy() for t in tensors]

    assert dec.decode_ragged_device(streams) == [0] * len(names)
    before = pixels()
    first, status = dec.transcode_ragged_device([(50, 0), (0, -1), (75, 1), (0, -1), (100, 2)], False, codes)
    assert status == [0] * len(names)
    assert all(np.array_equal(a, b) for a, b in zip(before, pixels()))
    again, _ = dec.transcode_ragged_device([(50, 0), (0, -1), (75, 1), (0, -1), (100, 2)], False, codes)
    assert again == first
    for i, name in enumerate(names):  # (goldens with partial MCUs and children of the single-image route, against the model)
        f, planes = _decoded(name)
        q = (50, None, 75, None, 100)[i]
        rc, out, ri, kept = api.transcode_plan_transformed(f, api.TRANSCODE_KEEP if q is None else q, (0, -1, 1, -1, 2)[i], codes[i])
        assert rc == 0 and first[i] == api.encode_coefficients(out, M.transcode_planes(f, planes, out, codes[i])[0], ri, False, threads=1), name


# ------------------------------------------------------------------------------------------------ 7. EXIF
def test_transcode_mixed_makes_exif_orientations_upright(dec):
    rng = np.random.default_rng(4365)
    colour, grey = _dc_only(rng, 24, 16, "444"), _dc_only(rng, 16, 40, "grey")
    com = b"\xff\xfe" + struct.pack(">H", 5) + b"abc"
    streams, want_codes = [], []
    for k in range(1, 9):
        streams += [_with_segments(colour, _app1(k, "II")), _with_segments(grey, com, _app1(k, "MM"))]
        want_codes += [EXIF_CODES[k]] * 2
    streams.append(colour)  # (no tag: orientation 1)
    want_codes.append(M.NONE)
    assert [batch.exif_orientation(s) for s in streams] == [k for k in range(1, 9) for _ in range(2)] + [1]
    base = _pixels(dec, [colour, grey])
    parts = [batch.transcode_mixed(streams, transform="exif", rank=r, world=2) for r in range(2)]
    upright = []
    for i in range(len(streams)):
        mine, other = parts[i % 2][i], parts[1 - i % 2][i]
        assert other is None and isinstance(mine, bytes), (i, mine)
        assert b"Exif" not in mine and batch.exif_orientation(mine) == 1  # (no APPn is carried across: no stale tag)
        upright.append(mine)
    for i, p in enumerate(_pixels(dec, upright)):
        assert np.array_equal(p, HWC_OPS[want_codes[i]](base[i % 2 if i < 16 else 0])), (i, M.NAMES[want_codes[i]])
    whole = batch.transcode_mixed(streams, transform="exif", decoder=dec)
    assert whole == upright and dec.transcode_transform_stats()["transformed"] == 14

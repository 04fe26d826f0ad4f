"""Ragged encode of lists that mix 8-bit and 12-bit pictures on the device (mijpeg_encode_ragged_device16, mijpeg_encode_ragged16,
libjpeg_amd.batch.encode_mixed): every stream byte for byte against the single-image encoders -- mijpeg_encode_image_ex
for an 8-bit picture, mijpeg_encode_image16 for a 12-bit one, both pinned to the reference encoder --, the goldens the reference
encoder wrote as one list, the widest symbols at picture boundaries, the launch and synchronisation counts, pass cutting and the
failure behaviour.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import enc12_util as U
from libjpeg_amd import api, batch, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _torch():
    import torch

    return torch


def _picture(w, h, layout, precision, seed):
    """Seeded content: enc12_util.synth12 at 12 bits, synth.synth_image at 8; grey pictures 2-D."""
    nc = 1 if layout == "grey" else 3
    img = U.synth12(w, h, seed, nc) if precision == 12 else synth.synth_image(w, h, seed, channels=nc)
    return np.ascontiguousarray(img[..., 0] if nc == 1 else img)


def _single(dec, img, q, layout, ri, opt) -> bytes:
    """The single-image encoder for one picture with the layout's sampling factors: mijpeg_encode_image16 for uint16 samples (its
    tables are always the picture's own), mijpeg_encode_image_ex otherwise; flags 0."""
    hs, vs = U.LAYOUTS[layout][0]
    if img.dtype == np.uint16:
        return dec._encode16(img, q, (hs, vs), ri, "gpu")
    h, w = img.shape[:2]
    nc = 1 if img.ndim == 2 else img.shape[2]
    L = api.lib()
    L.mijpeg_encode_image_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    p, n = C.c_void_p(), C.c_size_t()
    pad = (1,) * (4 - len(hs))
    dec._check(L.mijpeg_encode_image_ex(dec._h, img.ctypes.data, w, h, nc, w * nc, q, (C.c_int32 * 4)(*hs, *pad), (C.c_int32 * 4)(*vs, *pad), ri,
                                        1 if opt else 0, 0, C.byref(p), C.byref(n)))
    try:
        return C.string_at(p, n.value)
    finally:
        L.mijpeg_free(p)


def _frame(img, layout, q, ri, pixels):
    hs, vs = U.LAYOUTS[layout][0]
    h, w = img.shape[:2]
    return api.encode_frame(w, h, len(hs), q, (hs, vs), ri, pixels, w * len(hs) * img.itemsize)


def _upload(imgs):
    """The pictures in HBM (uint16 samples as int16: the same bits)."""
    torch = _torch()
    return [torch.from_numpy(im.view(np.int16) if im.dtype == np.uint16 else im).cuda() for im in imgs]


def _device_frames(cases, imgs):
    tensors = _upload(imgs)
    return [_frame(im, lay, q, ri, t.data_ptr()) for (_, _, lay, q, ri, _), im, t in zip(cases, imgs, tensors)], tensors


def _precisions(imgs):
    return [12 if im.dtype == np.uint16 else 8 for im in imgs]


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


# (width, height, layout): the 4:2:0 shapes -- below a tile (interior kernels only, an odd width: per-block kernel only), one tile
# without strips, tiles with strips and partial blocks, 256 x 256 twice in a row so that the work-list search crosses items of several
# workgroups -- and the other layouts
SHAPES = [(1, 1, "420"), (7, 9, "420"), (72, 40, "420"), (75, 45, "420"), (128, 128, "420"), (130, 200, "420"), (272, 144, "420"),
          (256, 256, "420"), (256, 256, "420"),
          (72, 40, "444"), (75, 45, "444"), (72, 40, "422"), (75, 45, "422"), (72, 40, "440"), (75, 45, "440"),
          (33, 17, "411"), (97, 61, "3x3"), (70, 50, "grey"), (1, 1, "grey")]
# shapes that come a second time at the other precision, so that every kernel family (tile, the four interior kernels, per-block)
# sees both precisions
BOTH = [(72, 40, "420"), (128, 128, "420"), (130, 200, "420"), (75, 45, "420"), (72, 40, "444"), (72, 40, "422"), (72, 40, "440"), (97, 61, "3x3"),
        (70, 50, "grey")]


def _mixed_cases():
    """(w, h, layout, quality, restart interval, precision): precisions alternate along the list."""
    shapes = list(SHAPES)
    first = {}
    for i, s in enumerate(shapes):
        first.setdefault(s, 12 if i % 2 else 8)
    for s in BOTH:
        if (12 if len(shapes) % 2 else 8) == first[s]:
            shapes.append((1, 1, "grey"))  # (shifts the next picture to the other precision)
        shapes.append(s)
    return [(w, h, lay, (2, 30, 85, 100)[i % 4], (0, 1, 4, 600)[(i // 2) % 4], 12 if i % 2 else 8) for i, (w, h, lay) in enumerate(shapes)]


@pytest.mark.parametrize("optimize", [False, True])
def test_mixed_precision_list_equals_the_single_image_encoders(dec, oracle, optimize):
    cases = _mixed_cases()
    assert 28 <= len(cases) <= 36 and [c[5] for c in cases] == [12 if i % 2 else 8 for i in range(len(cases))]
    assert {c[:3] for c in cases} >= set(SHAPES) and {c[3] for c in cases} == {2, 30, 85, 100} and {c[4] for c in cases} == {0, 1, 4, 600}
    for s in BOTH:
        assert {c[5] for c in cases if c[:3] == s} == {8, 12}, s
    assert cases[7][:3] == cases[8][:3] == (256, 256, "420")
    imgs = [_picture(w, h, lay, p, 7000 + i) for i, (w, h, lay, _, _, p) in enumerate(cases)]
    prec = _precisions(imgs)
    assert prec == [c[5] for c in cases]
    expected = [_single(dec, im, q, lay, ri, optimize) for im, (_, _, lay, q, ri, _) in zip(imgs, cases)]
    for e, c, im in zip(expected, cases, imgs):
        assert _sof(e) == ((0xC1, 12) if c[5] == 12 else (0xC0, 8)) and e[:2] == b"\xff\xd8" and e[-2:] == b"\xff\xd9"
        if c[2] != "3x3":  # (Decoder.encode takes the layouts it knows by name)
            assert e == dec.encode(im, c[3], "444" if c[2] == "grey" else c[2], c[4], optimize)
    frames, keep = _device_frames(cases, imgs)
    from_device = dec.encode_ragged_device(frames, optimize, precision=prec)
    st = dec.encode_ragged_stats()
    assert st["pictures"] == len(cases) and st["passes"] == 1 and 7 <= st["forward_launches"] <= 12 and st["host_syncs"] == 4
    hframes = [_frame(im, lay, q, ri, im.ctypes.data) for (_, _, lay, q, ri, _), im in zip(cases, imgs)]
    from_host = dec._encode_ragged(api.lib().mijpeg_encode_ragged16, hframes, optimize, precision=prec)
    quals, ris = [c[3] for c in cases], [c[4] for c in cases]
    subs = [U.LAYOUTS["444" if c[2] == "grey" else c[2]][0] for c in cases]  # (sampling factors: "3x3" has no name in api.ENCODE_LAYOUTS)
    from_numpy = batch.encode_mixed(imgs, quals, subs, ris, optimize, decoder=dec)
    from_tensors = batch.encode_mixed(keep, quals, subs, ris, optimize, decoder=dec)
    assert len(from_device) == len(from_host) == len(from_numpy) == len(from_tensors) == len(cases)
    for i, c in enumerate(cases):
        assert from_device[i] == expected[i], (i, c, len(from_device[i]), len(expected[i]))
        assert from_host[i] == expected[i], (i, c)
        assert from_numpy[i] == expected[i], (i, c)
        assert from_tensors[i] == expected[i], (i, c)
        # (implied by the bytes; catches a comparison that compares nothing)
        oi, _ = oracle.decode_coefficients(from_device[i])
        assert (oi.width, oi.height, oi.precision, oi.restart_interval) == (c[0], c[1], c[5], c[4]), (i, c)
    del keep


def test_goldens_as_one_list(dec, oracle):
    """The pictures of tests/golden/enc12 in one call, each with its own quality and restart interval: the reference encoder's own
    quantiser tables and coefficients.  (Without the -c golden: a ragged frame cannot ask for the identity transformation.)"""
    keys = [k for k in sorted(U.CASES) if "-c" not in U.CASES[k][6]]
    assert len(keys) == len(U.CASES) - 1 and {U.CASES[k][5] for k in keys} == {2, 30, 85, 100} and any(U.case_restart(k) for k in keys)
    imgs = []
    for k in keys:
        img = U.case_image(k)
        imgs.append(np.ascontiguousarray(img[..., 0] if U.CASES[k][2] == "grey" else img))
    cases = [(U.CASES[k][0], U.CASES[k][1], U.CASES[k][2], U.CASES[k][5], U.case_restart(k), 12) for k in keys]
    frames, keep = _device_frames(cases, imgs)
    streams = dec.encode_ragged_device(frames, False, precision=[12] * len(keys))
    for k, (w, h, lay, q, ri, _), data in zip(keys, cases, streams):
        assert _sof(data) == (0xC1, 12), k
        gold, gplanes = U.golden_coefficients(k)
        oi, planes = oracle.decode_coefficients(data)
        assert (oi.width, oi.height, oi.precision, oi.restart_interval, oi.ncomp) == (w, h, 12, ri, gold.ncomp), k
        for c in range(oi.ncomp):
            assert np.array_equal(U.oracle_quant(oi, c), U.oracle_quant(gold, c)), (k, c)
            nbx, nby = U.covered_blocks(w, h, oi.subx[c], oi.suby[c])
            assert planes[c].shape == gplanes[c].shape
            assert np.array_equal(planes[c][:nby, :nbx], gplanes[c][:nby, :nbx]), (k, c)
    del keep


@pytest.mark.parametrize("ri", [0, 1])
def test_widest_symbols_at_picture_boundaries(dec, oracle, ri):
    """AC category 14 (pixel_checker) and DC category 15 (block_checker) at quality 100, each between two 1 x 1 pictures of the other
    precision: no code word or value bit leaks into a neighbour's words, chunks or tables."""
    cases, imgs = [], []
    for content in (U.pixel_checker, U.block_checker):
        for k in range(3):
            if k == 1:
                cases.append((64, 40, "444", 100, ri, 12))
                imgs.append(content(64, 40))
            else:
                cases.append((1, 1, "444", 100, ri, 8))
                imgs.append(synth.synth_image(1, 1, 60 + k, channels=3))
    # ... and the other way round: an 8-bit checkerboard (the widest 8-bit symbols) between two 12-bit pixels
    for k in range(3):
        if k == 1:
            cases.append((64, 40, "444", 100, ri, 8))
            imgs.append((U.pixel_checker(64, 40) >> 4).astype(np.uint8))
        else:
            cases.append((1, 1, "444", 100, ri, 12))
            imgs.append(U.synth12(1, 1, 70 + k))
    imgs = [np.ascontiguousarray(im) for im in imgs]
    expected = [_single(dec, im, 100, "444", ri, False) for im in imgs]
    _, planes = oracle.decode_coefficients(expected[1])
    assert int(np.abs(planes[0][..., 1:]).max()).bit_length() == 14
    _, planes = oracle.decode_coefficients(expected[4])
    assert int(np.abs(np.diff(planes[0][..., 0].reshape(-1))).max()).bit_length() == 15
    frames, keep = _device_frames(cases, imgs)
    for opt in (False, True):
        got = dec.encode_ragged_device(frames, opt, precision=_precisions(imgs))
        for i, c in enumerate(cases):
            assert got[i] == (expected[i] if c[5] == 12 or not opt else _single(dec, imgs[i], 100, "444", ri, True)), (opt, i, c)
    del keep


def _small_list(n, precisions):
    """The same KIND of list for every n (as test_ragged_encode.py::_small_list): four layouts in turn, each with one width, heights
    16..24; precisions[i % len] is picture i's."""
    cases = [((16, 24, 20, 32)[i % 4], 16 + (i // 4) % 9, ("444", "420", "grey", "422")[i % 4], 85, 0, precisions[i % len(precisions)]) for i in range(n)]
    return cases, [_picture(w, h, lay, p, 100 + i) for i, (w, h, lay, _, _, p) in enumerate(cases)]


@pytest.mark.parametrize("kind", ["all12", "mixed", "all8", "all8_optimize"])
def test_launches_and_synchronisations_do_not_grow_with_n(dec, kind):
    # (mixed: the precision changes with every picture; a layout keeps its precision, so the list is of the same kind for every n)
    precisions = {"all12": (12,), "mixed": (8, 12)}.get(kind, (8,))
    optimize = kind == "all8_optimize"
    stats = {}
    for n in (4, 64):
        cases, imgs = _small_list(n, precisions)
        frames, keep = _device_frames(cases, imgs)
        streams = dec.encode_ragged_device(frames, optimize, precision=None if kind.startswith("all8") else _precisions(imgs))
        stats[n] = dec.encode_ragged_stats()
        assert stats[n]["pictures"] == n and stats[n]["passes"] == 1 and len(streams) == n
        for i in range(n):
            assert streams[i] == _single(dec, imgs[i], 85, cases[i][2], 0, optimize), (n, i, cases[i])
        if kind.startswith("all8"):  # streams and statistics of the old entry point
            assert dec.encode_ragged_device(frames, optimize) == streams
            assert dec.encode_ragged_stats() == stats[n]
            assert dec.encode_ragged_device(frames, optimize, precision=[8] * n) == streams
            assert dec.encode_ragged_stats() == stats[n]
        del keep
    for k in ("forward_launches", "coder_launches", "host_syncs"):
        assert stats[4][k] == stats[64][k] and stats[4][k] > 0, (k, stats)
    assert stats[64]["host_syncs"] == {"all12": 4, "mixed": 4, "all8": 3, "all8_optimize": 4}[kind]
    assert stats[64]["forward_launches"] <= (12 if kind == "mixed" else 6)
    assert stats[64]["bytes_downloaded"] > stats[4]["bytes_downloaded"] > 0


def test_pass_cutting_is_invisible(dec, monkeypatch):
    cases = [((64, 72, 56, 80)[i % 4], (64, 48, 80)[i % 3], ("444", "420", "422", "grey", "411")[i % 5], (30, 85, 100)[i % 3], (0, 2)[i % 2],
              (8, 12, 12)[i % 3] if i % 7 else 8) for i in range(20)]
    assert {c[5] for c in cases} == {8, 12}
    imgs = [_picture(w, h, lay, p, 500 + i) for i, (w, h, lay, _, _, p) in enumerate(cases)]
    prec = _precisions(imgs)
    frames, keep = _device_frames(cases, imgs)
    for opt in (False, True):
        expected = [_single(dec, im, q, lay, ri, opt) for im, (_, _, lay, q, ri, _) in zip(imgs, cases)]
        whole = dec.encode_ragged_device(frames, opt, precision=prec)
        assert dec.encode_ragged_stats()["passes"] == 1
        monkeypatch.setenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS", "1536")
        cut = dec.encode_ragged_device(frames, opt, precision=prec)
        st = dec.encode_ragged_stats()
        monkeypatch.delenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS")
        assert st["passes"] >= 3 and st["pictures"] == 20 and st["host_syncs"] <= 4 * st["passes"] and st["forward_launches"] <= 12 * st["passes"]
        for i in range(20):
            assert whole[i] == expected[i] and cut[i] == expected[i], (opt, i, cases[i])
    del keep


def test_reused_arenas_under_three_layouts(dec):
    """Three calls back to back on one object, so that the pass's arenas are laid out three ways over the same memory: eight pictures
    of every routing (4:4:4, 4:2:0 of one MCU, below a tile, exactly one tile, a tile with edge strips, 4:2:2, 1 x 2, grey) with
    precisions alternating 8 and 12 and no `optimize` -- table and histogram arenas of four --, then its first two pictures as 8-bit
    ones -- empty arenas, everything behind them further to the front --, then the first list again."""
    shapes = [(8, 8, "444"), (16, 16, "420"), (127, 127, "420"), (128, 128, "420"), (136, 130, "420"), (17, 9, "422"), (9, 17, "440"), (33, 7, "grey")]
    cases = [(w, h, lay, (30, 85, 100, 2)[i % 4], 0, 12 if i % 2 else 8) for i, (w, h, lay) in enumerate(shapes)]
    imgs = [_picture(w, h, lay, p, 900 + i) for i, (w, h, lay, _, _, p) in enumerate(cases)]
    two_cases = [c[:5] + (8,) for c in cases[:2]]
    two_imgs = [imgs[0], _picture(16, 16, "420", 8, 901)]
    expected = [_single(dec, im, q, lay, ri, False) for im, (_, _, lay, q, ri, _) in zip(imgs, cases)]
    two_expected = [_single(dec, im, q, lay, ri, False) for im, (_, _, lay, q, ri, _) in zip(two_imgs, two_cases)]
    frames, keep = _device_frames(cases, imgs)
    two_frames, two_keep = _device_frames(two_cases, two_imgs)
    first = dec.encode_ragged_device(frames, False, precision=_precisions(imgs))
    first_stats = dec.encode_ragged_stats()
    two = dec.encode_ragged_device(two_frames, False, precision=[8, 8])
    two_stats = dec.encode_ragged_stats()
    again = dec.encode_ragged_device(frames, False, precision=_precisions(imgs))
    assert dec.encode_ragged_stats() == first_stats
    assert first_stats["pictures"] == 8 and first_stats["passes"] == 1 and first_stats["host_syncs"] == 4
    assert two_stats["pictures"] == 2 and two_stats["passes"] == 1 and two_stats["host_syncs"] == 3
    assert len(first) == len(again) == 8 and len(two) == 2
    for i, c in enumerate(cases):
        assert _sof(expected[i]) == ((0xC1, 12) if c[5] == 12 else (0xC0, 8))
        assert first[i] == expected[i], ("first", i, c)
        assert again[i] == expected[i], ("again", i, c)
    for i, c in enumerate(two_cases):
        assert two[i] == two_expected[i], ("two", i, c)
    del keep, two_keep


def test_failure_leaves_nothing_behind(dec):
    L = api.lib()
    cases, imgs = _small_list(6, (8, 12))
    assert cases[3][5] == 12 and cases[3][2] == "422"
    frames, keep = _device_frames(cases, imgs)
    prec = _precisions(imgs)
    w3 = cases[3][0]
    wide = _torch().zeros((cases[3][1], w3 * 3 + 8), dtype=_torch().int16, device="cuda")  # room for an odd address and an odd stride
    spoils = (dict(precision=10),
              dict(pixels=wide.data_ptr(), row_stride=w3 * 6 + 1),  # an odd row stride at precision 12
              dict(pixels=wide.data_ptr() + 1, row_stride=w3 * 6 + 2),  # an odd pixel address
              dict(row_stride=w3 * 3))  # a line of 8-bit samples: too small at 2 bytes per sample
    for spoil in spoils:
        bad, bad_prec = list(frames), list(prec)
        f = api.MijpegEncodeFrame.from_buffer_copy(bytes(frames[3]))
        for k, v in spoil.items():
            if k == "precision":
                bad_prec[3] = v
            else:
                setattr(f, k, v)
        bad[3] = f
        arr = (api.MijpegEncodeFrame * 6)(*bad)
        for fn in (L.mijpeg_encode_ragged_device16, L.mijpeg_encode_ragged16):
            if fn is L.mijpeg_encode_ragged16:  # the same list in host memory
                host = [np.ascontiguousarray(im) for im in imgs]
                harr = (api.MijpegEncodeFrame * 6)(*bad)
                room = np.zeros(cases[3][1] * (w3 * 6 + 16) + 16, np.uint8)
                room = room[(-room.ctypes.data) % 2:]  # (an even address)
                for i, im in enumerate(host):
                    harr[i].pixels = im.ctypes.data
                if "pixels" in spoil:
                    harr[3].pixels = room.ctypes.data + (spoil["pixels"] - wide.data_ptr())
                call_arr = harr
            else:
                call_arr = arr
            ptrs, sizes = (C.c_void_p * 6)(*([0xdead0] * 6)), (C.c_size_t * 6)(*([77] * 6))
            assert fn(dec._h, call_arr, (C.c_int32 * 6)(*bad_prec), 6, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER, spoil
            assert all(not ptrs[i] for i in range(6)) and all(sizes[i] == 0 for i in range(6)), spoil
            msg = C.c_char_p()
            assert L.mijpeg_last_error(dec._h, C.byref(msg)) == api.ERR_INVALID_PARAMETER and msg.value
    # the object goes on working
    good = dec.encode_ragged_device(frames, False, precision=prec)
    for i in range(6):
        assert good[i] == _single(dec, imgs[i], 85, cases[i][2], 0, False), (i, cases[i])
    del keep, wide

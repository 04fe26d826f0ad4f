"""Ragged encode: lists of pictures of different shapes through one device pass (mijpeg_encode_ragged_plan,
mijpeg_encode_ragged_device, mijpeg_encode_ragged, libjpeg_amd.batch.encode_mixed).

CPU: the host-only planner against mijpeg_frame_layout and against what the host entropy coder writes for the same frames; its
argument checks; the device entry points on an object without a device.
GPU: every stream of every list byte for byte against mijpeg_encode_image_ex for the same picture (which is pinned to the
reference encoder), the launch and synchronisation counts, pass cutting, failure behaviour, the Python front end.
"""
import ctypes as C

import numpy as np
import pytest

from libjpeg_amd import api, batch, synth
from test_encoder import _oj_info

LAYOUTS = {"444": ((1, 1, 1), (1, 1, 1)), "420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "440": ((1, 1, 1), (2, 1, 1)),
           "411": ((4, 1, 1), (1, 1, 1)), "410": ((4, 1, 1), (2, 1, 1)), "grey": ((1,), (1,))}


def _quality_tables(q):
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.mijpeg_quality_tables.restype = None
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    L.mijpeg_quality_tables(q, luma.ctypes.data, chroma.ctypes.data)
    return luma, chroma


def _layout(w, h, layout, q):
    hs, vs = LAYOUTS[layout]
    return api.frame_layout(w, h, len(hs), hs, vs, list(_quality_tables(q)), quant_index=[0] * len(hs), ycbcr=1 if len(hs) == 3 else 0)


def _frame(w, h, layout, q=85, ri=0, pixels=0, row_stride=None):
    return api.encode_frame(w, h, len(LAYOUTS[layout][0]), q, LAYOUTS[layout], ri, pixels, row_stride)


def _restart_markers(stream: bytes) -> int:
    """RSTn markers in the entropy coded segment of a baseline stream with one scan."""
    at = stream.index(b"\xff\xda")
    at += 2 + int.from_bytes(stream[at + 2:at + 4], "big")
    body = np.frombuffer(stream[at:-2], np.uint8)
    ff = np.flatnonzero(body[:-1] == 0xff)
    return int(np.count_nonzero((body[ff + 1] >= 0xd0) & (body[ff + 1] <= 0xd7)))


# ------------------------------------------------------------------------------------------------ CPU: planner
SIDES = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 1000)


def _planner_list():
    """77 descriptions: every side of SIDES as a width and as a height, the seven layouts, restart intervals 0, 1, 3 and one
    beyond the picture's MCU count."""
    out = []
    names = list(LAYOUTS)
    for i, w in enumerate(SIDES):
        for j in range(7):
            h = SIDES[(i * 3 + j * 5) % len(SIDES)]
            layout = names[(i + j) % 7]
            ri = (0, 1, 3, 65000)[(i + 2 * j) % 4]
            out.append((w, h, layout, (5, 50, 85, 100)[(i + j) % 4], ri))
    return out


def test_planner_layouts_counts_and_index_spaces():
    cases = _planner_list()
    assert {c[0] for c in cases} == set(SIDES) and {c[1] for c in cases} == set(SIDES) and {c[2] for c in cases} == set(LAYOUTS)
    items, totals = api.encode_ragged_plan([_frame(w, h, lay, q, ri) for w, h, lay, q, ri in cases])
    assert len(items) == len(cases) and totals.passes == 1
    at_block = at_interval = 0
    spans = []
    for (w, h, lay, q, ri), it in zip(cases, items):
        # the completed frame is mijpeg_frame_layout's
        ref = _layout(w, h, lay, q)
        got = it.info
        nc = ref.components
        assert (got.width, got.height, got.components, got.precision, got.ycbcr, got.mcus_x, got.mcus_y, got.coef_count, got.sample_bytes) == \
               (w, h, nc, 8, ref.ycbcr, ref.mcus_x, ref.mcus_y, ref.coef_count, ref.sample_bytes)
        for c in range(nc):
            for k in ("hsamp", "vsamp", "subx", "suby", "blocks_w", "blocks_h", "coef_offset", "quant_index"):
                assert getattr(got, k)[c] == getattr(ref, k)[c], (w, h, lay, k, c)
        assert list(got.quant[0]) == list(ref.quant[0]) and list(got.quant[1]) == list(ref.quant[1])
        # blocks and intervals: what the host coder's stream of the same frame shows.  One MCU per interval: markers + 1 = MCUs
        per_mcu = sum(hs * vs for hs, vs in zip(*LAYOUTS[lay])) if nc == 3 else 1
        zeros = np.zeros(int(ref.coef_count), np.int16)
        mcus = ref.mcus_x * ref.mcus_y
        assert mcus <= 65535 or ri != 1
        if mcus <= 65535:
            assert _restart_markers(api.encode_coefficients(ref, zeros, 1)) + 1 == mcus
        assert it.blocks == mcus * per_mcu, (w, h, lay)
        assert it.intervals == _restart_markers(api.encode_coefficients(ref, zeros, ri)) + 1, (w, h, lay, ri)
        if ri == 65000:
            assert ri > mcus and it.intervals == 1
        # index spaces: whole workgroups per picture, list order, nothing shared
        assert it.first_block % 256 == 0 and it.first_block == at_block and it.first_interval == at_interval and it.pass_ == 0
        at_block += (it.blocks + 255) // 256 * 256
        at_interval += it.intervals
        spans.append((it.coef_base, int(ref.coef_count)))
    assert (totals.blocks, totals.intervals) == (at_block, at_interval)
    end = 0
    for base, count in sorted(spans):
        assert base >= end and base % 128 == 0
        end = base + count
    assert end <= totals.coef_count < end + 128


def test_planner_cuts_passes():
    frames = [_frame(64, 64, "444") for _ in range(20)]  # 192 blocks each, 256 with padding
    items, totals = api.encode_ragged_plan(frames, 2048)
    assert [it.pass_ for it in items] == [i // 8 for i in range(20)] and totals.passes == 3
    assert [it.first_block for it in items] == [256 * (i % 8) for i in range(20)]
    assert [it.first_interval for it in items] == [i % 8 for i in range(20)]
    assert [it.coef_base for it in items] == [items[1].coef_base * (i % 8) for i in range(20)]
    assert totals.blocks == 20 * 256 and totals.intervals == 20 and totals.coef_count == 8 * items[1].coef_base
    # a picture beyond the limit is a pass of its own
    items, totals = api.encode_ragged_plan([_frame(8, 8, "444"), _frame(1000, 1000, "444"), _frame(8, 8, "444")], 512)
    assert [it.pass_ for it in items] == [0, 1, 2] and totals.passes == 3


def test_planner_argument_errors():
    L = api.lib()
    good = _frame(64, 48, "420", 85, 2)
    items, totals = (api.MijpegEncodeRaggedItem * 2)(), api.MijpegEncodeRaggedTotals()

    def plan(frame_list, n=None, it=items, tot=totals):
        arr = (api.MijpegEncodeFrame * max(1, len(frame_list)))(*frame_list)
        return L.mijpeg_encode_ragged_plan(arr, len(frame_list) if n is None else n, 0, it, C.byref(tot) if tot is not None else None)

    assert plan([good]) == 0
    assert plan([good], n=0) == api.ERR_INVALID_PARAMETER
    assert plan([good], n=-1) == api.ERR_INVALID_PARAMETER
    assert plan([good], it=None) == api.ERR_INVALID_PARAMETER
    assert plan([good], tot=None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_encode_ragged_plan(None, 1, 0, items, C.byref(totals)) == api.ERR_INVALID_PARAMETER

    def bad(**kw):
        f = _frame(64, 48, "420", 85, 2)
        for k, v in kw.items():
            if isinstance(v, tuple):
                for c, x in enumerate(v):
                    getattr(f, k)[c] = x
            else:
                setattr(f, k, v)
        return f

    # (more than 64 blocks per MCU cannot be described with three components and factors up to 4 -- 48 at most --; the planner's
    # check of it is a guard for the coder's tables and has no case here)
    for kw in (dict(components=0), dict(components=2), dict(components=4), dict(hsamp=(0, 1, 1)), dict(hsamp=(5, 1, 1)), dict(vsamp=(2, 0, 1)),
               dict(vsamp=(1, 1, 5)), dict(hsamp=(3, 2, 1)), dict(restart_interval=-1), dict(restart_interval=65536), dict(width=0),
               dict(width=65536), dict(height=0), dict(height=65536), dict(height=-3)):
        assert plan([bad(**kw)]) == api.ERR_INVALID_PARAMETER, kw
        assert plan([good, bad(**kw)]) == api.ERR_INVALID_PARAMETER, kw  # anywhere in the list
    for kw in (dict(restart_interval=65535), dict(width=65535, height=1), dict(hsamp=(4, 2, 1), vsamp=(4, 1, 2))):
        assert plan([bad(**kw)]) == 0, kw


def test_device_entry_points_without_a_device():
    """As test_encoder_entry_points_reject_bad_arguments_without_a_device for the existing ones: NOT_AVAILABLE and a message."""
    L = api.lib()
    d = api.Decoder(None)
    img = synth.synth_image(24, 16, 3)
    with pytest.raises(api.MijpegError) as e:
        d.encode_ragged([img], 85, "420")
    assert e.value.code == api.ERR_NOT_AVAILABLE and "device" in e.value.message
    with pytest.raises(api.MijpegError) as e:
        d.encode_ragged_device([_frame(24, 16, "420", pixels=4096)])
    assert e.value.code == api.ERR_NOT_AVAILABLE and "device" in e.value.message
    with pytest.raises(api.MijpegError) as e:
        batch.encode_mixed([img], decoder=d)
    assert e.value.code == api.ERR_NOT_AVAILABLE
    # argument checks come first and need no device either
    arr = (api.MijpegEncodeFrame * 1)(_frame(24, 16, "420", pixels=4096))
    ptrs, sizes = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    for fn in (L.mijpeg_encode_ragged_device, L.mijpeg_encode_ragged):
        assert fn(d._h, arr, 0, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, None, 1, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, arr, 1, 0, 0, None, sizes) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, arr, 1, 0, 0, ptrs, None) == api.ERR_INVALID_PARAMETER
        assert fn(None, arr, 1, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER
    st = api.MijpegEncodeRaggedStats()
    assert L.mijpeg_encode_ragged_get_stats(d._h, None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_encode_ragged_get_stats(d._h, C.byref(st)) == 0 and st.pictures == 0
    d.close()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _torch():
    import torch

    return torch


def _single(dec, img, q, layout, ri, opt) -> bytes:
    """mijpeg_encode_image_ex for one picture with the layout's sampling factors (Decoder.encode knows five of them by name)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    nc = 1 if img.ndim == 2 else img.shape[2]
    hs, vs = LAYOUTS[layout]
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


def _images(cases, seed0):
    """cases: (w, h, layout, q, ri) -> synth images (grey ones 2-D)."""
    out = []
    for i, (w, h, lay, _, _) in enumerate(cases):
        img = synth.synth_image(w, h, seed0 + i, channels=1 if lay == "grey" else 3)
        out.append(img[..., 0] if lay == "grey" else img)
    return out


def _device_frames(cases, imgs):
    """The pictures in HBM (kept alive by the returned tensors) and their descriptions."""
    torch = _torch()
    tensors = [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]
    frames = [_frame(w, h, lay, q, ri, t.data_ptr()) for (w, h, lay, q, ri), t in zip(cases, tensors)]
    return frames, tensors


def _host_frames(cases, imgs):
    imgs = [np.ascontiguousarray(im) for im in imgs]
    return [_frame(w, h, lay, q, ri, im.ctypes.data) for (w, h, lay, q, ri), im in zip(cases, imgs)], imgs


def _mixed_cases():
    sizes = [(1, 1), (7, 9), (8, 8), (9, 7), (15, 17), (16, 16), (17, 15), (24, 40), (31, 33), (64, 64), (100, 60), (127, 129), (128, 128),
             (129, 127), (130, 200), (200, 130), (255, 257), (256, 256), (333, 257), (400, 300), (513, 140), (640, 360), (641, 361),
             (1000, 700), (1097, 693), (1100, 700)]
    names = list(LAYOUTS)
    cases = []
    for i in range(52):
        w, h = sizes[(i * 7) % len(sizes)]
        cases.append((w, h, names[i % 7], (5, 50, 85, 100)[(i // 2) % 4], (0, 1, 3, 600)[(i // 3) % 4]))
    # 4:2:0 on both sides of the tile kernel's 128 x 128, on the boundary, and off the 16-pixel grid
    cases += [(100, 60, "420", 85, 0), (128, 128, "420", 50, 3), (129, 127, "420", 100, 1), (1100, 700, "420", 85, 600), (641, 361, "420", 5, 0),
              (1, 1, "420", 100, 1), (1097, 693, "grey", 85, 3), (1000, 700, "444", 100, 1)]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("optimize", [False, True])
def test_mixed_list_equals_the_single_image_encoder(dec, oracle, optimize):
    cases = _mixed_cases()
    assert len(cases) >= 40 and {c[2] for c in cases} == set(LAYOUTS) and {c[3] for c in cases} == {5, 50, 85, 100} and {c[4] for c in cases} == {0, 1, 3, 600}
    small420 = [c for c in cases if c[2] == "420" and (c[0] < 128 or c[1] < 128)]
    large420 = [c for c in cases if c[2] == "420" and c[0] >= 128 and c[1] >= 128]
    assert small420 and large420 and any(c[0] % 16 and c[1] % 16 for c in large420)
    assert min(c[0] * c[1] for c in cases) == 1 and max(c[0] for c in cases) == 1100
    imgs = _images(cases, 4000)
    expected = [_single(dec, im, q, lay, ri, optimize) for im, (_, _, lay, q, ri) in zip(imgs, cases)]
    frames, keep = _device_frames(cases, imgs)
    from_device = dec.encode_ragged_device(frames, optimize)
    st = dec.encode_ragged_stats()
    assert st["pictures"] == len(cases) and st["passes"] == 1 and 1 <= st["forward_launches"] <= 6 and st["host_syncs"] == (4 if optimize else 3)
    hframes, keep_host = _host_frames(cases, imgs)
    from_host = dec._encode_ragged(api.lib().mijpeg_encode_ragged, hframes, optimize)
    assert len(from_device) == len(from_host) == len(cases)
    for i, c in enumerate(cases):
        assert from_device[i] == expected[i], (i, c, len(from_device[i]), len(expected[i]))
        assert from_host[i] == expected[i], (i, c)
        assert expected[i][:2] == b"\xff\xd8" and expected[i][-2:] == b"\xff\xd9" and len(expected[i]) > 100
        # (implied by the bytes; catches a comparison that compares nothing)
        a, b = oracle.decode(from_device[i]), oracle.decode(expected[i])
        assert a.shape[:2] == (c[1], c[0]) and np.array_equal(a, b), (i, c)
    del keep, keep_host


@pytest.mark.gpu
def test_uniform_list_equals_the_uniform_batch_call(dec):
    torch = _torch()
    w, h, n = 640, 360, 5
    imgs = [synth.synth_image(w, h, 300 + i) for i in range(n)]
    info = _layout(w, h, "420", 80)
    px = torch.from_numpy(np.stack(imgs)).cuda()
    coef = torch.empty((n, int(info.coef_count)), dtype=torch.int16, device="cuda")
    for ri, opt in ((4, True), (0, False)):
        uniform = dec.encode_batch_device(info, px.data_ptr(), coef.data_ptr(), n, w * 3, h * w * 3, restart_mcus=ri, optimize=opt)
        ragged = dec.encode_ragged_device([_frame(w, h, "420", 80, ri, px[i].data_ptr()) for i in range(n)], opt)
        assert len(uniform) == len(ragged) == n
        for i in range(n):
            assert ragged[i] == uniform[i], (ri, opt, i)


BOUNDARY_SEED = 10  # see _boundary_noise: the first seed whose host-coded stream ends on a stuffed 0xFF (asserted where it is used)


def _boundary_noise(oracle, seed):
    """High-contrast noise, 16 x 16, as the host coder writes it at quality 100 with one MCU per interval."""
    rng = np.random.default_rng(seed)
    img = (rng.integers(0, 2, (16, 16, 3)) * 255).astype(np.uint8)
    info = _layout(16, 16, "444", 100)
    planes = oracle.forward(_oj_info(oracle, info, 16, 16, list(_quality_tables(100))), img, 1)
    coef = np.concatenate([p.reshape(-1) for p in planes]).astype(np.int16)
    return img, api.encode_coefficients(info, coef, 1, False)


@pytest.mark.gpu
def test_picture_boundaries_in_the_bit_stream(dec, oracle):
    """Runs of 1-MCU pictures whose plain streams are shorter than one stuffing chunk, between them noise at quality 100 whose
    streams are full of 0xFF bytes, one MCU per interval: no word, chunk, marker count or stuffing byte leaks into a neighbour."""
    noise, host_coded = _boundary_noise(oracle, BOUNDARY_SEED)
    assert host_coded[-4:] == b"\xff\x00\xff\xd9"  # the seed was chosen on the CPU, with the host coder, for this
    cases, imgs = [], []
    rng = np.random.default_rng(99)
    for i in range(40):
        if i % 4 == 3:
            big = (rng.integers(0, 2, (48, 40, 3)) * 255).astype(np.uint8)
            cases.append((40, 48, "444", 100, 1))
            imgs.append(big)
            cases.append((16, 16, "444", 100, 1))
            imgs.append(noise)
        else:
            lay = ("444", "420", "grey")[i % 3]
            w, h = (8, 8) if lay != "420" else (16, 16)
            img = synth.synth_image(w, h, 800 + i, channels=1 if lay == "grey" else 3)
            cases.append((w, h, lay, 85, 1))
            imgs.append(img[..., 0] if lay == "grey" else img)
    expected = [_single(dec, im, q, lay, ri, False) for im, (_, _, lay, q, ri) in zip(imgs, cases)]
    # the premises: tiny streams below one chunk, streams full of 0xFF, one ending on a stuffed 0xFF
    assert sum(1 for e in expected if len(e) - e.index(b"\xff\xda") - 14 < 64) >= 20
    assert max(e.count(b"\xff\x00") for e in expected) >= 20
    assert any(e[-4:-2] == b"\xff\x00" for e in expected)
    assert host_coded in expected
    frames, keep = _device_frames(cases, imgs)
    got = dec.encode_ragged_device(frames, False)
    for i, c in enumerate(cases):
        assert got[i] == expected[i], (i, c)
    for opt in (False, True):
        hframes, keep_host = _host_frames(cases, imgs)
        got = dec._encode_ragged(api.lib().mijpeg_encode_ragged, hframes, opt)
        for i, (im, c) in enumerate(zip(imgs, cases)):
            assert got[i] == (_single(dec, im, c[3], c[2], c[4], True) if opt else expected[i]), (opt, i, c)
    del keep


def _small_list(n):
    """The same KIND of list for every n: four layouts in turn, each with one width (the forward routing looks at it: lines that
    can be read as dwords go through the interior kernels), heights 16..24."""
    cases = [((16, 24, 20, 32)[i % 4], 16 + (i // 4) % 9, ("444", "420", "grey", "422")[i % 4], 85, 0) for i in range(n)]
    return cases, _images(cases, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("optimize", [False, True])
def test_launches_and_synchronisations_do_not_grow_with_n(dec, optimize):
    stats = {}
    for n in (4, 64):
        cases, imgs = _small_list(n)
        frames, keep = _device_frames(cases, imgs)
        streams = dec.encode_ragged_device(frames, optimize)
        stats[n] = dec.encode_ragged_stats()
        assert stats[n]["pictures"] == n and stats[n]["passes"] == 1
        assert len(streams) == n
        for i in range(n):
            assert streams[i] == _single(dec, imgs[i], 85, cases[i][2], 0, optimize), (n, i, cases[i])
        del keep
    print("coder statistics", optimize, stats)
    for k in ("forward_launches", "coder_launches", "host_syncs"):
        assert stats[4][k] == stats[64][k] and stats[4][k] > 0, (k, stats)
    # seven single launches (count, interval bytes, two gathers, emit, 0xFF count, stuffing), three for the prefix sum over 1024 or
    # 16384 padded blocks, one each for the sums over intervals and chunks, one more for the statistics
    assert stats[64]["coder_launches"] == (13 if optimize else 12)
    assert stats[64]["host_syncs"] <= 4 * stats[64]["passes"]
    assert stats[64]["host_syncs"] == (4 if optimize else 3)
    assert stats[64]["forward_launches"] <= 6
    assert stats[64]["bytes_downloaded"] > stats[4]["bytes_downloaded"] > 0


@pytest.mark.gpu
def test_pass_cutting_is_invisible(dec, monkeypatch):
    cases = [((64, 72, 56, 80)[i % 4], (64, 48, 80)[i % 3], ("444", "420", "422", "grey", "411")[i % 5], (50, 85, 100)[i % 3], (0, 2)[i % 2]) for i in range(20)]
    imgs = _images(cases, 500)
    expected = [_single(dec, im, q, lay, ri, True) for im, (_, _, lay, q, ri) in zip(imgs, cases)]
    frames, keep = _device_frames(cases, imgs)
    whole = dec.encode_ragged_device(frames, True)
    assert dec.encode_ragged_stats()["passes"] == 1
    monkeypatch.setenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS", "1536")
    cut = dec.encode_ragged_device(frames, True)
    st = dec.encode_ragged_stats()
    monkeypatch.delenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS")
    assert st["passes"] >= 3 and st["pictures"] == 20 and st["host_syncs"] <= 4 * st["passes"] and st["forward_launches"] <= 6 * st["passes"]
    for i in range(20):
        assert whole[i] == expected[i] and cut[i] == expected[i], (i, cases[i])
    del keep


@pytest.mark.gpu
def test_failure_leaves_nothing_behind(dec):
    L = api.lib()
    cases, imgs = _small_list(6)
    frames, keep = _device_frames(cases, imgs)
    for spoil in (dict(components=2), dict(width=0), dict(restart_interval=70000), dict(pixels=None), dict(row_stride=3)):
        bad = list(frames)
        f = api.MijpegEncodeFrame.from_buffer_copy(bytes(frames[3]))
        for k, v in spoil.items():
            setattr(f, k, v)
        bad[3] = f
        arr = (api.MijpegEncodeFrame * 6)(*bad)
        ptrs, sizes = (C.c_void_p * 6)(*([0xdead0] * 6)), (C.c_size_t * 6)(*([77] * 6))
        assert L.mijpeg_encode_ragged_device(dec._h, arr, 6, 0, 0, ptrs, sizes) == api.ERR_INVALID_PARAMETER, spoil
        assert all(not ptrs[i] for i in range(6)) and all(sizes[i] == 0 for i in range(6)), spoil
        msg = C.c_char_p()
        assert L.mijpeg_last_error(dec._h, C.byref(msg)) == api.ERR_INVALID_PARAMETER and msg.value
    # unknown flags are refused, too
    arr = (api.MijpegEncodeFrame * 6)(*frames)
    ptrs, sizes = (C.c_void_p * 6)(), (C.c_size_t * 6)()
    assert L.mijpeg_encode_ragged_device(dec._h, arr, 6, 0, 0x80, ptrs, sizes) == api.ERR_INVALID_PARAMETER
    # the object goes on working
    good = dec.encode_ragged_device(frames, False)
    for i in range(6):
        assert good[i] == _single(dec, imgs[i], 85, cases[i][2], 0, False)
    del keep


@pytest.mark.gpu
def test_encode_mixed_front_end(dec):
    torch = _torch()
    cases = [(100, 60, "420", 85, 0), (128, 160, "444", 50, 3), (33, 77, "grey", 100, 1), (200, 130, "422", 5, 600), (64, 64, "411", 85, 0),
             (300, 200, "440", 85, 2)]
    imgs = _images(cases, 900)
    subs = [c[2] if c[2] != "grey" else "444" for c in cases]
    quals, ris = [c[3] for c in cases], [c[4] for c in cases]
    for opt in (False, True):
        expected = [_single(dec, im, q, lay, ri, opt) for im, (_, _, lay, q, ri) in zip(imgs, cases)]
        frames, keep = _device_frames(cases, imgs)
        assert dec.encode_ragged_device(frames, opt) == expected  # the C call
        assert batch.encode_mixed(imgs, quals, subs, ris, opt, decoder=dec) == expected
        tensors = [torch.from_numpy(im).cuda() for im in imgs]
        assert batch.encode_mixed(tensors, quals, subs, ris, opt, decoder=dec) == expected
        assert batch.encode_mixed(tensors, quals, subs, ris, opt) == expected  # an object of its own
    # scalars for all pictures; strided lines of a larger tensor
    colour = [im for im in imgs if im.ndim == 3]
    assert batch.encode_mixed(colour, 70, "420", 4, decoder=dec) == [dec.encode(im, 70, "420", 4) for im in colour]
    canvas = torch.from_numpy(synth.synth_image(256, 128, 5)).cuda()
    view = canvas[8:72, 16:116]
    assert not view.is_contiguous()
    assert batch.encode_mixed([view], 85, "420", decoder=dec) == [dec.encode(view.cpu().numpy(), 85, "420")]
    assert batch.encode_mixed([], decoder=dec) == []
    with pytest.raises(ValueError):
        batch.encode_mixed([imgs[0], tensors[1]], decoder=dec)
    with pytest.raises(ValueError):
        batch.encode_mixed(imgs, [85, 50], decoder=dec)

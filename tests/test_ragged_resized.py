"""Crops of a ragged batch resized into one batch tensor (mijpeg_reconstruct_ragged_resized_device, batch.decode_resized):
stage 1 is the crop call's body into an arena of the object, stage 2 ONE launch of resample_list_kernel for the whole list.

Expected, at tolerance 0: tests/resample_model.py's resize() -- the filter's definition in numpy -- of that rectangle of the oracle's
decode.  Every call writes into one device tensor of 0xA5 with 64 guard bytes at either end, padded lines, planes and slots and a base
at byte offset 0..3, and the WHOLE tensor is compared with what it must hold afterwards, as test_ragged_rect.Arena does for the crops.
One decode per list serves all its calls; the pictures are at most 300 x 270."""
import ctypes as C
import functools

import numpy as np
import pytest

import resample_model as M
from conftest import golden_jpeg
from libjpeg_amd import api
from test_ragged_gates import _expected
from test_ragged_rect import EDGE, GUARD, LAYOUT_NAMES, SIZES, _clip, _layout_list

WHOLE = (0, 0, EDGE, EDGE)
STATS0 = dict(images=0, resampled=0, refused=0, window_launches=0, resample_launches=0, arena_bytes=0)


class BatchArena:
    """The destination of one resized call in a device tensor of 0xA5: GUARD bytes, a base at byte offset `base`, n slots whose lines,
    planes and slots are padded by 5, 7 and 11 bytes, GUARD bytes.  expect(): the tensor as it must look afterwards."""

    def __init__(self, n, ow, oh, channels, planar, base=0):
        import torch

        self.n, self.ow, self.oh, self.channels, self.planar = n, ow, oh, channels, planar
        self.line = ow * (1 if planar else channels)
        self.row = self.line + 5
        self.plane = oh * self.row + 7 if planar else 0
        self.image = (channels * self.plane if planar else oh * self.row) + 11
        self.at = GUARD + base % 4
        self.size = self.at + n * self.image + GUARD
        self.dev = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(self, d, rects, **kw):
        return d.reconstruct_ragged_resized_device(rects, self.ow, self.oh, self.channels, self.dev.data_ptr() + self.at, self.image, self.plane, self.row, **kw)

    def expect(self, slots):
        """slots[i]: (oh, ow, channels) array, or None for a slot that stays as it is"""
        want = np.full(self.size, 0xA5, np.uint8)
        for i, pic in enumerate(slots):
            if pic is None:
                continue
            assert pic.shape == (self.oh, self.ow, self.channels), (pic.shape, i)
            parts = [pic[:, :, c] for c in range(self.channels)] if self.planar else [pic.reshape(self.oh, self.line)]
            for c, part in enumerate(parts):
                o = self.at + i * self.image + c * self.plane
                for y in range(self.oh):
                    want[o + y * self.row:o + y * self.row + self.line] = part[y]
        return want

    def check(self, slots, what=""):
        got, want = self.dev.cpu().numpy(), self.expect(slots)
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        slot, inside = divmod(int(bad[0]) - self.at, self.image)
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at offset {bad[0]} (slot {slot}, byte {inside} of it; got {got[bad[0]]}, want {want[bad[0]]})")


@functools.lru_cache(maxsize=None)
def _pictures(oracle, streams):
    return tuple(_expected(oracle, s, 8) for s in streams)


_want_cache = {}


def _want(key, pic, rect, ow, oh, channels):
    """The model's answer for one slot (computed once per picture, rectangle and size; read-only)."""
    k = (key, rect, ow, oh, channels)
    if k not in _want_cache:
        x0, y0, x1, y1 = _clip(rect, pic.shape[1], pic.shape[0])
        r = M.resize(pic[y0:y1 + 1, x0:x1 + 1], ow, oh)
        if r.shape[2] == 1 and channels == 3:
            r = np.repeat(r, 3, axis=2)
        r.setflags(write=False)
        _want_cache[k] = r
    return _want_cache[k]


def _crop_kinds(w, h):
    """The rectangles of one picture, by kind; a picture too small for a kind gives its whole canvas"""
    return [WHOLE,
            (9, 10, 14, 13) if w > 14 and h > 13 else WHOLE,
            (120, 120, 135, 135) if w > 135 and h > 135 else WHOLE,
            (127, 0, 128, h - 1) if w > 128 else WHOLE,
            (w - 1, h - 1, w - 1, h - 1)]


# ------------------------------------------------------------------------------------------------ 1: layouts x crops x sizes
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_layouts_crops_sizes(oracle, layout, planar):
    """Whole pictures and four crops of 16 x 16 ... 300 x 270, to 32 x 32, 1 x 1, 37 x 5, 224 x 224 and to every crop's own size: many
    taps (300 -> 1), one source sample (1 -> 224), odd widths, tiles cut on every side.  The own size is the identity: the slot holds
    the crop call's bytes."""
    import torch

    streams = _layout_list(layout)
    pictures = _pictures(oracle, streams)
    n = len(streams)
    channels = 1 if layout == "grey" else 3
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(list(streams)) == [0] * n
        for kind in range(5):
            rects = [_crop_kinds(w, h)[kind] for w, h in SIZES]
            boxes = [_clip(r, w, h) for r, (w, h) in zip(rects, SIZES)]
            own = sorted({(b[2] - b[0] + 1, b[3] - b[1] + 1) for b in boxes})
            for j, (ow, oh) in enumerate([(32, 32), (1, 1), (37, 5), (224, 224)] + own):
                arena = BatchArena(n, ow, oh, channels, planar, base=kind + j)
                assert arena.call(d, rects) == [0] * n
                arena.check([_want((layout, i), pictures[i], rects[i], ow, oh, channels) for i in range(n)], what=f"{layout} kind {kind} -> {ow} x {oh}")
                st = d.ragged_resized_stats()
                assert st["images"] == st["resampled"] == n and st["refused"] == 0 and st["resample_launches"] == 1, st
                if j < 4:
                    continue
                # the identity: the crop call's own bytes
                same = [i for i, b in enumerate(boxes) if (b[2] - b[0] + 1, b[3] - b[1] + 1) == (ow, oh)]
                crops = [torch.zeros((oh, ow, channels), dtype=torch.uint8, device="cuda") if i in same else None for i in range(n)]
                d.reconstruct_ragged_rect_device(rects, [t.data_ptr() if t is not None else 0 for t in crops], [ow * channels] * n)
                got = arena.dev.cpu().numpy()
                for i in same:
                    slot = arena.expect([crops[k].cpu().numpy() if k == i else None for k in range(n)])
                    lines = slot != 0xA5
                    assert np.array_equal(got[lines], slot[lines]), (kind, i)
                    assert np.array_equal(crops[i].cpu().numpy(), pictures[i][boxes[i][1]:boxes[i][3] + 1, boxes[i][0]:boxes[i][2] + 1]), (kind, i)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 2: grey and colour in one list
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_grey_and_colour_in_one_list(oracle, planar):
    """channels=3: a grey picture fills three equal planes.  channels=1: the colour pictures get NOT_IMPLEMENTED and their slots stay
    as they are, the grey ones are right."""
    streams = tuple(_layout_list(layout)[k] for layout in LAYOUT_NAMES for k in (2, 4))
    pictures = _pictures(oracle, streams)
    n = len(streams)
    grey = [p.shape[2] == 1 for p in pictures]
    assert sum(grey) == 2
    rects = [(3, 5, 100, 38)] * n
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(list(streams)) == [0] * n
        arena = BatchArena(n, 40, 33, 3, planar, base=1)
        assert arena.call(d, rects) == [0] * n
        want = [_want(("mixed", i), pictures[i], rects[i], 40, 33, 3) for i in range(n)]
        assert all(np.array_equal(w[:, :, 0], w[:, :, 1]) and np.array_equal(w[:, :, 0], w[:, :, 2]) for w, g in zip(want, grey) if g)
        arena.check(want, what="channels 3")
        arena = BatchArena(n, 40, 33, 1, planar, base=2)
        assert arena.call(d, rects) == [0 if g else api.ERR_NOT_IMPLEMENTED for g in grey]
        arena.check([_want(("mixed", i), pictures[i], rects[i], 40, 33, 1) if g else None for i, g in enumerate(grey)], what="channels 1")
        st = d.ragged_resized_stats()
        assert st["images"] == n and st["resampled"] == 2 and st["refused"] == n - 2 and st["resample_launches"] == 1, st
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 3: what is refused, what rides along
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_refused_members_and_the_copy_route(oracle, planar):
    """A 12-bit picture in its layout group, a progressive one on a child object, CMYK and garbage beside two group members: the 8-bit
    progressive picture is served through the copy route, exactly; 12 bit and CMYK are NOT_IMPLEMENTED, garbage keeps its decode
    status; their slots and everything around the slots are untouched."""
    good = (_layout_list("420")[4], _layout_list("grey")[3])
    garbage = bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8))
    streams = [good[0], golden_jpeg("p12_120x90_420_dri3"), golden_jpeg("pilprog_200x130_422"), golden_jpeg("pil_90x60_cmyk"), garbage, good[1]]
    served = [0, 2, 5]
    pictures = {i: _expected(oracle, streams[i], 8) for i in served}
    n = len(streams)
    d = api.Decoder(0)
    try:
        decode = d.decode_ragged_device(streams, with_12bit=True)
        assert [s != 0 for s in decode] == [False, False, False, False, True, False]
        assert [d.ragged_route(i)[0] for i in (0, 1, 2, 3, 5)] == [True, True, False, False, True]
        rects = [(130, 129, EDGE, EDGE), WHOLE, (7, 9, 150, 100), WHOLE, WHOLE, (1, 1, 200, 38)]
        for k, (ow, oh) in enumerate([(64, 48), (224, 224)]):
            arena = BatchArena(n, ow, oh, 3, planar, base=k)
            status = arena.call(d, rects)
            assert status == [0, api.ERR_NOT_IMPLEMENTED, 0, api.ERR_NOT_IMPLEMENTED, decode[4], 0]
            arena.check([_want(("refused", i), pictures[i], rects[i], ow, oh, 3) if i in served else None for i in range(n)], what=f"{ow} x {oh}")
            st = d.ragged_resized_stats()
            assert st["images"] == n and st["resampled"] == 3 and st["refused"] == 3 and st["resample_launches"] == 1 and st["window_launches"] == 2, st
        # nobody served: nothing launched, nothing written
        arena = BatchArena(n, 8, 8, 1, planar)
        only_grey = [WHOLE] * n
        status = arena.call(d, only_grey)
        assert status[5] == 0 and status[0] == status[2] == api.ERR_NOT_IMPLEMENTED
        arena.check([None] * 5 + [_want(("refused", 5), pictures[5], WHOLE, 8, 8, 1)], what="the grey picture alone")
        d2 = api.Decoder(0)
        try:
            d2.decode_ragged_device(streams[1:5], with_12bit=True)
            arena = BatchArena(4, 8, 8, 1, planar)
            assert all(s != 0 for s in arena.call(d2, None))
            arena.check([None] * 4, what="nobody served")
            st = d2.ragged_resized_stats()
            assert st == dict(images=4, resampled=0, refused=4, window_launches=0, resample_launches=0, arena_bytes=0), st
        finally:
            d2.close()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 4: launches
@pytest.mark.gpu
def test_one_resample_launch_for_any_list(oracle):
    """resample_launches == 1 for lists of 3 and of 15 pictures; window_launches is what the crop call reports for the same rectangles;
    the crop call's own statistics stay the last crop call's."""
    import torch

    all15 = tuple(s for layout in ("420", "444", "grey") for s in _layout_list(layout))
    for streams in (all15[:3], all15):
        n = len(streams)
        pictures = _pictures(oracle, streams)
        d = api.Decoder(0)
        try:
            assert d.decode_ragged_device(list(streams)) == [0] * n
            infos = [d.ragged_info(i) for i in range(n)]
            rects = [(f.width // 4, f.height // 5, f.width - 2, f.height - 1) for f in infos]
            bufs = [torch.empty((f.height, f.width, f.components), dtype=torch.uint8, device="cuda") for f in infos]
            d.reconstruct_ragged_rect_device(rects, [b.data_ptr() for b in bufs], [f.width * f.components for f in infos])
            crop_stats = d.ragged_rect_stats()
            assert crop_stats["launches"] >= 1 and crop_stats["fused"] == n
            arena = BatchArena(n, 48, 40, 3, True, base=3)
            assert arena.call(d, rects) == [0] * n
            arena.check([_want(("launches", n, i), pictures[i], rects[i], 48, 40, 3) for i in range(n)], what=f"{n} pictures")
            st = d.ragged_resized_stats()
            assert st["resample_launches"] == 1 and st["window_launches"] == crop_stats["launches"] and st["resampled"] == n, (st, crop_stats)
            clipped = [_clip(r, f.width, f.height) for r, f in zip(rects, infos)]
            assert st["arena_bytes"] == sum(((b[2] - b[0] + 1) * (b[3] - b[1] + 1) * f.components + 15) // 16 * 16 for b, f in zip(clipped, infos))
            assert d.ragged_rect_stats() == crop_stats
        finally:
            d.close()


# ------------------------------------------------------------------------------------------------ 5: two calls in flight
@pytest.mark.gpu
def test_two_calls_without_sync(oracle):
    """Two calls with sync=0 back to back on one decode -- other rectangles, other sizes, other tensors -- and one wait: both exact, so
    the first call's pinned tables were not overwritten on their way up, nor its crops in the arena before they were read."""
    streams = _layout_list("420")
    pictures = _pictures(oracle, streams)
    n = len(streams)
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(list(streams)) == [0] * n
        first = [WHOLE] * n
        second = [(w // 3, h // 2, w - 1, h - 2) if h > 2 else WHOLE for w, h in SIZES]
        a1, a2 = BatchArena(n, 224, 224, 3, True, base=1), BatchArena(n, 31, 45, 3, False, base=2)
        api._foreign_work_done()  # (the arenas' fills: the calls below do not wait for other streams)
        assert a1.call(d, first, sync=False, wait_foreign=False) == [0] * n
        assert a2.call(d, second, sync=False, wait_foreign=False) == [0] * n
        d.synchronize()
        a1.check([_want(("420", i), pictures[i], first[i], 224, 224, 3) for i in range(n)], what="first call")
        a2.check([_want(("420", i), pictures[i], second[i], 31, 45, 3) for i in range(n)], what="second call")
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 6: parameter errors
@pytest.mark.gpu
def test_parameter_errors_write_and_count_nothing(oracle):
    streams = _layout_list("444")
    n = len(streams)
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(list(streams)) == [0] * n
        arena = BatchArena(n, 20, 10, 3, True)
        ptr, fn = arena.dev.data_ptr() + arena.at, api.lib().mijpeg_reconstruct_ragged_resized_device
        good = dict(rects=None, ow=20, oh=10, channels=3, dst=ptr, image=arena.image, plane=arena.plane, row=arena.row)
        line, plane = 20, 9 * arena.row + 20
        cases = {"out_width 0": dict(ow=0), "out_height 0": dict(oh=0), "out_width -3": dict(ow=-3), "channels 2": dict(channels=2), "channels 4": dict(channels=4),
                 "channels 0": dict(channels=0), "NULL dst": dict(dst=None), "row below a line": dict(row=line - 1),
                 "plane below its lines": dict(plane=plane - 1), "negative plane": dict(plane=-arena.plane),
                 "image below its planes": dict(image=2 * arena.plane + plane - 1),
                 "interleaved: row below a line": dict(plane=0, row=59), "interleaved: image below its lines": dict(plane=0, row=60, image=9 * 60 + 59),
                 "min > max": dict(rects=[WHOLE] * 2 + [(10, 2, 9, 5)] + [WHOLE] * 2), "min beyond": dict(rects=[(16, 0, 20, 5)] + [WHOLE] * 4),
                 "negative min": dict(rects=[WHOLE] * 4 + [(0, -1, 5, 5)])}
        for name, change in cases.items():
            a = dict(good, **change)
            status = (C.c_int32 * n)(*[77] * n)
            rc = fn(d._h, api.rect_array(a["rects"]) if a["rects"] else None, a["ow"], a["oh"], a["channels"], a["dst"], a["image"], a["plane"], a["row"], 0, status, 1)
            assert rc == api.ERR_INVALID_PARAMETER, name
            assert list(status) == [77] * n, name
            arena.check([None] * n, what=name)
            assert d.ragged_resized_stats() == STATS0, name
        assert fn(None, None, 20, 10, 3, ptr, arena.image, arena.plane, arena.row, 0, None, 1) == api.ERR_INVALID_PARAMETER
        # the same arguments unchanged are served, status == NULL included
        assert fn(d._h, None, 20, 10, 3, ptr, arena.image, arena.plane, arena.row, 0, None, 1) == 0
        assert d.ragged_resized_stats()["resampled"] == n
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 7: batch.decode_resized
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_decode_resized(oracle, layout):
    from libjpeg_amd import batch

    garbage = bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8))
    streams = [_layout_list("420")[4], _layout_list("grey")[2], garbage, _layout_list("444")[3], _layout_list("422")[1], golden_jpeg("pil_90x60_cmyk")]
    crops = [(10, 20, 224, 224), None, None, (128, 3, 500, 500), (5, 5, 50, 40), None]  # (x, y, w, h)
    served = [0, 1, 3, 4]
    pictures = {i: _expected(oracle, streams[i], 8) for i in served}

    def want(i, h, w):
        c = crops[i] or (0, 0, EDGE, EDGE)
        r = _want(("resized", i), pictures[i], (c[0], c[1], min(EDGE, c[0] + c[2] - 1), min(EDGE, c[1] + c[3] - 1)), w, h, 3)
        return r.transpose(2, 0, 1) if layout == "chw" else r

    d = api.Decoder(0)
    try:
        out, errors = batch.decode_resized(streams, (48, 56), crops=crops, layout=layout, decoder=d)
        assert tuple(out.shape) == ((6, 3, 48, 56) if layout == "chw" else (6, 48, 56, 3)) and out.dtype.itemsize == 1
        got = out.cpu().numpy()
        for i in range(6):
            if i in served:
                assert errors[i] is None and np.array_equal(got[i], want(i, 48, 56)), i
            else:
                assert isinstance(errors[i], api.MijpegError) and not got[i].any(), i
        assert errors[5].code == api.ERR_NOT_IMPLEMENTED and errors[2].code not in (0, api.ERR_NOT_IMPLEMENTED)
        assert d.ragged_resized_stats()["resample_launches"] == 1
        # world = 2, rank 1: pictures 1, 3, 5 in slots 0, 1, 2; the other rank's crops are not this rank's
        part, perr = batch.decode_resized(streams, (48, 56), crops=[(999, 0, 1, 1)] + crops[1:], layout=layout, rank=1, world=2, decoder=d)
        assert part.shape[0] == 3 and [e is None for e in perr] == [True, True, False]
        assert np.array_equal(part.cpu().numpy()[:2], got[[1, 3]])
        # without crops, one channel: the grey picture alone
        grey, gerr = batch.decode_resized(streams, (9, 300), channels=1, layout=layout)
        assert tuple(grey.shape) == ((6, 1, 9, 300) if layout == "chw" else (6, 9, 300, 1))
        assert [e is None for e in gerr] == [False, True, False, False, False, False]
        exp = M.resize(pictures[1], 300, 9)
        assert np.array_equal(grey.cpu().numpy()[1], exp.transpose(2, 0, 1) if layout == "chw" else exp)
        before = d.ragged_resized_stats()
        for bad in [dict(size=(0, 5)), dict(size=(5,)), dict(channels=2), dict(layout="nchw"), dict(crops=crops[:3]), dict(crops=[(300, 0, 5, 5)] + crops[1:])]:
            with pytest.raises(ValueError):
                batch.decode_resized(streams, **dict(dict(size=(8, 8), layout=layout, decoder=d), **bad))
        assert d.ragged_resized_stats() == before
    finally:
        d.close()

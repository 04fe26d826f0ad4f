"""Crop windows of a ragged batch (mijpeg_reconstruct_ragged_rect_device / ..._rect_planar_device, decode_mixed(crops=...); DESIGN
4.1e): the window flavours of the 8-bit ragged kernels run only the tiles a picture's window touches and write only its pixels.

Every crop is compared, at tolerance 0, with that rectangle of the oracle's decode of the same stream.  The kernels address a
destination from a BIASED base -- where canvas pixel (0, 0) would lie -- so every call writes into one arena filled with 0xA5 in which
each destination has 64 guard bytes in front and behind, line padding and a base at byte offset 0..3, and the WHOLE arena is compared
with what it must hold afterwards: the crops' bytes and 0xA5 everywhere else.  One decode per list serves all its crop calls; the
pictures are at most 300 x 270 (3 x 3 tiles of 128 x 128)."""
import functools

import numpy as np
import pytest

from conftest import golden_jpeg
from libjpeg_amd import api, synth
from test_ragged_batch import _encode, _flavour
from test_ragged_gates import _expected, _list8

GUARD = 64
EDGE = 2**31 - 1
SIZES = [(16, 16), (128, 128), (129, 131), (257, 40), (300, 270)]
LAYOUT_NAMES = ["420", "422", "444", "grey"]


# ------------------------------------------------------------------------------------------------ the crops of the issue
def _crops(w, h):
    """(min_x, min_y, max_x, max_y) as a caller passes them, where a w x h picture has them."""
    out = [(0, 0, w - 1, h - 1), (0, 0, EDGE, EDGE), (0, 0, 0, 0), (w - 1, h - 1, w - 1, h - 1)]
    if w > 127 and h > 127:
        out.append((127, 127, 127, 127))
    if w > 128 and h > 128:
        out.append((128, 128, 128, 128))
    if w > 14 and h > 13:
        out.append((9, 10, 14, 13))  # inside one block
    for r in range(8):  # every left / right / top / bottom residue
        c = (r, r, w - 1 - (3 * r) % 8, h - 1 - (5 * r) % 8)
        if c[0] <= c[2] and c[1] <= c[3]:
            out.append(c)
    if w > 135 and h > 135:
        out.append((120, 120, 135, 135))  # across the tile seams
    if w > 128:
        out.append((127, 0, 128, h - 1))
    if h > 32:
        out.append((0, 31, w - 1, 32))  # across the wave seam inside a tile
    if (w, h) == (300, 270):
        out.append((130, 129, w - 1, h - 1))  # a window without tile column 0 and tile row 0
    return out


def _clip(rect, w, h):
    return rect[0], rect[1], min(rect[2], w - 1), min(rect[3], h - 1)


def _tiles(rect, w, h):
    x0, y0, x1, y1 = _clip(rect, w, h)
    return ((x1 >> 7) - (x0 >> 7) + 1) * ((y1 >> 7) - (y0 >> 7) + 1)


@functools.lru_cache(maxsize=None)
def _layout_list(layout):
    return tuple(_encode(w, h, 5100 + 10 * LAYOUT_NAMES.index(layout) + k, (85, 95, 50, 90, 75)[k], layout, 1 + k % 4, k % 2 == 1) for k, (w, h) in enumerate(SIZES))


# ------------------------------------------------------------------------------------------------ one guarded call
class Arena:
    """The destinations of one crop call in one device tensor of 0xA5: per picture (per plane) GUARD bytes, the crop's lines `row` bytes
    apart -- the last one padded too --, GUARD bytes; bases at byte offsets 0..3.  expect(): the arena as it must look afterwards."""

    def __init__(self, infos, rects, planar, pad, salt=0):
        import torch

        self.items, at = [], 0
        for i, (f, r) in enumerate(zip(infos, rects)):
            if f is None or r is None:
                self.items.append(None)
                continue
            x0, y0, x1, y1 = _clip(r, f.width, f.height)
            cw, ch, sb = x1 - x0 + 1, y1 - y0 + 1, max(1, f.sample_bytes)
            planes = f.components if planar else 1
            line = cw * sb * (1 if planar else f.components)
            row = line + pad
            offs = []
            for _ in range(planes):
                at = (at + 3) // 4 * 4 + (i + salt + len(offs)) % 4
                offs.append(at + GUARD)
                at += GUARD + ch * row + GUARD
            self.items.append(dict(offs=offs, row=row, line=line, ch=ch, cw=cw, box=(x0, y0, x1, y1), sb=sb))
        self.size = at + 4
        self.dev = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda")
        self.planar = planar

    def ptrs(self):
        base = self.dev.data_ptr()
        if self.planar:
            return [[base + o for o in it["offs"]] if it else None for it in self.items]
        return [base + it["offs"][0] if it else 0 for it in self.items]

    def rows(self):
        return [it["row"] if it else 0 for it in self.items]

    def expect(self, pictures, only=None):
        """pictures[i]: (h, w, c) array of the whole picture; only: the indices that were written (default: all with a destination)"""
        want = np.full(self.size, 0xA5, np.uint8)
        for i, it in enumerate(self.items):
            if it is None or (only is not None and i not in only):
                continue
            x0, y0, x1, y1 = it["box"]
            crop = np.ascontiguousarray(pictures[i][y0:y1 + 1, x0:x1 + 1])
            for k, o in enumerate(it["offs"]):
                part = np.ascontiguousarray(crop[:, :, k]) if self.planar else crop
                lines = part.view(np.uint8).reshape(it["ch"], it["line"])
                for y in range(it["ch"]):
                    want[o + y * it["row"]:o + y * it["row"] + it["line"]] = lines[y]
        return want

    def check(self, pictures, only=None, what=""):
        got, want = self.dev.cpu().numpy(), self.expect(pictures, only)
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        owner = [(i, it["box"]) for i, it in enumerate(self.items) if it and any(o - GUARD <= bad[0] < o + it["ch"] * it["row"] + GUARD for o in it["offs"])]
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at arena offset {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]}); destination {owner}")


def _call(d, arena, rects, planar, flags=0):
    rects = [r if r is not None else (0, 0, 0, 0) for r in rects]
    if planar:
        d.reconstruct_ragged_rect_planar_device(rects, arena.ptrs(), arena.rows(), flags)
    else:
        d.reconstruct_ragged_rect_device(rects, arena.ptrs(), arena.rows(), flags)
    return d.ragged_rect_stats()


def _oracle_pictures(oracle, streams, precisions=None):
    return [_expected(oracle, s, p) for s, p in zip(streams, precisions or [8] * len(streams))]


# ------------------------------------------------------------------------------------------------ layouts x sizes x crops
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_layouts_sizes_crops(oracle, layout, planar):
    """Every crop of _crops on 16 x 16, 128 x 128, 129 x 131, 257 x 40 and 300 x 270 in one list per layout: round j is ONE call with
    the j-th crop of every picture that has one, tight lines and lines padded by 5 bytes.  The statistics: all pictures by a window
    launch, one launch, the planner's tile count; a single-pixel round runs one workgroup per picture, the whole-picture rounds all."""
    streams = list(_layout_list(layout))
    pictures = _oracle_pictures(oracle, streams)
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(streams) == [0] * len(streams)
        infos = [d.ragged_info(i) for i in range(len(streams))]
        assert [(f.width, f.height) for f in infos] == SIZES
        per_picture = [_crops(w, h) for w, h in SIZES]
        full = sum(((w + 127) // 128) * ((h + 127) // 128) for w, h in SIZES)
        for j in range(max(len(c) for c in per_picture)):
            rects = [c[j] if j < len(c) else None for c in per_picture]
            n = sum(r is not None for r in rects)
            tiles = sum(_tiles(r, w, h) for r, (w, h) in zip(rects, SIZES) if r is not None)
            planned = api.ragged_rect_plan([f for f, r in zip(infos, rects) if r is not None], [r for r in rects if r is not None])
            assert sum(a * b for a, b in zip(planned[2], planned[3])) == tiles
            for pad in (0, 5):
                arena = Arena(infos, rects, planar, pad, salt=j)
                st = _call(d, arena, rects, planar)
                arena.check(pictures, what=f"{layout} round {j} {rects} pad {pad}")
                flavours = {_flavour(f) for f, r in zip(infos, rects) if r is not None}  # (what shares a launch inside a group)
                assert st["images"] == n and st["fused"] == n and st["copied"] == 0 and st["launches"] == len(flavours), (j, st)
                assert st["workgroups"] == tiles, (j, st)
                assert st["workgroups_full"] == sum(((w + 127) // 128) * ((h + 127) // 128) for r, (w, h) in zip(rects, SIZES) if r is not None)
                if j in (0, 1):  # the whole picture, exact bounds and INT32_MAX
                    assert st["workgroups"] == st["workgroups_full"] == full
                if j in (2, 3):  # single pixels
                    assert st["workgroups"] == st["fused"] == len(streams)
        # the window without tile column 0 and tile row 0 on 300 x 270: 4 of its 9 tiles
        rects = [None] * 4 + [(130, 129, 299, 269)]
        arena = Arena(infos, rects, planar, 5)
        st = _call(d, arena, rects, planar)
        arena.check(pictures, what="no tile column 0")
        assert st["workgroups"] == 4 and st["workgroups_full"] == 9 and st["workgroups"] < st["workgroups_full"]
    finally:
        d.close()


@pytest.mark.gpu
def test_full_window_equals_the_full_calls(oracle):
    """A rect that covers the picture gives the existing calls' bytes, interleaved and planar."""
    import torch

    streams = [s for layout in LAYOUT_NAMES for s in _layout_list(layout)[2:]]
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(streams) == [0] * len(streams)
        infos = [d.ragged_info(i) for i in range(len(streams))]
        rects = [(0, 0, EDGE, EDGE)] * len(streams)
        for planar in (False, True):
            full = Arena(infos, rects, planar, 3)
            if planar:
                d.reconstruct_ragged_planar_device(full.ptrs(), full.rows())
            else:
                d.reconstruct_ragged_device(full.ptrs(), full.rows())
            crop = Arena(infos, rects, planar, 3)
            st = _call(d, crop, rects, planar)
            assert torch.equal(full.dev, crop.dev)
            assert st["workgroups"] == st["workgroups_full"] and st["copied"] == 0 and st["launches"] == len({_flavour(f) for f in infos})
            crop.check(_oracle_pictures(oracle, streams), what="full window")
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ every arithmetic flavour
def _seam_crop(w, h):
    """Left / top residues 3 and 5, across the tile seam at 128 where the picture has one."""
    x0 = 123 if w > 128 else min(3, w - 1)
    y0 = 125 if h > 128 else min(5, h - 1)
    return x0, y0, min(w - 1, x0 + 20), min(h - 1, y0 + 20)


@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_every_arithmetic_flavour(oracle, planar):
    """The list of test_ragged_gates (packed, FAST and SAFE 4:2:0, packed and WIDE 4:2:2, 4:4:4 and grey at their gates, two frames one
    step beyond): one crop per member.  As many window launches as the full call makes launches; the members with a ragged flavour by
    a window launch, the two without by the copy route."""
    members = _list8()
    streams = [mb.stream for mb in members]
    pictures = _oracle_pictures(oracle, streams)
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(streams) == [0] * len(members)
        infos = [d.ragged_info(i) for i in range(len(members))]
        whole = Arena(infos, [(0, 0, EDGE, EDGE)] * len(members), False, 0)
        d.reconstruct_ragged_device(whole.ptrs(), whole.rows())
        full_stats = d.ragged_stats()
        rects = [_seam_crop(mb.w, mb.h) for mb in members]
        assert any(r[0] < 128 <= r[2] for r in rects) and any(r[1] < 128 <= r[3] for r in rects)
        arena = Arena(infos, rects, planar, 5)
        st = _call(d, arena, rects, planar)
        arena.check(pictures, what="gates")
        ragged = sum(mb.ragged for mb in members)
        assert st["launches"] == full_stats["recon_launches"] == 7, (st, full_stats)
        assert st["fused"] == ragged == 28 and st["copied"] == len(members) - ragged == 2 and st["images"] == len(members), st
        assert st["workgroups"] == sum(_tiles(r, mb.w, mb.h) for r, mb in zip(rects, members) if mb.ragged)
        assert d.ragged_stats() == full_stats  # (the crop calls have statistics of their own)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ fallback members
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("with_12bit", [False, True], ids=["8bit-groups", "12bit-groups"])
def test_fallback_members(oracle, with_12bit, planar):
    """Group members beside a progressive, a 12-bit, a 4:4:0, a CMYK and a JPEG XT stream: every crop is that rectangle of the full
    call's picture (and of the oracle's), `copied` counts exactly the members without a window flavour."""
    good = [_encode(300, 270, 5201, 85, "420", 3, False), _encode(129, 131, 5202, 90, "444", 0, True), _encode(257, 40, 5203, 75, "grey", 2, False)]
    p12 = golden_jpeg("p12_120x90_420_dri3")
    xt = golden_jpeg("xt_129x71_420")
    streams = [good[0], synth.synth_jpeg(200, 130, 3, 85, "420", 0, progressive=True), p12, good[1], golden_jpeg("ref_97x61_440"), golden_jpeg("pil_90x60_cmyk"), xt, good[2]]
    kinds = ["good", "progressive", "p12", "good", "440", "cmyk", "xt", "good"]
    n = len(streams)
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(streams, with_12bit=with_12bit) == [0] * n
        infos = [d.ragged_info(i) for i in range(n)]
        in_group = [d.ragged_route(i)[0] for i in range(n)]
        assert in_group == [k == "good" or (k == "p12" and with_12bit) for k in kinds]
        # the full pictures, as the existing call writes them
        everything = [(0, 0, EDGE, EDGE)] * n
        whole = Arena(infos, everything, False, 0)
        d.reconstruct_ragged_device(whole.ptrs(), whole.rows())
        flat = whole.dev.cpu().numpy()
        pictures = []
        for f, it in zip(infos, whole.items):
            body = flat[it["offs"][0]:it["offs"][0] + it["ch"] * it["row"]].reshape(it["ch"], it["row"])
            pictures.append(body.view("<u2" if it["sb"] == 2 else np.uint8).reshape(f.height, f.width, f.components))
        for i, k in enumerate(kinds):
            if k == "xt":
                exp = np.asarray(oracle.decode_xt(streams[i])[0])
                assert exp.dtype.itemsize == 2 and np.array_equal(pictures[i].view(exp.dtype), exp)
            else:
                assert np.array_equal(pictures[i], _expected(oracle, streams[i], 12 if k == "p12" else 8)), k
        rects = [(f.width // 3 + 1, f.height // 4 + 3, f.width - 4, f.height - 2) for f in infos]
        rects[0] = (130, 129, EDGE, EDGE)
        for pad in (0, 6):  # (even: 16-bit samples stay aligned)
            arena = Arena(infos, rects, planar, pad)
            st = _call(d, arena, rects, planar)
            arena.check(pictures, what=f"fallbacks pad {pad}")
            assert st == dict(images=n, fused=3, copied=n - 3, launches=3, workgroups=4 + _tiles(rects[3], 129, 131) + _tiles(rects[7], 257, 40),
                              workgroups_full=9 + 4 + 3), st
        # the copy route alone, and a call that skips pictures
        rects2 = [None, rects[1], None, None, None, rects[5], None, None]
        arena = Arena(infos, rects2, planar, 2)
        st = _call(d, arena, rects2, planar)
        arena.check(pictures, what="copies alone")
        assert st == dict(images=2, fused=0, copied=2, launches=0, workgroups=0, workgroups_full=0), st
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_refusals_write_nothing(oracle, planar):
    """min > max, a negative min, min beyond the picture, a stride below the crop's line, NULL rects: MIJPEG_ERR_INVALID_PARAMETER, not
    a byte of any destination changed -- the good pictures of the same call included -- and the previous call's statistics stay."""
    import ctypes as C

    streams = list(_layout_list("420"))
    pictures = _oracle_pictures(oracle, streams)
    d = api.Decoder(0)
    try:
        assert d.decode_ragged_device(streams) == [0] * len(streams)
        infos = [d.ragged_info(i) for i in range(len(streams))]
        good = [(1, 2, w - 2, h - 3) for w, h in SIZES]
        arena = Arena(infos, good, planar, 5)
        before = _call(d, arena, good, planar)
        arena.check(pictures, what="the good call")
        assert before["fused"] == len(streams)
        cases = {"min > max (x)": (4, (10, 2, 9, 5)), "min > max (y)": (4, (1, 6, 9, 5)), "negative min_x": (2, (-1, 0, 5, 5)), "negative min_y": (2, (0, -1, 5, 5)),
                 "min_x beyond": (0, (16, 0, 20, 5)), "min_y beyond": (3, (0, 40, 5, 45)), "max below 0": (1, (0, 0, -1, -1))}
        for name, (i, bad) in cases.items():
            rects = list(good)
            rects[i] = bad
            layout = list(good)
            layout[i] = (0, 0, 3, 3)  # (what the destination is sized for)
            arena = Arena(infos, layout, planar, 5)
            with pytest.raises(api.MijpegError) as e:
                if planar:
                    d.reconstruct_ragged_rect_planar_device(rects, arena.ptrs(), arena.rows())
                else:
                    d.reconstruct_ragged_rect_device(rects, arena.ptrs(), arena.rows())
            assert e.value.code == api.ERR_INVALID_PARAMETER, name
            arena.check(pictures, only=set(), what=name)
            assert d.ragged_rect_stats() == before, name
        # a stride one byte below the crop's line
        arena = Arena(infos, good, planar, 5)
        rows = arena.rows()
        rows[2] = arena.items[2]["line"] - 1
        with pytest.raises(api.MijpegError) as e:
            if planar:
                d.reconstruct_ragged_rect_planar_device(good, arena.ptrs(), rows)
            else:
                d.reconstruct_ragged_rect_device(good, arena.ptrs(), rows)
        assert e.value.code == api.ERR_INVALID_PARAMETER
        arena.check(pictures, only=set(), what="stride")
        # NULL rects
        n = len(streams)
        ptrs = arena.ptrs()
        if planar:
            dst = (C.c_void_p * (4 * n))(*[q for p in ptrs for q in list(p) + [None] * (4 - len(p))])
            fn = api.lib().mijpeg_reconstruct_ragged_rect_planar_device
        else:
            dst = (C.c_void_p * n)(*ptrs)
            fn = api.lib().mijpeg_reconstruct_ragged_rect_device
        assert fn(d._h, None, dst, (C.c_int64 * n)(*arena.rows()), 0, 1) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, api.rect_array(good), None, (C.c_int64 * n)(*arena.rows()), 0, 1) == api.ERR_INVALID_PARAMETER
        assert fn(d._h, api.rect_array(good), dst, None, 0, 1) == api.ERR_INVALID_PARAMETER
        arena.check(pictures, only=set(), what="NULL lists")
        assert d.ragged_rect_stats() == before
        if planar:  # a NULL plane of a component the picture has
            ptrs[1] = [ptrs[1][0], None, ptrs[1][2]]
            with pytest.raises(api.MijpegError) as e:
                d.reconstruct_ragged_rect_planar_device(good, ptrs, arena.rows())
            assert e.value.code == api.ERR_INVALID_PARAMETER
            arena.check(pictures, only=set(), what="NULL plane")
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ decode_mixed(crops=...)
MIXED_CROPS = [(10, 20, 224, 224), None, (0, 0, 1, 1), (128, 3, 500, 500), (5, 5, 50, 40), (3, 100, 120, 9)]


def _mixed_streams():
    shapes = [(300, 270, "420"), (129, 131, "444"), (257, 40, "422"), (300, 270, "grey"), (16, 16, "420")]
    streams = [_encode(w, h, 5300 + k, 85, layout, 1 + k % 3, False) for k, (w, h, layout) in enumerate(shapes)]
    return streams + [synth.synth_jpeg(200, 130, 3, 85, "420", 0, progressive=True)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_decode_mixed_crops(oracle, layout):
    from libjpeg_amd import batch

    streams = _mixed_streams()
    pictures = _oracle_pictures(oracle, streams)
    d = api.Decoder(0)
    try:
        whole = batch.decode_mixed(streams, 0, decoder=d, layout=layout)
        out = batch.decode_mixed(streams, 0, decoder=d, layout=layout, crops=MIXED_CROPS)
        st = d.ragged_rect_stats()
        assert st["images"] == 6 and st["fused"] == 5 and st["copied"] == 1 and st["workgroups"] < st["workgroups_full"], st
        for i, (t, c, pic) in enumerate(zip(out, MIXED_CROPS, pictures)):
            x, y, w, h = c or (0, 0, pic.shape[1], pic.shape[0])
            exp = pic[y:y + h, x:x + w]  # (numpy clips as the library does)
            assert exp.size > 0
            if layout == "chw":
                assert tuple(t.shape) == (exp.shape[2],) + exp.shape[:2], (i, t.shape)
                assert np.array_equal(t.cpu().numpy(), exp.transpose(2, 0, 1)), i
                assert np.array_equal(t.cpu().numpy(), whole[i][:, y:y + h, x:x + w].cpu().numpy()), i
            else:
                assert tuple(t.shape) == exp.shape, (i, t.shape)
                assert np.array_equal(t.cpu().numpy(), exp), i
                assert np.array_equal(t.cpu().numpy(), whole[i][y:y + h, x:x + w].cpu().numpy()), i
        # world = 2: rank r gets pictures r, r + 2, ... and nothing else; a bad crop of the OTHER rank's picture is not this rank's
        for rank in (0, 1):
            part = batch.decode_mixed(streams, 0, rank, 2, decoder=d, layout=layout, crops=MIXED_CROPS)
            for i, t in enumerate(part):
                assert (t is None) == (i % 2 != rank)
                if t is not None:
                    assert np.array_equal(t.cpu().numpy(), out[i].cpu().numpy()), i
        # bad crops: ValueError, and the decoder object has not been asked for anything (its statistics are the last call's)
        before = (d.ragged_stats(), d.ragged_rect_stats())
        for bad in [(0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -2, 5, 5), (300, 0, 5, 5), (0, 270, 5, 5), (1, 2, 3), "abcd", (1, 0, 2**31, 1)]:
            with pytest.raises(ValueError):
                batch.decode_mixed(streams, 0, decoder=d, layout=layout, crops=[bad] + MIXED_CROPS[1:])
        with pytest.raises(ValueError):
            batch.decode_mixed(streams, 0, decoder=d, layout=layout, crops=MIXED_CROPS[:3])
        assert (d.ragged_stats(), d.ragged_rect_stats()) == before
    finally:
        d.close()


@pytest.mark.gpu
def test_decode_mixed_crops_with_12bit_and_device_markers(oracle):
    from libjpeg_amd import batch

    streams = _mixed_streams()[:3] + [golden_jpeg("p12_120x90_420_dri3")]
    crops = [(100, 100, 150, 150), (1, 1, 127, 127), None, (7, 9, 100, 50)]
    pictures = _oracle_pictures(oracle, streams, [8, 8, 8, 12])
    for kw in (dict(with_12bit=True), dict(device_markers=True), dict(with_12bit=True, device_markers=True, layout="chw")):
        out = batch.decode_mixed(streams, 0, crops=crops, **kw)
        for i, (t, c, pic) in enumerate(zip(out, crops, pictures)):
            x, y, w, h = c or (0, 0, pic.shape[1], pic.shape[0])
            exp = pic[y:y + h, x:x + w]
            got = t.cpu().numpy()
            if kw.get("layout") == "chw":
                exp = exp.transpose(2, 0, 1)
            assert got.shape == exp.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)), (kw, i)

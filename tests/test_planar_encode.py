"""Planar (CHW) input for the ragged encode on the device (mijpeg_encode_ragged_planar_device16, mijpeg_interleave_device,
libjpeg_amd.batch.encode_mixed(layout="chw")): every stream byte for byte against the interleaved encoder
(mijpeg_encode_ragged_device16, pinned to the reference encoder) on the HWC copy of the same samples -- the planar-input flavours of
the three forward kernel families, the byte-wise route of planes off their dword boundaries, the two-pass route of 12-bit pictures,
one-component pictures as their own plane --, the routes and launch counts the call reports, pass cutting, the failure behaviour
and the interleave kernel on its own.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import planar_encode_util as PU
from libjpeg_amd import api, batch

pytestmark = pytest.mark.gpu

LAYOUTS = dict(api.ENCODE_LAYOUTS)
LAYOUTS["3x3"] = ((3, 1, 1), (3, 1, 1))  # (the 3x factors have no name there)


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _torch():
    import torch

    return torch


def _dev(a: np.ndarray):
    """A numpy array in HBM (uint16 samples as int16: the same bits)."""
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda()


def _precisions(pics):
    return [12 if p.dtype == np.uint16 else 8 for p in pics]


def _sampling(p, layout):
    return LAYOUTS[layout] if p.shape[0] == 3 else ((1, 1, 1), (1, 1, 1))


def _interleaved(dec, pics, cases, optimize):
    """The reference: mijpeg_encode_ragged_device16 on the HWC copy of every (C, H, W) picture."""
    keep = [_dev(p.transpose(1, 2, 0)) for p in pics]
    frames = [api.encode_frame(p.shape[2], p.shape[1], p.shape[0], q, _sampling(p, lay), ri, t.data_ptr(), p.shape[2] * p.shape[0] * p.itemsize)
              for p, t, (lay, q, ri) in zip(pics, keep, cases)]
    out = dec.encode_ragged_device(frames, optimize, precision=_precisions(pics))
    del keep
    return out, dec.encode_ragged_stats()


def _place(p, how="aligned", fill=None, pad=0, gap=0):
    """The planes of a (C, H, W) picture somewhere in HBM -> (what keeps them alive, plane addresses, pitch in bytes).
    aligned: one allocation, the pitch the next multiple of 4 (plus `pad`), `gap` bytes between planes (a multiple of 4 keeps them
    aligned); offsets: plane c starts c + 1 bytes off a dword boundary; oddpitch: an odd pitch; reversed: plane 2 first in memory;
    separate: an allocation per plane.  fill: seed of the random bytes in line padding and gaps (None: zeros).  8-bit pictures,
    but `aligned`, which also takes 16-bit samples."""
    torch = _torch()
    nc, h, w = p.shape
    sb = p.itemsize
    line = w * sb
    pitch = {"oddpitch": line | 1}.get(how, (line + 3) & ~3) + pad
    plane_bytes = h * pitch + gap
    order = list(range(nc))[::-1] if how == "reversed" else list(range(nc))
    starts, at = {}, 0
    for c in order:
        at = (at + 3) & ~3
        if how == "offsets":
            at += (c % 3) + 1
        starts[c] = at
        at += plane_bytes
    host = np.zeros(at + 8, np.uint8) if fill is None else np.random.default_rng(fill).integers(0, 256, at + 8, dtype=np.uint8)
    raw = np.ascontiguousarray(p).view(np.uint8).reshape(nc, h, line)
    for c in range(nc):
        rows = host[starts[c]:starts[c] + h * pitch].reshape(h, pitch)
        rows[:, :line] = raw[c]
    if how == "separate":
        keep = [torch.from_numpy(host[starts[c]:starts[c] + plane_bytes].copy()).cuda() for c in range(nc)]
        return keep, [t.data_ptr() for t in keep], pitch
    buf = torch.from_numpy(host).cuda()
    return buf, [buf.data_ptr() + starts[c] for c in range(nc)], pitch


def _planar(dec, pics, cases, optimize, how="aligned", **place):
    placed = [_place(p, how if p.shape[0] == 3 and p.itemsize == 1 else "aligned", **place) for p in pics]
    frames = [api.encode_frame(p.shape[2], p.shape[1], p.shape[0], q, _sampling(p, lay), ri, 0, pitch) for p, (_, _, pitch), (lay, q, ri) in zip(pics, placed, cases)]
    out = dec.encode_ragged_planar_device(frames, [ptrs for _, ptrs, _ in placed], optimize, _precisions(pics))
    del placed
    return out, dec.encode_ragged_stats(), dec.encode_planar_stats()


# (width, height, layout): every kernel family of the planar flavours -- one tile and nothing else; a tile plus partial strips; tiles
# plus a strip of whole blocks (interior <2,2> and <1,1> behind the tile kernel); below the tile; the other layouts' interior kernels
SHAPES = [(128, 128, "420"), (130, 200, "420"), (256, 144, "420"), (64, 64, "420"), (100, 60, "420"), (641, 361, "420"), (24, 40, "444"), (333, 257, "444"),
          (48, 24, "422"), (97, 61, "422"), (48, 24, "440"), (97, 61, "440")]
TINY = [(1, 1), (7, 9), (9, 7), (17, 15)]  # in every layout: the per-block kernel (3x and 4x factors have no other)
GREY = [(70, 50), (1, 1), (129, 130)]


def _mixed_list():
    shapes = [(w, h, lay, 3) for w, h, lay in SHAPES] + [(w, h, lay, 3) for lay in LAYOUTS for w, h in TINY]
    for k, (w, h) in enumerate(GREY):  # grey pictures among the colour ones
        shapes.insert(3 + 9 * k, (w, h, "444", 1))
    pics = [PU.planes(w, h, 400 + i, nc) for i, (w, h, _, nc) in enumerate(shapes)]
    cases = [(lay, (5, 50, 85, 100)[i % 4], (0, 1, 3, 600)[(i // 4 + i) % 4]) for i, (_, _, lay, _) in enumerate(shapes)]
    return shapes, pics, cases


@pytest.fixture(scope="module")
def mixed(dec):
    """The mixed list and, once, what the interleaved encoder makes of it without and with `optimize`."""
    shapes, pics, cases = _mixed_list()
    expected = {opt: _interleaved(dec, pics, cases, opt) for opt in (False, True)}
    return shapes, pics, cases, expected


def test_content_of_the_mixed_list(mixed):
    shapes, pics, cases, _ = mixed
    assert {s[:3] for s in shapes} >= set(SHAPES) and set(LAYOUTS) >= {"444", "420", "422", "440", "411", "3x3"}
    assert {(w, h, lay) for w, h, lay, nc in shapes if nc == 3} >= {(w, h, lay) for lay in LAYOUTS for w, h in TINY}
    assert {c[1] for c in cases} == {5, 50, 85, 100} and {c[2] for c in cases} == {0, 1, 3, 600} and sum(s[3] == 1 for s in shapes) == 3
    for s, p in zip(shapes, pics):
        assert PU.tells_planes_and_positions_apart(p) and PU.shifted_differs(p), s


@pytest.mark.parametrize("optimize", [False, True])
def test_mixed_list_equals_the_interleaved_encoder(dec, oracle, mixed, optimize):
    shapes, pics, cases, expected = mixed
    want, want_stats = expected[optimize]
    got, st, pst = _planar(dec, pics, cases, optimize)
    n = len(pics)
    assert len(got) == len(want) == n
    for i in range(n):
        assert got[i] == want[i], (i, shapes[i], cases[i], len(got[i]), len(want[i]))
        assert want[i][:2] == b"\xff\xd8" and want[i][-2:] == b"\xff\xd9" and len(want[i]) > 100
    greys = sum(s[3] == 1 for s in shapes)
    assert pst == dict(pictures=n, fused=n - greys, two_pass=0, own_plane=greys, interleave_launches=0)
    assert st["pictures"] == n and st["passes"] == 1 and 7 <= st["forward_launches"] <= 12, st  # (six planar lists, the grey pictures' per-block list)
    assert st["host_syncs"] == want_stats["host_syncs"] and st["coder_launches"] == want_stats["coder_launches"]
    assert st["bytes_downloaded"] == want_stats["bytes_downloaded"]
    # (implied by the bytes; catches a comparison that compares nothing)
    for i in (0, n - 1):
        (ia, pa), (ib, pb) = oracle.decode_coefficients(got[i]), oracle.decode_coefficients(want[i])
        assert (ia.width, ia.height, ia.ncomp) == (ib.width, ib.height, ib.ncomp) == shapes[i][:2] + (shapes[i][3],)
        assert len(pa) == len(pb) == shapes[i][3] and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert np.array_equal(oracle.decode(got[0]), oracle.decode(want[0]))
    # swapped planes are another picture: the content tells them apart all the way into the stream
    swapped = [p[::-1] if p.shape[0] == 3 else p for p in pics[:3]]
    other, _, _ = _planar(dec, swapped, cases[:3], optimize)
    assert other[0] != want[0] and other[1] != want[1] and other[2] != want[2]


ALIGNMENT = [(130, 200, "420"), (97, 61, "422")]


@pytest.mark.parametrize("how", ["offsets", "oddpitch", "reversed", "separate"])
def test_alignment(dec, mixed, how):
    """Planes at 1, 2 and 3 bytes off a dword boundary, an odd pitch, planes in reversed memory order, three allocations: the same
    streams, all pictures `fused`; off the dword boundaries the per-block kernel reads byte by byte and is the only launch."""
    shapes, pics, cases, expected = mixed
    idx = [shapes.index(s + (3,)) for s in ALIGNMENT]
    got, st, pst = _planar(dec, [pics[i] for i in idx], [cases[i] for i in idx], False, how)
    for k, i in enumerate(idx):
        assert got[k] == expected[False][0][i], (how, shapes[i])
    assert pst == dict(pictures=2, fused=2, two_pass=0, own_plane=0, interleave_launches=0)
    if how in ("offsets", "oddpitch"):
        assert st["forward_launches"] == 1, st
    else:
        assert st["forward_launches"] == 5, st  # tile, <1,1>, <2,2>, <2,1>, per-block


@pytest.mark.parametrize("pad", [5, 64])
def test_padding_is_not_read_as_data(dec, mixed, pad):
    """A pitch 5 and 64 bytes beyond the (rounded) width, gaps between the planes; random bytes in padding and gaps, different ones
    in the second run: both runs give the expected streams.  (5: planes on their dword boundaries, lines not -- the byte-wise route.)"""
    shapes, pics, cases, expected = mixed
    idx = [shapes.index(s + (3,)) for s in [(130, 200, "420"), (256, 144, "420"), (100, 60, "420"), (333, 257, "444"), (97, 61, "422"), (97, 61, "440"), (17, 15, "411")]]
    for seed in (1, 2):
        got, _, pst = _planar(dec, [pics[i] for i in idx], [cases[i] for i in idx], False, "aligned", fill=seed, pad=pad, gap=4 * pad)
        assert pst["fused"] == len(idx)
        for k, i in enumerate(idx):
            assert got[k] == expected[False][0][i], (pad, seed, shapes[i])


def test_12_bit_and_mixed_precision(dec):
    """12-bit colour pictures are interleaved first (two_pass, one launch each), a grey 12-bit picture is its own plane, 8-bit pictures
    between them take the fused route: the streams of mijpeg_encode_ragged_device16 on the interleaved pictures."""
    spec = [(130, 200, "420", 3, 12), (72, 40, "422", 3, 8), (64, 40, "420", 3, 12), (33, 17, "444", 3, 8), (70, 50, "444", 1, 12), (128, 128, "420", 3, 8)]
    pics = [PU.planes(w, h, 900 + i, nc, bits) for i, (w, h, _, nc, bits) in enumerate(spec)]
    cases = [(lay, (30, 85, 100)[i % 3], (0, 2)[i % 2]) for i, (_, _, lay, _, _) in enumerate(spec)]
    for p in pics:
        assert PU.tells_planes_and_positions_apart(p)
    for opt in (False, True):
        want, want_stats = _interleaved(dec, pics, cases, opt)
        got, st, pst = _planar(dec, pics, cases, opt)
        for i in range(len(spec)):
            assert got[i] == want[i], (opt, i, spec[i])
        assert pst == dict(pictures=6, fused=3, two_pass=2, own_plane=1, interleave_launches=2)  # (one interleave launch per two-pass picture)
        assert st["host_syncs"] == want_stats["host_syncs"] == 4 and st["passes"] == 1 and st["forward_launches"] <= 18


def test_two_pass_route_at_8_bit(dec, mixed, monkeypatch):
    """MIJPEG_ENCODE_PLANAR_TWO_PASS (what tools/planar_encode_bench.py times the planar kernels against): the 8-bit colour pictures
    are interleaved first as well -- same streams, one interleave launch each, nothing on the planar lists."""
    shapes, pics, cases, expected = mixed
    idx = list(range(0, len(pics), 3))
    sub, sub_cases = [pics[i] for i in idx], [cases[i] for i in idx]
    colour = sum(p.shape[0] == 3 for p in sub)
    monkeypatch.setenv("MIJPEG_ENCODE_PLANAR_TWO_PASS", "1")
    got, st, pst = _planar(dec, sub, sub_cases, False, "offsets")
    monkeypatch.delenv("MIJPEG_ENCODE_PLANAR_TWO_PASS")
    assert got == [expected[False][0][i] for i in idx]
    assert pst == dict(pictures=len(idx), fused=0, two_pass=colour, own_plane=len(idx) - colour, interleave_launches=colour) and 0 < colour < len(idx)
    assert st["forward_launches"] <= 6 and st["host_syncs"] == 3


def test_uniform_batch_as_nchw(dec):
    torch = _torch()
    nchw = torch.from_numpy(np.stack([PU.planes(640, 360, 70 + i) for i in range(5)])).cuda()
    hwc = [nchw[i].permute(1, 2, 0).contiguous() for i in range(5)]
    want = batch.encode_mixed(hwc, 85, "420", 0, decoder=dec)
    got = batch.encode_mixed(nchw, 85, "420", 0, decoder=dec, layout="chw")
    assert len(got) == 5 and got == want and len(set(got)) == 5
    assert dec.encode_planar_stats() == dict(pictures=5, fused=5, two_pass=0, own_plane=0, interleave_launches=0)
    assert batch.encode_mixed([nchw[i] for i in range(5)], 85, "420", 0, decoder=dec, layout="chw") == want


def test_round_trip(dec, mixed):
    """decode_mixed(layout="chw") -> encode_mixed(layout="chw") gives the streams of the HWC round trip."""
    shapes, _, _, expected = mixed
    idx = [i for i, s in enumerate(shapes) if s[2] in ("420", "444", "422") and (s[0] > 20 or s[3] == 1)]
    streams = [expected[False][0][i] for i in idx]
    subs = [shapes[i][2] for i in idx]
    assert len(idx) >= 10 and any(shapes[i][3] == 1 for i in idx)
    hwc = batch.decode_mixed(streams, 0, decoder=dec)
    chw = batch.decode_mixed(streams, 0, decoder=dec, layout="chw")
    assert not any(isinstance(t, Exception) for t in hwc + chw)
    want = batch.encode_mixed(hwc, 85, subs, 0, decoder=dec)
    got = batch.encode_mixed(chw, 85, subs, 0, decoder=dec, layout="chw")
    assert got == want and len(got) == len(idx)
    pst = dec.encode_planar_stats()
    assert pst["fused"] + pst["own_plane"] == len(idx) and pst["two_pass"] == 0


def test_pass_cutting_is_invisible(dec, mixed, monkeypatch):
    shapes, pics, cases, expected = mixed
    twelve = [PU.planes(64, 40, 77, 3, 12), PU.planes(130, 70, 78, 3, 12)]
    extra = [("420", 85, 0), ("444", 50, 2)]
    all_pics, all_cases = pics[:8] + twelve[:1] + pics[8:20] + twelve[1:], cases[:8] + extra[:1] + cases[8:20] + extra[1:]
    want12, _ = _interleaved(dec, twelve, extra, False)
    want = expected[False][0][:8] + want12[:1] + expected[False][0][8:20] + want12[1:]
    whole, st, pst = _planar(dec, all_pics, all_cases, False)
    assert st["passes"] == 1 and pst["two_pass"] == 2
    monkeypatch.setenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS", "1536")
    cut, st, pst = _planar(dec, all_pics, all_cases, False)
    monkeypatch.delenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS")
    assert st["passes"] >= 3 and st["pictures"] == len(all_pics) and st["host_syncs"] <= 4 * st["passes"] and st["forward_launches"] <= 18 * st["passes"]
    assert pst["pictures"] == len(all_pics) and pst["two_pass"] == 2 and pst["interleave_launches"] == 2 and pst["fused"] + pst["own_plane"] == len(all_pics) - 2
    for i in range(len(all_pics)):
        assert whole[i] == want[i] and cut[i] == want[i], (i, all_cases[i])


@pytest.mark.parametrize("optimize", [False, True])
def test_launches_and_waits_do_not_grow_with_n(dec, optimize):
    stats = {}
    for n in (4, 64):
        spec = [((16, 24, 20, 32)[i % 4], 16 + (i // 4) % 9, ("444", "420", "444", "422")[i % 4], 1 if i % 4 == 2 else 3) for i in range(n)]
        pics = [PU.planes(w, h, 100 + i, nc) for i, (w, h, _, nc) in enumerate(spec)]
        cases = [(lay, 85, 0) for _, _, lay, _ in spec]
        want, want_stats = _interleaved(dec, pics, cases, optimize)
        got, st, pst = _planar(dec, pics, cases, optimize)
        assert got == want and pst["fused"] == n - n // 4 and pst["own_plane"] == n // 4
        assert st["host_syncs"] == want_stats["host_syncs"] == (4 if optimize else 3)
        stats[n] = st
    for k in ("forward_launches", "coder_launches", "host_syncs", "passes"):
        assert stats[4][k] == stats[64][k] and stats[4][k] > 0, (k, stats)
    assert stats[64]["forward_launches"] <= 12


def test_argument_errors_leave_nothing_behind(dec, mixed):
    """Every error of the contract: INVALID_PARAMETER, all outputs cleared, the statistics of the last call left alone, the object
    usable -- the next good call gives the right streams."""
    shapes, pics, cases, expected = mixed
    L = api.lib()
    idx = [shapes.index(s + (3,)) for s in [(130, 200, "420"), (24, 40, "444"), (48, 24, "422")]]
    sub, sub_cases = [pics[i] for i in idx], [cases[i] for i in idx]
    twelve = PU.planes(48, 24, 5, 3, 12)
    good, _, before = _planar(dec, sub, sub_cases, False)
    before_ragged = dec.encode_ragged_stats()
    placed = [_place(p) for p in sub]
    p12 = _place(twelve)
    frames = [api.encode_frame(p.shape[2], p.shape[1], 3, q, LAYOUTS[lay], ri, 0, pitch) for p, (_, _, pitch), (lay, q, ri) in zip(sub, placed, sub_cases)]
    planes = [list(ptrs) for _, ptrs, _ in placed]

    def call(frames_, planes_, prec, null=()):
        arr = (api.MijpegEncodeFrame * 3)(*frames_)
        flat = []
        for p in planes_:
            flat += [q or None for q in p] + [None] * (4 - len(p))
        table = (C.c_void_p * 12)(*flat)
        ptrs, sizes = (C.c_void_p * 3)(*([0xdead0] * 3)), (C.c_size_t * 3)(*([77] * 3))
        rc = L.mijpeg_encode_ragged_planar_device16(dec._h, None if "frames" in null else arr, None if "planes" in null else table,
                                                    None if prec is None else (C.c_int32 * 3)(*prec), 3, 0, 0, ptrs, None if "sizes" in null else sizes)
        return rc, all(not ptrs[i] for i in range(3)) and all(sizes[i] == 0 for i in range(3))

    def spoiled(k, **kw):
        f = api.MijpegEncodeFrame.from_buffer_copy(bytes(frames[k]))
        for name, v in kw.items():
            setattr(f, name, v)
        return frames[:k] + [f] + frames[k + 1:]

    f12 = api.encode_frame(48, 24, 3, 85, LAYOUTS["422"], 0, 0, p12[2])
    bad = [(frames, planes, None, ("frames",)), (frames, planes, None, ("planes",)),
           (frames, [planes[0], [planes[1][0], 0, planes[1][2]], planes[2]], None, ()),  # a NULL plane that a picture needs
           (spoiled(2, row_stride=47), planes, None, ()),  # a pitch below one line
           (frames[:2] + [f12], planes[:2] + [[p12[1][0], p12[1][1] + 1, p12[1][2]]], [8, 8, 12], ()),  # an odd address at 12 bit
           (frames[:2] + [api.encode_frame(48, 24, 3, 85, LAYOUTS["422"], 0, 0, p12[2] + 1)], planes[:2] + [p12[1]], [8, 8, 12], ()),  # an odd pitch
           (frames[:2] + [api.encode_frame(48, 24, 3, 85, LAYOUTS["422"], 0, 0, 94)], planes[:2] + [p12[1]], [8, 8, 12], ()),  # a pitch below a line of 16-bit samples
           (frames, planes, [8, 10, 8], ())]  # a precision other than 8 or 12
    for frames_, planes_, prec, null in bad:
        rc, cleared = call(frames_, planes_, prec, null)
        assert rc == api.ERR_INVALID_PARAMETER and cleared, (prec, null)
        assert dec.encode_planar_stats() == before and dec.encode_ragged_stats() == before_ragged  # nothing launched, nothing counted
        again, _, _ = _planar(dec, sub, sub_cases, False)
        assert again == good
    assert call(frames, planes, None, ("sizes",))[0] == api.ERR_INVALID_PARAMETER
    for k, i in enumerate(idx):
        assert good[k] == expected[False][0][i]
    # the good 12-bit picture of the spoiled lists is a good picture
    got, _, pst = _planar(dec, sub[:2] + [twelve], sub_cases[:2] + [("422", 85, 0)], False)
    assert got[:2] == good[:2] and got[2] == _interleaved(dec, [twelve], [("422", 85, 0)], False)[0][0] and pst["two_pass"] == 1
    del placed, p12


@pytest.mark.parametrize("sample_bytes", [1, 2])
@pytest.mark.parametrize("components", [1, 3, 4])
def test_interleave_device(dec, components, sample_bytes):
    """mijpeg_interleave_device: the whole destination arena against numpy, guard bytes around it and line padding untouched."""
    torch = _torch()
    dt = np.uint8 if sample_bytes == 1 else np.uint16
    for w, h in ((1, 1), (7, 3), (8, 8), (9, 5), (130, 17)):
        src_pitch, dst_pitch = w * sample_bytes + 6, w * components * sample_bytes + 10
        rng = np.random.default_rng(w * 100 + h + components)
        planes = rng.integers(0, 1 << (8 * sample_bytes), (components, h, w)).astype(dt)
        src = rng.integers(0, 256, (components, h, src_pitch), dtype=np.uint8)
        src[:, :, :w * sample_bytes] = planes.view(np.uint8).reshape(components, h, w * sample_bytes)
        guard = 64
        arena = rng.integers(0, 256, guard + h * dst_pitch + guard, dtype=np.uint8)
        want = arena.copy()
        want[guard:guard + h * dst_pitch].reshape(h, dst_pitch)[:, :w * components * sample_bytes] = \
            np.ascontiguousarray(planes.transpose(1, 2, 0)).view(np.uint8).reshape(h, w * components * sample_bytes)
        dsrc, darena = torch.from_numpy(src).cuda(), torch.from_numpy(arena).cuda()
        api.interleave_device(dec, [dsrc[c].data_ptr() for c in range(components)], src_pitch, w, h, components, sample_bytes, darena.data_ptr() + guard, dst_pitch)
        assert np.array_equal(darena.cpu().numpy(), want), (w, h)


def test_front_end(dec, mixed):
    shapes, pics, cases, expected = mixed
    torch = _torch()
    i = shapes.index((130, 200, "420", 3))
    hwc = _dev(pics[i].transpose(1, 2, 0))
    lay, q, ri = cases[i]
    assert batch.encode_mixed([hwc], q, lay, ri, decoder=dec) == [expected[False][0][i]]  # layout="hwc" is what it was
    assert batch.encode_mixed([hwc], q, lay, ri, decoder=dec, layout="hwc") == [expected[False][0][i]]
    with pytest.raises(ValueError, match="hwc"):  # strided pixels: a permuted view of an HWC picture
        batch.encode_mixed([hwc.permute(2, 0, 1)], q, lay, ri, decoder=dec, layout="chw")
    with pytest.raises(ValueError, match="hwc"):
        batch.encode_mixed([pics[i]], q, lay, ri, decoder=dec, layout="chw")
    with pytest.raises(ValueError):
        batch.encode_mixed(np.stack([pics[i]]), q, lay, ri, decoder=dec, layout="chw")
    with pytest.raises(ValueError):
        batch.encode_mixed([hwc], q, lay, ri, decoder=dec, layout="nchw")
    # plane and line strides are free: a window of a larger (3, H, W) tensor, and a grey (H, W) picture
    big = torch.zeros((3, 220, 160), dtype=torch.uint8, device="cuda")
    big[:, 10:210, 12:142] = _dev(pics[i])
    assert batch.encode_mixed([big[:, 10:210, 12:142]], q, lay, ri, decoder=dec, layout="chw") == [expected[False][0][i]]
    g = shapes.index((70, 50, "444", 1))
    assert batch.encode_mixed([_dev(pics[g][0]), _dev(pics[g])], [cases[g][1]] * 2, "420", [cases[g][2]] * 2, decoder=dec, layout="chw") == [expected[False][0][g]] * 2
    assert batch.encode_mixed([], layout="chw") == []

"""Planar output on the device (include/mijpeg.h: mijpeg_reconstruct_planar_device, its batch and ragged forms): the
planar flavours of the fused ragged kernels (mij::planar) and the two-pass route (deinterleave_kernel).

The expectation is the oracle's decode of the same stream, transposed per component; tolerance 0.  Every destination is one buffer
pre-filled with a guard byte in which the planes lie at a chosen offset, with padded lines, gaps between planes and between
frames and a guard band in front and behind: after the call every byte that is not a sample of a plane must still hold the guard.
planar_stats says which route wrote a picture, so a build that de-interleaves everything fails the fused cases."""
import functools

import numpy as np
import pytest

from conftest import golden_jpeg
from libjpeg_amd import api, batch, synth
from test_ragged_batch import _flavour
from test_ragged_gates import K8, _gate

pytestmark = pytest.mark.gpu

GUARD = 0xA5
BAND = 192  # guard bytes in front of and behind everything


class Dest:
    """frames x comps planes of h x w samples of sb bytes in one guarded device buffer: plane (f, c) starts at
    BAND + base + f * frame_stride + c * plane_stride, its lines row bytes apart."""

    def __init__(self, frames, comps, h, w, sb=1, pad=5, plane_gap=7, frame_gap=11, base=0):
        import torch

        self.frames, self.comps, self.h, self.w, self.sb, self.base = frames, comps, h, w, sb, base
        self.row = w * sb + pad
        self.plane_stride = h * self.row + plane_gap
        self.frame_stride = comps * self.plane_stride + frame_gap
        self.size = BAND + base + frames * self.frame_stride + BAND
        self.buf = torch.full((self.size,), GUARD, dtype=torch.uint8, device="cuda")

    def offset(self, f, c):
        return BAND + self.base + f * self.frame_stride + c * self.plane_stride

    def ptr(self, f, c):
        return self.buf.data_ptr() + self.offset(f, c)

    def ptrs(self, f=0):
        return [self.ptr(f, c) for c in range(self.comps)]

    def result(self):
        """-> ([frame][component] planes, number of bytes outside the planes' samples that no longer hold the guard)"""
        flat = self.buf.cpu().numpy()
        written = np.zeros(self.size, bool)
        out = []
        for f in range(self.frames):
            planes = []
            for c in range(self.comps):
                o = self.offset(f, c)
                idx = o + (np.arange(self.h)[:, None] * self.row + np.arange(self.w * self.sb)[None, :])
                written[idx] = True
                p = np.ascontiguousarray(flat[idx])
                planes.append(p.view("<u2").reshape(self.h, self.w) if self.sb == 2 else p)
            out.append(planes)
        return out, int((flat[~written] != GUARD).sum())


def _expect_planes(pixels):
    return [np.ascontiguousarray(pixels[:, :, c]) for c in range(pixels.shape[2])]


def _same(planes, exp):
    return len(planes) == len(exp) and all(p.shape == e.shape and np.array_equal(p, e) for p, e in zip(planes, exp))


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ the fused planar flavours
# width x height, the smallest at which the store path can go wrong: less than one MCU, both edges cut inside one block; 2 x 2 tiles
# (a whole-wave path in tile (0, 0), partial blocks on both edges, plane offsets across tiles); three tiles across with the right
# edge on a block boundary
SHAPES = [(1, 1), (9, 23), (141, 150), (264, 136)]
# name -> (layout, kernel as mijpeg_kernel_name says it with per-frame tables, fast, flags, (luma, chroma) budget or None: a photograph)
FLAVOURS = {
    "420-packed": ("420", K8["420p"], 1, 0, None),
    "420-safe": ("420", K8["420"], 0, api.FLAG_FORCE_SAFE, None),
    "420-fast-2047": ("420", K8["420"], 1, 0, (16383, 2047)),
    "420-fast-16383": ("420", K8["420"], 1, 0, (16383, 16383)),
    "422-packed": ("422", K8["422"], 1, 0, None),
    "422-wide-2047": ("422", K8["422w"], 1, 0, (16383, 2047)),
    "422-wide-8189": ("422", K8["422w"], 1, 0, (16383, 8189)),
    "444": ("444", K8["444"], 1, 0, None),
}


@functools.lru_cache(maxsize=None)
def _stream(flavour, w, h):
    layout, kernel, fast, _flags, budgets = FLAVOURS[flavour]
    seed = 4000 + 7 * w + h
    if budgets is None:
        return synth.synth_jpeg(w, h, seed, 85, layout, 1 + seed % 7)
    return _gate(layout, w, h, 8, budgets[0], budgets[1], kernel, fast, seed).stream


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_fused_planar_flavour(dec, oracle, flavour, shape):
    w, h = shape
    layout, kernel, fast, flags, _budgets = FLAVOURS[flavour]
    data = _stream(flavour, w, h)
    f = dec.read(data)
    assert (f.width, f.height, f.components) == (w, h, 3)
    if not flags:  # (FORCE_SAFE is the caller's: the stream itself is a packed one)
        assert _flavour(f) == (kernel, fast), _flavour(f)
    dst = Dest(1, 3, h, w, base=1)
    dec.reconstruct_planar_device(dst.ptrs(), dst.row, flags)
    st = dec.planar_stats()
    planes, touched = dst.result()
    assert _same(planes[0], _expect_planes(oracle.decode(data)))
    assert touched == 0
    assert st == dict(images=1, fused=1, two_pass=0, fused_launches=1, two_pass_launches=0), st


@pytest.mark.parametrize("flavour", ["420-packed", "444"])
def test_plane_alignment(dec, oracle, flavour):
    """Plane bases 0..3 bytes off a 256-byte boundary, lines of 141 bytes (odd: every line starts at another alignment) and padded to 144."""
    w, h = 141, 150
    data = _stream(flavour, w, h)
    exp = _expect_planes(oracle.decode(data))
    dec.read(data)
    for base in range(4):
        for pad in (0, 3):
            dst = Dest(1, 3, h, w, pad=pad, plane_gap=64 - base if pad else 7, base=base)
            assert dst.buf.data_ptr() % 256 == 0
            dec.reconstruct_planar_device(dst.ptrs(), dst.row)
            planes, touched = dst.result()
            assert _same(planes[0], exp), (base, pad)
            assert touched == 0, (base, pad)
            assert dec.planar_stats()["fused"] == 1


def test_uniform_batch_as_nchw(oracle):
    streams = [synth.synth_jpeg(141, 150, 4500 + i, 85, "420", 3) for i in range(3)]
    d = api.Decoder(0)
    d.decode_batch_device(streams, 1)
    dst = Dest(3, 3, 150, 141, pad=3, plane_gap=77, frame_gap=1001, base=2)
    d.reconstruct_batch_planar_device(dst.ptr(0, 0), dst.frame_stride, dst.plane_stride, dst.row)
    st = d.planar_stats()
    planes, touched = dst.result()
    for i in range(3):
        assert _same(planes[i], _expect_planes(oracle.decode(streams[i]))), i
    assert touched == 0
    assert st == dict(images=3, fused=3, two_pass=0, fused_launches=1, two_pass_launches=0), st
    # strides that do not hold a plane or a frame are refused before anything runs
    for args in ((dst.frame_stride, 150 * dst.row - 1, dst.row), (3 * dst.plane_stride - 1, dst.plane_stride, dst.row), (dst.frame_stride, dst.plane_stride, 140)):
        with pytest.raises(api.MijpegError) as e:
            d.reconstruct_batch_planar_device(dst.ptr(0, 0), *args)
        assert e.value.code == api.ERR_INVALID_PARAMETER
    d.close()


# ------------------------------------------------------------------------------------------------ ragged lists
def test_ragged_list(oracle):
    """Pictures of four layouts and two precisions, one of the single-image route, a broken stream and a skipped picture in one
    call: every plane equals the interleaved ragged call's picture transposed (and the oracle's, for the 8-bit ones)."""
    import torch

    streams = [synth.synth_jpeg(200, 136, 4601, 85, "420", 4),             # 0: fused planar, packed 4:2:0
               synth.synth_jpeg(131, 77, 4602, 90, "422", 0),              # 1: fused planar, 4:2:2
               b"\xff\xd8 this is no JPEG stream \xff\xd9" * 3,            # 2: broken
               synth.synth_jpeg(150, 141, 4603, 75, "444", 2),             # 3: fused planar, 4:4:4
               synth.encode_jpeg(synth.synth_image(70, 45, 4604, channels=1), 85, "444", 0),  # 4: grey, its own plane
               golden_jpeg("ref_97x61_440"),                               # 5: single-image route, 4:4:0: two passes
               golden_jpeg("p12_120x90_420_dri3"),                         # 6: 12 bit: int16 planes, two passes
               synth.synth_jpeg(90, 50, 4605, 85, "420", 0)]               # 7: skipped
    d = api.Decoder(0)
    status = d.decode_ragged_device(streams, with_12bit=True)
    assert [s != 0 for s in status] == [i == 2 for i in range(8)], status
    infos = [d.ragged_info(i) if i != 2 else None for i in range(8)]
    assert infos[6].precision == 12 and infos[6].sample_bytes == 2 and infos[4].components == 1
    assert d.ragged_route(5)[0] is False and all(d.ragged_route(i)[0] for i in (0, 1, 3, 4, 6, 7))
    # the interleaved call
    inter = {}
    ptrs, rows = [], []
    for i, f in enumerate(infos):
        if f is None:
            ptrs.append(0)
            rows.append(0)
            continue
        inter[i] = torch.zeros((f.height, f.width, f.components), dtype=torch.int16 if f.sample_bytes > 1 else torch.uint8, device="cuda")
        ptrs.append(inter[i].data_ptr())
        rows.append(f.width * f.components * max(1, f.sample_bytes))
    d.reconstruct_ragged_device(ptrs, rows)
    inter = {i: t.cpu().numpy() for i, t in inter.items()}
    # the planar call: image 7 is skipped, image 2 has no picture
    dsts = {i: Dest(1, f.components, f.height, f.width, sb=max(1, f.sample_bytes), pad=(0, 6, 14)[i % 3], base=(0, 2)[i % 2] * max(1, f.sample_bytes))
            for i, f in enumerate(infos) if f is not None and i != 7}
    d.reconstruct_ragged_planar_device([dsts[i].ptrs() if i in dsts else None for i in range(8)], [dsts[i].row if i in dsts else 0 for i in range(8)])
    st = d.planar_stats()
    print("planar stats:", st)
    for i, dst in dsts.items():
        planes, touched = dst.result()
        exp = inter[i].view(np.uint16) if infos[i].sample_bytes > 1 else inter[i]
        assert _same(planes[0], _expect_planes(exp)), i
        if infos[i].precision == 8:
            want = oracle.decode(streams[i])
            assert _same(planes[0], _expect_planes(want.reshape(want.shape[0], want.shape[1], -1))), i
        assert touched == 0, i
    # 0, 1, 3: one fused planar launch each (three kernels); 4: grey, one pass into its plane; 5 and 6: two passes
    assert st == dict(images=6, fused=4, two_pass=2, fused_launches=3, two_pass_launches=2), st
    # a destination that does not hold a line is refused before anything is launched, whichever image it belongs to
    bad_rows = [dsts[i].row if i in dsts else 0 for i in range(8)]
    bad_rows[6] = infos[6].width * 2 - 1
    with pytest.raises(api.MijpegError) as e:
        d.reconstruct_ragged_planar_device([dsts[i].ptrs() if i in dsts else None for i in range(8)], bad_rows)
    assert e.value.code == api.ERR_INVALID_PARAMETER
    d.close()


def test_back_to_back_calls_share_the_pinned_tables(oracle):
    """The interleaved and the planar list call fill the same pinned tables (launch_fused_lists): three calls that nobody waits
    for in between, each into fresh destinations, write what the synchronised calls wrote -- the second and third wait for the
    upload before them instead of overwriting tables that are still on their way.  Three pictures of one or two tiles in three
    layouts: three launches per call, one table behind the other."""
    import torch

    streams = [synth.synth_jpeg(136, 8, 4801, 85, "420", 0), synth.synth_jpeg(8, 136, 4802, 85, "422", 0), synth.synth_jpeg(16, 16, 4803, 85, "444", 0)]
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams) == [0, 0, 0]
    infos = [d.ragged_info(i) for i in range(3)]
    assert [(f.width, f.height) for f in infos] == [(136, 8), (8, 136), (16, 16)]

    def interleaved(sync):
        outs = [torch.full((f.height, f.width, 3), GUARD, dtype=torch.uint8, device="cuda") for f in infos]
        d.reconstruct_ragged_device([t.data_ptr() for t in outs], [f.width * 3 for f in infos], sync=sync)
        return outs

    def planar(sync):
        dsts = [Dest(1, 3, f.height, f.width) for f in infos]
        d.reconstruct_ragged_planar_device([dst.ptrs() for dst in dsts], [dst.row for dst in dsts], sync=sync)
        return dsts

    exp = [t.cpu().numpy() for t in interleaved(True)]
    assert d.ragged_stats()["recon_launches"] == 3 and d.ragged_stats()["recon_single"] == 0
    exp_planes = [dst.result()[0][0] for dst in planar(True)]
    assert d.planar_stats() == dict(images=3, fused=3, two_pass=0, fused_launches=3, two_pass_launches=0)
    assert np.array_equal(exp[0], oracle.decode(streams[0]))
    for i in range(3):
        assert _same(exp_planes[i], _expect_planes(exp[i])), i
    first, second, third = interleaved(False), planar(False), interleaved(False)
    d.synchronize()
    for i in range(3):
        assert np.array_equal(first[i].cpu().numpy(), exp[i]), i
        planes, touched = second[i].result()
        assert _same(planes[0], exp_planes[i]) and touched == 0, i
        assert np.array_equal(third[i].cpu().numpy(), exp[i]), i
    d.close()


def test_decode_mixed_chw():
    streams = [synth.synth_jpeg(141, 150, 4701, 85, "420", 0), synth.synth_jpeg(64, 33, 4702, 85, "444", 2),
               synth.encode_jpeg(synth.synth_image(50, 20, 4703, channels=1), 85, "444", 0), golden_jpeg("p12_64x48_444"),
               golden_jpeg("pil_90x60_cmyk"), synth.synth_jpeg(9, 23, 4704, 85, "422", 1)]
    d = api.Decoder(0)
    hwc = batch.decode_mixed(streams, 0, decoder=d, with_12bit=True)
    chw = batch.decode_mixed(streams, 0, decoder=d, with_12bit=True, layout="chw")
    st = d.planar_stats()
    d.close()
    assert st["images"] == 6 and st["fused"] == 4 and st["two_pass"] == 2, st
    for i, (a, b) in enumerate(zip(hwc, chw)):
        assert b.dtype == a.dtype and tuple(b.shape) == (a.shape[2], a.shape[0], a.shape[1]) and b.is_contiguous(), i
        assert bool((a.permute(2, 0, 1) == b).all()), i
    with pytest.raises(ValueError):
        batch.decode_mixed(streams[:1], 0, layout="nchw")


# ------------------------------------------------------------------------------------------------ the two-pass route on its own
def test_two_pass_cmyk(dec, oracle):
    data = golden_jpeg("pil_90x60_cmyk")
    f = dec.read(data)
    assert f.components == 4
    dst = Dest(1, 4, f.height, f.width, base=3)
    dec.reconstruct_planar_device(dst.ptrs(), dst.row)
    planes, touched = dst.result()
    assert _same(planes[0], _expect_planes(oracle.decode(data)))
    assert touched == 0
    assert dec.planar_stats() == dict(images=1, fused=0, two_pass=1, fused_launches=0, two_pass_launches=1)


@pytest.mark.parametrize("name", ["xt_33x17_422", "xt_129x71_420"])
def test_two_pass_jpeg_xt(dec, oracle, name):
    data = golden_jpeg(name)
    f = dec.read(data)
    assert f.xt == 1 and f.sample_bytes == 2
    exp, _ = oracle.decode_xt(data)
    dst = Dest(1, 3, f.height, f.width, sb=2, pad=6, base=2)
    dec.reconstruct_planar_device(dst.ptrs(), dst.row)
    planes, touched = dst.result()
    assert _same(planes[0], _expect_planes(exp))
    assert touched == 0
    assert dec.planar_stats() == dict(images=1, fused=0, two_pass=1, fused_launches=0, two_pass_launches=1)


def test_force_generic_is_the_two_pass_route(dec, oracle):
    w, h = 141, 150
    data = _stream("420-packed", w, h)
    dec.read(data)
    fused, generic = Dest(1, 3, h, w), Dest(1, 3, h, w, pad=0, base=1)
    dec.reconstruct_planar_device(fused.ptrs(), fused.row)
    assert dec.planar_stats()["fused"] == 1
    dec.reconstruct_planar_device(generic.ptrs(), generic.row, api.FLAG_FORCE_GENERIC)
    assert dec.planar_stats() == dict(images=1, fused=0, two_pass=1, fused_launches=0, two_pass_launches=1)
    (a, ta), (b, tb) = fused.result(), generic.result()
    assert _same(a[0], b[0]) and _same(b[0], _expect_planes(oracle.decode(data)))
    assert ta == 0 and tb == 0
    # without the colour transformation the fused kernels do not apply: two passes again, the oracle's untransformed samples
    nct = Dest(1, 3, h, w, pad=2)
    dec.reconstruct_planar_device(nct.ptrs(), nct.row, api.FLAG_NO_COLOR_TRANSFORM)
    assert dec.planar_stats()["two_pass"] == 1
    c, tc = nct.result()
    assert _same(c[0], _expect_planes(oracle.decode(data, 0))) and tc == 0

"""Resized crops as a normalised float batch, mirrored per picture (mijpeg_reconstruct_ragged_normalized_device,
batch.decode_resized(dtype=...)): the resized call's one resample launch with a float store epilogue, mirroring in the tap
tables.

Expected, at tolerance 0 on BIT PATTERNS: tests/normalize_model.py's normalize() of tests/resample_model.py's resize() of the oracle's
decode.  Every call writes into one device tensor of 0xA5 bytes with 64 guard bytes at either end, lines, planes and slots padded by 5, 7
and 11 elements and a base an odd number of elements in, and the WHOLE tensor is compared with what it must hold afterwards, as
test_ragged_resized.BatchArena does for the uint8 call.  One decode per list serves all the tests (the `lists` fixture); the pictures
are at most 300 x 270."""
import ctypes as C

import numpy as np
import pytest

import normalize_model as N
from conftest import golden_jpeg
from libjpeg_amd import api
from test_ragged_gates import _expected
from test_ragged_rect import EDGE, GUARD, SIZES, _layout_list
from test_ragged_resized import WHOLE, _pictures, _want

TYPES = {"f32": N.F32, "f16": N.F16, "bf16": N.BF16}
LAYOUTS = ("420", "grey")
OUT_SIZES = [(1, 1), (37, 5), (63, 16), (64, 17), (65, 33), (224, 224)]  # tile edges on both axes; 3, 5, 8 taps in registers and more than 8
ALTERNATE = [True, False, True, False, True]


class NormArena:
    """The destination of one normalised call in a device tensor of 0xA5 bytes: GUARD bytes, a base 1 or 3 elements in, n slots whose
    lines, planes and slots are padded by 5, 7 and 11 elements, GUARD bytes.  Everything in bytes, as the call takes it."""

    def __init__(self, n, ow, oh, channels, planar, sample, base=0):
        import torch

        self.n, self.ow, self.oh, self.channels, self.planar, self.sample = n, ow, oh, channels, planar, sample
        self.es = es = api.SAMPLE_BYTES[sample]
        self.line = ow * (1 if planar else channels) * es
        self.row = self.line + 5 * es
        self.plane = oh * self.row + 7 * es if planar else 0
        self.image = (channels * self.plane if planar else oh * self.row) + 11 * es
        self.at = GUARD + (1 + 2 * (base % 2)) * es
        self.size = self.at + n * self.image + GUARD
        self.dev = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (self.dev.data_ptr() + self.at) % es == 0

    def call(self, d, rects, consts=None, mirror=None, **kw):
        scale, bias = consts if consts else (None, None)
        return d.reconstruct_ragged_normalized_device(rects, self.ow, self.oh, self.channels, self.sample, scale, bias, mirror, self.dev.data_ptr() + self.at,
                                                      self.image, self.plane, self.row, **kw)

    def call_resized(self, d, rects, **kw):
        """the uint8 resized call into the same layout"""
        assert self.es == 1
        return d.reconstruct_ragged_resized_device(rects, self.ow, self.oh, self.channels, self.dev.data_ptr() + self.at, self.image, self.plane, self.row, **kw)

    def _lines(self, i, c):
        o = self.at + i * self.image + c * self.plane
        return [(o + y * self.row, o + y * self.row + self.line) for y in range(self.oh)]

    def expect(self, slots):
        """slots[i]: (oh, ow, channels) array of the elements' bit patterns, or None for a slot that stays as it is"""
        want = np.full(self.size, 0xA5, np.uint8)
        for i, pic in enumerate(slots):
            if pic is None:
                continue
            assert pic.shape == (self.oh, self.ow, self.channels) and pic.dtype == N.ELEMENT[self.sample], (pic.shape, pic.dtype, i)
            parts = [np.ascontiguousarray(pic[:, :, c]) for c in range(self.channels)] if self.planar else [np.ascontiguousarray(pic).reshape(self.oh, -1)]
            for c, part in enumerate(parts):
                raw = part.view(np.uint8).reshape(self.oh, self.line)
                for y, (lo, hi) in enumerate(self._lines(i, c)):
                    want[lo:hi] = raw[y]
        return want

    def slot(self, host, i):
        """slot i of a copy of the tensor -> its (oh, ow, channels) bit patterns"""
        el = N.ELEMENT[self.sample]
        if self.planar:
            return np.stack([np.stack([host[lo:hi].view(el) for lo, hi in self._lines(i, c)]) for c in range(self.channels)], axis=2)
        return np.stack([host[lo:hi].view(el) for lo, hi in self._lines(i, 0)]).reshape(self.oh, self.ow, self.channels)

    def check(self, slots, what=""):
        got, want = self.dev.cpu().numpy(), self.expect(slots)
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        slot, inside = divmod(int(bad[0]) - self.at, self.image)
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at offset {bad[0]} (slot {slot}, byte {inside} of it; got {got[bad[0]]}, want {want[bad[0]]})")


def _norm(key, pic, rect, ow, oh, channels, sample, consts, mirror=False):
    """The model's answer for one slot: normalize() of the resized call's expected slot (shared with test_ragged_resized, read-only)."""
    scale, bias = consts if consts else (None, None)
    v = _want(key, pic, rect, ow, oh, channels)
    return N.normalize(v, scale[:channels] if scale else None, bias[:channels] if bias else None, sample, mirror)


@pytest.fixture(scope="module")
def lists(oracle):
    """One decoder and ONE decode per list, for every test of this module: {layout: (decoder, pictures)}"""
    made = {}
    try:
        for layout in LAYOUTS:
            streams = _layout_list(layout)
            d = api.Decoder(0)
            made[layout] = (d, _pictures(oracle, streams))
            assert d.decode_ragged_device(list(streams)) == [0] * len(streams)
        yield made
    finally:
        for d, _ in made.values():
            d.close()


# ------------------------------------------------------------------------------------------------ 1: types x layouts x sizes
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("sample", list(TYPES), ids=list(TYPES))
def test_types_layouts_sizes(lists, sample, planar):
    """Whole pictures of 16 x 16 ... 300 x 270 to six sizes, both constant sets; the grey list into three channels, each with its own
    scale and bias, and into one."""
    sample = TYPES[sample]
    for layout in LAYOUTS:
        d, pictures = lists[layout]
        n = len(pictures)
        for j, (ow, oh) in enumerate(OUT_SIZES):
            for name, consts in N.SETS.items():
                arena = NormArena(n, ow, oh, 3, planar, sample, base=j)
                assert arena.call(d, None, consts) == [0] * n
                arena.check([_norm((layout, i), pictures[i], WHOLE, ow, oh, 3, sample, consts) for i in range(n)], what=f"{layout} -> {ow} x {oh}, {name}")
                st = d.ragged_resized_stats()
                assert st["images"] == st["resampled"] == n and st["refused"] == 0 and st["resample_launches"] == 1, st
                assert d.ragged_normalized_stats() == dict(sample=sample, mirrored=0)
    d, pictures = lists["grey"]
    arena = NormArena(len(pictures), 65, 33, 1, planar, sample, base=1)
    assert arena.call(d, None, N.CRAFTED) == [0] * len(pictures)
    arena.check([_norm(("grey", i), pictures[i], WHOLE, 65, 33, 1, sample, N.CRAFTED) for i in range(len(pictures))], what="grey, one channel")


# ------------------------------------------------------------------------------------------------ 2: mirror
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_mirror(lists, planar):
    """Mirrored and unmirrored pictures in one launch, then all mirrored, at widths 1, 2, 63, 64, 65 and 224: with uint8 samples the
    bytes are the resized call's slot reversed, with float16 the model's; `mirrored` counts the flagged pictures."""
    crops = [(w // 5, h // 4, w - 1, h - 2) for w, h in SIZES]
    for layout in LAYOUTS:
        d, pictures = lists[layout]
        n = len(pictures)
        for j, ow in enumerate([1, 2, 63, 64, 65, 224]):
            oh, rects = 9 + j, (crops if j % 2 else None)
            old = NormArena(n, ow, oh, 3, planar, N.U8, base=j)
            assert old.call_resized(d, rects) == [0] * n
            assert d.ragged_normalized_stats() == dict(sample=N.U8, mirrored=0)
            host = old.dev.cpu().numpy()
            plain = [old.slot(host, i) for i in range(n)]
            for i in range(n):
                assert np.array_equal(plain[i], _want((layout, i), pictures[i], rects[i] if rects else WHOLE, ow, oh, 3)), (layout, ow, i)
            for flags in (ALTERNATE, [True] * n):
                arena = NormArena(n, ow, oh, 3, planar, N.U8, base=j)
                assert arena.call(d, rects, None, flags) == [0] * n
                arena.check([p[:, ::-1] if f else p for p, f in zip(plain, flags)], what=f"{layout} u8 width {ow} {flags}")
                assert d.ragged_normalized_stats() == dict(sample=N.U8, mirrored=sum(flags))
                arena = NormArena(n, ow, oh, 3, planar, N.F16, base=j + 1)
                assert arena.call(d, rects, N.IMAGENET, flags) == [0] * n
                arena.check([_norm((layout, i), pictures[i], rects[i] if rects else WHOLE, ow, oh, 3, N.F16, N.IMAGENET, flags[i]) for i in range(n)],
                            what=f"{layout} f16 width {ow} {flags}")
                assert d.ragged_normalized_stats() == dict(sample=N.F16, mirrored=sum(flags))
                assert d.ragged_resized_stats()["resample_launches"] == 1


# ------------------------------------------------------------------------------------------------ 3: uint8 through the new call
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_uint8_without_mirror_is_the_resized_call(lists, planar):
    """MIJPEG_SAMPLE_U8, nobody mirrored (NULL flags, and flags that are all 0): the resized call's tensor, byte for byte, and its
    statistics."""
    import torch

    for layout in LAYOUTS:
        d, pictures = lists[layout]
        n = len(pictures)
        channels = 1 if layout == "grey" else 3
        rects = [(1, 2, w - 2, h - 1) for w, h in SIZES]
        for ow, oh in [(64, 17), (224, 224), (37, 5)]:
            old = NormArena(n, ow, oh, channels, planar, N.U8, base=1)
            assert old.call_resized(d, rects) == [0] * n
            old_stats = d.ragged_resized_stats()
            for flags in (None, [False] * n):
                new = NormArena(n, ow, oh, channels, planar, N.U8, base=1)
                assert new.call(d, rects, None, flags) == [0] * n
                assert torch.equal(old.dev, new.dev), (layout, ow, oh)
                assert d.ragged_resized_stats() == old_stats and d.ragged_normalized_stats() == dict(sample=N.U8, mirrored=0)
            old.check([_want((layout, i), pictures[i], rects[i], ow, oh, channels) for i in range(n)], what=f"{layout} -> {ow} x {oh}")


# ------------------------------------------------------------------------------------------------ 4: launches
@pytest.mark.gpu
def test_one_resample_launch_whatever_the_type(oracle, lists):
    """resample_launches == 1 for lists of 1, 2 and 5 pictures, for every sample type, with and without mirror flags; window_launches is
    the resized call's for the same rectangles."""
    streams = _layout_list("420")
    for count in (1, 2, len(streams)):
        if count == len(streams):
            d, own = lists["420"][0], False
        else:
            d, own = api.Decoder(0), True
        try:
            if own:
                assert d.decode_ragged_device(list(streams[:count])) == [0] * count
            rects = [(w // 4, h // 5, w - 2, h - 1) for w, h in SIZES[:count]]
            old = NormArena(count, 33, 17, 3, True, N.U8)
            assert old.call_resized(d, rects) == [0] * count
            want = d.ragged_resized_stats()
            assert want["resample_launches"] == 1 and want["window_launches"] >= 1 and want["resampled"] == count, want
            for sample in (N.U8, N.F32, N.F16, N.BF16):
                for flags in (None, ALTERNATE[:count]):
                    arena = NormArena(count, 33, 17, 3, True, sample)
                    assert arena.call(d, rects, N.IMAGENET if sample else None, flags) == [0] * count
                    assert d.ragged_resized_stats() == want, (count, sample, flags)
                    assert d.ragged_normalized_stats() == dict(sample=sample, mirrored=sum(flags) if flags else 0)
        finally:
            if own:
                d.close()


# ------------------------------------------------------------------------------------------------ 5: refusals
@pytest.mark.gpu
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_refused_slots_stay_untouched(oracle, planar):
    """A 12-bit picture, a CMYK picture and a damaged stream beside three served ones: the resized call's status values; the refused
    slots and everything around the slots are still 0xA5, in the float types as well; `mirrored` counts served pictures only."""
    garbage = bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8))
    streams = [_layout_list("420")[4], golden_jpeg("p12_120x90_420_dri3"), golden_jpeg("pilprog_200x130_422"), golden_jpeg("pil_90x60_cmyk"), garbage,
               _layout_list("grey")[3]]
    served = [0, 2, 5]
    pictures = {i: _expected(oracle, streams[i], 8) for i in served}
    n = len(streams)
    rects = [(130, 129, EDGE, EDGE), WHOLE, (7, 9, 150, 100), WHOLE, WHOLE, (1, 1, 200, 38)]
    flags = [True, True, False, True, True, True]
    d = api.Decoder(0)
    try:
        decode = d.decode_ragged_device(streams, with_12bit=True)
        old = NormArena(n, 64, 48, 3, planar, N.U8)
        status = old.call_resized(d, rects)
        assert status == [0, api.ERR_NOT_IMPLEMENTED, 0, api.ERR_NOT_IMPLEMENTED, decode[4], 0] and decode[4] != 0
        old_stats = d.ragged_resized_stats()
        for k, sample in enumerate((N.F32, N.F16, N.BF16, N.U8)):
            arena = NormArena(n, 64, 48, 3, planar, sample, base=k)
            assert arena.call(d, rects, N.CRAFTED if sample else None, flags) == status
            arena.check([_norm(("refused", i), pictures[i], rects[i], 64, 48, 3, sample, N.CRAFTED, flags[i]) if i in served else None for i in range(n)],
                        what=f"sample {sample}")
            assert d.ragged_resized_stats() == old_stats and old_stats["resampled"] == 3 and old_stats["refused"] == 3
            assert d.ragged_normalized_stats() == dict(sample=sample, mirrored=2)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 6: parameter errors
@pytest.mark.gpu
def test_parameter_errors_write_and_count_nothing(lists):
    """Every new invalid-parameter case through raw ctypes: the error, status and tensor untouched, both statistics those of the call
    before."""
    d, pictures = lists["420"]
    n = len(pictures)
    first = NormArena(n, 20, 10, 3, True, N.F16)
    assert first.call(d, None, N.IMAGENET, ALTERNATE) == [0] * n
    before, nbefore = d.ragged_resized_stats(), d.ragged_normalized_stats()
    assert before["resampled"] == n and nbefore == dict(sample=N.F16, mirrored=3)
    fn = api.lib().mijpeg_reconstruct_ragged_normalized_device
    inf, nan = float("inf"), float("nan")

    def fmt(sample, reserved=0, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
        f = api.MijpegBatchFormat()
        f.sample, f.reserved = sample, reserved
        f.scale[:], f.bias[:] = scale, bias
        return f

    for sample in (N.F32, N.F16, N.BF16):
        es = api.SAMPLE_BYTES[sample]
        for planar in (True, False):
            arena = NormArena(n, 20, 10, 3, planar, sample)
            ptr = arena.dev.data_ptr() + arena.at
            good = dict(format=fmt(sample), channels=3, dst=ptr, image=arena.image, plane=arena.plane, row=arena.row)
            cases = {"dst one byte off": dict(dst=ptr + 1), "image_stride one byte more": dict(image=arena.image + 1), "row_stride one byte more": dict(row=arena.row + 1),
                     "scale inf": dict(format=fmt(sample, scale=(1.0, inf, 1.0))), "scale nan": dict(format=fmt(sample, scale=(nan, 1.0, 1.0))),
                     "bias -inf": dict(format=fmt(sample, bias=(0.0, 0.0, -inf))), "bias nan": dict(format=fmt(sample, bias=(0.0, nan, 0.0))),
                     "sample -1": dict(format=fmt(-1)), "sample 4": dict(format=fmt(4)), "reserved 1": dict(format=fmt(sample, reserved=1)), "NULL format": dict(format=None),
                     "row below a line of elements": dict(row=arena.line - es)}
            lines = 9 * arena.row + arena.line  # (what a plane, or an interleaved slot, spans)
            cases["image below a slot of elements"] = dict(image=(2 * arena.plane if planar else 0) + lines - es)
            if planar:
                cases["plane_stride one byte more"] = dict(plane=arena.plane + 1)
                cases["plane below its lines of elements"] = dict(plane=lines - es)
            if es == 4:
                cases.update({"dst two bytes off": dict(dst=ptr + 2), "row_stride two bytes more": dict(row=arena.row + 2), "image_stride two bytes more": dict(image=arena.image + 2)})
            for name, change in cases.items():
                a = dict(good, **change)
                status = (C.c_int32 * n)(*[77] * n)
                rc = fn(d._h, None, 20, 10, a["channels"], C.byref(a["format"]) if a["format"] is not None else None, a["dst"], a["image"], a["plane"], a["row"], 0,
                        status, 1)
                assert rc == api.ERR_INVALID_PARAMETER, (name, sample, planar)
                assert list(status) == [77] * n, name
                arena.check([None] * n, what=name)
                assert d.ragged_resized_stats() == before and d.ragged_normalized_stats() == nbefore, name
    # what is no error: constants behind `channels`, and any constants with uint8 samples -- served, status == NULL included
    d1, grey = lists["grey"]
    arena = NormArena(len(grey), 20, 10, 1, True, N.F32)
    f = fmt(N.F32, scale=(0.5, nan, inf), bias=(1.0, inf, nan))
    assert fn(d1._h, None, 20, 10, 1, C.byref(f), arena.dev.data_ptr() + arena.at, arena.image, arena.plane, arena.row, 0, None, 1) == 0
    arena.check([_norm(("grey", i), grey[i], WHOLE, 20, 10, 1, N.F32, ((np.float32(0.5),), (np.float32(1.0),))) for i in range(len(grey))], what="one channel")
    arena = NormArena(n, 20, 10, 3, False, N.U8)
    f = fmt(N.U8, scale=(nan, nan, nan), bias=(inf, inf, inf))
    assert fn(d._h, None, 20, 10, 3, C.byref(f), arena.dev.data_ptr() + arena.at, arena.image, arena.plane, arena.row, 0, None, 1) == 0
    arena.check([_want(("420", i), pictures[i], WHOLE, 20, 10, 3) for i in range(n)], what="uint8 samples")
    assert d.ragged_normalized_stats() == dict(sample=N.U8, mirrored=0)


# ------------------------------------------------------------------------------------------------ 7: two calls in flight
@pytest.mark.gpu
def test_two_calls_without_sync(lists):
    """Two calls with sync=0 back to back on one decode -- other types, other mirror sets, other rectangles and sizes -- and one wait:
    both exact, so the first call's pinned tables (its reversed columns among them) were not overwritten on their way up."""
    d, pictures = lists["420"]
    n = len(pictures)
    first = [WHOLE] * n
    second = [(w // 3, h // 2, w - 1, h - 2) if h > 2 else WHOLE for w, h in SIZES]
    m1, m2 = ALTERNATE, [not f for f in ALTERNATE]
    a1, a2 = NormArena(n, 224, 224, 3, True, N.F32, base=1), NormArena(n, 31, 45, 3, False, N.BF16, base=2)
    api._foreign_work_done()  # (the arenas' fills: the calls below do not wait for other streams)
    assert a1.call(d, first, N.IMAGENET, m1, sync=False, wait_foreign=False) == [0] * n
    assert a2.call(d, second, N.CRAFTED, m2, sync=False, wait_foreign=False) == [0] * n
    d.synchronize()
    a1.check([_norm(("420", i), pictures[i], first[i], 224, 224, 3, N.F32, N.IMAGENET, m1[i]) for i in range(n)], what="first call")
    a2.check([_norm(("420", i), pictures[i], second[i], 31, 45, 3, N.BF16, N.CRAFTED, m2[i]) for i in range(n)], what="second call")
    assert d.ragged_normalized_stats() == dict(sample=N.BF16, mirrored=2)


# ------------------------------------------------------------------------------------------------ 8: batch.decode_resized
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_decode_resized_float16(oracle, layout):
    """dtype=torch.float16 with ImageNet's constants, crops and mirror flags: the model's bit patterns; rank 1 of 2 picks its own mirror
    entries; the defaults still return today's uint8 tensor."""
    import torch

    from libjpeg_amd import batch

    garbage = bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8))
    streams = [_layout_list("420")[4], _layout_list("grey")[2], garbage, _layout_list("444")[3], _layout_list("422")[1], golden_jpeg("pil_90x60_cmyk")]
    crops = [(10, 20, 224, 224), None, None, (128, 3, 500, 500), (5, 5, 50, 40), None]  # (x, y, w, h)
    mirror = [True, True, True, False, True, False]
    served = [0, 1, 3, 4]
    pictures = {i: _expected(oracle, streams[i], 8) for i in served}
    consts = N.constants(N.IMAGENET_MEAN, N.IMAGENET_STD)

    def want(i, sample, flag):
        c = crops[i] or (0, 0, EDGE, EDGE)
        rect = (c[0], c[1], min(EDGE, c[0] + c[2] - 1), min(EDGE, c[1] + c[3] - 1))
        r = _norm(("resized", i), pictures[i], rect, 56, 48, 3, sample, consts if sample else None, flag)
        return r.transpose(2, 0, 1) if layout == "chw" else r

    def bits(t):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)

    d = api.Decoder(0)
    try:
        out, errors = batch.decode_resized(streams, (48, 56), crops=crops, layout=layout, decoder=d, dtype=torch.float16, mean=N.IMAGENET_MEAN, std=N.IMAGENET_STD,
                                           mirror=mirror)
        assert out.dtype == torch.float16 and tuple(out.shape) == ((6, 3, 48, 56) if layout == "chw" else (6, 48, 56, 3))
        got = bits(out)
        for i in range(6):
            if i in served:
                assert errors[i] is None and np.array_equal(got[i], want(i, N.F16, mirror[i])), i
            else:
                assert isinstance(errors[i], api.MijpegError) and not got[i].any(), i
        assert d.ragged_resized_stats()["resample_launches"] == 1 and d.ragged_normalized_stats() == dict(sample=N.F16, mirrored=3)
        # world = 2, rank 1: pictures 1, 3, 5 in slots 0, 1, 2 with the flags of 1, 3, 5
        part, perr = batch.decode_resized(streams, (48, 56), crops=crops, layout=layout, rank=1, world=2, decoder=d, dtype=torch.float16, mean=N.IMAGENET_MEAN,
                                          std=N.IMAGENET_STD, mirror=[False, True, False, False, True, True])
        assert part.shape[0] == 3 and [e is None for e in perr] == [True, True, False]
        assert np.array_equal(bits(part)[0], want(1, N.F16, True)) and np.array_equal(bits(part)[1], want(3, N.F16, False))
        assert d.ragged_normalized_stats() == dict(sample=N.F16, mirrored=1)
        # one mean and one std for all channels, float32 and bfloat16
        for dtype, sample, view in ((torch.float32, N.F32, torch.int32), (torch.bfloat16, N.BF16, torch.int16)):
            one, _ = batch.decode_resized(streams[:2], (48, 56), crops=crops[:2], layout=layout, decoder=d, dtype=dtype, mean=0.5, std=0.25)
            assert one.dtype == dtype
            flat = N.constants((0.5,) * 3, (0.25,) * 3)
            for i in range(2):
                c = crops[i] or (0, 0, EDGE, EDGE)
                r = _norm(("resized", i), pictures[i], (c[0], c[1], min(EDGE, c[0] + c[2] - 1), min(EDGE, c[1] + c[3] - 1)), 56, 48, 3, sample, flat)
                assert np.array_equal(one[i].view(view).cpu().numpy().view(N.ELEMENT[sample]), r.transpose(2, 0, 1) if layout == "chw" else r), (dtype, i)
        # the defaults: today's uint8 tensor through the resized call; mirror alone keeps uint8
        plain, _ = batch.decode_resized(streams, (48, 56), crops=crops, layout=layout, decoder=d)
        assert plain.dtype == torch.uint8 and d.ragged_normalized_stats() == dict(sample=N.U8, mirrored=0)
        flipped, _ = batch.decode_resized(streams, (48, 56), crops=crops, layout=layout, decoder=d, mirror=mirror)
        assert flipped.dtype == torch.uint8 and d.ragged_normalized_stats() == dict(sample=N.U8, mirrored=3)
        for i in served:
            assert np.array_equal(plain[i].cpu().numpy(), want(i, N.U8, False)), i
            assert np.array_equal(flipped[i].cpu().numpy(), want(i, N.U8, mirror[i])), i
    finally:
        d.close()

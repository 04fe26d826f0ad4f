"""Ragged decode of lists that mix 8-bit and 12-bit pictures in one device pass (mijpeg_decode_ragged_device16 +
mijpeg_reconstruct_ragged_device, Decoder.decode_ragged_device(with_12bit=True), batch.decode_mixed(with_12bit=True)):
every picture against the oracle, exactly; nothing written outside a picture; the statistics show that the 12-bit layout groups'
launches really ran, and the call without the 12-bit groups still does what it did.

12-bit streams come from synth.to_12bit (an 8-bit stream's entropy coded data under deltas times `scale`), from the reference's
12-bit encoder (tests/golden/enc12) and from this library's own (tables of the picture's own, categories above 11)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import enc12_util as U
from conftest import golden_jpeg
from libjpeg_amd import api, batch, synth
from test_ragged_batch import _flavour, _reconstruct_guarded

pytestmark = pytest.mark.gpu

FUSED12 = ("fused420_kernel<12>", "fused422_12_kernel", "fused444_12_kernel", "fused1_kernel<12>")  # (+ "/narrow")
NEW_REASON = "no layout group for this frame: 8-bit and 12-bit sequential 4:2:0, 4:2:2, 4:4:4 and grey frames have one"
PADS = (0, 4, 14)  # bytes behind a line: even, so that 16-bit samples stay aligned


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _jpeg8(w, h, seed, quality, layout, dri, optimize=False):
    img = synth.synth_image(w, h, seed, channels=1 if layout == "grey" else 3)
    return synth.encode_jpeg(img, quality, "444" if layout == "grey" else layout, dri, optimize=optimize)


def _own12(dec, w, h, seed, quality, layout, dri):
    """This library's 12-bit encoder on an 8-bit test picture widened to 12 bits (x * 16 + x / 16: 0..4095): tables of its own, ranges
    like the same picture's through to_12bit(.., 16).  (No noise in the low bits: a stream without restart markers that is all
    noise does not let the device walk settle, at either precision -- test_ragged_batch.test_every_interval_source_in_one_group.)"""
    nc = 1 if layout == "grey" else 3
    img8 = synth.synth_image(w, h, seed, channels=nc).astype(np.uint16)
    img = img8 * 16 + (img8 >> 4)
    img = np.ascontiguousarray(img[..., 0] if nc == 1 else img)
    return dec.encode(img, quality, "444" if layout == "grey" else layout, dri)


def _expected(oracle, streams, precisions):
    with ThreadPoolExecutor(16) as ex:  # (ctypes releases the GIL)
        return list(ex.map(lambda sp: oracle.decode16(sp[0]) if sp[1] == 12 else oracle.decode(sp[0]), zip(streams, precisions)))


def _same(pic, exp):
    return pic.shape == exp.shape and pic.dtype.itemsize == exp.dtype.itemsize and np.array_equal(pic, exp)


def _is_fused12(info):
    return _flavour(info)[0].split("/")[0] in FUSED12


# ------------------------------------------------------------------------------------------------ 3: the mixed list
SHAPES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (127, 129), (128, 128), (129, 127), (333, 200), (640, 480)]
LAYOUT_NAMES = ("420", "444", "422", "grey")


def _mixed_list(dec):
    """10 shapes x 4 layouts x {8, 12} bit.  DRI 0 / 1 / 4 cycles against shape, layout and precision, so every one of the eight groups
    holds all three (and its small members without restart markers are one interval: WholeScan).  12-bit members: this library's
    encoder on even shapes, to_12bit at scale 16 and 32 (inside and outside the one-sum colour bound, both inside the 12-bit gates)
    on odd ones -- and on every member that the device walks (no restart markers, 128 x 128 and up): a 12-bit picture coded at these
    qualities without restart markers is data of so high a rate that the walk does not settle within its rounds, which refuses the
    group's launch as noise does at 8 bits (test_ragged_batch.test_every_interval_source_in_one_group); what is walked here is the
    entropy coded data of an 8-bit stream under 12-bit tables."""
    jobs, streams = [], []
    for si, (w, h) in enumerate(SHAPES):
        for li, layout in enumerate(LAYOUT_NAMES):
            for p in (8, 12):
                dri = (0, 1, 4)[(si + li + (p == 12)) % 3]
                q = (50, 85, 95)[(si + li) % 3]
                seed = 1200 + (si * 4 + li) * 2 + (p == 12)
                if p == 8:
                    s = _jpeg8(w, h, seed, q, layout, dri, optimize=(si + li) % 2 == 1)
                elif si % 2 == 0 and (dri != 0 or w * h < 128 * 128):
                    s = _own12(dec, w, h, seed, q, layout, dri)
                else:
                    scale = 16 if (si // 2) % 2 == 0 else 32
                    s = synth.to_12bit(_jpeg8(w, h, seed, q if scale == 16 else max(q, 85), layout, dri), scale)  # (deltas stay <= 2047: the 12-bit kernels' gate)
                jobs.append((w, h, layout, p, dri))
                streams.append(s)
    return streams, jobs


def test_the_mixed_precision_list(dec, oracle):
    """80 streams in ONE decode call and ONE reconstruct call: every picture equals the oracle's, nothing outside a picture is written,
    no fallback, at most eight Huffman launches, no picture reconstructed on its own, and one reconstruction launch per (group, kernel,
    flavour) that the pictures' own range checks select."""
    streams, jobs = _mixed_list(dec)
    n = len(streams)
    assert n == 80
    for layout in LAYOUT_NAMES:
        for p in (8, 12):
            assert {j[4] for j in jobs if j[2] == layout and j[3] == p} == {0, 1, 4}
    exp = _expected(oracle, streams, [j[3] for j in jobs])
    d = api.Decoder(0)
    status = d.decode_ragged_device(streams, with_12bit=True)
    assert status == [0] * n
    infos = [d.ragged_info(i) for i in range(n)]
    for f, (w, h, layout, p, _) in zip(infos, jobs):
        assert (f.width, f.height, f.precision, f.sample_bytes) == (w, h, p, 2 if p == 12 else 1)
    assert [d.ragged_route(i) for i in range(n)] == [(True, None)] * n
    pics, touched = _reconstruct_guarded(d, infos, PADS)
    st = d.ragged_stats()
    print("ragged stats:", st)
    flavours = {(jobs[i][2], jobs[i][3]) + _flavour(infos[i]) for i in range(n)}
    print("flavours:", sorted(flavours))
    bad = [jobs[i] for i in range(n) if not _same(pics[i], exp[i])]
    assert not bad, bad
    assert not any(touched), [jobs[i] for i in range(n) if touched[i]]
    assert st["images"] == n and st["ragged"] == n and st["fallbacks"] == 0 and st["errors"] == 0, st
    assert 8 == len({(j[2], j[3]) for j in jobs}) and 1 <= st["entropy_launches"] <= 8, st
    assert st["walk_launches"] > 0  # (640 x 480 without restart markers is walked in every group that has it)
    assert st["recon_single"] == 0, [(jobs[i], _flavour(infos[i])) for i in range(n) if jobs[i][3] == 12 and not _is_fused12(infos[i])]
    assert st["recon_launches"] == len(flavours), (st, sorted(flavours))
    assert {fl[:2] for fl in flavours} == {(layout, p) for layout in LAYOUT_NAMES for p in (8, 12)}
    d.close()


# ------------------------------------------------------------------------------------------------ 4: flavour split and outlier
def test_colour_flavours_and_an_outlier_in_one_12bit_group(oracle):
    """Three 12-bit 4:2:0 pictures of different sizes: inside the one-sum colour bound, outside it but inside the 12-bit gates, beyond the
    gates (luma sum |c| q >= 49152).  One Huffman launch decodes all three; the first two get a ragged launch each, the third is
    reconstructed by a launch of its own."""
    noise = np.random.default_rng(63).integers(0, 256, (127, 129, 3)).astype(np.uint8)
    streams = [synth.to_12bit(synth.synth_jpeg(272, 144, 61, 85, "420", 0), 16), synth.to_12bit(synth.synth_jpeg(200, 136, 62, 95, "420", 4), 32),
               synth.to_12bit(synth.encode_jpeg(noise, 99, "420", restart_mcus=1), 16)]
    exp = _expected(oracle, streams, [12] * 3)
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams, with_12bit=True) == [0] * 3
    infos = [d.ragged_info(i) for i in range(3)]
    # the precondition: the range checks name the three kernels
    names = [_flavour(f)[0] for f in infos]
    assert names[:2] == ["fused420_kernel<12>/narrow", "fused420_kernel<12>"] and names[2].split("/")[0] not in FUSED12, (names, [list(f.range_max) for f in infos])
    assert infos[2].range_max[0] >= 49152 and max(infos[1].range_max[:3]) < 45056
    assert [d.ragged_route(i) for i in range(3)] == [(True, None)] * 3
    pics, touched = _reconstruct_guarded(d, infos, PADS)
    st = d.ragged_stats()
    assert st["ragged"] == 3 and st["fallbacks"] == 0 and st["entropy_launches"] == 1 and st["recon_launches"] == 2 and st["recon_single"] == 1, st
    for i in range(3):
        assert _same(pics[i], exp[i]), i
    assert not any(touched)
    d.close()


def test_device_walk_on_a_12bit_stream_with_tables_of_its_own(dec, oracle):
    """A 256 x 256 4:4:4 picture from this library's 12-bit encoder, no restart markers, at a quality whose rate the walk settles on
    (about 20 bytes per block: profiles/ragged_decode12.txt, section 4): walked on the device inside its group, exact."""
    s = _own12(dec, 256, 256, 77, 30, "444", 0)
    d = api.Decoder(0)
    assert d.decode_ragged_device([s], with_12bit=True) == [0]
    st = d.ragged_stats()
    assert d.ragged_route(0) == (True, None) and st["ragged"] == 1 and st["entropy_launches"] == 1 and st["walk_launches"] > 0, (d.ragged_route(0), st)
    f = d.ragged_info(0)
    pics, touched = _reconstruct_guarded(d, [f], PADS)
    assert _same(pics[0], oracle.decode16(s)) and not any(touched)
    d.close()


# ------------------------------------------------------------------------------------------------ 5: reference-written streams
def test_the_reference_written_12bit_streams_as_one_list(oracle):
    keys = sorted(U.CASES)
    streams = [U.golden_stream(k) for k in keys]
    assert len(streams) == 14
    exp = _expected(oracle, streams, [12] * 14)
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams, with_12bit=True) == [0] * 14
    infos = [d.ragged_info(i) for i in range(14)]
    grouped = [U.CASES[k][2] in ("420", "422", "444", "grey") for k in keys]
    assert sum(grouped) == 11
    for i, k in enumerate(keys):
        assert d.ragged_route(i) == ((True, None) if grouped[i] else (False, NEW_REASON)), k
    pics, touched = _reconstruct_guarded(d, infos, PADS)
    for i, k in enumerate(keys):
        assert _same(pics[i], exp[i]), k
    assert not any(touched)
    st = d.ragged_stats()
    # group members the 12-bit kernels do not take -- the identity (-c) stream, deltas beyond 2047 at quality 2 -- are reconstructed singly
    alone = [k for i, k in enumerate(keys) if grouped[i] and not _is_fused12(infos[i])]
    assert "444_41x23_identity" in alone and not infos[keys.index("444_41x23_identity")].ycbcr
    flavours = {(U.CASES[k][2],) + _flavour(infos[i]) for i, k in enumerate(keys) if grouped[i] and k not in alone}
    assert st["images"] == 14 and st["ragged"] == 11 and st["fallbacks"] == 3 and st["errors"] == 0, st
    assert st["entropy_launches"] == 4 and st["recon_single"] == len(alone) and st["recon_launches"] == len(flavours), (st, alone, sorted(flavours))
    d.close()


# ------------------------------------------------------------------------------------------------ 6: either call, same pictures
def test_either_call_gives_the_same_pictures(dec, oracle):
    """8-bit and 12-bit pictures, a progressive one, CMYK, a truncated 12-bit stream and garbage through mijpeg_decode_ragged_device and
    through mijpeg_decode_ragged_device16: status codes, warnings and pictures are the same member by member; the old call's routes and
    statistics are what they were (every 12-bit member alone), the new call's show the 12-bit groups."""
    p12 = [synth.to_12bit(_jpeg8(120, 90, 4, 85, "420", 0), 16), _own12(dec, 200, 136, 5, 85, "444", 4), U.golden_stream("grey_70x50"),
           synth.to_12bit(_jpeg8(333, 200, 6, 95, "422", 1), 16), dec.encode(U.block_checker(64, 40), 100, "444", 0)]  # (DC differences of category 15)
    p8 = [_jpeg8(640, 480, 40, 85, "420", 4), _jpeg8(127, 129, 41, 85, "444", 0), _jpeg8(333, 200, 42, 50, "grey", 1), _jpeg8(129, 127, 43, 95, "422", 0)]
    whole = synth.to_12bit(_jpeg8(272, 144, 7, 85, "420", 2), 16)
    truncated = whole[:len(whole) * 2 // 3]
    garbage = bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8))
    streams = [p8[0], p12[0], synth.synth_jpeg(200, 130, 3, 85, "420", 0, progressive=True), p12[1], p8[1], golden_jpeg("pil_90x60_cmyk"), p12[2], truncated,
               p8[2], p12[3], garbage, p8[3], p12[4]]
    kinds = ["p8", "p12", "other", "p12", "p8", "other", "p12", "truncated", "p8", "p12", "garbage", "p8", "p12"]
    n = len(streams)

    def run(with_12bit):
        d = api.Decoder(0)
        status = d.decode_ragged_device(streams, with_12bit=with_12bit)
        infos = [d.ragged_info(i) if status[i] == 0 else None for i in range(n)]
        pics, touched = _reconstruct_guarded(d, infos, PADS)
        assert not any(touched)
        res = status, pics, [d.ragged_warning(i) for i in range(n)], [d.ragged_route(i) for i in range(n)], d.ragged_stats()
        d.close()
        return res

    old_status, old_pics, old_warn, old_route, old_st = run(False)
    new_status, new_pics, new_warn, new_route, new_st = run(True)
    assert old_status == new_status and old_status[kinds.index("garbage")] < 0
    assert all(s == 0 for s, k in zip(old_status, kinds) if k in ("p8", "p12", "other"))
    assert old_warn == new_warn
    for i in range(n):
        assert (old_pics[i] is None) == (new_pics[i] is None) == (old_status[i] != 0), (i, kinds[i])
        if old_pics[i] is not None:
            assert _same(old_pics[i], new_pics[i]), (i, kinds[i])
            if kinds[i] != "truncated":
                exp = oracle.decode16(streams[i]) if kinds[i] == "p12" else oracle.decode(streams[i])
                assert _same(new_pics[i], exp), (i, kinds[i])
    errors = sum(s != 0 for s in old_status)
    # the old call, as ever: the 8-bit pictures in their groups, every 12-bit one on the single-image route
    assert [r[0] for r in old_route] == [k == "p8" for k in kinds]
    assert all(old_route[i][1] == "on-device entropy decoding: 8-bit frames (12-bit residual frames of JPEG XT) only" for i in range(n) if kinds[i] == "p12")
    assert old_st["images"] == n and old_st["ragged"] == 4 and old_st["fallbacks"] == n - 4 and old_st["errors"] == errors and old_st["entropy_launches"] == 4, old_st
    # the new one: the 12-bit pictures in theirs; everything else unchanged, reason by reason ("no layout group" names both precisions)
    assert [r[0] for r in new_route] == [k in ("p8", "p12") for k in kinds]
    old_reason = "no layout group for this frame: 8-bit sequential 4:2:0, 4:2:2, 4:4:4 and grey frames have one"
    assert old_route[5] == (False, old_reason) and new_route[5] == (False, NEW_REASON)  # (CMYK)
    for i in range(n):
        if kinds[i] not in ("p12", "truncated") and i != 5:
            assert new_route[i] == old_route[i], (i, kinds[i])
    assert new_st["images"] == n and new_st["ragged"] == 9 and new_st["fallbacks"] == n - 9 and new_st["errors"] == errors and new_st["entropy_launches"] == 8, new_st


# ------------------------------------------------------------------------------------------------ 7: round trip
def test_encode_mixed_then_decode_mixed(oracle):
    """batch.encode_mixed on 8-bit and 12-bit pictures alternating, then batch.decode_mixed(with_12bit=True): the tensors are the oracle's
    decode of the streams, and no picture left its group."""
    import torch

    cases = [(64, 64, "420", 0), (400, 300, "444", 4), (131, 77, "444", 0), (257, 129, "420", 4), (320, 240, "420", 0), (64, 40, "444", 0), (399, 65, "444", 4),
             (200, 400, "420", 4)]
    imgs = []
    for i, (w, h, _, _) in enumerate(cases):
        if i % 2 == 0:
            imgs.append(synth.synth_image(w, h, 300 + i))
        elif i == 5:
            imgs.append(U.block_checker(w, h))  # (quality 100 below: DC differences of category 15)
        else:
            imgs.append(U.synth12(w, h, 300 + i))
    tensors = [torch.from_numpy(im.view(np.int16) if im.dtype == np.uint16 else im).cuda() for im in imgs]
    d = api.Decoder(0)
    streams = batch.encode_mixed(tensors, [100 if i == 5 else 85 for i in range(len(cases))], [c[2] for c in cases], [c[3] for c in cases], decoder=d)
    precisions = [12 if i % 2 else 8 for i in range(len(cases))]
    exp = _expected(oracle, streams, precisions)
    out = batch.decode_mixed(streams, 0, decoder=d, with_12bit=True)
    st = d.ragged_stats()
    for i, (t, e) in enumerate(zip(out, exp)):
        assert str(t.device).startswith("cuda") and t.dtype == (torch.int16 if precisions[i] == 12 else torch.uint8), i
        got = t.cpu().numpy()
        assert _same(got.view(np.uint16) if precisions[i] == 12 else got, e), (i, cases[i])
    assert st["images"] == len(cases) and st["ragged"] == len(cases) and st["fallbacks"] == 0 and st["errors"] == 0 and st["entropy_launches"] <= 4, st
    # without the flag the same list gives the same tensors, the 12-bit ones one by one
    again = batch.decode_mixed(streams, 0, decoder=d)
    assert d.ragged_stats()["fallbacks"] == len(cases) // 2
    for a, b in zip(again, out):
        assert torch.equal(a, b)
    d.close()

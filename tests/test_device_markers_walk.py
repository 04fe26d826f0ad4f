"""Device marker route for streams without restart markers on the GPU (mijpeg_set_device_markers): the primitive
with one expected interval against its reference model, single images whose copy is shorter than the raw segment the walk was
sized from, the corruptions that make the route decline inside the call, and uniform batches that mix streams with and without
restart markers.
"""
import ctypes as C

import numpy as np
import pytest

import markers_model as M
from libjpeg_amd import api, batch
from test_device_markers import _batch_pixels, check, plain
from test_device_markers_cpu import host_search
from test_device_markers_walk_cpu import WALK_STREAMS, textured_stream, walk_stream

pytestmark = pytest.mark.gpu

LANE, CHUNK = 16, 4096  # bytes of a lane, of a workgroup (markers.hpp)
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5]


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def streams():
    return {key: walk_stream(*key) for key in WALK_STREAMS}


# ------------------------------------------------------------------------------------------------ 1. the primitive, expect = 1
def _check1(dec, seg):
    """check() plus what it leaves out: end[0] and the guard bytes behind a destination of the segment's own size."""
    seg = bytes(seg)
    m, r = check(dec, seg, 1, capacity=len(seg))
    if m["flags"] == 0:
        assert list(r["begin"]) == [0] and list(r["end"]) == [m["total"]]
    L = api.lib()
    cap = len(seg)
    dst = np.full(cap + 32, 0xA5, np.uint8)
    begin, end = np.full(9, 0xA5A5A5A5, np.uint32), np.full(9, 0xA5A5A5A5, np.uint32)
    term, flags = C.c_uint32(), C.c_uint32()
    total = L.mijpeg_device_marker_search(dec._h, seg, len(seg), 1, dst[16:].ctypes.data, cap, begin[4:].ctypes.data, end[4:].ctypes.data, C.byref(term),
                                          C.byref(flags))
    assert total >= 0 and (flags.value, term.value) == (m["flags"], m["term"])  # (a device copy's guard bytes: MIJPEG_ERR_PHASE_ERROR)
    assert (dst[:16] == 0xA5).all() and (dst[16 + cap:] == 0xA5).all()
    for t in (begin, end):
        assert (t[:4] == 0xA5A5A5A5).all() and (t[5:] == 0xA5A5A5A5).all()
    if m["flags"] == 0:
        assert total == m["total"] and begin[4] == 0 and end[4] == m["total"]
        assert bytes(dst[16:16 + total]) == m["kept"] and not dst[16 + total:16 + cap].any()
    return m


@pytest.mark.parametrize("n", SIZES)
def test_primitive_with_one_expected_interval(dec, n):
    rng = np.random.default_rng(n)
    base = plain(rng, n)
    if n >= 2:
        base[-2:] = b"\xff\xd9"
    m = _check1(dec, base)
    assert m["flags"] == (0 if n >= 2 else M.NO_END) and m["term"] == (n - 2 if n >= 2 else n)
    # FF 00 across every lane and chunk boundary the segment has (the FF last in its lane, the 00 first in the next)
    edges = list(range(LANE, n - 2, LANE))
    seg = bytearray(base)
    for e in edges:
        seg[e - 1:e + 1] = b"\xff\x00"
    m = _check1(dec, seg)
    if n >= 2:
        assert m["flags"] == 0 and m["total"] == n - 2 - len(edges)
    # ... and a pair that starts one byte later, across the same boundaries
    seg = bytearray(base)
    for e in edges:
        if e + 2 <= n - 2:
            seg[e:e + 2] = b"\xff\x00"
    assert _check1(dec, seg)["flags"] == (0 if n >= 2 else M.NO_END)
    # a lone FF as the last byte: NO_END
    seg = bytearray(plain(rng, n))
    seg[-1] = 0xFF
    m = _check1(dec, seg)
    assert m["flags"] == M.NO_END and m["term"] == n
    if n >= 15:
        for at in sorted({1, n // 2, n - 6}):
            # one FF D0 inside: COUNT (one marker, two intervals, one expected)
            seg = bytearray(base)
            seg[at:at + 3] = b"\xff\xd0\x55"
            assert _check1(dec, seg)["flags"] == M.COUNT, at
            # FF FF: FILL (in front of an ordinary byte the second FF ends the segment there)
            seg = bytearray(base)
            seg[at:at + 3] = b"\xff\xff\x55"
            m = _check1(dec, seg)
            assert m["flags"] == M.FILL and m["term"] == at + 1, at


# ------------------------------------------------------------------------------------------------ 2. single images
# mijpeg_decode_coefficients_device keeps the host's search for a stream without restart markers (tests/test_device_markers.py pins
# that for the option: "no restart markers" among its declines), so a single image goes through the uniform batch call as a batch of
# one.  That call hands out no coefficient planes: what is compared is every pixel -- against the option-off call and against the
# oracle -- and the range check, which is taken over the coefficients, against the option-off call's and the host decoder's.
def _planes(d, data):
    f = d.read(data, entropy="gpu")
    assert d.entropy_used == "gpu"
    return f, [d.coefficients(c).copy() for c in range(f.components)]


def _batch_outcome(d, streams):
    """(return code, what mijpeg_get_info says, pixels or None, warning) of mijpeg_decode_batch_device over `streams`."""
    import torch

    try:
        f = d.decode_batch_device(streams, 1)
    except api.MijpegError as e:
        return e.code, None, None, d.last_warning()
    row = f.width * f.components
    out = torch.zeros((len(streams), f.height, row), dtype=torch.uint8, device="cuda:0")
    d.reconstruct_batch_device(out.data_ptr(), f.height * row, row)
    facts = (f.width, f.height, f.components, f.precision, list(f.range_max), f.fast_arith)
    return 0, facts, out.cpu().numpy(), d.last_warning()


@pytest.mark.parametrize("key", WALK_STREAMS, ids=lambda k: "%s-%dx%d-seed%d" % k)
def test_single_image_is_searched_fitted_and_walked(streams, oracle, key):
    data = streams[key]
    off, on, host = api.Decoder(0), api.Decoder(0), api.Decoder(None)
    on.set_device_markers(1)
    rc0, facts0, want, warn0 = _batch_outcome(off, [data])
    assert rc0 == 0 and off.device_walk_rounds() > 0
    for round_ in range(2):  # (the second call reuses the object's buffers)
        rc1, facts1, got, warn1 = _batch_outcome(on, [data])
        assert rc1 == 0 and on.device_markers_stats() == (round_ + 1, 0)
        assert on.device_walk_rounds() > 0
        assert np.array_equal(got, want), key
        assert facts1 == facts0 and warn1 == warn0
    exp = oracle.decode(data)
    assert np.array_equal(want[0].reshape(exp.shape), exp), key
    fh = host.read(data)
    assert list(fh.range_max) == facts0[4] and fh.fast_arith == facts0[5], key
    assert off.device_markers_stats() == (0, 0)
    for d in (off, on, host):
        d.close()


def test_single_image_call_keeps_the_hosts_search(streams):
    data = streams[WALK_STREAMS[0]]
    off, on = api.Decoder(0), api.Decoder(0)
    on.set_device_markers(1)
    (fo, want), (fn, got) = _planes(off, data), _planes(on, data)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and list(fo.range_max) == list(fn.range_max)
    assert on.device_markers_stats() == (0, 1) and on.device_walk_rounds() > 0
    off.close()
    on.close()


# ------------------------------------------------------------------------------------------------ 3. declines inside the call
def _flipped_bit(data, mid):
    """`data` with one bit flipped, the first one from byte `mid` on that the host decoder notices (an error or the reference's
    warning).  Most single bits are value bits: flipping one gives another valid stream that every decoder decodes, and that no
    route can or should decline."""
    host = api.Decoder(None)
    try:
        for at in range(mid, mid + 64):
            if 0xFF in data[at - 1:at + 2]:
                continue
            for bit in range(8):
                flipped = bytearray(data)
                flipped[at] ^= 0x80 >> bit
                if flipped[at] == 0xFF:
                    continue
                try:
                    host.read(bytes(flipped))
                    noticed = host.last_warning()[0] != 0
                except api.MijpegError:
                    noticed = True
                if noticed:
                    return bytes(flipped)
    finally:
        host.close()
    raise AssertionError("no bit near the middle of the entropy coded data whose flip the host decoder notices")


def _corruptions(data):
    p0 = M.ecs_offset(data)
    mid = p0 + (len(data) - 2 - p0) // 2
    while 0xFF in data[mid - 1:mid + 3]:  # (a pair of ordinary bytes: what replaces them is the only FF there)
        mid += 1
    return {
        "a byte behind EOI": data + b"\x00",
        "FF FF in front of nothing": data[:mid] + b"\xff\xff" + data[mid + 2:],
        "a stray FF D3 in the data": data[:mid] + b"\xff\xd3" + data[mid + 2:],
        "one flipped bit": _flipped_bit(data, mid),
    }


@pytest.mark.parametrize("key", [WALK_STREAMS[0], WALK_STREAMS[5]], ids=lambda k: "%s-%dx%d-seed%d" % k)
@pytest.mark.parametrize("what", ["a byte behind EOI", "FF FF in front of nothing", "a stray FF D3 in the data", "one flipped bit"])
def test_corrupted_streams_decline_inside_the_call(streams, key, what):
    data = _corruptions(streams[key])[what]
    off, on = api.Decoder(0), api.Decoder(0)
    on.set_device_markers(1)
    rc0, facts0, pixels0, warn0 = _batch_outcome(off, [data])
    rc1, facts1, pixels1, warn1 = _batch_outcome(on, [data])
    print(what, key, "rc", rc0, rc1, "warning", warn0, warn1, "stats", on.device_markers_stats())
    assert (rc1, warn1, facts1) == (rc0, warn0, facts0), what
    assert (pixels0 is None) == (pixels1 is None), what
    assert pixels0 is None or np.array_equal(pixels0, pixels1), what
    assert on.device_markers_stats() == (0, 1), "a corrupted stream counted as searched and good"
    # ... and beside good streams: the whole call takes the ordinary route inside the same call
    good = streams[key]
    rc0, facts0, pixels0, warn0 = _batch_outcome(off, [good, data])
    rc1, facts1, pixels1, warn1 = _batch_outcome(on, [good, data])
    assert (rc1, warn1, facts1) == (rc0, warn0, facts0) and (pixels0 is None or np.array_equal(pixels0, pixels1)), what
    assert on.device_markers_stats() == (0, 3)
    # the object is as good as new afterwards
    rc0, _, pixels0, _ = _batch_outcome(off, [good])
    rc1, _, pixels1, _ = _batch_outcome(on, [good])
    assert rc0 == 0 and rc1 == 0 and np.array_equal(pixels0, pixels1) and on.device_markers_stats() == (1, 3)
    off.close()
    on.close()


# ------------------------------------------------------------------------------------------------ 4. uniform batches
@pytest.fixture(scope="module")
def mixed_batch():
    """Four streams of one shape: with DRI = 8, without, without, with."""
    return [textured_stream("420", 272, 272, 11, dri=8), walk_stream("420", 272, 272, 1), walk_stream("420", 272, 272, 77), textured_stream("420", 272, 272, 12, dri=8)]


@pytest.mark.parametrize("deferred", [False, True])
def test_uniform_batch_mixes_streams_with_and_without_restart_markers(mixed_batch, deferred):
    off, on = api.Decoder(0), api.Decoder(0)
    on.set_device_markers(1)
    want = _batch_pixels(off, mixed_batch, deferred)
    for round_ in range(2):
        got = _batch_pixels(on, mixed_batch, deferred)
        assert np.array_equal(got, want)
        assert on.device_markers_stats() == (4 * (round_ + 1), 0)
        assert on.device_walk_rounds() > 0
    for i, s in enumerate(mixed_batch):
        assert on.device_markers_staging(i) == s[M.ecs_offset(s):], i
    off.close()
    on.close()


def test_pipeline_mixes_streams_with_and_without_restart_markers(mixed_batch):
    a = batch.BatchShard(mixed_batch, 0, chunk=2, depth=2)
    b = batch.BatchShard(mixed_batch, 0, chunk=2, depth=2, device_markers=True)
    a.run()
    b.run()
    assert np.array_equal(a.out.cpu().numpy(), b.out.cpu().numpy())
    assert a.fallbacks == 0 and b.fallbacks == 0
    assert sum(d.device_markers_stats()[0] for d in b.decoders) == len(mixed_batch)
    assert sum(sum(d.device_markers_stats()) for d in a.decoders) == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. ragged lists
def _mixed_list():
    """(streams, how many of them a parse leaves to the device's search): plain 8-bit sequential streams that end in EOI."""
    from libjpeg_amd import synth

    walked = walk_stream(*WALK_STREAMS[0])
    members = [
        (textured_stream("420", 200, 120, 21, dri=4), True),  # DRI > 0
        (textured_stream("444", 72, 40, 22, dri=1), True),
        (walked, True),  # DRI = 0 above the walk threshold
        (walk_stream(*WALK_STREAMS[5]), True),
        (textured_stream("420", 16, 16, 23), True),  # DRI = 0, one interval
        (textured_stream("420", 8, 8, 24), True),
        (textured_stream("grey", 8, 8, 25), True),
        (synth.synth_jpeg(96, 64, 26, 85, "420", 0, progressive=True), False),
        (textured_stream("420", 200, 120, 27, dri=4) + b"\x00\x00", False),  # bytes behind EOI
        (synth.to_12bit(textured_stream("420", 64, 48, 28, dri=2)), False),
        (_corruptions(walked)["one flipped bit"], True),  # damaged: the search is good, the decode is not
    ]
    return [s for s, _ in members], sum(1 for _, skipped in members if skipped)


@pytest.mark.parametrize("with_12bit", [False, True])
def test_ragged_list_with_the_option_on_is_the_list_with_it_off(with_12bit):
    streams, skipped = _mixed_list()
    off, on = api.Decoder(0), api.Decoder(0)
    want = batch.decode_mixed(streams, 0, decoder=off, with_12bit=with_12bit)
    got = batch.decode_mixed(streams, 0, decoder=on, with_12bit=with_12bit, device_markers=True)
    for i, (a, b) in enumerate(zip(want, got)):
        assert off.ragged_route(i) == on.ragged_route(i), (i, off.ragged_route(i), on.ragged_route(i))
        if isinstance(a, api.MijpegError):
            assert isinstance(b, api.MijpegError) and (a.code, str(a)) == (b.code, str(b)), i
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy()), i
    st0, st1 = off.ragged_stats(), on.ragged_stats()
    print("with_12bit", with_12bit, "off", st0, "on", st1, "markers", on.device_markers_stats())
    assert st0["entropy_launches"] == st1["entropy_launches"] and st0 == st1
    assert on.device_markers_stats() == (skipped, len(streams) - skipped)
    assert off.device_markers_stats() == (0, 0)
    # the walked members are in their groups' launches either way, the damaged one is not
    assert on.ragged_route(2) == (True, None) and on.ragged_route(4) == (True, None) and on.ragged_route(len(streams) - 1)[0] is False
    off.close()
    on.close()

"""Device marker search on the GPU (mijpeg_set_device_markers): the primitive against its reference model on
crafted segments, real streams against the host's search, the opt-in route against the ordinary one (coefficients, pixels,
batches, the pipeline), and the inputs that make the route decline.
"""
import ctypes as C

import numpy as np
import pytest

import markers_model as M
from libjpeg_amd import api, batch, synth
from test_device_markers_cpu import LAYOUTS, host_search, layout_stream

pytestmark = pytest.mark.gpu

LANE, WAVE, CHUNK = 16, 1024, 4096  # bytes of a lane, of a wave's range, of a workgroup (markers.hpp)
GARBAGE = b"\xff\x00\xff\xd0\xff\xff\x12\xff\xd9"


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def check(dec, seg, expect, capacity=None):
    """The device's answer for `seg` equals the model's: everything when flags == 0, else flags and term."""
    m = M.search(seg, expect)
    r = dec.device_marker_search(seg, expect, capacity)
    assert (r["flags"], r["term"]) == (m["flags"], m["term"]), (len(seg), expect, r["flags"], r["term"], m["flags"], m["term"])
    if m["flags"] == 0:
        assert r["total"] == m["total"]
        assert bytes(r["dst"][:m["total"]]) == m["kept"]
        assert not r["dst"][m["total"]:].any(), "zero pad"
        assert list(r["begin"]) == m["begin"] and list(r["end"]) == m["end"]
    return m, r


def plain(rng, n):
    return bytearray(rng.integers(0, 255, n, dtype=np.uint8).tobytes())  # never FF


def test_lengths_and_random_soup(dec):
    rng = np.random.default_rng(20261018)
    sizes = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
    for n in sizes:
        # well-formed: stuffed pairs, markers in sequence, terminator (sizes below two bytes have no room for one)
        for markers in (0, 1, 2, 9):
            if n >= 2 + 2 * markers:
                m, _ = check(dec, M.wellformed(rng, n, markers), markers + 1)
                assert m["flags"] == 0
            if n >= 2 + 2 * markers + len(GARBAGE):
                m, _ = check(dec, M.wellformed(rng, n, markers, GARBAGE), markers + 1)
                assert m["flags"] == 0
        # anything at all: an alphabet that makes every pattern frequent
        alphabet = np.array([0x00, 0xFF, 0xFF, 0xD0, 0xD1, 0xD7, 0xD9, 0x55, 0xAA, 0x01], np.uint8)
        for _ in range(3):
            seg = alphabet[rng.integers(0, len(alphabet), n)].tobytes()
            check(dec, seg, int(rng.integers(1, 4)))
        check(dec, bytes(plain(rng, n)), 1)  # no terminator at all


@pytest.mark.parametrize("edge", [LANE, WAVE, CHUNK, 2 * CHUNK])
def test_pairs_across_boundaries(dec, edge):
    """An FF as the last byte of a lane's 16, of a wave's range and of a chunk, its follower on the other side."""
    rng = np.random.default_rng(edge)
    n = 3 * CHUNK + 5
    base = plain(rng, n)
    base[-2:] = b"\xff\xd9"
    for follower, expect in ((0x00, 1), (0xD0, 2), (0xD9, 1), (0xE0, 1), (0xFF, 1)):
        seg = bytearray(base)
        seg[edge - 1:edge + 1] = bytes((0xFF, follower))
        if follower == 0xFF:
            seg[edge + 1] = 0xD0  # FF FF D0: a fill byte in front of a marker
        m, _ = check(dec, bytes(seg), expect)
        if follower in (0x00, 0xD0):
            assert m["flags"] == 0 and m["term"] == n - 2
        elif follower != 0xFF:
            assert m["flags"] == 0 and m["term"] == edge - 1
    # the same with the pair one byte earlier and one byte later
    for shift in (-1, 1):
        seg = bytearray(base)
        seg[edge - 1 + shift:edge + 1 + shift] = b"\xff\xd0"
        assert check(dec, bytes(seg), 2)[0]["flags"] == 0


def test_every_flag_on_its_own(dec):
    rng = np.random.default_rng(5)
    a, b, c = bytes(plain(rng, 700)), bytes(plain(rng, 5000)), bytes(plain(rng, 33))
    end = b"\xff\xd9"
    cases = [
        (a + b"\xff\xff\xd1" + b + end, 2, M.FILL | M.SEQUENCE),  # FF FF D1
        (a + b"\xff\xff\xd0" + b + end, 2, M.FILL),
        (a + b"\xff\xd1" + b + b"\xff\xd0" + c + end, 3, M.SEQUENCE),  # swapped codes
        (a + b"\xff\xd0" + b + b"\xff\xd1" + c + end, 2, M.COUNT),  # one marker too many
        (a + b"\xff\xd0" + b + b"\xff\xd1" + c + end, 4, M.COUNT),  # one too few
        (a + b"\xff\xd0" + b, 2, M.NO_END),  # no terminator
        (a + b"\xff\xd0" + b + b"\xff", 2, M.NO_END),  # a lone trailing FF
        (a + b"\xff\xd0\xff\xd1" + b + end, 3, 0),  # two markers back to back
        (a + b + end, 1, 0),  # expect = 1 with no marker
        (a + end + GARBAGE * 600, 1, 0),  # garbage behind the terminator: none of it counts
    ]
    for seg, expect, flags in cases:
        m, r = check(dec, seg, expect)
        assert m["flags"] == flags and r["flags"] == flags, (expect, flags, m["flags"], r["flags"])


def test_nothing_outside_the_buffers_is_written(dec):
    """Guard bytes around dst, begin and end stay untouched -- on the host side of the call here, around the device copies
    inside it (the call answers MIJPEG_ERR_PHASE_ERROR otherwise) -- with markers beyond `expect` too."""
    L = api.lib()
    rng = np.random.default_rng(6)
    body = b"".join(bytes(plain(rng, 300)) + bytes((0xFF, 0xD0 + (k & 7))) for k in range(40)) + b"\xff\xd9"
    for expect in (1, 3, 41, 64):
        cap = len(body) + 5
        dst = np.full(cap + 32, 0xA5, np.uint8)
        begin, end = np.full(expect + 8, 0xA5A5A5A5, np.uint32), np.full(expect + 8, 0xA5A5A5A5, np.uint32)
        term, flags = C.c_uint32(), C.c_uint32()
        total = L.mijpeg_device_marker_search(dec._h, body, len(body), expect, dst[16:].ctypes.data, cap, begin[4:].ctypes.data, end[4:].ctypes.data,
                                              C.byref(term), C.byref(flags))
        m = M.search(body, expect)
        assert total >= 0 and (flags.value, term.value) == (m["flags"], m["term"])
        assert (dst[:16] == 0xA5).all() and (dst[16 + cap:] == 0xA5).all()
        for t in (begin, end):
            assert (t[:4] == 0xA5A5A5A5).all() and (t[4 + expect:] == 0xA5A5A5A5).all()
        if m["flags"] == 0:
            assert total == m["total"] and list(begin[4:4 + expect]) == m["begin"] and list(end[4:4 + expect]) == m["end"]


# ------------------------------------------------------------------------------------------------ real streams
STREAMS = [(name, w, h, dri, q) for name, w, h in LAYOUTS for dri in (1, 4, 7) for q in (50, 99)]


@pytest.fixture(scope="module")
def real_streams():
    return {k: layout_stream(*k) for k in STREAMS}


def test_primitive_is_the_hosts_search_on_real_streams(dec, real_streams):
    host = api.Decoder(None)
    for key, data in real_streams.items():
        host.read(data)
        kept, begin, nint = host_search(host, data)
        seg = data[M.ecs_offset(data):]
        r = dec.device_marker_search(seg, nint)
        assert r["flags"] == 0 and r["term"] == len(seg) - 2, key
        assert r["total"] == len(kept) and bytes(r["dst"][:r["total"]]) == kept and list(r["begin"]) == begin, key
        assert not r["dst"][r["total"]:].any()
    host.close()


def test_option_on_decodes_what_option_off_decodes(real_streams, oracle):
    off, on = api.Decoder(0), api.Decoder(0)
    on.set_device_markers(1)
    for n, (key, data) in enumerate(real_streams.items()):
        fo, fn = off.read(data, entropy="gpu"), on.read(data, entropy="gpu")
        assert on.entropy_used == "gpu"
        for c in range(fo.components):
            assert np.array_equal(off.coefficients(c), on.coefficients(c)), (key, c)
        assert list(fo.range_max) == list(fn.range_max) and fo.fast_arith == fn.fast_arith
        want = oracle.decode(data)
        assert np.array_equal(on.reconstruct().reshape(want.shape), want), key
        assert on.last_warning() == off.last_warning()
        assert on.device_markers_stats() == (n + 1, 0), key
    assert off.device_markers_stats() == (0, 0)
    off.close()
    on.close()


# ------------------------------------------------------------------------------------------------ batches
@pytest.fixture(scope="module")
def batch_streams():
    return [synth.synth_jpeg(320, 240, 100 + i, 85, "420", 2) for i in range(12)]


def _batch_pixels(d, streams, deferred):
    import torch

    if deferred:
        d.submit_batch_device(streams, 1)
        f = d.finish_batch_device()
    else:
        f = d.decode_batch_device(streams, 1)
    row = f.width * f.components
    out = torch.zeros((len(streams), f.height, row), dtype=torch.uint8, device="cuda:0")
    d.reconstruct_batch_device(out.data_ptr(), f.height * row, row)
    return out.cpu().numpy()


@pytest.mark.parametrize("deferred", [False, True])
def test_batch_planes_are_those_of_the_ordinary_route(batch_streams, deferred):
    off, on = api.Decoder(0), api.Decoder(0)
    on.set_device_markers(1)
    want = _batch_pixels(off, batch_streams, deferred)
    for round_ in range(2):  # (the second batch reuses the object's buffers)
        got = _batch_pixels(on, batch_streams, deferred)
        assert np.array_equal(got, want)
        assert on.device_markers_stats() == (12 * (round_ + 1), 0)
    assert on.device_markers_staging(3) == batch_streams[3][M.ecs_offset(batch_streams[3]):]
    off.close()
    on.close()


def test_pipeline_with_device_markers(batch_streams):
    streams = batch_streams * 2
    a = batch.BatchShard(streams, 0, chunk=8, depth=2)
    b = batch.BatchShard(streams, 0, chunk=8, depth=2, device_markers=True)
    a.run()
    b.run()
    assert np.array_equal(a.out.cpu().numpy(), b.out.cpu().numpy())
    assert b.fallbacks == 0
    assert sum(d.device_markers_stats()[0] for d in b.decoders) == len(streams)
    assert sum(sum(d.device_markers_stats()) for d in a.decoders) == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ declines
def _first_marker(data):
    p = M.ecs_offset(data)
    while not (data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7):
        p += 1
    return p


def _outcome(d, data):
    L = api.lib()
    d._data = data
    assert L.mijpeg_set_input(d._h, data, len(data)) == 0
    rc = L.mijpeg_decode_coefficients_device(d._h, 1)
    planes = None
    if rc == 0:
        info = api.MijpegInfo()
        assert L.mijpeg_get_info(d._h, C.byref(info)) == 0
        d.info = info
        planes = [d.coefficients(c) for c in range(info.components)]
    return rc, planes, d.last_warning()


def test_declines_are_the_ordinary_route(batch_streams):
    good = batch_streams[0]
    p = _first_marker(good)
    cases = {
        "fill byte in front of a marker": good[:p] + b"\xff" + good[p:],
        "bytes behind EOI": good + b"\x00\x00",
        "bytes behind EOI that end in EOI": good + b"\x00\xff\xd9",
        "no restart markers": synth.synth_jpeg(320, 240, 100, 85, "420", 0),
    }
    off, on = api.Decoder(0), api.Decoder(0)
    on.set_device_markers(1)
    declined = 0
    for what, data in cases.items():
        rc0, planes0, warn0 = _outcome(off, data)
        rc1, planes1, warn1 = _outcome(on, data)
        declined += 1
        assert rc1 == rc0 and warn1 == warn0, (what, rc0, rc1, warn0, warn1)
        assert (planes0 is None) == (planes1 is None), what
        for a, b in zip(planes0 or [], planes1 or []):
            assert np.array_equal(a, b), what
        assert on.device_markers_stats() == (0, declined), what
    # a marker out of sequence: damaged, the host decoder's business either way
    bad = bytearray(good)
    bad[p + 1] = 0xD3
    for d in (off, on):
        rc, _, _ = _outcome(d, bytes(bad))
        assert rc == api.ERR_NOT_AVAILABLE
    assert on.device_markers_stats() == (0, declined + 1)
    # ... and through submit / finish, which no longer has the bytes: NOT_AVAILABLE at finish, as for damaged streams
    # (the ordinary route decodes a legal fill byte; the pipeline's fallback is what takes such a chunk there)
    batch_ = batch_streams[:3] + [cases["fill byte in front of a marker"]]
    on.submit_batch_device(batch_, 1)
    with pytest.raises(api.MijpegError) as e:
        on.finish_batch_device()
    assert e.value.code == api.ERR_NOT_AVAILABLE
    assert on.device_markers_stats() == (0, declined + 1 + 4)
    want = _batch_pixels(off, batch_, True)
    on.decode_batch_device(batch_, 1)  # the synchronous call runs the ordinary route inside the same call
    assert on.device_markers_stats() == (0, declined + 1 + 8)
    shard = batch.BatchShard(batch_, 0, chunk=4, depth=2, device_markers=True)
    shard.run()
    assert shard.fallbacks == 1 and np.array_equal(shard.out.cpu().numpy(), want)
    shard.close()
    # the object is as good as new afterwards
    assert np.array_equal(_batch_pixels(on, batch_streams[:4], True), _batch_pixels(off, batch_streams[:4], True))
    off.close()
    on.close()

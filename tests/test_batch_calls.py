"""The uniform batch calls (batch_decode.cpp) on tiny pictures: one object over lists that shrink and grow, own tables then shared
tables, mijpeg_get_info as the call that awaits a submitted batch, an empty member of a ragged list -- every frame against the
single-image decode of its stream -- and the recorded outcomes of tests/batch_call_scripts.py, replayed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import batch_call_scripts as B
from conftest import GOLDEN_DIR
from libjpeg_amd import api

pytestmark = pytest.mark.gpu

_single = {}


def single(stream):
    """api.decode of the stream: computed once, shared, read-only."""
    if stream not in _single:
        _single[stream] = api.decode(stream)
        _single[stream].setflags(write=False)
    return _single[stream]


def batch_pixels(d, n, w, h, **kw):
    import torch

    out = torch.zeros((n, h, w * 3), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(out.data_ptr(), h * w * 3, w * 3, **kw)
    return out.cpu().numpy().reshape(n, h, w, 3)


def get_info(d):
    f = api.MijpegInfo()
    assert api.lib().mijpeg_get_info(d._h, C.byref(f)) == 0
    return f


@pytest.mark.parametrize("make,w,h", [(B.s420, B.W, B.H), (B.s444, B.W4, B.H4)])
def test_one_object_over_lists_of_5_2_5(make, w, h):
    streams = [make(60 + i) for i in range(5)]
    d = api.Decoder(0)
    for part in (streams, streams[3:], streams[::-1]):
        d.submit_batch_device(part, 1)
        got = batch_pixels(d, len(part), w, h)
        for i, s in enumerate(part):
            assert np.array_equal(got[i], single(s)), i
    d.close()


@pytest.mark.parametrize("make,w,h", [(B.s420, B.W, B.H), (B.s444, B.W4, B.H4)])
def test_own_tables_then_shared_tables(make, w, h):
    mixed = [make(70 + i, q) for i, q in enumerate((50, 90, 90, 50, 90))]
    shared = [make(80 + i) for i in range(3)]
    d = api.Decoder(0)
    info = d.decode_batch_device(mixed, 1)
    one = api.Decoder(None)
    members = [one.read_header(s) for s in mixed]
    members = [[list(f.quant[f.quant_index[c]]) for c in range(3)] for f in members]
    one.close()
    assert members[0] != members[1]
    for c in range(3):  # per component and position, the largest delta any member has
        assert list(info.quant[info.quant_index[c]]) == [max(m[c][k] for m in members) for k in range(64)], c
    got = batch_pixels(d, 5, w, h)
    for i, s in enumerate(mixed):
        assert np.array_equal(got[i], single(s)), i
    d.decode_batch_device(shared, 1)  # (the launch goes back to the tables in the kernel arguments)
    got = batch_pixels(d, 3, w, h)
    for i, s in enumerate(shared):
        assert np.array_equal(got[i], single(s)), i
    d.close()


def test_get_info_awaits_a_submitted_batch():
    streams = [B.s420(90 + i) for i in range(4)]
    d, blocking = api.Decoder(0), api.Decoder(0)
    want = blocking.decode_batch_device(streams, 1)
    d.submit_batch_device(streams, 1)
    f = get_info(d)  # no mijpeg_finish_batch_device in between
    assert d.batch_frames == 4
    assert list(f.range_max) == list(want.range_max) and f.fast_arith == want.fast_arith
    got = batch_pixels(d, 4, B.W, B.H)  # (the batch is decoded: there is nothing left to await)
    for i, s in enumerate(streams):
        assert np.array_equal(got[i], single(s)), i
    d.close()
    blocking.close()


def test_an_empty_member_of_a_ragged_list():
    import torch

    good = [B.s420(95), B.s444(96)]
    d = api.Decoder(0)
    assert d.decode_ragged_device([good[0], b"", good[1]], 1) == [0, -1027, 0]  # MIJPEG_ERR_STREAM_EMPTY
    outs = [torch.zeros((B.H, B.W * 3), dtype=torch.uint8, device="cuda"), None, torch.zeros((B.H4, B.W4 * 3), dtype=torch.uint8, device="cuda")]
    d.reconstruct_ragged_device([o.data_ptr() if o is not None else 0 for o in outs], [B.W * 3, 0, B.W4 * 3])
    assert np.array_equal(outs[0].cpu().numpy().reshape(B.H, B.W, 3), single(good[0]))
    assert np.array_equal(outs[2].cpu().numpy().reshape(B.H4, B.W4, 3), single(good[1]))
    d.close()


with open(os.path.join(GOLDEN_DIR, "batch_call_outcomes.json")) as _f:
    RECORD = json.load(_f)


def test_the_record_covers_the_scripts():
    assert sorted(RECORD["rows"]) == sorted(B.SCRIPTS) and len(B.SCRIPTS) >= 24
    assert RECORD["inputs"] == B.inputs_digest(), "the encoder of this machine writes other streams than the one the record was made with"


@pytest.mark.parametrize("name", sorted(B.SCRIPTS))
def test_recorded_outcomes(name):
    """The script's observations on this library are those recorded from the commit RECORD["recorded_from"]."""
    got = json.loads(json.dumps(B.run(name)))
    want = RECORD["rows"][name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k)
    assert len(got) == len(want)

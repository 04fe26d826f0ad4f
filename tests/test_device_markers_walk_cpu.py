"""Device marker route for streams without restart markers (mijpeg_set_device_markers), the part that needs no
GPU: the host half stages the raw segment of such a stream and counts it as searched, the streams that must keep the host's
search keep it, and the reference model with one expected interval is the host's search.  Also the streams the GPU tests
(test_device_markers_walk.py) decode, made and checked here.
"""
import ctypes as C

import numpy as np
import pytest

import craft
import markers_model as M
from libjpeg_amd import api, synth
from test_device_markers_cpu import host_search

SUB_BYTES = 128  # the walk's subsequence size for launches of up to 8 MB (device_walk_images)

# (layout, width, height, seed): textured pictures at quality 80, the smallest the uniform walk accepts (>= 256 MCUs, >= 4096 bytes
# of entropy coded data; 17 x 17 MCUs each) and one of 640 x 480.  Seeds found by trying: the raw segment and the copy without
# stuffing differ in their number of subsequences for all of them; 272 x 272 seed 77 -- the copy is a multiple of SUB_BYTES;
# 640 x 480 seed 125 -- the raw segment is and the copy is not.
WALK_STREAMS = [("420", 272, 272, 1), ("420", 272, 272, 77), ("420", 640, 480, 125), ("422", 264, 136, 1), ("444", 136, 136, 1), ("grey", 136, 136, 62)]
COPY_IS_A_MULTIPLE, RAW_IS_A_MULTIPLE = WALK_STREAMS[1], WALK_STREAMS[2]


def textured_stream(layout, w, h, seed, quality=80, dri=0):
    """The synthetic picture of libjpeg_amd.synth under Gaussian noise of sigma 20: enough bytes for a walk at these sizes, and
    blocks that end in EOB, which is what lets a walker that starts in the wrong place fall into step."""
    rng = np.random.default_rng(seed)
    ch = 1 if layout == "grey" else 3
    img = synth.synth_image(w, h, seed, ch).astype(np.float32) + rng.normal(0.0, 20.0, (h, w, ch)).astype(np.float32)
    return synth.encode_jpeg(np.clip(img, 0, 255).astype(np.uint8), quality, "420" if layout == "grey" else layout, dri)


def segment_sizes(data):
    """(raw bytes of the entropy coded segment up to the end of the stream, bytes of its copy without stuffing)."""
    seg = data[M.ecs_offset(data):]
    m = M.search(seg, 1)
    assert m["flags"] == 0 and m["term"] == len(seg) - 2
    return len(seg), m["total"]


def walk_stream(layout, w, h, seed):
    data = textured_stream(layout, w, h, seed)
    raw, copy = segment_sizes(data)
    assert -(-raw // SUB_BYTES) != -(-copy // SUB_BYTES), "the device's subsequence count must differ from the host's bound"
    return data


def test_walk_streams_have_the_sizes_the_gpu_tests_rely_on():
    for key in WALK_STREAMS:
        walk_stream(*key)
    raw, copy = segment_sizes(walk_stream(*COPY_IS_A_MULTIPLE))
    assert copy % SUB_BYTES == 0
    raw, copy = segment_sizes(walk_stream(*RAW_IS_A_MULTIPLE))
    assert raw % SUB_BYTES == 0 and copy % SUB_BYTES != 0


def test_option_on_a_stream_without_restart_markers():
    streams = [walk_stream(*key) for key in WALK_STREAMS[:2]] + [textured_stream("420", 272, 272, 5, dri=8)]
    d = api.Decoder(None)
    d.set_device_markers(1)
    d.prepare_batch_host(streams[:1])
    assert d.device_markers_stats() == (1, 0)
    assert d.device_markers_staging(0) == streams[0][M.ecs_offset(streams[0]):]
    # ... and side by side with a stream that has restart markers
    d.prepare_batch_host(streams)
    assert d.device_markers_stats() == (4, 0)
    for i, s in enumerate(streams):
        assert d.device_markers_staging(i) == s[M.ecs_offset(s):], i
    # too small for a walk: the ordinary route decides, as it does with the option off
    d.prepare_batch_host([synth.synth_jpeg(160, 120, 7, 85, "420", 0)])
    assert d.device_markers_stats() == (4, 1) and d.device_markers_staging(0) is None
    d.close()


def _prepare_rc(d, data):
    try:
        d.prepare_batch_host([data])
        return 0
    except api.MijpegError as e:
        return e.code


def _host_search_or_rc(d, data):
    try:
        d.read(data)
    except api.MijpegError as e:
        return e.code
    L = api.lib()
    L.mijpeg_unstuffed_scan.restype = C.c_int64
    L.mijpeg_unstuffed_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32)]
    total = L.mijpeg_unstuffed_scan(d._h, None, 0, None, 0, 0, None)
    return host_search(d, data) if total >= 0 else total  # (a DNL frame plans no scan: the call's error code)


def _decline_cases():
    good = walk_stream(*WALK_STREAMS[0])
    return {
        "bytes behind EOI": good + b"\x00",
        "no EOI": good[:-2],
        "progressive": synth.synth_jpeg(272, 272, 3, 95, "420", 0, progressive=True),
        "12 bit": synth.to_12bit(good),
        "DNL": craft.to_dnl(good),
    }


@pytest.mark.parametrize("what", ["bytes behind EOI", "no EOI", "progressive", "12 bit", "DNL"])
def test_streams_that_keep_the_hosts_search(what):
    data = _decline_cases()[what]
    off, on = api.Decoder(None), api.Decoder(None)
    on.set_device_markers(1)
    assert _prepare_rc(on, data) == _prepare_rc(off, data), what
    assert on.device_markers_stats() == (0, 1) and on.device_markers_staging(0) is None, what
    assert _host_search_or_rc(on, data) == _host_search_or_rc(off, data), what
    off.close()
    on.close()


def test_model_with_one_interval_is_the_hosts_search():
    d = api.Decoder(None)
    for key in WALK_STREAMS:
        data = walk_stream(*key)
        d.read(data)
        kept, begin, nint = host_search(d, data)
        seg = data[M.ecs_offset(data):]
        m = M.search(seg, 1)
        assert nint == 1 and begin == [0]
        assert m["flags"] == 0 and m["term"] == len(seg) - 2 and m["markers"] == 0
        assert m["kept"] == kept and m["begin"] == [0] and m["end"] == [len(kept)], key
    d.close()

"""The header pass of the list calls (parse_stream_headers, batch_decode.cpp) through the call that needs no device,
mijpeg_prepare_batch_host: the parsers and slots of a list that shrinks and grows again, and which stream's failure a call reports."""
import pytest

import markers_model as M
from libjpeg_amd import api, synth


def test_parsers_and_slots_survive_a_shrinking_and_growing_list():
    streams = [synth.synth_jpeg(72, 48, 40 + i, (50, 85, 99)[i % 3], "420", 2) for i in range(6)]
    d = api.Decoder(None)
    d.prepare_batch_host(streams)
    d.prepare_batch_host(streams[4:])
    d.set_device_markers(1)
    d.prepare_batch_host(streams)
    for i, s in enumerate(streams):
        assert d.device_markers_staging(i) == s[M.ecs_offset(s):], i
    assert d.device_markers_staging(6) is None and d.device_markers_stats() == (6, 0)
    d.close()


def test_a_call_reports_the_first_stream_that_failed():
    good = [synth.synth_jpeg(72, 48, 40 + i, 85, "420", 2) for i in range(3)]
    sof = good[1].find(b"\xff\xc0")
    arithmetic = good[1][:sof + 1] + b"\xc9" + good[1][sof + 2:]  # SOF9: a frame type this library declines
    garbage = b"\xff\xd8 not a jpeg at all"
    verdicts = []
    for bad in (arithmetic, garbage):
        d = api.Decoder(None)
        with pytest.raises(api.MijpegError) as e:
            d.read_header(bad)
        verdicts.append((e.value.code, e.value.message))
        d.close()
    assert verdicts[0][0] != verdicts[1][0] and verdicts[0][1] != verdicts[1][1]  # two different faults
    d = api.Decoder(None)
    for on in (0, 1):  # (the marker route's attempt reports nothing of its own: the call's verdict is the ordinary route's)
        d.set_device_markers(on)
        with pytest.raises(api.MijpegError) as e:
            d.prepare_batch_host([good[0], arithmetic, good[2], garbage])
        assert (e.value.code, e.value.message) == verdicts[0]
        with pytest.raises(api.MijpegError) as e:
            d.prepare_batch_host([good[0], garbage, good[2], arithmetic])
        assert (e.value.code, e.value.message) == verdicts[1]
    d.close()

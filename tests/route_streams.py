"""Streams and references the tests of device_entropy_batch's routes share (tests/test_gpu_parity.py, tests/test_ragged_batch.py)."""
import numpy as np

from libjpeg_amd import api, synth


def noise_jpeg(w, h, seed, sub="444", restart_mcus=0):
    """Noise at quality 100: the smallest pictures either walk takes (256 MCUs and 4 KiB of entropy coded data for the device's,
    four 32 KiB segments for the host's planner: 256 x 256 4:4:4 gives 1024 MCUs in 270 KB)."""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    return synth.encode_jpeg(img, 100, sub, restart_mcus=restart_mcus)


def grey_2x2_jpeg(w, h, seed, dri):
    """A grey picture whose frame header gives its one component sampling factors 2 x 2 (the scan of a single component is coded
    block by block whatever its factors are, so only the header differs): planes padded to whole 16 x 16 MCUs, scan over w/8 x h/8."""
    data = bytearray(synth.encode_jpeg(synth.synth_image(w, h, seed, channels=1), 90, "444", restart_mcus=dri))
    sof = data.find(b"\xff\xc0")
    assert data[sof + 9] == 1 and data[sof + 11] == 0x11
    data[sof + 11] = 0x22
    return bytes(data)


def host_decodes(streams):
    """-> per stream (pixels, range_max, fast_arith) of the host decoder."""
    host = api.Decoder(0)
    res = []
    for data in streams:
        f = host.read(data)
        res.append((host.reconstruct(), list(f.range_max), int(f.fast_arith)))
    host.close()
    return res

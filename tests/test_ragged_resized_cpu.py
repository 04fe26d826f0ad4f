"""The resized call's host half (mijpeg_resample_taps, libjpeg_amd/csrc/resample_taps.hpp), without a device: the exported
taps equal the numpy restatement of the filter (tests/resample_model.py) on every size pair of the list below, their invariants hold, the
filter is pinned to what users know (Pillow's BILINEAR) and the table builder runs under the sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_model as M
from conftest import ROOT
from libjpeg_amd import api
from test_ragged_twin_cpu import _run_under_sanitizers

SIZES = [1, 2, 3, 7, 8, 9, 16, 127, 128, 129, 300]
PAIRS = [(n, m) for n in SIZES for m in SIZES] + [(65535, 224), (224, 65535)]
# (source w x h, output w x h): the shape pairs the filter was specified on
SHAPES = [((300, 270), (224, 224)), ((129, 131), (32, 32)), ((257, 40), (224, 224)), ((16, 16), (224, 224)), ((300, 270), (1, 1)), ((1, 1), (32, 32)),
          ((224, 224), (224, 224)), ((500, 375), (224, 224)), ((37, 211), (64, 48)), ((1024, 768), (224, 224))]


def test_taps_equal_the_model_and_keep_their_invariants():
    for n, m in PAIRS:
        first, count, weights = api.resample_taps(n, m)
        mf, mc, mw = M.taps(n, m)
        assert weights.shape == mw.shape and weights.dtype == np.int16, (n, m)
        assert np.array_equal(first, mf) and np.array_equal(count, mc) and np.array_equal(weights, mw), (n, m)
        assert weights.min() >= 0 and (weights.astype(np.int64).sum(axis=1) == 16384).all(), (n, m)
        assert 1 <= count.min() and count.max() == weights.shape[1] <= M.bound(n, m), (n, m)
        assert first.min() >= 0 and (first + count).max() <= n, (n, m)
        assert all(not weights[o, count[o]:].any() for o in range(0, m, max(1, m // 64))), (n, m)  # (zero behind the count)
        if n == m:
            assert np.array_equal(first, np.arange(n)) and (count == 1).all() and (weights[:, 0] == 16384).all(), n


def test_taps_size_query_and_refusals():
    L = api.lib()
    assert L.mijpeg_resample_taps(300, 224, None, None, None, 0) == api.resample_taps(300, 224)[2].shape[1]
    assert L.mijpeg_resample_taps(300, 1, None, None, None, 0) == 300 and L.mijpeg_resample_taps(1, 300, None, None, None, 0) == 1
    for n, m in [(0, 4), (4, 0), (-1, 4), (65536, 4), (4, 65536)]:
        assert L.mijpeg_resample_taps(n, m, None, None, None, 0) == 0, (n, m)
    first, count, weights = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int16 * 16)()
    assert L.mijpeg_resample_taps(16, 4, first, count, weights, 2) == 0  # (a capacity below the axis's maximal count)
    with pytest.raises(api.MijpegError):
        api.resample_taps(0, 4)


def test_identity_resize_is_the_picture():
    img = np.random.default_rng(7).integers(0, 256, (23, 31, 3), dtype=np.uint8)
    assert np.array_equal(M.resize(img, 31, 23), img)
    assert np.array_equal(M.resize(img[:, :, 0], 31, 23), img[:, :, 0])


def test_model_against_pillow():
    """The figure measured when the filter was specified: at most one code value from Pillow's BILINEAR on seeded noise.  It pins the
    definition to something users know; it is not a tolerance on the kernel (the GPU tests compare with the model at tolerance 0)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20260)
    for (w, h), (ow, oh) in SHAPES:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR, reducing_gap=None))
        got = M.resize(img, ow, oh)
        assert got.shape == ref.shape
        assert np.abs(got.astype(np.int16) - ref.astype(np.int16)).max() <= 1, ((w, h), (ow, oh))


def test_resample_taps_under_sanitizers(tmp_path):
    """tests/cxx/resample_taps.cpp, a program of its own around resample_taps.hpp: single axes up to 65535 samples against the
    definition in 128-bit integers, the tables of a list with refused members read back from a heap buffer of exactly the layout's size,
    under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "resample_taps")


def test_exports_and_struct_sizes(tmp_path):
    L = api.lib()
    for name in ("mijpeg_reconstruct_ragged_resized_device", "mijpeg_ragged_resized_stats_get", "mijpeg_resample_taps"):
        assert hasattr(L, name), name
    assert C.sizeof(api.MijpegRaggedResizedStats) == 32 and api.MijpegRaggedResizedStats.arena_bytes.offset == 24
    assert api.ERR_NOT_IMPLEMENTED == -1034
    # the header's own word on it
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mijpeg.h"\nint main(void) { printf("%zu %zu %zu %d\\n", sizeof(mijpeg_ragged_resized_stats), '
                   'offsetof(mijpeg_ragged_resized_stats, arena_bytes), sizeof(mijpeg_rect), MIJPEG_ERR_NOT_IMPLEMENTED); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "24", str(C.sizeof(api.MijpegRect)), "-1034"], out
    # a host-only object: the statistics are readable and zero, the call itself needs a device
    d = api.Decoder(None)
    try:
        assert d.ragged_resized_stats() == dict(images=0, resampled=0, refused=0, window_launches=0, resample_launches=0, arena_bytes=0)
    finally:
        d.close()

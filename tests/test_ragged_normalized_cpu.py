"""The normalised resized call's host half (mijpeg_reconstruct_ragged_normalized_device, batch.decode_resized(dtype=...)),
without a device: exports and the structs' layouts, the numpy model's own checks (tests/normalize_model.py), the mirrored tap tables as a
program of its own under the sanitizers, every ValueError of batch.decode_resized, and the resample kernels' resources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import normalize_model as N
from conftest import ROOT, golden_jpeg
from libjpeg_amd import api, batch
from test_ragged_batch import LIB, READELF, _kernel_metadata
from test_ragged_twin_cpu import _run_under_sanitizers

TYPES = (N.F32, N.F16, N.BF16)


def test_exports_and_struct_layouts(tmp_path):
    L = api.lib()
    for name in ("mijpeg_reconstruct_ragged_normalized_device", "mijpeg_ragged_normalized_stats_get"):
        assert hasattr(L, name), name
    assert (api.SAMPLE_U8, api.SAMPLE_F32, api.SAMPLE_F16, api.SAMPLE_BF16) == (N.U8, N.F32, N.F16, N.BF16) == (0, 1, 2, 3)
    # the header's own word on the two structs, as a C compiler lays them out
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mijpeg.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", '
                   'sizeof(mijpeg_batch_format), offsetof(mijpeg_batch_format, sample), offsetof(mijpeg_batch_format, reserved), offsetof(mijpeg_batch_format, scale), '
                   'offsetof(mijpeg_batch_format, bias), offsetof(mijpeg_batch_format, mirror), sizeof(mijpeg_ragged_normalized_stats), '
                   'offsetof(mijpeg_ragged_normalized_stats, mirrored), offsetof(mijpeg_ragged_normalized_stats, reserved), '
                   'MIJPEG_SAMPLE_U8, MIJPEG_SAMPLE_F32, MIJPEG_SAMPLE_F16, MIJPEG_SAMPLE_BF16); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    F, S = api.MijpegBatchFormat, api.MijpegRaggedNormalizedStats
    assert out == [C.sizeof(F), F.sample.offset, F.reserved.offset, F.scale.offset, F.bias.offset, F.mirror.offset, C.sizeof(S), S.mirrored.offset, S.reserved.offset,
                   0, 1, 2, 3], out
    assert out[:7] == [40, 0, 4, 8, 20, 32, 16], out
    # a host-only object: the statistics are readable and zero, and the resized call's dictionary has not gained a key
    d = api.Decoder(None)
    try:
        assert d.ragged_normalized_stats() == dict(sample=0, mirrored=0)
        assert d.ragged_resized_stats() == dict(images=0, resampled=0, refused=0, window_launches=0, resample_launches=0, arena_bytes=0)
    finally:
        d.close()


def test_model_constant_sets_stay_on_specified_ground():
    """Both constant sets, every v in 0 .. 255, all three types: nothing is subnormal in its stored type (the model asserts it), nothing
    overflows binary16, the smallest non-zero magnitude is 0.0039; the crafted set has exact zeros, a negative slope, and values bfloat16
    merges."""
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    smallest = np.inf
    for scale, bias in N.SETS.values():
        f32 = N.normalize(v, scale, bias, N.F32).view(np.float32)
        f16 = N.normalize(v, scale, bias, N.F16).view(np.float16)
        b16 = (N.normalize(v, scale, bias, N.BF16).astype(np.uint32) << 16).view(np.float32)
        assert np.isfinite(f16).all() and np.isfinite(b16).all()
        for a in (f32, f16.astype(np.float32), b16):
            smallest = min(smallest, np.abs(a[a != 0]).min())
    assert 0.0039 <= smallest < 0.00393, smallest
    scale, bias = N.CRAFTED
    f32 = N.normalize(v, scale, bias, N.F32).view(np.float32)
    assert f32[0, 0, 0] == 0 and f32[0, 128, 1] == 0 and f32[0, 255, 2] < 0 < f32[0, 0, 2]
    assert len(np.unique(N.normalize(v, scale, bias, N.BF16)[0, :, 2])) < 256 == len(np.unique(f32[0, :, 2]))
    with pytest.raises(AssertionError):  # (2^-130: subnormal in float32 -- a test cannot expect it)
        N.normalize(v[:, 1:2], (np.float32(2.0 ** -130),) * 3, (np.float32(0),) * 3, N.F32)
    with pytest.raises(AssertionError):  # (1e-6 is a normal float32 and a subnormal binary16)
        N.normalize(v[:, 1:2], (np.float32(1e-6),) * 3, (np.float32(0),) * 3, N.F16)


def test_model_bf16_is_torchs_conversion():
    torch = pytest.importorskip("torch")
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    for scale, bias in N.SETS.values():
        y = np.ascontiguousarray(N.normalize(v, scale, bias, N.F32).view(np.float32))
        want = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(N.normalize(v, scale, bias, N.BF16), want)
        assert np.array_equal(N.bf16_bits(y), want)
        half = torch.from_numpy(y).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(N.normalize(v, scale, bias, N.F16), half)


def test_model_mirror_is_the_slot_reversed():
    v = np.random.default_rng(11).integers(0, 256, (5, 37, 3), dtype=np.uint8)
    scale, bias = N.IMAGENET
    for sample in (N.U8,) + TYPES:
        plain, flipped = N.normalize(v, scale, bias, sample), N.normalize(v, scale, bias, sample, mirror=True)
        assert plain.dtype == N.ELEMENT[sample] and plain.shape == v.shape
        assert np.array_equal(flipped, plain[:, ::-1]) and not np.array_equal(flipped, plain)
    assert np.array_equal(N.normalize(v, None, None, N.U8), v)


def test_constants_are_rounded_once():
    scale, bias = batch._normalize_constants(N.IMAGENET_MEAN, N.IMAGENET_STD, 3)
    assert tuple(np.float32(s) for s in scale) == N.IMAGENET[0] and tuple(np.float32(b) for b in bias) == N.IMAGENET[1]
    assert batch._normalize_constants(None, None, 3) == ([float(np.float32(1 / 255))] * 3, [0.0] * 3)
    assert batch._normalize_constants(0.5, 0.25, 1) == ([float(np.float32(1 / (255 * 0.25)))], [-2.0])


def test_mirrored_tables_under_sanitizers(tmp_path):
    """tests/cxx/resample_mirror.cpp, a program of its own around resample_taps.hpp: column x of a mirrored picture's x table against
    column m - 1 - x of the unmirrored one on the axes 1 -> 1, 1 -> 64, 65 -> 64, 300 -> 1, 300 -> 65, 17 -> 224, 270 -> 37, the y
    table untouched, under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "resample_mirror")


def test_decode_resized_value_errors():
    """Every ValueError of the new parameters, before any device work: a header-only decoder, no device."""
    torch = pytest.importorskip("torch")
    streams = [golden_jpeg("pil_90x60_cmyk"), golden_jpeg("pilprog_200x130_422")]
    inf, nan = float("inf"), float("nan")
    bad = {"unknown dtype": dict(dtype=torch.int16), "dtype float64": dict(dtype=torch.float64), "dtype by name": dict(dtype="float16"),
           "mean without a dtype": dict(mean=0.5), "std without a dtype": dict(std=0.5), "mean with uint8": dict(dtype=torch.uint8, mean=(0.1, 0.2, 0.3)),
           "std with uint8": dict(dtype=torch.uint8, std=0.5),
           "two means": dict(dtype=torch.float16, mean=(0.1, 0.2)), "four stds": dict(dtype=torch.float32, std=(1, 1, 1, 1)),
           "three means for one channel": dict(dtype=torch.float32, channels=1, mean=(0.1, 0.2, 0.3)),
           "one mirror flag": dict(mirror=[True]), "three mirror flags": dict(dtype=torch.bfloat16, mirror=[0, 1, 0]),
           "std 0": dict(dtype=torch.float16, std=0), "one std of 0": dict(dtype=torch.float16, std=(1, 0.0, 1)),
           "mean inf": dict(dtype=torch.float32, mean=inf), "mean nan": dict(dtype=torch.float32, mean=(0, nan, 0)), "std inf": dict(dtype=torch.float32, std=inf),
           "std nan": dict(dtype=torch.bfloat16, std=(1, 1, nan)), "scale overflows": dict(dtype=torch.float32, std=1e-45),
           "bias overflows": dict(dtype=torch.float32, mean=1e30, std=1e-30)}
    d = api.Decoder(None)
    try:
        for name, kw in bad.items():
            with pytest.raises(ValueError):
                batch.decode_resized(streams, (8, 8), decoder=d, **kw)
                pytest.fail(name)
        assert d.ragged_resized_stats()["images"] == 0 and d.ragged_normalized_stats() == dict(sample=0, mirrored=0)
    finally:
        d.close()


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_resample_kernels_resources():
    """mij::resample_list_kernel keeps the figures of profiles/ragged_resized.txt; the float flavours have no scratch, no spills, its
    4608 bytes of LDS, and registers for its four waves per SIMD (at most 128 VGPRs)."""
    meta = _kernel_metadata(LIB)
    old = meta["_ZN3mij20resample_list_kernelENS_12ResampleArgsE"]
    assert int(old["vgpr_count"]) == 112 and int(old["group_segment_fixed_size"]) == 4608 and int(old["private_segment_fixed_size"]) == 0, old
    new = {name: k for name, k in meta.items() if "resample" in name and k is not old}
    assert len(new) == 3, sorted(new)
    for name, k in new.items():
        assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
        assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
        assert int(k["group_segment_fixed_size"]) == 4608, name
        assert int(k["vgpr_count"]) + int(k.get("agpr_count", 0)) <= 128, f"{name}: fewer than four waves per SIMD"

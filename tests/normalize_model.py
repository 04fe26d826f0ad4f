"""The normalised resized call's store epilogue (include/mijpeg.h) restated in numpy, from its definition alone.  With v the
8-bit sample resample_model.resize() gives, an element of output channel c is

    y = fl32(fl32(float32(v) * scale[c]) + bias[c])        two binary32 operations, each rounded to nearest-even, no fused multiply-add

stored as binary32, as binary16 (to nearest-even) or as bfloat16 (the upper 16 bits of bits(y) + 0x7fff + ((bits(y) >> 16) & 1)); a
mirrored slot holds its lines reversed (resize, then flip).  normalize() returns BIT PATTERNS, which the GPU tests compare at tolerance 0.
A result that is subnormal in the stored type is outside the contract, so normalize() refuses to expect one.
(Not a test module: pytest collects test_*.py.)"""
import numpy as np

U8, F32, F16, BF16 = 0, 1, 2, 3  # MIJPEG_SAMPLE_*
ELEMENT = {U8: np.uint8, F32: np.uint32, F16: np.uint16, BF16: np.uint16}  # the bit patterns' types
SMALLEST_NORMAL = {F32: 2.0 ** -126, F16: 2.0 ** -14, BF16: 2.0 ** -126}

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def constants(mean, std):
    """(scale, bias) as batch.decode_resized derives them: float32(1 / (255 std)) and float32(-mean / std), from float64, rounded once."""
    return (tuple(np.float32(1.0 / (255.0 * s)) for s in std), tuple(np.float32(-m / s) for m, s in zip(mean, std)))


# the two constant sets of the tests: ImageNet's, and one with exact zeros, a negative slope and values that bfloat16 merges
IMAGENET = constants(IMAGENET_MEAN, IMAGENET_STD)
CRAFTED = ((np.float32(1 / 255), np.float32(0.5), np.float32(-3.0)), (np.float32(0.0), np.float32(-64.0), np.float32(7.25)))
SETS = {"imagenet": IMAGENET, "crafted": CRAFTED}


def bf16_bits(y):
    """float32 array -> the bfloat16 bit patterns of the contract's formula (uint16)."""
    bits = np.ascontiguousarray(y, np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def normalize(v, scale, bias, sample, mirror=False):
    """v: uint8 (h, w, c) as resample_model.resize returns it; scale, bias: c numbers -> (h, w, c) bit patterns of the stored elements
    (uint8 / uint32 / uint16 / uint16 for U8 / F32 / F16 / BF16), mirrored along x where `mirror`."""
    v = np.asarray(v)
    assert v.dtype == np.uint8 and v.ndim == 3, (v.dtype, v.shape)
    if mirror:
        v = v[:, ::-1]
    if sample == U8:
        return np.ascontiguousarray(v)
    scale, bias = np.asarray(scale, np.float32), np.asarray(bias, np.float32)
    assert scale.shape == bias.shape == (v.shape[2],), (scale.shape, bias.shape, v.shape)
    y = ((v.astype(np.float32) * scale).astype(np.float32) + bias).astype(np.float32)
    assert np.isfinite(y).all()
    if sample == F32:
        stored, bits = y, y.view(np.uint32)
    elif sample == F16:
        with np.errstate(over="ignore"):
            h = np.ascontiguousarray(y.astype(np.float16))
        stored, bits = h.astype(np.float32), h.view(np.uint16)
    elif sample == BF16:
        bits = bf16_bits(y)
        stored = (bits.astype(np.uint32) << 16).view(np.float32)
    else:
        raise ValueError(sample)
    # unspecified ground: a stored value that is subnormal in its type (non-zero, below the smallest normal), or what would become
    # one (a y below the type's smallest normal that is stored as zero)
    low = np.abs(np.where(stored != 0, stored, y).astype(np.float64))
    assert not ((low != 0) & (low < SMALLEST_NORMAL[sample])).any(), "an expected value is subnormal in the stored type"
    return np.ascontiguousarray(bits)

"""Content for the planar-input encode tests (tests/test_planar_encode.py, tests/test_planar_encode_cpu.py): pictures
as (C, H, W) arrays whose planes and positions can be told apart -- every plane from a seed of its own, plus a ramp in x and a ramp
in y with slopes of the plane's own -- so that two swapped planes, or an offset of one line or of 8 pixels, change the stream."""
import numpy as np

SLOPES = ((3, 5), (7, 2), (5, 11))  # (per pixel in x, per line in y) of planes 0, 1, 2: odd in one axis at least, all different


def planes(w: int, h: int, seed: int, components: int = 3, bits: int = 8) -> np.ndarray:
    """(components, h, w) uint8 (bits == 8) or uint16 samples below 2^bits."""
    top = 1 << bits
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    out = np.empty((components, h, w), np.uint8 if bits == 8 else np.uint16)
    for c in range(components):
        noise = np.random.default_rng(seed * 3 + c).integers(0, top // 8, (h, w))
        sx, sy = SLOPES[c]
        out[c] = (noise + (x * sx + y * sy) * (top // 256) + c * (top // 3)) % top
    return out


def tells_planes_and_positions_apart(p: np.ndarray) -> bool:
    """The planes differ from one another, and no plane is constant along either axis (where that axis has two samples)."""
    c, h, w = p.shape
    for a in range(c):
        for b in range(a + 1, c):
            if np.array_equal(p[a], p[b]):
                return False
    for a in range(c):
        if w > 1 and not (p[a][:, 1:] != p[a][:, :-1]).any(axis=1).all():  # every line changes along x
            return False
        if h > 1 and not (p[a][1:, :] != p[a][:-1, :]).any(axis=0).all():  # every column changes along y
            return False
    return True


def shifted_differs(p: np.ndarray) -> bool:
    """Content that an offset of one line or of 8 pixels does not map onto itself (pictures larger than the offset)."""
    c, h, w = p.shape
    ok = True
    if h > 1:
        ok = ok and not np.array_equal(p[:, 1:, :], p[:, :-1, :])
    if w > 8:
        ok = ok and not np.array_equal(p[:, :, 8:], p[:, :, :-8])
    return ok

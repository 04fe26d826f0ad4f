"""The resized call's filter (include/mijpeg.h) restated in numpy, from its definition alone: a separable triangle filter in
integer arithmetic whose support grows with the reduction, the horizontal pass first and rounded to 8 bits, the vertical pass on that
result.  What the GPU tests expect is resize() of the oracle's decode, at tolerance 0.  (Not a test module: pytest collects test_*.py.)"""
import functools

import numpy as np

ONE = 1 << 14


def bound(n, m):
    """The definition's bound of the tap count."""
    return min(n, 2 * -(-max(n, m) // m) + 1)


@functools.lru_cache(maxsize=None)
def taps(n, m):
    """One axis, n source samples -> m output samples: (first, count, weights) -- int64 arrays of m entries and an (m, max count) array of
    weights, zero behind an output's count.  Python integers throughout (exact at any size)."""
    S = 2 * max(n, m)
    firsts, runs = [], []
    for o in range(m):
        centre = (2 * o + 1) * n
        # w(i) > 0 <=> centre - S < (2i + 1) m < centre + S
        lo = max(0, (centre - S) // (2 * m) - 1)
        hi = min(n - 1, (centre + S) // (2 * m) + 1)
        w = [(i, S - abs((2 * i + 1) * m - centre)) for i in range(lo, hi + 1)]
        w = [(i, v) for i, v in w if v > 0]
        assert w and [i for i, _ in w] == list(range(w[0][0], w[0][0] + len(w))), (n, m, o)
        W = sum(v for _, v in w)
        k = [(v * ONE + W // 2) // W for _, v in w]
        big = max(v for _, v in w)
        k[[v for _, v in w].index(big)] += ONE - sum(k)  # (index: the lowest tap with the largest w)
        assert sum(k) == ONE and min(k) >= 0
        firsts.append(w[0][0])
        runs.append(k)
    cap = max(len(k) for k in runs)
    weights = np.zeros((m, cap), np.int64)
    for o, k in enumerate(runs):
        weights[o, :len(k)] = k
    return np.array(firsts, np.int64), np.array([len(k) for k in runs], np.int64), weights


def _axis(img, m):
    """The filter along axis 0 of an integer array (n, ...) -> (m, ...), rounded and clamped to 8 bits."""
    first, count, weights = taps(img.shape[0], m)
    out = np.empty((m,) + img.shape[1:], np.int64)
    for o in range(m):
        k = weights[o, :count[o]].reshape((-1,) + (1,) * (img.ndim - 1))
        out[o] = np.minimum(255, ((k * img[first[o]:first[o] + count[o]]).sum(axis=0) + (ONE >> 1)) >> 14)
    return out


def resize(img, ow, oh):
    """(h, w, c) or (h, w) uint8 -> (oh, ow, c) / (oh, ow) uint8: horizontally, then vertically."""
    a = np.asarray(img).astype(np.int64)
    a = np.swapaxes(_axis(np.swapaxes(a, 0, 1), ow), 0, 1)
    return _axis(a, oh).astype(np.uint8)

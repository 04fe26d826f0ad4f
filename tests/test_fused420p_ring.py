"""fused420p_kernel, phase A: two waves transform the tile's 8 x 8 interior chroma blocks of Cb and Cr in full, the other two take
the ring around them as single columns (left / right neighbours), single lines (the blocks above / below) and single samples
(the corners).  Every case is compared byte for byte with the oracle: synthetic coefficient planes through
api.launch_reconstruct (as test_pruned_idct_paths does), real streams through the ragged batch.

Shapes: 128 x 128 has no neighbour tile, 256 x 128 / 128 x 256 one, 384 x 384 a centre tile with all eight, 391 x 377 partial
last tiles (the ring meets the replicated edge), 130 x 130 / 144 x 144 a neighbour tile of one chroma column / one chroma block.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from libjpeg_amd import api, synth

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128), (256, 128), (128, 256), (384, 384), (391, 377), (130, 130), (144, 144)]
BIG = [(384, 384), (391, 377)]
FLAT_Q = [2] + [1] * 63  # the deltas of every synthetic case: sum |c| q of a block is easy to place


@functools.lru_cache(maxsize=None)
def _stream(w, h):
    return synth.synth_jpeg(w, h, 11 + w + h, 85, "420", 0)


def _frame(oracle, w, h, quant=FLAT_Q):
    """-> (the library's description of a w x h 4:2:0 frame, the oracle's), both with `quant` in every table."""
    d = api.Decoder(0)
    src = d.read(_stream(w, h))
    f = api.MijpegInfo()
    C.memmove(C.byref(f), C.byref(src), C.sizeof(api.MijpegInfo))
    d.close()
    info, _ = oracle.decode_coefficients(_stream(w, h))
    for t in range(4):
        for i in range(64):
            info.quant[t][i] = quant[i]
            f.quant[t][i] = quant[i]
    info.scan_state_valid = 0  # the tables set here, not the ones the scans of the stream latched per component
    return f, info


def _blocks(info, c):
    return info.bh[c], info.bw[c]


def _luma(rng, bh, bw):
    p = rng.integers(-3, 4, size=(bh, bw, 8, 8)).astype(np.int32)
    p[rng.random(p.shape) < 0.5] = 0
    p[..., 0, 0] = rng.integers(-60, 61, size=(bh, bw))
    return p


def _corner4x4(rng, bh, bw):
    p = np.zeros((bh, bw, 8, 8), np.int32)
    p[:, :, :4, :4] = rng.integers(-5, 6, size=(bh, bw, 4, 4))
    p[..., 0, 0] = rng.integers(-40, 41, size=(bh, bw))
    return p


def _rows03(rng, bh, bw):
    p = np.zeros((bh, bw, 8, 8), np.int32)
    p[:, :, :4, :] = rng.integers(-5, 6, size=(bh, bw, 4, 8))
    p[:, :, 0, 7] = rng.choice([-9, 9], size=(bh, bw))  # (columns 4..7 never all zero)
    p[..., 0, 0] = rng.integers(-40, 41, size=(bh, bw))
    return p


def _dense(rng, bh, bw):
    p = rng.integers(1, 6, size=(bh, bw, 8, 8)).astype(np.int32) * rng.choice([-1, 1], size=(bh, bw, 8, 8))
    p[..., 0, 0] = rng.integers(1, 41, size=(bh, bw)) * rng.choice([-1, 1], size=(bh, bw))
    assert (p != 0).all()
    return p


def _centre_differs(centre, others):
    """The 8 x 8 chroma blocks of tile (1, 1) from one generator, every other tile's from another: in the centre tile the interior
    waves and the ring waves then see different contents and choose different transform tiers, and so do its neighbours'."""
    def make(rng, bh, bw):
        p = others(rng, bh, bw)
        q = centre(rng, bh, bw)
        p[8:16, 8:16] = q[8:16, 8:16]
        return p
    return make


def _own_dc_and_highest_frequency(rng, bh, bw):
    """Every block its own DC and large terms of the highest horizontal, vertical and diagonal frequency with signs of their own:
    column 0 and column 7, line 0 and line 7 of a block then differ by hundreds, and so do neighbouring blocks."""
    p = np.zeros((bh, bw, 8, 8), np.int32)
    p[..., 0, 0] = rng.integers(-150, 151, size=(bh, bw))
    for v, u in ((7, 7), (0, 7), (7, 0)):
        p[..., v, u] = rng.integers(200, 401, size=(bh, bw)) * rng.choice([-1, 1], size=(bh, bw))
    return p


CONTENTS = {
    "corner4x4": _corner4x4,
    "rows03": _rows03,
    "dense": _dense,
    "ring_dense_interior_sparse": _centre_differs(_corner4x4, _dense),
    "ring_sparse_interior_dense": _centre_differs(_dense, _corner4x4),
    "own_dc_and_highest_frequency": _own_dc_and_highest_frequency,
}


def _at_budget(rng, bh, bw, budget):
    """Blocks whose sum |c| q is exactly `budget` under FLAT_Q: the DC term alone, one AC coefficient, dense ones (the generator of
    test_gpu_parity._extreme_coefficients)."""
    p = np.zeros((bh, bw, 64), np.int32)
    kind = rng.integers(0, 4, size=(bh, bw))
    sign = rng.choice([-1, 1], size=(bh, bw))
    p[..., 0] = np.where(kind == 0, sign * (budget // 2), 0)
    k = rng.integers(1, 64, size=(bh, bw))
    for by in range(bh):
        for bx in range(bw):
            if kind[by, bx] == 1:
                p[by, bx, k[by, bx]] = sign[by, bx] * budget
            elif kind[by, bx] >= 2:
                v = rng.integers(-40, 41, size=64)
                v[0] = 0
                v = (v * (budget / max(1, int(np.abs(v).sum())))).astype(np.int64)
                v[1] += np.sign(v[1] or 1) * (budget - int(np.abs(v).sum()))
                p[by, bx] = v
    return p.reshape(bh, bw, 8, 8)


def _planes(info, rng, chroma, luma=_luma):
    out = []
    for c in range(3):
        bh, bw = _blocks(info, c)
        out.append((chroma if c else luma)(rng, bh, bw).reshape(bh, bw, 64))
    return out


def _range_max(planes, c, quant):
    return int((np.abs(planes[c]).astype(np.int64) * np.array(quant, np.int64)).sum(axis=2).max())


def _store(planes):
    return np.concatenate([p.astype(np.int16).reshape(-1) for p in planes])


def _launch(f, stores, w, h, **kw):
    import torch

    assert torch.cuda.is_available()
    n = len(stores)
    coef = torch.from_numpy(np.stack(stores)).cuda()
    row = w * 3
    out = torch.zeros((n, h, row), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), n, row, h * row, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, h, w, 3)


def _check(res, exp, what=""):
    bad = int((res != exp).sum())
    assert bad == 0, f"{what}: {bad} differing samples, first at {np.argwhere(res != exp)[:4].tolist()}"


def _run(oracle, w, h, chroma, seed, luma=_luma):
    f, info = _frame(oracle, w, h)
    planes = _planes(info, np.random.default_rng(seed), chroma, luma)
    for c in range(3):
        f.range_max[c] = _range_max(planes, c, FLAT_Q)
    f.fast_arith = 1
    assert max(f.range_max[1], f.range_max[2]) < 2047, list(f.range_max)
    assert api.kernel_name(f) == "fused420p_kernel"
    _check(_launch(f, [_store(planes)], w, h)[0], oracle.reconstruct(info, planes), f"{w}x{h}")
    return f


@pytest.mark.parametrize("w,h", SHAPES)
def test_ring_on_every_tile_arrangement(oracle, w, h):
    """No neighbour, one, all eight, partial last tiles, neighbours of one chroma column / block -- with contents that change pixels
    when column 0 is taken for column 7, line 0 for line 7, or a sample from the wrong neighbour."""
    _run(oracle, w, h, _own_dc_and_highest_frequency, 1000 + w + h)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("w,h", BIG)
def test_ring_contents(oracle, w, h, content):
    """Chroma in the 4 x 4 corner, in rows 0..3, in all 64 coefficients; ring and interior of different density, both ways."""
    _run(oracle, w, h, CONTENTS[content], sorted(CONTENTS).index(content) * 7 + w)


@pytest.mark.parametrize("budget", [1476, 2046])
@pytest.mark.parametrize("w,h", BIG)
def test_ring_at_the_gates(oracle, w, h, budget):
    """Every block of every component at sum |c| q = budget: 1476 admits the 16-bit second pass (the D2 instantiation), 2046 is the
    packed gate and takes the other one."""
    def gen(rng, bh, bw):
        return _at_budget(rng, bh, bw, budget)
    f = _run(oracle, w, h, gen, budget + w, luma=gen)
    assert list(f.range_max[:3]) == [budget] * 3


@pytest.mark.parametrize("w,h", BIG)
def test_ring_with_per_frame_tables(oracle, w, h):
    """The same frames through tables in device memory (the QDEV instantiation): three frames of different contents, each with
    deltas of its own."""
    import torch

    tables = [FLAT_Q, [3] + [1 + (i % 3 == 0) for i in range(1, 64)], [1] * 64]
    names = ["own_dc_and_highest_frequency", "dense", "ring_dense_interior_sparse"]
    frames = []
    for i, (q, name) in enumerate(zip(tables, names)):
        f, info = _frame(oracle, w, h, q)
        planes = _planes(info, np.random.default_rng(300 + i + w), CONTENTS[name])
        frames.append((f, info, planes, q))
    f = frames[0][0]
    tabs = np.ones((3, 4, 64), np.uint16)
    for i, (_, _, _, q) in enumerate(frames):
        tabs[i, :3] = np.array(q, np.uint16)
    for c in range(3):
        f.quant_index[c] = c
        for k in range(64):
            f.quant[c][k] = int(tabs[:, c, k].max())
        f.range_max[c] = max(_range_max(planes, c, q) for _, _, planes, q in frames)
    f.fast_arith = 1
    assert max(f.range_max[1], f.range_max[2]) < 2047, list(f.range_max)
    assert api.kernel_name(f).split("/")[0] == "fused420p_kernel"
    qd = torch.from_numpy(tabs.view(np.int16)).cuda()
    wsb = api.workspace_bytes(f, 3, 0, own_tables=True)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    res = _launch(f, [_store(planes) for _, _, planes, _ in frames], w, h, workspace=ws.data_ptr(), workspace_bytes=wsb, quant_dev=qd.data_ptr())
    for i, (_, info, planes, _) in enumerate(frames):
        _check(res[i], oracle.reconstruct(info, planes), f"frame {i}")


def test_ring_in_a_ragged_batch(oracle):
    """384 x 384 and 391 x 377 (twice each, different pictures and qualities) in one ragged launch."""
    import torch

    jobs = [(384, 384, 1, 90), (391, 377, 2, 75), (384, 384, 3, 60), (391, 377, 4, 95)]
    streams = [synth.synth_jpeg(w, h, seed, q, "420", 0) for w, h, seed, q in jobs]
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams) == [0] * len(streams)
    outs = []
    for i, (w, h, _, _) in enumerate(jobs):
        f = d.ragged_info(i)
        assert d.ragged_route(i)[0], d.ragged_route(i)
        b = api.MijpegBatch()
        C.memmove(C.byref(b.info), C.byref(f), C.sizeof(api.MijpegInfo))
        b.frames = 1
        b.quant_dev = 16  # (only asked whether it is set)
        assert api.lib().mijpeg_kernel_name(C.byref(b)).decode().split("/")[0] == "fused420p_kernel"
        outs.append(torch.zeros((h, w * 3), dtype=torch.uint8, device="cuda"))
    d.reconstruct_ragged_device([o.data_ptr() for o in outs], [o.shape[1] for o in outs])
    st = d.ragged_stats()
    d.close()
    assert st["ragged"] == len(streams) and st["fallbacks"] == 0, st
    for (w, h, _, _), o, s in zip(jobs, outs, streams):
        _check(o.cpu().numpy().reshape(h, w, 3), oracle.decode(s), f"{w}x{h}")

"""fused_tile_kernel, fused_flat_kernel and the pair idct_planes_kernel + upsample_color_kernel (with its int32 twin
idct_planes_long_kernel) at their arithmetic gates ("The tile, flat and pair kernels at their gates"): the int16 sample
planes below GATE_INT16_SAMPLES = 7600, the 24-bit multiply-adds of the FAST flavour below 16384 and of fast12 below GATE_12_CHROMA =
45056, the wrapping SAFE flavour beyond.  The pattern is test_gpu_parity._extreme_coefficients': crafted coefficient planes go straight
into api.launch_reconstruct, range_max and fast_arith are set here, the oracle reconstructs the same planes under the same tables, and
the comparison is np.array_equal.

Crafting rule: a component has one delta d for all 64 terms and every one of its blocks has sum |c| = units, so sum |c| q is d * units
to the unit in every block (SPLIT) -- the DC term alone, one AC coefficient of either sign at a random position, or a dense block
(craft.blocks_at).  Three blocks of every plane of a 141 x 150 frame are pinned: the whole budget on coefficient 9 (row 1, column 1:
the largest basis amplitude, |sample * 16| about 3.85 B) with either sign and on the DC term, next to each other across block columns
8 and 16 where the plane is that wide.  Every component has a table of its own, so one component alone can step over a gate.

A 9 x 23 frame is a few blocks per plane, and a block of a saturating kind blanks its share of the picture: there ONE visible block
per plane is of that kind (a pinned one at a budget, a wrapping one, one with a coefficient beyond 16 bits), in the corner where both
edges are replicated, and the other visible blocks keep their samples spread over the range (_few_blocks) -- a wrong edge or filter
term shows instead of saturating away.

The header comes from craft.craft_stream, which writes any component count and any factors; its entropy coded data is not used.  The
CPU test pins the premises: range_max to the unit, the kernel every flag combination selects, that the rule for fast_arith used here
is the host decoder's, and that every picture of the oracle's is no trivial one: both ends of the range and at least 64 distinct
values at a budget (measured: 256 at 141 x 150 and 73 or more at 9 x 23 at 8 bit, 3879 and 286 or more at 12 bit), at least 50 for
wrap-around content (131 / 135 or more), at least a quarter of an int32 picture strictly inside the range (0.32 / 0.65 or more)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import craft
from libjpeg_amd import api, synth

NOCT, SAFE, GENERIC = api.FLAG_NO_COLOR_TRANSFORM, api.FLAG_FORCE_SAFE, api.FLAG_FORCE_GENERIC
TILE, FLAT = "fused_tile_kernel", "fused_flat_kernel"
PAIR, LONG = "idct_planes_kernel+upsample_color_kernel", "idct_planes_long_kernel+upsample_color_kernel"

LAYOUTS = {"3x1": [(3, 1), (1, 1), (1, 1)], "1x3": [(1, 3), (1, 1), (1, 1)], "1x4": [(1, 4), (1, 1), (1, 1)], "4x2": [(4, 2), (1, 1), (1, 1)],
           "lumasub": [(1, 1), (2, 2), (2, 2)], "mixed": [(2, 2), (2, 1), (1, 2)], "two": [(2, 1), (1, 2)], "four": [(2, 2), (1, 1), (2, 1), (1, 2)],
           "cmyk": [(1, 1)] * 4, "rgb": [(1, 1)] * 3, "420noct": [(2, 2), (1, 1), (1, 1)],
           "440": [(1, 2), (1, 1), (1, 1)], "411": [(4, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}
OWN_FLAG = {"rgb": NOCT, "420noct": NOCT}  # the flag without which a dedicated fused kernel takes the layout
LAYOUTS8 = ["3x1", "1x3", "1x4", "4x2", "lumasub", "mixed", "two", "four", "cmyk", "rgb", "420noct"]
LAYOUTS12 = ["3x1", "4x2", "lumasub", "440", "411"]
WIDE = [("3x1", 8), ("two", 8), ("cmyk", 8), ("420", 8), ("3x1", 12)]
BIG, SMALL = (141, 150), (9, 23)  # several tiles each way with partial MCUs at both edges; narrower than one MCU of a subsampled layout

# budget -> (delta, units) pairs with delta * units == budget: delta <= 255 at 8 bit, units <= 32767 (int16 coefficient planes)
SPLIT = {7599: [(3, 2533), (51, 149)], 7600: [(2, 3800), (16, 475)], 8189: [(19, 431)], 16383: [(3, 5461), (43, 381)], 16384: [(2, 8192)],
         45055: [(5, 9011)], 45056: [(2, 22528)], 49152: [(2, 24576)], 1000: [(2, 500)]}
GATES8 = (7599, 7600, 8189, 16383, 16384)
CASES12 = ((45055, 45055, 45055), (45055, 45056, 45055), (45056, 1000, 1000), (49152, 45055, 45055))
TABLE_BUDGETS = (7599, 7600, 16383)  # per-frame tables: the budgets with two factorizations


def _contents8(layout):
    """Every component at every gate, wrap-around content, and component 0 below the int16 line with the last one on it."""
    nc = len(LAYOUTS[layout])
    return [(b,) * nc for b in GATES8] + ["wrap", (7599,) * (nc - 1) + (7600,)]


def _shapes(layout):
    return [BIG + (1,), SMALL + (1,)] + ([SMALL + (3,)] if layout in ("1x4", "cmyk") else [])


# ------------------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def _header(layout, precision, w, h):
    samp = LAYOUTS[layout]
    data = craft.craft_stream(np.random.default_rng(len(layout) + w), samp, w, h, tq=list(range(len(samp))))
    return synth.to_12bit(data, 16) if precision == 12 else data


def _mijpeg_info(layout, precision, w, h):
    d = api.Decoder(None)
    f = d.read(_header(layout, precision, w, h), entropy="host")
    d.close()
    assert (f.width, f.height, f.precision, f.components) == (w, h, precision, len(LAYOUTS[layout]))
    assert [f.quant_index[c] for c in range(f.components)] == list(range(f.components)) and not f.coef_wide
    return f


def _pin_blocks(p, units, turn):
    """The whole budget on coefficient 9 with either sign and on DC, in three neighbouring blocks across block columns 8 and 16 (row 1
    and the last row) where the plane is that wide, in its first three blocks otherwise; `turn` rotates the order."""
    bh, bw = p.shape[:2]
    kinds = [(9, units), (9, -units), (0, units)]
    cells = [(by, start + i, (i + gi + turn) % 3) for gi, (by, start) in enumerate(((min(1, bh - 1), 7), (bh - 1, 15))) if bw >= start + 3 for i in range(3)]
    if not cells:
        cells = [(j // bw, j % bw, (j + turn) % 3) for j in range(3)]
    for by, bx, kind in cells:
        p[by, bx] = 0
        p[by, bx, kinds[kind][0]] = kinds[kind][1]


def _few_blocks(f, c):
    """The rule for the planes of a 9 x 23 frame, whatever the content.  Such a picture is a few blocks, and one block of a saturating
    kind blanks its share of it; so ONE visible block per plane is of that kind -- the last one, in the corner where the right and the
    bottom edge are both replicated -- and the other visible blocks are of a kind whose samples spread over the range (_spread_block at a
    budget).  A plane with a single visible block has no corner block.  Blocks that only pad the MCU follow the general recipe.
    -> None for the planes of a 141 x 150 frame, else (mask of the visible blocks that are no corner, corner cell or None)"""
    if f.blocks_w[c] * f.blocks_h[c] > 16:
        return None
    vbw, vbh = ((f.width + f.subx[c] - 1) // f.subx[c] + 7) // 8, ((f.height + f.suby[c] - 1) // f.suby[c] + 7) // 8
    inside = np.zeros((f.blocks_h[c], f.blocks_w[c]), bool)
    inside[:vbh, :vbw] = True
    corner = (vbh - 1, vbw - 1) if vbh * vbw > 1 else None
    if corner:
        inside[corner] = False
    return inside, corner


def _spread_block(rng, f, budget, units):
    """A block at the budget whose samples spread over the range without leaving most of it: sum |c| = units on n AC terms of equal
    share and random sign gives samples of rms budget / (8 sqrt(n)) (the transform is orthonormal); n makes that 0.7 of half the range
    where 63 terms allow -- craft.dense_block itself at the 8-bit gates (rms 119..256), about 15 terms at the 12-bit ones."""
    n = int((budget / (8 * 0.7 * (1 << (f.precision - 1)))) ** 2)
    if n >= 63:
        return craft.dense_block(rng, units)
    n = max(2, min(n, units))
    v = np.zeros(64, np.int64)
    where = rng.choice(np.arange(1, 64), size=n, replace=False)
    v[where] = units // n
    v[where[0]] += units - n * (units // n)
    v[where] *= rng.choice([-1, 1], size=n)
    return v


def _budget_plane(rng, f, c, budget, units, turn):
    p = craft.blocks_at(rng, f.blocks_h[c], f.blocks_w[c], units)
    few = _few_blocks(f, c)
    if few is None:
        _pin_blocks(p, units, turn)
    else:
        inside, corner = few
        for by, bx in np.argwhere(inside):
            p[by, bx] = _spread_block(rng, f, budget, units)
        if corner:
            p[corner] = 0
            p[corner][(9, 9, 0)[turn % 3]] = (units, -units, units)[turn % 3]
    assert (np.abs(p).sum(axis=2) == units).all()
    return p


def _wrap_plane(rng, f, c, q):
    """test_adversarial_coefficients_safe_flavour's content: |c| <= 32767, half of them zero (the deltas are 1..255).  The quiet blocks
    of a 9 x 23 frame (_few_blocks): a DC term and twelve AC terms of a few hundred after dequantisation."""
    shape = (f.blocks_h[c], f.blocks_w[c], 64)
    p = rng.integers(-32767, 32768, size=shape).astype(np.int32)
    p[rng.random(shape) < 0.5] = 0
    few = _few_blocks(f, c)
    if few is not None:
        for by, bx in np.argwhere(few[0]):
            target = np.zeros(64)
            target[0] = rng.integers(-600, 601)
            target[rng.choice(np.arange(1, 64), size=12, replace=False)] = rng.choice([-1, 1], size=12) * rng.integers(100, 401, size=12)
            p[by, bx] = np.rint(target / q).astype(np.int32)
    return p


def _wide_plane(rng, f, c):
    """Deltas of 3: sparse AC terms in +-6 on a DC term in +-150, in a third of the blocks one coefficient at a random position replaced
    by +-(32768 .. 2 000 000), and in a few blocks the DC term itself beyond 16 bits.  In a 9 x 23 frame (_few_blocks) the corner block
    has such a coefficient and the other visible blocks have neither."""
    shape = (f.blocks_h[c], f.blocks_w[c], 64)
    p = rng.integers(-6, 7, size=shape).astype(np.int32)
    p[rng.random(shape) < 0.85] = 0
    p[..., 0] = rng.integers(-150, 151, size=shape[:2])
    flat = p.reshape(-1, 64)
    few = _few_blocks(f, c)
    allowed = np.ones(len(flat), bool) if few is None else ~few[0].reshape(-1)
    huge = (rng.random(len(flat)) < 1 / 3) & allowed
    if few is not None and few[1]:
        huge[few[1][0] * shape[1] + few[1][1]] = True
    for b in np.flatnonzero(huge):
        flat[b, rng.integers(0, 64)] = int(rng.choice([-1, 1])) * int(rng.integers(32768, 2_000_001))
    where = np.flatnonzero(allowed)
    for b in rng.choice(where, size=min(len(where), max(1, len(flat) // 40)), replace=False):
        flat[b, 0] = int(rng.choice([-1, 1])) * int(rng.integers(40_000, 100_001))
    return p


def _range_max(planes, tables):
    return [int(min((np.abs(p).astype(np.int64) * np.asarray(q, np.int64)).sum(axis=2).max(), 0x7fffffff)) for p, q in zip(planes, tables)]


def _fast_rule(precision, ranges):
    """host_decoder.cpp, publish(): the fast flavour is for 8-bit frames with sum |c| q < 16384 in every block"""
    return 1 if precision == 8 and all(r < 16384 for r in ranges) else 0


class Case:
    """One launch: `frames` frames of one layout, each with planes and tables (one per component) of its own."""

    def __init__(self, layout, precision, w, h, frames, content, planes, tables, wide=False):
        self.layout, self.precision, self.w, self.h, self.frames, self.content, self.wide = layout, precision, w, h, frames, content, wide
        self.planes, self.tables = planes, tables
        self.ranges = [_range_max(p, t) for p, t in zip(planes, tables)]
        self.range_max = [max(r[c] for r in self.ranges) for c in range(len(LAYOUTS[layout]))]
        self.fast = 0 if wide else _fast_rule(precision, self.range_max)
        self.own_flag = OWN_FLAG.get(layout, 0)

    def __repr__(self):
        return f"{self.layout}/{self.precision} {self.w}x{self.h}x{self.frames} {self.content}"

    def info(self, own_tables=False):
        """The frame description of the launch: the case's tables (the per-entry maxima where every frame brings its own), its ranges
        and the arithmetic flavour they allow; int32 planes the way HostDecoder::decode_wide describes them."""
        f = _mijpeg_info(self.layout, self.precision, self.w, self.h)
        assert own_tables or self.frames == 1 or all(np.array_equal(t, self.tables[0]) for t in self.tables)
        for c in range(f.components):
            q = np.max([t[c] for t in self.tables], axis=0)
            for i in range(64):
                f.quant[c][i] = int(q[i])
            f.range_max[c] = self.range_max[c]
        f.fast_arith = self.fast
        if self.wide:
            f.coef_wide = 1
            for c in range(f.components):
                f.coef_offset[c] *= 2
            f.coef_count *= 2
        return f

    def expected_kernel(self, flags, own_tables=False):
        if self.wide:
            return LONG
        if own_tables or flags & GENERIC:
            return PAIR
        return FLAT if self.layout in ("cmyk", "rgb") and self.fast and not flags & SAFE else TILE

    def int16_planes(self, flags):
        """reconstruct_device.cpp generic_args_of: a.narrow"""
        return bool(self.fast and not flags & SAFE and self.precision == 8 and all(r < 7600 for r in self.range_max))


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def _case(layout, precision, w, h, frames, content, per_frame_tables=False):
    """content: a tuple of budgets per component (every block of component c at sum |c| q = content[c]; with per_frame_tables, frame i
    under the i-th factorization of the budget), "wrap" (test_adversarial_coefficients_safe_flavour's: |c| <= 32767 with half of them
    zero under deltas of 1..255) or "wide" (int32 planes: see _wide_plane)."""
    f = _mijpeg_info(layout, precision, w, h)
    rng = np.random.default_rng(_seed(layout, precision, w, h, frames, content, per_frame_tables))
    shapes = range(f.components)
    planes, tables = [], []
    for i in range(frames):
        if content == "wrap":
            qs = [rng.integers(1, 256, size=64) for _ in shapes] if per_frame_tables or i == 0 else tables[0]
            ps = [_wrap_plane(rng, f, c, qs[c]) for c in range(f.components)]
        elif content == "wide":
            ps, qs = [_wide_plane(rng, f, c) for c in range(f.components)], [np.full(64, 3)] * f.components
        else:
            ps, qs = [], []
            for c in range(f.components):
                d, units = SPLIT[content[c]][i if per_frame_tables else 0]
                assert d * units == content[c]
                ps.append(_budget_plane(rng, f, c, content[c], units, i + c))
                qs.append(np.full(64, d))
        planes.append(ps)
        tables.append(qs)
    case = Case(layout, precision, w, h, frames, content, planes, tables, wide=content == "wide")
    if isinstance(content, tuple):  # nothing else is trusted
        assert all(r == list(content) for r in case.ranges), (case, case.ranges)
    return case


@functools.lru_cache(maxsize=None)
def _expected(oracle, case):
    """The oracle's picture of every frame under the frame's own tables (computed once per case, shared, read-only)."""
    out = []
    for planes, tables in zip(case.planes, case.tables):
        info, _ = oracle.decode_coefficients(_header(case.layout, case.precision, case.w, case.h))
        assert [info.tq[c] for c in range(info.ncomp)] == list(range(info.ncomp))
        for c, q in enumerate(tables):
            for i in range(64):
                info.quant[c][i] = int(q[i])
        info.scan_state_valid = 0  # the tables set here, not the ones the header's scan latched
        pic = (oracle.reconstruct16 if case.precision == 12 else oracle.reconstruct)(info, planes, 0 if case.own_flag else -1)
        pic.setflags(write=False)
        out.append(pic)
    return tuple(out)


def _kernel_name(f, flags, own_tables=False):
    b = api.MijpegBatch()
    C.memmove(C.byref(b.info), C.byref(f), C.sizeof(api.MijpegInfo))
    b.flags = flags
    if own_tables:  # only asked whether it is set
        b.quant_dev = 16
    return api.lib().mijpeg_kernel_name(C.byref(b)).decode()


def _all_cases():
    for layout in LAYOUTS8:
        for w, h, frames in _shapes(layout):
            for content in _contents8(layout):
                yield _case(layout, 8, w, h, frames, content)
    for layout in LAYOUTS12:
        for w, h in (BIG, SMALL):
            for content in CASES12:
                yield _case(layout, 12, w, h, 1, content)
    for layout in ("3x1", "two"):
        for w, h in (BIG, SMALL):
            for content in [(b,) * len(LAYOUTS[layout]) for b in TABLE_BUDGETS] + ["wrap"]:
                yield _case(layout, 8, w, h, 2, content, True)
    for layout, precision in WIDE:
        for w, h in (BIG, SMALL):
            yield _case(layout, precision, w, h, 1, "wide")


# ------------------------------------------------------------------------------------------------ CPU: the premises
def test_the_crafted_frames_are_what_they_claim(oracle):
    for budget, pairs in SPLIT.items():
        for d, units in pairs:
            assert d * units == budget and d <= 255 and units <= 32767
    assert all(len(SPLIT[b]) == 2 and SPLIT[b][0] != SPLIT[b][1] for b in TABLE_BUDGETS)
    seen = set()
    for case in _all_cases():
        own_tables = case.frames == 2
        f = case.info(own_tables)
        o = case.own_flag
        nc = f.components
        seen.add((case.layout, case.precision, case.content if isinstance(case.content, str) else max(case.content)))
        # the ranges, to the unit, and the arithmetic flavour they allow
        if isinstance(case.content, tuple):
            assert list(f.range_max[:nc]) == list(case.content) and f.fast_arith == _fast_rule(case.precision, case.content), case
        elif case.content == "wrap":
            assert max(case.range_max) >= 16384 and f.fast_arith == 0, case
            assert min(case.range_max) >= 16384 or (case.w, case.h) == SMALL, case  # (a plane of one visible block is quiet there)
        else:
            assert f.coef_wide == 1 and f.fast_arith == 0 and max(case.range_max) > 3 * 32768, case
            assert any(np.abs(p[..., 0]).max() > 32767 for p in case.planes[0]) and any(np.abs(p[..., 1:]).max() > 32767 for p in case.planes[0])
        if not case.wide:
            assert all(np.abs(p).max() <= 32767 for ps in case.planes for p in ps), case
        # the kernels
        if case.wide:
            assert {_kernel_name(f, o | fl) for fl in (0, SAFE, GENERIC)} == {LONG}, case
        elif own_tables:
            assert {_kernel_name(f, o | fl, True) for fl in (0, SAFE)} == {PAIR}, case
        else:
            fast_flat = case.layout in ("cmyk", "rgb") and f.fast_arith == 1
            assert _kernel_name(f, o) == (FLAT if fast_flat else TILE) == case.expected_kernel(o), (case, _kernel_name(f, o))
            assert _kernel_name(f, o | SAFE) == TILE == case.expected_kernel(o | SAFE), case
            assert _kernel_name(f, o | GENERIC) == _kernel_name(f, o | GENERIC | SAFE) == PAIR == case.expected_kernel(o | GENERIC), case
        if case.precision == 8 and case.layout in ("cmyk", "rgb") and isinstance(case.content, tuple):
            assert (case.expected_kernel(o) == TILE) == (max(case.content) >= 16384), case
        # the int16 sample planes: one component on the line switches every plane
        if case.content == (7599,) * (nc - 1) + (7600,):
            assert not case.int16_planes(GENERIC) and _case(case.layout, 8, case.w, case.h, case.frames, (7599,) * nc).int16_planes(GENERIC)
        # the oracle's pictures, every one of them: both ends of the range and many values in between (measured: see the docstring)
        top = 255 if case.precision == 8 else 4095
        for frame, pic in enumerate(_expected(oracle, case)):
            assert pic.shape == (case.h, case.w, nc) and pic.dtype == (np.uint8 if case.precision == 8 else np.uint16)
            values = np.unique(pic)
            if case.wide:
                inside = np.count_nonzero((pic > 0) & (pic < top)) / pic.size
                assert inside >= 0.25, (case, frame, inside)
            else:
                assert len(values) >= (50 if case.content == "wrap" else 64) and values[0] == 0 and values[-1] == top, (case, frame, len(values), values[0], values[-1])
        # the oracle follows the same colour decision as the kernels
        info = oracle.read_info(_header(case.layout, case.precision, case.w, case.h))
        assert bool(info.ycbcr) == bool(f.ycbcr), case
    assert seen >= {(layout, 8, b) for layout in LAYOUTS8 for b in GATES8 + ("wrap",)} | {(layout, 12, b) for layout in LAYOUTS12 for b in (45055, 45056, 49152)}
    assert seen >= {(layout, precision, "wide") for layout, precision in WIDE}


def test_the_fast_arith_rule_is_the_host_decoders():
    """fast_arith = 1 iff 8 bit and every range_max < 16384: one 3x1 frame at 16383 and one at 16384 through the coder and back."""
    hs, vs = zip(*LAYOUTS["3x1"])
    for (d, units), fast in (((43, 381), 1), ((32, 512), 0)):
        f = api.frame_layout(141, 150, 3, hs, vs, [[d] * 64, [d] * 64])
        rng = np.random.default_rng(d)
        coef = np.zeros(f.coef_count, np.int16)
        for c in range(3):
            p = _budget_plane(rng, f, c, d * units, units, c)
            coef[f.coef_offset[c]:f.coef_offset[c] + p.size] = p.reshape(-1)
        dec = api.Decoder(None)
        g = dec.read(api.encode_coefficients(f, coef, restart_interval=3), entropy="host")
        dec.close()
        assert g.restart_interval == 3 and list(g.range_max[:3]) == [d * units] * 3 and g.fast_arith == fast == _fast_rule(8, g.range_max[:3])
        assert _kernel_name(g, 0) == TILE
    f = _mijpeg_info("3x1", 12, 9, 23)  # a 12-bit frame never has it
    assert f.fast_arith == 0 == _fast_rule(12, f.range_max[:3])


# ------------------------------------------------------------------------------------------------ GPU
GUARD, SENTINEL, WS_SENTINEL = 256, 0xA5, 0x5A


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _launch(case, flags, own_tables=False):
    """One launch of the case into a guarded buffer (padded lines, padded frames) with a guarded, pre-filled workspace.
    -> (pictures, what became of the workspace's sample planes: None without workspace, else "untouched", "lower" (the lower half
    written: int16 planes) or "both")"""
    torch = _torch()
    f = case.info(own_tables)
    nc, sb = f.components, 2 if case.precision == 12 else 1
    assert _kernel_name(f, flags, own_tables) == case.expected_kernel(flags, own_tables), (case, flags)
    # coefficients: int16 planes, or int32 planes seen as int16 (coef_offset and coef_count are doubled then)
    count = f.coef_count // 2 if case.wide else f.coef_count
    coef = np.zeros((case.frames, count), np.int32 if case.wide else np.int16)
    for i, planes in enumerate(case.planes):
        for c, p in enumerate(planes):
            off = f.coef_offset[c] // 2 if case.wide else f.coef_offset[c]
            assert p.shape == (f.blocks_h[c], f.blocks_w[c], 64) and off + p.size <= count
            coef[i, off:off + p.size] = p.reshape(-1)
    coef_dev = torch.from_numpy(coef.view(np.int16).reshape(-1)).cuda()
    assert coef_dev.numel() == case.frames * f.coef_count
    quant_dev = None
    if own_tables:
        q = np.ones((case.frames, 4, 64), np.uint16)
        for i, tables in enumerate(case.tables):
            for c, t in enumerate(tables):
                q[i, c] = t
        quant_dev = torch.from_numpy(q.reshape(-1)).cuda()
    # output: guard bytes in front and behind, lines padded by an odd number of bytes (even for 16-bit samples), frames padded too
    line = case.w * nc * sb
    row, tail = line + (14 if sb == 2 else 13), 38 if sb == 2 else 37
    frame_stride = case.h * row + tail
    out = torch.full((GUARD + case.frames * frame_stride + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    # workspace: [prefix][frames x coef_count x 4 bytes of sample planes][per-frame tables]
    ws_bytes = api.workspace_bytes(f, case.frames, flags, own_tables)
    area = case.frames * f.coef_count * 4
    prefix = api.workspace_bytes(f, 1, flags) - f.coef_count * 4
    assert ws_bytes == prefix + area + (case.frames * 4 * 64 * 4 if own_tables else 0) and prefix >= 0
    ws = torch.full((GUARD + ws_bytes + GUARD,), WS_SENTINEL, dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef_dev.data_ptr(), out.data_ptr() + GUARD, case.frames, row, frame_stride, flags=flags,
                           workspace=ws.data_ptr() + GUARD, workspace_bytes=ws_bytes, stream=torch.cuda.current_stream().cuda_stream,
                           quant_dev=quant_dev.data_ptr() if own_tables else 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    body = got[GUARD:GUARD + case.frames * frame_stride].reshape(case.frames, frame_stride)
    lines = body[:, :case.h * row].reshape(case.frames, case.h, row)
    # no byte outside width x components x sample bytes of a line changed
    assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), (case, flags, "guard bytes")
    assert (lines[:, :, line:] == SENTINEL).all() and (body[:, case.h * row:] == SENTINEL).all(), (case, flags, "padding bytes")
    pics = [np.ascontiguousarray(lines[i, :, :line]).view(np.uint16 if sb == 2 else np.uint8).reshape(case.h, case.w, nc) for i in range(case.frames)]
    w = ws.cpu().numpy()
    assert (w[:GUARD] == WS_SENTINEL).all() and (w[-GUARD:] == WS_SENTINEL).all() and (w[GUARD:GUARD + prefix] == WS_SENTINEL).all(), (case, flags, "workspace guards")
    samples = w[GUARD + prefix:GUARD + prefix + area]
    lower, upper = (samples[:area // 2] != WS_SENTINEL).any(), (samples[area // 2:] != WS_SENTINEL).any()
    state = {(False, False): "untouched", (True, False): "lower", (True, True): "both"}[(bool(lower), bool(upper))]
    return pics, state


def _check(oracle, case, flags, own_tables=False):
    pics, state = _launch(case, flags, own_tables)
    for i, (pic, exp) in enumerate(zip(pics, _expected(oracle, case))):
        bad = int((pic != exp).sum())
        assert bad == 0, f"{case} flags {flags} frame {i}: {bad} differing samples, first at {np.argwhere(pic != exp)[:4].tolist()}"
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS8)
def test_8bit_gates_on_the_tile_and_flat_kernels(oracle, layout):
    """7599 (int16 planes in LDS), 7600 and 8189 (FAST on int32 planes), 16383 (the last FAST budget), 16384 and wrap-around content
    (SAFE), and one component alone on the int16 line, each as selected and under FORCE_SAFE; the kernels leave the workspace alone
    (a launch that fell back to the pair would not)."""
    o = OWN_FLAG.get(layout, 0)
    for w, h, frames in _shapes(layout):
        for content in _contents8(layout):
            case = _case(layout, 8, w, h, frames, content)
            for flags in (o, o | SAFE):
                assert case.expected_kernel(flags) in (TILE, FLAT)
                assert _check(oracle, case, flags) == "untouched", (case, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS8)
def test_8bit_gates_on_the_pair(oracle, layout):
    """The same frames under FORCE_GENERIC: the specialised upsample_color_kernel layouts through lumasub and 420noct, LAYOUT_ANY through
    the others.  The flavour shows in the workspace only: int16 sample planes fill the lower half of the planes' area and leave the
    upper one alone, int32 planes -- from 7600 on in any one component, and under FORCE_SAFE -- fill both."""
    o = OWN_FLAG.get(layout, 0)
    for w, h, frames in _shapes(layout):
        for content in _contents8(layout):
            case = _case(layout, 8, w, h, frames, content)
            for flags in (o | GENERIC, o | GENERIC | SAFE):
                want = "lower" if isinstance(content, tuple) and max(content) < 7600 and not flags & SAFE else "both"
                assert want == ("lower" if case.int16_planes(flags) else "both")
                assert _check(oracle, case, flags) == want, (case, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["3x1", "two"])
def test_per_frame_tables_on_the_pair(oracle, layout):
    """Two frames that reach the same budget under different tables (quant_dev; info.quant holds the per-entry maxima): the QDEV
    instances of the pair off 4:2:0, each frame against the oracle under its own tables."""
    nc = len(LAYOUTS[layout])
    for w, h in (BIG, SMALL):
        for content in [(b,) * nc for b in TABLE_BUDGETS] + ["wrap"]:
            case = _case(layout, 8, w, h, 2, content, True)
            assert not all(np.array_equal(a, b) for a, b in zip(*case.tables))
            for flags in (0, SAFE):
                want = "lower" if case.int16_planes(flags) else "both"
                assert want == ("lower" if content == (7599,) * nc and not flags else "both")
                assert _check(oracle, case, flags, own_tables=True) == want, (case, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS12)
def test_12bit_gates_on_the_tile_kernel_and_the_pair(oracle, layout):
    """Every component at 45055 (fast12), the second one at 45056, luma alone at 45056 (the gate is per component) and luma at 49152
    (all SAFE), on the tile kernel and the pair, against the oracle's 16-bit reconstruction."""
    for w, h in (BIG, SMALL):
        for content in CASES12:
            case = _case(layout, 12, w, h, 1, content)
            assert _check(oracle, case, 0) == "untouched", case
            assert _check(oracle, case, GENERIC) == "both", case


@pytest.mark.gpu
@pytest.mark.parametrize("layout,precision", WIDE)
def test_int32_planes_on_the_long_kernel(oracle, layout, precision):
    """coef_wide frames (what a damaged stream's out-of-range coefficients produce): idct_planes_long_kernel on coefficients and DC
    terms far beyond 16 bits, the picture still with a good share of unsaturated samples."""
    for w, h in (BIG, SMALL):
        case = _case(layout, precision, w, h, 1, "wide")
        assert case.expected_kernel(0) == LONG
        assert _check(oracle, case, 0) == "lower", case  # (the area has four bytes per 16-bit half of a coefficient: the int32 planes fill half of it)

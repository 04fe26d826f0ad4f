"""The ragged flavours of the fused reconstruction kernels (launch_fused_list, tile_enter_ragged) at their arithmetic
gates and over their launch geometry.  The uniform twins of these kernels are pinned by crafted coefficient planes through
api.launch_reconstruct, which cannot launch a ragged flavour; here the crafted planes are coded to streams (api.encode_coefficients,
host-only) and reach the ragged launches the way every list does: Decoder.decode_ragged_device + reconstruct_ragged_device.  The
reference is the oracle's decode of the same stream, the tolerance 0.

Crafting rule: every delta of a table is one value d, and every block of a plane has sum |c| = units, so that sum |c| q is d * units
in every block -- the DC term alone, one AC coefficient of either sign at a random position, or a dense block whose remainder is spent
on coefficient 1.  The entropy coder takes |AC| <= 1023 and |DC difference| <= 2047 at 8 bit (units <= 1023 with DC-only blocks of both
signs next to each other), |AC| <= 16383 and |DC difference| <= 32767 at 12 bit (units <= 16383); SPLIT holds a factorization inside
these limits for every gate.  Every crafted stream has restart intervals of 1..7 MCUs: data of this rate without markers does not let
the device walk settle, which would refuse the whole group.

The CPU test checks that every stream sits where it claims to (range_max to the unit, kernel and arithmetic flavour, layout group,
the host decoder's coefficients) and that every list selects the intended launches, so that the GPU tests cannot pass on a list that
drifted away from the gates.  The GPU tests compare every picture with np.array_equal, reconstruct into guarded buffers with padded
row strides that differ per picture, and check the statistics: no fallback, the intended number of launches."""
import functools

import numpy as np
import pytest

from craft import blocks_at as _blocks_at  # (the three kinds of blocks at a budget: shared with test_tile_pair_gates)
from libjpeg_amd import api, synth
from test_fused420p_ring import CONTENTS, _luma
from test_gpu_parity import _narrow12_chroma_limit
from test_ragged_batch import LAYOUTS, _flavour, _reconstruct_guarded

PADS8, PADS12 = (0, 4, 13), (0, 4, 14)  # bytes behind a line (12 bit: even, so that 16-bit samples stay aligned)
PAIR = "idct_planes_kernel+upsample_color_kernel"
K8 = {"420": "fused420_kernel", "420p": "fused420p_kernel", "422": "fused422_kernel", "422w": "fused422_kernel<wide>", "444": "fused444_kernel",
      "grey": "fused1_kernel"}
K12 = {"420": "fused420_kernel<12>", "422": "fused422_12_kernel", "444": "fused444_12_kernel", "grey": "fused1_kernel<12>"}

# budget -> (delta, units) pairs: delta <= 255 and units <= 1023 for the 8-bit gates, delta <= 2047 and units <= 16383 for the 12-bit ones
SPLIT = {1476: [(4, 369)], 2046: [(2, 1023), (6, 341)], 2047: [(23, 89), (89, 23)], 8189: [(19, 431)], 8190: [(90, 91)], 16383: [(43, 381)], 16384: [(32, 512)],
         49151: [(23, 2137)], 45055: [(5, 9011)], 45056: [(11, 4096)], 49152: [(24, 2048)], 16000: [(8, 2000)], 32000: [(16, 2000)],
         # the narrow12 bound of the colour stage (test_gpu_parity._narrow12_chroma_limit) for luma 16000 and 32000, and one step beyond
         23168: [(8, 2896)], 23169: [(3, 7723)], 14139: [(3, 4713)], 14140: [(4, 3535)]}
GATES8 = (1476, 2046, 2047, 8189, 8190, 16383, 16384)
N12 = {ry: _narrow12_chroma_limit(ry) for ry in (16000, 32000)}


def _split(budget, which=0):
    d, units = SPLIT[budget][which]
    assert d * units == budget
    return d, units


# ------------------------------------------------------------------------------------------------ crafted streams
def _layout(layout, w, h, precision, tables):
    hs, vs = LAYOUTS[layout]
    return api.frame_layout(w, h, len(hs), hs, vs, tables[:2 if len(hs) > 1 else 1], precision=precision)


def _code(f, planes, dri):
    coef = np.zeros(f.coef_count, np.int16)
    for c, p in enumerate(planes):
        assert p.shape[:2] == (f.blocks_h[c], f.blocks_w[c])
        coef[f.coef_offset[c]:f.coef_offset[c] + p.size] = p.reshape(-1)
    return api.encode_coefficients(f, coef, restart_interval=dri)


@functools.lru_cache(maxsize=None)
def _craft(layout, w, h, precision, dy, uy, dc, uc, seed):
    """-> (stream, planes): every luma block at sum |c| q = dy * uy, every chroma block at dc * uc; restart interval 1 + seed % 7."""
    f = _layout(layout, w, h, precision, [[dy] * 64, [dc] * 64])
    rng = np.random.default_rng(seed)
    planes = [_blocks_at(rng, f.blocks_h[c], f.blocks_w[c], uc if c else uy) for c in range(f.components)]
    return _code(f, planes, 1 + seed % 7), planes


@functools.lru_cache(maxsize=None)
def _wrap(w, h, seed):
    """The content of test_ragged_batch.test_arithmetic_outlier_inside_a_group: |c| <= 1000 under deltas of 255, half of the
    coefficients zero, DC within +-500 -- intermediates of the transforms wrap around 2^32, the SAFE flavour's business."""
    f = _layout("420", w, h, 8, [[255] * 64, [255] * 64])
    rng = np.random.default_rng(seed)
    planes = []
    for c in range(3):
        p = rng.integers(-1000, 1001, size=(f.blocks_h[c], f.blocks_w[c], 64)).astype(np.int32)
        p[rng.random(p.shape) < 0.5] = 0
        p[..., 0] = rng.integers(-500, 501, size=p.shape[:2])
        planes.append(p)
    return _code(f, planes, 1 + seed % 7), planes


@functools.lru_cache(maxsize=None)
def _photo(layout, w, h, seed, quality, dri, precision=8):
    img = synth.synth_image(w, h, seed, channels=1 if layout == "grey" else 3)
    s = synth.encode_jpeg(img, quality, "444" if layout == "grey" else layout, dri)
    return synth.to_12bit(s, 16) if precision == 12 else s


class Member:
    """One stream of a list.  budgets: (luma, chroma) sum |c| q of every block, None where the stream is not crafted to a budget;
    kernel, fast: what test_ragged_batch._flavour must say; ragged: a ragged launch takes it (else a launch of its own)."""

    def __init__(self, layout, w, h, precision, kernel, fast, make, budgets=None, ragged=True):
        self.layout, self.w, self.h, self.precision, self.kernel, self.fast = layout, w, h, precision, kernel, fast
        self.make, self.budgets, self.ragged = make, budgets, ragged

    def __repr__(self):
        return f"{self.layout}/{self.precision} {self.w}x{self.h} {self.kernel} fast={self.fast} {self.budgets}"

    @property
    def stream(self):
        r = self.make()
        return r[0] if isinstance(r, tuple) else r

    @property
    def planes(self):
        r = self.make()
        return r[1] if isinstance(r, tuple) else None

    @property
    def group(self):
        return self.layout + ("_12" if self.precision == 12 else "")

    @property
    def flavour(self):
        return self.group, self.kernel, self.fast


def _gate(layout, w, h, precision, luma, chroma, kernel, fast, seed, ragged=True, which=0):
    dy, uy = _split(luma)
    dc, uc = _split(chroma, which) if layout != "grey" else (dy, uy)
    return Member(layout, w, h, precision, kernel, fast, functools.partial(_craft, layout, w, h, precision, dy, uy, dc, uc, seed),
                  (luma, chroma if layout != "grey" else None), ragged)


def _launch(layout, precision, kernel, fast, rows, ragged=True):
    """The members of one launch.  rows: (w, h, luma budget, chroma budget, seed[, which factorization of the chroma budget]) for a
    crafted frame, (w, h, "photo", quality, seed) for an ordinary picture, (w, h, "wrap", seed) for wrap-around content."""
    out = []
    for w, h, *rest in rows:
        if rest[0] == "photo":
            quality, seed = rest[1:]
            out.append(Member(layout, w, h, precision, kernel, fast, functools.partial(_photo, layout, w, h, seed, quality, 1 + seed % 7, precision)))
        elif rest[0] == "wrap":
            out.append(Member(layout, w, h, precision, kernel, fast, functools.partial(_wrap, w, h, rest[1])))
        else:
            out.append(_gate(layout, w, h, precision, rest[0], rest[1], kernel, fast, rest[2], ragged, *rest[3:]))
    return out


def _interleave(launches, singles):
    """Round-robin over the launches' member lists, the singles in between: the members of one launch are never neighbours in the list."""
    out, singles = [], list(singles)
    while any(launches):
        for members in launches:
            if members:
                out.append(members.pop(0))
        if singles:
            out.append(singles.pop(0))
    return out + singles


# ------------------------------------------------------------------------------------------------ the lists
@functools.lru_cache(maxsize=None)
def _list8():
    """Seven launches, three or more frames of different sizes each, and two frames one step beyond the int16 sample gate (8190)."""
    launches = [
        # packed 4:2:0: the 16-bit second pass's bound in every component; the packed gate under two different chroma tables
        _launch("420", 8, K8["420p"], 1, [(130, 130, 1476, 1476, 101), (129, 127, 16383, 2046, 102), (144, 272, "photo", 50, 103), (391, 377, 16383, 2046, 104, 1)]),
        # FAST 4:2:0: chroma at and beyond the packed gate
        _launch("420", 8, K8["420"], 1, [(144, 272, 16383, 2047, 111), (257, 17, 16383, 8189, 112), (7, 5, 16383, 2047, 113, 1), (130, 130, 16383, 8189, 114)]),
        # SAFE 4:2:0: one step beyond the FAST gate, and wrap-around content
        _launch("420", 8, K8["420"], 0, [(129, 127, 16384, 2046, 121), (144, 272, "wrap", 122), (16, 16, "wrap", 123), (391, 377, 16384, 2046, 124, 1)]),
        # packed 4:2:2
        _launch("422", 8, K8["422"], 1, [(130, 130, 16383, 2046, 131), (257, 17, 16383, 2046, 132, 1), (391, 377, "photo", 85, 133), (7, 5, 16383, 2046, 134)]),
        # WIDE 4:2:2
        _launch("422", 8, K8["422w"], 1, [(129, 127, 16383, 2047, 141), (144, 272, 16383, 8189, 142), (391, 377, 16383, 2047, 143, 1), (16, 16, 16383, 8189, 144)]),
        # 4:4:4
        _launch("444", 8, K8["444"], 1, [(130, 130, 16383, 8189, 151), (257, 17, 16383, 8189, 152), (129, 127, "photo", 95, 153), (16, 16, 16383, 8189, 154)]),
        # grey (its gate is 8190: 8189 is the last budget of fused1_kernel)
        _launch("grey", 8, K8["grey"], 1, [(129, 127, 8189, None, 161), (144, 272, 8189, None, 162), (391, 377, "photo", 50, 163), (16, 16, 8189, None, 164)]),
    ]
    singles = _launch("422", 8, PAIR, 1, [(16, 16, 16383, 8190, 171)], ragged=False) + _launch("444", 8, PAIR, 1, [(7, 5, 16383, 8190, 172)], ragged=False)
    return _interleave(launches, singles)


@functools.lru_cache(maxsize=None)
def _list12():
    """Two launches per colour group -- the colour stage's one-sum flavour (narrow12) and the other --, one for grey, and one frame one
    step beyond the luma gate (49152)."""
    sizes = {"420": [(130, 130), (129, 127), (144, 272), (257, 17), (391, 377), (16, 16)],
             "422": [(129, 127), (144, 272), (257, 17), (7, 5), (130, 130), (391, 377)],
             "444": [(257, 17), (130, 130), (16, 16), (129, 127), (144, 272), (7, 5)]}
    launches = []
    for li, layout in enumerate(("420", "422", "444")):
        s, seed = sizes[layout], 200 + 10 * li
        narrow = [s[0] + (16000, N12[16000], seed), s[1] + (32000, N12[32000], seed + 1), s[2] + ("photo", 85, seed + 2)]
        other = [s[3] + (49151, 45055, seed + 3), s[4] + (16000, N12[16000] + 1, seed + 4), s[5] + (32000, N12[32000] + 1, seed + 5)]
        launches += [_launch(layout, 12, K12[layout] + "/narrow", 0, narrow), _launch(layout, 12, K12[layout], 0, other)]
    launches.append(_launch("grey", 12, K12["grey"], 0, [(129, 127, 49151, None, 231), (144, 272, 49151, None, 232), (130, 130, "photo", 85, 233)]))
    return _interleave(launches, _launch("420", 12, PAIR, 0, [(16, 16, 49152, 45055, 241)], ragged=False))


RING_SHAPES = [(384, 384), (391, 377), (130, 130), (144, 144)]


def _ring_tables(i):
    """FLAT_Q-like deltas of frame i's own: DC 1..3, one of the first three AC terms 2, every other term 1 -- the luma and the chroma table
    differ, and so do the tables of neighbouring frames.  (Terms 7, 56 and 63 stay 1: own_dc_and_highest_frequency puts up to 400 on
    each, and chroma stays below the packed gate.)"""
    def tab(j):
        q = [1 + j % 3] + [1] * 63
        q[1 + (j // 3) % 3] = 2
        return q
    return [tab(i), tab(i + 4)]


@functools.lru_cache(maxsize=None)
def _ring(w, h, content, i):
    f = _layout("420", w, h, 8, _ring_tables(i))
    rng = np.random.default_rng(500 + i)
    planes = [(CONTENTS[content] if c else _luma)(rng, f.blocks_h[c], f.blocks_w[c]).reshape(f.blocks_h[c], f.blocks_w[c], 64) for c in range(3)]
    return _code(f, planes, 1 + i % 7), planes


@functools.lru_cache(maxsize=None)
def _list_ring():
    """Every content of test_fused420p_ring.CONTENTS on every shape, shapes and contents both changing from one frame to the next: the
    interior and ring waves of neighbouring workgroups belong to different frames with different densities and tables."""
    out = []
    names = list(CONTENTS)
    for i in range(len(names) * len(RING_SHAPES)):
        w, h = RING_SHAPES[i % len(RING_SHAPES)]
        content = names[(i + i // len(RING_SHAPES)) % len(names)]
        out.append(Member("420", w, h, 8, K8["420p"], 1, functools.partial(_ring, w, h, content, i)))
        out[-1].content = content
    return out


# launch geometry: per layout and frame count m, how many of the m pictures have 3 x 2 tiles (300 x 200) and 2 x 1 tiles (200 x 100);
# the others have one tile.  Grid = m + 5 b + t.  No m of the list gives 64 = m + 5 b or 11, so two lists hold 2 x 1-tile pictures as well.
SWEEP = {"grey": {1: (0, 0), 2: (0, 0), 3: (0, 0), 4: (0, 0), 5: (1, 0), 7: (1, 0), 8: (0, 0), 9: (1, 0), 15: (0, 0), 16: (0, 0), 17: (0, 0), 33: (6, 0)},
         "420": {1: (1, 0), 2: (1, 0), 3: (1, 0), 4: (1, 0), 5: (0, 0), 7: (0, 4), 8: (1, 0), 9: (0, 0), 15: (10, 0), 16: (2, 0), 17: (9, 2), 33: (6, 0)}}
SWEEP_GRIDS = {"grey": {1: 1, 2: 2, 3: 3, 4: 4, 5: 10, 7: 12, 8: 8, 9: 14, 15: 15, 16: 16, 17: 17, 33: 63},
               "420": {1: 6, 2: 7, 3: 8, 4: 9, 5: 5, 7: 11, 8: 13, 9: 9, 15: 65, 16: 26, 17: 64, 33: 63}}
SMALL = [(8, 8), (128, 128), (16, 16), (127, 65), (33, 120), (64, 64), (100, 9), (128, 1), (1, 128), (72, 56), (120, 128)]


def _sweep_list(layout, m):
    """m pictures, the k-th of a kind the same picture in every list (seed and quality of its own): the multi-tile ones at positions that
    a permutation seeded with m chooses, so they move from list to list."""
    b, t = SWEEP[layout][m]
    kinds = ["b"] * b + ["t"] * t + ["s"] * (m - b - t)
    kinds = [kinds[j] for j in np.random.default_rng(m).permutation(m)]
    count = {"b": 0, "t": 0, "s": 0}
    out = []
    for kind in kinds:
        k = count[kind]
        count[kind] += 1
        w, h = {"b": (300, 200), "t": (200, 100), "s": SMALL[k % len(SMALL)]}[kind]
        seed, quality = 3000 + 100 * "bts".index(kind) + k, 50 + (7 * k + 13 * "bts".index(kind)) % 49
        out.append(Member(layout, w, h, 8, K8["420p" if layout == "420" else "grey"], 1, functools.partial(_photo, layout, w, h, seed, quality, 1 + seed % 7)))
    return out


# ------------------------------------------------------------------------------------------------ CPU: the premises
def _host_info(member):
    """-> (the host decoder's description of the stream, its coefficient planes)"""
    d = api.Decoder(None)
    f = d.read(member.stream)
    planes = [d.coefficients(c) for c in range(f.components)] if member.planes is not None else None
    d.close()
    return f, planes


def _check_members(members, with_12bit):
    infos = []
    for mb in members:
        f, coef = _host_info(mb)
        assert (f.width, f.height, f.precision, f.components) == (mb.w, mb.h, mb.precision, len(LAYOUTS[mb.layout][0])), mb
        if mb.budgets is not None:
            want = [mb.budgets[0]] + [mb.budgets[1]] * (f.components - 1)
            assert list(f.range_max[:f.components]) == want, (mb, list(f.range_max))
        assert _flavour(f) == (mb.kernel, mb.fast), (mb, _flavour(f), list(f.range_max))
        if coef is not None:  # the blocks that cover samples (the coder repeats the DC predictor in the MCU padding blocks: their sums are no larger)
            for c, p in enumerate(mb.planes):
                nby, nbx = ((mb.h + f.suby[c] - 1) // f.suby[c] + 7) // 8, ((mb.w + f.subx[c] - 1) // f.subx[c] + 7) // 8
                assert np.array_equal(coef[c][:nby, :nbx], p[:nby, :nbx]), (mb, c)
        assert 1 <= f.restart_interval <= 7, mb
        infos.append(f)
    group, _, grids, _ = (api.ragged_plan16 if with_12bit else api.ragged_plan)(infos)
    names = api.RAGGED_GROUPS16 if with_12bit else api.RAGGED_GROUPS
    assert [names[g] if g >= 0 else None for g in group] == [mb.group for mb in members]
    return infos, grids


def _check_launches(members, launches, singles):
    """The list selects `launches` ragged launches and `singles` launches of their own; -> {flavour: sizes of its frames}"""
    ragged = {}
    for mb in members:
        if mb.ragged:
            ragged.setdefault(mb.flavour, []).append((mb.w, mb.h))
    assert len(ragged) == launches and sum(not mb.ragged for mb in members) == singles
    assert not {mb.flavour for mb in members if not mb.ragged} & set(ragged)
    return ragged


def test_the_crafted_lists_are_what_they_claim():
    # the gates' factorizations stay inside the coder's categories
    for budget, pairs in SPLIT.items():
        for d, units in pairs:
            assert d * units == budget and ((d <= 255 and units <= 1023) if budget in GATES8 else (d <= 2047 and units <= 16383)), budget
    assert N12 == {16000: 23168, 32000: 14139}
    # 8 bit: the table of the issue, to the unit
    members = _list8()
    assert len(members) == 30
    _check_members(members, False)
    ragged = _check_launches(members, 7, 2)
    for sizes in ragged.values():
        assert len(sizes) >= 3 and len(set(sizes)) == len(sizes), ragged
    assert set(ragged) == {("420", K8["420p"], 1), ("420", K8["420"], 1), ("420", K8["420"], 0), ("422", K8["422"], 1), ("422", K8["422w"], 1), ("444", K8["444"], 1),
                           ("grey", K8["grey"], 1)}
    budgets = {(mb.layout,) + mb.budgets + (mb.kernel, mb.fast) for mb in members if mb.budgets}
    assert budgets == {("420", 1476, 1476, K8["420p"], 1), ("420", 16383, 2046, K8["420p"], 1), ("420", 16383, 2047, K8["420"], 1), ("420", 16383, 8189, K8["420"], 1),
                       ("420", 16384, 2046, K8["420"], 0), ("422", 16383, 2046, K8["422"], 1), ("422", 16383, 2047, K8["422w"], 1), ("422", 16383, 8189, K8["422w"], 1),
                       ("422", 16383, 8190, PAIR, 1), ("444", 16383, 8189, K8["444"], 1), ("444", 16383, 8190, PAIR, 1), ("grey", 8189, None, K8["grey"], 1)}
    # the frames of the packed 4:2:0 and 4:2:2 launches bring both factorizations of 2046, the SAFE launch two frames of wrap-around content
    for layout, kernel in (("420", K8["420p"]), ("422", K8["422"])):
        at_2046 = [mb for mb in members if mb.layout == layout and mb.kernel == kernel and mb.budgets == (16383, 2046)]
        assert {tuple(mb.make.args[4:8]) for mb in at_2046} == {(43, 381, 2, 1023), (43, 381, 6, 341)}  # (luma delta, units, chroma delta, units)
    wraps = [mb for mb in members if mb.budgets is None and mb.fast == 0]
    assert len(wraps) == 2 and wraps[0].make.args != wraps[1].make.args and all(max(_host_info(mb)[0].range_max[:3]) >= 16384 for mb in wraps)
    # 12 bit
    members = _list12()
    assert len(members) == 22
    _check_members(members, True)
    ragged = _check_launches(members, 7, 1)
    for sizes in ragged.values():
        assert len(sizes) >= 2 and len(set(sizes)) == len(sizes), ragged
    assert set(ragged) == {(layout + "_12", K12[layout] + suffix, 0) for layout in ("420", "422", "444") for suffix in ("", "/narrow")} | {("grey_12", K12["grey"], 0)}
    budgets = {(mb.layout,) + mb.budgets + (mb.kernel,) for mb in members if mb.budgets}
    want = {("grey", 49151, None, K12["grey"]), ("420", 49152, 45055, PAIR)}
    for layout in ("420", "422", "444"):
        want |= {(layout, 49151, 45055, K12[layout]), (layout, 16000, 23168, K12[layout] + "/narrow"), (layout, 16000, 23169, K12[layout]),
                 (layout, 32000, 14139, K12[layout] + "/narrow"), (layout, 32000, 14140, K12[layout])}
    assert budgets == want
    # the ring list: one launch of the packed 4:2:0 kernel, every content on every shape, no two neighbours with the same tables
    members = _list_ring()
    infos, _ = _check_members(members, False)
    assert {mb.flavour for mb in members} == {("420", K8["420p"], 1)}
    assert {(mb.w, mb.h, mb.content) for mb in members} == {(w, h, c) for w, h in RING_SHAPES for c in CONTENTS}
    tables = [[list(f.quant[f.quant_index[c]]) for c in (0, 1)] for f in infos]
    assert all(a != b for a, b in zip(tables, tables[1:])) and all(t[0] != t[1] for t in tables)
    # the sweep: every frame count for both layouts, one launch each, the planner's grids
    grids_seen = set()
    for layout in ("grey", "420"):
        assert sorted(SWEEP[layout]) == [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33]
        for m in SWEEP[layout]:
            members = _sweep_list(layout, m)
            assert len(members) == m and len({mb.make.args for mb in members}) == m
            infos, grids = _check_members(members, False)
            assert {mb.flavour for mb in members} == {(layout, K8["420p" if layout == "420" else "grey"], 1)}
            grid = grids[api.RAGGED_GROUPS.index(layout)]
            assert grid == SWEEP_GRIDS[layout][m] == sum(((mb.w + 127) // 128) * ((mb.h + 127) // 128) for mb in members) and sum(grids) == grid
            grids_seen.add(grid)
    assert grids_seen >= set(range(1, 18)) | {63, 64, 65}


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def _expected(oracle, stream, precision):
    out = oracle.decode16(stream) if precision == 12 else oracle.decode(stream)
    out.setflags(write=False)
    return out


def _run_list(d, oracle, members, with_12bit, launches, singles, entropy_launches):
    """One decode call and one reconstruct call for the whole list; every picture against the oracle's, every byte outside the pictures
    untouched, and the statistics: all members in their groups, `launches` ragged launches -- the number of distinct (group, _flavour)
    values among the members that have a ragged flavour --, `singles` launches of their own."""
    n = len(members)
    streams = [mb.stream for mb in members]
    exp = [_expected(oracle, mb.stream, mb.precision) for mb in members]
    assert d.decode_ragged_device(streams, with_12bit=with_12bit) == [0] * n
    infos = [d.ragged_info(i) for i in range(n)]
    assert [d.ragged_route(i) for i in range(n)] == [(True, None)] * n
    for f, mb in zip(infos, members):  # the device's range check agrees with the host's, which the CPU test pinned
        assert (f.width, f.height, f.precision) == (mb.w, mb.h, mb.precision) and _flavour(f) == (mb.kernel, mb.fast), (mb, _flavour(f), list(f.range_max))
        if mb.budgets is not None:
            assert list(f.range_max[:f.components]) == [mb.budgets[0]] + [mb.budgets[1]] * (f.components - 1), (mb, list(f.range_max))
    pics, touched = _reconstruct_guarded(d, infos, PADS12 if with_12bit else PADS8)
    st = d.ragged_stats()
    bad = [mb for mb, pic, e in zip(members, pics, exp) if pic.shape != e.shape or pic.dtype.itemsize != e.dtype.itemsize or not np.array_equal(pic, e)]
    assert not bad, bad
    assert not any(touched), [mb for mb, t in zip(members, touched) if t]
    flavours = {(mb.group,) + _flavour(f) for f, mb in zip(infos, members) if mb.ragged}
    assert len(flavours) == launches
    assert st["images"] == n and st["ragged"] == n and st["fallbacks"] == 0 and st["errors"] == 0, st
    assert st["recon_launches"] == launches and st["recon_single"] == singles and st["entropy_launches"] == entropy_launches and st["walk_launches"] == 0, st


@pytest.mark.gpu
def test_every_8bit_flavour_at_its_gates(oracle):
    """Packed, FAST and SAFE 4:2:0, packed and WIDE 4:2:2, 4:4:4 and grey in one list, every launch with three crafted frames of different
    sizes right at its gates (1476; 2046 / 2047; 8189; 16383 / 16384) and, where ordinary pictures select the flavour, one of those in
    between; 4:2:2 and 4:4:4 frames at 8190 come back exact through launches of their own."""
    d = api.Decoder(0)
    _run_list(d, oracle, _list8(), False, 7, 2, 4)
    d.close()


@pytest.mark.gpu
def test_every_12bit_flavour_at_its_gates(oracle):
    """49151 / 45055 and the colour stage's one-sum bound (narrow12, at the bound and one step beyond for luma 16000 and 32000) in the
    three colour groups, 49151 in the grey one, an ordinary 12-bit picture in every narrow launch; 49152 takes a launch of its own."""
    d = api.Decoder(0)
    _run_list(d, oracle, _list12(), True, 7, 1, 4)
    d.close()


@pytest.mark.gpu
def test_ring_tiers_through_the_ragged_packed_kernel(oracle):
    """The contents of test_fused420p_ring (4 x 4 corner, rows 0..3, dense, ring and interior of different density, highest frequencies)
    on 384 x 384, 391 x 377, 130 x 130 and 144 x 144, each frame under tables of its own, all in one launch of fused420p_kernel's ragged
    flavour -- which takes per-frame tables and never the 16-bit second pass, unlike the instantiation the uniform ring tests run."""
    d = api.Decoder(0)
    _run_list(d, oracle, _list_ring(), False, 1, 0, 1)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["grey", "420"])
def test_launch_geometry_sweep(dec, oracle, layout):
    """tile_enter_ragged over frame counts 1, 2, 3 and 2^k +- 1 and grids of 1..17 and 63 / 64 / 65 workgroups (no multiple of eight
    among most of them): every picture has a seed and quality of its own, so a workgroup that takes a neighbour's frame, tile or
    table changes pixels.  One decoder object serves all lists."""
    for m in SWEEP[layout]:
        _run_list(dec, oracle, _sweep_list(layout, m), False, 1, 0, 1)

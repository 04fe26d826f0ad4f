"""fused420p_kernel's uniform flavours (one table set per launch) run lean transforms: every v_dot2 product in its three-operand
form, and -- where the second pass consumes packed 16-bit pairs (the D2 flavour, sum |c| q <= 1476 in all three components) -- a first
pass whose constants are scaled by 8 so that its rounded result is bytes 1..2 of the sum and no shift is issued.  Every case is
compared byte for byte with the oracle: synthetic coefficient planes through api.launch_reconstruct, as test_fused420p_ring does.

Where the arithmetic is tight.  A first-pass output is (sum_u s_u M_uj + 16) >> 5, with s_u the dequantised coefficients of one
coefficient row and M the butterfly's integer matrix.  Its largest entry, 710, belongs to horizontal frequency 1 at output columns 0
(+710) and 7 (-710): a block that spends its whole budget on ONE coefficient of column 1 reaches +-32749 in its row at 1476, the
closest bytes 1..2 of the scaled sum come to the ends of 16 bits.  Under FLAT_Q every AC delta is 1, so such a block is the single
coefficient +-budget at (v, 1).  Which row v carries it decides the tier the wave takes (wave-uniform, any block of the wave):
v < 4 with nothing in columns 4..7 the 4 x 4 tier (butterfly first pass, lean second pass), v < 4 beside a block with a term in
columns 4..7 the 4 x 8 tier, any v >= 4 the 8 x 8 tier -- the last two run the scaled first pass.

Shapes: 128 x 128 one tile; 144 x 136 2 x 2 tiles with partial right and bottom ones; 384 x 384 3 x 3 tiles, the centre one with
all eight neighbours (its ring blocks are real blocks of the picture)."""
import numpy as np
import pytest

from libjpeg_amd import api
from test_fused420p_ring import CONTENTS, FLAT_Q, _at_budget, _blocks, _check, _corner4x4, _dense, _frame, _launch, _range_max, _rows03, _store

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128), (144, 136), (384, 384)]
GATE_D2 = 1476  # the largest sum |c| q the 16-bit second pass is admitted for (reconstruct.hpp: GATE_DOT2 - 1)


def _on_the_largest_entry(budget, rows, spread=0.0, tail=0.0):
    """-> generator of blocks with sum |c| q == budget under FLAT_Q.  Most blocks: the single coefficient +-budget at (v, 1), v drawn
    from `rows`.  A share `spread` of them: all 64 coefficients set as CONTENTS' dense blocks have them (the rows restricted to
    `rows`' half when that is 0..3), the rest of the budget on (v, 1) in that term's sign.  A share `tail`: +-1 at (0, 7), the rest
    at (v, 1) -- a term in columns 4..7 that lifts a wave of rows 0..3 from the 4 x 4 to the 4 x 8 tier."""
    def make(rng, bh, bw):
        p = np.zeros((bh, bw, 8, 8), np.int64)
        kind = rng.random((bh, bw))
        v = rng.choice(rows, size=(bh, bw))
        sign = rng.choice([-1, 1], size=(bh, bw))
        dense = _dense(rng, bh, bw).astype(np.int64)
        if max(rows) < 4:
            dense[:, :, 4:, :] = 0
        q = np.array(FLAT_Q, np.int64).reshape(8, 8)
        for by in range(bh):
            for bx in range(bw):
                b = p[by, bx]
                if kind[by, bx] < spread:
                    b[:] = dense[by, bx]
                    b[v[by, bx], 1] = 0
                elif kind[by, bx] < spread + tail:
                    b[0, 7] = -sign[by, bx]
                b[v[by, bx], 1] = sign[by, bx] * (budget - int((np.abs(b) * q).sum()))
        assert ((np.abs(p) * q).sum(axis=(2, 3)) == budget).all() and (np.abs(p[..., 1]).max(axis=2) > budget - 400).all()
        return p.astype(np.int32)
    return make


def _run(oracle, w, h, gens, seed, declare=None):
    """gens: (luma, Cb, Cr) generators.  declare: range_max as the host would report it -- an upper bound of every block's
    sum |c| q, which is what selects the flavour; None: the planes' own maximum."""
    f, info = _frame(oracle, w, h)
    rng = np.random.default_rng(seed)
    planes = []
    for c in range(3):
        bh, bw = _blocks(info, c)
        planes.append(gens[c](rng, bh, bw).reshape(bh, bw, 64))
    for c in range(3):
        own = _range_max(planes, c, FLAT_Q)
        f.range_max[c] = own if declare is None else declare[c]
        assert own <= f.range_max[c]
    f.fast_arith = 1
    assert api.kernel_name(f) == "fused420p_kernel"
    _check(_launch(f, [_store(planes)], w, h)[0], oracle.reconstruct(info, planes), f"{w}x{h} {list(f.range_max[:3])}")
    return f


ALL_ROWS, LOW_ROWS = list(range(8)), list(range(4))


@pytest.mark.parametrize("rows", [ALL_ROWS, LOW_ROWS], ids=["rows0-7", "rows0-3"])
@pytest.mark.parametrize("luma,chroma", [(1476, 1476), (1477, 1477), (1477, 1476), (1476, 1477)])
@pytest.mark.parametrize("w,h", SHAPES)
def test_budget_on_the_largest_first_pass_entry_at_the_d2_gate(oracle, w, h, luma, chroma, rows):
    """Every block of luma and of both chroma planes (interior and ring blocks alike) spends its budget on (v, 1), both signs: at
    1476 in all three the D2 flavour runs and its first pass reaches +-32749; 1477 in luma or in chroma takes the other flavour,
    whose first pass keeps its shift.  rows0-7: the 8 x 8 tier; rows0-3: the 4 x 4 tier and, where a wave holds a block with its
    unit at (0, 7), the 4 x 8 tier."""
    tail = 0.0 if rows is ALL_ROWS else 0.02
    gens = [_on_the_largest_entry(b, rows, tail=tail) for b in (luma, chroma, chroma)]
    f = _run(oracle, w, h, gens, luma + chroma + w + len(rows))
    assert list(f.range_max[:3]) == [luma, chroma, chroma]


@pytest.mark.parametrize("budget", [1476, 1477])
@pytest.mark.parametrize("w,h", SHAPES)
def test_budget_spread_as_dense_content_at_the_d2_gate(oracle, w, h, budget):
    """All 64 coefficients of a block set, the rest of the budget on the largest entry; beside them blocks with the budget on one
    coefficient anywhere, on the DC term, or scattered over the 63 AC terms (test_fused420p_ring._at_budget)."""
    def mixed(rng, bh, bw):
        a, b = _on_the_largest_entry(budget, ALL_ROWS, spread=1.0)(rng, bh, bw), _at_budget(rng, bh, bw, budget)
        pick = rng.random((bh, bw)) < 0.5
        a[pick] = b[pick]
        return a
    f = _run(oracle, w, h, [mixed] * 3, budget + w)
    assert list(f.range_max[:3]) == [budget] * 3


@pytest.mark.parametrize("chroma", [1476, 2046])
@pytest.mark.parametrize("w,h", SHAPES)
def test_luma_below_the_16_bit_first_pass_bound(oracle, w, h, chroma):
    """Luma at sum |c| q = 16383 on the largest entry (the first pass's own bound: its sums reach 710 * 16383), chroma inside the
    packed gate: the three-operand first pass with its shift, the 32-bit second pass."""
    gens = [_on_the_largest_entry(16383, ALL_ROWS, spread=0.25)] + [_on_the_largest_entry(chroma, ALL_ROWS, spread=0.25)] * 2
    f = _run(oracle, w, h, gens, 16383 + chroma + w)
    assert list(f.range_max[:3]) == [16383, chroma, chroma]


TIERS = {"4x4": _corner4x4, "4x8": _rows03, "8x8": _dense}


@pytest.mark.parametrize("d2", [True, False], ids=["d2", "32bit"])
@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("w,h", [(144, 136), (384, 384)])
def test_every_tier_in_both_flavours(oracle, w, h, tier, d2):
    """One frame per tier, all three components of that tier's content (every wave of the launch takes it), in the D2 flavour and --
    the same planes declared one unit beyond its gate -- in the other."""
    assert CONTENTS["corner4x4"] is _corner4x4 and CONTENTS["rows03"] is _rows03 and CONTENTS["dense"] is _dense
    gen = TIERS[tier]
    _run(oracle, w, h, [gen] * 3, 50 + w + len(tier), declare=[GATE_D2 if d2 else GATE_D2 + 1] * 3)

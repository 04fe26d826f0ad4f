"""The cases of tests/forward_cases.py, without a GPU: that the corpus reaches the partitions, branches and quantiser ties it claims
(from the partition restatement and the model's pre-quantiser values), that the numpy restatement of the model's inner values is the
model's, that the model is a DCT (against float64), and whether the quantiser's (n > 0) term can be observed at all."""
import numpy as np
import pytest

import forward_cases as F


def _dct_matrix():
    k, i = np.mgrid[0:8, 0:8].astype(np.float64)
    m = np.cos((2 * i + 1) * k * np.pi / 16) * np.sqrt(2 / 8)
    m[0] = np.sqrt(1 / 8)
    return m


@pytest.mark.parametrize("precision", F.PRECISIONS)
def test_inner_values_are_the_models(precision):
    """block_samples -> pre_quantiser -> quantise is a third statement of the transform; the tests only use it to find and count ties
    and to feed the float64 comparison.  It gives the model's coefficients for every shape and content under the `random` and `pow2`
    tables (the blocks that cover samples; the model leaves the others zero)."""
    for w, h, layout in F.SHAPES:
        geo = F.geometry(w, h, layout)
        for i, content in enumerate(F.CONTENTS):
            table = ("random", "pow2")[(i + w) % 2] if content != "ties" else "pow2"
            img, planes = F.case(w, h, layout, precision, content, table)
            q = F.tables(table, len(geo))
            samples = F.block_samples(img, layout, precision)
            for c, (_, _, bw, bh, nbx, nby) in enumerate(geo):
                assert planes[c].shape == (bh, bw, 64) and samples[c].shape == (nby * 8, nbx * 8)
                mine = F.quantise(F.pre_quantiser(samples[c], precision), q[c].astype(np.int64))
                assert np.array_equal(mine, planes[c][:nby, :nbx]), (w, h, layout, content, c)
                pad = planes[c].copy()
                pad[:nby, :nbx] = 0
                assert not pad.any()


def _classes(**route):
    """{(w, h, layout): per component the set of owners that occur}"""
    return {s: [set(np.unique(o).tolist()) for o in F.owners(*s, **route)] for s in F.SHAPES}


def test_corpus_reaches_what_it_claims():
    # ---- the partitions.  forward_args_of's rule does not look at the sample size and every shape runs at both precisions, so
    # what holds for the corpus holds at 8 and at 12 bits
    assert F.PRECISIONS == (8, 12)
    occur = _classes()
    seen = set()
    for (w, h, layout), comps in occur.items():
        for c, owners in enumerate(comps):
            seen |= {(o, F.interior_kernel(layout, c)) if o == F.INTERIOR else (o,) for o in owners}
    assert seen >= {(F.TILE,), (F.EDGE,), (F.PAD,)} | {(F.INTERIOR, k) for k in ((1, 1), (2, 1), (1, 2), (2, 2))}, seen
    # 4:2:0: tile, interior and edge blocks all occur in one component -- 255 x 257: in every component; 144 x 136: in the chroma
    # components (its luma has whole blocks only)
    three = {s: [{F.TILE, F.INTERIOR, F.EDGE} <= o for o in comps] for s, comps in occur.items() if s[2] == "420"}
    assert three[(255, 257, "420")] == [True] * 3 and three[(144, 136, "420")] == [False, True, True], three
    assert occur[(144, 136, "420")][0] == {F.TILE, F.INTERIOR, F.PAD}  # (136 lines: 17 block rows, 9 MCU rows)
    # ... one of tiles alone (every other launch finds nothing to do), one of tiles and edges without interior blocks
    assert occur[(128, 128, "420")] == [{F.TILE}] * 3
    assert occur[(129, 129, "420")] == [{F.TILE, F.EDGE, F.PAD}, {F.TILE, F.EDGE}, {F.TILE, F.EDGE}]
    assert all(F.TILE not in o for s in F.NO_TILES_420 for o in occur[s + ("420",)])
    # every interior kernel with zero, one and several interior blocks, with edge columns and with edge rows
    for kernel in ((1, 1), (2, 1), (1, 2), (2, 2)):
        counts, edge_cols, edge_rows = set(), False, False
        for w, h, layout in F.SHAPES:
            fast = F.fast_components(layout)
            for c, own in enumerate(F.owners(w, h, layout)):
                if not fast[c] or F.interior_kernel(layout, c) != kernel:
                    continue
                n = int((own == F.INTERIOR).sum())
                counts.add(min(n, 2))
                edge_cols |= n > 0 and bool((own[0] == F.EDGE).any())
                edge_rows |= n > 0 and bool((own[:, 0] == F.EDGE).any())
        assert counts == {0, 1, 2} and edge_cols and edge_rows, (kernel, counts, edge_cols, edge_rows)
    # for each of these layouts a width that is a multiple of 4 and one that is not
    for layout in ("444", "422", "440", "420"):
        assert {w % 4 == 0 for w, _, lay in F.SHAPES if lay == layout} == {True, False}
    # off the dword route, under MIJPEG_FORWARD_SLOW, without the transformation and for grey nothing is fast; without tiles no tile
    for s in F.SHAPES:
        for route in (dict(dword=False), dict(slow=True)):
            assert all(F.TILE not in np.unique(o) and F.INTERIOR not in np.unique(o) for o in F.owners(*s, **route))
        assert all(F.TILE not in np.unique(o) for o in F.owners(*s, no_tiles=True))
        if s[2] in ("grey", "rgb"):
            assert not any(F.fast_components(s[2]))
    # ---- the sub-block cases: the mirror's clamp to 0, block rows without a line
    clamp = [(w, h, lay) for w, h, lay in F.SHAPES if any(F.mirror_clamps(w, sx) for sx, *_ in F.geometry(w, h, lay))]
    bare = [(w, h, lay) for w, h, lay in F.SHAPES if any(F.rows_without_lines(h, g[1]) for g in F.geometry(w, h, lay))]
    for lay in ("411", "3x3", "4x2", "mixed"):
        assert {(w, h) for w, h, l in clamp if l == lay} >= {(1, 1), (2, 3), (3, 2), (5, 1)}, (lay, clamp)
    for lay in ("3x3", "4x2", "mixed"):
        assert {(w, h) for w, h, l in bare if l == lay} >= {(1, 1), (5, 1), (7, 2), (9, 5)}, (lay, bare)
    # (the restated predicates against the model's own samples: where the clamp is reached the last column repeats sample 0's share,
    # and a row without lines is zero)
    img = F.picture(1, 1, "3x3", 8, "noise")
    s = F.block_samples(img, "3x3", 8)[1]
    assert s.shape == (8, 8) and (s[0] == s[0, 0]).all() and s[0, 0] > 0 and not s[1:].any()
    # ---- the ties pictures hold exact halves of both signs, at DC and at AC, under the tables they were made for
    for precision in F.PRECISIONS:
        total = np.zeros(4, np.int64)
        for w, h, layout in F.SHAPES:
            img = F.picture(w, h, layout, precision, "ties")
            t = F.count_ties(img, layout, precision, F.tables("pow2", F.components_of(layout)))
            total += t
            if w >= 16 and h >= 16:  # four whole blocks or more: one of each kind at least
                assert min(t) >= 1, (w, h, layout, precision, t)
        assert min(total) >= 100, total
        # the halves round towards +infinity whatever the sign: what the model gives for them
        img, planes = F.case(70, 50, "grey", precision, "ties", "pow2")
        n = F.pre_quantiser(F.block_samples(img, "grey", precision)[0], precision)
        tie = F.is_tie(n, F.tables("pow2", 1)[0])
        exact = n.astype(np.float64) * F.invq(F.tables("pow2", 1)[0]) / float(1 << 46)
        nby, nbx = tie.shape[:2]
        assert tie.any() and np.array_equal(planes[0][:nby, :nbx][tie], np.floor(exact[tie] + 0.5).astype(np.int32))
        assert (np.abs(exact[tie] - np.floor(exact[tie]) - 0.5) == 0).all()


MEASURED = {8: 0.916258, 12: 11.076625}  # what test_the_model_is_a_dct printed when it was written


@pytest.mark.parametrize("precision", F.PRECISIONS)
def test_the_model_is_a_dct(precision):
    """Two integer transforms that agree with each other need not be a DCT: the model's coefficients under all-ones tables against
    the orthonormal float64 DCT-II of the level-shifted samples the model itself feeds its transform (block_samples / 16 - 2^(P-1)).
    The integer transform's output is 8 x the orthonormal one with 13 fractional bits; the quantiser's shift by 46 = 30 + 13 + 3 takes
    both out, so under a delta of 1 the coefficient is the rounded DCT and the comparison is made in coefficient units.
    Measured over every shape and content of the corpus, largest |coefficient - DCT|: 0.916258 at 8 bits, 11.076625 at 12 bits (half
    a step of rounding plus the error of a transform whose constants have 9 fractional bits: about 7e-4 of the largest coefficient,
    1020 and 16380, which the saturated checkerboards reach).  Asserted: the measured maximum plus one quantisation step (1.0).  A
    transposed, swapped or mis-signed term of the transform is off by hundreds."""
    m = _dct_matrix()
    worst = 0.0
    for w, h, layout in F.SHAPES:
        geo = F.geometry(w, h, layout)
        for content in F.CONTENTS:
            img, planes = F.case(w, h, layout, precision, content, "ones")
            samples = F.block_samples(img, layout, precision)
            for c, (_, _, _, _, nbx, nby) in enumerate(geo):
                x = samples[c].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3) / 16.0 - (1 << (precision - 1))
                d = np.einsum("ki,abij,lj->abkl", m, x, m).reshape(nby, nbx, 64)
                worst = max(worst, float(np.abs(planes[c][:nby, :nbx] - d).max()))
    print(f"precision {precision}: largest |model - float64 DCT| = {worst:.6f}")
    assert worst <= MEASURED[precision] + 1.0, worst


def test_whether_the_positive_term_of_the_quantiser_can_be_observed():
    """(n * q + (n > 0) + 2^45) >> 46: the (n > 0) term changes the result only where n > 0 and n * q + 2^45 = -1 (mod 2^46).  Then q is
    odd, n is odd and n is one residue modulo 2^46 per q.  n is odd only at the positions whose row-pass output is not shifted left by
    9, columns 1, 2, 3, 5, 6, 7; there |coefficient| <= 2^(P-1) * sum|basis| <= 2^(P-1) * 2.83 * 2.57 < 0.91 * 8 * 2^(P-1), so with its 16
    fractional bits n < 0.91 * 2^30 at 12 bits (0.91 * 2^26 at 8), a margin a hundred times the transform's error.  Over ALL 16-bit
    deltas the solutions are listed below: none has n below 2^30.  So no input at either precision can observe the term, no case of the
    corpus does, and a kernel without it passes these tests -- as it computes the same function."""
    mod = 1 << 46
    hits = []
    for delta in range(1, 65536):
        q = int(F.invq(np.array([delta]))[0])
        if q % 2 == 0:
            continue
        n = (((1 << 45) - 1) * pow(q, -1, mod)) % mod
        assert (n * q + (1 << 45)) >> 46 != (n * q + 1 + (1 << 45)) >> 46
        if n < (1 << 32):
            hits.append((delta, n))
    print("deltas at which (n > 0) is observable below 2^32, with the one n:", hits)
    assert hits and all(n >= (1 << 30) for _, n in hits), hits

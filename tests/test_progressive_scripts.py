"""huffman_prog_kernel's refinement pass (prog_block_refine: two 32-bit history masks split at scan position 32, the list of
free positions, correction bits taken in one piece from the 32-bit window or past it, their 64-bit string and the rank of a
coefficient in the history, EOB runs that carry corrections only) and the level schedule of device_entropy_multiscan
(plan_multiscan in entropy_plan.hpp, whose levels, slots and lanes tests/test_entropy_plan_cpu.py asserts directly), on scan
scripts and coefficient histories made for them (huffcraft.scripts, huffcraft.history_content): bands that end and start at the
split of the masks, one-coefficient bands, three refinement levels over 1..63, DC with Al = 3, DC scans of one component, scans of
different components and kinds in one launch, frames that are not whole MCUs.

As in test_huffman_tables.py every stream is checked before a decoder sees it: the oracle decodes exactly the planes the writer
was given and the reference binary (where built) the oracle's pixels.  The host decoder and, with -m gpu, the device must
return those planes; the expected values never come from the device.  What the corpus makes the refinement pass do is not left
to chance: the writer's trace says so, and test_history_content_reaches_what_it_claims asserts it."""
import functools

import numpy as np
import pytest

import huffcraft as hc
from libjpeg_amd import api
from test_huffman_tables import LAYOUTS as WHOLE, check_stream, dev, device_matches, oracle_pixels, same_planes  # noqa: F401 (dev: fixture)

S420 = [(2, 2), (1, 1), (1, 1)]
LAYOUTS = {  # whole MCUs, and frames whose non-interleaved scans are narrower and shorter than the planes they write into
    "p420": WHOLE["p420"], "p444": WHOLE["p444"], "pgrey": WHOLE["pgrey"],
    "420_40x24": (40, 24, S420), "420_17x9": (17, 9, S420), "422_23x16": (23, 16, [(2, 1), (1, 1), (1, 1)]),
}
DRIS = (1, 3, 0, 1000)  # 0: one lane decodes the scan and the EOB run lives across all its blocks; 1000: the same behind a DRI marker
FAMILIES = ("annexk", "all_long", "len16_widest", "fixed8")
SCRIPTS = ("deep", "split32", "split33", "single")
PRECISIONS = (8, 12)
LANE_SLOTS = (104, 96)  # grey, 13 x 12 = 156 blocks: with DRI 1 two full waves of lane slots and 28 of a third


@functools.lru_cache(maxsize=None)
def make_case(script, precision, fam, layout, dri, size=None, phase=0):
    """-> (stream, intended planes, the writer's trace); Cb / Cr code with hc.chroma_variant of the family's tables"""
    w, h, samp = LAYOUTS[layout]
    if size:
        w, h = size
    nc = len(samp)
    scans, top_al = hc.scripts(nc)[script]
    dc, ac = hc.family(fam, precision, True)
    key = [precision, SCRIPTS.index(script), FAMILIES.index(fam), list(LAYOUTS).index(layout), dri, w, h]
    rng = np.random.default_rng(key)
    own = hc.own_dc_scans(scans, nc)
    planes = hc.content("history", hc.plane_shapes(w, h, samp), precision, rng, *hc.uses(dc, ac), top_al=top_al,
                        extents=hc.scan_extents(w, h, samp), dc_outside=[not o for o in own], phase=phase)
    quant = [rng.integers(1, 24 if precision == 8 else 200, 64) for _ in samp]
    tables = [(dc, ac)] + [(hc.chroma_variant(dc), hc.chroma_variant(ac))] * (nc - 1)
    trace = hc.Trace()
    data = hc.write(planes, w, h, samp, tables, precision=precision, quant=quant, dri=dri, progressive=True, script=scans, trace=trace)
    for p in planes:
        p.setflags(write=False)
    return data, planes, trace


def corpus(script, precision):
    """The streams of one script and precision: every layout at every restart interval, the family moving on with each (the
    full product with the families is four times the work for the same scans), so that every family meets every layout and
    every restart interval; the content's phase moves on with every stream of a family, so that the patterns which count
    something up (history_content) get through their range within each family.  -> [(fam, layout, dri, None, phase)]"""
    s = SCRIPTS.index(script)
    out, of_family = [], dict.fromkeys(FAMILIES, 0)
    for li, layout in enumerate(LAYOUTS):
        for di, dri in enumerate(DRIS):
            fam = FAMILIES[(li + di + s) % len(FAMILIES)]
            out.append((fam, layout, dri, None, 3 * of_family[fam] + s))
            of_family[fam] += 1
    return out


def lane_slot_cases(script):
    return [(script, precision, fam, "pgrey", 1, LANE_SLOTS) for precision, fam in ((8, "annexk"), (12, "all_long"), (8, "fixed8"), (12, "len16_widest"))]  # (phase 0)


def side_by_side_cases():
    return [("split33", precision, fam, "p420", dri) for precision in PRECISIONS for fam, dri in zip(FAMILIES, DRIS)]


def gpu_corpus():
    """Every stream a GPU test of this file decodes (arguments of make_case)."""
    out = [(script, precision) + c for script in SCRIPTS for precision in PRECISIONS for c in corpus(script, precision)]
    return out + [c for script in ("deep", "split32") for c in lane_slot_cases(script)] + side_by_side_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the scripts, the writer against the oracle and the reference, the host decoder, and what the corpus reaches
# ---------------------------------------------------------------------------------------------------------------------------
def test_corpus_meets_every_layout_and_restart_interval():
    for script in SCRIPTS:
        for precision in PRECISIONS:
            cases = corpus(script, precision)
            assert {(layout, dri) for _, layout, dri, _, _ in cases} == {(layout, dri) for layout in LAYOUTS for dri in DRIS}
            assert {c[0] for c in cases} == set(FAMILIES)
    for nc in (1, 3):
        assert set(hc.scripts(nc)) == set(SCRIPTS)
    for layout, (w, h, samp) in LAYOUTS.items():  # the last three really are what they are here for
        smaller = [e != s for e, s in zip(hc.scan_extents(w, h, samp), hc.plane_shapes(w, h, samp))]
        assert any(smaller) == (layout[0] != "p"), layout


def test_writer_refuses_coefficients_outside_a_components_own_blocks():
    w, h, samp = LAYOUTS["420_17x9"]
    dc, ac = hc.family("annexk", 8, True)
    for k, comp in ((1, 0), (63, 0), (1, 1)):
        planes = [np.zeros(s + (64,), np.int32) for s in hc.plane_shapes(w, h, samp)]
        ext = hc.scan_extents(w, h, samp)[comp]
        if ext == planes[comp].shape[:2]:
            continue
        planes[comp][-1, -1, hc.ZZ[k]] = 5
        with pytest.raises(AssertionError, match="own blocks"):
            hc.write(planes, w, h, samp, [(dc, ac)] * 3, progressive=True)
    planes = [np.zeros(s + (64,), np.int32) for s in hc.plane_shapes(w, h, samp)]
    planes[0][-1, -1, 0] = 5  # a DC value there travels in the interleaved DC scan ...
    hc.write(planes, w, h, samp, [(dc, ac)] * 3, progressive=True)
    with pytest.raises(AssertionError, match="own blocks"):  # ... and not in a DC scan of the component alone
        hc.write(planes, w, h, samp, [(dc, ac)] * 3, progressive=True, script=hc.scripts(3)["split33"][0])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("script", SCRIPTS)
def test_scripts_are_legal_and_streams_carry_their_planes(oracle, script, precision):
    for nc in (1, 3):
        hc.check_script(hc.scripts(nc)[script][0], nc)
    one, eight = api.Decoder(None), api.Decoder(None)
    try:
        for case in corpus(script, precision):
            fam, layout, dri = case[:3]
            data, planes, _ = make_case(script, precision, *case)
            check_stream(oracle, data, planes, precision)
            for d, threads in ((one, 1), (eight, 8)):
                f = d.read(data, threads=threads)
                assert f.progressive == 1 and f.precision == precision
                same_planes(d, planes, f"host decoder, {threads} threads, {script} {fam} {layout} DRI {dri}")
            assert list(one.info.range_max) == list(eight.info.range_max) and one.info.fast_arith == eight.info.fast_arith
    finally:
        one.close()
        eight.close()


def test_lane_slot_and_side_by_side_streams_carry_their_planes(oracle):
    d = api.Decoder(None)
    try:
        for case in [c for script in ("deep", "split32") for c in lane_slot_cases(script)] + side_by_side_cases():
            data, planes, _ = make_case(*case)
            check_stream(oracle, data, planes, case[1])
            d.read(data, threads=4)
            same_planes(d, planes, f"host decoder, {case}")
    finally:
        d.close()


def _events(cases):
    """What the refinement scans of these streams make a decoder do: {event: the families it came from}"""
    seen = {}

    def saw(event, fam):
        seen.setdefault(event, set()).add(fam)

    for case in cases:
        fam = case[2]
        for s in make_case(*case)[2].scans:
            width = s["se"] - s["ss"] + 1
            if s["ss"] == 0:
                if s["ah"] == 0 and s["al"] == 3:
                    saw("DC first pass with Al = 3", fam)
                if len(s["comps"]) == 1 and len(LAYOUTS[case[3]][2]) > 1:
                    saw("DC scan of one component (first pass)" if s["ah"] == 0 else "DC scan of one component (refinement)", fam)
                continue
            for edge in ("se", "ss"):
                saw(f"band with {edge} = {s[edge]}", fam)
            if s["ss"] == s["se"]:
                saw(f"band {s['ss']}..{s['se']}", fam)
            if s["ah"] == 0:
                continue
            for bits in s["symbols"]:
                saw(f"coefficient with tot + ncorr = {bits}" if bits < 48 else "coefficient with tot + ncorr >= 48", fam)
            for tot, ncorr in s["zrl"]:
                if tot + ncorr > 32:
                    saw("ZRL with tot + ncorr > 32", fam)
                if 1 <= ncorr <= 16:
                    saw("ZRL with 1..16 corrections", fam)
                    saw(f"ZRL with {ncorr} corrections", fam)
            for ncorr in s["trailing"]:
                if ncorr == width:
                    saw(f"trailing corrections fill a band of {width}", fam)
            for blocks, ncorr, empty_behind in s["runs"]:
                if blocks >= 4 and ncorr:
                    saw("EOB run of 4 blocks or more with corrections", fam)
                    if empty_behind:
                        saw("empty block inside an EOB run of 4 blocks or more that holds corrections", fam)
            if s["skipped"]:
                saw("blocks inside an EOB run", fam)
            for (coded, ncorr, _), (coded1, ncorr1, in_run1) in zip(s["blocks"], s["blocks"][1:]):
                if width == 63 and coded and ncorr and in_run1 and not coded1 and not ncorr1:  # (1..63: an empty BLOCK, not an empty band)
                    saw("empty block right behind corrections that wait behind a block's last new coefficient", fam)
            if max(coded for coded, _, _ in s["blocks"]) >= 6:
                saw("block with six new coefficients or more", fam)
        corners = np.array([k in (1, 31, 32, 33, 62, 63) for k in range(64)])[np.argsort(hc.ZZ)]
        top_al = hc.scripts(len(LAYOUTS[case[3]][2]))[case[0]][1]
        for p in make_case(*case)[1]:
            at = p.reshape(-1, 64)[(((p.reshape(-1, 64) != 0) == corners) | (np.arange(64) == 0)).all(axis=1)]
            if len(at) and (np.abs(at[:, corners]) < 2 << top_al).any() and (np.abs(at[:, corners]) >= 2 << top_al).any():
                saw("history and new coefficients at positions 1, 31, 32, 33, 62, 63 and nowhere else", fam)
    return seen


EVERY_FAMILY = [f"coefficient with tot + ncorr = {n}" for n in (31, 32, 33)] + ["coefficient with tot + ncorr >= 48", "ZRL with 1..16 corrections"]
SOMEWHERE = (["ZRL with tot + ncorr > 32", "EOB run of 4 blocks or more with corrections",
              "empty block inside an EOB run of 4 blocks or more that holds corrections", "blocks inside an EOB run",
              "empty block right behind corrections that wait behind a block's last new coefficient",
              "block with six new coefficients or more", "history and new coefficients at positions 1, 31, 32, 33, 62, 63 and nowhere else",
              "ZRL with 16 corrections", "ZRL with 9 corrections", "band with se = 31", "band with ss = 32", "band with se = 32", "band with ss = 33", "band 63..63", "band 1..1",
              "DC first pass with Al = 3", "DC scan of one component (first pass)", "DC scan of one component (refinement)"]
             + [f"trailing corrections fill a band of {w}" for w in (1, 31, 32, 63)])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_history_content_reaches_what_it_claims(precision):
    """From the writer's trace of every stream the GPU tests decode.  The sums 31, 32 and 33 bits (a symbol and its corrections
    just inside, filling and just past the reader's 32-bit window) come from every family: code lengths of 2..16 bits for the
    symbols (run, 1) meet correction counts of 12..50 (history_content, run_new).  ZRL with more than 32 bits needs 26 correction
    bits behind a 7-bit code at least, which zrl_long provides for every code length."""
    seen = _events([c for c in gpu_corpus() if c[1] == precision])
    for event in EVERY_FAMILY:
        assert seen.get(event, set()) >= set(FAMILIES), (event, sorted(seen.get(event, ())))
    for event in SOMEWHERE:
        assert seen.get(event), event
    assert seen["ZRL with tot + ncorr > 32"] >= set(FAMILIES)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def on_the_device(dev, oracle, case, what):
    data, planes, _ = make_case(*case)
    outcome = device_matches(dev, oracle, data, planes, case[1], f"{case} {what}")
    assert outcome.startswith("on the device"), (case, what, outcome)
    return outcome


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, "1", "2"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("script", SCRIPTS)
def test_prog_kernel_on_crafted_scripts(dev, oracle, monkeypatch, script, precision, lanes):
    """Every stream of the script's corpus decodes on the device -- the intended planes, the host decoder's range check, the
    oracle's pixels -- at the lane count the launch picks (1 for pictures this small) and with MIJPEG_HUFF_LANES 1 and 2."""
    if lanes:
        monkeypatch.setenv("MIJPEG_HUFF_LANES", lanes)
    outcomes = {on_the_device(dev, oracle, (script, precision) + c, f"lanes {lanes}") for c in corpus(script, precision)}
    print(f"{script} {precision}-bit lanes {lanes}: {len(corpus(script, precision))} streams, {sorted(outcomes)}")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("script", SCRIPTS)
def test_host_decoder_pixels_on_crafted_scripts(dev, oracle, script, precision):
    """The host entropy decoder's planes at 1 and 8 threads, reconstructed (a decoder object without a device has no
    reconstruction path): the oracle's pixels."""
    for case in corpus(script, precision):
        fam, layout, dri = case[:3]
        data, planes, _ = make_case(script, precision, *case)
        want = oracle_pixels(oracle, data, precision)
        for threads in (1, 8):
            dev.read(data, threads=threads, entropy="host")
            assert dev.entropy_used == "host"
            assert np.array_equal(dev.reconstruct(), want), f"{fam} {layout} DRI {dri}, {threads} threads"


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, "64"])
@pytest.mark.parametrize("script", ["deep", "split32"])
def test_prog_kernel_fills_every_lane_slot(dev, oracle, monkeypatch, script, lanes):
    """156 restart intervals of one block each, at the default lane count and at 64 lanes a wave: the largest MIJPEG_HUFF_LANES
    that lanes_for takes, and launch_huffman_prog accepts it -- 340 bytes a lane, four waves a workgroup and three tables at the
    most (an interleaved DC scan of three components; one here) are 97 536 bytes of the 160 KiB of LDS.  One workgroup then holds two full waves of block slots and lists of free
    positions and 28 lanes of a third (the fourth idles): the XOR swizzle of the slots over all eight chunk indices, every list
    of free positions, whole-wave and partial-wave fetches and write-backs."""
    if lanes:
        monkeypatch.setenv("MIJPEG_HUFF_LANES", lanes)
    for case in lane_slot_cases(script):
        planes = make_case(*case)[1]
        assert len(planes) == 1 and planes[0].shape[:2] == (12, 13)
        on_the_device(dev, oracle, case, f"lanes {lanes}")


@pytest.mark.gpu
def test_scans_side_by_side(dev, oracle):
    """split33 on 4:2:0: every component's six scans follow one another, so the device's schedule has six levels for the 18
    scans -- the three DC first passes of one component each in one launch, then three launches with one AC scan of every
    component (first passes beside refinements, luma beside chroma, other tables in every workgroup), the three DC refinements,
    the three refinements of 33..63.  (The library has no counter of these launches, so this asserts what they leave behind:
    the planes, the range check and the pixels.)"""
    for case in side_by_side_cases():
        on_the_device(dev, oracle, case, "side by side")

"""mijpeg_transcode_ragged_device on the device: the pictures of a decoded ragged batch coded again from their planes in HBM.
Everything is equality at tolerance 0.  The references:

  the model        tests/requant_model.py: the rule in numpy int64 over the source's planes, laid out in the output frame
  host coder       api.encode_coefficients(output frame, model planes, restart interval, optimize, threads=1): every served stream
                   equals it byte for byte, headers included -- so requant_list_kernel equals the model and the passes' coder the host's
  oracle decoder   oracle.decode_coefficients(output) returns the model's planes on the blocks that cover samples
  existing path    mijpeg_encode_coefficients_device of the same stream, for kept pictures
  reference binary where it is built, it decodes every 8-bit output of the mixed list to the oracle's pixels

Crafted sources are written by the host coder (api.encode_coefficients takes any tables), the rest are committed goldens."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import requant_model as M
from conftest import ROOT, golden_jpeg
from libjpeg_amd import api, batch
from test_ragged_transcode_cpu import _decoded

pytestmark = pytest.mark.gpu

LAYOUTS = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": [(1, 1)] * 3, "grey": [(1, 1)]}
GROUP = ["pil_131x77_422", "pil_80x48_444", "pil_70x40_gray", "pil_9x9_420", "pil_1x1_444", "p12_120x90_420_dri3", "p12_64x48_444"]
CHILDREN = ["pilprog_75x45_420", "refprog_64x64_444_dri5", "ref_97x61_440", "ref_97x61_411", "ref_64x64_2x4", "ref_23x50_lumasub", "ref_97x61_420_dnl",
            "ref_120x88_sof1_420"]
QUALITIES = [None, 2, 50, 95, 100]
INTERVALS = [None, 0, 1]


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ helpers
def _covered(f, c):
    """(rows, columns) of the blocks of component c that cover samples"""
    return ((f.height + f.suby[c] - 1) // f.suby[c] + 7) // 8, ((f.width + f.subx[c] - 1) // f.subx[c] + 7) // 8


def _expected(f, planes, quality, ri, optimize):
    """what the call owes for a decoded picture: (status, stream or None, output frame, model planes)"""
    rc, out, ri, kept = M.plan(f, quality, ri)
    if rc:
        return rc, None, None, None
    flat, beyond = M.transcode_planes(f, planes, out)
    if beyond:
        return api.ERR_OVERFLOW_PARAMETER, None, out, flat
    return 0, api.encode_coefficients(out, flat, ri, optimize, threads=1), out, flat


_oracle_seen = {}


def _check_against_oracle(oracle, stream, out, flat, ri, what):
    key = hashlib.sha256(stream).digest()
    if key in _oracle_seen:  # (the same bytes were checked against the same model)
        return
    _oracle_seen[key] = True
    oi, back = oracle.decode_coefficients(stream)
    assert (oi.width, oi.height, oi.precision, oi.restart_interval, oi.ncomp) == (out.width, out.height, out.precision, ri, out.components), what
    assert [list(oi.quant[oi.tq[c]]) for c in range(oi.ncomp)] == [list(out.quant[out.quant_index[c]]) for c in range(oi.ncomp)], what
    for c in range(out.components):
        rows, cols = _covered(out, c)
        want = flat[out.coef_offset[c]:out.coef_offset[c] + out.blocks_w[c] * out.blocks_h[c] * 64].reshape(out.blocks_h[c], out.blocks_w[c], 64)
        assert np.array_equal(np.asarray(back[c]).reshape(back[c].shape[0], back[c].shape[1], 64)[:rows, :cols], want[:rows, :cols]), (what, c)


def _specs(qualities, intervals):
    return [(api.TRANSCODE_KEEP if q is None else q, -1 if r is None else r) for q, r in zip(qualities, intervals)]


def _transcode_and_check(dec, oracle, sources, qualities, intervals, optimize, what, with_oracle=True):
    """sources: [(info, planes)] of the pictures the object has decoded; -> (streams, status)"""
    got, status = dec.transcode_ragged_device(_specs(qualities, intervals), optimize)
    for i, ((f, planes), q, r) in enumerate(zip(sources, qualities, intervals)):
        rc, want, out, flat = _expected(f, planes, q, r, optimize)
        assert status[i] == rc, (what, i, q, r, status[i], rc)
        assert got[i] == want, (what, i, q, r, None if got[i] is None else len(got[i]), None if want is None else len(want))
        if want is not None and with_oracle:
            _check_against_oracle(oracle, got[i], out, flat, M.plan(f, q, r)[2], (what, i, q, r))
    return got, status


# ------------------------------------------------------------------------------------------------ 1. crafted planes
def _crafted(precision):
    """[(name, info, planes, stream)]: every layout at every size under every table, noise inside the coding range at every position
    (|c| <= range // entry, so that no quality takes a value out of it), then the rule's halves and the range's extremes."""
    rng = np.random.default_rng(4300 + precision)
    dc_min, dc_max, ac_max = M.coding_range(precision)
    tables = {"ones": np.ones(64, int), "255": np.full(64, 255), "random": rng.integers(1, 256, 64)}
    if precision == 12:
        tables["wide"] = rng.integers(1, 32768, 64)
        tables["wide"][:3] = (32767, 1, 300)
    out = []

    def add(name, w, h, layout, tab0, tab1, fill, ri):
        samp = LAYOUTS[layout]
        f = api.frame_layout(w, h, len(samp), [s[0] for s in samp], [s[1] for s in samp], [tab0, tab1], ycbcr=int(len(samp) == 3), precision=precision)
        f.restart_interval = ri
        planes = [fill(c, (f.blocks_h[c], f.blocks_w[c], 64), np.array(f.quant[f.quant_index[c]][:])) for c in range(f.components)]
        flat = np.concatenate([p.reshape(-1) for p in planes]).astype(np.int16)
        out.append((name, f, planes, api.encode_coefficients(f, flat, ri, False, threads=1)))

    def noise(c, shape, tab):
        amp = ac_max // tab
        return rng.integers(-amp, amp + 1, shape).astype(np.int16)

    k = 0
    for layout in LAYOUTS:
        for w, h in [(8, 8), (17, 9), (40, 24)] + ([(136, 136)] if layout == "420" else []):
            for tname, tab in tables.items():
                add(f"{layout}_{w}x{h}_{tname}", w, h, layout, tab, tab[::-1].copy(), noise, (0, 2)[k % 2])
                k += 1
    # halves of both signs under entries of 1: c = (2 j + 1) b / 2 for the even entries b of the target tables, one below and above
    targets = sorted({int(b) for q in (2, 50, 95) for b in M.plan(out[0][1], q)[1].quant[0] if b % 2 == 0 and b // 2 <= ac_max})

    def halves(c, shape, tab):
        v = np.array([s * ((2 * j + 1) * b // 2 + d) for b in targets for j in range(3) for d in (-1, 0, 1) for s in (1, -1)])
        v = v[np.abs(v) <= ac_max]
        return np.resize(v, shape).astype(np.int16)

    def extremes(c, shape, tab):
        p = np.resize(np.array([ac_max, -ac_max, 1, -1, ac_max - 1, 0, -ac_max + 1]), shape).astype(np.int16)
        p[..., 0] = np.resize(np.array([dc_min, dc_max, 0, dc_max, dc_min]), shape[:2])
        return p

    add("halves_444", 40, 24, "444", tables["ones"], tables["ones"], halves, 0)
    add("halves_420", 17, 9, "420", tables["ones"], tables["ones"], halves, 1)
    add("extremes_422", 40, 24, "422", tables["ones"], tables["ones"], extremes, 0)
    add("extremes_grey", 17, 9, "grey", tables["ones"], tables["ones"], extremes, 0)
    return out


@pytest.mark.parametrize("precision", [8, 12])
def test_kernel_is_the_model_and_the_coder_is_the_host_coder(dec, oracle, precision):
    crafted = _crafted(precision)
    n = len(crafted)
    status = dec.decode_ragged_device([s for _, _, _, s in crafted], with_12bit=True)
    assert status == [0] * n
    sources = []
    for i, (name, f, planes, _) in enumerate(crafted):
        g = dec.ragged_info(i)
        assert (g.width, g.height, g.precision, g.restart_interval, list(g.quant[0])) == (f.width, f.height, precision, f.restart_interval, list(f.quant[0])), name
        sources.append((g, planes))
    assert dec.ragged_stats()["ragged"] == n  # (every crafted picture is a member of a layout group)
    served = 0
    for k, quality in enumerate(QUALITIES):
        for optimize in (False, True):
            qualities = [quality] * n
            intervals = [INTERVALS[(i + k + optimize) % 3] for i in range(n)]
            got, st = _transcode_and_check(dec, oracle, sources, qualities, intervals, optimize, (precision, quality, optimize))
            stats = dec.transcode_ragged_stats()
            assert stats["requant_launches"] == stats["passes"] == 1 and stats["pictures"] == n and stats["children"] == 0
            assert stats["served"] == sum(s is not None for s in got) and stats["kept"] == (stats["served"] if quality is None else 0)
            served += stats["served"]
            if quality is None:  # a kept recode is lossless: the oracle reads the source's coefficients back (checked above), nothing refused
                assert st == [0] * n
    assert served >= 9 * n  # (the extremes leave the range at some qualities; nearly everything else is served at all of them)


# ------------------------------------------------------------------------------------------------ 2. kept is the existing path
@pytest.mark.parametrize("name", ["pil_200x120_420_dri8", "ref_33x17_420_dri1", "enc12/420_272x144_z4"])
def test_kept_is_the_single_frame_path(dec, name):
    data = golden_jpeg(name)
    one = api.Decoder(0)
    try:
        info = one.read(data, entropy="gpu")
        want = {opt: one.encode_coefficients_device(info, one.device_coefficients(), info.restart_interval, opt) for opt in (False, True)}
    finally:
        one.close()
    assert dec.decode_ragged_device([data], with_12bit=True) == [0]
    for opt in (False, True):
        got, status = dec.transcode_ragged_device(None, opt)
        assert status == [0] and got[0] == want[opt], (name, opt)
        st = dec.transcode_ragged_stats()
        assert (st["served"], st["kept"], st["refused"], st["passes"], st["requant_launches"]) == (1, 1, 0, 1, 1)


# ------------------------------------------------------------------------------------------------ 3. one list, every route
def _mixed_list():
    names = GROUP + CHILDREN + ["pil_90x60_cmyk", "xt_64x48_444"]
    streams = [golden_jpeg(n) for n in names] + [golden_jpeg("pil_80x48_444")[:100], b""]
    qualities = [(None, 75, 30, None, 100, None, 50, 95, None, 75, 2, None, 50, None, 95)[i % 15] for i in range(len(names))] + [None, 50]
    intervals = [(None, 0, 1, 3, None)[i % 5] for i in range(len(streams))]
    return names, streams, qualities, intervals


def test_one_list_every_route(dec, oracle):
    names, streams, qualities, intervals = _mixed_list()
    n = len(streams)
    skip = names.index("pil_80x48_444")
    decode_status = dec.decode_ragged_device(streams, with_12bit=True)
    assert all(s == 0 for s in decode_status[:len(names)]) and decode_status[-2] != 0 and decode_status[-1] != 0
    group = [dec.ragged_route(i)[0] for i in range(len(names))]
    # (the route is the decode's to choose: an 8-bit SOF1 frame of a group's layout may be a member; the other seven have no group)
    assert group[:len(GROUP)] == [True] * len(GROUP) and sum(not g for g in group[len(GROUP):]) >= len(CHILDREN) - 1
    specs = _specs(qualities, intervals)
    specs[skip] = (api.TRANSCODE_SKIP, 0)
    for optimize in (False, True):
        got, status = dec.transcode_ragged_device(specs, optimize)
        stats = dec.transcode_ragged_stats()
        served = kept = children = 0
        for i in range(n):
            what = (names[i] if i < len(names) else "damaged", optimize)
            if i >= len(names):
                assert status[i] == decode_status[i] and got[i] is None, what
                continue
            if i == skip:
                assert status[i] == 0 and got[i] is None
                continue
            f, planes = _decoded(names[i]) if names[i] not in ("pil_90x60_cmyk", "xt_64x48_444") else (dec.ragged_info(i), None)
            if planes is None:
                assert status[i] == api.ERR_NOT_IMPLEMENTED and got[i] is None, what
                continue
            rc, want, out, flat = _expected(f, planes, qualities[i], intervals[i], optimize)
            assert rc == 0 and status[i] == 0 and got[i] == want, (what, qualities[i], intervals[i])
            _check_against_oracle(oracle, got[i], out, flat, M.plan(f, qualities[i], intervals[i])[2], what)
            served += 1
            kept += qualities[i] is None
            children += not group[i]
            if f.precision == 8:
                pixels = oracle.decode(got[i])
                if qualities[i] is None:  # a lossless recode: the source's pixels
                    assert np.array_equal(pixels, oracle.decode(streams[i])), what
                if oracle.have_reference():
                    assert np.array_equal(oracle.reference_decode(got[i]), pixels), what
        assert (stats["pictures"], stats["served"], stats["kept"], stats["children"]) == (n, served, kept, children) and served == len(names) - 3
        assert stats["refused"] == 4 and stats["passes"] == stats["requant_launches"] == 1 and stats["host_syncs"] == 4 and stats["bytes_downloaded"] > 0
        assert stats["child_uploads"] <= children


# ------------------------------------------------------------------------------------------------ 4. launches do not grow
def test_launches_and_waits_do_not_grow_with_the_list(dec):
    four = [golden_jpeg(n) for n in GROUP[:4]]
    stats = {}
    for times in (1, 8):
        assert dec.decode_ragged_device(four * times) == [0] * (4 * times)
        for optimize in (False, True):
            got, status = dec.transcode_ragged_device([(75, 0)] * (4 * times), optimize)
            assert status == [0] * (4 * times) and got[:4] * times == got
            stats[(times, optimize)] = dec.transcode_ragged_stats()
    for optimize in (False, True):
        a, b = stats[(1, optimize)], stats[(8, optimize)]
        assert (a["pictures"], b["pictures"]) == (4, 32) and b["bytes_downloaded"] > a["bytes_downloaded"]
        for k in ("requant_launches", "coder_launches", "host_syncs", "passes"):
            assert a[k] == b[k], (k, optimize, a, b)
        assert a["requant_launches"] == a["passes"] == 1 and a["host_syncs"] == (4 if optimize else 3)


# ------------------------------------------------------------------------------------------------ 5. pass cuts do not show
_CUT_CHILD = """
import hashlib, json, sys
sys.path.insert(0, "tests")
from conftest import golden_jpeg
from libjpeg_amd import api
names, specs = json.loads(sys.argv[1])
d = api.Decoder(0)
assert d.decode_ragged_device([golden_jpeg(n) for n in names], with_12bit=True) == [0] * len(names)
got, status = d.transcode_ragged_device([tuple(s) for s in specs], True)
print(json.dumps(dict(status=status, sha=[hashlib.sha256(g).hexdigest() for g in got], stats=d.transcode_ragged_stats())))
d.close()
"""


def test_pass_cuts_do_not_show(dec):
    specs = [(0, -1), (75, 0), (30, 1), (0, 2), (100, -1), (0, -1), (50, 3)]
    assert dec.decode_ragged_device([golden_jpeg(n) for n in GROUP], with_12bit=True) == [0] * len(GROUP)
    whole, status = dec.transcode_ragged_device(specs, True)
    assert status == [0] * len(GROUP) and dec.transcode_ragged_stats()["passes"] == 1
    env = dict(os.environ, MIJPEG_ENCODE_RAGGED_PASS_BLOCKS="256")
    r = subprocess.run([sys.executable, "-c", _CUT_CHILD, json.dumps([GROUP, specs])], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cut = json.loads(r.stdout.strip().splitlines()[-1])
    assert cut["status"] == status and cut["sha"] == [hashlib.sha256(g).hexdigest() for g in whole]
    st = cut["stats"]
    assert st["passes"] > 1 and st["requant_launches"] == st["passes"] and st["served"] == len(GROUP) and st["host_syncs"] <= 4 * st["passes"]


# ------------------------------------------------------------------------------------------------ 6. refusal by range
def _crafted_one(at, value, entry):
    f = api.frame_layout(24, 16, 3, (1, 1, 1), (1, 1, 1), [np.full(64, entry)] * 2, precision=8)
    planes = [np.zeros((2, 3, 64), np.int16) for _ in range(3)]
    planes[1][1, 2, at] = value
    planes[0][0, 0, 0] = 5
    return f, planes, api.encode_coefficients(f, np.concatenate([p.reshape(-1) for p in planes]), 0, False, threads=1)


def test_a_value_outside_the_coding_range_refuses_its_picture_alone(dec, oracle):
    f, planes, bad = _crafted_one(9, 1000, 16)  # an AC value of 1000 under an entry of 16: 16000 at quality 100
    neighbours = [golden_jpeg("pil_9x9_420"), golden_jpeg("pil_70x40_gray")]
    streams = [neighbours[0], bad, neighbours[1]]
    sources = [_decoded("pil_9x9_420"), (f, planes), _decoded("pil_70x40_gray")]
    assert dec.decode_ragged_device(streams) == [0, 0, 0]
    for optimize in (False, True):
        got, status = _transcode_and_check(dec, oracle, sources, [100, 100, 100], [None, None, 0], optimize, "range")
        assert status == [0, api.ERR_OVERFLOW_PARAMETER, 0] and got[1] is None and got[0] and got[2]
        st = dec.transcode_ragged_stats()
        assert (st["served"], st["refused"], st["kept"]) == (2, 1, 0)
        # the object serves the next call, and the same picture kept (1000 is inside the range) is served
        got, status = _transcode_and_check(dec, oracle, sources, [50, None, None], [None, None, None], optimize, "range, kept")
        assert status == [0, 0, 0] and all(got)
        _, back = oracle.decode_coefficients(got[1])
        assert back[1][1, 2].reshape(-1)[9] == 1000
    # a crafted stream's own planes go through the same check: a kept picture with a DC of 1500
    f2, planes2, dc = _crafted_one(0, 1500, 3)
    assert dec.decode_ragged_device([dc, neighbours[0]]) == [0, 0]
    got, status = _transcode_and_check(dec, oracle, [(f2, planes2), sources[0]], [None, None], [None, None], False, "kept dc")
    assert status == [api.ERR_OVERFLOW_PARAMETER, 0] and got[0] is None and got[1]
    # the call's own argument checks, with a decoded batch on the object: outputs cleared, nothing served
    for spec in ((101, 0), (-2, 0), (50, 65536)):
        with pytest.raises(api.MijpegError) as e:
            dec.transcode_ragged_device([spec, (0, -1)])
        assert e.value.code == api.ERR_INVALID_PARAMETER
    assert dec.transcode_ragged_device(None)[1] == [api.ERR_OVERFLOW_PARAMETER, 0]


# ------------------------------------------------------------------------------------------------ 7. the stores survive
def test_the_decodes_stores_survive(dec):
    import torch

    names = ["pil_131x77_422", "pil_70x40_gray", "pilprog_75x45_420", "ref_97x61_440", "pil_9x9_420"]
    streams = [golden_jpeg(n) for n in names]
    specs = [(50, 0), (0, -1), (75, 1), (0, -1), (100, 2)]

    def pixels():
        infos = [dec.ragged_info(i) for i in range(len(names))]
        tensors = [torch.zeros((f.height, f.width * f.components), dtype=torch.uint8, device="cuda:0") for f in infos]
        dec.reconstruct_ragged_device([t.data_ptr() for t in tensors], [f.width * f.components for f in infos])
        return [t.cpu().numpy() for t in tensors]

    assert dec.decode_ragged_device(streams) == [0] * len(names)
    before = pixels()
    first, status = dec.transcode_ragged_device(specs, False)
    assert status == [0] * len(names)
    after = pixels()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    again, _ = dec.transcode_ragged_device(specs, False)
    assert again == first
    # the same list through the device marker route
    marked = api.Decoder(0)
    try:
        marked.set_device_markers(1)
        assert marked.decode_ragged_device(streams) == [0] * len(names)
        assert marked.transcode_ragged_device(specs, False)[0] == first
    finally:
        marked.close()
    # without a decoded ragged batch the call fails as the reconstruction call does
    fresh = api.Decoder(0)
    try:
        with pytest.raises(api.MijpegError) as e:
            fresh.transcode_ragged_device(None)
        assert e.value.code == -1031
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 8. batch.transcode_mixed
def test_transcode_mixed(dec):
    names = ["pil_131x77_422", "pil_90x60_cmyk", "p12_64x48_444", "pilprog_75x45_420", "pil_70x40_gray"]
    streams = [golden_jpeg(n) for n in names] + [b"\xff\xd8 not a picture"]
    n = len(streams)
    quality = [50, 50, None, 75, None, 30]
    ri = [None, 0, 2, 0, None, 0]
    whole = batch.transcode_mixed(streams, quality, ri, decoder=dec)
    st = dec.transcode_ragged_stats()
    assert (st["pictures"], st["served"], st["refused"], st["kept"]) == (n, 4, 2, 2)
    for i in (0, 2, 3, 4):
        f, planes = _decoded(names[i])
        assert whole[i] == _expected(f, planes, quality[i], ri[i], False)[1], names[i]
    assert isinstance(whole[1], api.MijpegError) and whole[1].code == api.ERR_NOT_IMPLEMENTED
    assert isinstance(whole[5], api.MijpegError) and whole[5].code not in (0, api.ERR_NOT_IMPLEMENTED)
    # one value for all, and the defaults: everything kept
    same = batch.transcode_mixed(streams[:1] + streams[3:5], 50, 0, decoder=dec)
    assert same[0] == _expected(*_decoded(names[0]), 50, 0, False)[1] and same[2] == _expected(*_decoded(names[4]), 50, 0, False)[1]
    kept = batch.transcode_mixed(streams[:1] + streams[4:5], optimize=True)
    assert kept[0] == _expected(*_decoded(names[0]), None, None, True)[1] and kept[1] == _expected(*_decoded(names[4]), None, None, True)[1]
    # two ranks' results interleave to the single-rank list
    parts = [batch.transcode_mixed(streams, quality, ri, rank=r, world=2) for r in range(2)]
    for i in range(n):
        mine, other = parts[i % 2][i], parts[1 - i % 2][i]
        assert other is None
        if isinstance(whole[i], api.MijpegError):
            assert isinstance(mine, api.MijpegError) and mine.code == whole[i].code
        else:
            assert mine == whole[i]
    with pytest.raises(ValueError):
        batch.transcode_mixed(streams, quality[:2])

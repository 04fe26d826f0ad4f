"""Entropy decoders on Huffman tables and coefficients the test chose (tests/huffcraft.py): long codes past the device's
second-level tables (the canonical walk of huffman.hip:dev_lookup), the widest symbols (a 16-bit code and 15 value bits),
near-fixed-length codes for the self-synchronising walk, degenerate and incomplete tables, coefficients at every category
boundary, and the saturation of the range check.

Every stream is checked three ways before a decoder sees it: the oracle decodes exactly the coefficients the writer was given
(a writer bug cannot pass for a decoder bug), and where the reference binary is built its pixels are the oracle's.  Then the
host decoder (one and eight threads) and, with -m gpu, every device decoder must return those coefficients, the host's range
check, and the oracle's pixels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import huffcraft as hc
from libjpeg_amd import api

LAYOUTS = {  # (width, height, sampling); progressive frames are whole MCUs
    "420": (45, 29, [(2, 2), (1, 1), (1, 1)]), "444": (21, 19, [(1, 1)] * 3), "grey": (27, 13, [(1, 1)]),
    "p420": (48, 32, [(2, 2), (1, 1), (1, 1)]), "p444": (24, 16, [(1, 1)] * 3), "pgrey": (32, 24, [(1, 1)]),
}
CONTENTS_12 = hc.CONTENTS + ("saturate",)


def make_case(precision, progressive, fam, kind, dri, layout, seed=0, size=None, own_chroma=False):
    """-> (stream, intended planes, symbols written, (dc, ac)); own_chroma: Cb / Cr code with hc.chroma_variant of the tables"""
    dc, ac = hc.family(fam, precision, progressive)
    w, h, samp = LAYOUTS[layout]
    if size:
        w, h = size
    rng = np.random.default_rng([precision, int(progressive), hc.FAMILIES.index(fam), CONTENTS_12.index(kind), dri, seed])
    shapes = hc.plane_shapes(w, h, samp)
    dcs, acs = hc.uses(dc, ac)
    planes = hc.content("sparse" if kind == "saturate" else kind, shapes, precision, rng, dcs, acs)
    quant16 = kind == "saturate"
    if quant16:  # 16-bit deltas: sum |c| q passes 2^31 in one block of every component
        quant = [np.full(64, 65535 - 9 * c) for c in range(len(samp))]
        for p, q in zip(planes, quant):
            hc.saturating_block(p, q, precision)
    else:
        quant = [rng.integers(1, 24 if precision == 8 else 200, 64) for _ in samp]
    used = set()
    tables = [(dc, ac)] + [(hc.chroma_variant(dc), hc.chroma_variant(ac)) if own_chroma else (dc, ac)] * (len(samp) - 1)
    data = hc.write(planes, w, h, samp, tables, precision=precision, quant=quant, dri=dri, progressive=progressive,
                    quant16=quant16, used=used)
    return data, planes, used, (dc, ac)


def oracle_pixels(oracle, data, precision):
    return oracle.decode(data) if precision == 8 else oracle.decode16(data)


def check_stream(oracle, data, planes, precision):
    """The writer's self-check: the oracle decodes the intended coefficients; the reference binary (where built) the oracle's
    pixels."""
    _, got = oracle.decode_coefficients(data)
    assert len(got) == len(planes)
    for c, (g, p) in enumerate(zip(got, planes)):
        assert np.array_equal(g, p), f"writer / oracle: component {c}, {int((g != p).sum())} coefficients differ"
    if oracle.have_reference():
        px, err = oracle.reference_decode_status(data)
        assert err == 0, err
        assert np.array_equal(px.reshape(oracle_pixels(oracle, data, precision).shape), oracle_pixels(oracle, data, precision)), "reference / oracle"


def same_planes(dec, planes, what):
    for c, p in enumerate(planes):
        got = dec.coefficients(c).astype(np.int32)
        assert np.array_equal(got, p), f"{what}: component {c}, {int((got != p).sum())} coefficients differ"


SEQ = [(8, False, f) for f in hc.FAMILIES] + [(12, False, f) for f in hc.FAMILIES]
PROG = [(8, True, f) for f in hc.PROGRESSIVE_FAMILIES] + [(12, True, f) for f in hc.PROGRESSIVE_FAMILIES]


def contents(precision, fam):
    """(degenerate tables code no saturating block: one DC category, one AC symbol)"""
    return CONTENTS_12 if precision == 12 and fam != "degenerate" else hc.CONTENTS


# ---------------------------------------------------------------------------------------------------------------------------
# the tables themselves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,progressive", [(8, False), (12, False), (8, True), (12, True)])
def test_table_families_are_what_they_claim(precision, progressive):
    fams = hc.PROGRESSIVE_FAMILIES if progressive else hc.FAMILIES
    for fam in fams:
        dc, ac = hc.family(fam, precision, progressive)
        for t in (dc, ac):
            assert hc.kraft(l for _, l in t.codes.values()) < 1.0, fam
        if fam in ("prefixes8", "prefixes9"):
            pre = hc.long_prefixes(ac)
            assert len(pre) == int(fam[-1])
            # the most frequent symbols sit under the last prefix: EOB on the longest code
            assert ac.codes[0x00][1] == 12 and ac.codes[0x00][0] >> 2 == pre[-1]
        if fam == "all_long":
            assert all(l >= 11 for _, l in dc.codes.values()) and all(l >= 11 for _, l in ac.codes.values())
            assert len(hc.long_prefixes(ac)) > 8  # some lookups walk the canonical arrays
        if fam == "len16_widest":
            wd, wa = hc.widest(precision, progressive)
            assert all(dc.length(s) == 16 for s in wd) and all(ac.length(s) == 16 for s in wa)
        if fam == "fixed8":
            assert {l for _, l in ac.codes.values()} <= {8, 9} and {l for _, l in dc.codes.values()} <= {4, 5}
        if fam == "incomplete_with_unused":
            assert hc.kraft(l for _, l in ac.codes.values()) <= 0.5
            assert all(r << 4 in ac.codes for r in range(1, 15))
            if precision == 8:
                assert all(s in dc.codes for s in range(12, 16))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the writer against the oracle (and the reference), the host decoder against the intended coefficients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,progressive,fam", SEQ + PROG)
def test_host_decoder_on_crafted_tables(oracle, precision, progressive, fam):
    layouts = ("p420", "p444", "pgrey") if progressive else ("420", "444", "grey")
    one, eight = api.Decoder(None), api.Decoder(None)
    reached = set()
    for kind in contents(precision, fam):
        for i, dri in enumerate((0, 1, 7)):
            data, planes, used, (dc, ac) = make_case(precision, progressive, fam, kind, dri, layouts[i])
            reached |= {s for t, s in used if t == id(ac)}
            check_stream(oracle, data, planes, precision)
            for d, threads in ((one, 1), (eight, 8)):
                f = d.read(data, threads=threads)
                assert f.progressive == int(progressive) and f.precision == precision
                same_planes(d, planes, f"host decoder, {threads} threads, {kind}, DRI {dri}")
            assert list(one.info.range_max) == list(eight.info.range_max) and one.info.fast_arith == eight.info.fast_arith
            if kind == "saturate":
                assert max(one.info.range_max[:one.info.components]) == 2 ** 31 - 1
    if fam == "len16_widest":  # the symbols of the largest categories (and EOB14, test below) were really written
        wa = set(hc.widest(precision, progressive)[1]) - {0xE0}
        assert reached & wa, sorted(reached)
    one.close()
    eight.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision,progressive,fam", SEQ + PROG)
def test_host_decoder_pixels_on_crafted_tables(dev, oracle, precision, progressive, fam):
    """The host entropy decoder's planes at 1 and 8 threads, reconstructed (a decoder object without a device has no
    reconstruction path): the oracle's pixels."""
    layouts = ("p420", "p444", "pgrey") if progressive else ("420", "444", "grey")
    for kind in contents(precision, fam):
        for i, dri in enumerate((0, 1, 7)):
            data, planes, _, _ = make_case(precision, progressive, fam, kind, dri, layouts[i])
            want = oracle_pixels(oracle, data, precision)
            for threads in (1, 8):
                dev.read(data, threads=threads, entropy="host")
                assert dev.entropy_used == "host"
                assert np.array_equal(dev.reconstruct(), want), f"{kind}, DRI {dri}, {threads} threads"


def _eob14_case(fam="len16_widest", precision=8, dri=0):
    """A grey progressive picture of 16 640 blocks of which few carry AC coefficients: EOB runs past 16 384 blocks (EOB14)."""
    w, h = 1024, 1040
    dc, ac = hc.family(fam, precision, True)
    rng = np.random.default_rng(14)
    plane = np.zeros(hc.plane_shapes(w, h, [(1, 1)])[0] + (64,), np.int32)
    flat = plane.reshape(-1, 64)
    flat[:, 0] = np.clip(np.cumsum(rng.integers(-9, 10, len(flat))), -500, 500)
    for b in (0, 1, 2, len(flat) - 1):
        flat[b, hc.ZZ[1:20]] = rng.integers(-300, 300, 19)
    used = set()
    data = hc.write([plane], w, h, [(1, 1)], [(dc, ac)], precision=precision, dri=dri, progressive=True, used=used)
    assert (id(ac), 0xE0) in used
    return data, [plane]


def test_host_decoder_eob14_runs(oracle):
    data, planes = _eob14_case()
    check_stream(oracle, data, planes, 8)
    d = api.Decoder(None)
    d.read(data, threads=4)
    same_planes(d, planes, "host decoder, EOB14")
    d.close()


def test_host_speculative_decoder_on_long_codes(oracle):
    """About 1024 x 1024 without restart markers: large enough that the host cuts the scan into speculative ranges, with codes
    of 11..16 bits everywhere (all_long) and blocks of 63 coefficients."""
    dc, ac = hc.family("all_long", 8, False)
    w, h, samp = 1024, 1024, [(1, 1)]
    rng = np.random.default_rng(7)
    planes = hc.content("runs", hc.plane_shapes(w, h, samp), 8, rng)
    data = hc.write(planes, w, h, samp, [(dc, ac)], dri=0)
    assert len(data) > 400 << 10
    _, got = oracle.decode_coefficients(data)
    assert np.array_equal(got[0], planes[0])
    before = api.speculative_scans()[0]
    d = api.Decoder(None)
    d.read(data, threads=8)
    assert api.speculative_scans()[0] == before + 1  # really taken
    same_planes(d, planes, "speculative host decoder")
    d.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: every device decoder against the intended coefficients, the host's range check and the oracle's pixels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = api.Decoder(0)
    yield d
    d.close()


def device_matches(dev, oracle, data, planes, precision, what, may_decline=None):
    """entropy="gpu" must decode on the device and give the intended coefficients, the host decoder's range check and the
    oracle's pixels.  may_decline: the reason why the self-synchronising walk may give up on this stream -- then only with
    ERR_NOT_AVAILABLE "did not settle" (a walk that settled on something else, or any other refusal, fails), and "auto"
    must decode it exactly (on the host).  -> what happened, for the assertion messages."""
    host = api.Decoder(None)
    try:
        hi = host.read(data, threads=1)
        try:
            gi = dev.read(data, entropy="gpu")
            outcome = f"on the device, walk rounds {dev.device_walk_rounds()}"
        except api.MijpegError as e:
            if not may_decline:
                raise
            assert e.code == api.ERR_NOT_AVAILABLE and "did not settle" in str(e), (what, e.code, str(e))
            outcome = f"declined ({may_decline})"
            gi = dev.read(data, entropy="auto")
            assert dev.entropy_used == "host", (what, outcome)
        if outcome.startswith("on the device"):
            assert dev.entropy_used == "gpu", what
        assert gi.fast_arith == hi.fast_arith and list(gi.range_max) == list(hi.range_max), (what, outcome, list(gi.range_max), list(hi.range_max))
        out = dev.reconstruct()  # (the device's coefficients: fetched below)
        assert np.array_equal(out, oracle_pixels(oracle, data, precision)), f"{what}: pixels, {outcome}"
        same_planes(dev, planes, f"{what}, {outcome}")
    finally:
        host.close()
    return outcome


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, "1", "2", "64"])
@pytest.mark.parametrize("fam", hc.FAMILIES)
def test_scan_kernel_on_crafted_tables(dev, oracle, monkeypatch, fam, lanes):
    """huffman_scan_kernel (8-bit, restart markers), at the lane count it picks and at 1, 2 and 64 lanes a wave."""
    if lanes:
        monkeypatch.setenv("MIJPEG_HUFF_LANES", lanes)
    for kind in hc.CONTENTS:
        for dri, layout, size in ((1, "420", (96, 64)), (7, "444", (61, 37)), (3, "grey", None)):
            data, planes, _, _ = make_case(8, False, fam, kind, dri, layout, seed=1, size=size)
            device_matches(dev, oracle, data, planes, 8, f"{fam} {kind} DRI {dri} lanes {lanes}")


@pytest.mark.gpu
@pytest.mark.parametrize("sub", [None, "32"])
@pytest.mark.parametrize("fam", hc.FAMILIES)
def test_walk_kernel_on_crafted_tables(dev, oracle, monkeypatch, fam, sub):
    """huffman_walk_kernel (no restart markers: 256 MCUs, more than 4 KiB of data), at the default subsequence size (128 bytes
    here) and at 32 bytes, where the widest symbols straddle subsequence ends.  Luma and chroma have codes of their own (the
    walk cannot find its place in the MCU otherwise).  Every case decodes on the device but those in _walk_may_decline, which
    may give up with "did not settle" only."""
    if sub:
        monkeypatch.setenv("MIJPEG_WALK_SUB", sub)
    on_device = 0
    for kind in ("sparse", "boundaries", "runs"):
        data, planes, _, _ = make_case(8, False, fam, kind, 0, "420", seed=2, size=(256, 256), own_chroma=True)
        outcome = device_matches(dev, oracle, data, planes, 8, f"{fam} {kind} walk sub {sub}", _walk_may_decline(fam, kind, sub))
        on_device += outcome.startswith("on the device")
    if fam not in ("fixed8", "degenerate") and not (fam == "all_long" and sub):
        assert on_device >= 2, (fam, sub, on_device)


def _walk_may_decline(fam, kind, sub):
    """Why the walk may not settle within its 48 rounds on this stream (None: it must settle).  Rounds measured on these
    streams at 128 / 32 bytes a subsequence: sparse and boundaries content settle in 4-20 / 13-34 rounds for every family but
    the two below; a 4x finer split takes 3-4x the rounds."""
    if fam == "fixed8":
        return "near-fixed-length codes: a misaligned parse need not resynchronise"
    if fam == "degenerate":
        # (chroma_variant cannot change a code with one symbol per length: luma and chroma codes are the same)
        return "one code for all components: no parse can tell which block of the MCU it stands in"
    if kind == "runs" and not (fam == "all_long" and not sub):
        # (all_long settles in 28 rounds at 128 bytes; the other families need more than 48)
        return "three blocks in four end without an EOB: a parse that counts coefficient positions wrongly is corrected rarely"
    if fam == "all_long" and sub:
        return "11..16-bit codes settle in 15 / 20 rounds at 128 bytes a subsequence, beyond 48 at 32"
    return None


def _batch_tables():
    a = hc.family("all_long", 8, False)
    b = hc.family("prefixes9", 8, False)
    c = hc.family("straddle10", 8, False)
    return a, b, c


@pytest.mark.gpu
def test_batches_of_crafted_tables(oracle):
    """decode_batch_device and submit / finish: families mixed across the images, with and without restart markers; and a
    pair whose image 0 lets Cb / Cr share one table and whose image 1 does not (the sharing must hold in every image)."""
    torch = pytest.importorskip("torch")
    w, h, samp = 256, 256, [(2, 2), (1, 1), (1, 1)]
    shapes = hc.plane_shapes(w, h, samp)

    def stream(tables, dri, seed, kind="boundaries"):
        rng = np.random.default_rng(seed)
        planes = hc.content(kind, shapes, 8, rng)
        return hc.write(planes, w, h, samp, tables, quant=[np.full(64, 3)] * 3, dri=dri), planes

    fams = ["annexk", "prefixes8", "prefixes9", "all_long", "len16_widest", "straddle10", "incomplete_with_unused"]
    def own(f):
        dc, ac = hc.family(f, 8, False)
        return [(dc, ac)] + [(hc.chroma_variant(dc), hc.chroma_variant(ac))] * 2

    mixed = [stream(own(f), dri, 40 + i) for i, (f, dri) in enumerate(zip(fams, (4, 0, 1, 0, 5, 0, 2)))]
    a, b, c = _batch_tables()
    pair = [stream([a, b, b], 3, 60, "sparse"), stream([a, b, c], 3, 61, "sparse")]
    for group in (mixed, pair, pair[::-1]):
        streams = [s for s, _ in group]
        # the batch's range check is the largest of its images' (what the one reconstruction launch must cover)
        host = api.Decoder(None)
        try:
            want_range = np.max([list(host.read(s, threads=1).range_max)[:3] for s in streams], axis=0).tolist()
        finally:
            host.close()
        for deferred in (False, True):
            d = api.Decoder(0)
            try:
                if deferred:
                    d.submit_batch_device(streams, 1)
                    info = d.finish_batch_device()
                else:
                    info = d.decode_batch_device(streams, min_intervals=1)
                assert list(info.range_max)[:3] == want_range, (deferred, list(info.range_max), want_range)
                out = torch.zeros((len(streams), h, w * 3), dtype=torch.uint8, device="cuda")
                d.reconstruct_batch_device(out.data_ptr(), h * w * 3, w * 3)
                res = out.cpu().numpy().reshape(len(streams), h, w, 3)
                for i, s in enumerate(streams):
                    assert np.array_equal(res[i], oracle.decode(s)), (i, deferred)
            finally:
                d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, "1", "2"])
@pytest.mark.parametrize("precision,progressive,fam", PROG + [(12, False, f) for f in hc.FAMILIES])
def test_prog_kernel_on_crafted_tables(dev, oracle, monkeypatch, precision, progressive, fam, lanes):
    """huffman_prog_kernel: progressive frames of 8 and 12 bits, and 12-bit sequential ones, at 1, 2 and the default number of
    lanes a wave (1 and 2: per-wave staging areas that are not a multiple of 16 bytes unless rounded up)."""
    if lanes:
        monkeypatch.setenv("MIJPEG_HUFF_LANES", lanes)
    layouts = ("p420", "p444", "pgrey") if progressive else ("420", "444", "grey")
    for kind in contents(precision, fam):
        for i, dri in enumerate((2, 1, 7)):
            data, planes, _, _ = make_case(precision, progressive, fam, kind, dri, layouts[i], seed=3)
            device_matches(dev, oracle, data, planes, precision, f"{fam} {kind} DRI {dri} lanes {lanes}")


@pytest.mark.gpu
def test_prog_kernel_eob14_runs(dev, oracle):
    data, planes = _eob14_case(dri=20000)  # (one restart interval: a lane decodes every block of a scan)
    device_matches(dev, oracle, data, planes, 8, "EOB14")


_NO_SUB = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import huffcraft as hc
from libjpeg_amd import api
from oracle import oracle as O
d = api.Decoder(0)
n = 0
for fam in ("annexk", "all_long", "prefixes9", "len16_widest"):
    for prog, dri, w, h, samp in ((False, 1, 96, 64, [(2, 2), (1, 1), (1, 1)]), (False, 0, 256, 256, [(2, 2), (1, 1), (1, 1)]),
                                  (True, 2, 48, 32, [(2, 2), (1, 1), (1, 1)])):
        dc, ac = hc.family(fam, 8, prog)
        planes = hc.content("boundaries", hc.plane_shapes(w, h, samp), 8, np.random.default_rng(n))
        data = hc.write(planes, w, h, samp, [(dc, ac)] + [(hc.chroma_variant(dc), hc.chroma_variant(ac))] * 2, dri=dri, progressive=prog)
        d.read(data, entropy="gpu")
        assert d.entropy_used == "gpu"
        assert np.array_equal(d.reconstruct(), O.decode(data)), (fam, prog, dri)
        for c in range(3):
            assert np.array_equal(d.coefficients(c).astype(np.int32), planes[c]), (fam, prog, dri, c)
        n += 1
d.close()
print("decoded", n)
"""


@pytest.mark.gpu
def test_device_decoders_without_second_level_tables(oracle):
    """MIJPEG_HUFF_NO_SUBTABLES (read once per process): every code longer than ten bits takes the canonical walk -- in all three
    device decoders.  A fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _NO_SUB.format(root=root, tests=os.path.join(root, "tests"))
    env = dict(os.environ, MIJPEG_HUFF_NO_SUBTABLES="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "decoded 12" in r.stdout

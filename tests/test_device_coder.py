"""The device entropy coder (libjpeg_amd/csrc/hencode.hip) on coefficient planes the test writes into HBM.

mijpeg_encode_coefficients_device codes planes that are already in device memory, so the coder's edge cases no longer depend on
what the forward kernels make of a picture: ZRL chains, a coefficient at position 63, full blocks, both ends of every category,
16-bit codes with 14 or 15 value bits behind them, plain streams that are mostly 0xFF, intervals of one byte, and block, interval
and chunk counts on both sides of the prefix sums' tile size.  Everything is byte equality.  The references:

  host coder       api.encode_coefficients(..., threads=1): the device stream equals it, headers included
  oracle decoder   oracle.decode_coefficients returns the crafted planes on the blocks that cover samples
  huffcraft.write  (sizes of whole MCUs) the Python symbol writer, given the tables of the device stream's own DHT segments,
                   writes the same entropy coded data: a third coder that shares no C++ with the other two
  reference binary where it is built, it decodes the device stream (one case per group)

The premises of the crafted cases (which symbols, which code lengths, which stream lengths) are asserted from the planes and
from the host coder's streams, in tests that need no device, and again where the device test uses them.

Wall times of the large prefix-sum cases are recorded in their tests' docstrings."""
import ctypes as C

import numpy as np
import pytest

import huffcraft as hc
from conftest import golden_jpeg
from libjpeg_amd import api

ERR_OVERFLOW_PARAMETER = -1028
ERR_OPERATION_UNIMPLEMENTED = -1034

LAYOUTS = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "411": [(4, 1), (1, 1), (1, 1)],
           "odd": [(2, 2), (1, 2), (2, 1)]}  # odd: hs = (2, 1, 2), vs = (2, 2, 1) of test_encoder.py
ZZ = hc.ZZ


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ helpers
def _info(w, h, samp, precision=8):
    nc = len(samp)
    return api.frame_layout(w, h, nc, [s[0] for s in samp], [s[1] for s in samp], [np.ones(64, int)], ycbcr=int(nc == 3), precision=precision)


def _flat(planes):
    return np.concatenate([np.asarray(p).reshape(-1) for p in planes]).astype(np.int16)


def _parse(data: bytes):
    """-> ({(class, slot): huffcraft.Table} of the DHT segments, restart interval, entropy coded data behind SOS)."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    i, tables, dri = 2, {}, 0
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        body = data[i + 4:i + 2 + n]
        if m == 0xC4:
            p = 0
            while p < len(body):
                counts = list(body[p + 1:p + 17])
                tables[(body[p] >> 4, body[p] & 15)] = hc.Table(counts, list(body[p + 17:p + 17 + sum(counts)]))
                p += 17 + sum(counts)
        elif m == 0xDD:
            dri = int.from_bytes(body, "big")
        elif m == 0xDA:
            return tables, dri, data[i + 2 + n:-2]
        i += 2 + n


def _unstuff(ecs: bytes):
    """-> (plain bytes, stuffed 0xFF bytes among them, RSTn markers in order)."""
    plain, ff, markers, i = bytearray(), 0, [], 0
    while i < len(ecs):
        b = ecs[i]
        if b != 0xFF:
            plain.append(b)
            i += 1
            continue
        if ecs[i + 1] == 0:
            plain.append(0xFF)
            ff += 1
        else:
            assert 0xD0 <= ecs[i + 1] <= 0xD7, hex(ecs[i + 1])
            markers.append(ecs[i + 1])
        i += 2
    return bytes(plain), ff, markers


def _covered(w, h, samp, c):
    """(rows, columns) of the blocks of component c that cover samples."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    cw, ch = -(-w * samp[c][0] // hmax), -(-h * samp[c][1] // vmax)
    return (ch + 7) // 8, (cw + 7) // 8


def _coded_symbols(planes, w, h, samp, ri):
    """What the sequential coding of the planes puts into the stream, walked in scan order in Python: -> (DC categories, AC symbols,
    zero runs between two coefficients or in front of the first).  MCU padding blocks are coded as "same DC, no AC"."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    nc = len(samp)
    cov = [_covered(w, h, samp, c) for c in range(nc)]
    dc_cats, ac_syms, runs = set(), set(), set()
    pred = [0] * nc
    for m in range(mx * my):
        if ri and m % ri == 0:
            pred = [0] * nc
        for c in range(nc):
            hs, vs = (samp[c] if nc > 1 else (1, 1))
            for by in range(vs):
                for bx in range(hs):
                    y, x = (m // mx) * vs + by, (m % mx) * hs + bx
                    if y >= cov[c][0] or x >= cov[c][1]:
                        dc_cats.add(0)
                        ac_syms.add(0)
                        continue
                    blk = planes[c][y, x]
                    dc_cats.add(int(abs(int(blk[0]) - pred[c])).bit_length())
                    pred[c] = int(blk[0])
                    r = 0
                    for k in range(1, 64):
                        v = int(blk[ZZ[k]])
                        if v == 0:
                            r += 1
                            continue
                        runs.add(r)
                        while r > 15:
                            ac_syms.add(0xF0)
                            r -= 16
                        ac_syms.add((r << 4) | int(abs(v)).bit_length())
                        r = 0
                    if r:
                        ac_syms.add(0)
    return dc_cats, ac_syms, runs


def _same(got: bytes, want: bytes, what=""):
    if got != want:
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: device stream ({len(got)} bytes) differs from the host coder's ({len(want)}) at byte {at}: "
                             f"{got[at:at + 8].hex()} / {want[at:at + 8].hex()}")


def _device_stream(dec, info, coef, ri, opt):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(coef, np.int16).reshape(-1)).cuda()
    return dec.encode_coefficients_device(info, t.data_ptr(), ri, opt)


def _stream_tables(tables, nc):
    first = [(tables[(0, 0)], tables[(1, 0)])]
    return first + [(tables[(0, 1)], tables[(1, 1)])] * (nc - 1) if nc > 1 else first


def _check_references(oracle, got, planes, w, h, samp, precision, ri, opt, what, writer=True, reference=False):
    """The references that are independent of the host coder: the oracle's decoder, huffcraft.write, the reference binary."""
    nc = len(samp)
    oi, back = oracle.decode_coefficients(got)
    assert (oi.width, oi.height, oi.precision, oi.restart_interval) == (w, h, precision, ri), what
    for c in range(nc):
        rows, cols = _covered(w, h, samp, c)
        assert np.array_equal(back[c][:rows, :cols], planes[c][:rows, :cols]), (what, c)
    tables, dri, ecs = _parse(got)
    assert dri == ri
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    if writer and w % (8 * hmax) == 0 and h % (8 * vmax) == 0:
        if precision == 8 and not opt:  # Annex K.3, from a stream Pillow wrote
            k = hc._annexk_tables()
            assert all(tables[key] == k[key] for key in tables), what
            tables = k
        third = hc.write([np.asarray(p, np.int32) for p in planes], w, h, samp, _stream_tables(tables, nc), precision, dri=ri)
        assert _parse(third)[2] == ecs, f"{what}: huffcraft.write codes other bytes with the stream's own tables"
    if reference and oracle.have_reference():
        want_px = oracle.decode(got) if precision == 8 else oracle.decode16(got)
        px, err = oracle.reference_decode_status(got)
        assert err == 0, (what, err)
        assert np.array_equal(px.reshape(want_px.shape), want_px), f"{what}: the reference binary's pixels are not the oracle's"


def _check_case(dec, oracle, planes, w, h, samp, precision, ri, opt, what, **kw):
    info = _info(w, h, samp, precision)
    coef = _flat(planes)
    assert coef.size == info.coef_count
    want = api.encode_coefficients(info, coef, ri, opt, threads=1)
    got = _device_stream(dec, info, coef, ri, opt)
    _same(got, want, what)
    _check_references(oracle, got, planes, w, h, samp, precision, ri, opt, what, **kw)
    return got


# ------------------------------------------------------------------------------------------------ 1. symbol edges
def _edge_planes(kind, w, h, samp, precision, seed):
    rng = np.random.default_rng([hc.CONTENTS.index(kind), precision, w, h, seed])
    amax = 14 if precision == 12 else 10  # what the coders take (huffcraft's decoders' limit at 12 bits is 15)
    ac_syms = {(r << 4) | s for r in range(16) for s in range(1, amax + 1)} | {0x00, 0xF0}
    return hc.content(kind, hc.plane_shapes(w, h, samp), precision, rng, ac_syms=ac_syms)


def _edge_premises(kind, planes, w, h, samp, precision, ri):
    dc_cats, ac_syms, runs = _coded_symbols(planes, w, h, samp, ri)
    dmax, amax = (15, 14) if precision == 12 else (11, 10)
    assert max(dc_cats) <= dmax and max(s & 15 for s in ac_syms) <= amax
    if kind == "runs":
        assert 16 in runs and 15 in runs and 0xF0 in ac_syms, "a run of exactly 16 zeros (ZRL, then run 0) and one of 15"
        assert any(int(p.reshape(-1, 64)[:, ZZ[63]].any()) for p in planes), "a coefficient at zig-zag 63: no EOB"
        assert any((p.reshape(-1, 64)[:, ZZ[1:]] != 0).all(axis=1).any() for p in planes), "a block with all 63 AC coefficients"
    if kind == "dc_extremes":
        assert dmax in dc_cats
    if kind == "boundaries":
        cats = {s & 15 for s in ac_syms}
        assert amax in cats and 1 in cats
        mags = {abs(int(v)) for p in planes for v in np.unique(p.reshape(-1, 64)[:, 1:])}
        assert {(1 << amax) - 1, 1 << (amax - 1)} <= mags


# every kind meets every precision and both table modes (whole MCUs: huffcraft.write takes part), the layouts and restart
# intervals going round; then every layout at a size that is not of whole MCUs with one MCU per interval
_RIS = (0, 1, 5, 1000)  # 1000: more than the MCUs of any of these frames
EDGE_CASES = []
for _i, (_kind, _prec, _opt) in enumerate((k, p, o) for k in hc.CONTENTS for p in (8, 12) for o in (False, True)):
    EDGE_CASES.append((_kind, _prec, _opt, list(LAYOUTS)[_i % 5], (64, 48), _RIS[(_i + _i // 4) % 4]))
for _i, _lay in enumerate(LAYOUTS):
    EDGE_CASES.append((hc.CONTENTS[_i % 4], (8, 12)[_i % 2], bool(_i % 3 == 0), _lay, ((75, 45), (33, 17))[_i % 2], 1))
    EDGE_CASES.append((hc.CONTENTS[(_i + 2) % 4], (12, 8)[_i % 2], bool(_i % 2), _lay, ((33, 17), (75, 45))[_i % 2], (5, 0, 1000)[_i % 3]))
_REFERENCE_CASES = {0, 3}  # (one 8-bit and one 12-bit case go through the reference binary)


def test_edge_cases_cover_what_they_claim():
    seen = set()
    for kind, prec, opt, lay, (w, h), ri in EDGE_CASES:
        _edge_premises(kind, _edge_planes(kind, w, h, LAYOUTS[lay], prec, 1), w, h, LAYOUTS[lay], prec, ri)
        seen.add((kind, prec, opt))
    assert seen == {(k, p, o) for k in hc.CONTENTS for p in (8, 12) for o in (False, True)}
    assert {(lay, ri) for _, _, _, lay, size, ri in EDGE_CASES if size != (64, 48)} >= {(lay, 1) for lay in LAYOUTS}
    assert {ri for *_, ri in EDGE_CASES} == set(_RIS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(EDGE_CASES)), ids=lambda i: "-".join(str(x) for x in EDGE_CASES[i]).replace(" ", ""))
def test_symbol_edges(dec, oracle, case):
    kind, prec, opt, lay, (w, h), ri = EDGE_CASES[case]
    samp = LAYOUTS[lay]
    planes = _edge_planes(kind, w, h, samp, prec, 1)
    _edge_premises(kind, planes, w, h, samp, prec, ri)
    _check_case(dec, oracle, planes, w, h, samp, prec, ri, opt, str(EDGE_CASES[case]), reference=case in _REFERENCE_CASES)


# ------------------------------------------------------------------------------------------------ 2. widest symbols behind 16-bit codes
WIDE_AC_SIZE = (347 * 8, 6 * 8)  # 2082 blocks, grey


def _widest_ac_planes():
    """Precision 12, grey: AC symbol counts that double from symbol to symbol -- (15, 14) once, EOB twice, (1, 1) four times, then
    (0, 14) 8 times ... (0, 1) 2^16 times -- so that Annex K.2 gives the rare symbols 16 bits; the one coefficient behind a run of
    15 is 16383: fourteen value bits behind a 16-bit code."""
    rng = np.random.default_rng(2)
    vals = []
    for s in range(14, 0, -1):
        n = 8 << (14 - s)
        mag = rng.integers(1 << (s - 1), 1 << s, n)
        mag[0], mag[-1] = 1 << (s - 1), (1 << s) - 1
        vals.append(mag * rng.choice([-1, 1], n))
    vals = rng.permutation(np.concatenate(vals))
    assert len(vals) == (1 << 17) - 8
    nb = (WIDE_AC_SIZE[0] // 8) * (WIDE_AC_SIZE[1] // 8)
    z = np.zeros((nb, 64), np.int32)  # zig-zag order
    z[0, 16] = 16383  # fifteen zeros in front, EOB behind
    z[1, 1:33] = vals[:32]  # the second EOB
    at = 32
    for b in range(2, 6):  # (1, 1): a zero and a +-1, the rest of the block full
        z[b, 2] = 1 if b % 2 else -1
        z[b, 3:] = vals[at:at + 61]
        at += 61
    z[6:, 1:] = vals[at:].reshape(nb - 6, 63)  # full blocks: no EOB
    plane = np.zeros_like(z)
    plane[:, ZZ] = z
    return [plane.reshape(WIDE_AC_SIZE[1] // 8, WIDE_AC_SIZE[0] // 8, 64)]


WIDE_DC_BLOCKS = 4179  # the sum of the counts below


def _widest_dc_planes():
    """Precision 12, grey: DC differences of category c in Fibonacci numbers of blocks (category 15 once, category 0 1597 times):
    the flattest counts for which Annex K.2 still gives the rarest of the 16 symbols the longest code there is, 16 bits.  The
    category 15 difference is 32767: fifteen value bits behind a 16-bit code."""
    rng = np.random.default_rng(3)
    counts = [1597, 987, 610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1]
    assert sum(counts) == WIDE_DC_BLOCKS
    cats = rng.permutation(np.concatenate([np.full(n, c) for c, n in enumerate(counts)]))
    dc, cur = [], 0
    for c in cats:
        mag = 0 if c == 0 else 32767 if c == 15 else int(rng.integers(1 << (c - 1), 1 << c))
        cur = cur - mag if cur > 0 else cur + mag  # (stays inside int16)
        dc.append(cur)
    plane = np.zeros((1, WIDE_DC_BLOCKS, 64), np.int32)
    plane[0, :, 0] = dc
    plane[0, ::3, ZZ[1]] = 1  # (two AC symbols, so that the AC table is not the degenerate one)
    return [plane]


def _widest_premise(stream, which):
    tables, _, _ = _parse(stream)
    if which == "ac":
        assert tables[(1, 0)].length(0xFE) == 16, "the (15, 14) symbol has a 16-bit code"
    else:
        assert tables[(0, 0)].length(15) == 16 and max(l for _, l in tables[(0, 0)].codes.values()) == 16, "DC category 15 has a 16-bit code"


def _widest_case(which):
    if which == "ac":
        return _widest_ac_planes(), WIDE_AC_SIZE
    return _widest_dc_planes(), (WIDE_DC_BLOCKS * 8, 8)


@pytest.mark.parametrize("which", ["ac", "dc"])
def test_widest_symbol_premises_with_the_host_coder(oracle, which):
    planes, (w, h) = _widest_case(which)
    dc_cats, ac_syms, _ = _coded_symbols(planes, w, h, LAYOUTS["grey"], 0)
    assert (0xFE in ac_syms) if which == "ac" else (15 in dc_cats)
    stream = api.encode_coefficients(_info(w, h, LAYOUTS["grey"], 12), _flat(planes), 0, True, threads=1)
    _widest_premise(stream, which)
    _, back = oracle.decode_coefficients(stream)
    assert np.array_equal(back[0], planes[0])


@pytest.mark.gpu
@pytest.mark.parametrize("which,ri", [("ac", 0), ("ac", 1), ("dc", 0), ("dc", 7)])
def test_widest_symbol_behind_a_16_bit_code(dec, oracle, which, ri):
    planes, (w, h) = _widest_case(which)
    # (huffcraft.write takes a second per thousand full blocks: it joins in for the DC planes only)
    got = _check_case(dec, oracle, planes, w, h, LAYOUTS["grey"], 12, ri, True, f"widest {which} ri {ri}", writer=which == "dc", reference=ri == 0)
    if ri == 0:  # (with restart intervals the DC differences, and so the counts, are others)
        _widest_premise(got, which)


# ------------------------------------------------------------------------------------------------ 3. 0xFF flood
# (blocks, how many of the first DC values are set, value; plain bytes): found on the CPU with the host coder, asserted below.
# Every AC coefficient is 1023: the code of (0, 10) is 0xFF83 with ten one-bits behind it, 21 ones and 5 zeros over and over.
FLOOD_CASES = {  # (ri, plain bytes mod 64) -> (blocks, first DCs set, their value, plain bytes)
    (0, 1): (5, 0, 0, 1025), (0, 63): (9, 6, 100, 1855), (0, 0): (14, 6, 100, 2880),
    (1, 1): (5, 0, 0, 1025), (1, 63): (9, 5, 100, 1855), (1, 0): (14, 5, 100, 2880),
}
# The flood itself always ends on 0xFF (ten one-bits, then one-bit padding).  The seeded case has random DC values and four random
# coefficients at the end of its last block, so whether its last byte is a stuffed 0xFF depends on the seed: 11 is the first of
# 0..59 for which the host coder's stream ends so with and without restart markers (1 in 20 do; asserted where it is used)
FLOOD_SEED = 11


def _flood_planes(n, dc):
    plane = np.full((1, n, 64), 1023, np.int32)
    plane[0, :, 0] = dc
    return [plane]


def _flood_case(ri, rem):
    n, k, v, plain = FLOOD_CASES[(ri, rem)]
    dc = np.zeros(n, int)
    dc[:k] = v if ri else v * np.where(np.arange(k) % 2 == 0, 1, -1)
    return _flood_planes(n, dc), n, plain


def _flood_seeded():
    rng = np.random.default_rng(FLOOD_SEED)
    n = int(rng.integers(3, 20))
    planes = _flood_planes(n, rng.integers(-1000, 1000, n))
    planes[0][0, -1, ZZ[60:]] = rng.integers(1, 1023, 4) * rng.choice([-1, 1], 4)
    return planes, n


def _flood_premise(stream, plain_bytes=None):
    plain, ff, _ = _unstuff(_parse(stream)[2])
    assert ff >= 0.4 * len(plain), (ff, len(plain))
    assert plain_bytes is None or len(plain) == plain_bytes
    assert stream[-4:] == b"\xff\x00\xff\xd9"  # the stream ends on a stuffed 0xFF (the pure flood always does, see FLOOD_SEED)


def test_flood_premises_with_the_host_coder():
    for (ri, rem) in FLOOD_CASES:
        planes, n, plain = _flood_case(ri, rem)
        assert plain % 64 == rem
        _flood_premise(api.encode_coefficients(_info(8 * n, 8, LAYOUTS["grey"]), _flat(planes), ri, False, threads=1), plain)
    planes, n = _flood_seeded()
    for ri in (0, 1):
        _flood_premise(api.encode_coefficients(_info(8 * n, 8, LAYOUTS["grey"]), _flat(planes), ri, False, threads=1))


@pytest.mark.gpu
@pytest.mark.parametrize("ri,rem", sorted(FLOOD_CASES))
def test_ff_flood_around_the_stuffing_chunk(dec, oracle, ri, rem):
    planes, n, plain = _flood_case(ri, rem)
    got = _check_case(dec, oracle, planes, 8 * n, 8, LAYOUTS["grey"], 8, ri, False, f"flood ri {ri} plain {plain}", reference=rem == 0)
    _flood_premise(got, plain)


@pytest.mark.gpu
@pytest.mark.parametrize("ri", [0, 1])
def test_ff_flood_ends_on_a_stuffed_byte(dec, oracle, ri):
    planes, n = _flood_seeded()
    _flood_premise(_check_case(dec, oracle, planes, 8 * n, 8, LAYOUTS["grey"], 8, ri, False, f"flood seed {FLOOD_SEED} ri {ri}"))


# ------------------------------------------------------------------------------------------------ 4. one-byte intervals
ONE_BYTE_BLOCKS = 1111


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [False, True])
def test_one_byte_intervals(dec, oracle, opt):
    """All-zero planes, one MCU per interval: every interval is one byte, so a 64-byte stuffing chunk carries 64 interval starts and
    the RSTn number wraps inside and across chunks.  Standard tables: DC category 0 is 00, EOB 1010, two one-bits of padding;
    optimised: both tables have one symbol with the code 0."""
    n = ONE_BYTE_BLOCKS
    planes = [np.zeros((1, n, 64), np.int32)]
    got = _check_case(dec, oracle, planes, 8 * n, 8, LAYOUTS["grey"], 8, 1, opt, f"one-byte intervals, optimised {opt}", writer=True, reference=not opt)
    byte = 0x3F if opt else 0x2B
    want = bytearray([byte])
    for i in range(1, n):
        want += bytes([0xFF, 0xD0 + ((i - 1) & 7), byte])
    assert _parse(got)[2] == bytes(want)


# ------------------------------------------------------------------------------------------------ 5. prefix-sum tile edges
def _tile_edge_planes(w, h):
    shapes = hc.plane_shapes(w, h, LAYOUTS["grey"])
    planes = hc.content("sparse", shapes, 8, np.random.default_rng([5, w, h]))
    flat = planes[0].reshape(-1, 64)
    for b in (1022, 1023, 1024, 1025, 2047, 2048):  # distinct non-zero blocks on both sides of the tile edges
        if b < len(flat):
            flat[b, ZZ[1]], flat[b, ZZ[2 + b % 60]] = b % 1000 + 1, -(b % 37) - 1
    return planes


@pytest.mark.gpu
@pytest.mark.parametrize("ri", [1, 0])
@pytest.mark.parametrize("w,h", [(8184, 8), (8192, 8), (8200, 8), (8, 16392)])
def test_prefix_sum_tile_edges(dec, oracle, w, h, ri):
    """1023, 1024, 1025 and 2049 blocks: one tile of the prefix sums with and without room for the total, two tiles, three; with
    one MCU per interval the scan over the intervals crosses the same edges."""
    planes = _tile_edge_planes(w, h)
    assert planes[0].shape[0] * planes[0].shape[1] == w * h // 64
    _check_case(dec, oracle, planes, w, h, LAYOUTS["grey"], 8, ri, False, f"{w} x {h} ri {ri}", writer=(w, ri) == (8192, 1), reference=(w, ri) == (8200, 1))


def _marked_blocks(nb):
    """A few dozen block indices at and around the multiples of 1024 that matter to a scan in tiles of 1024, and the last block."""
    at = {0, nb - 1, nb - 2}
    for m in (1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 511, 512, 767, 768, 1021, 1022, 1023, 1024, 1025):
        for d in (-1, 0, 1):
            if 0 <= m * 1024 + d < nb:
                at.add(m * 1024 + d)
    return sorted(at)


def _marked_values(n, nb):
    rng = np.random.default_rng(nb)
    vals = np.zeros((n, 64), np.int16)
    vals[:, 0] = rng.integers(-1000, 1000, n)
    for i in range(n):
        vals[i, ZZ[1 + i % 63]] = (i + 1) * (-1) ** i
        vals[i, ZZ[63 - i % 7]] = 1 + i % 5
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("bw,bh,ri", [(1023, 1023, 0), (1023, 1024, 0), (1023, 1024, 1)], ids=["3-launches", "5-launches", "5-launches-ri1"])
def test_prefix_sums_on_both_sides_of_the_five_launch_threshold(dec, bw, bh, ri):
    """exclusive_scan_u32 over 1023 x 1023 blocks takes three launches, over 1023 x 1024 five (and with one MCU per interval the
    scan over the intervals does too).  Zero planes (134 MB) built on the device with a few dozen non-zero blocks scattered at and
    around multiples of 1024 and at the end; the expected stream is the host coder's on the same array.
    Measured on an MI355X (printed below; pytest's duration of the whole test call, which builds the planes, copies them to the
    host, runs the host coder and compares / of that the device call alone):
      1023 x 1023, no restart markers   0.10 s / 0.002 s
      1023 x 1024, no restart markers   0.06 s / 0.001 s
      1023 x 1024, one MCU per interval 0.06 s / 0.001 s"""
    import time

    import torch

    nb = bw * bh
    info = _info(8 * bw, 8 * bh, LAYOUTS["grey"])
    at = _marked_blocks(nb)
    assert 36 <= len(at) <= 64
    coef = torch.zeros((nb, 64), dtype=torch.int16, device="cuda")
    coef.index_copy_(0, torch.tensor(at, device="cuda"), torch.from_numpy(_marked_values(len(at), nb)).cuda())
    host = coef.cpu().numpy().reshape(-1)
    assert np.count_nonzero(host.reshape(nb, 64).any(axis=1)) == len(at)
    t0 = time.perf_counter()
    want = api.encode_coefficients(info, host, ri, False, threads=1)
    t1 = time.perf_counter()
    got = dec.encode_coefficients_device(info, coef.data_ptr(), ri, False)
    t2 = time.perf_counter()
    print(f"{bw} x {bh} blocks, ri {ri}: host coder {t1 - t0:.3f} s, device call {t2 - t1:.3f} s")
    _same(got, want, f"{bw} x {bh} blocks, ri {ri}")


@pytest.mark.gpu
def test_second_level_offsets_of_the_prefix_sums(dec):
    """At 1023 x 1024 elements the second level of the five-launch path has two tiles, but the second tile's offset only feeds an
    entry nobody reads (the total of the tile sums): a second level that dropped its offsets would go unnoticed there.  It shows
    from 2^20 + 1 elements on, where tile sums 1024 and up lie in the second tile.  Blocks and intervals cannot be taken there
    and a wrong scan be survivable -- positions that are too small make the emit pass write where the plain stream was never
    allocated -- but the scan over the stuffing chunks can: its results only place bytes inside the output arena.  So: 1023 x 1024
    blocks whose first 24 AC coefficients are 1023 (the 0xFF flood of above), 79 plain bytes a block, 1.29 million chunks with
    0xFF counts that are not zero.  Measured on an MI355X (whole test call / the device call alone): 0.44 s / 0.039 s."""
    import time

    import torch

    bw, bh = 1023, 1024
    nb = bw * bh
    info = _info(8 * bw, 8 * bh, LAYOUTS["grey"])
    coef = torch.zeros((nb, 64), dtype=torch.int16, device="cuda")
    coef[:, torch.from_numpy(ZZ[1:25]).cuda()] = 1023
    at = _marked_blocks(nb)
    coef.index_copy_(0, torch.tensor(at, device="cuda"), torch.from_numpy(_marked_values(len(at), nb)).cuda())
    host = coef.cpu().numpy().reshape(-1)
    want = api.encode_coefficients(info, host, 0, False, threads=1)
    plain_bytes = len(want) - want.count(b"\xff\x00")  # (headers and EOI: a few hundred bytes, no stuffing in them)
    assert plain_bytes > 64 * ((1 << 20) + 4096) and want.count(b"\xff\x00") > plain_bytes // 4
    t0 = time.perf_counter()
    got = dec.encode_coefficients_device(info, coef.data_ptr(), 0, False)
    print(f"dense 1023 x 1024 blocks: device call {time.perf_counter() - t0:.3f} s")
    _same(got, want, "dense 1023 x 1024 blocks")


# ------------------------------------------------------------------------------------------------ 6. refusals
def _refusal_cases(precision):
    """(name, planes of a 6 x 4 block grey frame with ONE value beyond the limit, the same planes with the largest legal value)."""
    w, h = 48, 32
    base = _edge_planes("sparse", w, h, LAYOUTS["grey"], precision, 6)[0]
    base[1, 2] = 0  # the block the cases write into
    base[1, 1, 0] = base[1, 2, 0] = base[1, 3, 0] = 0
    ac, dc = (1024, 2048) if precision == 8 else (16384, 65535)
    out = []

    def case(name, edit_bad, edit_ok):
        bad, ok = base.copy(), base.copy()
        edit_bad(bad[1, 2], bad[1, 3])
        edit_ok(ok[1, 2], ok[1, 3])
        out.append((name, [bad], [ok]))

    def put(k, v):
        def f(blk, _next):
            blk[ZZ[k]] = v
        return f

    def step(a, b):
        def f(blk, nxt):
            blk[0], nxt[0] = a, b
        return f

    if precision == 8:
        case("AC 1024", put(5, ac), put(5, ac - 1))
        case("AC -1024", put(5, -ac), put(5, -(ac - 1)))
        case("DC step 2048", step(-1024, 1024), step(-1024, 1023))
    else:
        case("AC 16384", put(5, ac), put(5, ac - 1))
        case("AC -32768 behind a run of 15", put(16, -32768), put(16, -16383))
        case("DC -32768 next to 32767", step(-32768, 32767), step(-16384, 16383))
    return w, h, out


def _host_refusal(info, coef, ri, opt):
    with pytest.raises(api.MijpegError) as e:
        api.encode_coefficients(info, coef, ri, opt, threads=1)
    return e.value.code


@pytest.mark.parametrize("precision", [8, 12])
def test_refusal_cases_are_what_the_host_coder_refuses(precision):
    w, h, cases = _refusal_cases(precision)
    info = _info(w, h, LAYOUTS["grey"], precision)
    for name, bad, ok in cases:
        for opt in (False, True):
            assert _host_refusal(info, _flat(bad), 0, opt) == ERR_OVERFLOW_PARAMETER, name
            assert api.encode_coefficients(info, _flat(ok), 0, opt, threads=1)[:2] == b"\xff\xd8", name
        assert int(np.count_nonzero(bad[0] != ok[0])) <= 2, name


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [False, True])
@pytest.mark.parametrize("precision", [8, 12])
def test_values_beyond_the_precision_are_refused_like_the_host_coder_does(dec, oracle, precision, opt):
    w, h, cases = _refusal_cases(precision)
    info = _info(w, h, LAYOUTS["grey"], precision)
    for name, bad, ok in cases:
        for ri in (0, 2):
            code = _host_refusal(info, _flat(bad), ri, opt)
            with pytest.raises(api.MijpegError) as e:
                _device_stream(dec, info, _flat(bad), ri, opt)
            assert e.value.code == code == ERR_OVERFLOW_PARAMETER, (name, ri)
        # the largest legal values beside them are coded and come back
        _check_case(dec, oracle, ok, w, h, LAYOUTS["grey"], precision, 0, opt, f"{name}: legal neighbour", reference=name == cases[0][0])
    # the object serves the next call as usual
    kind, prec, o, lay, (cw, ch), ri = EDGE_CASES[1]
    _check_case(dec, oracle, _edge_planes(kind, cw, ch, LAYOUTS[lay], prec, 1), cw, ch, LAYOUTS[lay], prec, ri, o, "after the refusals")


# ------------------------------------------------------------------------------------------------ 7. transcoding
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pil_200x120_420_dri8", "ref_33x17_420_dri1", "enc12/420_272x144_z4"])
def test_transcoding_without_leaving_hbm(dec, oracle, name):
    """A stream entropy-decoded on the device is coded again from mijpeg_device_coefficients(), with its own restart interval and
    with one MCU per interval, with the standard (8-bit) and with optimised tables: the host coder's stream of the downloaded
    planes, and the golden's coefficients back from the oracle."""
    data = golden_jpeg(name)
    info = dec.read(data, entropy="gpu")
    assert dec.entropy_used == "gpu" and not info.coef_wide and dec.device_coefficients()
    nc = info.components
    samp = [(info.hsamp[c], info.vsamp[c]) for c in range(nc)]
    assert info.restart_interval > 0 and (name != "pil_200x120_420_dri8" or samp == LAYOUTS["420"])
    assert info.precision == (12 if name.startswith("enc12/") else 8)
    planes = [dec.coefficients(c) for c in range(nc)]
    coef = _flat(planes)
    _, golden = oracle.decode_coefficients(data)
    for ri in (info.restart_interval, 1):
        for opt in (False, True):
            got = dec.encode_coefficients_device(info, dec.device_coefficients(), ri, opt)
            _same(got, api.encode_coefficients(info, coef, ri, opt, threads=1), f"{name} ri {ri} optimised {opt}")
            oi, back = oracle.decode_coefficients(got)
            assert (oi.width, oi.height, oi.precision, oi.restart_interval) == (info.width, info.height, info.precision, ri)
            for c in range(nc):
                rows, cols = _covered(info.width, info.height, samp, c)
                assert np.array_equal(back[c][:rows, :cols], golden[c][:rows, :cols]), (name, ri, opt, c)
    if oracle.have_reference() and info.precision == 8:
        assert np.array_equal(oracle.reference_decode(got), oracle.decode(data))


# ------------------------------------------------------------------------------------------------ argument checks (no device)
def test_argument_checks_come_before_any_device():
    L = api.lib()
    fn = L.mijpeg_encode_coefficients_device
    fn.argtypes = [C.c_void_p, C.POINTER(api.MijpegInfo), C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    d = api.Decoder(None)  # an object without a device: whatever gets past the checks ends in NOT_AVAILABLE
    p, n = C.c_void_p(), C.c_size_t()
    coef = 4096  # (never read)

    def call(info, coef_dev=coef, ri=0, handle=None, out=True):
        return fn(d._h if handle is None else handle, C.byref(info) if info is not None else None, coef_dev, ri, 0,
                  C.byref(p) if out else None, C.byref(n) if out else None)

    def copy_of(f):
        g = api.MijpegInfo()
        C.memmove(C.byref(g), C.byref(f), C.sizeof(api.MijpegInfo))
        return g

    good = _info(64, 48, LAYOUTS["420"])
    host = api.encode_coefficients
    # null pointers, restart interval: what the host twin answers
    assert call(good, handle=C.c_void_p()) == api.ERR_INVALID_PARAMETER
    assert call(None) == api.ERR_INVALID_PARAMETER
    assert call(good, coef_dev=None) == api.ERR_INVALID_PARAMETER
    assert call(good, out=False) == api.ERR_INVALID_PARAMETER
    for ri in (-1, 65536):
        assert call(good, ri=ri) == api.ERR_INVALID_PARAMETER
        with pytest.raises(api.MijpegError) as e:
            host(good, np.zeros(int(good.coef_count), np.int16), ri)
        assert e.value.code == api.ERR_INVALID_PARAMETER
    # precision, component count
    for field, value in (("precision", 10), ("precision", 16), ("components", 2), ("components", 4)):
        bad = copy_of(good)
        setattr(bad, field, value)
        assert call(bad) == ERR_OPERATION_UNIMPLEMENTED, (field, value)
        with pytest.raises(api.MijpegError) as e:
            host(bad, np.zeros(int(good.coef_count), np.int16))
        assert e.value.code == ERR_OPERATION_UNIMPLEMENTED
    # more than 64 blocks per MCU, 2^30 blocks or more: what the per-frame coder answers
    bad = copy_of(good)
    bad.hsamp[0] = bad.vsamp[0] = 8
    assert call(bad) == api.ERR_NOT_AVAILABLE
    with pytest.raises(api.MijpegError) as e:
        d._check(call(bad))
    assert "blocks per MCU" in str(e.value)
    bad = copy_of(good)
    bad.mcus_x, bad.mcus_y = 16384, 10923  # x 6 blocks: 2^30 and a few
    assert call(bad) == api.ERR_NOT_AVAILABLE
    with pytest.raises(api.MijpegError) as e:
        d._check(call(bad))
    assert "too large" in str(e.value)
    bad.mcus_y = 10922  # just below: through the checks, to the missing device
    assert bad.mcus_x * bad.mcus_y * 6 < 1 << 30
    with pytest.raises(api.MijpegError) as e:
        d._check(call(bad))
    assert e.value.code == api.ERR_NOT_AVAILABLE and "without a device" in str(e.value)
    # the edge itself, on a grey frame (one block per MCU): 2^30 - 1025 blocks pass, 2^30 - 1024 are refused
    grey = _info(64, 48, LAYOUTS["grey"])
    for mx, my, refused in ((6619, 162221, False), (1024, (1 << 20) - 1, True)):
        edge = copy_of(grey)
        edge.mcus_x, edge.mcus_y = mx, my
        assert mx * my == (1 << 30) - 1025 + int(refused)
        with pytest.raises(api.MijpegError) as e:
            d._check(call(edge))
        assert e.value.code == api.ERR_NOT_AVAILABLE and ("too large" if refused else "without a device") in str(e.value), (mx, my, str(e.value))
    # an info that was never laid out: refused before anything divides by its subsampling factors
    assert call(api.MijpegInfo(precision=8, components=1)) == api.ERR_INVALID_PARAMETER
    bad = copy_of(good)
    bad.suby[1] = 0
    assert call(bad) == api.ERR_INVALID_PARAMETER
    bad = copy_of(good)
    bad.mcus_x = bad.mcus_y = 65535  # (the product does not fit an int)
    assert call(bad) == api.ERR_INVALID_PARAMETER
    # a valid call on an object without a device, through the binding
    with pytest.raises(api.MijpegError) as e:
        d.encode_coefficients_device(good, coef)
    assert e.value.code == api.ERR_NOT_AVAILABLE and "without a device" in str(e.value)
    assert p.value is None and n.value == 0
    d.close()

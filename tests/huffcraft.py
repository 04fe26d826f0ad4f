"""JPEG streams with Huffman tables and coefficients chosen by the test (test infrastructure).

The entropy decoders are otherwise only fed what Pillow or the reference encoder wrote: Annex K tables or tables optimised
for natural content.  Here a test picks the code lengths (`Table`, the named `family()` recipes) and the quantised
coefficients (`content()`), and `write()` puts exactly those coefficients into a baseline / extended sequential (SOF0 /
SOF1) or progressive (SOF2, G.1.2) stream, symbol by symbol.  It is not an encoder: symbol order is whatever the
coefficients dictate, code lengths are whatever the recipe chose.  Byte stuffing and the bit writer are damage._BitWriter's.

Coefficient planes are int32 (blocks_h, blocks_w, 64) in natural order, one per component, laid out like the oracle's
decode_coefficients (MCU grid times sampling factors)."""
from __future__ import annotations

import heapq

import numpy as np

from damage import _BitWriter

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
               42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def max_categories(precision: int):
    """(largest DC category, largest AC category) the precision allows: 8-bit 11 / 10, 12-bit 15 / 15 (AC coefficients of a
    12-bit frame reach 2^15 - 1 in the int16 store; the decoders accept category 15 behind an AC code)."""
    return (11, 10) if precision == 8 else (15, 15)


# ---------------------------------------------------------------------------------------------------------------------------
# Huffman tables
# ---------------------------------------------------------------------------------------------------------------------------
class Table:
    """A DHT table: counts[16] (codes of 1..16 bits) and the values in code order.  Checked to be legal: at most 256 values,
    no length over-subscribed, and the all-ones code of the longest length unused (C.2: codes of all ones are reserved)."""

    def __init__(self, counts, values):
        self.counts = [int(c) for c in counts]
        self.values = [int(v) for v in values]
        assert len(self.counts) == 16 and sum(self.counts) == len(self.values) <= 256, (self.counts, len(self.values))
        assert len(set(self.values)) == len(self.values), "a symbol listed twice"
        self.codes = {}
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(self.counts[length - 1]):
                assert code < (1 << length) - 1 or k < len(self.values) - 1, "over-subscribed or the all-ones code used"
                assert code < (1 << length), "over-subscribed"
                self.codes[self.values[k]] = (code, length)
                code += 1
                k += 1
            code <<= 1
        last = self.codes[self.values[-1]]
        assert last[0] != (1 << last[1]) - 1, "the all-ones code used"

    @classmethod
    def from_lengths(cls, lengths: dict, order=None):
        """{symbol: length} -> Table; codes of one length go to the symbols in `order` (default: ascending symbol)."""
        order = list(order) if order is not None else sorted(lengths)
        rank = {s: i for i, s in enumerate(order)}
        syms = sorted(lengths, key=lambda s: (lengths[s], rank[s]))
        counts = [0] * 16
        for s in syms:
            counts[lengths[s] - 1] += 1
        return cls(counts, syms)

    def length(self, sym: int) -> int:
        return self.codes[sym][1]

    def dht(self, tc: int, th: int) -> bytes:
        return bytes([(tc << 4) | th]) + bytes(self.counts) + bytes(self.values)

    def __eq__(self, o):
        return isinstance(o, Table) and self.counts == o.counts and self.values == o.values

    def __hash__(self):
        return hash((tuple(self.counts), tuple(self.values)))


def kraft(lengths) -> float:
    return sum(2.0 ** -l for l in lengths)


def huffman_lengths(weights: dict, maxlen: int = 16) -> dict:
    """Code lengths of a Huffman code for {symbol: weight}, limited to `maxlen` bits and leaving the all-ones code free
    (K.2, Figures K.1-K.3: one reserved code point of weight zero, lengths cut by the adjust_BITS step)."""
    syms = sorted(weights, key=lambda s: (-weights[s], s))
    heap = [(float(weights[s]), i, [i]) for i, s in enumerate(syms)] + [(0.0, len(syms), [len(syms)])]  # + the reserved point
    heapq.heapify(heap)
    size = [0] * (len(syms) + 1)
    tie = len(syms) + 1
    while len(heap) > 1:
        w1, _, a = heapq.heappop(heap)
        w2, _, b = heapq.heappop(heap)
        for i in a + b:
            size[i] += 1
        heapq.heappush(heap, (w1 + w2, tie, a + b))
        tie += 1
    bits = [0] * 64
    for s in size:
        bits[s] += 1
    for i in range(63, maxlen, -1):  # K.3 Adjust_BITS
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = maxlen
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved code point
    out, k = {}, 0
    for length in range(1, maxlen + 1):
        for _ in range(bits[length]):
            out[syms[k]] = length
            k += 1
    return out


def dc_symbols(precision: int):
    return list(range(max_categories(precision)[0] + 1))


def ac_symbols(precision: int, progressive: bool):
    """Rank order (what sparse content uses most first): EOB, small categories at short runs, ZRL, ...; progressive scans add
    the EOB runs EOB1..EOB14 (r << 4, r = 1..14)."""
    smax = max_categories(precision)[1]
    rs = sorted(((r << 4) | s for r in range(16) for s in range(1, smax + 1)), key=lambda x: ((x & 15) + (x >> 4), x))
    out = [0x00] + rs[:12] + [0xF0] + rs[12:]
    if progressive:
        out[1:1] = [r << 4 for r in range(1, 15)]
    return out


def widest(precision: int, progressive: bool):
    """The symbols with the most value bits behind them: DC / AC of the largest category (12-bit: AC 14 and 15), EOB14."""
    dmax, amax = max_categories(precision)
    ac_s = {amax} if precision == 8 else {amax - 1, amax}
    ac = [(r << 4) | s for r in range(16) for s in sorted(ac_s)] + ([0xE0] if progressive else [])
    return [dmax], ac


def _geometric(syms, decay: float):
    return {s: decay ** i for i, s in enumerate(syms)}


def _annexk_tables():
    import craft  # Annex K tables (from a stream Pillow wrote)

    dht = craft._annex_k()[0]
    out, q = {}, 0
    while q < len(dht):
        ln = (dht[q + 2] << 8) | dht[q + 3]
        p, end = q + 4, q + 2 + ln
        while p < end:
            tc, th = dht[p] >> 4, dht[p] & 15
            counts = list(dht[p + 1:p + 17])
            vals = list(dht[p + 17:p + 17 + sum(counts)])
            out[(tc, th)] = Table(counts, vals)
            p += 17 + sum(counts)
        q = end
    return out


FAMILIES = ("annexk", "prefixes8", "prefixes9", "all_long", "len16_widest", "straddle10", "fixed8", "degenerate", "incomplete_with_unused")
PROGRESSIVE_FAMILIES = ("annexk", "prefixes9", "all_long", "len16_widest", "straddle10", "fixed8")  # (the others: sequential scans only)


def _prefixes(syms, n_prefixes: int, frequent: int):
    """Long codes (11..16 bits) over exactly `n_prefixes` ten-bit prefixes, the `frequent` first symbols of the rank order
    on the longest codes (canonical order puts them under the last prefix); two 11-bit codes fill each of the others, the
    rest have 5..10 bits."""
    lens = {}
    tail = [12, 13, 14, 15, 16, 16][:frequent]
    for s, l in zip(syms, tail):
        lens[s] = l
    pairs = syms[len(tail):len(tail) + 2 * (n_prefixes - 1)]
    for s in pairs:
        lens[s] = 11
    for i, s in enumerate(syms[len(tail) + len(pairs):]):
        lens[s] = min(10, 5 + i // 8)
    return lens


def long_prefixes(t: Table):
    """The distinct ten-bit prefixes of the codes longer than ten bits, in code order."""
    seen = []
    for code, length in sorted(t.codes.values(), key=lambda x: (x[1], x[0])):
        if length > 10 and (code >> (length - 10)) not in seen:
            seen.append(code >> (length - 10))
    return seen


def family(name: str, precision: int = 8, progressive: bool = False):
    """(DC table, AC table) of a named recipe for the symbols a frame of this precision / scan type can use."""
    dsyms, asyms = dc_symbols(precision), ac_symbols(precision, progressive)
    if name == "annexk":
        if precision == 8 and not progressive:
            k = _annexk_tables()
            return k[(0, 0)], k[(1, 0)]
        # (Annex K has no codes for the 12-bit categories nor for EOB runs: a Huffman code of the same rank order)
        return (Table.from_lengths(huffman_lengths(_geometric(dsyms, 0.7))),
                Table.from_lengths(huffman_lengths(_geometric(asyms, 0.93))))
    if name in ("prefixes8", "prefixes9"):
        n = int(name[-1])
        dc = Table.from_lengths(_prefixes(dsyms, 1, 3), order=dsyms)
        ac = Table.from_lengths(_prefixes(asyms, n, 6), order=asyms)
        assert len(long_prefixes(ac)) == n
        return dc, ac
    if name == "all_long":
        dc = {s: 11 + i % 6 for i, s in enumerate(dsyms)}
        ac = {s: 11 + i if i < 6 else 13 + i % 4 for i, s in enumerate(asyms)}
        return Table.from_lengths(dc, dsyms), Table.from_lengths(ac, asyms)
    if name == "len16_widest":
        wd, wa = widest(precision, progressive)
        out = []
        for syms, wide, decay in ((dsyms, wd, 0.7), (asyms, wa, 0.93)):
            lens = huffman_lengths(_geometric([s for s in syms if s not in wide], decay), maxlen=15)
            # room at 16 bits for the widest: lengthen the longest 15-bit codes until they fit (two 16-bit codes per 15-bit one)
            need = len(wide) + 1
            for s in sorted(lens, key=lambda s: (lens[s], syms.index(s)), reverse=True):
                if kraft(lens.values()) + need * 2.0 ** -16 <= 1.0:
                    break
                if lens[s] == 15:
                    lens[s] = 16
            for s in wide:
                lens[s] = 16
            out.append(Table.from_lengths(lens, syms))
        assert all(out[0].length(s) == 16 for s in wd) and all(out[1].length(s) == 16 for s in wa)
        return tuple(out)
    if name == "straddle10":
        # the last 10-bit code and the first 11-bit code: DC category 0 / 1 and AC (0, 1) / EOB -- what sparse content
        # alternates between
        out = []
        for syms, a, b, decay in ((dsyms, 0, 1, 0.7), (asyms, 0x01, 0x00, 0.93)):
            lens = huffman_lengths(_geometric(syms, decay), maxlen=16)
            assert lens[a] <= 10 and lens[b] <= 11  # (so that moving them there keeps the code legal)
            lens[a], lens[b] = 10, 11
            order = [s for s in syms if s not in (a, b)]
            t = Table.from_lengths(lens, [b] + order + [a])
            ca, cb = t.codes[a], t.codes[b]
            assert ca[1] == 10 and cb[1] == 11 and cb[0] == (ca[0] + 1) << 1, (ca, cb)
            out.append(t)
        return tuple(out)
    if name == "fixed8":
        dc = {s: 4 for s in dsyms}
        ac = {s: 8 for s in asyms}
        if len(dsyms) == 16:  # (the all-ones code stays free)
            dc[dsyms[-1]] = 5
        if len(asyms) == 256:
            ac[asyms[-1]] = 9
        return Table.from_lengths(dc, dsyms), Table.from_lengths(ac, asyms)
    if name == "degenerate":
        assert not progressive
        # DC: one symbol, category 0, on a 1-bit code; AC: EOB and (0, 1)
        return Table([1] + [0] * 15, [0]), Table([1, 1] + [0] * 14, [0x00, 0x01])
    if name == "incomplete_with_unused":
        assert not progressive
        # symbols that are defined but mean nothing (AC s = 0 with runs 1..14, 8-bit DC categories 12..15) on the SHORT codes,
        # the real ones behind them, and the top half of the code space unused
        junk_dc = [s for s in range(12, 16) if s not in dsyms]
        junk_ac = [r << 4 for r in range(1, 15)]
        out = []
        for syms, junk in ((dsyms, junk_dc), (asyms, junk_ac)):
            lens = huffman_lengths(_geometric(junk + syms, 0.9), maxlen=15)
            lens = {s: l + 1 for s, l in lens.items()}  # Kraft <= 1/2
            out.append(Table.from_lengths(lens, junk + syms))
            assert kraft(lens.values()) <= 0.5
        return tuple(out)
    raise ValueError(name)


def chroma_variant(t: Table) -> Table:
    """The same code lengths with the symbols of each length in reverse order: another code of the same shape.  A
    self-synchronising walk needs luma and chroma codes that differ -- with one code for all components a parse that starts
    at the wrong block of an MCU decodes as well as the right one, and only the start of the scan can tell them apart."""
    return Table.from_lengths({s: l for s, (_, l) in t.codes.items()}, order=t.values[::-1])


def uses(dc: Table, ac: Table):
    """(DC categories, AC (run, size) symbols) content may use with these tables."""
    return set(dc.codes), set(ac.codes)


# ---------------------------------------------------------------------------------------------------------------------------
# coefficient content
# ---------------------------------------------------------------------------------------------------------------------------
CONTENTS = ("sparse", "boundaries", "runs", "dc_extremes")


def content(kind: str, shapes, precision: int, rng: np.random.Generator, dc_cats=None, ac_syms=None, **history):
    """One int32 plane (bh, bw, 64) per shape.  dc_cats / ac_syms: what the tables can code (None: everything); content is
    shaped to stay inside it.  DC values stay inside int16 (the predictor with them).  kind "history" (not in CONTENTS: it is
    made for a scan script) takes history_content's keywords."""
    if kind == "history":
        return history_content(shapes, precision, rng, dc_cats, ac_syms, **history)
    assert not history
    dmax, amax = max_categories(precision)
    dc_cats = set(range(dmax + 1)) if dc_cats is None else dc_cats
    if ac_syms is not None:  # (no AC coefficient of a category the tables have no symbol for; amax only shapes `boundaries`)
        amax = min(amax, max(s & 15 for s in ac_syms))
    planes = [np.zeros(s + (64,), np.int32) for s in shapes]
    if dc_cats == {0}:  # degenerate: no DC difference, AC (0, 1) only (EOB or a +-1 at each next position)
        for p in planes:
            flat = p.reshape(-1, 64)
            for b in range(len(flat)):
                n = int(rng.integers(0, 4)) if b % 5 else 63
                flat[b, ZZ[1:1 + n]] = rng.choice([-1, 1], n)
        return planes
    lo_dc, hi_dc = -(1 << (dmax - 1)), (1 << (dmax - 1)) - 1  # DC differences up to +-(2^dmax - 1)
    for p in planes:
        flat = p.reshape(-1, 64)
        nb = len(flat)
        if kind == "dc_extremes":
            # alternate between the ends: every difference is the largest of its category, both signs; a few small steps between
            flat[:, 0] = np.where(np.arange(nb) % 2 == 0, lo_dc, hi_dc)
            flat[3::7, 0] = 0
            flat[1::4, ZZ[1]] = rng.choice([-1, 1], len(flat[1::4]))
        else:
            flat[:, 0] = np.clip(np.cumsum(rng.integers(-40, 41, nb)), -1000, 1000)
        if kind == "sparse":
            for b in range(nb):
                k = 1
                while k < 64 and rng.random() < 0.55:
                    k += int(rng.integers(0, 6))
                    if k > 63:
                        break
                    flat[b, ZZ[k]] = int(rng.choice([-1, 1])) * int(rng.integers(1, 40))
                    k += 1
        elif kind == "boundaries":
            # every AC category's smallest and largest magnitude, both signs, at positions that move from block to block
            vals = [v for c in range(1, amax + 1) for v in ((1 << (c - 1)), (1 << c) - 1)]
            vals = [sgn * v for v in vals for sgn in (1, -1)]
            i = 0
            for b in range(nb):
                for k in rng.choice(np.arange(1, 64), int(rng.integers(1, 9)), replace=False):
                    flat[b, ZZ[k]] = vals[i % len(vals)]
                    i += 1
        elif kind == "runs":
            for b in range(nb):
                m = b % 4
                if m == 0:  # ZRL x 3 then a coefficient at position 63 (run 14)
                    flat[b, ZZ[63]] = int(rng.integers(1, 60)) * int(rng.choice([-1, 1]))
                elif m == 1:  # a coefficient at 63 with no EOB behind it, some others before
                    flat[b, ZZ[63]] = -3
                    flat[b, ZZ[rng.choice(np.arange(1, 63), 5, replace=False)]] = rng.integers(1, 9, 5)
                elif m == 2:  # all 63 AC coefficients non-zero
                    flat[b, ZZ[1:]] = rng.choice([-1, 1], 63) * rng.integers(1, 300, 63)
                else:  # runs of exactly 15 and 16 zeros (the ZRL boundary)
                    flat[b, ZZ[16]] = 5
                    flat[b, ZZ[33]] = -7
    return planes


HISTORY_PATTERNS = ("trailing", "empty", "all", "corners", "alternating", "run_new", "zrl", "zrl_long")


def history_content(shapes, precision: int, rng: np.random.Generator, dc_cats=None, ac_syms=None, top_al: int = 1, extents=None,
                    dc_outside: bool = True, phase: int = 0, patterns=HISTORY_PATTERNS):
    """Blocks for the refinement scans of a script whose AC first passes have Al = top_al (>= 1).  For the scan at level a
    (Ah = a + 1, Al = a) a coefficient is HISTORY when |v| >= 2 << a, NEW when |v| >> a == 1, and a free zero below that.
    "History" here has |v| >= 2 << top_al: history in every refinement scan, with random correction bits at every level;
    new(a) has |v| >> a == 1: a free zero above level a, coded at level a, history below it.  Block i of component c's own
    blocks (extents, default: the whole plane; in scan order) takes pattern (i + phase + c) % 8, shaped by n = phase + i // 8:
      trailing     new coefficients at positions 1.., history only behind the last one: the block ends in an EOB whose
                   corrections wait for the run to be flushed -- and the next block
      empty        (no AC coefficient) extends that run,
      all          as do all 63 positions history, and
      corners      positions 1, 31, 32, 33, 62 and 63: history (every third n), else history and new of one level alternating;
      alternating  history and new coefficients alternating, the new ones spread over every level (and level top_al: magnitude
                   one in the first pass), a free zero now and then;
      run_new      12 + 3 (n % 13) history positions, then one new coefficient of every level top_al - 1 .. 0: the symbol of
                   level a arrives with 12 + 3 (n % 13) + (top_al - 1 - a) correction bits, 12 .. 50 over 13 blocks;
      zrl          16 free zeros with 1 + n % 16 history positions in between, then new coefficients as above: ZRL with corrections;
      zrl_long     16 free zeros with 26 + n % 18 history positions in between: more correction bits behind the ZRL than a
                   32-bit window holds behind its code.
    Outside the extents the blocks carry a DC value only (none with dc_outside False, which may be given per component: the
    script has a DC scan of the component alone).  dc_cats / ac_syms as in content(); the refinement symbols (run, 1), ZRL and EOB must be codable."""
    assert top_al >= 1
    dmax, amax = max_categories(precision)
    if ac_syms is not None:
        assert {0x00, 0xF0} | {(r << 4) | 1 for r in range(16)} <= set(ac_syms)
        amax = min(amax, min(max(s & 15 for s in ac_syms if s >> 4 == r) for r in range(16)))
    if dc_cats is not None:  # (DC differences of up to the largest category that comes with every smaller one)
        dmax = min(dmax, next(c for c in range(17) if c + 1 not in dc_cats))
    assert amax >= 3 and dmax >= 4 + top_al
    extents = list(extents) if extents is not None else list(shapes)
    big = (1 << amax) - 1
    outside = [dc_outside] * len(shapes) if isinstance(dc_outside, bool) else list(dc_outside)

    def sign():
        return int(rng.choice([-1, 1]))

    def hist():  # two or three bits in the first pass (now and then the widest category), random bits below
        if rng.random() < 0.06:
            return sign() * big
        return sign() * ((int(rng.integers(2, 8)) << top_al) | int(rng.integers(0, 1 << top_al)))

    def new(a):
        return sign() * ((1 << a) | int(rng.integers(0, 1 << a)))

    def news(z, k, first=None):  # one new coefficient of every level first .. 0 from position k on
        for a in range(top_al - 1 if first is None else first, -1, -1):
            if k <= 63:
                z[k] = new(a)
                k += 1

    def spread(z, zeros, nh):  # `zeros` free positions with nh history positions among them, from position 1 on -> next position
        order = np.zeros(zeros + nh, bool)
        order[np.round(np.linspace(0, zeros + nh - 2, nh)).astype(int)] = True  # (the last position stays a zero)
        assert order.sum() == nh
        for i, h in enumerate(order):
            if h:
                z[1 + i] = hist()
        return 1 + zeros + nh

    planes = [np.zeros(s + (64,), np.int32) for s in shapes]
    lim = min((1 << (dmax - 1)) - 1, (1 << (precision + 2)) - 1)
    for ci, (p, (eh, ew), keep_dc) in enumerate(zip(planes, extents, outside)):
        nb = p.shape[0] * p.shape[1]
        dc = np.clip(np.cumsum(rng.integers(-lim // 4, lim // 4 + 1, nb)), -lim // 2, lim // 2).reshape(p.shape[:2])
        p[:, :, 0] = dc
        if not keep_dc:
            p[eh:, :, 0] = 0
            p[:, ew:, 0] = 0
        for i in range(eh * ew):
            z = np.zeros(64, np.int64)
            kind, n = patterns[(i + phase + ci) % len(patterns)], phase + i // len(patterns)
            if kind == "trailing":
                news(z, 1)
                for k in rng.choice(np.arange(top_al + 2, 64), 1 + n % 9, replace=False):
                    z[k] = hist()
            elif kind == "all":
                z[1:] = [hist() for _ in range(63)]
            elif kind == "corners":
                a = n % top_al
                for j, k in enumerate((1, 31, 32, 33, 62, 63)):
                    z[k] = hist() if n % 3 == 0 or (j + n) % 2 else new(a)
            elif kind == "alternating":
                for k in range(1, 64):
                    a = (k // 2 + n) % (top_al + 2)
                    z[k] = hist() if k % 2 else 0 if a > top_al else new(a)
            elif kind == "run_new":
                nh = 12 + 3 * (n % 13)
                z[1:1 + nh] = [hist() for _ in range(nh)]
                news(z, 1 + nh)
            elif kind == "zrl":
                news(z, spread(z, 16, 1 + n % 16))
            elif kind == "zrl_long":
                news(z, spread(z, 16, 26 + n % 18), first=(n // 18) % top_al)
            else:
                assert kind == "empty", kind
            p[i // ew, i % ew, ZZ[1:]] = z[1:]
    return planes


def saturating_block(plane: np.ndarray, quant: np.ndarray, precision: int = 12):
    """Fill the first block of `plane` so that sum |c| q passes 2^31 (the range check saturates): needs 16-bit deltas."""
    amax = (1 << max_categories(precision)[1]) - 1
    blk = np.where(np.arange(64) % 2 == 0, amax, -amax).astype(np.int32)
    blk[0] = (1 << 14) - 1
    assert int((np.abs(blk).astype(np.int64) * quant.astype(np.int64)).sum()) > (1 << 31)
    plane.reshape(-1, 64)[0] = blk


def coded_dc_categories(planes, precision: int):
    """DC categories the sequential coding of these planes needs (predictor reset ignored: what the content generator checks)."""
    cats = set()
    for p in planes:
        dc = p.reshape(-1, 64)[:, 0].astype(np.int64)
        d = np.diff(np.concatenate([[0], dc]))
        cats |= {int(abs(int(x))).bit_length() for x in np.unique(d)}
    return cats


# ---------------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------------
class _Writer(_BitWriter):
    def __init__(self, used=None):
        super().__init__()
        self.used = used

    def code(self, table: Table, sym: int):
        c, l = table.codes[sym]
        self.put(c, l)
        if self.used is not None:
            self.used.add((id(table), sym))

    def value(self, table: Table, run: int, v: int):
        s = int(abs(v)).bit_length()
        self.code(table, (run << 4) | s)
        if s:
            self.put(v if v > 0 else v + (1 << s) - 1, s)


def _layout(width, height, samp):
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return hmax, vmax, mx, my


def plane_shapes(width: int, height: int, samp):
    """(blocks_h, blocks_w) of every component: the store the decoders fill."""
    _, _, mx, my = _layout(width, height, samp)
    return [(my * v, mx * h) for h, v in samp]


def scan_extents(width: int, height: int, samp):
    """(blocks_h, blocks_w) a non-interleaved scan of every component covers: the component's own blocks (A.2.3), which is less
    than plane_shapes' when the frame is not whole MCUs.  Interleaved scans cover the whole planes."""
    hmax, vmax, _, _ = _layout(width, height, samp)
    if len(samp) == 1:  # (one component: every scan is non-interleaved, the MCU is one block)
        return [(-(-height // 8), -(-width // 8))]
    return [(-(-(-(-height * v // vmax)) // 8), -(-(-(-width * h // hmax)) // 8)) for h, v in samp]


class Trace:
    """What the AC scans of a stream coded, as the writer saw it (write(trace=)): one record per scan.  tot: the bits of a code
    and what belongs to it (the value bits of a first pass, the sign bit of a refinement scan's new coefficient, nothing for
    ZRL); ncorr: the correction bits that follow it."""

    def __init__(self):
        self.scans = []

    def begin(self, comps, ss, se, ah, al):
        self.scans.append({"comps": tuple(comps), "ss": ss, "se": se, "ah": ah, "al": al,
                           "symbols": [],      # tot + ncorr of every coded coefficient
                           "zrl": [],          # (tot, ncorr) of every ZRL
                           "trailing": [],     # correction bits behind the last symbol of every block that is not empty (refinement)
                           "runs": [],         # (blocks, correction bits, empty blocks that joined it behind correction bits) of every EOB run
                           "skipped": 0,       # blocks that a decoder meets inside an EOB run (skip > 0)
                           "blocks": []})      # per block, in scan order: (symbols coded in it, trailing correction bits, inside a run)

    def symbol(self, tot, ncorr):
        self.scans[-1]["symbols"].append(tot + ncorr)

    def zrl(self, tot, ncorr):
        self.scans[-1]["zrl"].append((tot, ncorr))

    def trailing(self, ncorr):
        self.scans[-1]["trailing"].append(ncorr)

    def done(self, symbols, ncorr):
        self.scans[-1]["blocks"].append((symbols, ncorr, self._in_run))

    def run(self, blocks, ncorr, empty_behind):
        self.scans[-1]["runs"].append((blocks, ncorr, empty_behind))

    def block(self, in_run):
        self._in_run = bool(in_run)
        self.scans[-1]["skipped"] += bool(in_run)


def check_script(script, nc: int):
    """T.81 G.1.1.1: DC scans have Ss = Se = 0, AC scans one component and 1 <= Ss <= Se <= 63; a first pass (Ah = 0) codes
    coefficients no scan has coded, a refinement has Ah = the Al of the scan before it over the same coefficients and lowers
    it by one; the DC first pass of a component comes before its AC scans.  In the end every coefficient is complete."""
    al_of = [[None] * 64 for _ in range(nc)]
    for comps, ss, se, ah, al in script:
        assert len(set(comps)) == len(comps) >= 1 and all(0 <= c < nc for c in comps), comps
        assert (ss == 0 and se == 0) or (1 <= ss <= se <= 63 and len(comps) == 1), (comps, ss, se)
        assert 0 <= al <= 13 and 0 <= ah <= 13
        for c in comps:
            if ss:
                assert al_of[c][0] is not None, "AC scan in front of the component's DC first pass"
            for k in range(ss, se + 1):
                if ah == 0:
                    assert al_of[c][k] is None, (c, k, "coded twice")
                else:
                    assert al_of[c][k] == ah and al == ah - 1, (c, k, al_of[c][k], ah, al)
                al_of[c][k] = al
    assert all(a == 0 for c in al_of for a in c), "coefficients left incomplete"


def scripts(nc: int):
    """{name: (script, top_al)}: scan scripts aimed at the refinement pass and the level scheduler; top_al is the Al of the AC
    first passes (what history_content shapes its magnitudes by).
      deep     DC with Al = 3, every component's 1..63 with Al = 3, then DC and AC refinement 3 -> 2 -> 1 -> 0: at the last
               level all 63 positions of a block can be history
      split32  bands 1..31 and 32..63 (the device keeps the history in two 32-bit masks, split at position 32) with Al = 2, the
               last component first; refined in the opposite order
      split33  bands 1..32 and 33..63 with Al = 1; one DC scan per component, the last component first; a band's refinement
               stands in front of first passes of other bands and components, so that the scans of one level of the device's
               schedule are of different components AND kinds
      single   bands 63..63, 1..1, 2..2 and 3..62 with Al = 2, refined 2 -> 1 -> 0 in another band order each time"""
    every, rev = tuple(range(nc)), list(range(nc))[::-1]
    deep = [(every, 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in range(nc)]
    for al in (2, 1, 0):
        deep += [(every, 0, 0, al + 1, al)] + [((c,), 1, 63, al + 1, al) for c in range(nc)]
    split32 = [(every, 0, 0, 0, 1)]
    split32 += [((c,), ss, se, 0, 2) for c in rev for ss, se in ((1, 31), (32, 63))]
    split32 += [((c,), ss, se, 2, 1) for c in range(nc) for ss, se in ((32, 63), (1, 31))] + [(every, 0, 0, 1, 0)]
    split32 += [((c,), ss, se, 1, 0) for c in rev for ss, se in ((32, 63), (1, 31))]
    lo, hi = (1, 32), (33, 63)
    split33 = [((c,), 0, 0, 0, 1) for c in rev]
    first_lo, refine_lo, first_hi = (lo, 0), (lo, 1), (hi, 0)
    # the i-th AC scan of every component shares a level of the device's schedule: another kind for every component
    turns = ([first_lo, refine_lo, first_hi], [first_hi, first_lo, refine_lo], [first_lo, first_hi, refine_lo])
    for i in range(3):
        for c in rev:
            (ss, se), ah = turns[c % 3][i]
            split33.append(((c,), ss, se, ah, 0 if ah else 1))
    split33 += [((c,), 0, 0, 1, 0) for c in range(nc)]
    split33 += [((c,), hi[0], hi[1], 1, 0) for c in rev]
    single_bands = [(63, 63), (1, 1), (2, 2), (3, 62)]
    single = [(every, 0, 0, 0, 0)] + [((c,), ss, se, 0, 2) for c in range(nc) for ss, se in single_bands]
    single += [((c,), ss, se, 2, 1) for c in rev for ss, se in (single_bands[2], single_bands[0], single_bands[3], single_bands[1])]
    single += [((c,), ss, se, 1, 0) for c in range(nc) for ss, se in (single_bands[3], single_bands[1], single_bands[0], single_bands[2])]
    out = {"deep": (deep, 3), "split32": (split32, 2), "split33": (split33, 1), "single": (single, 2)}
    for script, _ in out.values():
        check_script(script, nc)
    return out


def own_dc_scans(script, nc: int):
    """Per component: has the script a DC scan of the component alone (in a frame of more components)?  Then the blocks outside
    the component's own ones can carry nothing at all."""
    return [nc > 1 and any(ss == 0 and comps == (c,) for comps, ss, _, _, _ in script) for c in range(nc)]


def _progressive_script(nc: int):
    """(components, Ss, Se, Ah, Al): DC first with Al = 1, AC first passes with and without point transform, DC and AC
    refinement.  Component 0's band 1..5 is coded at full precision in one pass (the widest categories live there)."""
    s = [(tuple(range(nc)), 0, 0, 0, 1), ((0,), 1, 5, 0, 0), ((0,), 6, 63, 0, 2)]
    s += [((c,), 1, 63, 0, 1) for c in range(1, nc)]
    s += [(tuple(range(nc)), 0, 0, 1, 0), ((0,), 6, 63, 2, 1), ((0,), 6, 63, 1, 0)]
    s += [((c,), 1, 63, 1, 0) for c in range(1, nc)]
    return s


def write(planes, width: int, height: int, samp, tables, precision: int = 8, quant=None, dri: int = 0, progressive: bool = False,
          quant16: bool = False, script=None, used: set | None = None, trace: "Trace | None" = None) -> bytes:
    """A stream that carries exactly `planes`.

    tables: per component (DC Table, AC Table); equal tables share one DHT slot.  quant: per component 64 deltas in natural
    order (default: all ones).  quant16: Pq = 1 (16-bit entries; implies SOF1 unless progressive).  The non-interleaved scans
    of a progressive frame cover the component's own blocks only (scan_extents): outside them a plane may hold nothing such a
    scan would have to carry (_scan asserts it; with an interleaved DC scan that leaves the DC values).  used: receives
    (id(table), symbol) of every Huffman symbol written.  trace: receives what the AC scans coded (Trace)."""
    nc = len(samp)
    assert len(planes) == nc == len(tables)
    shapes = plane_shapes(width, height, samp)
    for p, s in zip(planes, shapes):
        assert p.shape == s + (64,), (p.shape, s)
    hmax, vmax, mx, my = _layout(width, height, samp)
    extents = scan_extents(width, height, samp)
    quant = [np.ones(64, np.int64)] * nc if quant is None else [np.asarray(q, np.int64) for q in quant]
    qids, qtabs = [], []
    for q in quant:
        for i, t in enumerate(qtabs):
            if np.array_equal(t, q):
                qids.append(i)
                break
        else:
            qids.append(len(qtabs))
            qtabs.append(q)
    ids = {0: [], 1: []}
    slots = {0: [], 1: []}
    for dc, ac in tables:
        for tc, t in ((0, dc), (1, ac)):
            if t not in slots[tc]:
                slots[tc].append(t)
            ids[tc].append(slots[tc].index(t))
    assert len(slots[0]) <= 4 and len(slots[1]) <= 4 and len(qtabs) <= 4
    extended = precision != 8 or quant16 or len(slots[0]) > 2 or len(slots[1]) > 2
    sof = 0xC2 if progressive else (0xC1 if extended else 0xC0)

    out = bytearray(b"\xff\xd8")
    for i, q in enumerate(qtabs):
        assert q.min() >= 1 and q.max() <= (65535 if quant16 else 255)
        body = bytes([(int(quant16) << 4) | i]) + b"".join(int(q[ZZ[k]]).to_bytes(2 if quant16 else 1, "big") for k in range(64))
        out += b"\xff\xdb" + (2 + len(body)).to_bytes(2, "big") + body
    out += bytes([0xFF, sof]) + (8 + 3 * nc).to_bytes(2, "big") + bytes([precision]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        out += bytes([c + 1, (samp[c][0] << 4) | samp[c][1], qids[c]])
    body = b"".join(t.dht(tc, i) for tc in (0, 1) for i, t in enumerate(slots[tc]))
    out += b"\xff\xc4" + (2 + len(body)).to_bytes(2, "big") + body
    if dri:
        out += b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big")

    def sos(comps, ss, se, ah, al):
        b = bytes([len(comps)]) + b"".join(bytes([c + 1, (ids[0][c] << 4) | ids[1][c]]) for c in comps) + bytes([ss, se, (ah << 4) | al])
        return b"\xff\xda" + (2 + len(b)).to_bytes(2, "big") + b

    if not progressive:
        out += sos(tuple(range(nc)), 0, 63, 0, 0)
        out += _scan(planes, tables, samp, mx, my, tuple(range(nc)), 0, 63, 0, 0, dri, False, used, extents)
    else:
        for comps, ss, se, ah, al in (script or _progressive_script(nc)):
            out += sos(comps, ss, se, ah, al)
            if trace is not None:
                trace.begin(comps, ss, se, ah, al)
            out += _scan(planes, tables, samp, mx, my, comps, ss, se, ah, al, dri, True, used, extents, trace)
    return bytes(out) + b"\xff\xd9"


def _outside_is_empty(plane, ext, ss, se, ah, al) -> bool:
    """Nothing for this scan in the blocks of `plane` outside the extent `ext`?"""
    out = np.ones(plane.shape[:2], bool)
    out[:ext[0], :ext[1]] = False
    blk = plane[out]
    if ss == 0:
        dc = blk[:, 0] >> al
        return not (dc.any() if ah == 0 else (dc & 1).any())
    return not blk[:, ZZ[ss:se + 1]].any()


def _scan(planes, tables, samp, mx, my, comps, ss, se, ah, al, dri, progressive, used=None, extents=None, trace=None) -> bytes:
    """Entropy coded data of one scan (restart markers included)."""
    bw = _Writer(used)
    interleaved = len(comps) > 1
    if interleaved:
        units = [[(c, my_ * samp[c][1] + y, mx_ * samp[c][0] + x) for c in comps for y in range(samp[c][1]) for x in range(samp[c][0])]
                 for my_ in range(my) for mx_ in range(mx)]
    else:
        c = comps[0]
        # a non-interleaved scan covers the component's own blocks: with whole MCUs (or one component) the whole plane
        assert len(samp) == 1 or progressive
        bh, bwid = extents[c] if extents is not None else planes[c].shape[:2]
        assert _outside_is_empty(planes[c], (bh, bwid), ss, se, ah, al), "coefficients outside the component's own blocks"
        units = [[(c, y, x)] for y in range(bh) for x in range(bwid)]
    pred = {c: 0 for c in comps}
    # EOB run and the correction bits that wait for it (refinement); for the trace: empty blocks that joined a run with such bits
    state = {"eobrun": 0, "be": [], "empty_behind": 0}

    def flush_eobrun(ac):
        n = state["eobrun"]
        if trace is not None and n:
            trace.run(n, len(state["be"]), state["empty_behind"])
        state["empty_behind"] = 0
        if n:
            r = n.bit_length() - 1
            bw.code(ac, r << 4)
            if r:
                bw.put(n, r)
            state["eobrun"] = 0
        for bit in state["be"]:
            bw.put(bit, 1)
        state["be"] = []

    for m, unit in enumerate(units):
        if dri and m and m % dri == 0:
            if progressive and ss > 0:
                flush_eobrun(tables[comps[0]][1])
            bw.flush()
            bw.out += bytes([0xFF, 0xD0 + ((m // dri - 1) & 7)])
            pred = {c: 0 for c in comps}
        for c, y, x in unit:
            blk = planes[c][y, x]
            dc_t, ac_t = tables[c]
            if ss == 0:
                if ah == 0:  # DC first (or sequential): the difference of the point-transformed values
                    v = int(blk[0]) >> al
                    bw.value(dc_t, 0, v - pred[c])
                    pred[c] = v
                else:  # DC refinement: one raw bit
                    bw.put((int(blk[0]) >> al) & 1, 1)
                if progressive:
                    continue
                _ac_sequential(bw, ac_t, blk)
            elif ah == 0:
                _ac_first(bw, ac_t, blk, ss, se, al, state, flush_eobrun, trace)
            else:
                _ac_refine(bw, ac_t, blk, ss, se, al, state, flush_eobrun, trace)
    if progressive and ss > 0:
        flush_eobrun(tables[comps[0]][1])
    bw.flush()
    return bytes(bw.out)


def _ac_sequential(bw, ac, blk):
    z = blk[ZZ]
    r = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            r += 1
            continue
        while r > 15:
            bw.code(ac, 0xF0)
            r -= 16
        bw.value(ac, r, v)
        r = 0
    if r:
        bw.code(ac, 0x00)


def _pt(v: int, al: int) -> int:
    """AC point transform: the magnitude shifted, the sign kept (G.1.2.2)."""
    return (abs(v) >> al) * (1 if v > 0 else -1)


def _ac_first(bw, ac, blk, ss, se, al, state, flush_eobrun, trace=None):
    if trace is not None:
        trace.block(state["eobrun"] > 0)
    if not (np.abs(blk[ZZ[ss:se + 1]]) >> al).any():  # (the common case of a large sparse picture: one more block in the run)
        state["eobrun"] += 1
        if state["eobrun"] == 0x7FFF:
            flush_eobrun(ac)
        return
    z = [_pt(int(v), al) for v in blk[ZZ[ss:se + 1]]]
    r = 0
    for v in z:
        if v == 0:
            r += 1
            continue
        flush_eobrun(ac)
        while r > 15:
            bw.code(ac, 0xF0)
            r -= 16
            if trace is not None:
                trace.zrl(ac.length(0xF0), 0)
        bw.value(ac, r, v)
        if trace is not None:
            s = int(abs(v)).bit_length()
            trace.symbol(ac.length((r << 4) | s) + s, 0)
        r = 0
    if r:
        state["eobrun"] += 1
        if state["eobrun"] == 0x7FFF:
            flush_eobrun(ac)


def _ac_refine(bw, ac, blk, ss, se, al, state, flush_eobrun, trace=None):
    """G.1.2.3: newly non-zero coefficients (magnitude 1 at this Al) are coded with a run of coefficients that have been zero so
    far; coefficients that were non-zero before contribute a correction bit, sent behind the next symbol (or the EOB run)."""
    if trace is not None:
        trace.block(state["eobrun"] > 0)
    if not (np.abs(blk[ZZ[ss:se + 1]]) >> al).any():
        state["empty_behind"] += bool(state["be"])
        if trace is not None:
            trace.done(0, 0)
        state["eobrun"] += 1
        if state["eobrun"] == 0x7FFF:
            flush_eobrun(ac)
        return
    vals = [int(v) for v in blk[ZZ[ss:se + 1]]]
    mag = [abs(v) >> al for v in vals]
    eob = max((i for i, a in enumerate(mag) if a == 1), default=-1)
    r, br, coded = 0, [], 0
    for i, a in enumerate(mag):
        if a == 0:
            r += 1
            continue
        while r > 15 and i <= eob:
            flush_eobrun(ac)
            bw.code(ac, 0xF0)
            r -= 16
            for bit in br:
                bw.put(bit, 1)
            if trace is not None:
                trace.zrl(ac.length(0xF0), len(br))
            br = []
        if a > 1:
            br.append(a & 1)
            continue
        flush_eobrun(ac)
        bw.code(ac, (r << 4) | 1)
        bw.put(1 if vals[i] > 0 else 0, 1)
        for bit in br:
            bw.put(bit, 1)
        if trace is not None:
            trace.symbol(ac.length((r << 4) | 1) + 1, len(br))
        br, r, coded = [], 0, coded + 1
    if trace is not None:
        trace.trailing(len(br))
        trace.done(coded, len(br))
    if r or br:
        state["eobrun"] += 1
        state["be"] += br
        if state["eobrun"] == 0x7FFF or len(state["be"]) > 937:
            flush_eobrun(ac)

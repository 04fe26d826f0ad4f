"""The forward (encoder direction) kernels at their partition edges, pitches and ties (forward.hip, forward_kernels.inc,
encode_list.hpp::forward_args_of): every comparison is with the reference model of tests/forward_cases.py -- oracle.forward
at 8 bits, enc12_util.forward12 at 12, never the library's own forward path --, covers every block that covers samples, and is exact.

1. uniform launches (mijpeg_launch_forward): three frames of different content, padded row and frame strides, bases and pitches on
   and off the dword boundaries, a padded coefficient frame stride; the whole coefficient tensor is compared, guards and gaps included.
2. the same pictures through tile + interior + block kernels, interior + block, and the block kernel alone.
3. ragged lists of interleaved pictures (mijpeg_encode_ragged_device16), each a view into one guarded buffer.
4. the same lists as component planes (mijpeg_encode_ragged_planar_device16).
Which route a combination takes is asserted from the restated rule of forward_args_of (forward_cases.owners and friends)."""
import numpy as np
import pytest

import enc12_util as U
import forward_cases as F
from libjpeg_amd import api

pytestmark = pytest.mark.gpu

FILL = 0x5A5A
GUARD = 64  # int16 elements in front of and behind the coefficient frames; bytes around the pixels

GROUPS = {"420_tiles": [(w, h, "420") for w, h in F.TILES_420], "420_no_tiles": [(w, h, "420") for w, h in F.NO_TILES_420],
          **{"small_" + lay: [(w, h, lay) for w, h in F.SMALL] for lay in ("444", "422", "440", "420")},
          **{lay: [(w, h, lay) for w, h in F.SUB_BLOCK] for lay in ("411", "3x3", "4x2", "mixed")},
          "plain": [(w, h, lay) for lay in ("grey", "rgb") for w, h in F.PLAIN]}
assert sorted(s for g in GROUPS.values() for s in g) == sorted(F.SHAPES)


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _torch():
    import torch

    return torch


def _bytes_of(img: np.ndarray) -> np.ndarray:
    """A picture's lines as bytes: (h, line bytes)."""
    return np.ascontiguousarray(img).view(np.uint8).reshape(img.shape[0], -1)


def _contents(i: int):
    return [F.CONTENTS[(i + j) % len(F.CONTENTS)] for j in range(3)]


def _launch(w, h, layout, precision, base, pitch, table, contents):
    """One uniform launch of three frames -> nothing; asserts the whole coefficient tensor and that the pixels are what they were."""
    torch = _torch()
    nc, frames = F.components_of(layout), len(contents)
    hs, vs = F.LAYOUTS[layout]
    quants = F.tables(table, nc)
    info = api.frame_layout(w, h, nc, hs, vs, quants, quant_index=list(range(nc)), ycbcr=1 if F.ycbcr_of(layout) else 0, precision=precision)
    offs, count = F.coef_layout(w, h, layout)
    assert int(info.coef_count) == count and [int(info.coef_offset[c]) for c in range(nc)] == offs
    line = w * nc * (1 if precision == 8 else 2)
    assert pitch >= line
    frame_stride = h * pitch + 8  # (a multiple of 4 where the pitch is one)
    rng = np.random.default_rng(w * 7 + h)
    host = rng.integers(0, 256, GUARD + base + frames * frame_stride + GUARD, dtype=np.uint8)  # (padding and gaps: random bytes)
    expect = np.full(GUARD + frames * (count + 3 * GUARD) + GUARD, FILL, np.int16)
    cstride = count + 3 * GUARD  # frames start on 128-byte boundaries, 192 elements of fill between them
    for f, content in enumerate(contents):
        img, planes = F.case(w, h, layout, precision, content, table)
        rows = host[GUARD + base + f * frame_stride:][:h * pitch].reshape(h, pitch)
        rows[:, :line] = _bytes_of(img)
        expect[GUARD + f * cstride:][:count] = F.coefficient_store(planes, w, h, layout)
    px = torch.from_numpy(host).cuda()
    coef = torch.full((expect.size,), FILL, dtype=torch.int16, device="cuda")
    assert px.data_ptr() % 16 == 0 and coef.data_ptr() % 128 == 0
    first = px.data_ptr() + GUARD + base
    dword = F.dword_lines(first, pitch, frame_stride)
    assert dword == (base % 4 == 0 and pitch % 4 == 0)
    api.launch_forward(info, first, coef.data_ptr() + 2 * GUARD, frames, pitch, frame_stride, coef_frame_stride=cstride,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = coef.cpu().numpy()
    if not np.array_equal(got, expect):
        bad = np.flatnonzero(got != expect)
        where = []
        for at in bad[:4].tolist():
            f, e = divmod(at - GUARD, cstride)
            c = max([k for k in range(nc) if offs[k] <= e], default=0) if 0 <= e < count and at >= GUARD else -1
            where.append((at, f, c, (e - offs[c]) // 64 if c >= 0 else None, int(got[at]), int(expect[at])))
        raise AssertionError(f"{w}x{h} {layout} P{precision} base {base} pitch {pitch} {table} {contents} dword {dword}: {bad.size} elements differ; "
                             f"(index, frame, component, block, got, expected): {where}")
    assert np.array_equal(px.cpu().numpy(), host), "the source pixels were written to"
    return dword


def _pitches(line: int, precision: int):
    extra = (0, 1, 4, 5) if precision == 8 else (0, 2, 4, 6)
    return sorted({line + e for e in extra} | {(line + 3) & ~3})  # (and the next multiple of 4: a dword pitch for every width)


@pytest.mark.parametrize("precision", F.PRECISIONS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_uniform_launches_at_every_base_and_pitch(group, precision):
    """8 bit: bases 0 .. 3 bytes off a dword boundary, pitches of a line + 0, 1, 4, 5 bytes; 12 bit: bases 0 and 2, pitches of a line
    + 0, 2, 4, 6; both with the line rounded up to a dword as well, so that every width has a combination on the dword route (tile and
    interior kernels where the layout has them) and several off it (the per-block kernel alone): the same answer."""
    for w, h, layout in GROUPS[group]:
        line = w * F.components_of(layout) * (1 if precision == 8 else 2)
        routes, i = set(), 0
        for base in ((0, 1, 2, 3) if precision == 8 else (0, 2)):
            for pitch in _pitches(line, precision):
                routes.add(_launch(w, h, layout, precision, base, pitch, F.TABLES[i % 4], _contents(i)))
                i += 1
        assert routes == {False, True}, (w, h, layout)


@pytest.mark.parametrize("precision", F.PRECISIONS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_three_routes_one_answer(group, precision, monkeypatch):
    """Dword lines, every table, every content: as routed (tile + interior + block kernels), with MIJPEG_FORWARD_NO_TILES (interior +
    block) and with MIJPEG_FORWARD_SLOW (the block kernel alone); forward_args_of reads the variables on every call.  A failure of
    one route alone names the kernel."""
    for env in (None, "MIJPEG_FORWARD_NO_TILES", "MIJPEG_FORWARD_SLOW"):
        if env:
            monkeypatch.setenv(env, "1")
        for w, h, layout in GROUPS[group]:
            line = w * F.components_of(layout) * (1 if precision == 8 else 2)
            for i, table in enumerate(F.TABLES):
                assert _launch(w, h, layout, precision, 0, ((line + 3) & ~3) + 4 * (i & 1), table, _contents(i))
        if env:
            monkeypatch.delenv(env)
    # what the three runs reached, from the restated rule
    kinds = [{int(k) for s in GROUPS[group] for o in F.owners(*s, **route) for k in np.unique(o)} for route in ({}, dict(no_tiles=True), dict(slow=True))]
    assert F.TILE not in kinds[1] and not kinds[2] & {F.TILE, F.INTERIOR}
    if group == "420_tiles":
        assert kinds[0] >= {F.TILE, F.INTERIOR, F.EDGE, F.PAD} and kinds[1] >= {F.INTERIOR, F.EDGE, F.PAD}
    if group.startswith("small_") or group == "420_no_tiles":
        assert F.INTERIOR in kinds[0]


# ---- ragged lists -------------------------------------------------------------------------------------------------------------------------
RAGGED_SHAPES = [s for s in F.SHAPES if s[2] != "rgb"]  # (a ragged frame cannot ask for the identity transformation)


def _entries(flip: int):
    """(w, h, layout, precision, content, quality, dword wanted) for the whole corpus: precision, quality, content and route change along
    the list; `flip` gives every shape the other precision and quality.  Behind them the 4:2:0 pictures with whole tiles once more, at
    the other precision and on the dword route: over the two lists each of them meets the tile kernel of either precision."""
    out = [(w, h, lay, (8, 12)[(i + flip) % 2], F.CONTENTS[(i + 2 * flip) % 5], (100, 5)[(i // 2 + flip) % 2], (i + flip) % 3 != 0)
           for i, (w, h, lay) in enumerate(RAGGED_SHAPES)]
    return out + [(w, h, lay, 20 - p, F.CONTENTS[(i + 3) % 5], 105 - q, True) for i, (w, h, lay, p, _, q, _) in enumerate(out[:len(F.TILES_420)])]


def _place(e, k: int):
    """Where picture k of a list goes: (bytes off a 16-byte boundary, pitch).  Wanted on the dword route: base 0, the line rounded up
    plus 0 or 4; otherwise a base or a pitch off it (8 bit: 1 .. 3 bytes; 12 bit: 2)."""
    w, h, lay, precision, _, _, want = e
    sb = 1 if precision == 8 else 2
    line = w * F.components_of(lay) * sb
    up = (line + 3) & ~3
    if want:
        return 0, up + 4 * (k & 1)
    if precision == 12:
        return ((2, up + 4), (0, up + 2), (2, up + 2))[k % 3]
    return ((1, up), (0, up + 1), (2, up + 5), (3, up + 3), (0, up + 2))[k % 5]


def _launch_lists(entries, places):
    """The work lists a pass of these pictures fills, from the rule: {(flavour, kernel family)}."""
    lists = set()
    for (w, h, lay, precision, _, _, _), (dword, flavour) in zip(entries, places):
        for c, own in enumerate(F.owners(w, h, lay, dword=dword)):
            if (own == F.TILE).any():
                lists.add((flavour, "tile"))
            # (the interior kernels are launched over all whole blocks of a fast component, the tile kernel's among them)
            if F.fast_components(lay, dword)[c] and (w // (8 * F.interior_kernel(lay, c)[0])) * (h // (8 * F.interior_kernel(lay, c)[1])) > 0:
                lists.add((flavour, F.interior_kernel(lay, c)))
        lists.add((flavour, "block"))
    return lists


def _check_streams(oracle, streams, entries, what):
    for k, (data, (w, h, lay, precision, content, q, _)) in enumerate(zip(streams, entries)):
        oi, planes = oracle.decode_coefficients(data)
        nc = F.components_of(lay)
        assert (oi.width, oi.height, oi.precision, oi.ncomp) == (w, h, precision, nc), (what, k)
        hs, vs = F.LAYOUTS[lay]
        quants = [U.oracle_quant(oi, c) for c in range(nc)]
        assert int(quants[0].max()) == 1 if q == 100 else int(quants[0].max()) >= 255
        exp = F.expected(F.picture(w, h, lay, precision, content), hs, vs, quants, precision, True)
        for c, (_, _, bw, bh, nbx, nby) in enumerate(F.geometry(w, h, lay)):
            assert planes[c].shape == (bh, bw, 64)
            g, e = planes[c][:nby, :nbx], exp[c][:nby, :nbx]
            assert np.array_equal(g, e), (what, k, (w, h, lay, precision, content, q), c, np.argwhere(g != e)[:4].tolist())
            pad = planes[c].copy()  # MCU padding blocks: the entropy coder repeats the DC in front of them and codes no AC
            pad[:nby, :nbx] = 0
            assert not pad[..., 1:].any(), (what, k, c)


def _interleaved_list(entries):
    """The pictures of a list in ONE guarded host buffer, each at its own base and pitch -> (host bytes, [(offset, pitch)])."""
    at, spots = GUARD, []
    for k, e in enumerate(entries):
        off, pitch = _place(e, k)
        at = ((at + 15) & ~15) + off
        spots.append((at, pitch))
        at += e[1] * pitch + 3
    host = np.random.default_rng(len(entries)).integers(0, 256, at + GUARD, dtype=np.uint8)
    for (w, h, lay, precision, content, _, _), (start, pitch) in zip(entries, spots):
        b = _bytes_of(F.picture(w, h, lay, precision, content))
        host[start:start + h * pitch].reshape(h, pitch)[:, :b.shape[1]] = b
    return host, spots


def _run_interleaved(dec, oracle, entries, what):
    torch = _torch()
    host, spots = _interleaved_list(entries)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    frames, places = [], []
    for (w, h, lay, precision, _, q, want), (start, pitch) in zip(entries, spots):
        frames.append(api.encode_frame(w, h, F.components_of(lay), q, F.LAYOUTS[lay], 0, buf.data_ptr() + start, pitch))
        dword = F.dword_lines(buf.data_ptr() + start, pitch, pitch * h)
        assert dword == want, (what, w, h, lay, start, pitch)
        places.append((dword, precision))
    streams = dec.encode_ragged_device(frames, False, precision=[e[3] for e in entries])
    st = dec.encode_ragged_stats()
    assert st["pictures"] == len(entries) and st["passes"] == 1
    assert st["forward_launches"] == len(_launch_lists(entries, places)), (what, st, sorted(map(str, _launch_lists(entries, places))))
    assert np.array_equal(buf.cpu().numpy(), host), "the source pixels were written to"
    _check_streams(oracle, streams, entries, what)


@pytest.mark.parametrize("flip", [0, 1])
def test_ragged_list_of_the_whole_corpus(dec, oracle, flip):
    """Every shape of the corpus (but the identity transformation, which a ragged frame cannot ask for) in one list, precisions,
    qualities 100 and 5, contents and routes changing along it, every picture a view into one guarded buffer with a base and a pitch of
    its own; each stream decoded by the oracle and compared with the model under the stream's own tables."""
    entries = _entries(flip)
    assert {e[3] for e in entries} == {8, 12} and {e[5] for e in entries} == {100, 5} and {e[4] for e in entries} == set(F.CONTENTS) and {e[6] for e in entries} == {True, False}
    for lay in ("420", "444", "422", "440"):  # each of these layouts on the dword route and off it, at both precisions
        assert {(e[3], e[6]) for e in entries if e[2] == lay} == {(8, True), (8, False), (12, True), (12, False)}, lay
    _run_interleaved(dec, oracle, entries, f"all, flip {flip}")


def _short_lists(entries, n: int):
    """Where the lists of n pictures start: every fifth (n = 1) or seventh picture, and every 4:2:0 picture with whole tiles that is on
    the dword route (a list of one: the tile kernel's work list, and what it leaves to the others, with a single item)."""
    tiles = {i for i, e in enumerate(entries) if e[:3] in [(w, h, "420") for w, h in F.TILES_420] and e[6]}
    assert {entries[i][3] for i in tiles} == {8, 12} and {entries[i][:2] for i in tiles} >= {(144, 136), (255, 257)}
    return sorted((set(range(0, len(entries), 5 if n == 1 else 7)) | tiles) & set(range(len(entries) - n + 1)))


@pytest.mark.parametrize("n", [1, 2])
def test_ragged_lists_of_one_and_two(dec, oracle, n):
    """Work lists of one and two items: the binary search of a workgroup for its picture at its ends."""
    entries = _entries(0) + _entries(1)
    for i in _short_lists(entries, n):
        _run_interleaved(dec, oracle, entries[i:i + n], f"{n} at {i}")


def _planar_list(entries):
    """The same pictures as component planes in one guarded host buffer -> (host bytes, [(plane offsets, pitch)]).  Wanted on the dword
    route: every plane and the pitch on dword boundaries; otherwise plane c starts c + 1 bytes off one (16-bit samples: 2 bytes off,
    or a pitch off), the pitch padded."""
    at, spots = GUARD, []
    for k, (w, h, lay, precision, _, _, want) in enumerate(entries):
        sb = 1 if precision == 8 else 2
        up = (w * sb + 3) & ~3
        pitch = up + 4 * (k & 1) if want else up + ((1, 4, 5, 3)[k % 4] if sb == 1 else (2, 4, 6)[k % 3])
        starts = []
        for c in range(F.components_of(lay)):
            at = ((at + 15) & ~15) + (0 if want else (c + 1 + k) % 4 if sb == 1 else 2 * ((c + k) % 2))
            starts.append(at)
            at += h * pitch + 5
        spots.append((starts, pitch))
    host = np.random.default_rng(len(entries) + 1).integers(0, 256, at + GUARD, dtype=np.uint8)
    for (w, h, lay, precision, content, _, _), (starts, pitch) in zip(entries, spots):
        img = F.picture(w, h, lay, precision, content)
        for c, start in enumerate(starts):
            b = _bytes_of(img if img.ndim == 2 else img[..., c])
            host[start:start + h * pitch].reshape(h, pitch)[:, :b.shape[1]] = b
    return host, spots


def _run_planar(dec, oracle, entries, what):
    torch = _torch()
    host, spots = _planar_list(entries)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    frames, planes, places = [], [], []
    fused = two_pass = own = 0
    for (w, h, lay, precision, _, q, want), (starts, pitch) in zip(entries, spots):
        nc = F.components_of(lay)
        frames.append(api.encode_frame(w, h, nc, q, F.LAYOUTS[lay], 0, 0, pitch))
        planes.append([buf.data_ptr() + s for s in starts])
        if nc == 1:  # its own plane: an interleaved picture of one component, never fast
            own += 1
            places.append((False, precision))
        elif precision == 12:  # interleaved first, into lines on dword boundaries
            two_pass += 1
            places.append((True, 12))
        else:
            fused += 1
            dword = all(s % 4 == 0 for s in starts) and pitch % 4 == 0
            assert dword == want, (what, w, h, lay, starts, pitch)
            places.append((dword, "planar"))
    streams = dec.encode_ragged_planar_device(frames, planes, False, [e[3] for e in entries])
    st, pst = dec.encode_ragged_stats(), dec.encode_planar_stats()
    assert pst == dict(pictures=len(entries), fused=fused, two_pass=two_pass, own_plane=own, interleave_launches=two_pass), (what, pst)
    assert st["pictures"] == len(entries) and st["passes"] == 1
    assert st["forward_launches"] == len(_launch_lists(entries, places)), (what, st)
    assert np.array_equal(buf.cpu().numpy(), host), "the source planes were written to"
    _check_streams(oracle, streams, entries, what)


@pytest.mark.parametrize("flip", [0, 1])
def test_ragged_planar_list_of_the_whole_corpus(dec, oracle, flip):
    """The same list as component planes, plane bases off their dword boundaries and padded plane pitches for the pictures off the dword
    route: the planar-input flavours of the three kernel families (8-bit colour), interleave_kernel and the ragged 12-bit flavours
    (12-bit colour, always on the dword route: the interleaved copy's lines are), one-component pictures as their own plane."""
    entries = _entries(flip)
    _run_planar(dec, oracle, entries, f"planar all, flip {flip}")


@pytest.mark.parametrize("n", [1, 2])
def test_ragged_planar_lists_of_one_and_two(dec, oracle, n):
    entries = _entries(0) + _entries(1)
    for i in _short_lists(entries, n):
        _run_planar(dec, oracle, entries[i:i + n], f"planar {n} at {i}")

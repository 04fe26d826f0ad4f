"""Ragged batches: n streams of different shapes through one device pass (mijpeg_decode_ragged_device /
mijpeg_reconstruct_ragged_device, libjpeg_amd.batch.decode_mixed).

CPU: the host-only planner (grouping, workgroup ranges, coefficient bases) and a guard on the machine code -- the ragged
flavours of the five fused kernels use no scratch, the flavours that existed before keep their register counts.
GPU: every picture against the oracle, exactly; the statistics show that the group launches really ran.
"""
import ctypes as C
import os
import re
import socket
import subprocess
import sys
import tempfile
import textwrap
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT, golden_jpeg
from libjpeg_amd import api, synth
from route_streams import grey_2x2_jpeg, host_decodes, noise_jpeg
from test_isa_guard import LIB, gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
LAYOUTS = {"420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "444": ((1, 1, 1), (1, 1, 1)), "grey": ((1,), (1,))}


# ------------------------------------------------------------------------------------------------ CPU: planner
def _layout(w, h, hs, vs):
    q = [[16] * 64, [17] * 64]
    return api.frame_layout(w, h, len(hs), hs, vs, q)


def _planner_list():
    """300 frame descriptions, seeded: sizes 1..4100 in the four layouts, every ninth one something no group takes."""
    rng = np.random.default_rng(20261016)
    infos, eligible = [], []
    names = list(LAYOUTS)
    for i in range(300):
        w, h = int(rng.integers(1, 4101)), int(rng.integers(1, 4101))
        if i % 9 == 4:
            kind = (i // 9) % 4
            if kind == 0:
                f = _layout(w, h, (1, 1, 1), (2, 1, 1))  # 4:4:0
            elif kind == 1:
                f = _layout(w, h, (4, 1, 1), (1, 1, 1))  # 4:1:1
            elif kind == 2:
                f = _layout(w, h, (2, 1, 1), (2, 1, 1))
                f.precision = 12
            else:
                f = _layout(w, h, (2, 1, 1), (2, 1, 1))
                f.progressive = 1
            eligible.append(None)
        else:
            name = names[int(rng.integers(0, 4))]
            f = _layout(w, h, *LAYOUTS[name])
            eligible.append(name)
        infos.append(f)
    return infos, eligible


def test_planner_groups_ranges_and_bases():
    infos, eligible = _planner_list()
    group, frames, grids, total = api.ragged_plan(infos)
    # every eligible image is in exactly one group -- its layout's -- and everything else is reported as fallback
    for i, name in enumerate(eligible):
        assert group[i] == (api.RAGGED_GROUPS.index(name) if name else -1), (i, name, group[i])
    # workgroup ranges: per group disjoint, in list order, exactly tiles_x * tiles_y per frame (128 x 128 tiles), no padding
    for g in range(4):
        at = 0
        for i in range(len(infos)):
            if group[i] != g:
                continue
            fr, f = frames[i], infos[i]
            assert (fr.tiles_x, fr.tiles_y) == ((f.width + 127) // 128, (f.height + 127) // 128)
            assert fr.first_workgroup == at, (g, i)
            at += fr.tiles_x * fr.tiles_y
            assert (fr.width, fr.height, fr.bw_y, fr.bh_y) == (f.width, f.height, f.blocks_w[0], f.blocks_h[0])
            # valid chroma samples, as the uniform launches of the same kernels have them: only 4:2:2 keeps the full height
            assert fr.cw == (f.width + 1) // 2
            assert fr.ch == (f.height if g == api.RAGGED_GROUPS.index("422") else (f.height + 1) // 2)
            if f.components == 3:
                assert (fr.bw_c, fr.bh_c, fr.off_cb, fr.off_cr) == (f.blocks_w[1], f.blocks_h[1], f.coef_offset[1], f.coef_offset[2])
        assert grids[g] == at
    assert all(grids[g] > 0 for g in range(4))
    # coefficient stores: back to back in list order, coef_count each, nothing overlaps
    spans = sorted((frames[i].coef_base, infos[i].coef_count) for i in range(len(infos)) if group[i] >= 0)
    at = 0
    for base, count in spans:
        assert base == at and count > 0
        at += count
    assert total == at


def test_planner_argument_errors():
    L = api.lib()
    f = _layout(64, 64, *LAYOUTS["420"])
    group, frames, grids, total = (C.c_int32 * 1)(), (api.MijpegRaggedFrame * 1)(), (C.c_int32 * 4)(), C.c_int64()
    ok = (C.byref(f), 1, group, frames, grids, C.byref(total))
    assert L.mijpeg_ragged_plan(*ok) == 0
    assert L.mijpeg_ragged_plan(C.byref(f), 0, group, frames, grids, C.byref(total)) == api.ERR_INVALID_PARAMETER
    for k in (0, 2, 3, 4, 5):
        args = list(ok)
        args[k] = None
        assert L.mijpeg_ragged_plan(*args) == api.ERR_INVALID_PARAMETER, k
    # the decoder-object calls: NULL lists, n = 0 (no device needed to be told so)
    d = api.Decoder(None)
    status = (C.c_int32 * 1)()
    arr, sizes = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    assert L.mijpeg_decode_ragged_device(d._h, arr, sizes, 0, 0, status) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_decode_ragged_device(d._h, None, sizes, 1, 0, status) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_decode_ragged_device(d._h, arr, sizes, 1, 0, None) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_reconstruct_ragged_device(d._h, None, None, 0, 1) == api.ERR_INVALID_PARAMETER
    assert L.mijpeg_decode_ragged_device(d._h, arr, sizes, 1, 0, status) == api.ERR_NOT_AVAILABLE  # created without a device
    d.close()


# ------------------------------------------------------------------------------------------------ CPU: machine code
# VGPRs of the five kernels' instantiations in a build of the parent commit 3768c42 ("Give the fused tile kernels one copy of
# their shared steps"), same compiler (ROCm 7.2 hipcc, --offload-arch=gfx950 -O3); key: kernel, template arguments as mangled.
PARENT_VGPRS = {
    ("fused1_kernel", (0, 12)): 97, ("fused1_kernel", (0, 8)): 91, ("fused1_kernel", (1, 12)): 96, ("fused1_kernel", (1, 8)): 96,
    ("fused420_kernel", (0, 2, 0, 8, 0)): 193, ("fused420_kernel", (0, 2, 1, 8, 0)): 193,
    ("fused420_kernel", (1, 2, 0, 12, 0)): 129, ("fused420_kernel", (1, 2, 0, 12, 1)): 128, ("fused420_kernel", (1, 2, 0, 8, 0)): 133,
    ("fused420_kernel", (1, 2, 1, 12, 0)): 130, ("fused420_kernel", (1, 2, 1, 12, 1)): 130, ("fused420_kernel", (1, 2, 1, 8, 0)): 131,
    ("fused422_kernel", (3, 0, 0)): 128, ("fused422_kernel", (3, 0, 1)): 128, ("fused422_kernel", (3, 1, 0)): 135, ("fused422_kernel", (3, 1, 1)): 135,
    ("fused444_kernel", (2, 1)): 175, ("fused444_kernel", (3, 0)): 160,
    ("fused420p_kernel", (3, 1, 0)): 133, ("fused420p_kernel", (4, 0, 0)): 127, ("fused420p_kernel", (4, 0, 1)): 128,
}


def _kernel_metadata(path):
    """{mangled name: {field: value}} from the code objects' AMDGPU metadata notes."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(gfx950_code_objects(path)):
            f = os.path.join(tmp, f"k{i}.co")
            open(f, "wb").write(co)
            txt = subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout
            cur = None
            for ln in txt.splitlines():
                head = re.match(r"^  - \.(\w+):\s*(.*)", ln)  # an element of amdhsa.kernels
                field = head or re.match(r"^    \.(\w+):\s*(.*)", ln)  # ... and its scalar fields (arguments sit deeper)
                if head:
                    cur = {}
                if field and cur is not None:
                    cur[field.group(1)] = field.group(2).strip()
                    if field.group(1) == "name":
                        out[cur["name"]] = cur
    return out


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_ragged_flavours_cost_the_existing_kernels_nothing():
    meta = _kernel_metadata(LIB)
    pat = re.compile(r"^_ZN3mij\d+(fused(?:420p|420|422|444|1)_kernel)I((?:L[bi]\d+E)+)EEvNS_12Fused420ArgsE$")
    seen, ragged = set(), []
    for name, k in meta.items():
        m = pat.match(name)
        if not m:
            continue
        args = tuple(int(x) for x in re.findall(r"L[bi](\d+)E", m.group(2)))
        if args[-1]:  # RAGGED is the last template parameter of all five
            ragged.append(m.group(1))
            assert int(k["private_segment_fixed_size"]) == 0, f"{name}: scratch"
            assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, name
            assert int(k["vgpr_count"]) <= PARENT_VGPRS.get((m.group(1), args[:-1]), 512), f"{name}: more VGPRs than its uniform twin"
        else:
            key = (m.group(1), args[:-1])
            assert key in PARENT_VGPRS, f"instantiation the parent did not have: {name}"
            assert int(k["vgpr_count"]) == PARENT_VGPRS[key], f"{name}: {k['vgpr_count']} VGPRs, the parent's build had {PARENT_VGPRS[key]}"
            assert int(k["private_segment_fixed_size"]) == 0, name
            seen.add(key)
    assert seen == set(PARENT_VGPRS), sorted(set(PARENT_VGPRS) - seen)
    # packed 4:2:0; 4:2:0 fast and safe; 4:2:2 packed and wide; 4:4:4; grey
    assert sorted(ragged) == sorted(["fused420p_kernel", "fused420_kernel", "fused420_kernel", "fused422_kernel", "fused422_kernel", "fused444_kernel", "fused1_kernel"])


# ------------------------------------------------------------------------------------------------ GPU
SHAPES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (127, 129), (128, 128), (129, 127), (500, 375), (375, 500), (640, 480), (1000, 3), (3, 1000),
          (1280, 720), (333, 2049), (2048, 2048), (3840, 2160)]


def _encode(w, h, seed, quality, layout, dri, optimize):
    img = synth.synth_image(w, h, seed, channels=1 if layout == "grey" else 3)
    return synth.encode_jpeg(img, quality, "444" if layout == "grey" else layout, dri, optimize=optimize)


def _mixed_list():
    """17 shapes x {4:2:0, 4:4:4, 4:2:2, grey}: qualities 50/85/95/99, DRI 0/1/4/7 (both cycling against shape and layout so that
    every group holds every DRI), optimised tables on every other stream."""
    jobs = []
    for si, (w, h) in enumerate(SHAPES):
        for li, layout in enumerate(("420", "444", "422", "grey")):
            k = si * 4 + li
            jobs.append((w, h, 700 + k, (50, 85, 95, 99)[(si + li) % 4], layout, (0, 1, 4, 7)[(si + 2 * li + si // 4) % 4], k % 2 == 1))
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda j: _encode(*j), jobs)), jobs


def _decode_all(oracle, streams, fn=None):
    with ThreadPoolExecutor(16) as ex:  # (ctypes releases the GIL)
        return list(ex.map(fn or oracle.decode, streams))


def _flavour(info):
    """(kernel name with per-frame tables, fast arithmetic) -- what shares a launch inside a group."""
    b = api.MijpegBatch()
    C.memmove(C.byref(b.info), C.byref(info), C.sizeof(api.MijpegInfo))
    b.frames = 1
    b.quant_dev = 16  # (only asked whether it is set)
    return api.lib().mijpeg_kernel_name(C.byref(b)).decode(), int(info.fast_arith)


def _reconstruct_guarded(d, infos, pads):
    """Every image into a buffer of its own, pre-filled with 0xA5, with guard bytes before and behind its rows and a padded
    row stride; -> (pictures, True where a byte outside a picture's width x components per line changed).  infos[i] None: the
    image has no picture (a stream in error) and gets no destination."""
    import torch

    GUARD = 64
    bufs, ptrs, rows = [], [], []
    for i, f in enumerate(infos):
        if f is None:
            bufs.append(None)
            ptrs.append(0)
            rows.append(0)
            continue
        line = f.width * f.components * max(1, f.sample_bytes)
        row = line + pads[i % len(pads)]
        t = torch.full((GUARD + f.height * row + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        bufs.append(t)
        ptrs.append(t.data_ptr() + GUARD)
        rows.append(row)
    d.reconstruct_ragged_device(ptrs, rows)
    pics, touched = [], []
    for i, f in enumerate(infos):
        if f is None:
            pics.append(None)
            touched.append(False)
            continue
        line, row = f.width * f.components * max(1, f.sample_bytes), rows[i]
        flat = bufs[i].cpu().numpy()
        body = flat[GUARD:GUARD + f.height * row].reshape(f.height, row)
        touched.append(bool((flat[:GUARD] != 0xA5).any() or (flat[GUARD + f.height * row:] != 0xA5).any() or (body[:, line:] != 0xA5).any()))
        pix = np.ascontiguousarray(body[:, :line])
        pics.append(pix.view("<u2").reshape(f.height, f.width, f.components) if f.sample_bytes > 1 else pix.reshape(f.height, f.width, f.components))
    return pics, touched


@pytest.mark.gpu
def test_the_mixed_list(oracle):
    """68 streams of 17 shapes x 4 layouts in ONE decode call and ONE reconstruct call: every picture equals the oracle's, nothing
    outside a picture is written, and the statistics show the group launches did it: no fallback, one Huffman launch per group,
    one reconstruction launch per group and arithmetic flavour.

    A group is split by arithmetic flavour (an image beyond the packed chroma gate of 2047 or the FAST gate does not take the
    others along: test_arithmetic_outlier_inside_a_group), so the bound is the number of flavours the range checks select, computed
    here from every image's own info.  On this list they select one per group -- the packed 4:2:0 and 4:2:2 kernels, the 4:4:4
    and the grey kernel: four reconstruction launches."""
    streams, jobs = _mixed_list()
    assert len(streams) == 68
    exp = _decode_all(oracle, streams)
    d = api.Decoder(0)
    status = d.decode_ragged_device(streams)
    assert status == [0] * 68
    infos = [d.ragged_info(i) for i in range(68)]
    for f, (w, h, *_rest) in zip(infos, jobs):
        assert (f.width, f.height) == (w, h)
    pics, touched = _reconstruct_guarded(d, infos, (0, 4, 13))
    st = d.ragged_stats()
    print("ragged stats:", st)
    flavours = {(jobs[i][4],) + _flavour(infos[i]) for i in range(68)}
    print("flavours:", sorted(flavours))
    bad = [i for i in range(68) if pics[i].shape != exp[i].shape or not np.array_equal(pics[i], exp[i])]
    assert not bad, [jobs[i] for i in bad]
    assert not any(touched), [jobs[i] for i in range(68) if touched[i]]
    assert st["images"] == 68 and st["ragged"] == 68 and st["fallbacks"] == 0 and st["errors"] == 0
    assert 1 <= st["entropy_launches"] <= 4
    assert st["walk_launches"] > 0  # every group holds streams without restart markers
    assert st["recon_single"] == 0
    assert st["recon_launches"] == len(flavours) and st["recon_launches"] <= 4 * 3
    d.close()


@pytest.mark.gpu
def test_uniform_list_equals_the_uniform_batch_calls():
    import torch

    streams = [synth.synth_jpeg(1280, 720, 900 + i, 85, "420", 8) for i in range(12)]
    row = 1280 * 3
    d = api.Decoder(0)
    d.decode_batch_device(streams, 1)
    ref = torch.zeros((12, 720, row), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(ref.data_ptr(), 720 * row, row)
    assert d.decode_ragged_device(streams) == [0] * 12
    out = torch.zeros((12, 720, row), dtype=torch.uint8, device="cuda")
    d.reconstruct_ragged_device([out[i].data_ptr() for i in range(12)], [row] * 12)
    st = d.ragged_stats()
    assert st["ragged"] == 12 and st["entropy_launches"] == 1 and st["walk_launches"] == 0 and st["recon_launches"] == 1 and st["recon_single"] == 0
    assert torch.equal(out, ref)
    # a uniform decode on the same object takes the coefficient store: the ragged batch is over (and its statistics are not
    # counted up by launches that were not its own)
    d.decode_batch_device(streams[:3], 1)
    assert d.ragged_stats() == st
    with pytest.raises(api.MijpegError) as e:
        d.reconstruct_ragged_device([out[i].data_ptr() for i in range(12)], [row] * 12)
    assert e.value.code == -1031  # MIJPEG_ERR_OBJECT_DOESNT_EXIST
    d.close()


@pytest.mark.gpu
def test_fallback_members(oracle):
    """What the group launches do not cover rides along through the single-image route: all pictures arrive, the damaged one
    with the single-image path's pixels and warning, garbage with its error code, and the statistics name exactly these."""
    good = [_encode(w, h, 40 + k, 85, layout, dri, False) for k, (w, h, layout, dri) in
            enumerate([(640, 480, "420", 4), (127, 129, "444", 0), (500, 375, "422", 1), (333, 200, "grey", 0), (1280, 720, "420", 0)])]
    base = synth.synth_jpeg(320, 240, 1, 85, "420", 2)
    damaged = bytearray(base)
    damaged[len(damaged) // 2] ^= 0x5A
    damaged[len(damaged) // 2 + 1] = 0xFF
    damaged[len(damaged) // 2 + 2] = 0xD9  # an EOI in the middle of the data: restart intervals go missing
    damaged = bytes(damaged)
    garbage = bytes(np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8))
    extra = {"progressive": synth.synth_jpeg(200, 130, 3, 85, "420", 0, progressive=True), "p12": synth.to_12bit(synth.synth_jpeg(120, 90, 4, 85, "420", 0)),
             "440": golden_jpeg("ref_97x61_440"), "cmyk": golden_jpeg("pil_90x60_cmyk"), "damaged": damaged, "garbage": garbage}
    streams = good[:2] + [extra["progressive"], extra["p12"]] + good[2:4] + [extra["440"], extra["cmyk"], extra["damaged"]] + good[4:] + [extra["garbage"]]
    kinds = ["good"] * 2 + ["progressive", "p12"] + ["good"] * 2 + ["440", "cmyk", "damaged"] + ["good"] + ["garbage"]
    n = len(streams)
    # what the single-image path says about the two that are not plainly valid
    single = api.Decoder(0)
    single.read(damaged)
    damaged_pixels, damaged_warning = single.reconstruct(), single.last_warning()
    with pytest.raises(api.MijpegError) as e:
        single.read(garbage)
    garbage_code = e.value.code
    single.close()
    assert garbage_code < 0

    d = api.Decoder(0)
    status = d.decode_ragged_device(streams)
    assert [s != 0 for s in status] == [k == "garbage" for k in kinds]
    assert status[-1] == garbage_code
    with pytest.raises(api.MijpegError) as e:
        d.ragged_info(n - 1)
    assert e.value.code == garbage_code
    infos = [d.ragged_info(i) if kinds[i] != "garbage" else None for i in range(n)]
    with pytest.raises(ValueError):  # one destination per stream of the decode call, in error or not
        d.reconstruct_ragged_device([0] * (n - 1), [0] * (n - 1))
    pics, touched = _reconstruct_guarded(d, infos, (0, 4, 13))
    assert not any(touched)
    for i, pic in enumerate(pics):
        in_group, why = d.ragged_route(i)
        assert in_group == (kinds[i] == "good") and (why is None) == in_group, (i, kinds[i], why)
        if kinds[i] == "garbage":
            continue
        if kinds[i] == "damaged":
            assert np.array_equal(pic, damaged_pixels)
            assert d.ragged_warning(i) == damaged_warning and damaged_warning[1]
        else:
            exp = oracle.decode16(streams[i]) if kinds[i] == "p12" else oracle.decode(streams[i])
            assert pic.shape == exp.shape and np.array_equal(pic, exp), (i, kinds[i])
            assert d.ragged_warning(i) == (0, None)
    st = d.ragged_stats()
    assert st["images"] == n and st["ragged"] == 5 and st["fallbacks"] == 6 and st["errors"] == 1, st
    d.close()


@pytest.mark.gpu
def test_arithmetic_outlier_inside_a_group(oracle):
    """One stream whose coefficients lie far beyond the FAST gate (sum |c| q >= 16384: deltas of 255 under coefficients no
    encoder of pictures writes) inside a 4:2:0 group of ordinary ones: it runs the SAFE flavour in a launch of its own, the
    others keep their fast kernel, and all pictures are exact."""
    rng = np.random.default_rng(2024)
    f = api.frame_layout(272, 144, 3, (2, 1, 1), (2, 1, 1), [[255] * 64, [255] * 64])
    coef = rng.integers(-1000, 1001, size=f.coef_count).astype(np.int16)
    coef[rng.random(f.coef_count) < 0.5] = 0
    coef.reshape(-1, 64)[:, 0] = rng.integers(-500, 501, size=f.coef_count // 64)  # (DC differences a baseline table can code)
    outlier = api.encode_coefficients(f, coef, restart_interval=3)
    streams = [synth.synth_jpeg(500, 375, 60, 85, "420", 4), synth.synth_jpeg(272, 144, 61, 85, "420", 0), outlier, synth.synth_jpeg(129, 127, 62, 95, "420", 1)]
    exp = _decode_all(oracle, streams)
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams) == [0] * 4
    infos = [d.ragged_info(i) for i in range(4)]
    assert [int(x.fast_arith) for x in infos] == [1, 1, 0, 1] and max(infos[2].range_max[:3]) >= 16384
    pics, touched = _reconstruct_guarded(d, infos, (0, 4, 13))
    st = d.ragged_stats()
    assert st["ragged"] == 4 and st["fallbacks"] == 0 and st["entropy_launches"] == 1 and st["recon_launches"] == 2 and st["recon_single"] == 0, st
    for i in range(4):
        assert np.array_equal(pics[i], exp[i]), i
    assert not any(touched)
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["device", "host"])
def test_every_interval_source_in_one_group(monkeypatch, walk):
    """One 4:4:4 group whose members get their intervals in three ways: a stream without restart markers that is walked (on the
    device, or with MIJPEG_DEVICE_WALK=0 on the host), one too small for a walk (64 x 64: the whole scan is one interval) and one
    with restart markers.  The walked one is 256 x 256, the smallest either walk takes: noise for the host's planner, which wants
    four 32 KiB segments, a picture for the device's (on the noise this group's launch is refused and its members take the
    single-image route).  One Huffman launch; walk launches only where the device walks.  The planes stay in HBM: range checks
    and pixels are compared with the host decoder's."""
    monkeypatch.setenv("MIJPEG_DEVICE_WALK", "1" if walk == "device" else "0")
    walked = synth.synth_jpeg(256, 256, 21, 95, "444", 0) if walk == "device" else noise_jpeg(256, 256, 21, "444", 0)
    streams = [walked, noise_jpeg(64, 64, 22, "444", 0), noise_jpeg(200, 136, 23, "444", 3)]
    want = host_decodes(streams)
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams) == [0] * 3
    st = d.ragged_stats()
    assert st["ragged"] == 3 and st["fallbacks"] == 0 and st["entropy_launches"] == 1, (st, [d.ragged_route(i) for i in range(3)])
    assert (st["walk_launches"] > 0) == (walk == "device"), st
    infos = [d.ragged_info(i) for i in range(3)]
    for i, f in enumerate(infos):
        assert d.ragged_route(i) == (True, None)
        assert list(f.range_max) == want[i][1] and int(f.fast_arith) == want[i][2], i
    pics, touched = _reconstruct_guarded(d, infos, (0, 4, 13))
    assert not any(touched)
    for i in range(3):
        assert np.array_equal(pics[i], want[i][0]), i
    d.close()


@pytest.mark.gpu
def test_single_component_with_sampling_factors_leaves_the_groups():
    """A frame whose only component has sampling factors 2 x 2 (40 x 24: its scan leaves blocks of its planes unwritten) is not
    decoded in a ragged launch: it takes the single-image route, which clears the planes first."""
    odd = grey_2x2_jpeg(40, 24, 5, 2)
    streams = [_encode(64, 64, 31, 85, "grey", 2, False), odd]
    want = host_decodes(streams)
    d = api.Decoder(0)
    assert d.decode_ragged_device(streams) == [0, 0]
    assert d.ragged_route(0) == (True, None)
    assert d.ragged_route(1) == (False, "no layout group for this frame: 8-bit sequential 4:2:0, 4:2:2, 4:4:4 and grey frames have one")
    infos = [d.ragged_info(i) for i in range(2)]
    assert list(infos[1].range_max) == want[1][1]
    pics, touched = _reconstruct_guarded(d, infos, (0, 4))
    assert not any(touched)
    for i in range(2):
        assert np.array_equal(pics[i], want[i][0].reshape(pics[i].shape)), i
    st = d.ragged_stats()
    assert st["ragged"] == 1 and st["fallbacks"] == 1 and st["errors"] == 0, st
    d.close()


MIXED_WORKER = textwrap.dedent("""
    import sys
    sys.path.insert(0, %r)
    import numpy as np
    import torch.distributed as dist
    from libjpeg_amd import batch, synth
    from oracle import oracle as O

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    shapes = [(640, 480, "420", 4), (127, 129, "444", 0), (500, 375, "422", 1), (375, 500, "420", 0), (1000, 3, "444", 7), (1280, 720, "420", 0), (64, 64, "422", 0)]
    streams = [synth.synth_jpeg(w, h, 500 + k, 85, sub, dri) for k, (w, h, sub, dri) in enumerate(shapes)]
    out = batch.decode_mixed(streams, 0, rank, world)
    mine = [i for i, t in enumerate(out) if t is not None]
    for i in mine:
        assert np.array_equal(out[i].cpu().numpy(), O.decode(streams[i])), i
    print("RANK", rank, "pictures", mine, "ok", flush=True)
    dist.barrier()
    dist.destroy_process_group()
""")


@pytest.mark.gpu
def test_decode_mixed(oracle, tmp_path):
    """batch.decode_mixed: one tensor per picture, equal to the oracle; on two gloo ranks every picture goes to exactly one rank."""
    from libjpeg_amd import batch

    streams = [_encode(w, h, 80 + k, q, layout, dri, k % 2 == 0) for k, (w, h, q, layout, dri) in
               enumerate([(640, 480, 85, "420", 0), (17, 33, 99, "444", 1), (333, 2049, 50, "422", 4), (128, 128, 95, "grey", 0)])]
    streams.append(synth.synth_jpeg(200, 130, 3, 85, "420", 0, progressive=True))
    garbage = bytes(np.random.default_rng(6).integers(0, 256, 100, dtype=np.uint8))
    out = batch.decode_mixed(streams[:2] + [garbage] + streams[2:], 0)
    assert isinstance(out[2], api.MijpegError) and out[2].code < 0  # a stream in error does not stop the others
    for t, s in zip(out[:2] + out[3:], streams):
        assert str(t.device).startswith("cuda") and np.array_equal(t.cpu().numpy(), oracle.decode(s))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "mixed_worker.py"
    script.write_text(MIXED_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    assert "pictures [0, 2, 4, 6] ok" in outs[0] and "pictures [1, 3, 5] ok" in outs[1]

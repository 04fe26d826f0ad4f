"""12-bit encoder direction on the device: the precision-12 flavours of the forward kernels (forward.hip) against the coefficients in
the streams the reference encoder wrote (tests/golden/enc12) and against the validated numpy restatement (tests/enc12_util.py),
mijpeg_encode_image16 with the device and the host entropy coder, mijpeg_encode_batch_device at precision 12, and the command line
tool with 16-bit PNMs.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import enc12_util as U
from conftest import ROOT
from libjpeg_amd import api

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (33, 17), (75, 45), (129, 71)]
# (three 16-bit samples per pixel: lines of an odd width never start dword-aligned, so those sizes go through fdct_blocks_kernel
# alone; an even width for the interior kernels of every layout, one beyond 128 x 128 with edge strips for the tile kernel)
SIZES_FORWARD = SIZES + [(72, 40), (136, 152)]
LAYOUT_NAMES = ["444", "420", "422", "440", "411", "grey"]
EXE = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _torch():
    import torch

    return torch


def _to_device(frames: np.ndarray):
    """uint16 samples -> a device tensor (as int16: the same bits)."""
    return _torch().from_numpy(np.ascontiguousarray(frames, np.uint16).view(np.int16)).cuda()


def _forward(frames: np.ndarray, hs, vs, quants, ycbcr: bool):
    """mijpeg_launch_forward at precision 12 on (n, h, w[, 3]) pictures, every component on its own quantiser table: [(n, bh, bw, 64)]
    per component."""
    torch = _torch()
    n, h, w = frames.shape[:3]
    nc = 1 if frames.ndim == 3 else 3
    info = api.frame_layout(w, h, nc, hs, vs, quants, quant_index=list(range(nc)), ycbcr=1 if ycbcr else 0, precision=12)
    px = _to_device(frames)
    coef = torch.full((n, int(info.coef_count)), 0x5A5A, dtype=torch.int16, device="cuda")
    api.launch_forward(info, px.data_ptr(), coef.data_ptr(), n, w * nc * 2, h * w * nc * 2, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = coef.cpu().numpy()
    return info, [out[:, info.coef_offset[c]:info.coef_offset[c] + info.blocks_w[c] * info.blocks_h[c] * 64].reshape(n, info.blocks_h[c], info.blocks_w[c], 64)
                  for c in range(nc)]


def _check_planes(got, exp, w, h, info, frame, what):
    """Blocks that cover samples equal, MCU padding blocks zero."""
    for c in range(len(exp)):
        nbx, nby = U.covered_blocks(w, h, info.subx[c], info.suby[c])
        g = got[c][frame]
        assert np.array_equal(g[:nby, :nbx], exp[c][:nby, :nbx]), (what, c, np.argwhere(g[:nby, :nbx] != exp[c][:nby, :nbx])[:4].tolist())
        assert not g[nby:].any() and not g[:, nbx:].any(), (what, c, "padding blocks")


@pytest.mark.parametrize("key", sorted(U.CASES))
def test_forward_kernels_give_the_goldens_coefficients(key):
    w, h, layout, _, _, _, extra = U.CASES[key]
    oi, planes = U.golden_coefficients(key)
    hs, vs = U.LAYOUTS[layout][0]
    ycbcr = "-c" not in extra
    img = U.case_image(key)
    if layout == "grey":
        img = img[..., 0]
    other = np.ascontiguousarray(img[::-1, ::-1])  # a second frame in the same launch
    quants = [U.oracle_quant(oi, c) for c in range(oi.ncomp)]
    info, got = _forward(np.stack([img, other]), hs, vs, quants, ycbcr)
    _check_planes(got, planes, w, h, info, 0, key)
    _check_planes(got, U.forward12(other, hs, vs, quants, ycbcr), w, h, info, 1, key + " (second frame)")


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("w,h", SIZES_FORWARD)
def test_forward_kernels_against_the_restatement(w, h, layout):
    rng = np.random.default_rng(w * 1000 + h + len(layout))
    hs, vs = U.LAYOUTS[layout][0]
    shape = (h, w) if layout == "grey" else (h, w, 3)
    noise = rng.integers(0, 4096, shape).astype(np.uint16)
    saturated = (rng.integers(0, 2, shape) * 4095).astype(np.uint16)
    quants = [rng.integers(1, 256, 64).astype(np.uint16) for _ in hs]
    info, got = _forward(np.stack([noise, saturated]), hs, vs, quants, True)
    for f, img in enumerate((noise, saturated)):
        _check_planes(got, U.forward12(img, hs, vs, quants, True), w, h, info, f, (w, h, layout, f))


def _sof(data: bytes):
    i = data.find(b"\xff\xc1")
    assert i > 0 and b"\xff\xc0" not in data[:i]
    return data[i + 4]


def _check_stream(dec, oracle, data, img, layout, ri):
    """An encoded stream: SOF1 / P = 12, the restatement's coefficients with the stream's own tables, and the library's 12-bit
    decode of it is the oracle's."""
    h, w = img.shape[:2]
    assert _sof(data) == 12
    oi, planes = oracle.decode_coefficients(data)
    assert (oi.width, oi.height, oi.precision, oi.restart_interval) == (w, h, 12, ri)
    hs, vs = U.LAYOUTS[layout][0]
    exp = U.forward12(img, hs, vs, [U.oracle_quant(oi, c) for c in range(oi.ncomp)], True)
    for c in range(oi.ncomp):
        nbx, nby = U.covered_blocks(w, h, oi.subx[c], oi.suby[c])
        assert np.array_equal(planes[c][:nby, :nbx], exp[c][:nby, :nbx]), c
    f = dec.read(data)
    assert f.precision == 12
    out = dec.reconstruct()
    assert out.dtype == np.uint16 and np.array_equal(out.reshape(h, w, -1), np.asarray(oracle.decode16(data)).reshape(h, w, -1))
    return oi


@pytest.mark.parametrize("ri", [0, 1, 5])
@pytest.mark.parametrize("w,h", SIZES + [(72, 40)])
def test_encode_image16_device_coder_writes_the_host_coders_bytes(dec, oracle, w, h, ri):
    layout = LAYOUT_NAMES[(w + ri) % len(LAYOUT_NAMES)]
    img = U.synth12(w, h, w + ri, 1 if layout == "grey" else 3)
    if layout == "grey":
        img = img[..., 0]
    sub = "444" if layout == "grey" else layout
    gpu = dec.encode(img, 85, sub, ri, coder="gpu")
    host = dec.encode(img, 85, sub, ri, coder="host")
    assert gpu == host, (len(gpu), len(host))
    _check_stream(dec, oracle, gpu, img, layout, ri)


@pytest.mark.parametrize("content", ["pixel_checker", "block_checker"])
def test_checkerboards_at_quality_100(dec, oracle, content):
    """The widest AC coefficients (category 14) and DC differences (category 15) through both coders."""
    key = "444_64x40_q100_" + content
    img = U.case_image(key)
    gpu = dec.encode(img, 100, "444", coder="gpu")
    assert gpu == dec.encode(img, 100, "444", coder="host")
    _check_stream(dec, oracle, gpu, img, "444", 0)
    _, planes = oracle.decode_coefficients(gpu)
    _, gold = U.golden_coefficients(key)
    assert all(np.array_equal(a, b) for a, b in zip(planes, gold))  # (64 x 40 at 4:4:4: no padding blocks)


@pytest.mark.parametrize("q", [2, 30, 85, 100])
def test_quantiser_tables_are_the_reference_encoders_at_12_bits(dec, oracle, q):
    key = {2: "420_64x40_q2", 30: "420_64x40_q30", 85: "420_80x48", 100: "420_64x40_q100"}[q]
    gold, _ = U.golden_coefficients(key)
    img = U.case_image(key)
    data = dec.encode(img, q, "420")
    oi, planes = oracle.decode_coefficients(data)
    assert list(oi.tq[:3]) == [0, 0, 0] and list(oi.quant[0]) == list(gold.quant[0])
    _, gplanes = U.golden_coefficients(key)
    for c in range(3):
        nbx, nby = U.covered_blocks(oi.width, oi.height, oi.subx[c], oi.suby[c])
        assert np.array_equal(planes[c][:nby, :nbx], gplanes[c][:nby, :nbx]), c


@pytest.mark.parametrize("layout,q,w,h", [("420", 85, 75, 45), ("444", 30, 33, 17), ("422", 100, 129, 71), ("grey", 85, 75, 45), ("411", 2, 33, 17)])
def test_live_reference_encoder_has_the_same_tables_and_coefficients(dec, oracle, layout, q, w, h):
    if not oracle.have_reference():
        pytest.skip("the reference binary is not built here (the goldens stand in for it)")
    img = U.synth12(w, h, q + w, 1 if layout == "grey" else 3)
    sub = U.LAYOUTS[layout][1]
    rc, ref, err = U.reference_encode12(img, ["-q", str(q)] + (["-s", sub] if sub else []))
    assert rc == 0 and ref, err
    data = dec.encode(img[..., 0] if layout == "grey" else img, q, "444" if layout == "grey" else layout)
    ri, rp = oracle.decode_coefficients(ref)
    mi, mp = oracle.decode_coefficients(data)
    assert ri.precision == mi.precision == 12 and ri.ncomp == mi.ncomp
    for c in range(ri.ncomp):
        assert list(ri.quant[ri.tq[c]]) == list(mi.quant[mi.tq[c]])
        nbx, nby = U.covered_blocks(w, h, ri.subx[c], ri.suby[c])
        assert np.array_equal(rp[c][:nby, :nbx], mp[c][:nby, :nbx]), c


def test_batch_device_at_precision_12_equals_the_single_image_call(dec):
    torch = _torch()
    w, h, n, ri = 272, 144, 3, 4
    imgs = [U.synth12(w, h, 40 + i) for i in range(n)]
    single = [dec.encode(im, 85, "420", ri) for im in imgs]
    tables = U.golden_coefficients("420_272x144_z4")[0].quant[0]  # the tables of -q 85 at 12 bits
    info = api.frame_layout(w, h, 3, (2, 1, 1), (2, 1, 1), [list(tables)], quant_index=[0, 0, 0], precision=12)
    px = _to_device(np.stack(imgs))
    coef = torch.empty((n, int(info.coef_count)), dtype=torch.int16, device="cuda")
    for opt in (False, True):  # (ignored at precision 12)
        streams = dec.encode_batch_device(info, px.data_ptr(), coef.data_ptr(), n, w * 6, h * w * 6, restart_mcus=ri, optimize=opt)
        assert [len(s) for s in streams] == [len(s) for s in single]
        assert streams == single


def _run_cli(args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("layout", ["420", "grey"])
def test_cli_encodes_16_bit_pnm(oracle, tmp_path, layout):
    assert os.path.exists(EXE), "libjpeg_amd/bin/jpeg not built (run __graft_entry__.build())"
    w, h = 80, 48
    img = U.synth12(w, h, 1, 1 if layout == "grey" else 3)
    src, dst = tmp_path / "in.pnm", tmp_path / "out.jpg"
    U.write_pnm16(str(src), img)
    sub = ["-s", "1x1,2x2,2x2"] if layout == "420" else []
    r = _run_cli(["-q", "85", *sub, "-z", "3", "-d", "0", str(src), str(dst)])
    assert r.returncode == 0, r.stderr
    data = dst.read_bytes()
    assert _sof(data) == 12
    oi, planes = oracle.decode_coefficients(data)
    assert (oi.width, oi.height, oi.restart_interval) == (w, h, 3)
    hs, vs = U.LAYOUTS[layout][0]
    exp = U.forward12(img, hs, vs, [U.oracle_quant(oi, c) for c in range(oi.ncomp)], True)
    for c in range(oi.ncomp):
        nbx, nby = U.covered_blocks(w, h, oi.subx[c], oi.suby[c])
        assert np.array_equal(planes[c][:nby, :nbx], exp[c][:nby, :nbx]), c
    if layout == "420":  # the same picture is a golden: the reference's tables and coefficients
        gi, gp = U.golden_coefficients("420_80x48")
        assert list(gi.quant[0]) == list(oi.quant[0])
        for c in range(3):
            nbx, nby = U.covered_blocks(w, h, oi.subx[c], oi.suby[c])
            assert np.array_equal(planes[c][:nby, :nbx], gp[c][:nby, :nbx]), c


def test_cli_refusals(tmp_path):
    img = U.synth12(16, 16, 3)
    src, dst = tmp_path / "in.ppm", tmp_path / "out.jpg"
    U.write_pnm16(str(src), img)
    r = _run_cli(["-q", "85", "-bl", "-d", "0", str(src), str(dst)])  # baseline Huffman coding only supports 8bpp scans
    assert r.returncode != 0 and "-1024" in r.stderr, r.stderr
    U.write_pnm16(str(src), np.minimum(img, 1023), maxval=1023)
    r = _run_cli(["-q", "85", "-d", "0", str(src), str(dst)])
    assert r.returncode != 0 and "maxval 255 or 4095" in r.stderr, r.stderr

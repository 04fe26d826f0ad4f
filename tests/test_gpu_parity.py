"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (libjpeg_amd/libmijpeg.so), against
  * the committed golden vectors (pixels produced by the real reference binary), and
  * the pinned CPU oracle (oracle/jpeg_oracle.c) on seeded inputs, including full-size 4K / 8K frames,
    tile-edge sizes, every sampling layout, both arithmetic flavours, and adversarial coefficients.
Bar: bit-exact (integer path).  No test in here can pass on a CPU fallback: the product has none."""
import hashlib

import numpy as np
import pytest

from conftest import BIG_CASES, MANIFEST, P12_CASES, SMALL_CASES, XT_CASES, big_jpeg, golden_jpeg, golden_pixels
from libjpeg_amd import api, synth
from route_streams import grey_2x2_jpeg, host_decodes, noise_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = api.Decoder(0)
    yield d
    d.close()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE, api.FLAG_FORCE_GENERIC, api.FLAG_FORCE_GENERIC | api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_golden_reference_vectors(dec, name, flags):
    ent = MANIFEST[name]
    dec.read(golden_jpeg(name))
    out = dec.reconstruct(flags)
    assert out.shape == (ent["height"], ent["width"], ent["channels"])
    exp = golden_pixels(name)
    if exp is not None:
        bad = int((out != exp).sum())
        assert bad == 0, f"{bad} differing samples, first at {np.argwhere(out != exp)[:4].tolist()}"
    assert _sha(out) == ent["pixels_sha256"]


# sizes straddling the 128-pixel tile and 16-pixel MCU boundaries of the fused 4:2:0 kernel
EDGE_SIZES = [(127, 127), (128, 128), (129, 129), (255, 130), (257, 127), (130, 258), (1, 1), (2, 3), (15, 17),
              (16, 16), (17, 15), (143, 97), (384, 256), (400, 144)]


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("w,h", EDGE_SIZES)
def test_fused420_tile_edges_vs_oracle(dec, oracle, w, h, flags):
    data = synth.synth_jpeg(w, h, 100 + w + h, 90, "420", (w * h) % 4)
    f = dec.read(data)
    assert api.kernel_name(f, flags) == ("fused420_kernel" if flags else "fused420p_kernel")  # packed chroma flavour when the range allows
    out = dec.reconstruct(flags)
    exp = oracle.decode(data)
    bad = int((out != exp).sum())
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(out != exp)[:4].tolist()}"


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("w,h", EDGE_SIZES + [(512, 512), (1920, 1080)])
def test_fused444_vs_oracle(dec, oracle, w, h, flags):
    data = synth.synth_jpeg(w, h, 300 + w + h, 88, "444", (w + h) % 5)
    f = dec.read(data)
    # the dedicated kernel only exists in the fast flavour; FORCE_SAFE must route to the one-pass tile kernel (SAFE arithmetic)
    assert api.kernel_name(f, flags) == ("fused444_kernel" if flags == 0 else "fused_tile_kernel")
    out = dec.reconstruct(flags)
    exp = oracle.decode(data)
    bad = int((out != exp).sum())
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(out != exp)[:4].tolist()}"


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("w,h", EDGE_SIZES + [(512, 512), (1920, 1080), (1000, 999)])
def test_fused422_vs_oracle(dec, oracle, w, h, flags):
    data = synth.synth_jpeg(w, h, 500 + w + h, 87, "422", (w + 2 * h) % 5)
    f = dec.read(data)
    # the dedicated kernel only exists in the fast flavour; FORCE_SAFE must route to the one-pass tile kernel (SAFE arithmetic)
    assert api.kernel_name(f, flags) == ("fused422_kernel" if flags == 0 else "fused_tile_kernel")
    out = dec.reconstruct(flags)
    exp = oracle.decode(data)
    bad = int((out != exp).sum())
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(out != exp)[:4].tolist()}"


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("w,h", EDGE_SIZES + [(512, 512), (1920, 1080), (999, 1000)])
def test_fused440_vs_oracle(dec, oracle, w, h, flags):
    """4:4:0 (Y 1x2 over chroma: a losslessly rotated 4:2:2 picture).  Pillow cannot write the layout: the streams come from
    this library's own encoder, whose output the reference decoder (the oracle) reads like any other."""
    ri = (w + 2 * h) % 5
    data = dec.encode(synth.synth_image(w, h, 700 + w + h), 87, "440", ri, ri == 2)
    f = dec.read(data)
    assert (f.hsamp[0], f.vsamp[0], f.hsamp[1], f.vsamp[1]) == (1, 2, 1, 1)
    # the dedicated kernel only exists in the fast flavour; FORCE_SAFE must route to the one-pass tile kernel (SAFE arithmetic)
    assert api.kernel_name(f, flags) == ("fused440_kernel" if flags == 0 else "fused_tile_kernel")
    out = dec.reconstruct(flags)
    exp = oracle.decode(data)
    bad = int((out != exp).sum())
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(out != exp)[:4].tolist()}"


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("w,h", EDGE_SIZES + [(512, 512), (1920, 1080), (1003, 998), (129, 40), (31, 300), (33, 9)])
def test_fused411_vs_oracle(dec, oracle, w, h, flags):
    """4:1:1 (chroma subsampled 4x1): the four-fold horizontal core of upsampling/upsampler.cpp:367-387 in a fused kernel.
    Streams from this library's own encoder (Pillow cannot write the layout) and saturated content among them."""
    ri = (w + 2 * h) % 5
    img = synth.synth_image(w, h, 800 + w + h)
    if (w + h) % 3 == 0:
        img = img.copy()
        img[:, w // 3: w // 3 + 7] = (255, 0, 0)
        img[:, w // 2: w // 2 + 3] = (0, 0, 255)
    data = dec.encode(img, 87, "411", ri, ri == 2)
    f = dec.read(data)
    assert (f.hsamp[0], f.vsamp[0], f.hsamp[1], f.vsamp[1]) == (4, 1, 1, 1)
    worst = max(f.range_max[1], f.range_max[2])
    assert api.kernel_name(f, flags) == ("fused411_kernel" if flags == 0 and worst < 8190 else "fused_tile_kernel")
    out = dec.reconstruct(flags)
    exp = oracle.decode(data)
    bad = int((out != exp).sum())
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(out != exp)[:4].tolist()}"


def test_fused440_packed_chroma_gate(dec, oracle):
    """Same 16-bit filter arithmetic and gate as the other packed flavours; batches of frames through the C ABI."""
    img = np.zeros((400, 272, 3), np.uint8)
    img[:130] = (255, 0, 0)
    img[130:260] = (0, 0, 255)
    img[260:] = (0, 255, 0)
    img[:, 100:150] = (255, 255, 0)
    seen = set()
    for q in (50, 75, 90, 100):
        data = dec.encode(img, q, "440", 3)
        f = dec.read(data)
        name = api.kernel_name(f)
        worst = max(f.range_max[1], f.range_max[2])
        assert f.fast_arith == 1
        assert name == ("fused440_kernel" if worst < 2047 else "fused440_kernel<wide>" if worst < 8190 else "fused_tile_kernel")
        seen.add(name)
        assert np.array_equal(dec.reconstruct(), oracle.decode(data)), q
    assert "fused440_kernel<wide>" in seen  # saturated graphics lie beyond the packed gate: 32-bit filters, still fused
    rng = np.random.default_rng(16)
    img = rng.integers(0, 256, (208, 144, 3)).astype(np.uint8)
    for q in (60, 95):
        data = dec.encode(img, q, "440")
        dec.read(data)
        assert np.array_equal(dec.reconstruct(), oracle.decode(data))


@pytest.mark.parametrize("w,h", EDGE_SIZES + [(512, 512), (1920, 1080), (1001, 999)])
def test_fused_single_component_vs_oracle(dec, oracle, w, h):
    """Grey scale frames: one lane per block, identity transformation; FORCE_GENERIC and FORCE_SAFE take the two-kernel path."""
    img = synth.synth_image(w, h, 900 + w, channels=1)
    for q, ri in ((85, 0), (35, 3)):
        data = synth.encode_jpeg(img, q, "444", restart_mcus=ri)
        f = dec.read(data)
        assert f.components == 1
        assert api.kernel_name(f) == "fused1_kernel" and api.kernel_name(f, api.FLAG_FORCE_SAFE) == "fused_tile_kernel"
        exp = oracle.decode(data)
        out = dec.reconstruct()
        assert np.array_equal(out.squeeze(), exp.squeeze())
        assert np.array_equal(dec.reconstruct(api.FLAG_FORCE_GENERIC).squeeze(), exp.squeeze())


def test_fused422_packed_chroma_gate(dec, oracle):
    """Same 16-bit filter arithmetic, hence the same gate, as the packed 4:2:0 flavour; beyond it the generic kernels."""
    img = np.zeros((272, 400, 3), np.uint8)
    img[:, :130] = (255, 0, 0)
    img[:, 130:260] = (0, 0, 255)
    img[:, 260:] = (0, 255, 0)
    img[100:150] = (255, 255, 0)
    seen = set()
    for q in (50, 75, 90, 100):
        data = synth.encode_jpeg(img, q, "422", restart_mcus=3)
        f = dec.read(data)
        name = api.kernel_name(f)
        worst = max(f.range_max[1], f.range_max[2])
        assert f.fast_arith == 1
        assert name == ("fused422_kernel" if worst < 2047 else "fused422_kernel<wide>" if worst < 8190 else "fused_tile_kernel")
        seen.add(name)
        assert np.array_equal(dec.reconstruct(), oracle.decode(data)), q
    assert "fused422_kernel<wide>" in seen  # saturated graphics lie beyond the packed gate: 32-bit filters, still fused
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (144, 208, 3)).astype(np.uint8)
    for q in (60, 95):
        data = synth.encode_jpeg(img, q, "422")
        dec.read(data)
        assert np.array_equal(dec.reconstruct(), oracle.decode(data))


def test_fused444_range_gate(dec, oracle):
    """Chroma samples are kept as packed int16 in the fused 4:4:4 kernel: a frame whose range check does not bound
    them below 2^15 must take the generic path (and still be exact)."""
    data = synth.synth_jpeg(96, 64, 11, 1, "444", 0)  # quality 1: deltas of 255, huge dequantised sums
    f = dec.read(data)
    name = api.kernel_name(f)
    assert (name == "fused444_kernel") == (f.fast_arith == 1 and f.range_max[1] < 8190 and f.range_max[2] < 8190)
    assert np.array_equal(dec.reconstruct(), oracle.decode(data))


def test_fused420_packed_chroma_gate(dec, oracle):
    """The packed flavour of the fused 4:2:0 kernel filters (Cb, Cr) pairs in 16 bits; frames whose range check does not
    keep 4 * (a + 3 b + r) inside int16 take the 32-bit flavour: saturated graphics right at and beyond the gate."""
    img = np.zeros((272, 400, 3), np.uint8)
    img[:, :130] = (255, 0, 0)
    img[:, 130:260] = (0, 0, 255)
    img[:, 260:] = (0, 255, 0)
    img[100:150] = (255, 255, 0)
    seen = set()
    for q in (50, 75, 90, 100):
        data = synth.encode_jpeg(img, q, "420", restart_mcus=3)
        f = dec.read(data)
        name = api.kernel_name(f)
        packed = f.fast_arith == 1 and f.range_max[1] < 2047 and f.range_max[2] < 2047
        assert name == ("fused420p_kernel" if packed else "fused420_kernel")
        seen.add(name)
        assert np.array_equal(dec.reconstruct(), oracle.decode(data)), q
    assert "fused420_kernel" in seen  # the gate was exercised
    # moderately coloured content right below the gate stays exact in 16 bits
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (144, 208, 3)).astype(np.uint8)
    for q in (60, 95):
        data = synth.encode_jpeg(img, q, "420")
        dec.read(data)
        assert np.array_equal(dec.reconstruct(), oracle.decode(data))


@pytest.mark.parametrize("sub", ["444", "422", "420"])
@pytest.mark.parametrize("w,h", [(640, 360), (333, 211)])
def test_generic_path_vs_oracle(dec, oracle, w, h, sub):
    data = synth.synth_jpeg(w, h, 7, 80, sub, 3)
    dec.read(data)
    out = dec.reconstruct(api.FLAG_FORCE_GENERIC)
    assert np.array_equal(out, oracle.decode(data))


def test_no_color_transform_flag(dec, oracle):
    # CLI -c: JPGTAG_MATRIX_LTRAFO = NONE -> identity transformation on a YCbCr stream
    data = golden_jpeg("ref_80x48_420")
    dec.read(data)
    out = dec.reconstruct(api.FLAG_NO_COLOR_TRANSFORM)
    assert np.array_equal(out, oracle.decode(data, use_ycbcr=0))


def test_stripe_service_like_cmd_reconstruct(dec, oracle):
    # cmd/reconstruct.cpp:334-342: DisplayRectangle per 8-line stripe, top down
    data = golden_jpeg("pil_200x120_420_dri8")
    f = dec.read(data)
    out = np.zeros((f.height, f.width, 3), np.uint8)
    for y in range(0, f.height, 8):
        dec.reconstruct_rect(0, y, f.width - 1, min(y + 7, f.height - 1), out=out)
    assert np.array_equal(out, golden_pixels("pil_200x120_420_dri8"))
    # a sub-rectangle and a single component into a planar destination
    part = np.zeros_like(out)
    dec.reconstruct_rect(17, 9, 120, 77, out=part)
    assert np.array_equal(part[9:78, 17:121], out[9:78, 17:121]) and part[:9].sum() == 0


@pytest.mark.parametrize("name", BIG_CASES)
def test_full_size_frames(dec, oracle, name):
    """BASELINE configs 2/3: 4K and 8K 4:2:0 (with and without DRI) bit-exact vs the reference."""
    ent = MANIFEST[name]
    data = big_jpeg(name)
    pinned_by_reference = data is not None
    if data is None:  # other Pillow build: same recipe, compare against the pinned oracle instead
        data = synth.synth_jpeg(ent["width"], ent["height"], ent["seed"], ent["quality"], ent["sub"], ent["dri"])
    f = dec.read(data)
    assert f.fast_arith == 1
    out = dec.reconstruct()
    if pinned_by_reference:
        assert _sha(out) == ent["pixels_sha256"]
    exp = oracle.decode(data)
    assert np.array_equal(out, exp)
    # the safe flavour must agree too
    assert np.array_equal(dec.reconstruct(api.FLAG_FORCE_SAFE), exp)


# ------------------------------------------------------------------------------------------------------
# JPEG XT profile C (BASELINE config 5) and 12-bit frames
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", XT_CASES)
def test_xt_profile_c_golden(dec, oracle, name):
    """Half-float codes from the GPU, expanded exactly (cmd/iohelpers.hpp:60-77), must equal bit for bit the floats the
    reference wrote into its PFM; tolerance 0."""
    ent = MANIFEST[name]
    f = dec.read(golden_jpeg(name))
    assert f.xt == 1 and f.is_float == 1 and f.sample_bytes == 2
    # 8-bit 4:2:0 legacy + 4:4:4 residual has fused kernels -- 12-bit residual: fusedxt420_kernel, residual with hidden bits
    # (-rR n: 13..16 bits, int32 coefficients, the reference's wrapping IDCT<4,QUAD>): fusedxtw420_kernel (round 3); hidden
    # bits in the legacy frame (-R n) and 4:4:4 / 4:2:2 legacy frames take the three-kernel path
    fused = "_420" in name and "_R" not in name
    assert api.kernel_name(f, xt=dec.xt_params()) == (("fusedxtw420_kernel" if "_rR" in name else "fusedxt420_kernel") if fused else
                                                      "idct_planes_kernel+xt_merge_kernel")
    codes = dec.reconstruct()
    assert codes.dtype == np.uint16 and codes.shape == (ent["height"], ent["width"], 3)
    if fused:
        assert np.array_equal(codes, dec.reconstruct(api.FLAG_FORCE_GENERIC))
    exp_codes, _ = oracle.decode_xt(golden_jpeg(name))
    bad = int((codes != exp_codes).sum())
    assert bad == 0, f"{bad} differing half codes, first at {np.argwhere(codes != exp_codes)[:4].tolist()}"
    out = oracle.half_codes_to_float(codes)
    assert hashlib.sha256(np.ascontiguousarray(out, "<f4").tobytes()).hexdigest() == ent["pixels_sha256"]


@pytest.mark.parametrize("name", P12_CASES)
def test_12bit_golden(dec, oracle, name):
    ent = MANIFEST[name]
    f = dec.read(golden_jpeg(name))
    assert f.precision == 12 and f.sample_bytes == 2 and f.xt == 0
    out = dec.reconstruct()
    assert out.dtype == np.uint16
    exp = golden_pixels(name)
    assert np.array_equal(out, exp if exp is not None else oracle.decode16(golden_jpeg(name)))
    assert hashlib.sha256(np.ascontiguousarray(out, "<u2").tobytes()).hexdigest() == ent["pixels_sha256"]


def test_xt_hidden_residual_bits_1080p_vs_oracle(dec, oracle):
    """Config 5's -rR 4 variant on a frame of many tiles: fusedxtw420_kernel (int32 residual coefficients, the wrap of the
    reference's IDCT<4,QUAD> as a correction of the exact 32-bit transform, 20-bit residual samples) against the oracle's
    literal 64-bit restatement and against the three-kernel path."""
    if not oracle.have_reference():
        pytest.skip("needs oracle/_ref/jpeg to encode the HDR stream")
    for rr, size in ((4, (1920, 1080)), (3, (1000, 600))):
        data = oracle.reference_encode_hdr(synth.synth_hdr(size[0], size[1], 99 + rr),
                                           ["-r", "-q", "85", "-Q", "90", "-h", "-profile", "c", "-r12", "-rR", str(rr), "-s", "1x1,2x2,2x2"])
        f = dec.read(data)
        assert api.kernel_name(f, xt=dec.xt_params()) == "fusedxtw420_kernel"
        codes = dec.reconstruct()
        exp, _ = oracle.decode_xt(data)
        assert np.array_equal(codes, exp), rr
        assert np.array_equal(dec.reconstruct(api.FLAG_FORCE_GENERIC), exp), rr


def test_xt_4k_vs_oracle(dec, oracle):
    """BASELINE config 5 at its full 4K size (reference-encoded on the fly where the reference binary is available,
    i.e. in the build container; on the GPU box the committed small vectors above stand in)."""
    if not oracle.have_reference():
        pytest.skip("needs oracle/_ref/jpeg to encode the HDR stream")
    data = oracle.reference_encode_hdr(synth.synth_hdr(3840, 2160, 99),
                                       ["-r", "-q", "85", "-Q", "90", "-h", "-profile", "c", "-r12", "-s", "1x1,2x2,2x2"])
    f = dec.read(data)
    assert api.kernel_name(f, xt=dec.xt_params()) == "fusedxt420_kernel"
    codes = dec.reconstruct()
    exp, _ = oracle.decode_xt(data)
    assert np.array_equal(codes, exp)
    assert np.array_equal(dec.reconstruct(api.FLAG_FORCE_GENERIC), exp)
    # both codestreams (8-bit legacy, 12-bit residual; neither has restart markers) entropy-decoded on the device
    host = api.Decoder(0)
    host.read(data)
    dec.read(data, entropy="gpu")
    assert dec.entropy_used == "gpu" and dec.device_walk_rounds() > 0
    assert np.array_equal(dec.reconstruct(), exp)
    xg, xh = dec.xt_params(), host.xt_params()
    assert list(xg.residual.range_max) == list(xh.residual.range_max) and list(dec.info.range_max) == list(host.info.range_max)
    for c in range(3):
        assert np.array_equal(dec.coefficients(c), host.coefficients(c))
    host.close()


@pytest.mark.parametrize("w,h", [(136, 72), (250, 130), (1023, 517), (128, 128)])
def test_fused_xt_kernel_tile_edges(dec, oracle, w, h):
    """Fused profile C kernel at sizes that leave partial tiles / blocks and a residual plane narrower than the luma plane."""
    if not oracle.have_reference():
        pytest.skip("needs oracle/_ref/jpeg to encode the HDR stream")
    for q, rq in ((85, 90), (30, 60)):
        data = oracle.reference_encode_hdr(synth.synth_hdr(w, h, 5 + w), ["-r", "-q", str(q), "-Q", str(rq), "-h", "-profile", "c", "-r12", "-s", "1x1,2x2,2x2"])
        f = dec.read(data)
        assert api.kernel_name(f, xt=dec.xt_params()) == "fusedxt420_kernel"
        exp, _ = oracle.decode_xt(data)
        assert np.array_equal(dec.reconstruct(), exp)
        dec.read(data, entropy="auto")  # large enough: both codestreams on the device; otherwise the host decoder
        assert np.array_equal(dec.reconstruct(), exp)
        assert dec.entropy_used == ("gpu" if w * h > 200_000 else "host")


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def test_batch_launch_device_resident(oracle):
    """Stateless entry point: several frames' coefficients resident in HBM -> pixels in HBM, one launch."""
    torch = _torch()
    frames = []
    d = api.Decoder(0)
    for seed in (1, 2, 3):
        data = synth.synth_jpeg(400, 272, seed, 85, "420", 4)
        f = d.read(data)
        planes = [d.coefficients(c).reshape(-1) for c in range(3)]
        frames.append((data, np.concatenate(planes)))
    n = int(f.coef_count)
    coef = torch.from_numpy(np.stack([fr[1] for fr in frames])).cuda()
    row = 400 * 3
    out = torch.zeros((3, 272, row), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 3, row, 272 * row, n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = out.cpu().numpy().reshape(3, 272, 400, 3)
    for i, (data, _) in enumerate(frames):
        assert np.array_equal(res[i], oracle.decode(data)), f"frame {i}"
    d.close()


@pytest.mark.parametrize("sub", ["420", "422", "gray"])
def test_frames_beyond_32_bit_offsets_take_the_generic_kernels(oracle, sub):
    """The fused kernels address inside a frame with 32-bit offsets.  A destination whose lines are 1 MiB apart puts the last
    lines of a 4200-line picture beyond 4 GiB: such a launch must run the generic kernels (64-bit addressing), bit-exact,
    and must ask for their workspace; just below the limit the fused kernel runs into the same padded destination."""
    torch = _torch()
    w, h = 256, 4200
    nc = 1 if sub == "gray" else 3
    data = synth.encode_jpeg(synth.synth_image(w, h, 77, channels=nc), 85, "444" if sub == "gray" else sub, restart_mcus=4)
    exp = oracle.decode(data).reshape(h, w * nc)
    d = api.Decoder(0)
    f = d.read(data)
    coef = torch.from_numpy(np.concatenate([d.coefficients(c).reshape(-1) for c in range(nc)])).cuda()
    assert api.workspace_bytes(f, 1) == 0  # tightly packed lines: a fused kernel
    for stride, fused in ((1 << 20, False), (1 << 19, True)):
        out = torch.empty(h * stride, dtype=torch.uint8, device="cuda")
        if fused:
            api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, stride, h * stride, stream=torch.cuda.current_stream().cuda_stream)
        else:
            with pytest.raises(api.MijpegError):  # the generic kernels' workspace is missing
                api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, stride, h * stride, stream=torch.cuda.current_stream().cuda_stream)
            wsb = api.workspace_bytes(f, 1, api.FLAG_FORCE_GENERIC)
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, stride, h * stride, workspace=ws.data_ptr(), workspace_bytes=wsb,
                                   stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = out.view(h, stride)[:, :w * nc].cpu().numpy()
        assert np.array_equal(got, exp), (sub, stride)
        del out
    d.close()


@pytest.mark.parametrize("sub", ["420", "444", "422", "gray"])
def test_unaligned_output_stride(oracle, sub):
    """Bitmaps whose lines start at any byte address (row strides 393 = 131 * 3, 395, 400, 401; base addresses + 0, 1, 3, 6):
    the kernels store every full 8-pixel group as dwordx2 / dwordx4 wherever it lies (gfx950 does; rounds 1-2 fell to byte
    stores unless everything was 8-byte aligned); a padded destination must not be written outside the picture."""
    torch = _torch()
    d = api.Decoder(0)
    nc = 1 if sub == "gray" else 3
    data = synth.encode_jpeg(synth.synth_image(131, 77, 9, channels=nc), 85, "444" if sub == "gray" else sub)
    f = d.read(data)
    coef = torch.from_numpy(np.concatenate([d.coefficients(c).reshape(-1) for c in range(nc)])).cuda()
    d.close()
    exp = oracle.decode(data).reshape(77, 131 * nc)
    line = 131 * nc
    for row, base in ((line, 0), (line, 1), (line + 2, 3), (line + 7, 6), (line + 8, 0), (line + 8, 1)):
        buf = torch.full((77 * row + 16,), 0xAB, dtype=torch.uint8, device="cuda")
        api.launch_reconstruct(f, coef.data_ptr(), buf.data_ptr() + base, 1, row, 77 * row, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        flat = buf.cpu().numpy()
        res = flat[base:base + 77 * row].reshape(77, row)
        assert np.array_equal(res[:, :line], exp), f"row stride {row}, base + {base}"
        assert (res[:, line:] == 0xAB).all() and (flat[:base] == 0xAB).all() and (flat[base + 77 * row:] == 0xAB).all()


def test_unaligned_output_stride_whole_tiles(oracle):
    """The same with tiles that lie wholly inside the picture (every lane of a wave holds a whole block): lines at byte addresses
    1, 2, 3 mod 4 take the shifted store of the packed 4:2:0 kernel -- a DPP move from the left neighbour, v_alignbyte_b32, aligned
    stores, the row's first and last bytes by hand (store24_nt_shifted).  Widths 398 and 401 (packed lines of 1194 = 2 mod 4 and
    1203 = 3 mod 4 bytes), padded strides of every residue, base addresses + 0..3; nothing outside the picture is written."""
    torch = _torch()
    for w, h in ((398, 300), (401, 272)):
        d = api.Decoder(0)
        data = synth.synth_jpeg(w, h, 21 + w, 85, "420", 0)
        f = d.read(data)
        assert api.kernel_name(f) == "fused420p_kernel"
        coef = torch.from_numpy(np.concatenate([d.coefficients(c).reshape(-1) for c in range(3)])).cuda()
        d.close()
        line = w * 3
        exp = oracle.decode(data).reshape(h, line)
        for row, base in ((line, 0), (line, 1), (line, 2), (line, 3), (line + 1, 0), (line + 3, 2), (line + 5, 1), (line + 6, 0)):
            buf = torch.full((h * row + 16,), 0xAB, dtype=torch.uint8, device="cuda")
            api.launch_reconstruct(f, coef.data_ptr(), buf.data_ptr() + base, 1, row, h * row, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            flat = buf.cpu().numpy()
            res = flat[base:base + h * row].reshape(h, row)
            assert np.array_equal(res[:, :line], exp), f"{w}x{h}: row stride {row}, base + {base}: {np.count_nonzero(res[:, :line] != exp)} bytes differ"
            assert (res[:, line:] == 0xAB).all() and (flat[:base] == 0xAB).all() and (flat[base + h * row:] == 0xAB).all()


def test_staged_stores_at_every_dword_aligned_address(oracle):
    """Whole waves of whole blocks of the packed 4:2:0 kernel send their pixels through LDS and store 16 contiguous bytes per lane
    (F420P_STAGED, round 6): lines at every dword-aligned address -- base + 0, 4, 8, 12, strides 0, 4, 8, 12 mod 16 -- where those
    stores are not 16-byte aligned; widths with and without a partial last tile column; nothing outside the picture is written."""
    torch = _torch()
    for w, h in ((400, 300), (512, 272), (1024, 136)):
        d = api.Decoder(0)
        data = synth.synth_jpeg(w, h, 31 + w, 85, "420", 0)
        f = d.read(data)
        assert api.kernel_name(f) == "fused420p_kernel"
        coef = torch.from_numpy(np.concatenate([d.coefficients(c).reshape(-1) for c in range(3)])).cuda()
        d.close()
        line = w * 3
        exp = oracle.decode(data).reshape(h, line)
        for row, base in ((line, 0), (line, 4), (line + 4, 8), (line + 8, 12), (line + 12, 0), (line + 16, 4), (line + 20, 12)):
            buf = torch.full((h * row + 32,), 0xAB, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            api.launch_reconstruct(f, coef.data_ptr(), buf.data_ptr() + base, 1, row, h * row, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            flat = buf.cpu().numpy()
            res = flat[base:base + h * row].reshape(h, row)
            assert np.array_equal(res[:, :line], exp), f"{w}x{h}: row stride {row}, base + {base}: {np.count_nonzero(res[:, :line] != exp)} bytes differ"
            assert (res[:, line:] == 0xAB).all() and (flat[:base] == 0xAB).all() and (flat[base + h * row:] == 0xAB).all()


@pytest.mark.parametrize("generic", [False, True])
def test_adversarial_coefficients_safe_flavour(oracle, generic):
    """Coefficients no encoder would produce (|c| up to 32767, q up to 255): intermediates wrap around 2^32.
    The SAFE flavour must still reproduce the reference's LONG / QUAD arithmetic bit for bit."""
    torch = _torch()
    d = api.Decoder(0)
    data = synth.synth_jpeg(272, 144, 5, 85, "420", 0)
    f = d.read(data)
    d.close()
    rng = np.random.default_rng(2024)
    info, _ = oracle.decode_coefficients(data)
    planes = []
    for c in range(3):
        shape = (info.bh[c], info.bw[c], 64)
        p = rng.integers(-32768, 32768, size=shape).astype(np.int32)
        p[rng.random(shape) < 0.5] = 0
        planes.append(p)
    for t in range(4):
        for i in range(64):
            info.quant[t][i] = int(rng.integers(1, 256))
            f.quant[t][i] = info.quant[t][i]
    info.scan_state_valid = 0  # the tables edited here, not the ones the scans of `data` latched per component
    f.fast_arith = 0
    exp = oracle.reconstruct(info, planes)
    coef = torch.from_numpy(np.concatenate([p.astype(np.int16).reshape(-1) for p in planes])).cuda()
    row = 272 * 3
    out = torch.zeros((144, row), dtype=torch.uint8, device="cuda")
    flags = api.FLAG_FORCE_GENERIC if generic else 0
    ws_bytes = api.workspace_bytes(f, 1, flags)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, row, 144 * row, flags=flags,
                           workspace=ws.data_ptr(), workspace_bytes=ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = out.cpu().numpy().reshape(144, 272, 3)
    bad = int((res != exp).sum())
    assert bad == 0, f"{bad} differing samples"


@pytest.mark.parametrize("sub,chroma_budget,kernel", [("420", 2046, "fused420p_kernel"), ("422", 2046, "fused422_kernel"), ("440", 2046, "fused440_kernel"),
                                                      ("422", 8189, "fused422_kernel<wide>"), ("440", 8189, "fused440_kernel<wide>"),
                                                      ("420", 8189, "fused420_kernel"), ("444", 8189, "fused444_kernel"), ("411", 8189, "fused411_kernel")])
def test_extreme_coefficients_at_the_packed_chroma_gate(dec, oracle, sub, chroma_budget, kernel):
    """The packed flavours are admitted by sum |c| q < 2047 per chroma block, the int16 sample store of the 4:2:2 / 4:4:0 /
    4:4:4 kernels by < 8190.  Blocks that sit right at those bounds with every sign pattern (DC-only, single AC, dense) drive
    the 16-bit filter sums / the 16-bit samples to their limits; the result must still be the reference's."""
    _extreme_coefficients(dec, oracle, sub, 8000, chroma_budget, kernel)


@pytest.mark.parametrize("sub,chroma_budget,kernel", [("420", 2046, "fused420p_kernel"), ("420", 8189, "fused420_kernel"), ("444", 8189, "fused444_kernel"),
                                                      ("422", 2046, "fused422_kernel"), ("440", 8189, "fused440_kernel<wide>"), ("411", 8189, "fused411_kernel")])
def test_extreme_coefficients_at_the_16bit_first_pass(dec, oracle, sub, chroma_budget, kernel):
    """The first transform pass of the fast 8-bit kernels runs on 16-bit dequantised coefficients (dequant_idct16): admitted by
    the range check sum |c| q < 16384 per block.  Luma blocks at 16383 -- the DC term alone (level shift on top), one AC
    coefficient of either sign, dense blocks that add up to it -- must come out as the reference's."""
    _extreme_coefficients(dec, oracle, sub, 16383, chroma_budget, kernel)


@pytest.mark.parametrize("budget,flags,equal", [(1476, 0, True), (1477, 0, True), (1477, api.FLAG_FORCE_DOT2, False), (900, 0, True)])
def test_extreme_coefficients_at_the_16bit_second_pass(dec, oracle, budget, flags, equal):
    """fused420p_kernel runs the SECOND pass of its transforms on v_dot2 as well where the first pass's results fit 16 bits: admitted
    by sum |c| q <= 1476 in every block of every component ((710 * 1476 + 16) >> 5 = 32749, idct_columns_dot2).  Blocks right at that
    bound -- DC alone, one AC coefficient of either sign at every position (the matrix entry 710 belongs to columns 1 and 7), dense
    ones -- come out as the reference's; one step beyond, the kernel keeps the 32-bit pass (and agrees), and the 16-bit pass FORCED
    there does not: the bound is tight."""
    _extreme_coefficients(dec, oracle, "420", budget, budget, "fused420p_kernel", flags, equal)


def _extreme_coefficients(dec, oracle, sub, luma_budget, chroma_budget, kernel, flags=0, expect_equal=True):
    torch = _torch()
    d = api.Decoder(0)
    if sub in ("440", "411"):
        data = dec.encode(synth.synth_image(272, 144, 5), 85, sub, 0)
    else:
        data = synth.synth_jpeg(272, 144, 5, 85, sub, 0)
    f = d.read(data)
    d.close()
    rng = np.random.default_rng(77)
    info, _ = oracle.decode_coefficients(data)
    for t in range(4):
        for i in range(64):
            info.quant[t][i] = 1 if i else 2
            f.quant[t][i] = info.quant[t][i]
    info.scan_state_valid = 0  # see above
    planes = []
    for c in range(3):
        shape = (info.bh[c], info.bw[c], 64)
        p = np.zeros(shape, np.int32)
        kind = rng.integers(0, 4, size=shape[:2])
        sign = rng.choice([-1, 1], size=shape[:2])
        budget = chroma_budget if c else luma_budget
        p[..., 0] = np.where(kind == 0, sign * (budget // 2), 0)  # DC alone: q[0] = 2
        k = rng.integers(1, 64, size=shape[:2])
        for by in range(shape[0]):
            for bx in range(shape[1]):
                if kind[by, bx] == 1:
                    p[by, bx, k[by, bx]] = sign[by, bx] * budget  # one AC coefficient carries everything
                elif kind[by, bx] >= 2:
                    v = rng.integers(-40, 41, size=64)
                    v[0] = 0
                    scale = budget / max(1, int(np.abs(v).sum()))
                    v = (v * scale).astype(np.int64)
                    v[1] += np.sign(v[1] or 1) * (budget - int(np.abs(v).sum()))  # spend the rest: the sum is exactly the budget
                    p[by, bx] = v
        planes.append(p)
    for c in range(3):
        q = np.array(info.quant[info.tq[c]], np.int64)
        f.range_max[c] = int((np.abs(planes[c]).astype(np.int64) * q).sum(axis=2).max())
    assert f.range_max[1] <= chroma_budget and f.range_max[2] <= chroma_budget
    f.fast_arith = 1
    assert api.kernel_name(f) == kernel
    exp = oracle.reconstruct(info, planes)
    coef = torch.from_numpy(np.concatenate([p.astype(np.int16).reshape(-1) for p in planes])).cuda()
    row = 272 * 3
    out = torch.zeros((144, row), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, row, 144 * row, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = out.cpu().numpy().reshape(144, 272, 3)
    bad = int((res != exp).sum())
    if not expect_equal:
        assert bad > 0
        return
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(res != exp)[:4].tolist()}"


@pytest.mark.parametrize("sub", ["420", "444", "422"])
@pytest.mark.parametrize("shape", ["rows03", "corner4x4", "corner_plus_one_dense_block"])
def test_pruned_idct_paths(oracle, sub, shape):
    """The fast kernels skip the transform work of coefficient rows / columns 4..7 when they are zero in all 64 blocks a
    wave holds.  Planes built to take each path (only rows 0..3; only the 4 x 4 low-frequency corner; the same with
    one dense block somewhere, which must switch its whole wave back to the full transform)."""
    torch = _torch()
    W, H = 400, 272
    d = api.Decoder(0)
    data = synth.synth_jpeg(W, H, 5, 85, sub, 0)
    f = d.read(data)
    d.close()
    rng = np.random.default_rng(hash((sub, shape)) % 2**32)
    info, _ = oracle.decode_coefficients(data)
    planes = []
    for c in range(3):
        bh, bw = info.bh[c], info.bw[c]
        p = rng.integers(-3, 4, size=(bh, bw, 8, 8)).astype(np.int32)
        p[rng.random(p.shape) < 0.4] = 0
        p[:, :, 4:, :] = 0
        if shape != "rows03":
            p[:, :, :, 4:] = 0
        if shape == "corner_plus_one_dense_block":
            p[bh // 2, bw // 3] = rng.integers(-1, 2, size=(8, 8))
        p[..., 0, 0] = rng.integers(-40, 41, size=(bh, bw))
        planes.append(p.reshape(bh, bw, 64))
    for c in range(3):
        q = np.array(info.quant[info.tq[c]], np.int64)
        f.range_max[c] = int((np.abs(planes[c]).astype(np.int64) * q).sum(axis=2).max())
    f.fast_arith = 1
    assert max(f.range_max[:3]) < 2047, list(f.range_max)
    exp = oracle.reconstruct(info, planes)
    coef = torch.from_numpy(np.concatenate([p.astype(np.int16).reshape(-1) for p in planes])).cuda()
    row = W * 3
    out = torch.zeros((H, row), dtype=torch.uint8, device="cuda")
    ws_bytes = api.workspace_bytes(f, 1)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, row, H * row, workspace=ws.data_ptr(), workspace_bytes=ws_bytes,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = out.cpu().numpy().reshape(H, W, 3)
    bad = int((res != exp).sum())
    assert bad == 0, f"{api.kernel_name(f)}: {bad} differing samples, first at {np.argwhere(res != exp)[:4].tolist()}"


def test_round_trip_properties_8k(dec):
    """Size-independent properties at BASELINE's full 8K size: the three code paths (fast fused, safe fused,
    generic two-kernel) agree line band by line band (checksum of checksums), reconstruction is idempotent,
    and the stripe service returns exactly the whole-frame pixels."""
    data = synth.synth_jpeg(7680, 4320, 4321, 85, "420", 8)
    f = dec.read(data)

    def band_hashes(img):
        return [_sha(img[y:y + 135]) for y in range(0, 4320, 135)]

    a = dec.reconstruct()
    ha = band_hashes(a)
    assert band_hashes(dec.reconstruct(api.FLAG_FORCE_SAFE)) == ha
    assert band_hashes(dec.reconstruct(api.FLAG_FORCE_GENERIC)) == ha
    assert band_hashes(dec.reconstruct()) == ha
    stripes = np.zeros_like(a)
    for y in range(0, f.height, 8):
        dec.reconstruct_rect(0, y, f.width - 1, y + 7, out=stripes)
    assert band_hashes(stripes) == ha


# ------------------------------------------------------------------------------------------------------
# the drop-in surface: `class JPEG` (tag/hook API) driven by the cmd/reconstruct-compatible front end
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg1_512x512_444_q75_ref", "ref_75x45_420_dri2", "pil_200x120_420_dri8", "pil_70x40_gray",
                                  "ref_97x61_3x3", "pil_33x17_420_dri1"])
def test_cli_writes_the_references_pnm(tmp_path, name):
    """`jpeg in.jpg out.ppm` (class JPEG: Read / GetInformation / DisplayRectangle per 8-line stripe with an I/O
    hook and a bitmap hook) must write byte for byte the PNM the reference binary writes."""
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT

    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    assert os.path.exists(exe), "libjpeg_amd/bin/jpeg not built (run __graft_entry__.build())"
    ent = MANIFEST[name]
    out = tmp_path / "out.pnm"
    r = subprocess.run([exe, os.path.join(GOLDEN_DIR, name + ".jpg"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    header = b"P%d\n%d %d\n255\n" % (6 if ent["channels"] == 3 else 5, ent["width"], ent["height"])
    assert data.startswith(header)
    assert hashlib.sha256(data[len(header):]).hexdigest() == ent["pixels_sha256"]


@pytest.mark.parametrize("name", ["cfg1_512x512_444_q75_ref", "ref_75x45_420_dri2", "pil_200x120_420_dri8", "pil_70x40_gray",
                                  "ref_97x61_3x3", "pil_33x17_420_dri1", "xt_129x71_420", "xt_64x48_444"])
def test_the_references_own_client_runs_on_this_library(tmp_path, name):
    """oracle/_ref/jpeg_dropin is the reference's cmd/reconstruct.cpp with its bitmap and file hooks, compiled UNCHANGED
    from the reference tree against libjpeg_amd's interface headers and linked with libmijpeg.so (oracle/Makefile,
    target dropin; built where the reference sources are present).  It must write the bytes the reference binary writes."""
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT

    exe = os.path.join(ROOT, "oracle", "_ref", "jpeg_dropin")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/jpeg_dropin is built from the reference sources (make -C oracle dropin)")
    ent = MANIFEST[name]
    out = tmp_path / "out.pnm"
    r = subprocess.run([exe, os.path.join(GOLDEN_DIR, name + ".jpg"), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    data = out.read_bytes()
    if ent.get("kind") == "xt_float32":  # 'PF' file with big-endian floats (cmd/reconstruct.cpp:321-323)
        header = b"PF\n%d %d\n1\n" % (ent["width"], ent["height"])
        assert data.startswith(header)
        body = np.frombuffer(data[len(header):], ">f4").astype("<f4")
        assert hashlib.sha256(body.tobytes()).hexdigest() == ent["pixels_sha256"]
    else:
        header = b"P%d\n%d %d\n255\n" % (6 if ent["channels"] == 3 else 5, ent["width"], ent["height"])
        assert data.startswith(header)
        assert hashlib.sha256(data[len(header):]).hexdigest() == ent["pixels_sha256"]


@pytest.mark.parametrize("name", ["ref_75x45_420_dri2", "pil_200x120_420_dri8", "pilprog_75x45_420", "pil_70x40_gray"])
def test_the_references_marker_injection_client_runs_on_this_library(tmp_path, name):
    """oracle/_ref/jpeg_dropin_inject = the same unchanged cmd/reconstruct.cpp compiled with -DTEST_MARKER_INJECTION
    (cmd/reconstruct.cpp:80-119): JPEG::Read with JPGTAG_DECODER_STOP = STOP_FRAME, PeekMarker after every step, APP9 segments
    taken out with ReadMarker + SkipMarker, then the remaining Read.  APP9 segments are injected behind every header segment;
    the picture must be the reference's picture of the clean stream."""
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT
    from test_marker_calls import inject

    exe = os.path.join(ROOT, "oracle", "_ref", "jpeg_dropin_inject")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/jpeg_dropin_inject is built from the reference sources (make -C oracle dropin)")
    ent = MANIFEST[name]
    src = tmp_path / "in.jpg"
    src.write_bytes(inject(golden_jpeg(name), 0))
    out = tmp_path / "out.pnm"
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    data = out.read_bytes()
    header = b"P%d\n%d %d\n255\n" % (6 if ent["channels"] == 3 else 5, ent["width"], ent["height"])
    assert data.startswith(header)
    assert hashlib.sha256(data[len(header):]).hexdigest() == ent["pixels_sha256"]


@pytest.mark.parametrize("entropy", ["0", "1"])
def test_cli_4k_with_restart_markers_device_and_host_entropy(tmp_path, oracle, entropy):
    """A 4K frame with 16 200 restart intervals goes through the on-device entropy decoder inside JPEG::Read
    (MIJPEG_ENTROPY=0, the default) and through the host decoder (=1): the same PNM as the reference's."""
    import os
    import subprocess

    from conftest import ROOT

    ent = MANIFEST["big_4k_420_q85_dri8"]
    data = big_jpeg("big_4k_420_q85_dri8")
    pinned_by_reference = data is not None
    if data is None:
        data = synth.synth_jpeg(ent["width"], ent["height"], ent["seed"], ent["quality"], ent["sub"], ent["dri"])
    src, out = tmp_path / "in.jpg", tmp_path / "out.ppm"
    src.write_bytes(data)
    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, env=dict(os.environ, MIJPEG_ENTROPY=entropy))
    assert r.returncode == 0, r.stderr
    got = out.read_bytes()
    header = b"P6\n%d %d\n255\n" % (ent["width"], ent["height"])
    assert got.startswith(header)
    if pinned_by_reference:
        assert hashlib.sha256(got[len(header):]).hexdigest() == ent["pixels_sha256"]
    else:
        assert got[len(header):] == oracle.decode(data).tobytes()


@pytest.mark.parametrize("name", XT_CASES[:3] + P12_CASES)
def test_cli_writes_the_references_pfm_and_16bit_pnm(tmp_path, name):
    """JPEG XT -> 'PF' file with big-endian floats (cmd/reconstruct.cpp:321-323, cmd/bitmaphook.cpp:282-305),
    12 bit -> P6 with maxval 4095 and big-endian samples: the bytes the reference CLI writes."""
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT

    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    ent = MANIFEST[name]
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, os.path.join(GOLDEN_DIR, name + ".jpg"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    if ent["kind"] == "xt_float32":
        header = b"PF\n%d %d\n1\n" % (ent["width"], ent["height"])
        body = np.frombuffer(data[len(header):], ">f4").astype("<f4")
    else:
        header = b"P6\n%d %d\n4095\n" % (ent["width"], ent["height"])
        body = np.frombuffer(data[len(header):], ">u2").astype("<u2")
    assert data.startswith(header)
    assert hashlib.sha256(body.tobytes()).hexdigest() == ent["pixels_sha256"]


def test_cli_no_color_transform_and_errors(tmp_path, oracle):
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT

    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    src = os.path.join(GOLDEN_DIR, "ref_80x48_420.jpg")
    out = tmp_path / "o.ppm"
    r = subprocess.run([exe, "-c", src, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exp = oracle.decode(golden_jpeg("ref_80x48_420"), use_ycbcr=0)
    assert out.read_bytes().split(b"255\n", 1)[1] == exp.tobytes()
    bad = tmp_path / "bad.jpg"
    bad.write_bytes(b"\xff\xd8\xff\xc2garbage")
    r = subprocess.run([exe, str(bad), str(out)], capture_output=True, text=True)
    assert r.returncode != 0 and "reading a JPEG file failed - error" in r.stderr


def test_frame_pipeline_batch(oracle):
    """BASELINE config 4 in miniature: a batch of independent frames through the overlapped pipeline (several decoder
    objects / streams per GPU), every frame bit-exact."""
    from libjpeg_amd import pipeline

    streams = [synth.synth_jpeg(320 + 16 * (i % 3), 208, 1000 + i, 85, "420", 4) for i in range(12)]
    frames = list(pipeline.decode_batch(streams, device=0, depth=3))
    assert len(frames) == len(streams)
    for data, px in zip(streams, frames):
        assert np.array_equal(px, oracle.decode(data))


# ---------------------------------------------------------------------------------------------------------------
# on-device entropy decoding (one thread per restart interval) against the host decoder and the oracle
# ---------------------------------------------------------------------------------------------------------------
def _same_coefficients(a, b, ncomp):
    for c in range(ncomp):
        assert np.array_equal(a.coefficients(c), b.coefficients(c)), f"component {c}"


@pytest.mark.parametrize("w,h,sub,ri,q", [
    (640, 480, "420", 1, 85), (641, 479, "420", 7, 95), (1000, 333, "444", 5, 75), (515, 260, "422", 3, 30),
    (256, 256, "420", 16, 100), (2048, 1024, "420", 128, 90), (333, 777, "444", 1000, 50),
])
def test_device_entropy_decoder_matches_host(dec, oracle, w, h, sub, ri, q):
    data = synth.encode_jpeg(synth.synth_image(w, h, seed=w + h), q, sub, restart_mcus=ri)
    host = api.Decoder(0)
    hi = host.read(data)
    gi = dec.read(data, entropy="gpu")
    assert dec.entropy_used == "gpu"
    assert gi.fast_arith == hi.fast_arith and list(gi.range_max) == list(hi.range_max)
    out = dec.reconstruct()  # before the planes are fetched: the device copy is what the kernels read
    assert np.array_equal(out, oracle.decode(data))
    _same_coefficients(dec, host, hi.components)
    host.close()


def test_device_entropy_decoder_grey_and_optimized_tables(dec, oracle):
    grey = synth.encode_jpeg(synth.synth_image(500, 300, 5, channels=1), 90, restart_mcus=4, optimize=True)
    dec.read(grey, entropy="gpu")
    assert np.array_equal(dec.reconstruct(), oracle.decode(grey))
    col = synth.encode_jpeg(synth.synth_image(500, 300, 6), 92, "420", restart_mcus=2, optimize=True)
    dec.read(col, entropy="gpu")
    assert np.array_equal(dec.reconstruct(), oracle.decode(col))


def test_device_entropy_decoder_eligibility_and_errors(dec):
    # tiny without restart markers (the walk wants 256 MCUs), a progressive picture whose scans have no restart markers and are
    # beyond a lane's reach (AC refinement is serial by construction): not available on the device ("auto" falls back
    # to the host silently)
    for data in (synth.synth_jpeg(160, 120), synth.synth_jpeg(1600, 1200, quality=92, progressive=True)):
        with pytest.raises(api.MijpegError) as e:
            dec.read(data, entropy="gpu")
        assert e.value.code == api.ERR_NOT_AVAILABLE
        dec.read(data, entropy="auto")
        assert dec.entropy_used == "host"
    # ... with restart markers a progressive picture is the device's since round 6 (tests/test_device_multiscan.py); "auto" keeps a
    # small one on the host, like a small sequential one
    data = synth.synth_jpeg(320, 240, restart_mcus=4, progressive=True)
    dec.read(data, entropy="gpu")
    assert dec.entropy_used == "gpu"
    dec.read(data, entropy="auto")
    assert dec.entropy_used == "host"
    # few intervals: "auto" keeps it on the host, "gpu" forces it
    data = synth.synth_jpeg(320, 240, restart_mcus=4)
    dec.read(data, entropy="auto")
    assert dec.entropy_used == "host"
    # corrupted entropy coded data: same error class as the host decoder
    good = bytearray(synth.synth_jpeg(640, 480, restart_mcus=2, quality=95))
    sos = good.find(b"\xff\xda")
    rng = np.random.default_rng(3)
    host = api.Decoder(0)
    seen = on_device = 0
    for trial in range(40):
        bad = bytearray(good)
        for pos in rng.integers(sos + 20, len(bad) - 2, size=8):
            if bad[pos] != 0xFF and bad[pos - 1] != 0xFF:
                bad[pos] = int(rng.integers(0, 255))
        codes = []
        for d, mode in ((host, "host"), (dec, "prefer-gpu")):
            try:
                d.read(bytes(bad), entropy=mode)
                codes.append(0)
            except api.MijpegError as e:
                codes.append(e.code)
        assert codes[0] == codes[1], (trial, codes)
        on_device += dec.entropy_used == "gpu"
        if codes[0] == 0:
            _same_coefficients(dec, host, 3)
        else:
            seen += 1
    assert on_device > 0 and seen > 0, (on_device, seen)
    host.close()


def test_device_entropy_decoder_8k(dec):
    """BASELINE config 3 (8K 4:2:0, DRI 8: 32 400 restart intervals) entropy-decoded on the device."""
    ent = MANIFEST["big_8k_420_q85_dri8"]
    data = big_jpeg("big_8k_420_q85_dri8")
    pinned_by_reference = data is not None
    if data is None:
        data = synth.synth_jpeg(ent["width"], ent["height"], ent["seed"], ent["quality"], ent["sub"], ent["dri"])
    host = api.Decoder(0)
    hi = host.read(data)
    gi = dec.read(data, entropy="auto")
    assert dec.entropy_used == "gpu"
    assert gi.fast_arith == hi.fast_arith == 1 and list(gi.range_max) == list(hi.range_max)
    out = dec.reconstruct()
    if pinned_by_reference:
        assert _sha(out) == ent["pixels_sha256"]
    assert np.array_equal(out, host.reconstruct())
    _same_coefficients(dec, host, 3)
    host.close()


# ---------------------------------------------------------------------------------------------------------------
# device-side bitmap hand-off (MIJPEG_FLAG_DEVICE_OUTPUT / JPGTAG_MIJPEG_DEVICE_BITMAPS)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pil_200x120_420_dri8", "ref_97x61_3x3", "pil_70x40_gray"])
def test_rectangles_into_device_bitmaps(dec, name):
    import torch

    data = golden_jpeg(name)
    exp = golden_pixels(name)
    f = dec.read(data)
    H, W, C_ = exp.shape
    # interleaved device bitmap with a padded row stride, served in 8-line stripes like cmd/reconstruct
    stride = W * C_ + 13
    buf = torch.zeros((H, stride), dtype=torch.uint8, device="cuda")
    for y in range(0, H, 8):
        dec.reconstruct_rect_device(0, y, W - 1, min(H, y + 8) - 1, [buf.data_ptr() + c for c in range(C_)], [C_] * C_, [stride] * C_)
    got = buf.cpu().numpy()[:, : W * C_].reshape(H, W, C_)
    assert np.array_equal(got, exp)
    assert int(buf[:, W * C_:].sum()) == 0  # nothing beyond the lines
    # planar device bitmaps, inner rectangle, one component left out
    planes = torch.zeros((C_, H, W), dtype=torch.uint8, device="cuda")
    x0, y0, x1, y1 = 3, 5, W - 7, H - 4
    ptrs = [planes[c].data_ptr() for c in range(C_)]
    if C_ == 3:
        ptrs[1] = None
    dec.reconstruct_rect_device(x0, y0, x1, y1, ptrs, [1] * C_, [W] * C_)
    got = planes.cpu().numpy()
    for c in range(C_):
        want = np.zeros((H, W), np.uint8)
        if not (C_ == 3 and c == 1):
            want[y0:y1 + 1, x0:x1 + 1] = exp[y0:y1 + 1, x0:x1 + 1, c]
        assert np.array_equal(got[c], want), c
    # host rectangles still work afterwards (the device frame is reused, the host copy is made on demand)
    assert np.array_equal(dec.reconstruct(), exp)


def test_device_bitmaps_16bit_samples(dec):
    import torch

    name = P12_CASES[0]
    exp = golden_pixels(name)
    dec.read(golden_jpeg(name))
    H, W, C_ = exp.shape
    buf = torch.zeros((H, W, C_), dtype=torch.int16, device="cuda")
    dec.reconstruct_rect_device(0, 0, W - 1, H - 1, [buf.data_ptr() + 2 * c for c in range(C_)], [2 * C_] * C_, [2 * W * C_] * C_)
    assert np.array_equal(buf.cpu().numpy().view(np.uint16), exp)


# ---------------------------------------------------------------------------------------------------------------
# JPGTAG_DECODER_UPSAMPLE = false / CLI -U, and PGX output for images with neither one nor three components
# ---------------------------------------------------------------------------------------------------------------
UNSAMPLED_CASES = sorted(k for k, v in MANIFEST.items() if "unsampled" in v)


@pytest.mark.parametrize("name", UNSAMPLED_CASES)
def test_cli_without_upsampling_writes_the_references_pgx(tmp_path, name):
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT

    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    out = tmp_path / "out"
    r = subprocess.run([exe, "-U", os.path.join(GOLDEN_DIR, name + ".jpg"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = MANIFEST[name]["unsampled"]
    assert out.read_text().split() == ["%s_%d.raw" % (out, k) for k in range(len(want))]
    for k, u in enumerate(want):
        assert (tmp_path / ("out_%d.h" % k)).read_text() == u["header"]
        assert hashlib.sha256((tmp_path / ("out_%d.raw" % k)).read_bytes()).hexdigest() == u["sha256"], (name, k)


@pytest.mark.parametrize("w,h,sub", [(333, 111, "420"), (64, 64, "444"), (129, 257, "422")])
def test_unsampled_components_vs_oracle(dec, oracle, w, h, sub):
    """Without upsampling a component is its IDCT output, rounded and clamped: (s + 8) >> 4 (identity transformation)."""
    data = synth.synth_jpeg(w, h, 7, 80, sub, 3)
    f = dec.read(data)
    info, planes = oracle.decode_coefficients(data)
    for c in range(3):
        samples = oracle.idct_plane(planes[c].reshape(info.bh[c], info.bw[c], 64), np.array(info.quant[info.tq[c]]), 8)
        exp = np.clip((samples + 8) >> 4, 0, 255).astype(np.uint8)[: info.ch[c], : info.cw[c]]
        assert np.array_equal(dec.reconstruct_unsampled(c), exp), c
    # a host rectangle of the upsampled picture afterwards: the cached frame is replaced, not mixed up
    assert np.array_equal(dec.reconstruct(), oracle.decode(data))
    with pytest.raises(api.MijpegError):  # components only one by one
        dst = (api.C.c_void_p * 4)()
        z = (api.C.c_int32 * 4)()
        dec._check(api.lib().mijpeg_reconstruct_rect(dec._h, 0, 0, w - 1, h - 1, 0, 2, api.FLAG_NO_UPSAMPLING, dst, z, z))


def test_cli_cmyk_writes_pgx_planes(tmp_path):
    import os
    import subprocess

    from conftest import GOLDEN_DIR, ROOT

    name = "pil_90x60_cmyk"
    exp = golden_pixels(name)
    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    out = tmp_path / "out"
    r = subprocess.run([exe, os.path.join(GOLDEN_DIR, name + ".jpg"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for k in range(4):
        assert (tmp_path / ("out_%d.h" % k)).read_text() == "PG ML +8 90 60\n"
        got = np.frombuffer((tmp_path / ("out_%d.raw" % k)).read_bytes(), np.uint8).reshape(60, 90)
        assert np.array_equal(got, exp[..., k]), k


# ---------------------------------------------------------------------------------------------------------------
# batches: n streams -> one Huffman kernel launch -> one reconstruction launch (mijpeg_decode_batch_device)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,sub,ri,n", [(640, 480, "420", 2, 7), (333, 211, "444", 1, 5), (512, 256, "422", 4, 3), (1920, 1080, "420", 8, 16)])
def test_batch_decode_on_the_device(oracle, w, h, sub, ri, n):
    torch = _torch()
    imgs = [synth.synth_image(w, h, 300 + i) for i in range(n)]
    # optimised Huffman tables differ from image to image; the quantisation tables (same quality) do not
    streams = [synth.encode_jpeg(im, 88, sub, restart_mcus=ri, optimize=(i % 2 == 1)) for i, im in enumerate(imgs)]
    d = api.Decoder(0)
    info = d.decode_batch_device(streams, min_intervals=1)
    row = w * 3
    out = torch.zeros((n, h, row), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(out.data_ptr(), h * row, row)
    res = out.cpu().numpy().reshape(n, h, w, 3)
    for i in range(n):
        assert np.array_equal(res[i], oracle.decode(streams[i])), i
    # the decoder object goes back to single images afterwards
    one = d.read(streams[0])
    assert np.array_equal(d.reconstruct(), res[0])
    d.close()


@pytest.mark.parametrize("flags", [0, api.FLAG_FORCE_SAFE])
@pytest.mark.parametrize("w,h,sub", [(640, 480, "420"), (333, 211, "444"), (515, 260, "422"), (301, 415, "440"), (400, 300, "gray"), (272, 144, "411")])
def test_batch_whose_images_bring_their_own_quantisation_tables(oracle, w, h, sub, flags):
    """Motion JPEG under rate control: same shape, another quality per frame.  One Huffman launch, one reconstruction launch
    that reads per-frame tables from device memory (mijpeg_batch.quant_dev) instead of the kernel arguments."""
    torch = _torch()
    quals = [85, 40, 97, 85, 12, 70, 100]
    n = len(quals)
    nc = 1 if sub == "gray" else 3
    imgs = [synth.synth_image(w, h, 800 + i, channels=nc) for i in range(n)]
    d = api.Decoder(0)
    if sub in ("440", "411"):  # Pillow cannot write these layouts: this library's own encoder does
        streams = [d.encode(im, q, sub, 3, i % 2 == 1) for i, (im, q) in enumerate(zip(imgs, quals))]
    else:
        streams = [synth.encode_jpeg(im, q, "444" if sub == "gray" else sub, restart_mcus=3, optimize=(i % 2 == 1)) for i, (im, q) in enumerate(zip(imgs, quals))]
    info = d.decode_batch_device(streams, min_intervals=1)
    # the batch's info carries the largest delta of any image at each position
    singles = [api.Decoder(0) for _ in range(2)]
    q0 = max(int(singles[0].read(st).quant[0][63]) for st in streams)
    assert int(info.quant[0][63]) == q0
    row = w * nc
    out = torch.zeros((n, h, row), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(out.data_ptr(), h * row, row, flags)
    res = out.cpu().numpy().reshape(n, h, w, nc)
    for i in range(n):
        assert np.array_equal(res[i].squeeze(), oracle.decode(streams[i]).squeeze()), (i, quals[i])
    # a batch of equal tables afterwards goes back to the kernel arguments
    d.decode_batch_device([streams[0], streams[3]], min_intervals=1)
    out2 = torch.zeros((2, h, row), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(out2.data_ptr(), h * row, row, flags)
    assert np.array_equal(out2.cpu().numpy().reshape(2, h, w, nc), res[[0, 3]])
    for x in singles:
        x.close()
    d.close()


@pytest.mark.parametrize("sub,p12,kernel", [("420", False, None), ("420", True, "fused420_kernel<12>"), ("444", True, "fused444_12_kernel"), ("422", True, "fused422_12_kernel")])
def test_stateless_launch_with_per_frame_tables(oracle, sub, p12, kernel):
    """mijpeg_launch_reconstruct with quant_dev: coefficient stores of three images side by side, their deltas as u16
    [frames][4][64] in device memory, info.quant = the element-wise maximum.  8-bit 4:2:0 and the 12-bit kernels' QDEV builds."""
    torch = _torch()
    w, h = 384, 256
    streams = [synth.synth_jpeg(w, h, 50 + i, q, sub, 4) for i, q in enumerate((90, 35, 75))]
    if p12:
        streams = [synth.to_12bit(st, sc) for st, sc in zip(streams, (16, 11, 16))]
    n = len(streams)
    d = api.Decoder(0)
    infos, coefs = [], []
    import ctypes as C
    for st in streams:
        f = api.MijpegInfo()
        C.memmove(C.byref(f), C.byref(d.read(st)), C.sizeof(api.MijpegInfo))
        infos.append(f)
        store = np.zeros(int(f.coef_count), np.int16)
        for c in range(3):
            plane = d.coefficients(c).reshape(-1)
            store[int(f.coef_offset[c]):int(f.coef_offset[c]) + plane.size] = plane
        coefs.append(store)
    info = api.MijpegInfo()
    C.memmove(C.byref(info), C.byref(infos[0]), C.sizeof(api.MijpegInfo))
    tabs = np.ones((n, 4, 64), np.uint16)
    for i, f in enumerate(infos):
        for c in range(3):
            tabs[i, c] = np.array(f.quant[f.quant_index[c]][:], np.uint16)
    for c in range(3):
        info.quant_index[c] = c
        for k in range(64):
            info.quant[c][k] = int(tabs[:, c, k].max())
        info.range_max[c] = max(int(f.range_max[c]) for f in infos)
    coef = torch.from_numpy(np.stack(coefs)).cuda()
    qd = torch.from_numpy(tabs.view(np.int16)).cuda()
    row = w * (6 if p12 else 3)
    out = torch.zeros((n, h, row), dtype=torch.uint8, device="cuda")
    if kernel:
        assert api.kernel_name(info).split("/")[0] == kernel, (api.kernel_name(info), list(info.range_max))
    for flags in (0, api.FLAG_FORCE_GENERIC):
        out.zero_()
        wsb = api.workspace_bytes(info, n, flags, own_tables=True)
        assert wsb >= n * 4 * 64 * 4
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        with pytest.raises(api.MijpegError):  # the expanded tables live in the workspace
            api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), n, row, h * row, flags=flags, quant_dev=qd.data_ptr())
        api.launch_reconstruct(info, coef.data_ptr(), out.data_ptr(), n, row, h * row, flags=flags, workspace=ws.data_ptr(), workspace_bytes=wsb,
                               quant_dev=qd.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(np.uint16).reshape(n, h, w, 3) if p12 else out.cpu().numpy().reshape(n, h, w, 3)
        for i in range(n):
            assert np.array_equal(res[i], oracle.decode16(streams[i]) if p12 else oracle.decode(streams[i])), (flags, i)
    d.close()


def test_batch_decode_rejects_what_is_not_a_batch():
    d = api.Decoder(0)
    a = synth.synth_jpeg(320, 240, 1, 85, "420", 2)
    # an Adobe marker with transform = 0 switches the colour transformation off for that image only: one reconstruction
    # launch cannot serve both (APP14 segment as marker/adobemarker.cpp lays it out, right behind SOI)
    import struct
    adobe_rgb = a[:2] + b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0) + a[2:]
    for other in (synth.synth_jpeg(336, 240, 1, 85, "420", 2),   # another width
                  synth.synth_jpeg(320, 240, 1, 85, "444", 2),   # another sampling
                  adobe_rgb):                                    # another colour transformation
        with pytest.raises(api.MijpegError) as e:
            d.decode_batch_device([a, other], min_intervals=1)
        assert e.value.code == api.ERR_NOT_AVAILABLE
    bad = bytearray(a)
    bad[len(bad) // 2] ^= 0x5A
    bad[len(bad) // 2 + 1] = 0xFF
    bad[len(bad) // 2 + 2] = 0xD9  # an EOI in the middle of the data: restart intervals go missing
    # a damaged member: the batch is handed back (the host decoder walks such streams with the reference's resynchronisation)
    with pytest.raises(api.MijpegError) as e:
        d.decode_batch_device([a, bytes(bad)], min_intervals=1)
    assert e.value.code == api.ERR_NOT_AVAILABLE and "damaged" in e.value.message
    d.close()


@pytest.mark.parametrize("walk", ["device", "host"])
@pytest.mark.parametrize("w,h,sub,q", [(3840, 2160, "420", 85), (2560, 1440, "444", 95), (2048, 2048, "gray", 90),
                                       (1000, 700, "422", 50), (7680, 4320, "420", 92), (640, 480, "420", 99)])
def test_device_entropy_decoder_without_restart_markers(dec, monkeypatch, walk, w, h, sub, q):
    """No DRI: a self-synchronising walk -- on the device (rounds of huffman_walk_kernel until the hand-over states
    are a fixed point) or, MIJPEG_DEVICE_WALK=0, on the host -- supplies exact restart points (bit offset + DC
    predictors) and the device kernel decodes from them; coefficients and pixels must equal the host decoder's."""
    monkeypatch.setenv("MIJPEG_DEVICE_WALK", "1" if walk == "device" else "0")
    img = synth.synth_image(w, h, 12, channels=1 if sub == "gray" else 3)
    data = synth.encode_jpeg(img, q, sub if sub != "gray" else "444")
    host = api.Decoder(0)
    hi = host.read(data)
    try:
        gi = dec.read(data, entropy="gpu")
    except api.MijpegError as e:
        # the host's planner wants longer streams (four of its 32 KiB segments) than the device walk (4 KiB)
        assert walk == "host" and e.code == api.ERR_NOT_AVAILABLE and len(data) < 200_000
        host.close()
        return
    assert dec.entropy_used == "gpu"
    assert (dec.device_walk_rounds() > 0) == (walk == "device")
    assert gi.fast_arith == hi.fast_arith and list(gi.range_max) == list(hi.range_max)
    assert np.array_equal(dec.reconstruct(), host.reconstruct())
    _same_coefficients(dec, host, hi.components)
    host.close()


@pytest.mark.parametrize("w,h,sub,n,mixed", [(1280, 720, "420", 6, False), (800, 608, "444", 4, True), (1920, 1080, "420", 9, True),
                                             (3840, 2160, "420", 10, False)])  # the last one: pipelined uploads
def test_batch_without_restart_markers(oracle, w, h, sub, n, mixed):
    """Batches whose streams carry no restart markers (or only some do): one walk over all of them, one decode launch."""
    torch = _torch()
    streams = [synth.encode_jpeg(synth.synth_image(w, h, 500 + i), 85, sub, restart_mcus=(4 if mixed and i % 2 else 0),
                                 optimize=(i % 3 == 1)) for i in range(n)]
    d = api.Decoder(0)
    d.decode_batch_device(streams, min_intervals=1)
    assert d.device_walk_rounds() > 0
    row = w * 3
    out = torch.zeros((n, h, row), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(out.data_ptr(), h * row, row)
    res = out.cpu().numpy().reshape(n, h, w, 3)
    for i in range(n):
        assert np.array_equal(res[i], oracle.decode(streams[i])), i
    d.close()


@pytest.mark.parametrize("deferred", [False, True])
def test_host_walk_in_uniform_batches(monkeypatch, deferred):
    """MIJPEG_DEVICE_WALK=0 in a batch, in one call and submitted: the host plans every image's restart points, one launch decodes
    them.  A batch's planes stay in HBM, so what is compared are the range check the Huffman kernel reports and the pixels, both
    with the host decoder's."""
    torch = _torch()
    monkeypatch.setenv("MIJPEG_DEVICE_WALK", "0")
    w = h = 256
    streams = [noise_jpeg(w, h, 40 + i) for i in range(3)]
    want = host_decodes(streams)
    d = api.Decoder(0)
    if deferred:
        d.submit_batch_device(streams, 1)
        info = d.finish_batch_device()
    else:
        info = d.decode_batch_device(streams, min_intervals=1)
    assert d.device_walk_rounds() == 0
    assert list(info.range_max)[:3] == [max(x[1][c] for x in want) for c in range(3)]
    out = torch.zeros((3, h, w * 3), dtype=torch.uint8, device="cuda")
    d.reconstruct_batch_device(out.data_ptr(), h * w * 3, w * 3)
    res = out.cpu().numpy().reshape(3, h, w, 3)
    for i in range(3):
        assert np.array_equal(res[i], want[i][0]), i
    d.close()


def test_single_component_with_sampling_factors_on_the_device(dec):
    """A frame whose only component has sampling factors 2 x 2, 40 x 24: its scan covers 5 x 3 blocks of planes that hold 6 x 4,
    and the blocks it leaves out must read as zero although the store held another picture's coefficients."""
    data = grey_2x2_jpeg(40, 24, 5, 2)
    host = api.Decoder(0)
    hi = host.read(data)
    want = host.coefficients(0)
    assert want.shape[:2] == (4, 6) and want[:3, :5].any() and not want[:, 5].any() and not want[3].any()
    dec.read(noise_jpeg(64, 48, 9, restart_mcus=1), entropy="gpu")  # (what the store holds before)
    assert dec.entropy_used == "gpu" and dec.coefficients(0).reshape(-1, 64)[:24].any(axis=1).all()  # (the 24 blocks the planes will lie on)
    gi = dec.read(data, entropy="gpu")
    assert dec.entropy_used == "gpu"
    assert np.array_equal(dec.coefficients(0), want)
    assert list(gi.range_max) == list(hi.range_max) and gi.fast_arith == hi.fast_arith
    assert np.array_equal(dec.reconstruct(), host.reconstruct())
    host.close()


def test_xt_codestreams_with_restart_markers_on_the_device(dec):
    """Both codestreams of a JPEG XT profile C file (8-bit legacy frame 4:2:0, 12-bit residual frame, restart markers every two
    MCUs in each, no hidden bits) through the sequential device decoder, the residual one on the helper object: planes of both
    frames, range checks and codes equal the host decoder's."""
    data = golden_jpeg("profile_c_129x71_420_dri2")
    host = api.Decoder(0)
    hi = host.read(data)
    assert hi.xt and not hi.progressive and not host.xt_params().residual_wide
    gi = dec.read(data, entropy="gpu")
    assert dec.entropy_used == "gpu" and dec.device_walk_rounds() == 0
    assert list(gi.range_max) == list(hi.range_max)
    assert list(dec.xt_params().residual.range_max) == list(host.xt_params().residual.range_max)
    codes = dec.reconstruct()  # (before the planes are fetched: the device copy is what the kernels read)
    assert np.array_equal(codes, host.reconstruct())
    for c in range(3):
        assert np.array_equal(dec.coefficients(c), host.coefficients(c)), c
        assert np.array_equal(dec.residual_coefficients(c), host.residual_coefficients(c)), c
    host.close()


def test_device_walk_on_damaged_streams_agrees_with_the_host(dec):
    """Corrupt entropy data without restart markers, "auto": either the device decodes exactly what the host decodes, or
    the walk refuses (no fixed point that is a decode of the frame) and the host decoder gets the stream -- in every case
    the caller sees what the host decoder alone would have produced, error class included; nothing hangs."""
    good = bytearray(synth.synth_jpeg(1024, 768, 3, 90, "420", 0))
    sos = good.find(b"\xff\xda")
    rng = np.random.default_rng(17)
    host = api.Decoder(0)
    on_device = errors = 0
    for trial in range(30):
        bad = bytearray(good)
        kind = trial % 3
        if kind == 0:    # flipped bytes
            for pos in rng.integers(sos + 20, len(bad) - 2, size=6):
                if bad[pos] != 0xFF and bad[pos - 1] != 0xFF:
                    bad[pos] = int(rng.integers(0, 255))
        elif kind == 1:  # a marker in the middle of the data
            pos = int(rng.integers(sos + 200, len(bad) - 200))
            bad[pos:pos + 2] = bytes([0xFF, int(rng.choice([0xD0, 0xD9, 0xC4, 0xE0]))])
        else:            # truncation (the EOI is kept)
            cut = int(rng.integers(sos + 500, len(bad) - 2))
            bad = bad[:cut] + bytearray(b"\xff\xd9")
        codes = []
        for d, mode in ((host, "host"), (dec, "auto")):
            try:
                d.read(bytes(bad), entropy=mode)
                codes.append(0)
            except api.MijpegError as e:
                codes.append(e.code)
        assert codes[0] == codes[1], (trial, kind, codes)
        if codes[0] == 0:
            _same_coefficients(dec, host, 3)
            on_device += dec.entropy_used == "gpu"
        else:
            errors += 1
    assert on_device > 0 or errors > 0
    host.close()


def test_randomised_streams_through_every_entry_path(oracle):
    """60 seeded random streams (size, sampling, quality, restart interval, optimised tables, progressive, grey) through the
    decoder object with entropy = host / auto, against the oracle; sizes small enough for the oracle to stay fast."""
    rng = np.random.default_rng(20260925)
    d = api.Decoder(0)
    for t in range(60):
        w, h = int(rng.integers(1, 700)), int(rng.integers(1, 500))
        sub = ["444", "422", "420", "gray"][int(rng.integers(0, 4))]
        q = int(rng.choice([5, 30, 50, 75, 90, 98]))
        dri = int(rng.choice([0, 0, 1, 2, 5, 16]))
        prog = bool(rng.integers(0, 5) == 0)
        opt = bool(rng.integers(0, 2))
        img = synth.synth_image(w, h, 1000 + t, channels=1 if sub == "gray" else 3)
        if rng.integers(0, 3) == 0:  # noise: dense coefficients, many 0xFF bytes in the stream
            img = rng.integers(0, 256, img.shape).astype(np.uint8)
        try:
            data = synth.encode_jpeg(img, q, sub if sub != "gray" else "444", restart_mcus=dri, optimize=opt, progressive=prog)
        except OSError:  # Pillow refuses a few combinations (tiny images with restart markers)
            continue
        exp = oracle.decode(data)
        for mode in ("host", "auto"):
            d.read(data, threads=int(rng.integers(1, 9)), entropy=mode)
            got = d.reconstruct()
            assert got.shape == exp.shape and np.array_equal(got, exp), (t, w, h, sub, q, dri, prog, opt, mode, d.entropy_used)
    d.close()


# ---------------------------------------------------------------------------------------------------------------
# encoder direction of the block pipeline: pixels in HBM -> quantised coefficient planes in HBM
# ---------------------------------------------------------------------------------------------------------------
def _forward_on_device(info, img, frames=1):
    torch = _torch()
    h, w = img.shape[:2]
    nc = 1 if img.ndim == 2 else img.shape[2]
    px = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    launched = frames
    if frames > 1:
        # the launch gets one frame more: its second frame is another picture (this one turned round), the ones behind it are `img`
        # again.  The caller sees the frames of `img` alone, and they are right only if pixel_frame_stride and coef_frame_stride are used
        launched = frames + 1
        other = torch.from_numpy(np.ascontiguousarray(img[::-1, ::-1])).cuda()
        px = torch.stack([other if f == 1 else px for f in range(launched)]).contiguous()
    coef = torch.full((launched, int(info.coef_count)), 0x5A5A, dtype=torch.int16, device="cuda")
    api.launch_forward(info, px.data_ptr(), coef.data_ptr(), launched, w * nc, h * w * nc, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = coef.cpu().numpy()
    if frames > 1:
        assert not np.array_equal(out[1], out[0])  # (the other picture was read)
        out = np.delete(out, 1, axis=0)
    res = []
    for f in range(frames):
        res.append([out[f, info.coef_offset[c]:info.coef_offset[c] + info.blocks_w[c] * info.blocks_h[c] * 64]
                    .reshape(info.blocks_h[c], info.blocks_w[c], 64) for c in range(info.components)])
    return res


FWD_LAYOUTS = {"444": ((1, 1, 1), (1, 1, 1)), "420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "440": ((1, 1, 1), (2, 1, 1)),
               "411": ((4, 1, 1), (1, 1, 1)), "3x3": ((3, 1, 1), (3, 1, 1)), "4x2": ((4, 1, 1), (2, 1, 1)), "mixed": ((2, 1, 2), (2, 2, 1))}


@pytest.mark.parametrize("sub", list(FWD_LAYOUTS))
@pytest.mark.parametrize("w,h", [(64, 48), (75, 45), (33, 17), (129, 71), (8, 8), (1, 1), (640, 360)])
def test_forward_kernel_vs_oracle(oracle, w, h, sub):
    """Forward L transformation + box downsampling + FDCT + quantiser on the device against the oracle's restatement
    (which is pinned against the reference encoder): every layout, partial blocks, mirrored right edge, missing lines."""
    hs, vs = FWD_LAYOUTS[sub]
    rng = np.random.default_rng(w * 1000 + h)
    img = synth.synth_image(w, h, 40 + w) if (w + h) % 2 else rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    quant = [rng.integers(1, 60, 64), rng.integers(1, 255, 64)]
    info = api.frame_layout(w, h, 3, hs, vs, quant)
    oi = oracle.OjInfo()
    oi.width, oi.height, oi.precision, oi.ncomp = w, h, 8, 3
    for c in range(3):
        oi.hs[c], oi.vs[c], oi.tq[c] = hs[c], vs[c], info.quant_index[c]
        oi.subx[c], oi.suby[c], oi.bw[c], oi.bh[c] = info.subx[c], info.suby[c], info.blocks_w[c], info.blocks_h[c]
        oi.cw[c], oi.ch[c] = -(-w // info.subx[c]), -(-h // info.suby[c])
    for t in range(2):
        for i in range(64):
            oi.quant[t][i] = int(quant[t][i])
    exp = oracle.forward(oi, img, 1)
    got = _forward_on_device(info, img)[0]
    for c in range(3):
        assert np.array_equal(got[c].astype(np.int32), exp[c]), (sub, c, np.argwhere(got[c] != exp[c])[:3].tolist())


@pytest.mark.parametrize("name", ["ref_80x48_420", "ref_100x9_422", "ref_97x61_440", "ref_97x61_3x3", "ref_97x61_mixed", "ref_64x40_q2",
                                  "ref_64x40_q100", "cfg1_512x512_444_q75_ref"])
def test_forward_kernel_reproduces_the_reference_encoders_coefficients(dec, name):
    """The golden files were written by the reference encoder from synth_image(w, h, seed): the device must arrive at the
    coefficients that are in them (blocks that cover samples; the padding blocks belong to the entropy coder)."""
    ent = MANIFEST[name]
    if "seed" not in ent:
        pytest.skip("no recipe for the source picture in the manifest")
    img = synth.synth_image(ent["width"], ent["height"], ent["seed"])
    f = dec.read(golden_jpeg(name))
    info = api.frame_layout(f.width, f.height, 3, list(f.hsamp)[:3], list(f.vsamp)[:3], [list(f.quant[t]) for t in range(4)],
                            quant_index=list(f.quant_index)[:3])
    got = _forward_on_device(info, img, frames=2)
    for c in range(3):
        ref = dec.coefficients(c).reshape(f.blocks_h[c], f.blocks_w[c], 64)
        nby, nbx = (-(-f.height // f.suby[c]) + 7) // 8, (-(-f.width // f.subx[c]) + 7) // 8
        for fr in range(2):
            assert np.array_equal(got[fr][c][:nby, :nbx], ref[:nby, :nbx]), (name, c, fr)
            pad = got[fr][c].copy()
            pad[:nby, :nbx] = 0
            assert not pad.any()


def test_forward_kernel_grey(oracle):
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (50, 70)).astype(np.uint8)
    quant = [rng.integers(1, 40, 64)]
    info = api.frame_layout(70, 50, 1, (1,), (1,), quant, ycbcr=0)
    oi = oracle.OjInfo()
    oi.width, oi.height, oi.precision, oi.ncomp = 70, 50, 8, 1
    oi.hs[0] = oi.vs[0] = oi.subx[0] = oi.suby[0] = 1
    oi.bw[0], oi.bh[0], oi.cw[0], oi.ch[0] = info.blocks_w[0], info.blocks_h[0], 70, 50
    for i in range(64):
        oi.quant[0][i] = int(quant[0][i])
    exp = oracle.forward(oi, img[..., None], 0)
    got = _forward_on_device(info, img)[0]
    assert np.array_equal(got[0].astype(np.int32), exp[0])


@pytest.mark.parametrize("w,h,sub,q,ri,opt", [(512, 512, "444", 75, 0, False), (640, 360, "420", 85, 8, True), (333, 211, "422", 40, 3, False),
                                              (129, 71, "440", 95, 0, True), (1920, 1080, "420", 85, 16, False)])
def test_encoder_pipeline_matches_the_reference_encoder(dec, oracle, w, h, sub, q, ri, opt):
    """mijpeg_encode_image (upload, forward kernel, download, entropy coder) against `jpeg -bl -q .. -s .. -z ..` of the
    reference: the same quantiser tables and the same coefficients, hence -- decoded by anybody -- the same picture."""
    img = synth.synth_image(w, h, 70 + w)
    data = dec.encode(img, q, sub, ri, opt)
    refsub = {"444": "1x1,1x1,1x1", "420": "1x1,2x2,2x2", "422": "1x1,2x1,2x1", "440": "1x1,1x2,1x2"}[sub]
    mine_info, mine = oracle.decode_coefficients(data)
    assert mine_info.restart_interval == ri
    if oracle.have_reference():
        ref = oracle.reference_encode(img, ["-bl", "-q", str(q), "-s", refsub] + (["-z", str(ri)] if ri else []))
        ref_info, refc = oracle.decode_coefficients(ref)
        assert [list(ref_info.quant[0]), list(ref_info.quant[1])[:0]] == [list(mine_info.quant[0]), []]
        for c in range(3):
            nby, nbx = (ref_info.ch[c] + 7) // 8, (ref_info.cw[c] + 7) // 8
            assert np.array_equal(mine[c][:nby, :nbx], refc[c][:nby, :nbx]), c
        assert np.array_equal(oracle.reference_decode(data), oracle.reference_decode(ref))
    # without the reference binary (GPU box): the oracle's forward restatement stands in
    exp = oracle.forward(mine_info, img, 1)
    for c in range(3):
        nby, nbx = (mine_info.ch[c] + 7) // 8, (mine_info.cw[c] + 7) // 8
        assert np.array_equal(mine[c][:nby, :nbx], exp[c][:nby, :nbx]), c
    # and the decoder of this library reads its encoder's stream back to the same pixels as the oracle
    dec.read(data, entropy="auto")
    assert np.array_equal(dec.reconstruct(), oracle.decode(data))


def test_cli_encodes_like_the_reference_cli(tmp_path, oracle):
    import os
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "libjpeg_amd", "bin", "jpeg")
    img = synth.synth_image(200, 120, 77)
    src, dst = tmp_path / "in.ppm", tmp_path / "out.jpg"
    oracle.write_ppm(str(src), img)
    r = subprocess.run([exe, "-bl", "-q", "85", "-s", "1x1,2x2,2x2", "-z", "4", "-h", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = dst.read_bytes()
    info, mine = oracle.decode_coefficients(data)
    exp = oracle.forward(info, img, 1)
    for c in range(3):
        nby, nbx = (info.ch[c] + 7) // 8, (info.cw[c] + 7) // 8
        assert np.array_equal(mine[c][:nby, :nbx], exp[c][:nby, :nbx])
    if oracle.have_reference():
        ref = oracle.reference_encode(img, ["-bl", "-q", "85", "-s", "1x1,2x2,2x2", "-z", "4", "-h"])
        assert np.array_equal(oracle.reference_decode(data), oracle.reference_decode(ref))
    # grey scale
    g = tmp_path / "g.pgm"
    oracle.write_ppm(str(g), img[..., 0])
    r = subprocess.run([exe, "-q", "90", str(g), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert oracle.decode(dst.read_bytes()).shape[:2] == (120, 200)


@pytest.mark.parametrize("w,h,sub,q,ri,opt", [(64, 48, "444", 75, 0, False), (75, 45, "420", 85, 2, True), (129, 71, "422", 30, 5, False),
                                              (33, 17, "411", 95, 1, True), (640, 360, "420", 85, 8, False), (1000, 700, "440", 99, 0, True),
                                              (1920, 1080, "420", 85, 0, False), (8, 8, "444", 50, 0, False), (1, 1, "420", 90, 1, True)])
def test_device_entropy_coder_writes_the_host_coders_stream(dec, oracle, w, h, sub, q, ri, opt):
    """hencode.hip (count, prefix sums, emit with atomicOr, stuffing with RSTn markers) against encoder.cpp: the same bytes;
    noise pictures at high quality make plenty of 0xFF bytes and long codes."""
    rng = np.random.default_rng(w + h)
    img = synth.synth_image(w, h, 90 + w) if w != 1000 else rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    on_device = dec.encode(img, q, sub, ri, opt, coder="gpu")
    on_host = dec.encode(img, q, sub, ri, opt, coder="host")
    assert on_device == on_host
    info, planes = oracle.decode_coefficients(on_device)
    exp = oracle.forward(info, img, 1)
    for c in range(3):
        nby, nbx = (info.ch[c] + 7) // 8, (info.cw[c] + 7) // 8
        assert np.array_equal(planes[c][:nby, :nbx], exp[c][:nby, :nbx])


def test_device_entropy_coder_grey(dec, oracle):
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (123, 77)).astype(np.uint8)
    for ri, opt in ((0, False), (3, True)):
        a = dec.encode(img, 92, "444", ri, opt, coder="gpu")
        assert a == dec.encode(img, 92, "444", ri, opt, coder="host")
        assert np.abs(oracle.decode(a).squeeze().astype(int) - img).max() < 40


def test_encode_batch_of_frames_resident_in_hbm(dec, oracle):
    """mijpeg_encode_batch_device: one forward launch for the batch, the device coder per frame; every stream equals the one
    mijpeg_encode_image makes of the same picture and quantiser tables."""
    import ctypes as C

    torch = _torch()
    w, h, n = 640, 360, 5
    imgs = [synth.synth_image(w, h, 300 + i) for i in range(n)]
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    L = api.lib()
    L.mijpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.mijpeg_quality_tables.restype = None
    L.mijpeg_quality_tables(80, luma.ctypes.data, chroma.ctypes.data)
    info = api.frame_layout(w, h, 3, (2, 1, 1), (2, 1, 1), [luma, chroma], quant_index=[0, 0, 0])
    px = torch.from_numpy(np.stack(imgs)).cuda()
    coef = torch.empty((n, int(info.coef_count)), dtype=torch.int16, device="cuda")
    streams = dec.encode_batch_device(info, px.data_ptr(), coef.data_ptr(), n, w * 3, h * w * 3, restart_mcus=4, optimize=True)
    for i in range(n):
        assert streams[i] == dec.encode(imgs[i], 80, "420", 4, True), i
        assert np.array_equal(oracle.decode(streams[i]).shape, (h, w, 3))



def test_rectangle_service_band_waits(dec, oracle):
    """The host copy of a reconstructed frame arrives in bands (one event each); requests wait for the bands they touch.
    Requests in any order, mixed with device-side requests and with other flags, over frames of changing size, always return
    the frame's pixels."""
    torch = _torch()
    rng = np.random.default_rng(99)
    for w, h, sub in ((4000, 3000, "420"), (640, 480, "444"), (5000, 2500, "422")):
        data = synth.synth_jpeg(w, h, 60 + w, 85, sub, 8)
        f = dec.read(data)
        exp = oracle.decode(data)
        out = np.zeros((h, w, 3), np.uint8)
        # bottom stripe first (waits for every band), then random stripes, then the top
        ys = [h - 8] + [int(y) & ~7 for y in rng.integers(0, h - 8, 12)] + [0]
        for y in ys:
            dec.reconstruct_rect(0, y, w - 1, min(h, y + 8) - 1, out=out)
            assert np.array_equal(out[y:y + 8], exp[y:y + 8]), (w, h, y)
        # a device-side request in between, then another colour mode (new reconstruction, new bands), then the first again
        dev = torch.zeros((h, w * 3), dtype=torch.uint8, device="cuda")
        dec.reconstruct_rect_device(0, 0, w - 1, h - 1, [dev.data_ptr() + c for c in range(3)], [3] * 3, [w * 3] * 3)
        assert np.array_equal(dev.cpu().numpy().reshape(h, w, 3), exp)
        raw = dec.reconstruct(api.FLAG_NO_COLOR_TRANSFORM)
        assert np.array_equal(raw, oracle.decode(data, use_ycbcr=0))
        full = dec.reconstruct()
        assert np.array_equal(full, exp)


# ------------------------------------------------------------------------------------------------------
# 12-bit 4:2:0 frames on the fused kernel (fused420_kernel<12>)
# ------------------------------------------------------------------------------------------------------
KERNEL_12 = {"420": "fused420_kernel<12>", "444": "fused444_12_kernel", "422": "fused422_12_kernel"}


def _k12(name):
    """The 12-bit kernels come in two flavours of the colour stage ("/narrow": every channel's sum in 32 bits, narrow12_colour in
    reconstruct_device.cpp); the kernel is the part in front."""
    return name.split("/")[0]


def _narrow12_admits(ry, rc):
    """reconstruct_device.cpp narrow12_colour, restated: (|y'| + 32776) * 8192 + 14516 |c| < 2^31 with |y'| <= 4.02 ry + 2, |c| <= 4.02 rc + 4"""
    return ((402 * ry + 99) // 100 + 2 + 32776) * 8192 + 14516 * ((402 * rc + 99) // 100 + 4) < 2 ** 31


def _narrow12_chroma_limit(ry):
    rc = 0
    while _narrow12_admits(ry, rc + 1):
        rc += 1
    return rc


@pytest.mark.parametrize("sub", ["420", "444", "422"])
@pytest.mark.parametrize("w,h,dri,scale", [(200, 120, 8, 16), (272, 144, 0, 16), (129, 71, 3, 9), (640, 368, 4, 16), (1, 1, 0, 16), (17, 250, 1, 5)])
def test_fused420_12bit_vs_oracle(dec, oracle, w, h, dri, scale, sub):
    """12-bit extended sequential 4:2:0, 4:4:4 and 4:2:2 frames (synth.to_12bit: the 8-bit stream's entropy coded data with deltas times
    `scale`): the 12-bit flavours of the fused kernels against the oracle (which the CPU tests pin against the reference binary
    on the same kind of stream), against the unfused kernels, and through the stripe service."""
    data = synth.to_12bit(synth.synth_jpeg(w, h, 11 + w, 85, sub, dri), scale)
    f = dec.read(data)
    assert f.precision == 12 and f.sample_bytes == 2
    assert _k12(api.kernel_name(f)) == KERNEL_12[sub], list(f.range_max)
    assert api.kernel_name(f).endswith("/narrow") == _narrow12_admits(f.range_max[0], max(f.range_max[1], f.range_max[2]))
    exp = oracle.decode16(data)
    out = dec.reconstruct()
    assert out.dtype == np.uint16 and np.array_equal(out, exp)
    assert np.array_equal(dec.reconstruct(api.FLAG_FORCE_GENERIC), exp)
    stripes = np.zeros_like(out)
    for y in range(0, h, 16):
        dec.reconstruct_rect(0, y, w - 1, min(h, y + 16) - 1, out=stripes)
    assert np.array_equal(stripes, exp)
    if oracle.have_reference() and w > 1:
        rpx, rerr = oracle.reference_decode_status(data)
        assert rerr == 0 and np.array_equal(np.asarray(rpx).reshape(exp.shape), exp)


@pytest.mark.parametrize("sub", ["420", "444", "422"])
@pytest.mark.parametrize("luma_budget,chroma_budget,fused", [(49151, 45055, True), (49151, 45056, False), (49152, 1000, False), (30000, 45055, True), (45055, 32767, True),
                                                             # the colour stage's 32-bit flavour at its bound and one step beyond, along the bound's curve
                                                             (16000, _narrow12_chroma_limit(16000), True), (16000, _narrow12_chroma_limit(16000) + 1, True),
                                                             (4000, _narrow12_chroma_limit(4000), True), (4000, _narrow12_chroma_limit(4000) + 1, True),
                                                             (32000, _narrow12_chroma_limit(32000), True), (32000, _narrow12_chroma_limit(32000) + 1, True),
                                                             (49151, _narrow12_chroma_limit(49151), True), (49151, _narrow12_chroma_limit(49151) + 1, True)])
def test_extreme_coefficients_at_the_12bit_gates(oracle, luma_budget, chroma_budget, fused, sub):
    """fused420_kernel<12> (and fused444_12_kernel, fused422_12_kernel: same bounds) is admitted by sum |c| q < 49152 (the 32-bit butterflies) and < 45056 for the chroma planes (the
    32-bit colour products).  Blocks right at those bounds with every sign pattern (DC-only, one AC coefficient, dense) must still come
    out like the reference's 64-bit arithmetic; one step beyond, the unfused kernels take the frame (and agree as well)."""
    torch = _torch()
    W, H = 272, 144
    d = api.Decoder(0)
    data = synth.to_12bit(synth.synth_jpeg(W, H, 5, 85, sub, 0))
    f = d.read(data)
    d.close()
    rng = np.random.default_rng(luma_budget + chroma_budget)
    info, _ = oracle.decode_coefficients(data)
    for t in range(4):
        for i in range(64):
            info.quant[t][i] = 3 if i else 4
            f.quant[t][i] = info.quant[t][i]
    info.scan_state_valid = 0
    planes = []
    for c in range(3):
        shape = (info.bh[c], info.bw[c], 64)
        p = np.zeros(shape, np.int32)
        kind = rng.integers(0, 4, size=shape[:2])
        sign = rng.choice([-1, 1], size=shape[:2])
        budget = chroma_budget if c else luma_budget
        p[..., 0] = np.where(kind == 0, sign * (budget // 4), 0)  # DC alone: q[0] = 4
        k = rng.integers(1, 64, size=shape[:2])
        for by in range(shape[0]):
            for bx in range(shape[1]):
                if kind[by, bx] == 1:
                    p[by, bx, k[by, bx]] = sign[by, bx] * (budget // 3)  # one AC coefficient carries everything
                elif kind[by, bx] >= 2:
                    v = rng.integers(-40, 41, size=64)
                    v[0] = 0
                    v = (v * ((budget // 3) / max(1, int(np.abs(v).sum())))).astype(np.int64)
                    v[1] += np.sign(v[1] or 1) * (budget // 3 - int(np.abs(v).sum()))
                    p[by, bx] = v
        # one block per plane spends the budget to the last unit: DC (q = 4) plus one AC step (q = 3)
        p[0, 0] = 0
        nb = next(b for b in range(4) if (budget - 3 * b) % 4 == 0)
        p[0, 0, 0] = (budget - 3 * nb) // 4
        p[0, 0, 9] = -nb
        planes.append(p)
    for c in range(3):
        q = np.array(info.quant[info.tq[c]], np.int64)
        f.range_max[c] = int((np.abs(planes[c]).astype(np.int64) * q).sum(axis=2).max())
    assert f.range_max[0] <= luma_budget and f.range_max[1] <= chroma_budget and f.range_max[2] <= chroma_budget
    assert f.range_max[0] == luma_budget and f.range_max[1] == chroma_budget, list(f.range_max)
    assert (_k12(api.kernel_name(f)) == KERNEL_12[sub]) == fused, (api.kernel_name(f), list(f.range_max))
    assert api.kernel_name(f).endswith("/narrow") == (fused and _narrow12_admits(luma_budget, chroma_budget)), (api.kernel_name(f), list(f.range_max))
    exp = oracle.reconstruct16(info, planes)
    coef = torch.from_numpy(np.concatenate([p.astype(np.int16).reshape(-1) for p in planes])).cuda()
    row = W * 6
    out = torch.zeros((H, row), dtype=torch.uint8, device="cuda")
    ws_bytes = api.workspace_bytes(f, 1)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, row, H * row, workspace=ws.data_ptr(), workspace_bytes=ws_bytes,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = out.cpu().numpy().view(np.uint16).reshape(H, W, 3)
    bad = int((res != exp).sum())
    assert bad == 0, f"{api.kernel_name(f)}: {bad} differing samples, first at {np.argwhere(res != exp)[:4].tolist()}"


def test_fused420_12bit_large_frame_properties(dec):
    """A 4K 12-bit frame: fused and unfused kernels agree band by band; an odd row stride takes the unaligned store path."""
    data = synth.to_12bit(synth.synth_jpeg(3840, 2160, 77, 85, "420", 8))
    f = dec.read(data)
    assert _k12(api.kernel_name(f)) == "fused420_kernel<12>", list(f.range_max)
    a = dec.reconstruct()
    b = dec.reconstruct(api.FLAG_FORCE_GENERIC)
    assert [_sha(a[y:y + 135]) for y in range(0, 2160, 135)] == [_sha(b[y:y + 135]) for y in range(0, 2160, 135)]


@pytest.mark.parametrize("w,h,scale", [(200, 120, 16), (129, 71, 9), (1000, 700, 16), (1, 1, 16), (7, 300, 3)])
def test_fused1_12bit_vs_oracle(dec, oracle, w, h, scale):
    """12-bit single-component frames (what medical pictures are) on fused1_kernel<12>: against the oracle, the unfused kernels,
    the reference binary where present; plus one block per gate value through the stateless launch."""
    import io

    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth.synth_image(w, h, 21 + w)).convert("L").save(b, "JPEG", quality=85)
    data = synth.to_12bit(b.getvalue(), scale)
    f = dec.read(data)
    assert f.precision == 12 and f.components == 1 and api.kernel_name(f) == "fused1_kernel<12>", list(f.range_max)
    exp = oracle.decode16(data)
    out = dec.reconstruct()
    assert out.dtype == np.uint16 and np.array_equal(out.reshape(exp.shape), exp)
    assert np.array_equal(dec.reconstruct(api.FLAG_FORCE_GENERIC).reshape(exp.shape), exp)
    if oracle.have_reference() and w > 1:
        rpx, rerr = oracle.reference_decode_status(data)
        assert rerr == 0 and np.array_equal(np.asarray(rpx).reshape(exp.shape), exp)
    # the gate: sum |c| q = 49151 in every block (DC alone, one AC coefficient, both signs) stays on the kernel, 49152 leaves it
    torch = _torch()
    info, _ = oracle.decode_coefficients(data)
    for i in range(64):
        info.quant[0][i] = 1
        f.quant[0][i] = 1
    info.scan_state_valid = 0
    rng = np.random.default_rng(w)
    p = np.zeros((info.bh[0], info.bw[0], 64), np.int32)
    k = rng.integers(0, 64, size=p.shape[:2])
    sgn = rng.choice([-1, 1], size=p.shape[:2])
    for by in range(p.shape[0]):
        for bx in range(p.shape[1]):
            p[by, bx, k[by, bx]] = sgn[by, bx] * 24575
            p[by, bx, (k[by, bx] + 7) % 64] = -sgn[by, bx] * 24576
    f.range_max[0] = 49151
    assert api.kernel_name(f) == "fused1_kernel<12>"
    f.range_max[0] = 49152
    assert api.kernel_name(f) != "fused1_kernel<12>"
    f.range_max[0] = 49151
    expg = oracle.reconstruct16(info, [p])
    coef = torch.from_numpy(p.astype(np.int16).reshape(-1)).cuda()
    row = w * 2
    outg = torch.zeros((h, row), dtype=torch.uint8, device="cuda")
    api.launch_reconstruct(f, coef.data_ptr(), outg.data_ptr(), 1, row, h * row, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(outg.cpu().numpy().view(np.uint16).reshape(expg.shape), expg)


# ------------------------------------------------------------------------------------------------
# fused_tile_kernel: every layout without a dedicated fused kernel in one pass through LDS (round 3)
@pytest.mark.gpu
def test_fused_tile_kernel_on_random_layouts(oracle):
    """One to four components, sampling factors 1..4 x 1..4, sizes 1..140 (tiles cut by the frame, halo blocks at every edge),
    DRI: the one-pass kernel (FAST, its int16 and int32 sample planes, and SAFE arithmetic) and the two-kernel pair it
    replaces all equal the oracle's whole-frame reconstruction; 12-bit twins of some of them as well."""
    import craft
    from libjpeg_amd import synth
    dec = api.Decoder(0)
    names = set()
    n = 0
    for t in range(160):
        rng = np.random.default_rng(88000 + t)
        samp, w, h, dri = craft.random_layout(rng)
        data = craft.craft_stream(rng, samp, w, h, dri, ac_density=0.15 if t % 3 else 0.02)
        if t % 5 == 0 and len(samp) in (1, 3):
            data = synth.to_12bit(data, 16)
        info, planes = oracle.decode_coefficients(data)
        exp = oracle.reconstruct(info, planes) if info.precision == 8 else oracle.reconstruct16(info, planes)
        f = dec.read(data, entropy="host")
        names.add(api.kernel_name(f))
        for flags in (0, api.FLAG_FORCE_SAFE, api.FLAG_FORCE_GENERIC):
            got = dec.reconstruct(flags)
            assert np.array_equal(got, exp), (t, samp, w, h, dri, info.precision, flags, api.kernel_name(f, flags))
        n += 1
    dec.close()
    assert "fused_tile_kernel" in names and n == 160


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", EDGE_SIZES + [(640, 360), (1921, 1083)])
@pytest.mark.parametrize("nc", [3, 4])
def test_fused_flat_kernel_vs_oracle(dec, oracle, nc, w, h):
    """Every component 1 x 1 and no colour transformation -- CMYK, RGB stored as such (four / three components): one lane per
    block position, bytes packed behind every transform, the interleaved line a byte permutation (fused_flat_kernel).  Edge
    sizes (tiles cut by the frame on both sides), DRI, dense and sparse content; SAFE and the unfused pair give the same."""
    import craft
    rng = np.random.default_rng(9100 + 7 * w + h + nc)
    data = craft.craft_stream(rng, [(1, 1)] * nc, w, h, dri=(w + h) % 4, ac_density=0.02 if (w + h) % 3 else 0.2)
    info, planes = oracle.decode_coefficients(data)
    flags = api.FLAG_NO_COLOR_TRANSFORM if nc == 3 else 0
    f = dec.read(data, entropy="host")
    assert api.kernel_name(f, flags) == "fused_flat_kernel", list(f.range_max)
    exp = oracle.reconstruct(info, planes, use_ycbcr=0)
    out = dec.reconstruct(flags)
    assert np.array_equal(out, exp), (nc, w, h, np.argwhere(out != exp)[:4].tolist())
    assert np.array_equal(dec.reconstruct(flags | api.FLAG_FORCE_SAFE), exp) and np.array_equal(dec.reconstruct(flags | api.FLAG_FORCE_GENERIC), exp)


@pytest.mark.gpu
def test_fused_flat_kernel_on_the_references_rgb_files(dec, oracle):
    """`jpeg -c` (RGB stored as such, a merging specification with the identity L transformation) at 4:4:4 and the CMYK fixture:
    the files the kernel is for, against the reference decoder's pixels."""
    names = [n for n in MANIFEST if n.startswith("refc_") and "444" in n] + ["pil_90x60_cmyk"]
    assert len(names) >= 2
    for name in names:
        f = dec.read(golden_jpeg(name))
        if all(f.subx[c] == 1 and f.suby[c] == 1 for c in range(f.components)) and f.components in (3, 4):
            assert api.kernel_name(f) == "fused_flat_kernel", name
        assert np.array_equal(dec.reconstruct(), golden_pixels(name)), name


@pytest.mark.gpu
def test_fused_tile_kernel_on_big_frames(oracle):
    """Frames of many tiles in layouts the dedicated kernels do not cover -- CMYK, 3x1, 1x4, luma subsampled against chroma,
    two components -- with dense content: hashes of the one-pass kernel equal those of the generic pair (which the test above
    and the goldens tie to the oracle), and one of them is checked against the oracle directly."""
    import craft
    dec = api.Decoder(0)
    layouts = [[(1, 1)] * 4, [(3, 1), (1, 1), (1, 1)], [(1, 4), (1, 1), (1, 1)], [(1, 1), (2, 2), (2, 2)], [(2, 1), (1, 2)], [(4, 2), (2, 1), (1, 2), (2, 2)]]
    for k, samp in enumerate(layouts):
        rng = np.random.default_rng(4400 + k)
        w, h = 1000 + 37 * k, 700 + 13 * k
        data = craft.craft_stream(rng, samp, w, h, dri=[0, 7][k % 2], ac_density=0.12)
        f = dec.read(data, entropy="host")
        assert api.kernel_name(f) == ("fused_flat_kernel" if k == 0 else "fused_tile_kernel")  # (four components 1 x 1: no LDS round trip)
        a = dec.reconstruct(0)
        b = dec.reconstruct(api.FLAG_FORCE_GENERIC)
        c = dec.reconstruct(api.FLAG_FORCE_SAFE)
        assert np.array_equal(a, b) and np.array_equal(a, c), samp
        if k == 1:
            assert np.array_equal(a, oracle.decode(data))
    dec.close()


@pytest.mark.parametrize("luma_budget", [7599, 7600, 16383])  # below / at the int16 luma line of the two-wave flavour, at the kernel's gate
@pytest.mark.parametrize("is_float", [1, 0])
def test_hidden_bit_kernel_on_adversarial_coefficients(oracle, luma_budget, is_float):
    """fusedxtw420_kernel in both flavours -- round 6's two waves per SIMD (legacy luma through LDS as int16, the residual chain
    finished where the samples are packed, results kept in sixteen bits with 65536 as 65535) and round 5's -- on synthetic
    coefficient planes that drive the residual samples to both ends of their range (DC coefficients that saturate the Q clamp,
    dense blocks at the 65535 gate, sums that make the reference's IDCT<4,QUAD> wrap) and the legacy luma plane to its budget:
    bit for bit the unfused kernels' output (idct_planes + xt_merge: the literal chain in 64-bit sums, pinned by the oracle
    in test_xt_hidden_residual_bits_1080p_vs_oracle)."""
    if not oracle.have_reference():
        pytest.skip("needs oracle/_ref/jpeg to encode the HDR stream the layout comes from")
    import ctypes as C

    torch = _torch()
    W, H = 264, 136
    data = oracle.reference_encode_hdr(synth.synth_hdr(W, H, 3), ["-r", "-q", "85", "-Q", "90", "-h", "-profile", "c", "-r12", "-rR", "4", "-s", "1x1,2x2,2x2"])
    d = api.Decoder(0)
    f = d.read(data)
    xt = d.xt_params()
    assert api.kernel_name(f, xt=xt) == "fusedxtw420_kernel" and xt.residual_wide
    rng = np.random.default_rng(luma_budget * 2 + is_float)
    n16 = int(f.coef_count)
    buf = np.zeros(n16, np.int16)
    # legacy planes (int16): random sparse blocks scaled to the budget; component 0 spends it exactly somewhere
    for c in range(3):
        bw, bh = f.blocks_w[c], f.blocks_h[c]
        q = np.array(f.quant[f.quant_index[c]], np.int64)
        p = np.zeros((bh, bw, 64), np.int64)
        budget = luma_budget if c == 0 else 2000
        for by in range(bh):
            for bx in range(bw):
                k = rng.integers(0, 64, size=3)
                s = rng.choice([-1, 1], size=3)
                share = budget // 3
                for kk, ss in zip(k, s):
                    p[by, bx, kk] += ss * (share // q[kk])
        p[0, 0] = 0
        p[0, 0, 0] = budget // q[0]
        p[0, 0, 1] = -((budget - (budget // q[0]) * q[0]) // q[1])
        rm = int((np.abs(p) * q).sum(axis=2).max())
        assert rm <= budget
        f.range_max[c] = rm if c else budget  # (the host's range check: what selects the flavour)
        off = int(f.coef_offset[c])
        buf[off:off + p.size] = p.reshape(-1).astype(np.int16)
    # residual planes (int32, two int16 slots each): DC at both ends, dense noise, sums near the 65535 gate
    r = xt.residual
    wide = np.zeros((n16 - int(r.coef_offset[0])) // 2, np.int32)
    for c in range(3):
        bw, bh = r.blocks_w[c], r.blocks_h[c]
        q = np.array(r.quant[r.quant_index[c]], np.int64)
        p = np.zeros((bh, bw, 64), np.int64)
        kind = rng.integers(0, 4, size=(bh, bw))
        for by in range(bh):
            for bx in range(bw):
                if kind[by, bx] == 0:
                    p[by, bx, 0] = rng.choice([-1, 1]) * (65000 // q[0])  # saturates the Q table's clamp one way or the other
                elif kind[by, bx] == 1:
                    v = rng.integers(-30, 31, size=64)
                    tot = int((np.abs(v) * q).sum())
                    p[by, bx] = v * max(1, 60000 // max(tot, 1))
                else:
                    k = rng.integers(0, 64)
                    p[by, bx, k] = rng.choice([-1, 1]) * (64000 // q[k])
        rm = int((np.abs(p) * q).sum(axis=2).max())
        assert rm < 65536
        xt.residual.range_max[c] = rm
        off = (int(r.coef_offset[c]) - int(r.coef_offset[0])) // 2
        wide[off:off + p.size] = p.reshape(-1).astype(np.int32)
    buf[int(r.coef_offset[0]):] = wide.view(np.int16)
    xt.is_float = is_float
    f.is_float = is_float
    coef = torch.from_numpy(buf).cuda()
    row = W * 6
    outs = []
    for flags in (0, api.FLAG_FORCE_GENERIC):
        out = torch.zeros((H, row), dtype=torch.uint8, device="cuda")
        wsb = api.workspace_bytes(f, 1, flags=flags, xt=xt)
        ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device="cuda")
        api.launch_reconstruct(f, coef.data_ptr(), out.data_ptr(), 1, row, H * row, n16, flags=flags, workspace=ws.data_ptr(), workspace_bytes=wsb,
                               stream=torch.cuda.current_stream().cuda_stream, xt=xt)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().view(np.uint16).reshape(H, W, 3))
    d.close()
    bad = int((outs[0] != outs[1]).sum())
    assert bad == 0, f"{bad} differing samples, first at {np.argwhere(outs[0] != outs[1])[:4].tolist()}"
    assert len(np.unique(outs[0])) > 50  # (not a constant picture: both ends of the range and what lies between)

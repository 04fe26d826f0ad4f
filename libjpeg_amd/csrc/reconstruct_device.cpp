// reconstruct_device.cpp -- the reconstruction of decoded coefficients on the device: which kernel takes a batch and in which
// flavour (plan_reconstruct), its workspace, its argument block and its launch, stateless (mijpeg_launch_reconstruct) and on a
// decoder object's stream (reconstruct_on).  There is NO CPU fallback.  Private to libmijpeg.so.
#include <string.h>

#include <algorithm>
#include <string>

#include "fused_list.hpp"
#include "reconstruct.hpp"

using namespace mij;

Sampling sampling_of(const mijpeg_info &f)
{
  if (f.components == 1) return Sampling::GREY;
  if (f.components != 3 || f.hsamp[1] != 1 || f.vsamp[1] != 1 || f.hsamp[2] != 1 || f.vsamp[2] != 1) return Sampling::OTHER;
  const int h = f.hsamp[0], v = f.vsamp[0];
  return h == 2 && v == 2 ? Sampling::S420 : h == 2 && v == 1 ? Sampling::S422 : h == 1 && v == 2 ? Sampling::S440
         : h == 4 && v == 1 ? Sampling::S411 : h == 1 && v == 1 ? Sampling::S444 : Sampling::OTHER;
}

// The fused kernels address inside a frame with 32-bit byte offsets (planes and pixels; frames are 64 bits apart): frames
// beyond that -- a 65535 x 65535 picture has 8.6 GB of luma coefficients and 12.9 GB of pixels -- take the generic kernels,
// whose addressing is 64 bits wide throughout.
// DNL frames (mijpeg_info::dnl): the vertical filter of a subsampled component reads the line below the picture's last one,
// and when the picture ends on a block row boundary that line belongs to the block row the first scan creates behind the
// picture -- unless it met the marker before it got there.  Then the row does not exist, the reference reads NULL and
// transforms it to samples of value 0 (control/blockbitmaprequester.cpp:1097-1108, dct/idct.cpp:336-338): no coefficients
// give that, the unfused kernels write the zeros themselves (GenericArgs::zero_from).
static bool dnl_row_missing(const mijpeg_info &f)
{
  if (!f.dnl) return false;
  for (int c = 0; c < f.components && c < MIJPEG_MAX_COMPONENTS; c++) {
    const int ch = (f.height + f.suby[c] - 1) / f.suby[c];
    if (f.suby[c] > 1 && (ch & 7) == 0 && f.rows[c] <= (ch >> 3)) return true;
  }
  return false;
}

static bool fits32(const mijpeg_batch *b)
{
  const mijpeg_info &f = b->info;
  const uint64_t lim = 0xffffffffull;
  if (f.coef_wide) return false; // int32 coefficients (damaged stream): the unfused kernels' business
  if (dnl_row_missing(f)) return false; // (the fused kernels have no way to say "this block row is NULL")
  for (int c = 0; c < f.components; c++)
    if ((uint64_t)f.blocks_w[c] * (uint64_t)f.blocks_h[c] * 128u > lim) return false;
  if (f.xt && b->xt)
    for (int c = 0; c < b->xt->residual.components; c++)
      if ((uint64_t)b->xt->residual.blocks_w[c] * (uint64_t)b->xt->residual.blocks_h[c] * 128u > lim) return false;
  if (b->out_row_stride < 0) return false; // bottom-up bitmaps: the offsets are unsigned
  // (a batch description without strides -- mijpeg_kernel_name, mijpeg_workspace_bytes asked ahead of time -- is taken to
  // have tightly packed lines)
  const uint64_t line = (uint64_t)f.width * (uint64_t)f.components * (f.xt ? (uint64_t)(f.sample_bytes > 1 ? 2 : 1) : f.precision > 8 ? 2u : 1u);
  const uint64_t rs = b->out_row_stride ? (uint64_t)b->out_row_stride : line;
  return (uint64_t)f.height * rs + line <= lim;
}

// every delta << 4 a signed 16-bit operand (the fast transforms)
static bool deltas_fit16(const mijpeg_info &f)
{
  if (f.components > MIJPEG_MAX_COMPONENTS) return false;
  for (int c = 0; c < f.components; c++) {
    if ((unsigned)f.quant_index[c] >= 4) return false;
    for (int i = 0; i < 64; i++)
      if (f.quant[f.quant_index[c]][i] > 2047) return false;
  }
  return true;
}

// The 12-bit kernels' colour stage in one 32-bit sum per channel (colour12<true>, kernels.hip): the luma sample times 16 is at most
// 4.02 * range_max[0] + 2 in magnitude, a chroma sample behind the upsampling filters 4.02 * range_max[c] + 4 (the bounds of
// the 12-bit gate of plan_reconstruct; the filters are convex combinations plus a rounding), so (|y'| + 32776) * 8192 + 14516 |c| --
// 14516 is the largest weight a channel puts on chroma, 2819 + 5850 the green one's -- stays below 2^31 where this holds.  Monotone
// in every range: a speculative launch that assumed larger ranges and selected the flavour holds for the smaller ones.
static bool narrow12_colour(const mijpeg_info &f)
{
  if (f.precision != 12 || f.components != 3) return false;
  const int64_t ry = f.range_max[0], rc = std::max(f.range_max[1], f.range_max[2]);
  if (ry <= 0 || rc < 0) return false;
  const int64_t sum = ((402 * ry + 99) / 100 + 2 + 32776) * 8192 + 14516 * ((402 * rc + 99) / 100 + 4);
  return sum < ((int64_t)1 << 31);
}

// JPEG XT: the L transformation in force for this launch.  A request without colour transformation (the command line's -c)
// replaces the STANDARD YCbCr transformation by the identity and leaves everything else of the merge alone
// (colortrafo/colortransformerfactory.cpp:231-232: `if (ltrafo == YCbCr && disabletorgb) ltrafo = Identity`)
static bool xt_ltrafo_ycbcr(const mijpeg_batch *b)
{
  const mijpeg_xt_params &x = *b->xt;
  return x.ltrafo_ycbcr && !((b->flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM) && x.ltrafo_standard);
}

// JPEG XT profile C in the shape the fused kernels cover (the legacy frame's part is plan_reconstruct's): 12-bit 4:4:4
// residual frame of the legacy frame's size, L transformation on, the residual frame within the range the fast transforms
// are exact for
static bool fused_xt_shape(const mijpeg_batch *b)
{
  const mijpeg_xt_params &x = *b->xt;
  const mijpeg_info &r = x.residual;
  if (x.general) return false; // free-form matrices, table gathers, DCT bypass: xt_merge_general_kernel
  if (x.no_residual) return false; // (a legacy codestream without its EOI: the unfused merge kernels know how to merge nothing)
  // hidden bits in the RESIDUAL frame (-rR n: 13..16-bit samples, int32 coefficients) have a kernel of their own
  // (fusedxtw420_kernel); hidden bits in the legacy frame change its precision and stay on the three-kernel path
  if (x.hidden_bits || x.residual_hidden_bits < 0 || x.residual_hidden_bits > 4 || (x.residual_wide != 0) != (x.residual_hidden_bits > 0) ||
      x.ltable_entries != 256 || !xt_ltrafo_ycbcr(b) || r.precision != 12 || r.components != 3 || x.out_max != 65535 || x.out_shift != 32768)
    return false;
  for (int c = 0; c < 3; c++)
    if (r.subx[c] != 1 || r.suby[c] != 1 || r.blocks_w[c] != r.blocks_w[0] || r.blocks_h[c] != r.blocks_h[0] || r.range_max[c] >= GATE_XT_RESIDUAL)
      return false;
  return deltas_fit16(r) && r.width == b->info.width && r.height == b->info.height;
}

// Which kernel reconstructs a batch, and in which flavour: the one place that decides it (mijpeg_kernel_name,
// mijpeg_workspace_bytes and launch_reconstruct_ex each ask once).  Safe on any batch description, a JPEG XT frame without
// its parameter block and a batch without strides included.  (A rectangle request needs MIJPEG_FLAG_FORCE_GENERIC, which
// alone rules out the fused, flat and tile kernels.)
ReconPlan plan_reconstruct(const mijpeg_batch *b)
{
  const mijpeg_info &f = b->info;
  const int32_t *r = f.range_max;
  const bool generic = b->flags & MIJPEG_FLAG_FORCE_GENERIC, safe = b->flags & MIJPEG_FLAG_FORCE_SAFE;
  const bool ycc = f.ycbcr && !(b->flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM); // (the fused three-component kernels transform colour)
  const bool deltas16 = deltas_fit16(f); // (false for more components than a frame can have)
  const auto chroma_below = [&](int32_t gate) { return r[1] < gate && r[2] < gate; };
  ReconPlan p{};
  p.sampling = sampling_of(f);
  p.fast = f.fast_arith && !safe && !f.coef_wide && deltas16;
  const auto plan = [&](Recon k) { p.kernel = k; return p; };
  if (f.xt) {
    // (fast_arith itself is never set for XT frames: the generic kernels run SAFE on them; the fused ones check the range here)
    if (b->xt && p.sampling == Sampling::S420 && f.precision == 8 && !generic && !safe && deltas16 && r[0] < GATE_XT_LEGACY &&
        chroma_below(GATE_XT_LEGACY) && fits32(b) && fused_xt_shape(b))
      return plan(b->xt->residual_hidden_bits ? Recon::FUSEDXTW420 : Recon::FUSEDXT420);
    if (f.coef_wide) return plan(Recon::PAIR_LONG);
    if (f.components == 1) return plan(Recon::XT_MERGE1);
    return plan(b->xt && b->xt->general ? Recon::XT_MERGE_GENERAL : Recon::XT_MERGE);
  }
  if (f.coef_wide) return plan(Recon::PAIR_LONG); // int32 coefficients (damaged stream)
  const bool fits = f.components >= 1 && f.components <= MIJPEG_MAX_COMPONENTS && fits32(b); // (no missing DNL row either)
  if (fits && !generic && f.precision == 8) {
    // single components: samples travel as packed int16
    if (p.sampling == Sampling::GREY && p.fast && r[0] < GATE_FUSED8) return plan(Recon::FUSED1);
    // 4:2:0 in any range; the packed flavour filters (Cb, Cr) pairs in 16 bits: every chroma sample * 16 is bounded by
    // 4 * range_max, and the filter sums a + 3 b + r by four times that.  Where the first-pass results of every transform fit
    // 16 bits its second pass runs on v_dot2 as well (MIJPEG_FLAG_FORCE_DOT2, for testing: whatever the range check says).
    if (p.sampling == Sampling::S420 && ycc) {
      if (!p.fast || !chroma_below(GATE_PACKED)) return plan(Recon::FUSED420);
      p.dot2 = !b->quant_dev && ((b->flags & MIJPEG_FLAG_FORCE_DOT2) || (r[0] < GATE_DOT2 && chroma_below(GATE_DOT2)));
      return plan(Recon::FUSED420P);
    }
    // 4:2:2, 4:4:0 (what a losslessly rotated 4:2:2 picture is), 4:1:1, 4:4:4: chroma samples travel through LDS as int16 pairs
    // (4 * range_max < 32768); 4:2:2 and 4:4:0 filter on the pairs below the packed gate, on 32-bit values between the two
    if (p.sampling != Sampling::GREY && p.sampling != Sampling::OTHER && ycc && p.fast && chroma_below(GATE_FUSED8)) {
      const Sampling s = p.sampling;
      p.wide = (s == Sampling::S422 || s == Sampling::S440) && !chroma_below(GATE_PACKED);
      return plan(s == Sampling::S422 ? Recon::FUSED422 : s == Sampling::S440 ? Recon::FUSED440 : s == Sampling::S411 ? Recon::FUSED411 : Recon::FUSED444);
    }
  }
  // 12 bit (SOF1, P = 12): 4:2:0, 4:2:2, 4:4:4 and single components inside the ranges the 12-bit flavours are exact for: every
  // delta << 4 a signed 16-bit operand; sum |c| q < 49152 bounds every butterfly intermediate by 1573 * 16 * 49152 < 2^31 (first
  // pass; the second pass sees at most 22.2 * range_max per column) and every multiplicand by 2^23; chroma sum |c| q < 45056 bounds
  // the chroma samples (times 16) by 4.02 * 45056 + 2 < 181 200 (|basis| <= 1/4 per coefficient, the 9-bit constants and the
  // roundings add < 0.5 %), whose products with the colour constants (11485; 2819 + 5850; 14516 taken as 4 * 3629) fit 32 bits.
  // (The horizontal filter of 4:2:2 weighs samples below 2^18 with 4 in total.)
  if (fits && !generic && f.precision == 12 && !safe && deltas16 && r[0] > 0 && r[0] < GATE_12_LUMA) {
    if (p.sampling == Sampling::GREY) return plan(Recon::FUSED1_12);
    const Sampling s = p.sampling;
    if ((s == Sampling::S420 || s == Sampling::S422 || s == Sampling::S444) && ycc && chroma_below(GATE_12_CHROMA)) {
      p.narrow12 = narrow12_colour(f);
      return plan(s == Sampling::S420 ? Recon::FUSED420_12 : s == Sampling::S422 ? Recon::FUSED422_12 : Recon::FUSED444_12);
    }
  }
  // every component 1 x 1, three or four of them, 8 bit, no colour transformation, fast arithmetic: fused_flat_kernel
  // (CMYK; RGB stored as such -- Adobe transform 0, a merging specification with the identity L transformation, the caller's
  // MIJPEG_FLAG_NO_COLOR_TRANSFORM on a 4:4:4 frame)
  bool flat = f.precision == 8 && !b->quant_dev && !generic && (f.components == 4 || (f.components == 3 && !ycc)) && p.fast && fits;
  for (int c = 0; c < f.components && flat; c++)
    flat = f.subx[c] == 1 && f.suby[c] == 1 && f.blocks_w[c] == f.blocks_w[0] && f.blocks_h[c] == f.blocks_h[0];
  if (flat) return plan(Recon::FLAT);
  // plain JPEG frames of any layout go through LDS in one pass (fused_tile_kernel); the pair with its sample planes in HBM
  // stays for per-frame tables in device memory, MIJPEG_FLAG_FORCE_GENERIC (rectangle requests) and missing DNL rows
  if (b->quant_dev || generic || dnl_row_missing(f)) return plan(Recon::PAIR);
  // 12-bit frames of the tile kernel: the bounds of the 12-bit gate above, the chroma one for every component (the upsampling
  // filters weigh two samples, < 2^18 each with the level shift, with at most 8 in total: far inside the fast flavour's 24-bit
  // operands and 32-bit sums)
  p.fast12 = f.precision == 12 && !safe && deltas16 && r[0] > 0;
  for (int c = 0; c < f.components && p.fast12; c++) p.fast12 = r[c] < GATE_12_CHROMA;
  return plan(Recon::TILE);
}

// per Recon: the name, and that of the flavour (ReconPlan::wide, ReconPlan::narrow12) where the kernel has one
static const char *const RECON_NAMES[][2] = {
    {"fused420p_kernel", nullptr},
    {"fused420_kernel", nullptr},
    {"fused422_kernel", "fused422_kernel<wide>"},
    {"fused440_kernel", "fused440_kernel<wide>"},
    {"fused411_kernel", nullptr},
    {"fused444_kernel", nullptr},
    {"fused1_kernel", nullptr},
    {"fused420_kernel<12>", "fused420_kernel<12>/narrow"},
    {"fused422_12_kernel", "fused422_12_kernel/narrow"},
    {"fused444_12_kernel", "fused444_12_kernel/narrow"},
    {"fused1_kernel<12>", nullptr},
    {"fusedxt420_kernel", nullptr},
    {"fusedxtw420_kernel", nullptr},
    {"fused_flat_kernel", nullptr},
    {"fused_tile_kernel", nullptr},
    {"idct_planes_kernel+upsample_color_kernel", nullptr},
    {"idct_planes_long_kernel+upsample_color_kernel", nullptr},
    {"idct_planes_kernel+xt_merge_kernel", nullptr},
    {"idct_planes_kernel+xt_merge_general_kernel", nullptr},
    {"idct_planes_kernel+xt_merge1_kernel", nullptr},
};
static_assert(sizeof(RECON_NAMES) / sizeof(RECON_NAMES[0]) == (size_t)Recon::XT_MERGE1 + 1, "one name per kernel");

static const size_t LUT_BYTES = 3 * 4096 * sizeof(int32_t);

// JPEG XT with real Q / R2 tables (mijpeg_xt_params.general): they travel in the workspace behind everything else
static size_t xt_table_bytes(const mijpeg_batch *b)
{
  if (!b->info.xt || !b->xt || !b->xt->general) return 0;
  size_t n = 0;
  for (int c = 0; c < 3; c++) {
    if (b->xt->qtable[c]) n += (size_t)b->xt->qtable_entries * sizeof(int32_t);
    if (b->xt->r2table[c]) n += ((size_t)(b->xt->out_max + 1) << 4) * sizeof(int32_t);
  }
  return n;
}

// per-frame tables (quant_dev) are expanded to the transforms' operands (deltas << 4, int32) in the workspace
static size_t expanded_tables_bytes(const mijpeg_batch *b) { return b->quant_dev ? (size_t)b->frames * 4 * 64 * sizeof(int32_t) : 0; }

static bool is_fused_xt(Recon k) { return k == Recon::FUSEDXT420 || k == Recon::FUSEDXTW420; }

size_t workspace_need(const mijpeg_batch *b, const ReconPlan &p)
{
  if (is_fused_xt(p.kernel)) return LUT_BYTES;
  if (p.kernel < Recon::FUSEDXT420) return expanded_tables_bytes(b);
  // [LUT_BYTES: L lookup tables (JPEG XT, up to 3 x 4096 entries)] [per frame: int32 sample planes, one sample per
  // coefficient: coef_count of them, fewer when the residual planes hold 32-bit coefficients] [expanded per-frame tables]
  // [JPEG XT tables]
  return LUT_BYTES + (size_t)b->info.coef_count * sizeof(int32_t) * (size_t)b->frames + expanded_tables_bytes(b) + xt_table_bytes(b);
}

// JPEG XT: the three L tables of the merging specification into the front of the workspace
static bool upload_ltables(const mijpeg_batch *b, size_t entries, hipStream_t s)
{
  for (int c = 0; c < 3; c++)
    if (hipMemcpyAsync((int32_t *)b->workspace + (size_t)c * entries, b->xt->ltable[c], entries * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess)
      return false;
  return true;
}

// the kernels up to FUSEDXTW420 (uploads the L tables of the JPEG XT ones)
static int fused_args_of(const mijpeg_batch *b, const ReconPlan &p, const int32_t *qdev, hipStream_t s, FusedXtArgs &xa)
{
  const mijpeg_info &f = b->info;
  memset(&xa, 0, sizeof(xa));
  Fused420Args &a = xa.base;
  fused_geometry(f, p.sampling, a);
  a.coef = b->coef_dev;
  a.coef_frame_stride = b->coef_frame_stride;
  a.out = b->out_dev;
  a.out_frame_stride = b->out_frame_stride;
  a.row_stride = b->out_row_stride;
  a.frames = b->frames;
  for (int c = 0; c < 3; c++)
    fill_deltas(a.q[c], f.quant[f.quant_index[c]]);
  a.qdev = qdev;
  if (!is_fused_xt(p.kernel)) return MIJPEG_OK;
  const mijpeg_xt_params &x = *b->xt;
  const mijpeg_info &r = x.residual;
  for (int c = 0; c < 3; c++) {
    xa.ext.off_r[c] = r.coef_offset[c];
    for (int i = 0; i < 64; i++) xa.ext.rq[c][i] = (int32_t)r.quant[r.quant_index[c]][i] << 4;
  }
  if (!upload_ltables(b, 256, s)) return MIJPEG_ERR_DEVICE;
  xa.ext.bw_r = r.blocks_w[0];
  xa.ext.bh_r = r.blocks_h[0];
  xa.ext.ltable = (const int32_t *)b->workspace;
  xa.ext.rtrafo_ycbcr = x.rtrafo_ycbcr;
  xa.ext.is_float = x.is_float;
  xa.ext.out_max = x.out_max;
  xa.ext.out_shift = x.out_shift;
  xa.ext.rprecision = r.precision + x.residual_hidden_bits;
  // (the two-wave flavour of the hidden-bit kernel keeps the luma block as int16: sample * 16 + 2056 with |sample * 16| <= 4 sum |c| q)
  xa.luma_fits16 = f.range_max[0] < GATE_INT16_SAMPLES ? 1 : 0;
  return MIJPEG_OK;
}

// plane pn of the unfused kernels and the tile kernels: component c of frame g, reconstructed at `precision` bits
static void generic_plane(GenericArgs &a, int pn, const mijpeg_info &g, int c, int precision, int64_t &sample_off)
{
  a.coef_off[pn] = g.coef_offset[c];
  a.sample_off[pn] = sample_off;
  sample_off += (int64_t)g.blocks_w[c] * g.blocks_h[c] * 64;
  a.bw[pn] = g.blocks_w[c];
  a.bh[pn] = g.blocks_h[c];
  a.subx[pn] = g.subx[c];
  a.suby[pn] = g.suby[c];
  a.cw[pn] = (g.width + g.subx[c] - 1) / g.subx[c];
  a.ch[pn] = (g.height + g.suby[c] - 1) / g.suby[c];
  if (g.dnl && g.suby[c] > 1) { // no bottom edge (fused_geometry); rows nobody created are NULL: zeros
    if ((a.ch[pn] & 7) == 0 && g.rows[c] <= (a.ch[pn] >> 3)) a.zero_from[pn] = g.rows[c];
    a.ch[pn] = g.blocks_h[c] * 8;
  }
  a.dcoff[pn] = (1 << (precision - 1)) << 7;
  fill_deltas(a.q[pn], g.quant[g.quant_index[c]]);
}

// JPEG XT: the residual planes and the merge (uploads the L tables and, for general frames, the Q / R2 tables)
static int xt_args_of(const mijpeg_batch *b, size_t need, int lprec, int64_t &sample_off, hipStream_t s, GenericArgs &a)
{
  const mijpeg_info &f = b->info;
  const mijpeg_xt_params &x = *b->xt;
  const int rprec = x.residual.precision + x.residual_hidden_bits;
  // (a parameter block filled in before the lossless flavours existed has zeros there: with clamping that means four bits)
  const int xrbits = (x.rbits == 0 && x.clamp) ? 4 : x.rbits;
  if (x.hidden_bits < 0 || x.hidden_bits > 4 || x.residual_hidden_bits < 0 || x.residual_hidden_bits > 4 || rprec - (x.rct ? 1 : 0) > 16 ||
      x.ltable_entries != (256 << x.hidden_bits) || (x.residual_wide != 0) != (x.residual_hidden_bits > 0 || x.residual.precision > 12) ||
      (xrbits != 4 && !(x.general && x.rdct_bypass)) || (x.rct && (x.clamp || xrbits != 1)) || (!x.clamp && !x.general))
    return MIJPEG_ERR_INVALID_PARAMETER;
  // the flavours without clamping (RCT, lossless identity) index their Q tables directly: a caller-made block without them is refused
  if ((x.rct || !x.clamp) && !x.no_residual)
    for (int c = 0; c < x.residual.components && c < 3; c++)
      if (!x.qtable[c]) return MIJPEG_ERR_INVALID_PARAMETER;
  for (int c = 0; c < x.residual.components && c < 3; c++) generic_plane(a, 3 + c, x.residual, c, rprec, sample_off); // (one component: planes 4, 5 stay empty)
  if (!x.residual.components) // (no residual frame at all -- a specification without a residual codestream: the merge reads nothing there)
    for (int pn = 3; pn < 6; pn++) a.subx[pn] = a.suby[pn] = 1;
  // int32 planes: beyond 12 bits (hidden bits included) the reference transforms with IDCT<4,QUAD>, up to 12 with the LONG
  // flavour like every other frame (codestream/tables.cpp:1876-1891) -- the same numbers until a damaged scan leaves a
  // coefficient that overflows 32 bits on the way (an 8-bit alpha residual with one hidden bit and 52 241 in a block:
  // tools/xt_gpu_damage_campaign.py, seed 2002)
  if (x.residual_wide) { a.wide_first = 3; a.wide_count = 3; a.wide_long = rprec <= 12 ? 1 : 0; }
  a.ltable_entries = x.ltable_entries;
  a.nplanes = 6;
  a.xt = 1;
  a.ycbcr = xt_ltrafo_ycbcr(b) ? 1 : 0; // the L transformation of the merging specification, or the identity the -c switch puts in its place
  a.rtrafo_ycbcr = x.rtrafo_ycbcr;
  a.out_shift = x.out_shift;
  a.out_max = x.out_max;
  a.is_float = x.is_float;
  a.rprecision = rprec;
  a.xt_no_residual = x.no_residual;
  a.xt_rct = x.rct;
  a.xt_noclamp = x.clamp ? 0 : 1;
  a.xt_rbits = x.residual.components ? xrbits : 4;
  a.legacy32 = lprec == 8 && f.range_max[0] < GATE_XT_LEGACY && f.range_max[1] < GATE_XT_LEGACY && f.range_max[2] < GATE_XT_LEGACY &&
               !(b->flags & MIJPEG_FLAG_FORCE_SAFE);
  a.ltable = (const int32_t *)b->workspace;
  if (!upload_ltables(b, (size_t)x.ltable_entries, s)) return MIJPEG_ERR_DEVICE;
  if (!x.general) return MIJPEG_OK;
  if (x.residual.components && x.qtable_entries != (1 << (rprec - (xrbits == 1) + xrbits))) return MIJPEG_ERR_INVALID_PARAMETER; // (no residual frame: no Q tables)
  a.xt_general = 1;
  a.rbypass = x.rdct_bypass;
  a.rnoise = x.noise_shaping;
  a.rdcshift = (1 << rprec) >> 1;
  memcpy(a.lmat, x.lmat, sizeof(a.lmat));
  memcpy(a.rmat, x.rmat, sizeof(a.rmat));
  memcpy(a.cmat, x.cmat, sizeof(a.cmat));
  char *tp = (char *)b->workspace + (need - xt_table_bytes(b)); // real Q / R2 tables: behind everything else in the workspace
  for (int c = 0; c < 3; c++) {
    // only the highest-frequency delta is used, with the colour bits folded in (residualblockhelper.cpp:351-364)
    // (m_usQuantization is a UWORD: deltas >= 4096 wrap; shifted where the path has more than one fractional bit)
    a.rquant63[c] = xrbits > 1 ? ((int32_t)x.residual.quant[x.residual.quant_index[c]][63] << xrbits) & 0xffff : (int32_t)x.residual.quant[x.residual.quant_index[c]][63];
    // (components that share a table share its copy)
    for (int j = 0; j < c; j++) {
      if (x.qtable[c] && x.qtable[j] == x.qtable[c]) a.qlut[c] = a.qlut[j];
      if (x.r2table[c] && x.r2table[j] == x.r2table[c]) a.r2lut[c] = a.r2lut[j];
    }
    if (x.qtable[c] && !a.qlut[c]) {
      const size_t n = (size_t)x.qtable_entries * sizeof(int32_t);
      if (hipMemcpyAsync(tp, x.qtable[c], n, hipMemcpyHostToDevice, s) != hipSuccess) return MIJPEG_ERR_DEVICE;
      a.qlut[c] = (const int32_t *)tp;
      tp += n;
    }
    if (x.r2table[c] && !a.r2lut[c]) {
      const size_t n = ((size_t)(x.out_max + 1) << 4) * sizeof(int32_t);
      if (hipMemcpyAsync(tp, x.r2table[c], n, hipMemcpyHostToDevice, s) != hipSuccess) return MIJPEG_ERR_DEVICE;
      a.r2lut[c] = (const int32_t *)tp;
      tp += n;
    }
  }
  return MIJPEG_OK;
}

// every other kernel: the plane description
static int generic_args_of(const mijpeg_batch *b, const ReconPlan &p, size_t need, const int32_t *qdev, const RequestExtra *rx, hipStream_t s, GenericArgs &a)
{
  const mijpeg_info &f = b->info;
  memset(&a, 0, sizeof(a));
  a.coef = b->coef_dev;
  a.coef_frame_stride = b->coef_frame_stride;
  a.samples = (int32_t *)((char *)b->workspace + LUT_BYTES);
  a.sample_frame_stride = f.coef_count;
  a.out = b->out_dev;
  a.out_frame_stride = b->out_frame_stride;
  a.row_stride = b->out_row_stride;
  a.width = f.width;
  a.height = f.height;
  a.ncomp = f.components;
  a.ycbcr = (f.ycbcr && !(b->flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM)) ? 1 : 0;
  a.frames = b->frames;
  a.qdev = qdev;
  a.nplanes = f.components;
  a.sample_bytes = f.xt ? (b->xt->out_max > 255 ? 2 : 1) : f.precision > 8 ? 2 : 1;
  // JPEG XT frames reconstruct at their precision plus the bits that travelled in hidden refinement scans
  // (Frame::HiddenPrecisionOf, marker/frame.cpp:368-373)
  const int lprec = f.precision + (f.xt ? b->xt->hidden_bits : 0);
  int64_t sample_off = 0;
  for (int c = 0; c < f.components; c++) generic_plane(a, c, f, c, lprec, sample_off);
  if (f.coef_wide) { a.wide_first = 0; a.wide_count = f.components; a.wide_long = 1; }
  // int16 sample planes between the two kernels: |sample * 16| <= 2048 (level shift) + 4 * range_max must fit 16 bits
  a.narrow = p.fast && !f.xt && f.precision == 8;
  for (int c = 0; c < f.components && a.narrow; c++)
    if (f.range_max[c] >= GATE_INT16_SAMPLES) a.narrow = 0;
  a.maxval = (1 << lprec) - 1;
  a.dcshift = (1 << (lprec - 1)) << 4;
  if (f.xt)
    if (const int rc = xt_args_of(b, need, lprec, sample_off, s, a)) return rc;
  if (rx) {
    a.rowmap = rx->rowmap_dev;
    a.rowmap_stride = rx->rowmap_stride;
    a.request = 1;
    a.req_x0 = rx->corner_x;
    a.req_y0 = rx->corner_y;
    a.y_base = rx->y_base;
    a.y_count = rx->y_count;
    for (int c = 0; c < a.nplanes && c < MAXP; c++) {
      a.wstart[c] = rx->wstart[c];
      a.wlimit[c] = rx->wlimit[c];
    }
    if (!f.xt) a.ycbcr = rx->ycc; // the colour transformer the first request built (colortransformerfactory.cpp:220-221)
  }
  return MIJPEG_OK;
}

int launch_reconstruct_ex(const mijpeg_batch *b, void *stream, const RequestExtra *rx)
{
  // what no kernel takes, before anything is planned or enqueued
  if (!b || !b->coef_dev || !b->out_dev || b->frames < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (rx && !(b->flags & MIJPEG_FLAG_FORCE_GENERIC)) return MIJPEG_ERR_INVALID_PARAMETER;
  if (b->quant_dev && b->info.xt) return MIJPEG_ERR_OPERATION_UNIMPLEMENTED; // per-frame tables: plain JPEG only
  const mijpeg_info &f = b->info;
  if ((f.precision != 8 && f.precision != 12) || f.components < 1 || f.components > 4) return MIJPEG_ERR_OPERATION_UNIMPLEMENTED;
  if (f.xt && (!b->xt || (f.components != 3 && f.components != 1))) return MIJPEG_ERR_MISSING_PARAMETER; // (one component: grey scale with a residual)
  if (f.coef_wide && (f.xt || b->quant_dev)) return MIJPEG_ERR_INVALID_PARAMETER; // int32 planes: single plain JPEG frames only
  const ReconPlan p = plan_reconstruct(b);
  const size_t need = workspace_need(b, p);
  if (need && (!b->workspace || b->workspace_bytes < need)) return MIJPEG_ERR_MISSING_PARAMETER;
  hipStream_t s = (hipStream_t)stream;
  const int32_t *qdev = nullptr;
  if (b->quant_dev) {
    int32_t *dst = (int32_t *)((char *)b->workspace + (need - expanded_tables_bytes(b) - xt_table_bytes(b)));
    if (launch_expand_deltas(b->quant_dev, dst, b->frames, s)) return MIJPEG_ERR_DEVICE;
    qdev = dst;
  }
  int rc;
  if (p.kernel <= Recon::FUSEDXTW420) {
    FusedXtArgs xa;
    if (const int arc = fused_args_of(b, p, qdev, s, xa)) return arc;
    rc = launch_fused(p, xa, s);
  } else {
    GenericArgs a;
    if (const int arc = generic_args_of(b, p, need, qdev, rx, s, a)) return arc;
    rc = p.kernel == Recon::FLAT ? launch_fused_flat(a, s) : p.kernel == Recon::TILE ? launch_fused_tile(a, p.fast || p.fast12, s) : -1;
    if (rc == -1) rc = launch_generic(a, p.fast, s); // (also where no tile of fused_tile_kernel fits LDS)
  }
  return rc ? MIJPEG_ERR_DEVICE : MIJPEG_OK;
}

mijpeg_batch batch_of(const mijpeg_info &info, const int16_t *coef_dev, void *out_dev, int64_t row_stride, int64_t frame_stride, int frames, uint32_t flags)
{
  mijpeg_batch b;
  memset(&b, 0, sizeof(b));
  b.info = info;
  b.coef_dev = coef_dev;
  b.coef_frame_stride = info.coef_count;
  b.out_dev = (uint8_t *)out_dev;
  b.out_row_stride = row_stride;
  b.out_frame_stride = frame_stride;
  b.frames = frames;
  b.flags = flags;
  return b;
}

ReconPlan plan_list_member(const mijpeg_info &f, const int16_t *coef_dev, void *out_dev, int64_t row_stride, uint32_t flags)
{
  static const uint16_t per_frame_tables = 0; // (quant_dev is only tested by the planner: the list launches read their own tables)
  mijpeg_batch b = batch_of(f, coef_dev, out_dev, row_stride, 0, 1, flags);
  b.quant_dev = &per_frame_tables;
  return plan_reconstruct(&b);
}

int reconstruct_on(mijpeg_decoder *d, mijpeg_batch &b, const RequestExtra *rx, const char *noun)
{
  const size_t ws = workspace_need(&b, plan_reconstruct(&b));
  if (ws) {
    const int rc = ensure_dev(d, (void **)&d->ws_dev, &d->ws_cap, ws);
    if (rc) return rc;
    b.workspace = d->ws_dev;
    b.workspace_bytes = d->ws_cap;
  }
  const int rc = launch_reconstruct_ex(&b, d->stream, rx);
  if (rc && noun)
    set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError())
                                             : std::string("reconstruction not available for this ") + noun);
  return rc;
}

int reconstruct_view(mijpeg_decoder *d, int comp, void *dst_device, int64_t row_stride, uint32_t flags, int sync)
{
  HIP_TRY(d, hipSetDevice(d->device));
  const mijpeg_info v = view_of(d->host.info, comp);
  mijpeg_batch b = batch_of(v, d->coef_dev + (comp < 0 ? 0 : d->host.info.coef_offset[comp]), dst_device, row_stride, row_stride * v.height, 1, flags);
  b.xt = d->host.is_xt() ? &d->host.xt : nullptr;
  if (const int rc = reconstruct_on(d, b, nullptr, "stream")) return rc;
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
}

// ------------------------------------------------------------------------------------------------
// planar output
// ------------------------------------------------------------------------------------------------
int planar_check(const mijpeg_info &f, void *const *planes, int64_t row_stride)
{
  if (f.components < 1 || f.components > MIJPEG_MAX_COMPONENTS || f.width < 1 || f.height < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  for (int c = 0; c < f.components; c++)
    if (!planes[c]) return MIJPEG_ERR_INVALID_PARAMETER;
  return row_stride >= (int64_t)f.width * sample_bytes_of(f) ? MIJPEG_OK : MIJPEG_ERR_INVALID_PARAMETER;
}

int launch_fused_lists(mijpeg_decoder *d, const FusedListItem *items, const std::vector<FusedListLaunch> &launches, bool planar, bool window)
{
  if (launches.empty()) return 0;
  const std::vector<FusedListTable> tables = fused_list_layout(launches, planar, window);
  const size_t bytes = tables.back().end;
  PinnedUpload &u = d->list_tables;
  if (const int rc = pinned_upload_reserve(d, u, bytes)) return rc;
  for (size_t l = 0; l < launches.size(); l++) fused_list_fill(u.host, tables[l], launches[l], items, planar, window);
  if (const int rc = pinned_upload_send(d, u, bytes)) return rc;
  for (size_t l = 0; l < launches.size(); l++) {
    Fused420Args a;
    memset(&a, 0, sizeof(a));
    a.coef = d->coef_dev;
    a.frames = (int32_t)launches[l].members.size();
    a.ragged = (const RaggedFrame *)(u.dev + tables[l].frames);
    a.ragged_first = (const uint32_t *)(u.dev + tables[l].first);
    a.qdev = (const int32_t *)(u.dev + tables[l].deltas);
    const bool planes = planar && !(window && launches[l].p.sampling == Sampling::GREY); // (a window call's grey launches: their own plane)
    if (planes) a.out = u.dev + tables[l].planes; // (the PlanarFrame table: kernels.hpp; a window launch finds its WindowFrame table behind it)
    else if (window) a.out = u.dev + tables[l].windows;
    if (launch_fused_list(launches[l].p, a, (unsigned)launches[l].grid, planes, d->stream, window))
      return set_error(d, MIJPEG_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
  }
  return (int)launches.size();
}

// what deinterleave_kernel takes: an interleaved picture (or a rectangle of one: src at its first sample) -> a plane per component
static DeinterleaveArgs deinterleave_args(const void *src, int64_t src_row, int components, int sample_bytes, int32_t width, int32_t height, void *const *planes,
                                          int64_t row_stride)
{
  DeinterleaveArgs a;
  memset(&a, 0, sizeof(a));
  a.src = (const uint8_t *)src; a.src_row = src_row;
  a.ncomp = components; a.sample_bytes = sample_bytes; a.width = width; a.height = height;
  for (int c = 0; c < components; c++) a.dst[c] = (uint8_t *)planes[c];
  a.dst_row = row_stride;
  return a;
}

int staged_rect_out(mijpeg_decoder *d, const uint8_t *full, const mijpeg_info &f, const mijpeg_rect &w, void *const *ptrs, int64_t row_stride, bool planar)
{
  const int sb = sample_bytes_of(f);
  const int64_t bpp = (int64_t)f.components * sb, line = (int64_t)f.width * bpp;
  const int32_t cw = w.max_x - w.min_x + 1, ch = w.max_y - w.min_y + 1;
  const uint8_t *src = full + (int64_t)w.min_y * line + (int64_t)w.min_x * bpp;
  if (!planar) {
    HIP_TRY(d, hipMemcpy2DAsync(ptrs[0], (size_t)row_stride, src, (size_t)line, (size_t)(cw * bpp), (size_t)ch, hipMemcpyDeviceToDevice, d->stream));
    return MIJPEG_OK;
  }
  return launch_deinterleave(deinterleave_args(src, line, f.components, sb, cw, ch, ptrs, row_stride), d->stream) ? MIJPEG_ERR_DEVICE : MIJPEG_OK;
}

int reconstruct_staged(mijpeg_decoder *d, mijpeg_batch &b, uint8_t *staging, const mijpeg_rect &w, void *const *ptrs, int64_t row_stride, bool planar)
{
  b.out_dev = staging;
  b.out_row_stride = (int64_t)b.info.width * b.info.components * sample_bytes_of(b.info);
  b.out_frame_stride = b.out_row_stride * b.info.height;
  const int rc = reconstruct_on(d, b, nullptr, nullptr);
  return rc ? rc : staged_rect_out(d, staging, b.info, w, ptrs, row_stride, planar);
}

int reconstruct_planar_items(mijpeg_decoder *d, const PlanarItem *items, int n, uint32_t flags, RaggedFailures &failures, const int *image_of)
{
  std::vector<FusedListItem> fused;
  std::vector<FusedListLaunch> launches;
  std::vector<int> two_pass;
  size_t staging = 0;
  for (int i = 0; i < n; i++) {
    const PlanarItem &it = items[i];
    const mijpeg_info &f = *it.info;
    if (f.components == 1) { two_pass.push_back(i); continue; } // (its own plane: the existing kernel, no second pass)
    const ReconPlan p = plan_list_member(f, it.coef_dev, it.planes[0], it.row_stride, flags);
    if (f.components != 3 || f.precision != 8 || f.xt || !planar_twin(p) || fused_list_tiles(f) > 0x7fffffffull) {
      two_pass.push_back(i);
      staging = std::max(staging, picture_bytes(f));
      continue;
    }
    fused_list_add(launches, p, (int)fused.size(), f);
    fused.push_back(FusedListItem{&f, it.coef_dev - d->coef_dev, {it.planes[0], it.planes[1], it.planes[2]}, it.row_stride, it.own_deltas}); // (every item's store lies in the object's)
  }
  const int made = launch_fused_lists(d, fused.data(), launches, true);
  if (made < 0) return made;
  d->planar_stats.fused_launches += made;
  d->planar_stats.fused += (int32_t)fused.size();
  // the others: the staged second pass with the whole picture as the rectangle
  if (const int rc = ensure_dev(d, (void **)&d->planar_tmp_dev, &d->planar_tmp_cap, staging)) return rc; // (nobody staged: nothing to grow)
  for (int i : two_pass) {
    const PlanarItem &it = items[i];
    const mijpeg_info &f = *it.info;
    const bool own_plane = f.components == 1; // (one pass either way for a single component)
    mijpeg_batch b = batch_of(f, it.coef_dev, it.planes[0], it.row_stride, it.row_stride * f.height, 1, flags);
    b.xt = it.xt;
    b.quant_dev = it.own_deltas_dev;
    const int rc = own_plane ? reconstruct_on(d, b, nullptr, nullptr)
                             : reconstruct_staged(d, b, d->planar_tmp_dev, mijpeg_rect{0, 0, f.width - 1, f.height - 1}, it.planes, it.row_stride, true);
    if (!rc) (own_plane ? d->planar_stats.fused : d->planar_stats.two_pass)++;
    if (!rc && !own_plane) d->planar_stats.two_pass_launches++;
    failures.note(image_of ? image_of[i] : i, rc);
  }
  return failures.code;
}

extern "C" {

int mijpeg_planar_stats_get(mijpeg_decoder *d, mijpeg_planar_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->planar_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_planar_stats_get"); }

int mijpeg_deinterleave_device(mijpeg_decoder *d, const void *src_device, int64_t src_row_stride, int32_t width, int32_t height, int32_t components,
                               int32_t sample_bytes, void *const planes[MIJPEG_MAX_COMPONENTS], int64_t row_stride)
try {
  if (!d || !src_device || !planes || width < 1 || height < 1 || components < 1 || components > MIJPEG_MAX_COMPONENTS || (sample_bytes != 1 && sample_bytes != 2))
    return MIJPEG_ERR_INVALID_PARAMETER;
  for (int c = 0; c < components; c++)
    if (!planes[c]) return MIJPEG_ERR_INVALID_PARAMETER;
  if (row_stride < (int64_t)width * sample_bytes || src_row_stride < (int64_t)width * sample_bytes * components) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  if (launch_deinterleave(deinterleave_args(src_device, src_row_stride, components, sample_bytes, width, height, planes, row_stride), d->stream)) return hip_fail(d, hipGetLastError(), "deinterleave_kernel launch");
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_deinterleave_device"); }

const char *mijpeg_kernel_name(const mijpeg_batch *b)
try {
  if (!b) return "";
  const ReconPlan p = plan_reconstruct(b);
  return RECON_NAMES[(int)p.kernel][p.wide || p.narrow12 ? 1 : 0];
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_kernel_name"); return nullptr; }

size_t mijpeg_workspace_bytes(const mijpeg_batch *b)
try {
  return b ? workspace_need(b, plan_reconstruct(b)) : 0;
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_workspace_bytes"); return 0; }

int mijpeg_launch_reconstruct(const mijpeg_batch *b, void *stream)
try {
  return launch_reconstruct_ex(b, stream, nullptr);
} catch (...) { return boundary_catch(nullptr, "mijpeg_launch_reconstruct"); }

} // extern "C"

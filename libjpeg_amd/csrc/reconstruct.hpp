// reconstruct.hpp -- what reconstruct_device.cpp (kernel selection, workspace and launch of the reconstruction) shares with the
// decoder object's entry points in capi.cpp, batch_decode.cpp, rect_service.cpp, ragged_decode.cpp and ragged_reconstruct.cpp.
// Private to libmijpeg.so.
#pragma once
#include "decoder.hpp"
#include "kernels.hpp"
#include "ragged_failures.hpp"
#include "rect_request.hpp"

// The range gates of the kernel selection (plan_reconstruct): a kernel or flavour is admitted where mijpeg_info::range_max
// (sum |c| q of a block) is below its gate
constexpr int32_t GATE_DOT2 = 1477;          // fused420p_kernel's second pass on v_dot2 (idct_columns_dot2: sum |c| q <= 1476)
constexpr int32_t GATE_PACKED = 2047;        // chroma filtered as int16 pairs (packed 4:2:0, 4:2:2, 4:4:0)
constexpr int32_t GATE_INT16_SAMPLES = 7600; // int16 sample planes of the kernel pair; int16 luma of fusedxtw420_kernel<true>
constexpr int32_t GATE_FUSED8 = 8190;        // chroma of the 8-bit fused 4:2:2 / 4:4:0 / 4:1:1 / 4:4:4 kernels, fused1_kernel
constexpr int32_t GATE_XT_LEGACY = 16384;    // legacy frame of the JPEG XT kernels (fused, and the merge's 32-bit colour stage)
constexpr int32_t GATE_12_CHROMA = 45056;    // 12-bit fused kernels: chroma (every component of fused_tile_kernel's fast12)
constexpr int32_t GATE_12_LUMA = 49152;      // 12-bit fused kernels: luma
constexpr int32_t GATE_XT_RESIDUAL = 65536;  // residual frame of the fused JPEG XT kernels
constexpr int32_t RANGE_GATES[] = { // (ascending)
    GATE_DOT2, GATE_PACKED, GATE_INT16_SAMPLES, GATE_FUSED8, GATE_XT_LEGACY, GATE_12_CHROMA, GATE_12_LUMA, GATE_XT_RESIDUAL};

mij::Sampling sampling_of(const mijpeg_info &f);
// Which kernel reconstructs a batch, and in which flavour; what it needs as workspace
mij::ReconPlan plan_reconstruct(const mijpeg_batch *b);
size_t workspace_need(const mijpeg_batch *b, const mij::ReconPlan &p);
// ... of one frame as a member of a list launch, which brings per-frame tables
mij::ReconPlan plan_list_member(const mijpeg_info &f, const int16_t *coef_dev, void *out_dev, int64_t row_stride, uint32_t flags);

// A frame as the fused kernels address it, into g (Fused420Args, RaggedFrame, the planner's mijpeg_ragged_frame): its size, the
// luma and chroma planes in blocks and where they start in the coefficient store, valid chroma samples, the grid of 128 x 128 tiles
template <class Frame> void fused_geometry(const mijpeg_info &f, mij::Sampling s, Frame &g)
{
  const bool colour = f.components > 1;
  g.width = f.width; g.height = f.height;
  g.off_y = f.coef_offset[0]; g.off_cb = colour ? f.coef_offset[1] : 0; g.off_cr = colour ? f.coef_offset[2] : 0;
  g.bw_y = f.blocks_w[0]; g.bh_y = f.blocks_h[0]; g.bw_c = colour ? f.blocks_w[1] : 0; g.bh_c = colour ? f.blocks_h[1] : 0;
  const bool full_height = s == mij::Sampling::S422 || s == mij::Sampling::S411; // (chroma subsampled horizontally only)
  g.cw = s == mij::Sampling::S440 ? f.width : s == mij::Sampling::S411 ? (f.width + 3) / 4 : (f.width + 1) / 2;
  g.ch = full_height ? f.height : (f.height + 1) / 2;
  // DNL frames: the reference's upsamplers never learnt the height (upsampling/upsamplerbase.cpp:61-75), their line buffers
  // have no bottom edge: below the last chroma line comes what the block rows hold (the padding of the last one, then the
  // MCU row the first scan created behind the picture: the store has it, include/mijpeg.h) instead of that line again
  if (f.dnl && !full_height && colour) g.ch = g.bh_c * 8;
  g.tiles_x = (f.width + 127) / 128; g.tiles_y = (f.height + 127) / 128;
}

// rx: what a rectangle request that does not show the plain picture adds to a launch (RequestExtra, rect_request.hpp)
int launch_reconstruct_ex(const mijpeg_batch *b, void *stream, const RequestExtra *rx);

// `frames` frames of `info`, their coefficient stores one behind the other from coef_dev, to out_dev (strides in bytes)
mijpeg_batch batch_of(const mijpeg_info &info, const int16_t *coef_dev, void *out_dev, int64_t row_stride, int64_t frame_stride, int frames, uint32_t flags);

// The batch on the object's stream: sizes the workspace, grows d->ws_dev, launches, sets the object's error ("... not available
// for this <noun>"; no noun: the code alone, the caller reports)
int reconstruct_on(mijpeg_decoder *d, mijpeg_batch &b, const RequestExtra *rx, const char *noun);
// The decoded frame -- or, without upsampling, component `comp` of it on its own grid (view_of, rect_request.hpp) -- on the
// object's stream into dst_device; sync: the call waits for it
int reconstruct_view(mijpeg_decoder *d, int comp, void *dst_device, int64_t row_stride, uint32_t flags, int sync);

// ---- lists of differently shaped frames in fused launches (fused_list.hpp: items, launches, table layout) ----
struct FusedListItem;
struct FusedListLaunch;
// The launches on the object's stream (nothing is waited for): their tables into d->list_tables once the last call's upload
// has left it, one upload, one launch_fused_list each.  -> the number of launches made, or the (negative) error, set on the object.
// window: the launches run the items' crop windows (FusedListItem::window, every item has one); a planar window call's
// one-component launches are their own plane and take the interleaved window flavour.
int launch_fused_lists(mijpeg_decoder *d, const FusedListItem *items, const std::vector<FusedListLaunch> &launches, bool planar, bool window = false);

// ---- planar output: component planes instead of interleaved pixels ----
// One picture of a planar call: its frame description and coefficient store (in the object's device memory), where its planes go.
struct PlanarItem {
  const mijpeg_info *info;
  const int16_t *coef_dev;
  void *planes[MIJPEG_MAX_COMPONENTS]; // device; [0 .. components)
  int64_t row_stride;                  // bytes per line of every plane
  const uint16_t *own_deltas = nullptr;     // host, [4][64] per COMPONENT: the frame's own tables in a batch that has them (else info's)
  const uint16_t *own_deltas_dev = nullptr; // ... and their place on the device
  const mijpeg_xt_params *xt = nullptr;
};
constexpr uint32_t PLANAR_FLAGS = MIJPEG_FLAG_FORCE_SAFE | MIJPEG_FLAG_FORCE_GENERIC | MIJPEG_FLAG_NO_COLOR_TRANSFORM; // what the planar calls take
// bytes per sample of a frame's reconstruction; of the whole picture, interleaved with tightly packed lines
inline int sample_bytes_of(const mijpeg_info &f) { return f.xt ? (f.sample_bytes > 1 ? 2 : 1) : f.precision > 8 ? 2 : 1; }
inline size_t picture_bytes(const mijpeg_info &f) { return (size_t)f.height * (size_t)f.width * (size_t)f.components * (size_t)sample_bytes_of(f); }
// MIJPEG_ERR_INVALID_PARAMETER where a plane of a component the frame has is missing or row_stride is below a line of samples
int planar_check(const mijpeg_info &f, void *const *planes, int64_t row_stride);
// The staged second pass, on the object's stream: rectangle w (inclusive) of the full picture at `full` (interleaved, tightly packed
// lines) to ptrs -- a strided device copy to ptrs[0], or (planar) deinterleave_kernel to a plane each ...
int staged_rect_out(mijpeg_decoder *d, const uint8_t *full, const mijpeg_info &f, const mijpeg_rect &w, void *const *ptrs, int64_t row_stride, bool planar);
// ... behind the first: the frame of b in full, as the existing kernels write it, into `staging` (b's destination is set here; the
// stream orders one picture after the other), and its rectangle w to ptrs.  No message: the caller reports.
int reconstruct_staged(mijpeg_decoder *d, mijpeg_batch &b, uint8_t *staging, const mijpeg_rect &w, void *const *ptrs, int64_t row_stride, bool planar);
// The items on the object's stream (nothing is waited for): those whose plan (plan_list_member) has a planar twin share one launch
// of it per kernel and flavour; the others take the staged second pass through planar_tmp_dev.  One-component frames are their own
// plane.  Adds to d->planar_stats.  An item that fails does not stop the others: item i is noted in `failures` (empty on entry) as
// image image_of[i] (i without a map).  -> what ends the call with nothing noted (a whole launch that fails), or the first noted code.
int reconstruct_planar_items(mijpeg_decoder *d, const PlanarItem *items, int n, uint32_t flags, RaggedFailures &failures, const int *image_of = nullptr);

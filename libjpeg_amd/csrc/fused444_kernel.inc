// fused444_kernel.inc -- the text of fused444_kernel, included by kernels.hip (see there: once in mij, once in mij::planar, and in
// mij::window and mij::window::planar, where WINDOW_OUT is true: the crop windows of a list)
// ==============================================================================================
// fused 4:4:4 kernel (three components, no subsampling, YCbCr): ReconstructUnsampled,
// control/blockbitmaprequester.cpp:1013-1074
// ==============================================================================================
// One lane owns one block POSITION and transforms its Cb, Cr and Y blocks one after the other; the two
// chroma results are kept as packed int16 pairs (32 + 32 VGPRs) that the colour multiply-adds read half by half
// (v_mad_i32_i16 op_sel), the luma result stays in 64 VGPRs.  No barrier, no halo, LDS only for the coalesced
// block fetch.  FAST arithmetic only, and only when the host's range check bounds every chroma sample by
// 4 * range_max < 32768 (so the packing is exact); everything else takes the generic two-kernel path.
// Algorithmic bytes: 3 x 2 B in + 3 B out = 9 B/pixel.
template <int MINW, bool QDEV, bool RAGGED = false>
__global__ __launch_bounds__(F420_THREADS, MINW) void fused444_kernel(Fused420Args a)
{
  static_assert(!RAGGED || QDEV, "ragged launches: per-frame tables");
  static_assert(!PLANAR_OUT || RAGGED, "planar output: the ragged flavours");
  static_assert(!WINDOW_OUT || RAGGED, "crop windows: the ragged flavours");
  __shared__ __attribute__((aligned(16))) u32x4 stage_all[4][128];
  PlanarBases pb{};
  WindowBox wb{};
  const TileCtx t = WINDOW_OUT ? tile_enter_window<PLANAR_OUT>(a, stage_all, pb, wb) : PLANAR_OUT ? tile_enter_planar(a, stage_all, pb) : RAGGED ? tile_enter_ragged(a, stage_all) : tile_enter(a, stage_all);
  if (t.padding) return;
  const int frame = t.frame;

  // all three planes have the same geometry (bw_y x bh_y blocks)
  auto fetch = [&](u32x4 (&rows)[8], int64_t plane_off) { fetch_tile_blocks(rows, t, t.coef + plane_off, a.bw_y, a.bh_y); };

  unsigned cbp[32], crp[32];
  {
    u32x4 rows[8];
    int v[64];
    fetch(rows, a.off_cb);
    dequant_idct_sparse<!QDEV>(rows, frame_deltas<QDEV>(a, frame, 1), v);
#pragma unroll
    for (int i = 0; i < 32; i++) cbp[i] = pack_lo16_now(v[2 * i + 1], v[2 * i]);
    __builtin_amdgcn_sched_barrier(0); // keep the next component's loads from being hoisted above this transform (register pressure)
    fetch(rows, a.off_cr);
    dequant_idct_sparse<!QDEV>(rows, frame_deltas<QDEV>(a, frame, 2), v);
#pragma unroll
    for (int i = 0; i < 32; i++) crp[i] = pack_lo16_now(v[2 * i + 1], v[2 * i]);
    __builtin_amdgcn_sched_barrier(0);
  }
  WindowClip wc{};
  const BlockOut o = WINDOW_OUT ? block_out_window<PLANAR_OUT ? 1 : 3>(a, t, wb, wc) : block_out<PLANAR_OUT ? 1 : 3>(a, t);
  int yv[64];
  {
    u32x4 rows[8];
    fetch(rows, a.off_y);
    if (o.outside) return;
    dequant_idct_sparse<!QDEV, true>(rows, frame_deltas<QDEV>(a, frame, 0), yv, 0, LUMA_FOLD_R2);
  }
#pragma unroll
  for (int l = 0; l < 8; l++) {
    if (WINDOW_OUT ? l >= wc.ln0 && l < o.nln : l < o.nln) {
      int rr[8], gg[8], bb[8];
#pragma unroll
      for (int x = 0; x < 8; x++) {
        const int yk = luma13(yv[l * 8 + x]); // (level shift and rounding are inside: LUMA_FOLD_R2)
        const unsigned cb2 = cbp[(l * 8 + x) >> 1], cr2 = crp[(l * 8 + x) >> 1];
        if (x & 1) {
          rr[x] = mad16_hi(cr2, L_CR_R, yk);
          gg[x] = mad16_hi(cr2, -L_CR_G, mad16_hi(cb2, -L_CB_G, yk));
          bb[x] = mad16_hi(cb2, L_CB_B, yk);
        } else {
          rr[x] = mad16_lo(cr2, L_CR_R, yk);
          gg[x] = mad16_lo(cr2, -L_CR_G, mad16_lo(cb2, -L_CB_G, yk));
          bb[x] = mad16_lo(cb2, L_CB_B, yk);
        }
      }
      // (LINE_BY_LINE: one line at a time -- do not interleave the lines' temporaries)
      if (PLANAR_OUT) {
        if (WINDOW_OUT) store_planar8_line(o.out_frame, pb, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx, wc.px0);
        else store_planar8_line(o.out_frame, pb, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
        if (o.fast_store) __builtin_amdgcn_sched_barrier(0);
      } else if (WINDOW_OUT) {
        store_rgb8_line<STORE24_3X8, true>(o.out_frame, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx, wc.px0);
      } else {
        store_rgb8_line<STORE24_3X8, true>(o.out_frame, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
      }
    }
  }
}

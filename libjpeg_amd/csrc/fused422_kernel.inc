// fused422_kernel.inc -- the text of fused422_kernel, included by kernels.hip (see there: once in mij, once in mij::planar, and in
// mij::window and mij::window::planar, where WINDOW_OUT is true: the crop windows of a list)
// ==============================================================================================
// fused 4:2:2 kernel (Y 1x1, Cb/Cr subsampled 2x1), packed chroma
// ==============================================================================================
// fused420p_kernel without the vertical direction: the chroma planes have the luma plane's height, so a 128x128 tile
// needs (8 + 2) x 16 chroma blocks per component -- 1.25 rounds of transforms for the four waves where 4:2:0 needs
// one -- and no halo lines; the samples of a line go through the horizontal filter only.  Same gate as the packed
// 4:2:0 flavour (FAST arithmetic, chroma range_max < 2047), same store path.  Algorithmic bytes: 4 B in + 3 B out per pixel.
// WIDE: the samples still travel through LDS as int16 pairs (|sample * 16| <= 4 * range_max < 2^15 for range_max < 8190,
// the fused 4:4:4 kernel's bound, which legitimate 8-bit content cannot exceed: sum |c| q <= 8 sqrt(64 * 128^2) by
// Cauchy-Schwarz), but the filter runs on unpacked 32-bit values: frames between the packed gate (2047) and 8190 --
// saturated colours with hard edges -- stay on a fused kernel instead of falling to the generic pair.
template <int MINW, bool QDEV, bool WIDE, bool RAGGED = false>
__global__ __launch_bounds__(F420_THREADS, MINW) void fused422_kernel(Fused420Args a)
{
  static_assert(!RAGGED || QDEV, "ragged launches: per-frame tables");
  static_assert(!PLANAR_OUT || RAGGED, "planar output: the ragged flavours");
  static_assert(!WINDOW_OUT || RAGGED, "crop windows: the ragged flavours");
  __shared__ __attribute__((aligned(16))) unsigned cpair[F422_CROWS * F420_CPITCH];
  __shared__ __attribute__((aligned(16))) u32x4 stage_all[4][128];

  PlanarBases pb{};
  WindowBox wb{};
  const TileCtx t = WINDOW_OUT ? tile_enter_window<PLANAR_OUT>(a, stage_all, pb, wb) : PLANAR_OUT ? tile_enter_planar(a, stage_all, pb) : RAGGED ? tile_enter_ragged(a, stage_all) : tile_enter(a, stage_all);
  if (t.padding) return;

  // ------------------------------------------------------------------ phase A: chroma -> LDS halves (Cb low, Cr high), edge fix-up
  f422_chroma_to_lds<QDEV, !QDEV>(a, t, LdsPairHalf(cpair, t.wave >> 1));
  __syncthreads();
  f422_chroma_edges<1>(a, cpair, t.tid, t.tx);

  // ------------------------------------------------------------------ phase B: luma, upsampling, colour
  u32x4 rows[8];
  fetch_tile_blocks(rows, t, t.coef + a.off_y, a.bw_y, a.bh_y);
  WindowClip wc{};
  const BlockOut o = WINDOW_OUT ? block_out_window<PLANAR_OUT ? 1 : 3>(a, t, wb, wc) : block_out<PLANAR_OUT ? 1 : 3>(a, t);
  if (o.outside) return; // no barrier below this point
  int yv[64];
  dequant_idct_sparse<!QDEV, true>(rows, frame_deltas<QDEV>(a, t.frame, 0), yv, 0, LUMA_FOLD_R2);

  // chroma window of this block: lines pr = 8 by + l, columns pc = 4 bx + 3 + j
  const unsigned *c_base = cpair + (8 * o.by) * F420_CPITCH + 4 * o.bx;
#pragma unroll
  for (int l = 0; l < 8; l++) {
    {
      // no vertical filter (VerticalFilterCore<1>, upsampler.cpp:118-131: a copy); horizontal filter in place
      // (upsampler.cpp:291-303); src[k] = v[k + 1]
      unsigned v[6];
      load6(c_base + l * F420_CPITCH, v);
      unsigned u[8];
      int ub[8], ur[8]; // WIDE: the two components on their own, 32 bits
      if (WIDE) {
        int vb[6], vr[6];
#pragma unroll
        for (int j = 0; j < 6; j++) { vb[j] = (int)(short)(v[j] & 0xffffu); vr[j] = (int)v[j] >> 16; }
        hfilter8(vb, ub);
        hfilter8(vr, ur);
      } else {
        u[7] = tap13_pk(v[5], v[4], 1);
        u[6] = tap13_pk(v[3], v[4], 2);
        u[5] = tap13_pk(v[4], v[3], 1);
        u[4] = tap13_pk(v[2], v[3], 2);
        u[3] = tap13_pk(v[3], v[2], 1);
        u[2] = tap13_pk(v[1], v[2], 2);
        u[1] = tap13_pk(u[2], v[1], 1); // src[1] has already been overwritten by out[2]
        u[0] = tap13_pk(v[0], v[1], 2);
      }
      if (WINDOW_OUT ? l >= wc.ln0 && l < o.nln : l < o.nln) {
        int rr[8], gg[8], bb[8];
#pragma unroll
        for (int x = 0; x < 8; x++) {
          const int yk = luma13(yv[l * 8 + x]); // (level shift and rounding are inside: LUMA_FOLD_R2)
          if (WIDE) {
            rr[x] = mad24(ur[x], L_CR_R, yk); // still scaled by 2^17
            bb[x] = mad24(ub[x], L_CB_B, yk);
            gg[x] = mad24(ur[x], -L_CR_G, mad24(ub[x], -L_CB_G, yk));
          } else {
            rr[x] = mad16_hi(u[x], L_CR_R, yk); // still scaled by 2^17
            bb[x] = mad16_lo(u[x], L_CB_B, yk);
            gg[x] = dot2_16(u[x], -L_CB_G, -L_CR_G, yk);
          }
        }
        if (WINDOW_OUT && PLANAR_OUT) store_planar8_line(o.out_frame, pb, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx, wc.px0);
        else if (WINDOW_OUT) store_rgb8_line<STORE24_NT>(o.out_frame, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx, wc.px0);
        else if (PLANAR_OUT) store_planar8_line(o.out_frame, pb, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
        else store_rgb8_line<STORE24_NT>(o.out_frame, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
      }
    }
  }
}

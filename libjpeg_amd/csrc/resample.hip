// resample.hip -- resample_list_kernel (resample.hpp).
//
// A workgroup owns RESAMPLE_TILE_W x RESAMPLE_TILE_H output pixels of one picture, which it finds in the prefix table of first
// workgroups (wave-uniform loads, a binary search: what tile_enter_ragged does for the reconstruction launches).  Lane (x, g) -- x
// the tile column, g = 0..3 -- keeps the vertical sums of output lines 4g .. 4g + 3 of its column in int32 registers.  The source
// lines the tile's output lines need are walked in strips of RESAMPLE_STRIP lines: the horizontal pass of a strip goes, rounded to 8
// bits, into LDS, a pixel's components in one word; beside it the strip's vertical weights per output line of the tile (zero where a
// strip line lies outside the line's run), so that the vertical pass behind the barrier is sixteen multiply-adds per output line with
// nothing to wait for; a second barrier frees the strip.  So the LDS is 4.5 KiB whatever the reduction is, and an 8K picture to a
// thumbnail only makes more strips.  The kernel waits for memory, not for arithmetic: where an axis has at most RESAMPLE_REG_TAPS
// taps per output (reductions up to three and every enlargement) the lane's horizontal weights live in registers and its taps are
// loaded without a loop -- 3, 5 or 8 of them, by the axis's maximal count, a three-component pixel in one unaligned word, which is
// why the arena ends in 16 spare bytes.
// Stores are contiguous along x: a wave writes 64 neighbouring pixels of one line.
//
// The normalised flavours are the same text up to round8(acc): their store epilogue maps the 8-bit sample v to
// fl32(fl32((float)v * scale[c]) + bias[c]) -- two roundings, never a fused multiply-add -- and stores it as binary32, binary16 or
// bfloat16.  A mirrored picture is a matter of its x table (resample_taps.hpp): no kernel here knows the flag.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "resample.hpp"

namespace mij {

constexpr int TW = RESAMPLE_TILE_W, TH = RESAMPLE_TILE_H, SH = RESAMPLE_STRIP;
static_assert(TW == 64 && RESAMPLE_GROUP == 4 * TW && TH == 16 && SH == 16, "lane (x, g): 64 columns, 4 groups of 4 output lines and of 4 strip lines");

__device__ __forceinline__ int round8(int sum)
{
  const int v = (sum + (RESAMPLE_ONE >> 1)) >> RESAMPLE_BITS;
  return v > 255 ? 255 : v;
}

// the pixel at p: its SC components in the low bytes of a word (SC == 3: four bytes are read)
template <int SC>
__device__ __forceinline__ unsigned load_pixel(const uint8_t *__restrict__ p)
{
  if (SC == 1) return *p;
  struct __attribute__((packed)) Word { unsigned v; };
  return reinterpret_cast<const Word *>(p)->v;
}

// One output sample of the horizontal pass from K taps whose weights are in registers: all K pixels are loaded before the first is
// used (behind the run: its last tap again, weight 0) -> the rounded components in one word
template <int SC, int K>
__device__ __forceinline__ unsigned filter_row(const uint8_t *__restrict__ row, int xc, const int (&kr)[RESAMPLE_REG_TAPS])
{
  unsigned v[K];
#pragma unroll
  for (int t = 0; t < K; t++) v[t] = load_pixel<SC>(row + (unsigned)min(t, xc - 1) * SC);
  unsigned packed = 0;
#pragma unroll
  for (int c = 0; c < SC; c++) {
    int sum = 0;
#pragma unroll
    for (int t = 0; t < K; t++) sum += kr[t] * (int)((v[t] >> (8 * c)) & 255u);
    packed |= (unsigned)round8(sum) << (8 * c);
  }
  return packed;
}

// The normalised call's float value of the 8-bit sample v: a product and a sum, each rounded to nearest-even.  A contracted fma would
// round once, and the header's __fmul_rn / __fadd_rn are plain operators the compiler may contract: so the operators stand here,
// under the pragma that forbids it
__device__ __forceinline__ float normalized(int v, float scale, float bias)
{
#pragma clang fp contract(off)
  const float product = (float)v * scale;
  return product + bias;
}

// One sample of the destination, OUT a MIJPEG_SAMPLE_* of include/mijpeg.h: the 8-bit sample itself, or its float value in the
// stored type
template <int OUT>
__device__ __forceinline__ void store_sample(uint8_t *__restrict__ at, int v, float scale, float bias)
{
  if (OUT == RESAMPLE_U8) {
    *at = (uint8_t)v;
    return;
  }
  const float y = normalized(v, scale, bias);
  if (OUT == RESAMPLE_F32) *reinterpret_cast<float *>(at) = y;
  else if (OUT == RESAMPLE_F16) *reinterpret_cast<unsigned short *>(at) = __half_as_ushort(__float2half_rn(y));
  else {
    const unsigned bits = __float_as_uint(y); // (to nearest-even on the upper 16 bits, as torch's conversion has it for finite values)
    *reinterpret_cast<unsigned short *>(at) = (unsigned short)((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
  }
}

template <int SC, int OUT>
__device__ __forceinline__ void resample_tile(const ResampleArgs &a, const ResamplePicture &p, unsigned tx, unsigned ty, unsigned (*px)[TW], int16_t (*wy)[SH])
{
  constexpr int KR = RESAMPLE_REG_TAPS;
  const unsigned lx = threadIdx.x & 63u, g = threadIdx.x >> 6;
  const int ox = (int)(tx * TW + lx), oy0 = (int)(ty * TH);
  const bool xin = ox < a.out_w;
  const int32_t *__restrict__ xfirst = reinterpret_cast<const int32_t *>(a.tables + p.xtab);
  const int32_t *__restrict__ yfirst = reinterpret_cast<const int32_t *>(a.tables + p.ytab);
  const int32_t *__restrict__ xcount = xfirst + a.out_w, *__restrict__ ycount = yfirst + a.out_h;
  const int16_t *__restrict__ xw = reinterpret_cast<const int16_t *>(xfirst + 2 * (size_t)a.out_w);
  const int16_t *__restrict__ yw = reinterpret_cast<const int16_t *>(yfirst + 2 * (size_t)a.out_h);
  // this lane's column: its run, and its weights in registers where the axis has few
  int xf = 0, xc = 1;
  if (xin) { xf = xfirst[ox]; xc = xcount[ox]; }
  const int16_t *__restrict__ kx = xw + (unsigned)(xin ? ox : 0) * (unsigned)p.xcap;
  const bool few = p.xcap <= KR; // (uniform)
  int kr[KR];
#pragma unroll
  for (int t = 0; t < KR; t++) kr[t] = few && xin && t < xc ? (int)kx[t] : 0;
  // the vertical weight this lane fetches per strip: of output line tid / 16 at strip line tid % 16
  const int wl = (int)(threadIdx.x & 15u), wo = (int)(threadIdx.x >> 4), woy = oy0 + wo;
  int wf = 0, wc = 0;
  if (woy < a.out_h) { wf = yfirst[woy]; wc = ycount[woy]; }
  const int16_t *__restrict__ kyw = yw + (unsigned)(woy < a.out_h ? woy : 0) * (unsigned)p.ycap;
  int acc[4][SC];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int c = 0; c < SC; c++) acc[j][c] = 0;
  // the source lines of the tile (uniform): the runs of neighbouring output lines overlap or touch
  const int last = min(oy0 + TH, a.out_h) - 1;
  const int s_begin = yfirst[oy0], s_end = yfirst[last] + ycount[last];
  const uint8_t *__restrict__ src = a.src + p.src_off;
  const unsigned line_bytes = (unsigned)p.src_w * SC;
  for (int s0 = s_begin; s0 < s_end; s0 += SH) {
    const int lines = min(SH, s_end - s0);
    {
      const int t = s0 + wl - wf;
      wy[wo][wl] = wl < lines && t >= 0 && t < wc ? kyw[t] : (int16_t)0;
    }
    // horizontal pass of the strip: lane (x, g) filters lines g, g + 4, g + 8, g + 12 at its column
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int l = (int)g + 4 * j;
      if (l < lines && xin) {
        const uint8_t *__restrict__ row = src + ((unsigned)(s0 + l) * line_bytes + (unsigned)xf * SC);
        unsigned packed = 0;
        if (p.xcap <= 3) packed = filter_row<SC, 3>(row, xc, kr);      // (uniform: every enlargement)
        else if (p.xcap <= 5) packed = filter_row<SC, 5>(row, xc, kr); // (reductions up to two)
        else if (few) packed = filter_row<SC, KR>(row, xc, kr);        // (up to three)
        else {
          int sum[SC];
#pragma unroll
          for (int c = 0; c < SC; c++) sum[c] = 0;
          for (int t = 0; t < xc; t++) {
            const int k = kx[t];
#pragma unroll
            for (int c = 0; c < SC; c++) sum[c] += k * (int)row[t * SC + c];
          }
#pragma unroll
          for (int c = 0; c < SC; c++) packed |= (unsigned)round8(sum[c]) << (8 * c);
        }
        px[l][lx] = packed;
      }
    }
    __syncthreads();
    // vertical pass: every strip line with its weight for each of the lane's four output lines (lines behind `lines` hold
    // whatever an earlier strip left: their weights are zero)
    if (xin) {
#pragma unroll
      for (int l = 0; l < SH; l++) {
        const unsigned v = px[l][lx];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int k = wy[g * 4 + j][l];
#pragma unroll
          for (int c = 0; c < SC; c++) acc[j][c] += k * (int)((v >> (8 * c)) & 255u);
        }
      }
    }
    __syncthreads();
  }
  if (!xin) return;
  // 64-bit base of the slot, 32-bit byte offsets inside it
  constexpr unsigned ES = OUT == RESAMPLE_U8 ? 1u : OUT == RESAMPLE_F32 ? 4u : 2u;
  uint8_t *__restrict__ out = a.dst + p.dst_off;
  const unsigned cstep = a.plane_stride ? a.plane_stride : ES, pix = (a.plane_stride ? 1u : (unsigned)a.channels) * ES;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int oy = oy0 + (int)g * 4 + j;
    if (oy >= a.out_h) continue;
    const unsigned at = (unsigned)oy * a.row_stride + (unsigned)ox * pix;
    if (SC == 3) {
#pragma unroll
      for (int c = 0; c < SC; c++) store_sample<OUT>(out + (at + (unsigned)c * cstep), round8(acc[j][c]), a.scale[c], a.bias[c]);
    } else if (OUT == RESAMPLE_U8) {
      const uint8_t v = (uint8_t)round8(acc[j][0]);
      for (int c = 0; c < a.channels; c++) out[at + (unsigned)c * cstep] = v; // (a grey picture in a 3-channel batch: all three)
    } else {
      const int v = round8(acc[j][0]);
#pragma unroll
      for (int c = 0; c < 3; c++) // (... each with its channel's constants, which stay in scalar registers: no indexed access)
        if (c < a.channels) store_sample<OUT>(out + (at + (unsigned)c * cstep), v, a.scale[c], a.bias[c]);
    }
  }
}

// A workgroup's frame around resample_tile, the text both kernels below share: its picture from the prefix table of first workgroups
// (wave-uniform loads, a binary search), its tile in it, the tile by the picture's components.  A macro and no function template:
// through a function the uint8 kernel compiles to the same number of instructions in another order and with other registers, and it
// is to stay, instruction for instruction, the kernel profiles/ragged_resized.txt measured
#define RESAMPLE_WORKGROUP(OUT)                                                                                                   \
  __shared__ unsigned px[SH][TW];                             /* the strip behind the horizontal pass */                           \
  __shared__ __attribute__((aligned(16))) int16_t wy[TH][SH]; /* its vertical weights per output line of the tile */               \
  const unsigned wg = blockIdx.x;                                                                                                  \
  const uint32_t *__restrict__ first = a.first;                                                                                    \
  unsigned lo = 0, hi = (unsigned)a.served; /* first[lo] <= wg < first[hi] */                                                      \
  while (hi - lo > 1) {                                                                                                            \
    const unsigned mid = (lo + hi) >> 1;                                                                                           \
    if (first[mid] <= wg) lo = mid;                                                                                                \
    else hi = mid;                                                                                                                 \
  }                                                                                                                                \
  const ResamplePicture p = a.pictures[lo];                                                                                        \
  const unsigned local = wg - first[lo], ty = local / (unsigned)p.tiles_x, tx = local - ty * (unsigned)p.tiles_x;                  \
  if (p.comps == 3) resample_tile<3, OUT>(a, p, tx, ty, px, wy);                                                                   \
  else resample_tile<1, OUT>(a, p, tx, ty, px, wy);

__global__ __launch_bounds__(RESAMPLE_GROUP) void resample_list_kernel(ResampleArgs a) { RESAMPLE_WORKGROUP(RESAMPLE_U8) }

// The normalised call's float flavours: OUT is RESAMPLE_F32, RESAMPLE_F16 or RESAMPLE_BF16
template <int OUT>
__global__ __launch_bounds__(RESAMPLE_GROUP) void resample_list_normalized_kernel(ResampleArgs a) { RESAMPLE_WORKGROUP(OUT) }
#undef RESAMPLE_WORKGROUP

int launch_resample_list(const ResampleArgs &a, int sample, unsigned grid, hipStream_t stream)
{
  if (!grid) return 0;
  // the one place a kernel is chosen: the uint8 kernel serves the resized call and the normalised call's uint8 samples
  void (*kernel)(ResampleArgs) = nullptr;
  switch (sample) {
  case RESAMPLE_U8: kernel = resample_list_kernel; break;
  case RESAMPLE_F32: kernel = resample_list_normalized_kernel<RESAMPLE_F32>; break;
  case RESAMPLE_F16: kernel = resample_list_normalized_kernel<RESAMPLE_F16>; break;
  case RESAMPLE_BF16: kernel = resample_list_normalized_kernel<RESAMPLE_BF16>; break;
  default: return (int)hipErrorInvalidValue; // (a missing kernel is an error)
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(RESAMPLE_GROUP), 0, stream, a);
  return (int)hipGetLastError();
}

} // namespace mij

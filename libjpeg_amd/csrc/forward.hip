// forward.hip -- encoder direction of the block pipeline: pixels -> quantised coefficient planes.
//
// What the reference does per 8x8 block in front of its entropy coder (control/blockbitmaprequester.cpp:505-576,
// 708-846): forward L transformation RGB -> YCbCr at FIX_BITS 13 into samples with COLOR_BITS = 4 fractional bits
// (colortrafo/ycbcrtrafo.cpp:85-242, matrix colortransformerfactory.cpp:177-183), box downsampling of subsampled
// components (upsampling/downsampler.cpp:70-139; right edge mirrored, lines below the image missing:
// downsamplerbase.cpp:124-155), forward DCT and quantisation (dct/idct.cpp:114-222, dct/idct.hpp:90-111).
// Everything is integer arithmetic; the results are the reference's bits (oracle/jpeg_oracle.c: oj_forward, pinned
// against the coefficients the reference encoder writes).
//
// One lane, one coefficient block; no intermediate planes: the only HBM traffic is the image and the coefficients
// (128-byte stores in the decoder's plane layout).  Three kernels share the blocks of a frame:
//   fdct420_tile_kernel    4:2:0, 128 x 128 tiles wholly inside the picture: luma lanes read their pixels once and leave the
//                          box-filtered chroma samples in LDS for the lanes that transform the chroma blocks
//   fdct_interior_kernel   other layouts with subsampling factors 1 or 2: whole blocks inside the picture, pixels read as
//                          dwords in batches, only the block's own component converted
//   fdct_blocks_kernel     everything else (edges with pre-fill / mirror / missing lines, 3x and 4x factors, grey, identity
//                          transformation): per-pixel gather
// The integer work is in 32-bit wrapping arithmetic like the reference's LONG; the quantiser is its 64-bit
// multiply-and-shift.
// Each kernel has a RAGGED flavour for lists of pictures of different shapes (ForwardRaggedArgs): the workgroup looks its
// picture up and runs the same body on that picture's argument block in device memory.  The kernels' text is forward_kernels.inc.
// Each kernel also has a precision-12 flavour (template parameter P; extended sequential frames, SOF1): interleaved native-endian
// uint16_t samples, 0..4095.  What differs from the 8-bit flavour is cited where it does: the level shift 2^(P-1) in the colour
// transformation's DC offset, its clamp, the pre-fill of partial blocks and the transform's dcoffset; the width of the loads;
// the type of the chroma samples in LDS.  The transform itself is the same wrapping 32-bit one (Tables::BuildDCT,
// codestream/tables.cpp:1876-1906, takes LOSSYDCT<COLOR_BITS, LONG> up to precision 12); where 16-bit samples make the
// reference's LONG wrap, so does this.
// The ragged 8-bit kernels also have a PLANAR-INPUT flavour (namespace mij::planar_in): a picture's three samples come
// from three planes, found through a table beside the argument blocks; everything behind the samples is the same text.
// interleave_kernel makes an interleaved picture of planes for the pictures those flavours do not take.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forward.hpp"

namespace mij {

#define F9(x) ((int)((x) * 512.0 + 0.5)) // TO_FIX, dct/idct.cpp:65

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_dword_aligned __attribute__((aligned(4))); // a 16-byte load from a dword-aligned line

__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int wmul(int a, int c) { return (int)((unsigned)a * (unsigned)c); }

// Quantize, dct/idct.hpp:100-103 (no dead zone): (n * q + (n > 0) + 2^45) >> 46
__device__ __forceinline__ int quantize(int n, int q)
{
  const long long p = (long long)n * (long long)q + (long long)((unsigned)(-n) >> 31) + (1ll << 45);
  return (int)(p >> 46);
}

// One 8-point forward transform, dct/idct.cpp:126-169; outputs before any shift: o[0], o[4] plain sums, the others
// scaled by 2^9 (FIX_BITS)
__device__ __forceinline__ void fdct_1d(const int (&s)[8], int (&o)[8])
{
  int tmp0 = wadd(s[0], s[7]), tmp1 = wadd(s[1], s[6]), tmp2 = wadd(s[2], s[5]), tmp3 = wadd(s[3], s[4]);
  int tmp10 = wadd(tmp0, tmp3), tmp12 = wsub(tmp0, tmp3), tmp11 = wadd(tmp1, tmp2), tmp13 = wsub(tmp1, tmp2);
  tmp0 = wsub(s[0], s[7]); tmp1 = wsub(s[1], s[6]); tmp2 = wsub(s[2], s[5]); tmp3 = wsub(s[3], s[4]);
  o[0] = wadd(tmp10, tmp11);
  o[4] = wsub(tmp10, tmp11);
  int z1 = wmul(wadd(tmp12, tmp13), F9(0.541196100));
  o[2] = wadd(z1, wmul(tmp12, F9(0.765366865)));
  o[6] = wadd(z1, wmul(tmp13, -F9(1.847759065)));
  tmp10 = wadd(tmp0, tmp3); tmp11 = wadd(tmp1, tmp2); tmp12 = wadd(tmp0, tmp2); tmp13 = wadd(tmp1, tmp3);
  z1 = wmul(wadd(tmp12, tmp13), F9(1.175875602));
  const int tt0 = wmul(tmp0, F9(1.501321110)), tt1 = wmul(tmp1, F9(3.072711026)), tt2 = wmul(tmp2, F9(2.053119869)), tt3 = wmul(tmp3, F9(0.298631336));
  const int tt10 = wmul(tmp10, -F9(0.899976223)), tt11 = wmul(tmp11, -F9(2.562915447));
  const int tt12 = wadd(wmul(tmp12, -F9(0.390180644)), z1), tt13 = wadd(wmul(tmp13, -F9(1.961570560)), z1);
  o[1] = wadd(wadd(tt0, tt10), tt12);
  o[3] = wadd(wadd(tt1, tt11), tt13);
  o[5] = wadd(wadd(tt2, tt11), tt12);
  o[7] = wadd(wadd(tt3, tt10), tt13);
}

// component `c` of the forward L transformation of one pixel (ycbcrtrafo.cpp:176-199): FIX_TO_COLOR, clamp; m_lDCShift is
// 2^(P-1), m_lMax 2^P - 1 (12-bit samples: the sums stay below 2^30, the reference's QUAD is not needed)
template <int P>
__device__ __forceinline__ int ycc_component(int c, int r, int g, int b)
{
  const int dc = ((1 << (P - 1)) << 13) + 256;
  int v;
  if (c == 0) v = (r * 2449 + g * 4809 + b * 934 + 256) >> 9;
  else if (c == 1) v = (r * -1382 + g * -2714 + b * 4096 + dc) >> 9;
  else v = (r * 4096 + g * -3430 + b * -666 + dc) >> 9;
  return min(max(v, 0), ((1 << P) << 4) - 1);
}

// forward transform of one block of samples, quantisation, 128-byte store (idct.cpp:125-170 columns, :174-218 rows)
template <int P, class Q>
__device__ __forceinline__ void transform_and_store_from(const int (&blk)[64], Q invq, int16_t *dst)
{
  // pass over columns (idct.cpp:125-170), then rows with quantisation (:174-218)
  int t[64];
#pragma unroll
  for (int col = 0; col < 8; col++) {
    const int s[8] = {blk[col], blk[8 + col], blk[16 + col], blk[24 + col], blk[32 + col], blk[40 + col], blk[48 + col], blk[56 + col]};
    int o[8];
    fdct_1d(s, o);
    t[col] = o[0];
    t[32 + col] = o[4];
#pragma unroll
    for (int k = 1; k < 8; k++)
      if (k != 4) t[k * 8 + col] = wadd(o[k], 256) >> 9; // FIXED_TO_INTERMEDIATE
  }
  const int dcoffset = (1 << (P - 1)) << 10; // 2^(P-1) << (preshift + 3 + 3)
  unsigned packed[32];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int s[8] = {t[r * 8], t[r * 8 + 1], t[r * 8 + 2], t[r * 8 + 3], t[r * 8 + 4], t[r * 8 + 5], t[r * 8 + 6], t[r * 8 + 7]};
    int o[8];
    fdct_1d(s, o);
    o[0] = (int)((unsigned)wsub(o[0], r == 0 ? dcoffset : 0) << 9);
    o[4] = (int)((unsigned)o[4] << 9);
    int qv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) qv[k] = quantize(o[k], invq[r * 8 + k]);
#pragma unroll
    for (int k = 0; k < 4; k++) packed[r * 4 + k] = ((unsigned)qv[2 * k] & 0xffffu) | ((unsigned)qv[2 * k + 1] << 16);
  }
  u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
#pragma unroll
  for (int i = 0; i < 8; i++) d4[i] = u32x4{packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]};
}

// invq from the kernel's own arguments, or -- ragged flavours -- from the picture's argument block in the constant address space
template <int P>
__device__ __forceinline__ void transform_and_store(const int (&blk)[64], const int *__restrict__ invq, int16_t *dst)
{
  transform_and_store_from<P>(blk, invq, dst);
}
template <int P>
__device__ __forceinline__ void transform_and_store(const int (&blk)[64], const __attribute__((address_space(4))) int *invq, int16_t *dst)
{
  transform_and_store_from<P>(blk, invq, dst);
}

// One line of W pixels' worth of interleaved RGB samples as dwords: ND of them.  8-bit: dword loads; 12-bit (2-byte samples, rows
// of 48 bytes per 8 pixels): 16-byte loads
template <int P, int ND>
__device__ __forceinline__ void load_line(const uint8_t *line, unsigned (&dw)[ND])
{
  if constexpr (P == 8) {
    const unsigned *l = reinterpret_cast<const unsigned *>(line);
#pragma unroll
    for (int i = 0; i < ND; i++) dw[i] = l[i];
  } else {
    const u32x4_dword_aligned *l = reinterpret_cast<const u32x4_dword_aligned *>(line);
#pragma unroll
    for (int i = 0; i < ND / 4; i++) {
      const u32x4 v = l[i];
      dw[4 * i] = v.x; dw[4 * i + 1] = v.y; dw[4 * i + 2] = v.z; dw[4 * i + 3] = v.w;
    }
  }
}
// sample s (pixel * 3 + channel) of such a line
template <int P, int ND>
__device__ __forceinline__ int line_sample(const unsigned (&d)[ND], int s)
{
  if constexpr (P == 8) return (int)((d[s >> 2] >> (8 * (s & 3))) & 0xffu);
  else return (int)((d[s >> 1] >> (16 * (s & 1))) & 0xffffu);
}

// Planar input, 8 bit: the same line of W pixels out of three planes, W contiguous bytes of each -- ND / 3 dwords per plane (two:
// one 8-byte load; four: one 16-byte load), plane after plane in dw.  Lines start dword-aligned, no more is asked (as at 12 bit).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_dword_aligned __attribute__((aligned(4)));
template <int ND>
__device__ __forceinline__ void load_line_planar(const uint8_t *l0, const uint8_t *l1, const uint8_t *l2, unsigned (&dw)[ND])
{
  constexpr int PD = ND / 3; // dwords of a plane's line
  static_assert(PD == 2 || PD == 4, "8 or 16 pixels of a line");
  const uint8_t *const l[3] = {l0, l1, l2};
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    if constexpr (PD == 2) {
      const u32x2 v = *reinterpret_cast<const u32x2_dword_aligned *>(l[ch]);
      dw[ch * PD] = v.x; dw[ch * PD + 1] = v.y;
    } else {
      const u32x4 v = *reinterpret_cast<const u32x4_dword_aligned *>(l[ch]);
      dw[ch * PD] = v.x; dw[ch * PD + 1] = v.y; dw[ch * PD + 2] = v.z; dw[ch * PD + 3] = v.w;
    }
  }
}
// channel ch of pixel i of such a line: byte i of the plane's dwords
template <int ND>
__device__ __forceinline__ int line_sample_planar(const unsigned (&d)[ND], int ch, int i)
{
  return (int)((d[ch * (ND / 3) + (i >> 2)] >> (8 * (i & 3))) & 0xffu);
}

// Interior blocks of RGB -> YCbCr frames with subsampling factors 1 or 2: the block's SX*8 x SY*8 pixels are read as
// dwords (rows of 24 * SX bytes, 48 * SX at precision 12; the host checks that lines start dword-aligned), the samples picked
// apart in registers, only the block's own component computed, the box filter's division a shift (the sums are not negative).
template <int SX, int SY, int P>
__device__ __forceinline__ void gather_block_fast(const uint8_t *img, int64_t row_stride, int x0, int y0, int c, int (&blk)[64])
{
  constexpr int SB = P == 8 ? 1 : 2;         // bytes per sample
  constexpr int ND = 6 * SX * SB;            // dwords per line of the block
  constexpr int RB = 8 / (SX * SY * SB);     // output rows per batch: 48 dwords in flight at a time, one memory round trip each
#pragma unroll
  for (int r0 = 0; r0 < 8; r0 += RB) {
    unsigned dw[RB * SY][ND];
#pragma unroll
    for (int l = 0; l < RB * SY; l++)
      load_line<P>(img + (int64_t)(y0 + r0 * SY + l) * row_stride + (int64_t)x0 * (3 * SB), dw[l]);
    __builtin_amdgcn_sched_barrier(0); // the loads of one batch together, those of the next not before this one is used up
#pragma unroll
    for (int rr = 0; rr < RB; rr++) {
      int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int ly = 0; ly < SY; ly++)
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
          for (int k = 0; k < SX; k++) {
            const int j = 3 * (i * SX + k); // sample of the pixel's R inside the line
            const auto &d = dw[rr * SY + ly];
            acc[i] += ycc_component<P>(c, line_sample<P>(d, j), line_sample<P>(d, j + 1), line_sample<P>(d, j + 2));
          }
#pragma unroll
      for (int i = 0; i < 8; i++) blk[(r0 + rr) * 8 + i] = acc[i] >> (SX * SY == 4 ? 2 : SX * SY == 2 ? 1 : 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The same block out of three planes (8 bit): lines of 8 * SX bytes per plane, 6 * SX dwords a line and 48 in flight as above;
// R, G and B of a pixel are the same byte of the three planes' dwords.
template <int SX, int SY>
__device__ __forceinline__ void gather_block_fast_planar(const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int64_t row_stride, int x0, int y0, int c,
                                                         int (&blk)[64])
{
  constexpr int ND = 6 * SX;
  constexpr int RB = 8 / (SX * SY);
#pragma unroll
  for (int r0 = 0; r0 < 8; r0 += RB) {
    unsigned dw[RB * SY][ND];
#pragma unroll
    for (int l = 0; l < RB * SY; l++) {
      const int64_t at = (int64_t)(y0 + r0 * SY + l) * row_stride + x0;
      load_line_planar(p0 + at, p1 + at, p2 + at, dw[l]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rr = 0; rr < RB; rr++) {
      int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int ly = 0; ly < SY; ly++)
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
          for (int k = 0; k < SX; k++) {
            const int j = i * SX + k; // the pixel inside the line
            const auto &d = dw[rr * SY + ly];
            acc[i] += ycc_component<8>(c, line_sample_planar(d, 0, j), line_sample_planar(d, 1, j), line_sample_planar(d, 2, j));
          }
#pragma unroll
      for (int i = 0; i < 8; i++) blk[(r0 + rr) * 8 + i] = acc[i] >> (SX * SY == 4 ? 2 : SX * SY == 2 ? 1 : 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the box-filtered chroma samples the 4:2:0 tile kernel keeps in LDS (see there: unsigned at precision 12)
template <int P>
struct ChromaSample {
  typedef short type;
};
template <>
struct ChromaSample<12> {
  typedef unsigned short type;
};

// ---- where a workgroup finds its arguments ----------------------------------------------------------------------
template <bool RAGGED>
struct KernelArgs {
  typedef ForwardArgs type;
};
template <>
struct KernelArgs<true> {
  typedef ForwardRaggedArgs type;
};
// the argument block of a picture in device memory, read-only for the whole launch: the constant address space makes every
// read of it with a uniform address a scalar load (the geometry and the quantiser multipliers stay in SGPRs)
typedef const __attribute__((address_space(4))) ForwardArgs ConstForwardArgs;
typedef const __attribute__((address_space(4))) uint32_t const_u32;

struct RaggedItem {
  unsigned pic, comp, wg; // picture, component, workgroup inside the item -- uniform
};
__device__ __forceinline__ RaggedItem find_item(const ForwardRaggedArgs &r)
{
  const_u32 *first = (const_u32 *)r.first_wg;
  unsigned lo = 0, hi = r.items; // first[lo] <= blockIdx.x < first[hi]
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (first[mid] <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const unsigned it = ((const_u32 *)r.item)[lo];
  return RaggedItem{it >> 2, it & 3u, blockIdx.x - first[lo]};
}

// the argument block the workgroup works with: the kernel's own, or -- ragged -- its picture's in device memory
__device__ __forceinline__ const ForwardArgs &args_of(const ForwardArgs &k, const RaggedItem &) { return k; }
__device__ __forceinline__ ConstForwardArgs &args_of(const ForwardRaggedArgs &k, const RaggedItem &it) { return *((ConstForwardArgs *)k.pics + it.pic); }

// Planes 1 and 2 of the workgroup's picture where the input is planar (PL: the including namespace's PLANAR_IN), read like the
// argument block through the constant address space: the bases stay in SGPRs.  Elsewhere two nulls nobody reads, and no code.
struct InputPlanes {
  const uint8_t *p1, *p2;
};
typedef const __attribute__((address_space(4))) ForwardPlanes ConstForwardPlanes;
template <bool PL, class K>
__device__ __forceinline__ InputPlanes input_planes(const K &k, const RaggedItem &it)
{
  if constexpr (PL) {
    ConstForwardPlanes &e = *((ConstForwardPlanes *)k.planes + it.pic);
    return InputPlanes{e.p1, e.p2};
  } else
    return InputPlanes{nullptr, nullptr};
}

constexpr bool PLANAR_IN = false; // (mij and mij::ragged12: interleaved input; mij::planar_in below says otherwise)
#include "forward_kernels.inc"

// The ragged 12-bit flavours are the same text once more, in a namespace of their own.  As plain instantiations <..., true, 12> of the
// templates above they would compile just as well; they stand apart because tests/test_encode12_cpu.py pins, by mangled name, that
// no mij::fdct*_kernel<..., 12> has its RAGGED argument set (and that every 8-bit instantiation keeps its register count exactly,
// which wrapping the bodies in shared __device__ functions does not: the 8-bit tile kernel went from 197 to 207 VGPRs).  A second
// inclusion leaves every existing instantiation instruction for instruction as it was.  Only <..., true, 12> is instantiated from
// this copy; a change that may touch that test can fold them back into mij.
namespace ragged12 {
#include "forward_kernels.inc"
} // namespace ragged12

// The planar-input flavours, by the same rule a third copy: 8-bit pictures of three components whose samples lie in
// three planes.  PLANAR_IN selects where a pixel's three samples come from and nothing else; the copies above fold it away.  The
// kernels of this copy take ForwardRaggedPlanarArgs -- the ragged arguments and the table of planes 1 and 2 -- and only the six
// ragged 8-bit flavours <..., true, 8> are instantiated from it.
namespace planar_in {
constexpr bool PLANAR_IN = true;
template <bool RAGGED>
struct KernelArgs {
  typedef ForwardRaggedPlanarArgs type;
};
#include "forward_kernels.inc"
} // namespace planar_in

// ---- planes -> interleaved picture: the first pass of the two-pass route of planar input ------------------------------------------
// One lane takes eight pixels of a line: one load of 8 * SB bytes per plane (at any address), 8 * NC * SB contiguous bytes out in
// 16-byte pieces (and one of 8 where that leaves a remainder).  The last lane of a line copies its npx < 8 pixels sample by sample.
typedef u32x2 u32x2_any __attribute__((aligned(1)));
typedef u32x4 u32x4_any __attribute__((aligned(1)));
constexpr int INTERLEAVE_LINES = 4; // lines per workgroup (one wave each)
template <int NC, int SB>
__global__ __launch_bounds__(64 * INTERLEAVE_LINES) void interleave_kernel(const InterleaveArgs a)
{
  constexpr int BYTES = 8 * NC * SB;
  const int chunk = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * INTERLEAVE_LINES + threadIdx.y;
  const int x0 = chunk * 8;
  if (x0 >= a.width || y >= a.height) return;
  const int64_t src_off = (int64_t)y * a.src_row + (int64_t)x0 * SB;
  uint8_t *__restrict__ dst = a.dst + (int64_t)y * a.dst_row + (int64_t)chunk * BYTES;
  const int npx = min(8, a.width - x0);
  if (npx == 8) {
    unsigned w[BYTES / 4];
#pragma unroll
    for (int i = 0; i < BYTES / 4; i++) w[i] = 0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      unsigned s[2 * SB];
      if constexpr (SB == 1) {
        const u32x2 v = *reinterpret_cast<const u32x2_any *>(a.src[c] + src_off);
        s[0] = v.x; s[1] = v.y;
      } else {
        const u32x4 v = *reinterpret_cast<const u32x4_any *>(a.src[c] + src_off);
        s[0] = v.x; s[1] = v.y; s[2 * SB - 2] = v.z; s[2 * SB - 1] = v.w;
      }
#pragma unroll
      for (int x = 0; x < 8; x++) {
        const int e = x * NC + c; // the sample's index in the lane's piece
        if constexpr (SB == 1) w[e >> 2] |= ((s[x >> 2] >> (8 * (x & 3))) & 0xffu) << (8 * (e & 3));
        else w[e >> 1] |= ((s[x >> 1] >> (16 * (x & 1))) & 0xffffu) << (16 * (e & 1));
      }
    }
#pragma unroll
    for (int i = 0; i < BYTES / 16; i++) reinterpret_cast<u32x4_any *>(dst)[i] = u32x4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
    if constexpr (BYTES % 16 != 0) *reinterpret_cast<u32x2_any *>(dst + (BYTES - 8)) = u32x2{w[BYTES / 4 - 2], w[BYTES / 4 - 1]};
  } else {
    for (int x = 0; x < npx; x++)
#pragma unroll
      for (int c = 0; c < NC; c++)
#pragma unroll
        for (int k = 0; k < SB; k++) dst[(x * NC + c) * SB + k] = a.src[c][src_off + x * SB + k];
  }
}

int launch_interleave(const InterleaveArgs &a, hipStream_t stream)
{
  if (a.width <= 0 || a.height <= 0) return 0;
  if (a.ncomp < 1 || a.ncomp > 4 || (a.sample_bytes != 1 && a.sample_bytes != 2)) return -1;
  const dim3 grid((unsigned)((a.width + 511) / 512), (unsigned)((a.height + INTERLEAVE_LINES - 1) / INTERLEAVE_LINES)), block(64, INTERLEAVE_LINES);
  void (*kernel)(const InterleaveArgs) = nullptr;
  switch (a.ncomp * 2 + a.sample_bytes - 1) {
  case 2: kernel = interleave_kernel<1, 1>; break;
  case 3: kernel = interleave_kernel<1, 2>; break;
  case 4: kernel = interleave_kernel<2, 1>; break;
  case 5: kernel = interleave_kernel<2, 2>; break;
  case 6: kernel = interleave_kernel<3, 1>; break;
  case 7: kernel = interleave_kernel<3, 2>; break;
  case 8: kernel = interleave_kernel<4, 1>; break;
  default: kernel = interleave_kernel<4, 2>; break;
  }
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
  return (int)hipGetLastError();
}

template <int P>
static int launch_forward_of(const ForwardArgs &a, hipStream_t stream)
{
  const unsigned per_frame = a.first_block[a.ncomp];
  if (per_frame == 0 || a.frames < 1) return 0;
  if (a.tiled420) hipLaunchKernelGGL((fdct420_tile_kernel<false, P>), dim3((unsigned)(a.width >> 7) * (unsigned)(a.height >> 7), a.frames), dim3(256), 0, stream, a);
  for (int c = 0; c < a.ncomp; c++) {
    if (!a.fast[c]) continue;
    const unsigned n = (unsigned)a.fast_nbx[c] * (unsigned)a.fast_nby[c];
    if (n == 0) continue;
    const dim3 grid((n + 255) / 256, a.frames);
    const int key = a.subx[c] * 4 + a.suby[c];
    if (key == 5) hipLaunchKernelGGL((fdct_interior_kernel<1, 1, false, P>), grid, dim3(256), 0, stream, a, c);
    else if (key == 10) hipLaunchKernelGGL((fdct_interior_kernel<2, 2, false, P>), grid, dim3(256), 0, stream, a, c);
    else if (key == 9) hipLaunchKernelGGL((fdct_interior_kernel<2, 1, false, P>), grid, dim3(256), 0, stream, a, c);
    else hipLaunchKernelGGL((fdct_interior_kernel<1, 2, false, P>), grid, dim3(256), 0, stream, a, c);
  }
  hipLaunchKernelGGL((fdct_blocks_kernel<false, P>), dim3((per_frame + 255) / 256, a.frames), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

int launch_forward(const ForwardArgs &a, int precision, hipStream_t stream)
{
  return precision == 12 ? launch_forward_of<12>(a, stream) : launch_forward_of<8>(a, stream);
}

int launch_forward_ragged(const ForwardRaggedPlan &p, hipStream_t stream, int *launches)
{
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    const ForwardRaggedArgs &r = p.launch[l];
    if (r.items == 0 || p.grid[l] == 0) continue;
    const dim3 grid(p.grid[l]);
    ForwardRaggedPlanarArgs rp;
    static_cast<ForwardRaggedArgs &>(rp) = r;
    rp.planes = p.planes;
    if (l >= 2 * FORWARD_RAGGED_LAUNCHES && !p.planes) return (int)hipErrorInvalidValue; // a planar list without its plane table
    switch (l) {
    case 0: hipLaunchKernelGGL((fdct420_tile_kernel<true, 8>), grid, dim3(256), 0, stream, r); break;
    case 1: hipLaunchKernelGGL((fdct_interior_kernel<1, 1, true, 8>), grid, dim3(256), 0, stream, r, 0); break;
    case 2: hipLaunchKernelGGL((fdct_interior_kernel<2, 2, true, 8>), grid, dim3(256), 0, stream, r, 0); break;
    case 3: hipLaunchKernelGGL((fdct_interior_kernel<2, 1, true, 8>), grid, dim3(256), 0, stream, r, 0); break;
    case 4: hipLaunchKernelGGL((fdct_interior_kernel<1, 2, true, 8>), grid, dim3(256), 0, stream, r, 0); break;
    case 5: hipLaunchKernelGGL((fdct_blocks_kernel<true, 8>), grid, dim3(256), 0, stream, r); break;
    // the lists of the 12-bit pictures
    case 6: hipLaunchKernelGGL((ragged12::fdct420_tile_kernel<true, 12>), grid, dim3(256), 0, stream, r); break;
    case 7: hipLaunchKernelGGL((ragged12::fdct_interior_kernel<1, 1, true, 12>), grid, dim3(256), 0, stream, r, 0); break;
    case 8: hipLaunchKernelGGL((ragged12::fdct_interior_kernel<2, 2, true, 12>), grid, dim3(256), 0, stream, r, 0); break;
    case 9: hipLaunchKernelGGL((ragged12::fdct_interior_kernel<2, 1, true, 12>), grid, dim3(256), 0, stream, r, 0); break;
    case 10: hipLaunchKernelGGL((ragged12::fdct_interior_kernel<1, 2, true, 12>), grid, dim3(256), 0, stream, r, 0); break;
    case 11: hipLaunchKernelGGL((ragged12::fdct_blocks_kernel<true, 12>), grid, dim3(256), 0, stream, r); break;
    // the lists of the planar 8-bit pictures of three components
    case 12: hipLaunchKernelGGL((planar_in::fdct420_tile_kernel<true, 8>), grid, dim3(256), 0, stream, rp); break;
    case 13: hipLaunchKernelGGL((planar_in::fdct_interior_kernel<1, 1, true, 8>), grid, dim3(256), 0, stream, rp, 0); break;
    case 14: hipLaunchKernelGGL((planar_in::fdct_interior_kernel<2, 2, true, 8>), grid, dim3(256), 0, stream, rp, 0); break;
    case 15: hipLaunchKernelGGL((planar_in::fdct_interior_kernel<2, 1, true, 8>), grid, dim3(256), 0, stream, rp, 0); break;
    case 16: hipLaunchKernelGGL((planar_in::fdct_interior_kernel<1, 2, true, 8>), grid, dim3(256), 0, stream, rp, 0); break;
    default: hipLaunchKernelGGL((planar_in::fdct_blocks_kernel<true, 8>), grid, dim3(256), 0, stream, rp); break;
    }
    if (launches) ++*launches;
  }
  return (int)hipGetLastError();
}

} // namespace mij

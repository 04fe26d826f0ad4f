// forward.hpp -- argument block of the encoder-direction kernel (forward.hip); internal to libmijpeg.so.
#ifndef MIJ_FORWARD_HPP
#define MIJ_FORWARD_HPP
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace mij {

struct ForwardArgs {
  const uint8_t *pixels;          // interleaved samples, ncomp per pixel: 8-bit, or -- precision 12 -- native-endian uint16_t
  int64_t pixel_frame_stride;     // bytes
  int64_t pixel_row_stride;       // bytes
  int16_t *coef;                  // coefficient store, the decoder's layout
  int64_t coef_frame_stride;      // int16 units
  int32_t width, height, ncomp, ycbcr, frames;
  // interior blocks -- whole blocks inside the picture: columns < fast_nbx, rows < fast_nby -- of components with subsampling
  // factors 1 or 2 go through fdct_interior_kernel when the lines can be read as dwords (RGB -> YCbCr frames only)
  int32_t fast[4], fast_nbx[4], fast_nby[4];
  // 4:2:0 frames: the whole 128 x 128 tiles go through fdct420_tile_kernel (blocks with column < tile_nbx and row < tile_nby);
  // the interior kernels then only take the whole blocks to the right of and below the tiles
  int32_t tiled420, tile_nbx[4], tile_nby[4];
  int32_t subx[4], suby[4];       // subsampling factors per component
  int32_t bw[4], bh[4];           // plane size in blocks (MCU padded)
  int32_t nbx[4], nby[4];         // blocks that cover samples: ceil(ceil(W / subx) / 8), ...
  int64_t coef_off[4];            // plane offsets (int16 units)
  uint32_t first_block[5];        // prefix sums of bw * bh over the components: block index -> component
  int32_t invq[4][64];            // quantiser multipliers LONG(FLOAT(1 << 30) / delta + 0.5), per component, natural order
};

// precision: 8, or 12 (a.pixels are 16-bit samples 0..4095; strides stay in bytes)
int launch_forward(const ForwardArgs &a, int precision, hipStream_t stream);

// Ragged flavour: pictures of different sizes and layouts in one launch per kernel family.  Every picture has a filled
// ForwardArgs of its own in device memory (frames = 1, its own pixels, coefficient store and invq: the 1 KiB of quantiser
// multipliers per picture).  A launch is a list of work items -- a picture, for the interior kernels a picture's component --
// each with a whole number of workgroups; a workgroup finds its item by a binary search over first_wg and never spans two.
struct ForwardRaggedArgs {
  const ForwardArgs *pics;   // device
  const uint32_t *first_wg;  // device, items + 1 entries: first workgroup of every item, the launch's grid behind the last
  const uint32_t *item;      // device, per item: picture * 4 + component
  uint32_t items;
};
// Planar input: an 8-bit picture of three components whose samples lie in three planes.  Its ForwardArgs holds plane 0
// in `pixels` and the planes' line pitch in `pixel_row_stride`; planes 1 and 2 travel in a table beside `pics`, one entry of 16 bytes
// per picture of the pass (an interleaved picture's entry is two nulls).  ForwardArgs itself is what it was.
struct ForwardPlanes {
  const uint8_t *p1, *p2;
};
// what the planar-input flavours (mij::planar_in) are launched with: the ragged arguments and that table
struct ForwardRaggedPlanarArgs : ForwardRaggedArgs {
  const ForwardPlanes *planes; // device, indexed by picture like pics
};
// The launches of a ragged list of one precision, in the order launch_forward_ragged issues them: the 4:2:0 tile kernel, the interior
// kernels <1,1> <2,2> <2,1> <1,2>, the per-block kernel.  The routing per picture is launch_forward's.
// Precision is a property of the picture: the 8-bit pictures of a list have their work lists (0 .. 5), the 12-bit pictures theirs
// (6 .. 11, forward_ragged_list), and the planar 8-bit pictures of three components theirs (12 .. 17), so a workgroup never sees
// pictures of two flavours.  An interleaved list costs at most twelve launches a pass; a planar list, whose colour pictures are in
// 12 .. 17 (8 bit) or 6 .. 11 (12 bit, interleaved first) and whose grey pictures are in 0 .. 5 and 6 .. 11, at most eighteen.
constexpr int FORWARD_RAGGED_LAUNCHES = 6;
constexpr int FORWARD_RAGGED_LISTS = 3 * FORWARD_RAGGED_LAUNCHES;
inline int forward_ragged_list(int which, int precision, bool planar = false)
{
  return which + (planar ? 2 * FORWARD_RAGGED_LAUNCHES : precision == 12 ? FORWARD_RAGGED_LAUNCHES : 0);
}
struct ForwardRaggedPlan {
  ForwardRaggedArgs launch[FORWARD_RAGGED_LISTS]; // items == 0: not launched
  uint32_t grid[FORWARD_RAGGED_LISTS];
  const ForwardPlanes *planes;                    // device; what lists 12 .. 17 read beside pics (null without them)
};
// The work items picture `a` contributes: wgs[k] workgroups and item component comp[k] per entry, launch index which[k]; returns
// the number of entries (at most 5).  Host side of the routing rule: plain arithmetic, what launch_forward launches for a frame.
inline int forward_ragged_items(const ForwardArgs &a, int which[5], uint32_t wgs[5], int comp[5])
{
  int k = 0;
  const unsigned per_frame = a.first_block[a.ncomp];
  if (per_frame == 0) return 0;
  if (a.tiled420) { which[k] = 0; wgs[k] = (unsigned)(a.width >> 7) * (unsigned)(a.height >> 7); comp[k++] = 0; }
  for (int c = 0; c < a.ncomp; c++) {
    if (!a.fast[c]) continue;
    const unsigned n = (unsigned)a.fast_nbx[c] * (unsigned)a.fast_nby[c];
    if (n == 0) continue;
    const int key = a.subx[c] * 4 + a.suby[c];
    which[k] = key == 5 ? 1 : key == 10 ? 2 : key == 9 ? 3 : 4;
    wgs[k] = (n + 255) / 256;
    comp[k++] = c;
  }
  which[k] = 5; wgs[k] = (per_frame + 255) / 256; comp[k++] = 0;
  return k;
}
// returns 0 or a hipError_t; *launches: kernels launched
int launch_forward_ragged(const ForwardRaggedPlan &p, hipStream_t stream, int *launches);

// Component planes -> an interleaved picture (ncomp x sample_bytes per pixel): the first pass of the two-pass route of planar input,
// deinterleave_kernel turned round
struct InterleaveArgs {
  const uint8_t *src[4];
  int64_t src_row;             // bytes per line of every plane
  int32_t ncomp, sample_bytes; // 1..4; 1 or 2
  int32_t width, height;
  uint8_t *dst;
  int64_t dst_row;             // bytes per line of dst
};
int launch_interleave(const InterleaveArgs &a, hipStream_t stream);

} // namespace mij
#endif

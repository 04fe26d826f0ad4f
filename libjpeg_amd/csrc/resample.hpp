// resample.hpp -- the resized crop call's kernel (resample.hip; include/mijpeg.h): the crops of a list, interleaved
// 8-bit pictures back to back in an arena, through the separable integer triangle filter of resample_taps.hpp into the slots of one
// batch tensor, all pictures in one launch.
#ifndef MIJ_RESAMPLE_HPP
#define MIJ_RESAMPLE_HPP
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "resample_taps.hpp"

namespace mij {

constexpr unsigned RESAMPLE_GROUP = 256;       // lanes of a workgroup: RESAMPLE_TILE_W columns x 4 groups of lines
constexpr int RESAMPLE_STRIP = 16;             // source lines a workgroup filters horizontally at a time (its LDS: STRIP x TILE_W words)
constexpr int RESAMPLE_REG_TAPS = 8;           // horizontal taps per output up to which a lane keeps its weights in registers
constexpr size_t RESAMPLE_ARENA_SPARE = 16;    // bytes behind the last crop: a three-component pixel is read as one word
// what a launch stores per sample: the values of MIJPEG_SAMPLE_* (include/mijpeg.h; ragged_reconstruct.cpp asserts that they agree)
constexpr int RESAMPLE_U8 = 0, RESAMPLE_F32 = 1, RESAMPLE_F16 = 2, RESAMPLE_BF16 = 3;
inline unsigned resample_sample_bytes(int sample) { return sample == RESAMPLE_U8 ? 1u : sample == RESAMPLE_F32 ? 4u : 2u; }

struct ResampleArgs {
  const uint8_t *src;              // device: the arena of the crops, RESAMPLE_ARENA_SPARE readable bytes behind them
  uint8_t *dst;                    // device: slot 0 of the destination
  const uint8_t *tables;           // device: the call's tables (ResampleLayout), 16-byte aligned
  const ResamplePicture *pictures; // device: tables + ResampleLayout::pictures
  const uint32_t *first;           // device: first workgroup per served picture, and the grid behind the last
  int32_t served;                  // pictures of the launch (>= 1)
  int32_t out_w, out_h;            // every slot's size
  int32_t channels;                // 1 or 3; a one-component picture fills all of them
  uint32_t plane_stride;           // bytes from channel to channel; 0: interleaved pixels
  uint32_t row_stride;             // bytes from line to line
  float scale[3], bias[3];         // the float flavours: channel c stores fl32(fl32(v * scale[c]) + bias[c]); kernel arguments, so scalar registers
};

// One launch of `grid` workgroups on `stream`, of the kernel that stores `sample` (RESAMPLE_*: elements of 1, 4, 2, 2 bytes, every
// stride and slot offset in bytes and a multiple of the element); 0 or a hipError_t.  The host has seen to it that a crop's bytes and a slot's span
// both stay below 2^32 (the kernel's offsets inside one picture are 32 bits wide).
int launch_resample_list(const ResampleArgs &a, int sample, unsigned grid, hipStream_t stream);

} // namespace mij
#endif

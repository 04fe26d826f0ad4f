// transpose_variants.hip -- the two ways transform_list_kernel could fetch a column of a source block, as a program of
// its own: profiles/ragged_transform.txt (b).  Both kernels transpose every 8 x 8 block of int16 of a plane in place of its index, with
// the library kernel's ownership: 256 lanes, a lane one destination row, a 16-byte store.
//   lds      a 16-byte row load and the 8 x 4 dword exchange through LDS at a pitch of 40 dwords a block: what the library builds
//   strided  eight 2-byte loads 16 bytes apart: a block's eight lanes still consume exactly its one 128-byte line
// The two alternate, medians of 9 with [min .. max] from events around each launch; the outputs are compared once.
//   hipcc --offload-arch=gfx950 -O3 tools/microbench/transpose_variants.hip -o tools/microbench/transpose_variants
//   tools/microbench/transpose_variants [blocks]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define TRY(x)                                                                      \
  do {                                                                              \
    const hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                         \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);  \
      return 1;                                                                     \
    }                                                                               \
  } while (0)

struct alignas(16) Row32 { uint32_t v[4]; };
constexpr unsigned GROUP = 256, PITCH = 40;

__global__ __launch_bounds__(GROUP) void transpose_lds(const int16_t *__restrict__ src, int16_t *__restrict__ dst, unsigned blocks)
{
  __shared__ Row32 tile[GROUP / 8 * PITCH / 4];
  const unsigned slot = threadIdx.x >> 3, row = threadIdx.x & 7u, blk = blockIdx.x * (GROUP / 8) + slot;
  Row32 in = {{0u, 0u, 0u, 0u}};
  if (blk < blocks) in = *reinterpret_cast<const Row32 *>(src + (uint64_t)blk * 64 + row * 8);
  uint32_t *mine = reinterpret_cast<uint32_t *>(tile) + slot * PITCH;
#pragma unroll
  for (int k = 0; k < 4; k++) mine[k * 8 + row] = in.v[k];
  __syncthreads();
  const Row32 d0 = tile[(slot * PITCH + (row >> 1) * 8) / 4], d1 = tile[(slot * PITCH + (row >> 1) * 8) / 4 + 1];
  const unsigned sh = (row & 1u) * 16;
  Row32 out;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    out.v[k] = ((d0.v[2 * k] >> sh) & 0xffffu) | ((d0.v[2 * k + 1] >> sh) << 16);
    out.v[k + 2] = ((d1.v[2 * k] >> sh) & 0xffffu) | ((d1.v[2 * k + 1] >> sh) << 16);
  }
  if (blk < blocks) *reinterpret_cast<Row32 *>(dst + (uint64_t)blk * 64 + row * 8) = out;
}

__global__ __launch_bounds__(GROUP) void transpose_strided(const int16_t *__restrict__ src, int16_t *__restrict__ dst, unsigned blocks)
{
  const unsigned slot = threadIdx.x >> 3, row = threadIdx.x & 7u, blk = blockIdx.x * (GROUP / 8) + slot;
  if (blk >= blocks) return;
  const uint16_t *in = reinterpret_cast<const uint16_t *>(src) + (uint64_t)blk * 64 + row;
  Row32 out;
#pragma unroll
  for (int k = 0; k < 4; k++) out.v[k] = (uint32_t)in[16 * k] | ((uint32_t)in[16 * k + 8] << 16);
  *reinterpret_cast<Row32 *>(dst + (uint64_t)blk * 64 + row * 8) = out;
}

int main(int argc, char **argv)
{
  const unsigned blocks = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 1671680u; // (106.99 M coefficients: the 256-picture list's)
  if (blocks < 1 || blocks > (1u << 25)) return 2;
  const size_t bytes = (size_t)blocks * 128;
  std::vector<int16_t> host(bytes / 2), a(bytes / 2), b(bytes / 2);
  uint32_t s = 12345;
  for (int16_t &v : host) { s = s * 1664525u + 1013904223u; v = (int16_t)(s >> 16); }
  int16_t *src, *out_lds, *out_strided;
  TRY(hipMalloc(&src, bytes));
  TRY(hipMalloc(&out_lds, bytes));
  TRY(hipMalloc(&out_strided, bytes));
  TRY(hipMemcpy(src, host.data(), bytes, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  TRY(hipEventCreate(&e0));
  TRY(hipEventCreate(&e1));
  const unsigned grid = (blocks + GROUP / 8 - 1) / (GROUP / 8);
  std::vector<float> ms[2];
  for (int rep = 0; rep < 10; rep++) // (the first round warms up)
    for (int which = 0; which < 2; which++) {
      TRY(hipEventRecord(e0));
      if (which == 0) hipLaunchKernelGGL(transpose_lds, dim3(grid), dim3(GROUP), 0, 0, src, out_lds, blocks);
      else hipLaunchKernelGGL(transpose_strided, dim3(grid), dim3(GROUP), 0, 0, src, out_strided, blocks);
      TRY(hipGetLastError());
      TRY(hipEventRecord(e1));
      TRY(hipEventSynchronize(e1));
      float t = 0;
      TRY(hipEventElapsedTime(&t, e0, e1));
      if (rep) ms[which].push_back(t);
    }
  TRY(hipMemcpy(a.data(), out_lds, bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(b.data(), out_strided, bytes, hipMemcpyDeviceToHost));
  bool same = a == b;
  for (unsigned k = 0; same && k < 64; k++) same = a[(size_t)(blocks - 1) * 64 + k] == host[(size_t)(blocks - 1) * 64 + (k & 7) * 8 + (k >> 3)];
  const char *names[2] = {"lds", "strided"};
  for (int which = 0; which < 2; which++) {
    std::sort(ms[which].begin(), ms[which].end());
    const float med = ms[which][ms[which].size() / 2];
    printf("%-8s %8.2f us [%8.2f .. %8.2f]  %6.2f TB/s by the median (%.2f MB read + %.2f MB written)\n", names[which], med * 1e3, ms[which].front() * 1e3,
           ms[which].back() * 1e3, 2.0 * (double)bytes / (med * 1e-3) / 1e12, bytes / 1e6, bytes / 1e6);
  }
  printf("outputs %s\n", same ? "equal, and the transposition of the source" : "DIFFER");
  return same ? 0 : 1;
}

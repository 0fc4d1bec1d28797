// listprof.hip -- dgs_list_profile: what the tile lists of a forward look like, read on the device from what the forward
// left behind.  Per (subframe, tile): the list's length (ranges.y - ranges.x) and how far the forward walked it (the
// largest n_contrib among the tile's pixels inside the image: past that position no pixel of the tile blends anything);
// per subframe and over all of them: counts, sums, maxima, 64-entry batches (the compositing kernels' unit of work) and
// two power-of-two histograms.  The instrument behind "would splitting long lists pay on this scene".
//   * One wave64 per tile, as the compositing kernels have it: lane (lx = lane & 7, ly = lane >> 3) holds the pixel
//     (16 tx + lx, 16 ty + ly) of each 8x8 quadrant -- four loads -- and the wave's maximum is a __shfl_xor butterfly.
//   * Every figure is an integer: a block adds its tiles into LDS words (integer LDS atomics), stores ONE partial row with
//     plain stores, and a second launch adds the partial rows.  No float atomics, no global atomics: bitwise reproducible.
//   * Nothing is kept between calls, no device word is read by the host, nothing is allocated: the call can be captured.
#include <stdio.h>

#include "dgs_common.h"

namespace {

constexpr int LP_WORDS = DGS_LIST_PROFILE_WORDS;
constexpr int LP_BUCKETS = 33;               // value 0, then [2^(b-1), 2^b) for b = 1..32
constexpr int LP_WAVES = 4;                  // waves per block
constexpr int LP_TILES_PER_WAVE = 8;
constexpr int LP_TILES_PER_BLOCK = LP_WAVES * LP_TILES_PER_WAVE;   // one partial row per 32 tiles
constexpr int LP_REDUCE_SLICES = 8;          // the reduce block: 128 word slots x 8 slices of the partial rows
static_assert(LP_WORDS == 8 + 2 * LP_BUCKETS, "summary row: eight scalars and two histograms");
static_assert(LP_WORDS <= 128, "the reduce kernel gives every word one of 128 slots");

// word indices of a summary row (include/dgs_hip.h)
enum { LP_TILES = 0, LP_NONEMPTY, LP_TOTAL, LP_MAX_LENGTH, LP_BATCHES, LP_WALKED_TOTAL, LP_WALKED_MAX, LP_WALKED_BATCHES,
       LP_HIST_LENGTH, LP_HIST_WALKED = LP_HIST_LENGTH + LP_BUCKETS };

__host__ __device__ inline uint32_t lp_blocks_per_subframe(uint32_t T) {
  return (T + LP_TILES_PER_BLOCK - 1) / LP_TILES_PER_BLOCK;
}
__device__ __forceinline__ bool lp_is_max(int word) { return word == LP_MAX_LENGTH || word == LP_WALKED_MAX; }
__device__ __forceinline__ int lp_bucket(uint32_t v) { return v == 0u ? 0 : 32 - __clz((int)v); }

// grid (blocks per subframe, K).  per_tile and n_contrib may be null.
__global__ void __launch_bounds__(64 * LP_WAVES)
list_profile_tiles_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ n_contrib, int W, int H, int gx,
                          uint32_t T, uint2* __restrict__ per_tile, unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long s_sum[LP_WORDS];
  for (int i = (int)threadIdx.x; i < LP_WORDS; i += 64 * LP_WAVES) s_sum[i] = 0ull;
  __syncthreads();
  const int lane = dgs_lane(), w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lx = lane & 7, ly = lane >> 3;
  const uint32_t k = blockIdx.y;
  const size_t N = (size_t)W * (size_t)H;
  for (int i = 0; i < LP_TILES_PER_WAVE; i++) {
    const uint32_t tile = blockIdx.x * LP_TILES_PER_BLOCK + (uint32_t)(i * LP_WAVES + w);   // wave-uniform
    if (tile >= T) break;
    const size_t gw = (size_t)k * T + tile;
    const uint2 r = ranges[gw];
    const uint32_t length = r.y - r.x;
    uint32_t walked = 0u;
    if (n_contrib != nullptr) {
      const int ty = (int)(tile / (uint32_t)gx), tx = (int)(tile - (uint32_t)ty * (uint32_t)gx);
      const int px0 = tx * DGS_TILE + lx, py0 = ty * DGS_TILE + ly;   // quadrant 0 pixel; +8 for the others
      uint32_t m = 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int px = px0 + (q & 1) * 8, py = py0 + (q >> 1) * 8;
        if (px < W && py < H) m = max(m, n_contrib[(size_t)k * N + (size_t)py * W + px]);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
      walked = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
    }
    if (lane == 0) {
      if (per_tile != nullptr) per_tile[gw] = make_uint2(length, walked);
      atomicAdd(&s_sum[LP_TILES], 1ull);
      if (length != 0u) atomicAdd(&s_sum[LP_NONEMPTY], 1ull);
      atomicAdd(&s_sum[LP_TOTAL], (unsigned long long)length);
      atomicMax(&s_sum[LP_MAX_LENGTH], (unsigned long long)length);
      atomicAdd(&s_sum[LP_BATCHES], ((unsigned long long)length + 63ull) / 64ull);
      atomicAdd(&s_sum[LP_WALKED_TOTAL], (unsigned long long)walked);
      atomicMax(&s_sum[LP_WALKED_MAX], (unsigned long long)walked);
      atomicAdd(&s_sum[LP_WALKED_BATCHES], ((unsigned long long)walked + 63ull) / 64ull);
      atomicAdd(&s_sum[LP_HIST_LENGTH + lp_bucket(length)], 1ull);
      atomicAdd(&s_sum[LP_HIST_WALKED + lp_bucket(walked)], 1ull);
    }
  }
  __syncthreads();
  unsigned long long* __restrict__ dst = partial + ((size_t)k * gridDim.x + blockIdx.x) * LP_WORDS;
  for (int i = (int)threadIdx.x; i < LP_WORDS; i += 64 * LP_WAVES) dst[i] = s_sum[i];
}

// grid K + 1: block k < K combines the nb partial rows of subframe k, block K all K nb of them (not the K summary rows:
// no block waits for another).  Sums, and maxima for the two max words; integers, so the order does not matter.
__global__ void __launch_bounds__(128 * LP_REDUCE_SLICES)
list_profile_reduce_kernel(const unsigned long long* __restrict__ partial, uint32_t nb, int K,
                           unsigned long long* __restrict__ summary) {
  __shared__ unsigned long long s_acc[LP_REDUCE_SLICES][128];
  const int word = (int)(threadIdx.x & 127u), slice = (int)(threadIdx.x >> 7);
  const int row = (int)blockIdx.x;
  const size_t first = row < K ? (size_t)row * nb : 0;
  const size_t count = row < K ? (size_t)nb : (size_t)K * nb;
  const bool is_max = lp_is_max(word);
  unsigned long long acc = 0ull;
  if (word < LP_WORDS) {
    for (size_t i = (size_t)slice; i < count; i += LP_REDUCE_SLICES) {
      const unsigned long long v = partial[(first + i) * LP_WORDS + word];
      acc = is_max ? (v > acc ? v : acc) : acc + v;
    }
  }
  s_acc[slice][word] = acc;
  __syncthreads();
  if (slice == 0 && word < LP_WORDS) {
    for (int s = 1; s < LP_REDUCE_SLICES; s++) {
      const unsigned long long v = s_acc[s][word];
      acc = is_max ? (v > acc ? v : acc) : acc + v;
    }
    summary[(size_t)row * LP_WORDS + word] = acc;
  }
}

const char* lp_check_sizes(int32_t W, int32_t H, int32_t K) {
  if (W < 1 || H < 1) return "empty image";
  if (W > 65536 || H > 65536) return "W and H must be at most 65536";
  if (K < 1 || K > DGS_MAX_K) return "K must be in 1..DGS_MAX_K";
  return nullptr;
}

}  // namespace

extern "C" {

size_t dgs_list_profile_tmp_bytes(int32_t W, int32_t H, int32_t K) {
  if (lp_check_sizes(W, H, K) != nullptr) return 0;
  const uint32_t T = (uint32_t)((W + DGS_TILE - 1) / DGS_TILE) * (uint32_t)((H + DGS_TILE - 1) / DGS_TILE);
  return (size_t)K * lp_blocks_per_subframe(T) * LP_WORDS * sizeof(uint64_t);
}

int dgs_list_profile(const uint32_t* ranges, const uint32_t* n_contrib, int32_t W, int32_t H, int32_t K, uint32_t* per_tile,
                     uint64_t* summary, void* tmp, dgs_stream_t stream) {
  char msg[96];
  if (const char* bad = lp_check_sizes(W, H, K)) {
    snprintf(msg, sizeof msg, "list_profile: %s", bad);
    return dgs_fail_arg(msg);
  }
  if (ranges == nullptr || summary == nullptr || tmp == nullptr)
    return dgs_fail_arg("list_profile: null pointer (ranges, summary and tmp are required)");
  if ((reinterpret_cast<uintptr_t>(ranges) & 7u) != 0 || (reinterpret_cast<uintptr_t>(per_tile) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(summary) & 7u) != 0 || (reinterpret_cast<uintptr_t>(tmp) & 7u) != 0)
    return dgs_fail_arg("list_profile: ranges, per_tile, summary and tmp must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(n_contrib) & 3u) != 0) return dgs_fail_arg("list_profile: n_contrib must be 4-byte aligned");
  const int gx = (W + DGS_TILE - 1) / DGS_TILE, gy = (H + DGS_TILE - 1) / DGS_TILE;
  const uint32_t T = (uint32_t)gx * (uint32_t)gy;
  const uint32_t nb = lp_blocks_per_subframe(T);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* partial = reinterpret_cast<unsigned long long*>(tmp);
  hipLaunchKernelGGL(list_profile_tiles_kernel, dim3(nb, (uint32_t)K), dim3(64 * LP_WAVES), 0, s,
                     reinterpret_cast<const uint2*>(ranges), n_contrib, (int)W, (int)H, gx, T,
                     reinterpret_cast<uint2*>(per_tile), partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "list_profile (tiles)");
  hipLaunchKernelGGL(list_profile_reduce_kernel, dim3((uint32_t)K + 1u), dim3(128 * LP_REDUCE_SLICES), 0, s, partial, nb,
                     (int)K, reinterpret_cast<unsigned long long*>(summary));
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "list_profile (reduce)");
}

}  // extern "C"

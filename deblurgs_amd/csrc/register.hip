// register.hip -- coarse photometric registration of unposed test images (deblurgs_amd/registration.py; no counterpart in
// the reference, which shells out to COLMAP for this step, test.py:188-398).  Two integer kernels on the 8-bit frames
// dgs_frames_finish makes:
//   * dgs_box_reduce_u8: s x s box mean of K packed RGB frames, one dword r | g << 8 | b << 16 per output pixel, rows of
//     images padded to a multiple of four dwords (the pad is zero-filled);
//   * dgs_sad_matrix: the sum of absolute byte differences of every pair of two banks of such images (or of image i against
//     its own group of m), with v_sad_u8 on 16-byte loads.
// Integers only: every result is exact and independent of the order of the additions.  Plain loads and stores, an LDS
// exchange between the four waves of a block, no atomics, nothing kept between calls.
#include "dgs_common.h"

namespace {

// ------------------------------------------------------------------------------------------- box mean
// Thread t of image g: output dword t of the image's row of `pitch` dwords -- pixel (t / w, t % w) for t < h w, the zero
// pad after it.  A thread reads its s x s x 3 bytes (byte loads: `in` has no alignment); neighbouring threads read
// neighbouring 3 s-byte runs of a row.  The largest channel sum is 64 * 64 * 255 + 2048 < 2^21.
__global__ void __launch_bounds__(256)
box_reduce_u8_kernel(const uint8_t* __restrict__ in, int H, int W, int s, int h, int w, uint32_t pitch,
                     uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= pitch) return;
  const size_t g = blockIdx.y;
  uint32_t word = 0;
  if (t < (uint32_t)h * (uint32_t)w) {
    const int oy = (int)(t / (uint32_t)w), ox = (int)(t % (uint32_t)w);
    const uint8_t* src = in + ((g * (size_t)H + (size_t)oy * (size_t)s) * (size_t)W + (size_t)ox * (size_t)s) * 3;
    uint32_t r = 0, gr = 0, b = 0;
    for (int dy = 0; dy < s; dy++) {
      const uint8_t* row = src + (size_t)dy * (size_t)W * 3;
      for (int dx = 0; dx < s; dx++) {
        r += row[3 * dx + 0];
        gr += row[3 * dx + 1];
        b += row[3 * dx + 2];
      }
    }
    const uint32_t n = (uint32_t)(s * s), half = n / 2;
    word = ((r + half) / n) | (((gr + half) / n) << 8) | (((b + half) / n) << 16);
  }
  out[g * (size_t)pitch + t] = word;
}

// ------------------------------------------------------------------------------------------- SAD matrix
// A block: TA images of `a` against TB images of `b` over one chunk of DGS_SAD_CHUNK_DWORDS dwords.  A thread walks the
// chunk's 16-byte quads with stride 256; per quad it loads the TA quads of `a` into registers, then each of the TB quads of
// `b` ONCE and charges it to all TA accumulators of its column (four v_sad_u8 each): a dword of `b` is fetched once per
// a-tile, a dword of `a` once per b-tile.  A tile index past the end is clamped to the last image (its result is computed
// and not stored), so no load is predicated.  TA TB uint32 accumulators per thread: a thread sees at most
// DGS_SAD_CHUNK_DWORDS / 256 dwords of a pair, the block's total is below 4 * 255 * DGS_SAD_CHUNK_DWORDS < 2^32.
// GROUPED: column j of row i is image i m + j of `b` (TA = 1: the rows of a tile would share no column).
// Grid (1-D): b-tile fastest, then a-tile, then chunk.  partials [chunk][row][column] uint32.
template <int TA, int TB, bool GROUPED>
__global__ void __launch_bounds__(256)
sad_matrix_kernel(const uint4* __restrict__ a, int na, const uint4* __restrict__ b, int nb, int m, uint64_t quads,
                  uint32_t tiles_a, uint32_t tiles_b, uint32_t* __restrict__ partials) {
  static_assert(TA * TB <= 64, "one lane of the first wave stores each pair of a tile");
  __shared__ uint32_t red[4][TA * TB];
  const int cols = GROUPED ? m : nb;
  const uint32_t bt = blockIdx.x % tiles_b;
  const uint32_t at = (blockIdx.x / tiles_b) % tiles_a;
  const uint32_t chunk = blockIdx.x / (tiles_b * tiles_a);
  const int i0 = (int)at * TA, j0 = (int)bt * TB;
  constexpr uint64_t CHUNK_QUADS = DGS_SAD_CHUNK_DWORDS / 4;
  const uint64_t q0 = (uint64_t)chunk * CHUNK_QUADS;
  const uint64_t q1 = (q0 + CHUNK_QUADS < quads) ? (q0 + CHUNK_QUADS) : quads;

  const uint4* pa[TA];
  const uint4* pb[TB];
#pragma unroll
  for (int i = 0; i < TA; i++) {
    const int ia = (i0 + i < na) ? (i0 + i) : (na - 1);
    pa[i] = a + (uint64_t)ia * quads;
  }
  {
    const int ia = (i0 < na) ? i0 : (na - 1);           // (GROUPED has TA == 1: the row of this block)
#pragma unroll
    for (int j = 0; j < TB; j++) {
      const int jc = (j0 + j < cols) ? (j0 + j) : (cols - 1);
      const uint64_t jb = GROUPED ? ((uint64_t)ia * (uint64_t)m + (uint64_t)jc) : (uint64_t)jc;
      pb[j] = b + jb * quads;
    }
  }

  uint32_t acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; i++)
#pragma unroll
    for (int j = 0; j < TB; j++) acc[i][j] = 0;

  for (uint64_t q = q0 + threadIdx.x; q < q1; q += 256) {
    uint4 va[TA];
#pragma unroll
    for (int i = 0; i < TA; i++) va[i] = pa[i][q];
#pragma unroll
    for (int j = 0; j < TB; j++) {
      const uint4 vb = pb[j][q];
#pragma unroll
      for (int i = 0; i < TA; i++) {
        uint32_t s = acc[i][j];
        s = __builtin_amdgcn_sad_u8(va[i].x, vb.x, s);
        s = __builtin_amdgcn_sad_u8(va[i].y, vb.y, s);
        s = __builtin_amdgcn_sad_u8(va[i].z, vb.z, s);
        s = __builtin_amdgcn_sad_u8(va[i].w, vb.w, s);
        acc[i][j] = s;
      }
    }
  }

  // the block's TA TB totals: a butterfly over the 64 lanes of each wave, then the four waves through LDS
  const int lane = dgs_lane(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int i = 0; i < TA; i++) {
#pragma unroll
    for (int j = 0; j < TB; j++) {
      uint32_t v = acc[i][j];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
      if (lane == 0) red[wave][i * TB + j] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < TA * TB) {
    const int i = (int)threadIdx.x / TB, j = (int)threadIdx.x % TB;
    if (i0 + i < na && j0 + j < cols) {
      const uint32_t total = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
      partials[((uint64_t)chunk * (uint64_t)na + (uint64_t)(i0 + i)) * (uint64_t)cols + (uint64_t)(j0 + j)] = total;
    }
  }
}

// out[e] = the 64-bit sum of the chunks' partials of pair e (one thread per pair; consecutive threads read consecutive
// words of every chunk's row)
__global__ void __launch_bounds__(256)
sad_matrix_final_kernel(const uint32_t* __restrict__ partials, uint64_t pairs, uint32_t chunks, uint64_t* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= pairs) return;
  uint64_t total = 0;
  for (uint32_t c = 0; c < chunks; c++) total += partials[(uint64_t)c * pairs + e];
  out[e] = total;
}

constexpr int SAD_TB = 8;            // columns per block of the all-pairs kernel
constexpr int SAD_GROUP_TB = 12;     // columns per block of the grouped kernel: one 12-pose lattice

inline uint64_t sad_chunks(uint64_t L) { return (L + DGS_SAD_CHUNK_DWORDS - 1) / DGS_SAD_CHUNK_DWORDS; }

}  // namespace

extern "C" {

int dgs_box_reduce_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t s, uint32_t* out, dgs_stream_t stream) {
  if (in == nullptr || out == nullptr) return dgs_fail_arg("box_reduce_u8: null pointer");
  if (G < 1 || G > 65535) return dgs_fail_arg("box_reduce_u8: G must be in 1..65535");
  if (s < 1 || s > 64) return dgs_fail_arg("box_reduce_u8: s must be in 1..64");
  if (H < 1 || W < 1 || H / s < 1 || W / s < 1) return dgs_fail_arg("box_reduce_u8: empty output image (H / s or W / s is 0)");
  if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0) return dgs_fail_arg("box_reduce_u8: out must be 16-byte aligned");
  const int h = H / s, w = W / s;
  const uint64_t pixels = (uint64_t)h * (uint64_t)w;
  if (pixels > (1ull << 30)) return dgs_fail_arg("box_reduce_u8: more than 2^30 output pixels per image");
  const uint32_t pitch = (uint32_t)((pixels + 3) & ~3ull);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((pitch + 255) / 256, (uint32_t)G);
  hipLaunchKernelGGL(box_reduce_u8_kernel, grid, dim3(256), 0, st, in, (int)H, (int)W, (int)s, h, w, pitch, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "box_reduce_u8");
}

size_t dgs_sad_matrix_tmp_bytes(int32_t na, int32_t nb, uint64_t L) {
  if (na < 1 || nb < 1 || L < 4 || (L & 3u) != 0 || L > (1ull << 40)) return 0;
  return (size_t)(sad_chunks(L) * (uint64_t)na * (uint64_t)nb * sizeof(uint32_t));
}

int dgs_sad_matrix(const uint32_t* a, int32_t na, const uint32_t* b, int32_t nb, int32_t group, uint64_t L, uint64_t* out,
                   void* tmp, dgs_stream_t stream) {
  if (a == nullptr || b == nullptr || out == nullptr || tmp == nullptr) return dgs_fail_arg("sad_matrix: null pointer");
  if (na < 1 || nb < 1) return dgs_fail_arg("sad_matrix: na and nb must be at least 1");
  if (L < 4 || (L & 3u) != 0) return dgs_fail_arg("sad_matrix: L must be a positive multiple of 4 dwords");
  if (L > (1ull << 40)) return dgs_fail_arg("sad_matrix: L above 2^40 dwords");
  if (group < 0) return dgs_fail_arg("sad_matrix: group must be 0 (all pairs) or the images per group");
  if (group > 0 && (int64_t)na * (int64_t)group != (int64_t)nb)
    return dgs_fail_arg("sad_matrix: with group = m, nb must equal na * m");
  if ((reinterpret_cast<uintptr_t>(a) & 15u) != 0 || (reinterpret_cast<uintptr_t>(b) & 15u) != 0)
    return dgs_fail_arg("sad_matrix: a and b must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(out) & 7u) != 0 || (reinterpret_cast<uintptr_t>(tmp) & 3u) != 0)
    return dgs_fail_arg("sad_matrix: out must be 8-byte and tmp 4-byte aligned");
  const uint64_t chunks = sad_chunks(L);
  const int cols = group > 0 ? group : nb;
  const uint64_t tiles_a = group > 0 ? (uint64_t)na : ((uint64_t)na + DGS_SAD_TILE_A - 1) / DGS_SAD_TILE_A;
  const int tb = group > 0 ? SAD_GROUP_TB : SAD_TB;
  const uint64_t tiles_b = ((uint64_t)cols + (uint64_t)tb - 1) / (uint64_t)tb;
  const uint64_t blocks = tiles_a * tiles_b * chunks;                  // a function of (na, nb, group, L) only
  const uint64_t pairs = (uint64_t)na * (uint64_t)cols;
  if (blocks > 0x7fffffffull || chunks > 0xffffffffull) return dgs_fail_arg("sad_matrix: more than 2^31 - 1 blocks");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* partials = reinterpret_cast<uint32_t*>(tmp);
  const uint4* qa = reinterpret_cast<const uint4*>(a);
  const uint4* qb = reinterpret_cast<const uint4*>(b);
  if (group > 0)
    hipLaunchKernelGGL((sad_matrix_kernel<1, SAD_GROUP_TB, true>), dim3((uint32_t)blocks), dim3(256), 0, st, qa, (int)na, qb,
                       (int)nb, (int)group, L / 4, (uint32_t)tiles_a, (uint32_t)tiles_b, partials);
  else
    hipLaunchKernelGGL((sad_matrix_kernel<DGS_SAD_TILE_A, SAD_TB, false>), dim3((uint32_t)blocks), dim3(256), 0, st, qa,
                       (int)na, qb, (int)nb, 0, L / 4, (uint32_t)tiles_a, (uint32_t)tiles_b, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "sad_matrix");
  hipLaunchKernelGGL(sad_matrix_final_kernel, dim3((uint32_t)((pairs + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)partials, pairs, (uint32_t)chunks, out);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "sad_matrix (final)");
}

}  // extern "C"

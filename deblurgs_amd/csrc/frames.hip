// frames.hip -- what the reference does on the host after a camera path is rendered (render_spiral.py:32-33,
// render_trainview.py:41-48, utils/export_utils.py:44-65), on the device:
//   * dgs_frames_finish: tone mapping, clip to [0, 1], * 255, the truncating cast to 8 bits, the NCHW -> NHWC permute and
//     the centre crop of K rendered frames in one pass: 12 bytes read and 3 written per pixel, packed frames leave;
//   * dgs_depth_range + dgs_depth_colorize: depth_colorize with clip_percentage = 1 -- the range of a whole path's depth
//     images stays in device memory (the reference reads it back with three .item() calls), the colour map is a 256-entry
//     RGBA table indexed as matplotlib indexes it.
// Built with -ffp-contract=off (deblurgs_amd/build.py): every statement rounds once, as the torch / numpy expression it
// restates does.  Plain loads, stores and an LDS tree: no atomics, nothing kept between calls.
#include <math.h>

#include "dgs_common.h"

namespace {

// ------------------------------------------------------------------------------------------- 8-bit frames
// One value: tone_map as view_loss_image (metrics.hip) evaluates it -- same expression, same powf -- then numpy's
// (clip(y, 0, 1) * 255.0).astype(uint8): the cast truncates.  fmaxf drops a NaN operand, so a NaN pow result gives 0; a NaN
// INPUT gives 0 in both modes by decision (numpy's cast of a NaN is undefined; fmaxf(u, eps) alone would make it eps).
template <int GAMMA>
__device__ __forceinline__ uint32_t frame_level(float xv, float eps, float bound, float inv_span, float ex) {
  float y = xv;
  if (GAMMA) {
    const float u = (xv - bound) / inv_span;
    const float uc = fmaxf(u, eps);
    y = powf(uc, ex);
  }
  const float c = (xv != xv) ? 0.0f : fminf(fmaxf(y, 0.0f), 1.0f);
  return (uint32_t)(c * 255.0f);
}

// Thread t of a row: output pixels [4 t, 4 t + 4) of the window -- three plane reads (one 16-byte load each where the
// address allows, scalar loads otherwise), twelve bytes out (three dword stores where the address allows, byte stores
// otherwise).  Both alignments are the same for every full thread of a block (a block is one row of one frame: the source
// moves by 16 bytes per thread, the destination by 12), so neither test diverges; only a row's last thread can hold fewer
// than four pixels.  Grid: x over the row's quads, y = row of the window, z = frame.
template <int GAMMA>
__global__ void __launch_bounds__(256)
frames_finish_kernel(const float* __restrict__ color, int H, int W, float eps, float bound, int y0, int x0, int h, int w,
                     uint8_t* __restrict__ out) {
  const int quad = (int)(blockIdx.x * 256 + threadIdx.x);
  if (quad >= (w + 3) / 4) return;
  const int p0 = 4 * quad;
  const int nv = (w - p0 < 4) ? (w - p0) : 4;
  const int row = (int)blockIdx.y, k = (int)blockIdx.z;
  const size_t plane = (size_t)H * (size_t)W;
  const float* src = color + (size_t)k * 3 * plane + (size_t)(y0 + row) * (size_t)W + (size_t)(x0 + p0);
  uint8_t* dst = out + (((size_t)k * (size_t)h + (size_t)row) * (size_t)w + (size_t)p0) * 3;
  const float inv_span = 1.0f - 2.0f * bound;
  const float ex = (float)(1.0 / 2.2);
  uint32_t lv[3][4];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float* s = src + (size_t)c * plane;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (nv == 4 && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(s);
      v[0] = q.x;
      v[1] = q.y;
      v[2] = q.z;
      v[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (i < nv) v[i] = s[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) lv[c][i] = frame_level<GAMMA>(v[i], eps, bound, inv_span, ex);
  }
  if (nv == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
    // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3, little endian
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    d[0] = lv[0][0] | (lv[1][0] << 8) | (lv[2][0] << 16) | (lv[0][1] << 24);
    d[1] = lv[1][1] | (lv[2][1] << 8) | (lv[0][2] << 16) | (lv[1][2] << 24);
    d[2] = lv[2][2] | (lv[0][3] << 8) | (lv[1][3] << 16) | (lv[2][3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (i < nv) {
        dst[3 * i + 0] = (uint8_t)lv[0][i];
        dst[3 * i + 1] = (uint8_t)lv[1][i];
        dst[3 * i + 2] = (uint8_t)lv[2][i];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- depth range
// min / max over the 256 threads of a block (fminf / fmaxf are exact and commutative: any order gives the same two
// numbers; the tree's order is fixed all the same); valid in thread 0
__device__ __forceinline__ void block_min_max_256(float& lo, float& hi, float* red_lo, float* red_hi) {
  red_lo[threadIdx.x] = lo;
  red_hi[threadIdx.x] = hi;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_lo[threadIdx.x] = fminf(red_lo[threadIdx.x], red_lo[threadIdx.x + s]);
      red_hi[threadIdx.x] = fmaxf(red_hi[threadIdx.x], red_hi[threadIdx.x + s]);
    }
    __syncthreads();
  }
  lo = red_lo[0];
  hi = red_hi[0];
}

constexpr int RANGE_MAX_BLOCKS = 1024;
__host__ __device__ inline uint32_t range_blocks(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (uint32_t)(want < (uint64_t)RANGE_MAX_BLOCKS ? want : (uint64_t)RANGE_MAX_BLOCKS);
}

// fminf / fmaxf drop a NaN operand: NaNs do not count (torch.min / torch.max would return NaN); nothing but NaNs leaves
// (+inf, -inf).  First launch: in [n] -> partials [gridDim.x][2]; second launch (one block): partials -> lo_hi [2].
__global__ void __launch_bounds__(256)
depth_range_kernel(const float* __restrict__ in, size_t n, float* __restrict__ partials) {
  __shared__ float red_lo[256], red_hi[256];
  const float inf = __int_as_float(0x7f800000);
  float lo = inf, hi = -inf;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const float v = in[e];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_min_max_256(lo, hi, red_lo, red_hi);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = lo;
    partials[2 * blockIdx.x + 1] = hi;
  }
}
__global__ void __launch_bounds__(256)
depth_range_final_kernel(const float* __restrict__ partials, int nb, float* __restrict__ lo_hi) {
  __shared__ float red_lo[256], red_hi[256];
  const float inf = __int_as_float(0x7f800000);
  float lo = inf, hi = -inf;
  for (int i = threadIdx.x; i < nb; i += 256) {
    lo = fminf(lo, partials[2 * i]);
    hi = fmaxf(hi, partials[2 * i + 1]);
  }
  block_min_max_256(lo, hi, red_lo, red_hi);
  if (threadIdx.x == 0) {
    lo_hi[0] = lo;
    lo_hi[1] = hi;
  }
}

// ------------------------------------------------------------------------------------------- depth colours
// depth_colorize (utils/export_utils.py:44-65) with clip_percentage = 1: lo = max(z_near, min), hi = min(z_far, max) from
// the two device words, d = clip((x - lo) / (hi - lo), 0, 1), then the colour map's own indexing of a float in [0, 1]
// (matplotlib Colormap.__call__: int(d * 256), 256 -> 255) into the 256 x RGBA table, which already holds
// (colour * 255).astype(uint8).  hi == lo, or a NaN anywhere in the chain, gives the map's "bad" colour (0, 0, 0, 0).
__global__ void __launch_bounds__(256)
depth_colorize_kernel(const float* __restrict__ depth, size_t n, const float* __restrict__ lo_hi, float z_near, float z_far,
                      const uint32_t* __restrict__ lut, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const float lo = fmaxf(z_near, lo_hi[0]), hi = fminf(z_far, lo_hi[1]);
  const float span = hi - lo;
  const bool flat = !(hi != lo) || (span != span);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const float d0 = (depth[e] - lo) / span;
    const float d = fminf(fmaxf(d0, 0.0f), 1.0f);
    int idx = (int)(d * 256.0f);
    idx = idx > 255 ? 255 : idx;
    out[e] = (flat || d0 != d0) ? 0u : s_lut[idx];
  }
}

}  // namespace

extern "C" {

int dgs_frames_finish(const float* color, int32_t K, int32_t H, int32_t W, int32_t tone_mapping, float eps, float bound,
                      int32_t y0, int32_t x0, int32_t h, int32_t w, uint8_t* out, dgs_stream_t stream) {
  if (color == nullptr || out == nullptr) return dgs_fail_arg("frames_finish: null pointer");
  if (K < 1 || K > 65535) return dgs_fail_arg("frames_finish: K must be in 1..65535");
  if (H < 1 || W < 1 || W > (1 << 30)) return dgs_fail_arg("frames_finish: empty image (or W above 2^30)");
  if (h < 1 || w < 1) return dgs_fail_arg("frames_finish: empty window");
  if (y0 < 0 || x0 < 0 || (int64_t)y0 + (int64_t)h > (int64_t)H || (int64_t)x0 + (int64_t)w > (int64_t)W)
    return dgs_fail_arg("frames_finish: the window leaves the image");
  if (h > 65535) return dgs_fail_arg("frames_finish: window taller than 65535 rows");
  if (tone_mapping != DGS_TONE_IDENTITY && tone_mapping != DGS_TONE_GAMMA)
    return dgs_fail_arg("frames_finish: tone_mapping must be DGS_TONE_IDENTITY or DGS_TONE_GAMMA");
  if (tone_mapping == DGS_TONE_GAMMA && !(bound < 0.5f)) return dgs_fail_arg("frames_finish: bound must be below 0.5");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int quads = (w + 3) / 4;
  const dim3 grid((uint32_t)((quads + 255) / 256), (uint32_t)h, (uint32_t)K);
  if (tone_mapping == DGS_TONE_GAMMA)
    hipLaunchKernelGGL(frames_finish_kernel<1>, grid, dim3(256), 0, s, color, (int)H, (int)W, eps, bound, (int)y0, (int)x0,
                       (int)h, (int)w, out);
  else
    hipLaunchKernelGGL(frames_finish_kernel<0>, grid, dim3(256), 0, s, color, (int)H, (int)W, eps, bound, (int)y0, (int)x0,
                       (int)h, (int)w, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "frames_finish");
}

size_t dgs_depth_range_tmp_bytes(uint64_t n) {
  return (size_t)range_blocks(n) * 2 * sizeof(float);
}

int dgs_depth_range(const float* depth, uint64_t n, float* lo_hi, void* tmp, dgs_stream_t stream) {
  if (depth == nullptr || lo_hi == nullptr || tmp == nullptr) return dgs_fail_arg("depth_range: null pointer");
  if (n < 1) return dgs_fail_arg("depth_range: n must be at least 1");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t nb = range_blocks(n);      // a function of n only
  float* partials = reinterpret_cast<float*>(tmp);
  hipLaunchKernelGGL(depth_range_kernel, dim3(nb), dim3(256), 0, s, depth, (size_t)n, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "depth_range");
  hipLaunchKernelGGL(depth_range_final_kernel, dim3(1), dim3(256), 0, s, (const float*)partials, (int)nb, lo_hi);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "depth_range (final)");
}

int dgs_depth_colorize(const float* depth, uint64_t n, const float* lo_hi, float z_near, float z_far, const uint8_t* lut,
                       uint8_t* out, dgs_stream_t stream) {
  if (depth == nullptr || lo_hi == nullptr || lut == nullptr || out == nullptr)
    return dgs_fail_arg("depth_colorize: null pointer");
  if (n < 1) return dgs_fail_arg("depth_colorize: n must be at least 1");
  if ((reinterpret_cast<uintptr_t>(lut) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out) & 3u) != 0)
    return dgs_fail_arg("depth_colorize: lut and out must be 4-byte aligned (one RGBA word per entry)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t want = (n + 255) / 256;
  const dim3 grid((uint32_t)(want < 8192 ? want : 8192));
  hipLaunchKernelGGL(depth_colorize_kernel, grid, dim3(256), 0, s, depth, (size_t)n, lo_hi, z_near, z_far,
                     reinterpret_cast<const uint32_t*>(lut), reinterpret_cast<uint32_t*>(out));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "depth_colorize");
}

}  // extern "C"

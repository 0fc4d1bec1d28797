// scene.hip -- the two device parts of scene loading (deblurgs_amd/scene.py): the image resize of the reference's PILtoTorch
// (utils/general_utils.py:23-29, i.e. Pillow's antialiased BICUBIC `Image.resize` on 8-bit images) and the per-camera depth
// keys of get_bds (scene/dataset_readers.py:164-209).
//
//   * dgs_resample_ksize / dgs_resample_coeffs (host only, no HIP call): Pillow's precompute_coeffs + normalize_coeffs_8bpc
//     for the bicubic filter (a = -0.5, support 2), restated in double one rounding per statement (-ffp-contract=off): per
//     output index the first input index, the number of taps and the taps as integers scaled by 2^22.
//   * dgs_resize_u8: Pillow's ImagingResample for 8-bit images in ONE launch.  Horizontal pass first, its result ROUNDED TO
//     BYTES, then the vertical pass on those bytes; each sample starts at 2^21, adds pixel * tap in 32-bit integers, is
//     shifted right by 22 (arithmetic) and clamped to 0..255.  A pass whose size does not change is skipped.
//       tile      a block of 256 threads owns TH x TW output pixels of one image, all C channels: 16 x 64 by default.  It
//                 resamples the input rows [r0, r1) its output rows read horizontally, for its TW columns only, into LDS as
//                 bytes (row-major, pixel-interleaved; a thread makes the C channels of one pixel in C accumulators from one
//                 load of every tap: 3.16 against 6.06 ms for 30 4K images with one thread per channel), runs the vertical pass
//                 out of LDS into a second LDS array of TH TW C result bytes, and stores that array twice: interleaved as u8
//                 [h,w,C] and planar as float [C,h,w] (byte / 255.0f, one correctly rounded division), both with
//                 neighbouring threads on neighbouring addresses.  The [G,H,w,C] intermediate never touches HBM.
//       LDS       RESIZE_ROWS_BYTES = 32 KiB for the rows + 3 KiB for the result tile (35 KiB a block: four blocks a CU).
//                 The rows of a tile span at most (TH - 1) s + 2 support + 2 input rows (s = H / h, support = 2 max(s, 1)):
//                 where 16 rows of 64 pixels do not fit -- 19 s + 2 > 170 rows at C = 3: vertical ratios above ~8.8 -- the host
//                 halves TH down to 1, then TW (ratio 64, C = 3: 258 rows of 32 pixels, 24.2 KiB), so every ratio in
//                 [1/64, 64] is one launch and no temporary is needed.  Neighbouring tiles resample overlapping input rows
//                 (1.25 x the rows at 2160 -> 900, 2.5 x at ratio 33 where a tile is two rows): the price of no round trip
//                 through HBM.  The choice is a function of the arguments only.
//       bounds    the tables come from the caller: the kernel clamps every index it derives from them (taps to ksize, input
//                 columns to W, input rows to H and to the LDS rows it holds), so a wrong table gives wrong bytes, never an
//                 access outside the buffers.
//   * dgs_depth_bound_keys: for every (camera, point) the expressions of get_bds in double.  NOTE the reference multiplies
//     the ROW vector of camera coordinates by inv(K), not K (dataset_readers.py:195): with cam = R p + t,
//         u = cam.x / fx,  v = cam.y / fy,  d = cam.z - cam.x (w/2) / fx - cam.y (h/2) / fy,  px = u / d,  py = v / d
//     and a point counts when cam.z > 0.01, 0 <= px < w, 0 <= py < h -- with the FIRST camera's w, h, fx, fy for every camera.
//     This is a parity trap, not a projection; it is restated, not repaired.  Key = (float)cam.z of a counted pair, a quiet
//     NaN otherwise (NaNs sort last in dgs_order_stats: the ranks below the count index exactly the counted depths); the
//     counts are an integer sum (one atomicAdd of a block's popcount per block; the launcher's first kernel zeroes them).
//   * dgs_resize_rgba_u8: Pillow's `Image.resize` of an RGBA image, which is NOT four independent channels: the image is
//     converted to premultiplied alpha (RGBa: MULDIV255(c, a), t = c a + 128, ((t >> 8) + t) >> 8), the four bytes are
//     resampled, and the result is converted back (colour copied where alpha is 0 or 255, else min(255, 255 c / a)).  The
//     same kernel template with C = 4 and the alpha pixel policy: premultiplied where a pixel is LOADED (the horizontal
//     pass, or the row copy when only the vertical pass runs), un-premultiplied where the result tile is STORED.  When no
//     pass runs it is Pillow's plain copy: no round trip, the colour under alpha 0 survives.  LDS: 32 KiB of rows + 4 KiB of
//     result tile (36 KiB a block: still four blocks a CU of 160 KiB); 128 rows of 64 pixels fit, so the tile shrinks from
//     vertical ratios above ~6.6 on.
//   * dgs_rgba_over_u8: the Blender reader's composite over black or white (scene/dataset_readers.py:335-341), per colour
//     byte trunc(((c / 255.0) (a / 255.0) + bg (1.0 - a / 255.0)) 255.0) in IEEE double, one rounding per operation, in the
//     reference's order (the `+ 0.0 (..)` of black included).  x / 255.0 comes from a 256-entry LDS table every block
//     fills with one correctly rounded division per thread; the rest is three multiplications, a subtraction and an
//     addition per byte.  A thread makes 4 consecutive pixels of the flat [G H W] pixel array (one 16-byte load where the
//     input is 16-byte aligned, byte loads where it is not); a block stages its 1024 x 3 result bytes in LDS and stores
//     them twice with neighbouring lanes on neighbouring addresses: as dwords (bytes where the output is misaligned) of
//     the interleaved u8 [G,H,W,3], and as float planes [3,H,W] per image (byte / 255.0f).
// No allocation, no host synchronisation, nothing kept between calls, no float atomics: capturable.
#include "dgs_common.h"

#include <math.h>
#include <stdio.h>

namespace {

constexpr int RESIZE_PRECISION_BITS = 32 - 8 - 2;     // Pillow's PRECISION_BITS for 8-bit channels
constexpr int RESIZE_ROWS_BYTES = 32768;              // LDS for the horizontally resampled rows of a tile
constexpr int RESIZE_TH = 16, RESIZE_TW = 64;         // the default (largest) output tile
constexpr int RESIZE_MAX_C = 4;
constexpr int RESIZE_MAX_DIM = 65536;                 // per axis, input and output
constexpr double RESIZE_MAX_RATIO = 64.0;

// ------------------------------------------------------------------------------------------- coefficient tables (host)
inline double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

inline bool ratio_ok(int in_size, int out_size) {
  if (in_size < 1 || out_size < 1 || in_size > RESIZE_MAX_DIM || out_size > RESIZE_MAX_DIM) return false;
  return (double)in_size <= RESIZE_MAX_RATIO * (double)out_size && (double)out_size <= RESIZE_MAX_RATIO * (double)in_size;
}

struct AxisScale {
  double scale, filterscale, support;
  int ksize;
};
inline AxisScale axis_scale(int in_size, int out_size) {
  AxisScale a;
  a.scale = a.filterscale = (double)in_size / (double)out_size;
  if (a.filterscale < 1.0) a.filterscale = 1.0;
  a.support = 2.0 * a.filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  return a;
}

// the most input rows [r0, r1) the vertical pass of `th` consecutive output rows can read
inline int rows_span(int H, int h, int th) {
  if (H == h) return th;
  const AxisScale a = axis_scale(H, h);
  const double span = ceil((double)(th - 1) * a.scale + 2.0 * a.support) + 2.0;
  return span < (double)H ? (int)span : H;
}

// ------------------------------------------------------------------------------------------- resize
struct ResizeArgs {
  const uint8_t* in;
  int H, W, C, h, w;
  const int32_t* kk_h;       // [w, ksize_h], nullptr when W == w
  const int32_t* bounds_h;   // [w, 2]
  const int32_t* kk_v;       // [h, ksize_v], nullptr when H == h
  const int32_t* bounds_v;   // [h, 2]
  int ksize_h, ksize_v;
  int th, tw, cap_rows;      // the output tile and the LDS rows of tw pixels it may fill
  uint32_t tiles_x, tiles_y;
  uint8_t* out_u8;           // [G,h,w,C] or nullptr
  float* out_f32;            // [G] x image_stride floats, [C,h,w] each, or nullptr
  uint64_t image_stride;
};

__device__ __forceinline__ int clip8(int v) {
  v >>= RESIZE_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow's RGBA -> RGBa (premultiply) and RGBa -> RGBA conversions of one colour byte (Convert.c)
__device__ __forceinline__ int premultiply8(int c, int alpha) {
  const int t = c * alpha + 128;
  return ((t >> 8) + t) >> 8;
}
__device__ __forceinline__ int unpremultiply8(int c, int alpha) {
  if (alpha == 0 || alpha == 255) return c;
  const int v = 255 * c / alpha;
  return v > 255 ? 255 : v;
}

// ALPHA (C = 4 only): the fourth byte is an alpha the three others are premultiplied by while they are resampled
template <int C, bool ALPHA>
__global__ void __launch_bounds__(256)
resize_u8_kernel(const ResizeArgs a) {
  static_assert(C >= 1 && C <= RESIZE_MAX_C && (!ALPHA || C == 4), "channels");
  __shared__ uint8_t rows[RESIZE_ROWS_BYTES];
  __shared__ uint8_t tile[RESIZE_TH * RESIZE_TW * C];
  const uint32_t tx = blockIdx.x % a.tiles_x;
  const uint32_t ty = (blockIdx.x / a.tiles_x) % a.tiles_y;
  const size_t g = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int x0 = (int)tx * a.tw, y0 = (int)ty * a.th;
  const int nx = min(a.tw, a.w - x0), ny = min(a.th, a.h - y0);
  const bool do_h = a.kk_h != nullptr, do_v = a.kk_v != nullptr;
  const bool premul = ALPHA && (do_h || do_v);                 // (neither pass: Pillow's plain copy)

  // the input rows this tile's vertical pass reads (the first taps of the bounds table do not decrease with the row)
  int r0 = y0, r1 = y0 + ny;
  if (do_v) {
    r0 = a.bounds_v[2 * y0];
    r1 = a.bounds_v[2 * (y0 + ny - 1)] + a.bounds_v[2 * (y0 + ny - 1) + 1];
  }
  r0 = max(0, min(r0, a.H));
  r1 = max(r0, min(r1, min(a.H, r0 + a.cap_rows)));
  const int nrows = r1 - r0;
  const int pitch = nx * C;                                   // bytes of an LDS row
  const uint8_t* img = a.in + g * (size_t)a.H * (size_t)a.W * (size_t)C;

  // horizontal pass: item i = (row, column); a thread makes the C channels of its pixel from one load of every tap
  for (int i = (int)threadIdx.x; i < nrows * nx; i += 256) {
    const int r = i / nx, x = i - r * nx;
    const uint8_t* src = img + (size_t)(r0 + r) * (size_t)a.W * (size_t)C;
    uint8_t* dst = rows + r * pitch + x * C;
    if (do_h) {
      const int ox = x0 + x;
      const int xmin = max(0, a.bounds_h[2 * ox]);
      const int xmax = min(min(a.bounds_h[2 * ox + 1], a.ksize_h), a.W - xmin);
      const int32_t* __restrict__ k = a.kk_h + (size_t)ox * (size_t)a.ksize_h;
      const uint8_t* p = src + (size_t)xmin * (size_t)C;
      int ss[C];
#pragma unroll
      for (int c = 0; c < C; c++) ss[c] = 1 << (RESIZE_PRECISION_BITS - 1);
      for (int t = 0; t < xmax; t++) {
        const int kt = k[t];
        if constexpr (ALPHA) {
          const int alpha = (int)p[t * C + C - 1];
#pragma unroll
          for (int c = 0; c < C - 1; c++) ss[c] += premultiply8((int)p[t * C + c], alpha) * kt;
          ss[C - 1] += alpha * kt;
        } else {
#pragma unroll
          for (int c = 0; c < C; c++) ss[c] += (int)p[t * C + c] * kt;
        }
      }
#pragma unroll
      for (int c = 0; c < C; c++) dst[c] = (uint8_t)clip8(ss[c]);
    } else {
      if (premul) {
        const uint8_t* p = src + (size_t)(x0 + x) * (size_t)C;
        const int alpha = (int)p[C - 1];
#pragma unroll
        for (int c = 0; c < C - 1; c++) dst[c] = (uint8_t)premultiply8((int)p[c], alpha);
        dst[C - 1] = (uint8_t)alpha;
      } else {
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] = src[(size_t)(x0 + x) * (size_t)C + c];
      }
    }
  }
  __syncthreads();

  // vertical pass out of LDS: item i = (output row, column, channel) of the tile
  const int tile_pitch = nx * C;
  for (int i = (int)threadIdx.x; i < ny * tile_pitch; i += 256) {
    const int y = i / tile_pitch, xc = i - y * tile_pitch;
    int v;
    if (do_v) {
      const int oy = y0 + y;
      const int ymin = a.bounds_v[2 * oy];
      const int ymax = min(a.bounds_v[2 * oy + 1], a.ksize_v);
      const int32_t* k = a.kk_v + (size_t)oy * (size_t)a.ksize_v;
      int ss = 1 << (RESIZE_PRECISION_BITS - 1);
      for (int t = 0; t < ymax; t++) {
        const int r = ymin + t - r0;
        if (r >= 0 && r < nrows) ss += (int)rows[r * pitch + xc] * k[t];
      }
      v = clip8(ss);
    } else {
      v = y < nrows ? rows[y * pitch + xc] : 0;
    }
    tile[i] = (uint8_t)v;
  }
  __syncthreads();

  if (a.out_u8 != nullptr) {      // interleaved: a tile row is nx C consecutive bytes of the image row
    uint8_t* dst = a.out_u8 + ((g * (size_t)a.h + (size_t)y0) * (size_t)a.w + (size_t)x0) * (size_t)C;
    for (int i = (int)threadIdx.x; i < ny * tile_pitch; i += 256) {
      const int y = i / tile_pitch, xc = i - y * tile_pitch;
      uint8_t v = tile[i];
      if constexpr (ALPHA) {      // (C = 4: the pixel's alpha is byte 3 of its dword)
        if (premul && (i & 3) != 3) v = (uint8_t)unpremultiply8((int)v, (int)tile[i | 3]);
      }
      dst[(size_t)y * (size_t)a.w * (size_t)C + xc] = v;
    }
  }
  if (a.out_f32 != nullptr) {     // planar: item i = (channel, row, column), column fastest
    float* dst = a.out_f32 + g * (size_t)a.image_stride;
    const int plane = ny * nx;
    for (int i = (int)threadIdx.x; i < C * plane; i += 256) {
      const int c = i / plane, rem = i - c * plane;
      const int y = rem / nx, x = rem - y * nx;
      uint8_t v = tile[y * tile_pitch + x * C + c];
      if constexpr (ALPHA) {
        if (premul && c != C - 1) v = (uint8_t)unpremultiply8((int)v, (int)tile[y * tile_pitch + x * C + C - 1]);
      }
      dst[((size_t)c * (size_t)a.h + (size_t)(y0 + y)) * (size_t)a.w + (size_t)(x0 + x)] = (float)v / 255.0f;
    }
  }
}

int resize_fail(const char* who, const char* what) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return dgs_fail_arg(msg);
}

// The argument checks, the tile choice and the launch shared by dgs_resize_u8 (C = 1 or 3; 0 stands for a refused channel
// count) and dgs_resize_rgba_u8 (C = 4 with the alpha policy).
int resize_call(const char* who, bool alpha, const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t C, int32_t h,
                int32_t w, const int32_t* kk_h, const int32_t* bounds_h, const int32_t* kk_v, const int32_t* bounds_v,
                uint8_t* out_u8, float* out_f32, uint64_t f32_image_stride, dgs_stream_t stream) {
  if (in == nullptr) return resize_fail(who, "null input pointer");
  if (out_u8 == nullptr && out_f32 == nullptr) return resize_fail(who, "both outputs are null");
  if (G < 1) return resize_fail(who, "G must be at least 1");
  if (C == 0) return resize_fail(who, "C must be 1 or 3");
  if (H < 1 || W < 1 || h < 1 || w < 1 || H > RESIZE_MAX_DIM || W > RESIZE_MAX_DIM || h > RESIZE_MAX_DIM || w > RESIZE_MAX_DIM)
    return resize_fail(who, "sizes must be in 1..65536");
  if (!ratio_ok(H, h) || !ratio_ok(W, w)) return resize_fail(who, "ratio outside [1/64, 64] on an axis");
  if (W != w && (kk_h == nullptr || bounds_h == nullptr)) return resize_fail(who, "null horizontal table");
  if (H != h && (kk_v == nullptr || bounds_v == nullptr)) return resize_fail(who, "null vertical table");
  if (((reinterpret_cast<uintptr_t>(kk_h) | reinterpret_cast<uintptr_t>(bounds_h) | reinterpret_cast<uintptr_t>(kk_v) |
        reinterpret_cast<uintptr_t>(bounds_v) | reinterpret_cast<uintptr_t>(out_f32)) & 3u) != 0)
    return resize_fail(who, "the tables and the float output must be 4-byte aligned");
  if (out_f32 != nullptr && f32_image_stride < (uint64_t)C * (uint64_t)h * (uint64_t)w)
    return resize_fail(who, alpha ? "the float image stride is below 4 * h * w" : "the float image stride is below C * h * w");
  ResizeArgs a;
  a.in = in;
  a.H = H, a.W = W, a.C = C, a.h = h, a.w = w;
  a.kk_h = (W != w) ? kk_h : nullptr;
  a.bounds_h = (W != w) ? bounds_h : nullptr;
  a.kk_v = (H != h) ? kk_v : nullptr;
  a.bounds_v = (H != h) ? bounds_v : nullptr;
  a.ksize_h = axis_scale(W, w).ksize;
  a.ksize_v = axis_scale(H, h).ksize;
  // the largest tile whose rows fit the LDS: rows first (they cost recomputed taps), then columns
  int th = RESIZE_TH, tw = RESIZE_TW;
  while ((int64_t)rows_span(H, h, th) * tw * C > RESIZE_ROWS_BYTES) {
    if (th > 1) th /= 2;
    else if (tw > 1) tw /= 2;
    else return resize_fail(who, "no tile fits the LDS budget");                 // (not reachable within the ratio limits)
  }
  a.th = th, a.tw = tw;
  a.cap_rows = RESIZE_ROWS_BYTES / (tw * C);
  a.tiles_x = (uint32_t)((w + tw - 1) / tw);
  a.tiles_y = (uint32_t)((h + th - 1) / th);
  const uint64_t blocks = (uint64_t)G * a.tiles_x * a.tiles_y;
  if (blocks > 0x7fffffffull) return resize_fail(who, "more than 2^31 - 1 blocks");
  a.out_u8 = out_u8;
  a.out_f32 = out_f32;
  a.image_stride = f32_image_stride;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (alpha)
    hipLaunchKernelGGL((resize_u8_kernel<4, true>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
  else if (C == 3)
    hipLaunchKernelGGL((resize_u8_kernel<3, false>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((resize_u8_kernel<1, false>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, who);
}

// ------------------------------------------------------------------------------------------- RGBA over a background
constexpr int OVER_PIXELS = 4;                         // per thread: 16 input bytes
constexpr int OVER_BLOCK_PIXELS = 256 * OVER_PIXELS;

struct OverArgs {
  const uint8_t* in;         // [n_pixels, 4]
  uint64_t n_pixels;         // G H W
  uint64_t plane;            // H W
  double bg;                 // 0.0 or 1.0
  uint8_t* out_u8;           // [n_pixels, 3] or nullptr
  float* out_f32;            // [G] x image_stride floats, [3,H,W] each, or nullptr
  uint64_t image_stride;
};

__global__ void __launch_bounds__(256)
rgba_over_kernel(const OverArgs a) {
  __shared__ double unit[256];                         // x / 255.0
  __shared__ uint32_t stage[OVER_BLOCK_PIXELS * 3 / 4];      // the block's result bytes, pixel-interleaved
  const uint32_t t = threadIdx.x;
  unit[t] = (double)t / 255.0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * (uint64_t)OVER_BLOCK_PIXELS;
  const uint64_t p0 = base + (uint64_t)t * OVER_PIXELS;
  uint32_t px[OVER_PIXELS] = {0u, 0u, 0u, 0u};
  if (p0 + OVER_PIXELS <= a.n_pixels && (reinterpret_cast<uintptr_t>(a.in) & 15u) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(a.in + p0 * 4);
    px[0] = q.x, px[1] = q.y, px[2] = q.z, px[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < OVER_PIXELS; j++) {
      if (p0 + j < a.n_pixels) {
        const uint8_t* p = a.in + (p0 + j) * 4;
        px[j] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      }
    }
  }
  uint32_t packed[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < OVER_PIXELS; j++) {
    const double alpha = unit[px[j] >> 24];
    const double rest = a.bg * (1.0 - alpha);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double v = (unit[(px[j] >> (8 * c)) & 255u] * alpha + rest) * 255.0;
      const uint32_t byte = (uint32_t)(int)v & 255u;   // np.byte: truncation toward zero, the low byte kept
      const int k = 3 * j + c;
      packed[k >> 2] |= byte << (8 * (k & 3));
    }
  }
  stage[3 * t + 0] = packed[0], stage[3 * t + 1] = packed[1], stage[3 * t + 2] = packed[2];
  __syncthreads();
  if (base >= a.n_pixels) return;
  const uint64_t left = a.n_pixels - base;
  const uint32_t npix = left < (uint64_t)OVER_BLOCK_PIXELS ? (uint32_t)left : (uint32_t)OVER_BLOCK_PIXELS;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage);
  if (a.out_u8 != nullptr) {
    uint8_t* dst = a.out_u8 + base * 3;                // (base * 3 is a multiple of 4)
    const uint32_t nbytes = npix * 3u;
    if ((reinterpret_cast<uintptr_t>(a.out_u8) & 3u) == 0) {
      for (uint32_t i = t; i * 4u < nbytes; i += 256u) {
        if (i * 4u + 4u <= nbytes) {
          reinterpret_cast<uint32_t*>(dst)[i] = stage[i];
        } else {
          for (uint32_t b = i * 4u; b < nbytes; b++) dst[b] = bytes[b];
        }
      }
    } else {
      for (uint32_t i = t; i < nbytes; i += 256u) dst[i] = bytes[i];
    }
  }
  if (a.out_f32 != nullptr) {     // planar: lane t takes pixel t, t + 256, ... of the block, one plane after the other
#pragma unroll
    for (int k = 0; k < OVER_PIXELS; k++) {
      const uint32_t q = (uint32_t)k * 256u + t;
      if (q < npix) {
        const uint64_t p = base + q;
        const uint64_t g = p / a.plane, rem = p - g * a.plane;
        float* dst = a.out_f32 + g * a.image_stride + rem;
#pragma unroll
        for (int c = 0; c < 3; c++) dst[(uint64_t)c * a.plane] = (float)bytes[q * 3u + (uint32_t)c] / 255.0f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- depth keys
__global__ void __launch_bounds__(256)
zero_counts_kernel(uint32_t* __restrict__ counts, int m) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < m) counts[i] = 0u;
}

// grid (blocks over the points, camera).  One thread per (camera, point); the block's count of valid pairs goes through
// the wave ballots and LDS to ONE integer atomicAdd.
__global__ void __launch_bounds__(256)
depth_bound_keys_kernel(const double* __restrict__ points, int n, const double* __restrict__ w2c, double w, double h,
                        double fx, double fy, float* __restrict__ keys, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_count[4];
  const int cam = (int)blockIdx.y;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const double* m = w2c + (size_t)cam * 12;
  bool valid = false;
  if (i < (uint32_t)n) {
    const double px = points[(size_t)i * 3 + 0], py = points[(size_t)i * 3 + 1], pz = points[(size_t)i * 3 + 2];
    const double cx = m[0] * px + m[1] * py + m[2] * pz + m[3];
    const double cy = m[4] * px + m[5] * py + m[6] * pz + m[7];
    const double cz = m[8] * px + m[9] * py + m[10] * pz + m[11];
    const double u = cx / fx, v = cy / fy;
    const double d = cz - cx * (w / 2) / fx - cy * (h / 2) / fy;
    const double qx = u / d, qy = v / d;
    valid = cz > 0.01 && qx >= 0.0 && qx < w && qy >= 0.0 && qy < h;      // (a NaN compares false: not counted)
    keys[(size_t)cam * (size_t)n + i] = valid ? (float)cz : __int_as_float(0x7fc00000);
  }
  const unsigned long long ballot = __ballot(valid);
  if (dgs_lane() == 0) wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    if (total != 0u) atomicAdd(&counts[cam], total);
  }
}

}  // namespace

extern "C" {

int32_t dgs_resample_ksize(int32_t in_size, int32_t out_size) {
  if (!ratio_ok(in_size, out_size)) return 0;
  return axis_scale(in_size, out_size).ksize;
}

int dgs_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* kk, uint64_t kk_capacity, int32_t* bounds) {
  if (kk == nullptr || bounds == nullptr) return dgs_fail_arg("resample_coeffs: null pointer");
  if (in_size < 1 || out_size < 1 || in_size > RESIZE_MAX_DIM || out_size > RESIZE_MAX_DIM)
    return dgs_fail_arg("resample_coeffs: sizes must be in 1..65536");
  if (!ratio_ok(in_size, out_size)) return dgs_fail_arg("resample_coeffs: ratio in_size / out_size outside [1/64, 64]");
  const AxisScale a = axis_scale(in_size, out_size);
  if (kk_capacity < (uint64_t)out_size * (uint64_t)a.ksize)
    return dgs_fail_arg("resample_coeffs: kk holds fewer than out_size * ksize entries");
  const double ss = 1.0 / a.filterscale;
  double w[2 * 2 * (int)RESIZE_MAX_RATIO + 4];        // ksize <= 2 * 128 + 1
  for (int xx = 0; xx < out_size; xx++) {
    const double center = (xx + 0.5) * a.scale;
    int xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; x++) {
      w[x] = bicubic_filter((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int32_t* k = kk + (size_t)xx * (size_t)a.ksize;
    for (int x = 0; x < xmax; x++) {
      if (ww != 0.0) w[x] /= ww;
      k[x] = w[x] < 0 ? (int32_t)(-0.5 + w[x] * (1 << RESIZE_PRECISION_BITS))
                      : (int32_t)(0.5 + w[x] * (1 << RESIZE_PRECISION_BITS));
    }
    for (int x = xmax; x < a.ksize; x++) k[x] = 0;
    bounds[2 * xx + 0] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return DGS_OK;
}

int dgs_resize_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, const int32_t* kk_h,
                  const int32_t* bounds_h, const int32_t* kk_v, const int32_t* bounds_v, uint8_t* out_u8, float* out_f32,
                  uint64_t f32_image_stride, dgs_stream_t stream) {
  return resize_call("resize_u8", false, in, G, H, W, (C == 1 || C == 3) ? C : 0, h, w, kk_h, bounds_h, kk_v, bounds_v, out_u8,
                     out_f32, f32_image_stride, stream);
}

int dgs_resize_rgba_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t h, int32_t w, const int32_t* kk_h,
                       const int32_t* bounds_h, const int32_t* kk_v, const int32_t* bounds_v, uint8_t* out_u8, float* out_f32,
                       uint64_t f32_image_stride, dgs_stream_t stream) {
  return resize_call("resize_rgba_u8", true, in, G, H, W, 4, h, w, kk_h, bounds_h, kk_v, bounds_v, out_u8, out_f32,
                     f32_image_stride, stream);
}

int dgs_rgba_over_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t white, uint8_t* out_u8, float* out_f32,
                     uint64_t f32_image_stride, dgs_stream_t stream) {
  if (in == nullptr) return dgs_fail_arg("rgba_over_u8: null input pointer");
  if (out_u8 == nullptr && out_f32 == nullptr) return dgs_fail_arg("rgba_over_u8: both outputs are null");
  if (G < 1) return dgs_fail_arg("rgba_over_u8: G must be at least 1");
  if (H < 1 || W < 1 || H > RESIZE_MAX_DIM || W > RESIZE_MAX_DIM) return dgs_fail_arg("rgba_over_u8: sizes must be in 1..65536");
  if ((reinterpret_cast<uintptr_t>(out_f32) & 3u) != 0)
    return dgs_fail_arg("rgba_over_u8: the float output must be 4-byte aligned");
  const uint64_t plane = (uint64_t)H * (uint64_t)W;
  if (out_f32 != nullptr && f32_image_stride < 3 * plane)
    return dgs_fail_arg("rgba_over_u8: the float image stride is below 3 * H * W");
  OverArgs a;
  a.in = in;
  a.n_pixels = (uint64_t)G * plane;
  a.plane = plane;
  a.bg = white != 0 ? 1.0 : 0.0;
  a.out_u8 = out_u8;
  a.out_f32 = out_f32;
  a.image_stride = f32_image_stride;
  const uint64_t blocks = (a.n_pixels + OVER_BLOCK_PIXELS - 1) / OVER_BLOCK_PIXELS;
  if (blocks > 0x7fffffffull) return dgs_fail_arg("rgba_over_u8: more than 2^31 - 1 blocks");
  hipLaunchKernelGGL(rgba_over_kernel, dim3((uint32_t)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "rgba_over_u8");
}

int dgs_depth_bound_keys(const double* points, int32_t n, const double* w2c, int32_t m, double w, double h, double fx,
                         double fy, float* keys, uint32_t* counts, dgs_stream_t stream) {
  if (points == nullptr || w2c == nullptr || keys == nullptr || counts == nullptr)
    return dgs_fail_arg("depth_bound_keys: null pointer");
  if (n < 1) return dgs_fail_arg("depth_bound_keys: n must be at least 1");
  if (m < 1 || m > 65535) return dgs_fail_arg("depth_bound_keys: m must be in 1..65535");
  if (!(w > 0.0) || !(h > 0.0) || !(fx > 0.0) || !(fy > 0.0) || !isfinite(w) || !isfinite(h) || !isfinite(fx) || !isfinite(fy))
    return dgs_fail_arg("depth_bound_keys: w, h, fx, fy must be positive and finite");
  if (((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(w2c)) & 7u) != 0)
    return dgs_fail_arg("depth_bound_keys: points and w2c must be 8-byte aligned");
  if (((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(counts)) & 3u) != 0)
    return dgs_fail_arg("depth_bound_keys: keys and counts must be 4-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(zero_counts_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, counts, (int)m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "depth_bound_keys (clear)");
  hipLaunchKernelGGL(depth_bound_keys_kernel, dim3((uint32_t)(((uint32_t)n + 255u) / 256u), (uint32_t)m), dim3(256), 0, st,
                     points, (int)n, w2c, w, h, fx, fy, keys, counts);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "depth_bound_keys");
}

}  // extern "C"

// draw.hip -- what the reference's training-progress visualiser draws on the host (utils/visualization.py:138-189: numpy
// projections and cv2.line per camera cone), on the device:
//   * dgs_draw_prims: a list of one-pixel lines and filled discs painted into an 8-bit RGB image in painter's order.  A
//     first kernel -- one wave per primitive, its lanes striding the primitive's pixels -- raises owner[pixel] to the
//     primitive's index + 1 with an integer atomicMax; a second pass writes the colour of that primitive into every pixel
//     that has an owner.  The maximum does not depend on the order of arrival: the bytes are a function of the arguments.
//   * dgs_cone_segments: draw_cone_on_render_img's arithmetic in double, one thread per drawn camera, 8 line records each.
// Built with -ffp-contract=off (deblurgs_amd/build.py): the double chain rounds once per statement, as numpy's does.
// Integer global atomics (atomicMax on 32-bit words) in the mark kernel only; pixels leave by plain byte stores.
#include <math.h>
#include <stdio.h>

#include "dgs_common.h"

namespace {

constexpr int DRAW_THREADS = 256;
constexpr int DRAW_WAVES = DRAW_THREADS / DGS_WAVE;
constexpr int DRAW_MAX_COORD = 1 << 29;      // |coordinate| above this: the record is skipped (64-bit products stay exact)
constexpr int DRAW_MAX_RADIUS = 64;
constexpr int DRAW_REC = 6;                  // x0, y0, x1, y1, r, rgb

__device__ __forceinline__ bool draw_coord_ok(int v) { return v >= -DRAW_MAX_COORD && v <= DRAW_MAX_COORD; }

// One wave per record.  Line (r == 0): step i = 0 .. maj along the major axis from (x0, y0); the minor offset at step i is
// floor((2 min i + maj - 1) / (2 maj)) -- the integer Bresenham walk with error term maj - 2 min in closed form, ties to
// the start point.  The step range is clipped to the image along the major axis BEFORE the loop (hi - lo < the image's
// extent on that axis), so a lane loops at most max(W, H) / 64 + 1 times wherever the endpoints lie; a step whose minor
// coordinate is outside is dropped.  Disc (r > 0): the pixels of its bounding box clipped to the image, at most 129 x 129.
__global__ void __launch_bounds__(DRAW_THREADS)
draw_mark_kernel(const int32_t* __restrict__ prims, int n, int W, int H, uint32_t* __restrict__ owner) {
  const int lane = dgs_lane();
  const int64_t p = (int64_t)blockIdx.x * DRAW_WAVES + (int64_t)(threadIdx.x >> 6);
  if (p >= (int64_t)n) return;
  const int32_t* __restrict__ rec = prims + p * DRAW_REC;
  const int x0 = rec[0], y0 = rec[1], x1 = rec[2], y1 = rec[3], r = rec[4];
  if (r < 0 || !draw_coord_ok(x0) || !draw_coord_ok(y0) || !draw_coord_ok(x1) || !draw_coord_ok(y1)) return;
  const uint32_t tag = (uint32_t)p + 1u;
  if (r > 0) {
    if (x0 != x1 || y0 != y1 || r > DRAW_MAX_RADIUS) return;
    const int bx0 = max(x0 - r, 0), bx1 = min(x0 + r, W - 1), by0 = max(y0 - r, 0), by1 = min(y0 + r, H - 1);
    if (bx0 > bx1 || by0 > by1) return;
    const int bw = bx1 - bx0 + 1, count = bw * (by1 - by0 + 1);
    for (int i = lane; i < count; i += DGS_WAVE) {
      const int y = by0 + i / bw, x = bx0 + i % bw;
      const int ex = x - x0, ey = y - y0;          // both within [-r, r]
      if (ex * ex + ey * ey <= r * r) atomicMax(&owner[(size_t)y * (size_t)W + (size_t)x], tag);
    }
    return;
  }
  const int64_t dx = x1 > x0 ? (int64_t)x1 - x0 : (int64_t)x0 - x1, dy = y1 > y0 ? (int64_t)y1 - y0 : (int64_t)y0 - y1;
  const bool steep = dy > dx;
  const int64_t maj = steep ? dy : dx, mn = steep ? dx : dy;
  const int sx = x1 > x0 ? 1 : (x1 < x0 ? -1 : 0), sy = y1 > y0 ? 1 : (y1 < y0 ? -1 : 0);
  const int64_t m0 = steep ? y0 : x0, n0 = steep ? x0 : y0;
  const int sm = steep ? sy : sx, sn = steep ? sx : sy;
  const int64_t Lm = steep ? H : W, Ln = steep ? W : H;
  int64_t lo = 0, hi = maj;
  if (sm > 0) {
    lo = max(lo, -m0);
    hi = min(hi, Lm - 1 - m0);
  } else if (sm < 0) {
    lo = max(lo, m0 - (Lm - 1));
    hi = min(hi, m0);
  } else if (m0 < 0 || m0 >= Lm) {      // a single point (maj == 0)
    return;
  }
  const bool small = maj < 32768;       // 2 min i + maj - 1 < 2^31: 32-bit division
  for (int64_t i = lo + lane; i <= hi; i += DGS_WAVE) {
    int64_t off = 0;
    if (maj > 0)
      off = small ? (int64_t)((2u * (uint32_t)mn * (uint32_t)i + (uint32_t)maj - 1u) / (2u * (uint32_t)maj))
                  : (2 * mn * i + maj - 1) / (2 * maj);
    const int64_t m = m0 + sm * i, q = n0 + sn * off;
    if (q < 0 || q >= Ln) continue;
    const int64_t x = steep ? q : m, y = steep ? m : q;
    atomicMax(&owner[(size_t)y * (size_t)W + (size_t)x], tag);
  }
}

// Every pixel with an owner takes that record's colour; every other byte of the image stays as it was.
__global__ void __launch_bounds__(DRAW_THREADS)
draw_resolve_kernel(uint8_t* __restrict__ img, size_t npix, const uint32_t* __restrict__ owner,
                    const int32_t* __restrict__ prims) {
  for (size_t pix = (size_t)blockIdx.x * DRAW_THREADS + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * DRAW_THREADS) {
    const uint32_t o = owner[pix];
    if (o == 0u) continue;
    const uint32_t rgb = (uint32_t)prims[(size_t)(o - 1u) * DRAW_REC + 5];
    img[3 * pix + 0] = (uint8_t)(rgb & 255u);
    img[3 * pix + 1] = (uint8_t)((rgb >> 8) & 255u);
    img[3 * pix + 2] = (uint8_t)((rgb >> 16) & 255u);
  }
}

struct ConeArgs {
  double tanx, tany, scale;
  int W, H;
};

// (a pixel coordinate as astype(int) leaves it: truncated toward zero; false where the reference's cv2.line would have
// raised -- a non-finite value -- or the record would be skipped by dgs_draw_prims anyway)
__device__ __forceinline__ bool cone_pixel(double v, int32_t& out) {
  const double t = trunc(v);
  if (!(fabs(t) <= (double)DRAW_MAX_COORD)) return false;
  out = (int32_t)t;
  return true;
}

// utils/visualization.py:156-185 for camera c.  Row-vector convention throughout: hom @ M is out[j] = sum_k hom[k] M[k][j].
__global__ void __launch_bounds__(DRAW_THREADS)
cone_segments_kernel(const float* __restrict__ view, const float* __restrict__ campos, ConeArgs a,
                     const float* __restrict__ render_view, const float* __restrict__ render_proj,
                     const int32_t* __restrict__ rgb, int32_t* __restrict__ out, int C) {
  const int c = (int)(blockIdx.x * DRAW_THREADS + threadIdx.x);
  if (c >= C) return;
  const float* __restrict__ v = view + (size_t)c * 16;
  double c2w[3][4];      // get_c2w: the rotation block of the view matrix, the camera centre; the last row is (0, 0, 0, 1)
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c2w[i][j] = (double)v[i * 4 + j];
    c2w[i][3] = (double)campos[(size_t)c * 3 + i];
  }
  const double sgx[5] = {0.0, 1.0, 1.0, -1.0, -1.0}, sgy[5] = {0.0, 1.0, -1.0, -1.0, 1.0};
  int32_t px[5] = {0, 0, 0, 0, 0}, py[5] = {0, 0, 0, 0, 0};
  bool ok[5];
  bool behind = false;
  for (int k = 0; k < 5; k++) {
    const double local[4] = {sgx[k] * a.tanx * a.scale, sgy[k] * a.tany * a.scale, (k == 0 ? 0.0 : 1.0) * a.scale, 1.0};
    // the skip test takes the camera-LOCAL cone through the render camera's view matrix, as the reference does
    double cz = 0.0, cw = 0.0;
    for (int i = 0; i < 4; i++) {
      cz += local[i] * (double)render_view[i * 4 + 2];
      cw += local[i] * (double)render_view[i * 4 + 3];
    }
    if (cz / cw < 0.1) behind = true;
    double world[4];     // local @ c2w.T
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int i = 0; i < 4; i++) s += local[i] * c2w[j][i];
      world[j] = s;
    }
    world[3] = 1.0;
    double nx = 0.0, ny = 0.0, nw = 0.0;
    for (int i = 0; i < 4; i++) {
      nx += world[i] * (double)render_proj[i * 4 + 0];
      ny += world[i] * (double)render_proj[i * 4 + 1];
      nw += world[i] * (double)render_proj[i * 4 + 3];
    }
    const double fx = ((nx / nw + 1.0) * (double)a.W - 1.0) * 0.5, fy = ((ny / nw + 1.0) * (double)a.H - 1.0) * 0.5;
    const bool okx = cone_pixel(fx, px[k]), oky = cone_pixel(fy, py[k]);
    ok[k] = okx && oky;
  }
  const int ea[8] = {0, 0, 0, 0, 1, 2, 3, 4}, eb[8] = {1, 2, 3, 4, 2, 3, 4, 1};
  const int32_t colour = rgb[c];
  int32_t* __restrict__ dst = out + (size_t)c * 8 * DRAW_REC;
  for (int e = 0; e < 8; e++) {
    const int i = ea[e], j = eb[e];
    const bool drawn = !behind && ok[i] && ok[j];
    dst[e * DRAW_REC + 0] = drawn ? px[i] : 0;
    dst[e * DRAW_REC + 1] = drawn ? py[i] : 0;
    dst[e * DRAW_REC + 2] = drawn ? px[j] : 0;
    dst[e * DRAW_REC + 3] = drawn ? py[j] : 0;
    dst[e * DRAW_REC + 4] = drawn ? 0 : -1;
    dst[e * DRAW_REC + 5] = colour;
  }
}

}  // namespace

extern "C" {

int dgs_draw_prims(uint8_t* img, int32_t W, int32_t H, const int32_t* prims, int32_t n, uint32_t* owner,
                   dgs_stream_t stream) {
  if (img == nullptr || prims == nullptr || owner == nullptr) return dgs_fail_arg("draw_prims: null pointer");
  if (W <= 0 || H <= 0) return dgs_fail_arg("draw_prims: W and H must be positive");
  if ((uint64_t)W * (uint64_t)H >= (1ull << 31)) return dgs_fail_arg("draw_prims: image of 2^31 pixels or more");
  if (n < 0) return dgs_fail_arg("draw_prims: n must not be negative");
  if (n == 0) return DGS_OK;
  if ((reinterpret_cast<uintptr_t>(prims) & 3u) != 0 || (reinterpret_cast<uintptr_t>(owner) & 3u) != 0)
    return dgs_fail_arg("draw_prims: prims and owner must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t npix = (size_t)W * (size_t)H;
  hipError_t e = hipMemsetAsync(owner, 0, npix * sizeof(uint32_t), s);
  if (e != hipSuccess) return dgs_fail_hip(e, "draw_prims (clear)");
  const uint32_t mark_blocks = (uint32_t)(((int64_t)n + DRAW_WAVES - 1) / DRAW_WAVES);
  hipLaunchKernelGGL(draw_mark_kernel, dim3(mark_blocks), dim3(DRAW_THREADS), 0, s, prims, (int)n, (int)W, (int)H, owner);
  e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "draw_prims (mark)");
  const size_t want = (npix + DRAW_THREADS - 1) / DRAW_THREADS;
  hipLaunchKernelGGL(draw_resolve_kernel, dim3((uint32_t)(want < 8192 ? want : 8192)), dim3(DRAW_THREADS), 0, s, img, npix,
                     owner, prims);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "draw_prims (resolve)");
}

int dgs_cone_segments(int32_t C, const float* view, const float* campos, double tanx, double tany, double scale,
                      const float* render_view, const float* render_proj, int32_t W, int32_t H, const int32_t* rgb,
                      int32_t* prims_out, dgs_stream_t stream) {
  if (view == nullptr || campos == nullptr || render_view == nullptr || render_proj == nullptr || rgb == nullptr ||
      prims_out == nullptr)
    return dgs_fail_arg("cone_segments: null pointer");
  if (W <= 0 || H <= 0) return dgs_fail_arg("cone_segments: W and H must be positive");
  if (C < 0) return dgs_fail_arg("cone_segments: C must not be negative");
  if (C == 0) return DGS_OK;
  if (((reinterpret_cast<uintptr_t>(view) | reinterpret_cast<uintptr_t>(campos) | reinterpret_cast<uintptr_t>(render_view) |
        reinterpret_cast<uintptr_t>(render_proj) | reinterpret_cast<uintptr_t>(rgb) |
        reinterpret_cast<uintptr_t>(prims_out)) & 3u) != 0)
    return dgs_fail_arg("cone_segments: pointers must be 4-byte aligned");
  if (C > (1 << 24)) return dgs_fail_arg("cone_segments: C above 2^24");
  ConeArgs a;
  a.tanx = tanx;
  a.tany = tany;
  a.scale = scale;
  a.W = (int)W;
  a.H = (int)H;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cone_segments_kernel, dim3((uint32_t)((C + DRAW_THREADS - 1) / DRAW_THREADS)), dim3(DRAW_THREADS), 0, s,
                     view, campos, a, render_view, render_proj, rgb, prims_out, (int)C);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "cone_segments");
}

}  // extern "C"

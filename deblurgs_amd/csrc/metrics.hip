// metrics.hip -- the image-space kernels of the evaluation protocol (test.py:93-186 of the reference):
//   * dgs_view_loss_grad: the loss of one step of the test-view pose fit (test.py:171-178) -- tone mapping
//     (scene/tonemapping.py), clamp to [0, 1], L1 against the test image -- with its value, the MSE of the reference's
//     l2_error_ema and dL/d(render) in one pass;
//   * dgs_image_metrics: PSNR (utils/image_utils.py:17-19) and SSIM (utils/loss_utils.py:23-63) of two [3,H,W] images in
//     one launch plus a reduction.
// Built with -ffp-contract=off (deblurgs_amd/build.py): the SSIM of an image with itself is exactly 1 only while
// 2 (mu1 mu2) and mu1^2 + mu2^2 round the same way.
// Every total is deterministic: per-block sums in a fixed order, then either integer (fixed-point) atomics or a second
// kernel that adds the blocks in index order.
#include <math.h>
#include <string.h>

#include "dgs_common.h"

namespace {

// sum over the 256 threads of a block in a fixed order (lane order inside a wave, then wave order); valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------------------------------- view loss
// One element per thread and grid stride: y = clamp(tone_map(x), 0, 1), d = y - gt, l1 += |d|, mse += d^2,
//   dL/dx = upstream * sign(d) / E * [0 <= tone_map(x) <= 1] * tone_map'(x)
// with torch's conventions: clamp and clamp_min pass the gradient on the bound, sign(0) = 0.  gamma:
//   tone_map(x) = max((x - bound) / (1 - 2 bound), eps) ^ (1 / 2.2)   (losses.ToneMapping)
// and its derivative as torch's pow backward forms it: (1 / 2.2) u ^ (1 / 2.2 - 1), exponents rounded to fp32.
// work: 12 words, zeroed by the launcher -- [0] l1, [1] mse (fp32), [2..7] the deterministic totals' own words
// (dgs_totals_publish, dgs_common.h), [8..9] / [10..11] the two values as fp64.
// (the body of both kernels below: one image on the blocks of grid-x)
template <int GAMMA>
__device__ __forceinline__ void view_loss_image(const float* __restrict__ x, const float* __restrict__ gt, size_t E, float eps,
                                                float bound, const float* __restrict__ upstream, float* __restrict__ dL_dx,
                                                float* __restrict__ work, float* __restrict__ l2_ema,
                                                const uint32_t* __restrict__ skip_flag, double* red) {
  const float up = (upstream != nullptr) ? upstream[0] : 1.0f;
  const float c_l1 = (float)((double)up / (double)E);
  const float inv_span = 1.0f - 2.0f * bound;
  const float ex = (float)(1.0 / 2.2), ex1 = (float)(1.0 / 2.2 - 1.0);
  double l1 = 0.0, l2 = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (size_t)gridDim.x * 256) {
    const float xv = x[e];
    float y0 = xv, dy = 1.0f;
    if (GAMMA) {
      const float u = (xv - bound) / inv_span;
      const float uc = fmaxf(u, eps);
      y0 = powf(uc, ex);
      // d/dx of clamp_min(u, eps) ^ ex: zero below eps, (ex * uc ^ (ex - 1)) / (1 - 2 bound) from eps on
      dy = (u >= eps) ? (ex * powf(uc, ex1)) / inv_span : 0.0f;
    }
    // (fmaxf / fminf drop a NaN operand, torch's clamp and clamp_min pass it on: a NaN in x must reach the totals)
    const float y = (xv != xv) ? xv : fminf(1.0f, fmaxf(0.0f, y0));
    const bool pass = y0 >= 0.0f && y0 <= 1.0f;   // torch.clamp passes the gradient inside and on the bounds
    const float d = y - gt[e];
    l1 += (double)fabsf(d);
    l2 += (double)d * (double)d;
    if (dL_dx != nullptr) dL_dx[e] = (pass && dy != 0.0f) ? (c_l1 * dgs_sgn(d)) * dy : 0.0f;
  }
  if (work == nullptr) return;
  const double a = block_sum_256(l1, red), c = block_sum_256(l2, red);
  if (threadIdx.x != 0) return;
  unsigned long long t0, t1;
  bool bad;
  if (dgs_totals_publish(a, c, work, t0, t1, bad)) {
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const double v1 = bad ? nanv : ((double)t0 / DGS_TOTALS_FX) / (double)E;
    const double v2 = bad ? nanv : ((double)t1 / DGS_TOTALS_FX) / (double)E;
    work[0] = (float)v1;
    work[1] = (float)v2;
    reinterpret_cast<double*>(work + 8)[0] = v1;
    reinterpret_cast<double*>(work + 8)[1] = v2;
    // l2_error_ema = 0.6 l2_error_ema + 0.4 mse (test.py:178); a step whose forward overflowed its capacity does not count
    if (l2_ema != nullptr && (skip_flag == nullptr || skip_flag[0] == 0u)) l2_ema[0] = l2_ema[0] * 0.6f + (float)v2 * 0.4f;
  }
}

template <int GAMMA>
__global__ void __launch_bounds__(256)
view_loss_kernel(const float* __restrict__ x, const float* __restrict__ gt_base, const int32_t* __restrict__ gt_index,
                 int n_gt, size_t E, float eps, float bound, const float* __restrict__ upstream, float* __restrict__ dL_dx,
                 float* __restrict__ work, float* __restrict__ l2_ema, const uint32_t* __restrict__ skip_flag) {
  __shared__ double red[256];
  int gi = (gt_index != nullptr) ? gt_index[0] : 0;
  if (gi < 0 || gi >= n_gt) gi = 0;   // (a corrupt index must not read out of bounds; testpose_kernel does the same)
  view_loss_image<GAMMA>(x, gt_base + (size_t)gi * E, E, eps, bound, upstream, dL_dx, work, l2_ema, skip_flag, red);
}

// G images in one launch (EpochPoseFit): image k = blockIdx.y of x [G,C,HW] against image row_begin + k of the stack, its
// own gradient image and its own 12-word work area.  Grid-x is the single-image launcher's, so every image's block sums,
// totals and gradient are those of a dgs_view_loss_grad call on it.
template <int GAMMA>
__global__ void __launch_bounds__(256)
view_loss_rows_kernel(const float* __restrict__ x, const float* __restrict__ gt_base, int row_begin, size_t E, float eps,
                      float bound, const float* __restrict__ upstream, float* __restrict__ dL_dx, float* __restrict__ work) {
  __shared__ double red[256];
  const size_t k = blockIdx.y;
  view_loss_image<GAMMA>(x + k * E, gt_base + ((size_t)row_begin + k) * E, E, eps, bound, upstream,
                         dL_dx != nullptr ? dL_dx + k * E : nullptr, work + 12 * k, nullptr, nullptr, red);
}

// l2_error_ema over an epoch (test.py:178): ema = 0.6 ema + 0.4 mse of the views IN THE ORDER OF THEIR TURNS.  work
// [n,12]: the views' work areas by row; pos [n]: the turn of row r (the inverse of the epoch's order).  The rows of a
// group whose forward overflowed (its skip word is non-zero) do not count.  One block: thread r files row r under its
// turn, thread 0 walks the turns.
struct EmaGroups {
  const uint32_t* skip[DGS_MAX_K];
  int32_t begin[DGS_MAX_K + 1];     // group g covers rows [begin[g], begin[g + 1])
  int n_groups;
};
__global__ void __launch_bounds__(DGS_MAX_K)
l2_ema_epoch_kernel(const float* __restrict__ work, const int32_t* __restrict__ pos, int n, EmaGroups groups,
                    float* __restrict__ l2_ema) {
  __shared__ int s_row[DGS_MAX_K];
  __shared__ unsigned char s_skip[DGS_MAX_K];
  const int r = threadIdx.x;
  s_row[r] = -1;
  __syncthreads();
  if (r < n) {
    int g = 0;
    while (g < groups.n_groups - 1 && r >= groups.begin[g + 1]) g++;
    s_skip[r] = (groups.skip[g] != nullptr && groups.skip[g][0] != 0u) ? 1 : 0;
    const int turn = pos[r];
    if (turn >= 0 && turn < n) s_row[turn] = r;   // (a corrupt position files nothing: no write out of bounds)
  }
  __syncthreads();
  if (r != 0) return;
  float ema = l2_ema[0];
  for (int j = 0; j < n; j++) {
    const int row = s_row[j];
    if (row < 0 || s_skip[row]) continue;
    ema = ema * 0.6f + work[12 * row + 1] * 0.4f;
  }
  l2_ema[0] = ema;
}

// ------------------------------------------------------------------------------------------- PSNR + SSIM
// One block per 16 x 16 output tile of one channel.  The (16 + 10)^2 halo of both images goes to LDS (zeros outside the
// image: conv2d's zero padding), the 11-tap Gaussian runs along x for the five windowed quantities (a, b, a^2, b^2, a b),
// then along y; arithmetic in fp64 (the variance terms are differences of nearly equal numbers; the kernel is far from
// any fp64 limit: 110 multiply-adds per pixel and channel).  The block writes its SSIM-map sum and its squared-error sum
// to partials[block][2]; metrics_reduce_kernel adds the blocks of every channel in index order.
constexpr int MT = 16, MR = 5, MH = MT + 2 * MR;   // tile, window radius, tile + halo

struct SsimWindow {
  float w[2 * MR + 1];
};

__global__ void __launch_bounds__(256)
metrics_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, SsimWindow win,
                    double* __restrict__ partials) {
  __shared__ double s_a[MH][MH + 1], s_b[MH][MH + 1];
  __shared__ double s_h[5][MH][MT + 1];
  __shared__ double red[256];
  const int ch = blockIdx.z;
  const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
  const float* pa = a + (size_t)ch * H * W;
  const float* pb = b + (size_t)ch * H * W;
  double se = 0.0;
  for (int i = threadIdx.x; i < MH * MH; i += 256) {
    const int ly = i / MH, lx = i % MH;
    const int gy = y0 + ly - MR, gx = x0 + lx - MR;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const double va = in ? (double)pa[(size_t)gy * W + gx] : 0.0;
    const double vb = in ? (double)pb[(size_t)gy * W + gx] : 0.0;
    s_a[ly][lx] = va;
    s_b[ly][lx] = vb;
    // the squared error of the tile's own pixels (PSNR)
    if (in && ly >= MR && ly < MR + MT && lx >= MR && lx < MR + MT) se += (va - vb) * (va - vb);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MH * MT; i += 256) {
    const int ly = i / MT, lx = i % MT;
    double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
    for (int t = 0; t < 2 * MR + 1; t++) {
      const double w = (double)win.w[t];
      const double va = s_a[ly][lx + t], vb = s_b[ly][lx + t];
      ha += w * va;
      hb += w * vb;
      haa += w * (va * va);
      hbb += w * (vb * vb);
      hab += w * (va * vb);
    }
    s_h[0][ly][lx] = ha;
    s_h[1][ly][lx] = hb;
    s_h[2][ly][lx] = haa;
    s_h[3][ly][lx] = hbb;
    s_h[4][ly][lx] = hab;
  }
  __syncthreads();
  const int ly = threadIdx.x / MT, lx = threadIdx.x % MT;
  double ss = 0.0;
  if (y0 + ly < H && x0 + lx < W) {
    double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int t = 0; t < 2 * MR + 1; t++) {
      const double w = (double)win.w[t];
      mu1 += w * s_h[0][ly + t][lx];
      mu2 += w * s_h[1][ly + t][lx];
      e11 += w * s_h[2][ly + t][lx];
      e22 += w * s_h[3][ly + t][lx];
      e12 += w * s_h[4][ly + t][lx];
    }
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    ss = ((2.0 * mu1_mu2 + C1) * (2.0 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2));
  }
  const double tot_ss = block_sum_256(ss, red), tot_se = block_sum_256(se, red);
  if (threadIdx.x == 0) {
    const size_t blk = ((size_t)ch * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * blk] = tot_ss;
    partials[2 * blk + 1] = tot_se;
  }
}

// out[0] = mean over the channels of 20 log10(1 / sqrt(mse_c)), out[1] = mean of the SSIM map, out[2 + c] = the PSNR of
// channel c
__global__ void __launch_bounds__(256)
metrics_reduce_kernel(const double* __restrict__ partials, int blocks_per_channel, int C, double HW,
                      float* __restrict__ out) {
  __shared__ double red[256];
  double psnr = 0.0, ssim = 0.0;
  for (int c = 0; c < C; c++) {
    double ss = 0.0, se = 0.0;
    for (int i = threadIdx.x; i < blocks_per_channel; i += 256) {
      ss += partials[2 * ((size_t)c * blocks_per_channel + i)];
      se += partials[2 * ((size_t)c * blocks_per_channel + i) + 1];
    }
    ss = block_sum_256(ss, red);
    se = block_sum_256(se, red);
    ssim += ss;
    const double db = 20.0 * log10(1.0 / sqrt(se / HW));
    psnr += db;
    if (threadIdx.x == 0) out[2 + c] = (float)db;
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(psnr / (double)C);
    out[1] = (float)(ssim / (HW * (double)C));
  }
}

}  // namespace

extern "C" {

int dgs_view_loss_grad(const float* x, const float* gt, const int32_t* gt_index_dev, int32_t n_gt, int32_t C, int32_t HW,
                       int32_t tone_mapping, float eps, float bound, const float* upstream, float* dL_dx, float* work,
                       float* l2_ema, const uint32_t* skip_flag, dgs_stream_t stream) {
  if (x == nullptr || gt == nullptr || n_gt < 1 || C < 1 || HW < 1 || (dL_dx == nullptr && work == nullptr))
    return dgs_fail_arg("view_loss_grad: null image, empty image or no output requested");
  if (tone_mapping != DGS_TONE_IDENTITY && tone_mapping != DGS_TONE_GAMMA)
    return dgs_fail_arg("view_loss_grad: tone_mapping must be DGS_TONE_IDENTITY or DGS_TONE_GAMMA");
  if (tone_mapping == DGS_TONE_GAMMA && !(bound < 0.5f)) return dgs_fail_arg("view_loss_grad: bound must be below 0.5");
  if (l2_ema != nullptr && work == nullptr) return dgs_fail_arg("view_loss_grad: l2_ema needs the work area");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t E = (size_t)C * (size_t)HW;
  if (work != nullptr) {
    hipError_t e = dgs_launch_clear_words(reinterpret_cast<uint32_t*>(work), 12, s);
    if (e != hipSuccess) return dgs_fail_hip(e, "view_loss_grad (clear)");
  }
  const size_t want = (E + 255) / 256;
  const dim3 grid((uint32_t)(want < 1024 ? want : 1024));   // a function of E only: the totals are reproducible
  if (tone_mapping == DGS_TONE_GAMMA)
    hipLaunchKernelGGL(view_loss_kernel<1>, grid, dim3(256), 0, s, x, gt, gt_index_dev, (int)n_gt, E, eps, bound, upstream, dL_dx, work,
                       l2_ema, skip_flag);
  else
    hipLaunchKernelGGL(view_loss_kernel<0>, grid, dim3(256), 0, s, x, gt, gt_index_dev, (int)n_gt, E, eps, bound, upstream, dL_dx, work,
                       l2_ema, skip_flag);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "view_loss_grad");
}

int dgs_view_loss_grad_rows(const float* x, const float* gt, int32_t n_gt, int32_t row_begin, int32_t row_end, int32_t C,
                            int32_t HW, int32_t tone_mapping, float eps, float bound, const float* upstream, float* dL_dx,
                            float* work, dgs_stream_t stream) {
  if (x == nullptr || gt == nullptr || work == nullptr || C < 1 || HW < 1)
    return dgs_fail_arg("view_loss_grad_rows: null image, empty image or no work area");
  if (n_gt < 1 || row_begin < 0 || row_end > n_gt || row_begin >= row_end)
    return dgs_fail_arg("view_loss_grad_rows: n_gt < 1, empty row range or row_end > n_gt");
  if (row_end - row_begin > DGS_MAX_K) return dgs_fail_arg("view_loss_grad_rows: more than DGS_MAX_K images");
  if (tone_mapping != DGS_TONE_IDENTITY && tone_mapping != DGS_TONE_GAMMA)
    return dgs_fail_arg("view_loss_grad_rows: tone_mapping must be DGS_TONE_IDENTITY or DGS_TONE_GAMMA");
  if (tone_mapping == DGS_TONE_GAMMA && !(bound < 0.5f)) return dgs_fail_arg("view_loss_grad_rows: bound must be below 0.5");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int G = row_end - row_begin;
  const size_t E = (size_t)C * (size_t)HW;
  hipError_t e = dgs_launch_clear_words(reinterpret_cast<uint32_t*>(work), 12 * G, s);
  if (e != hipSuccess) return dgs_fail_hip(e, "view_loss_grad_rows (clear)");
  const size_t want = (E + 255) / 256;
  const dim3 grid((uint32_t)(want < 1024 ? want : 1024), (uint32_t)G);   // grid-x: dgs_view_loss_grad's, a function of E only
  if (tone_mapping == DGS_TONE_GAMMA)
    hipLaunchKernelGGL(view_loss_rows_kernel<1>, grid, dim3(256), 0, s, x, gt, (int)row_begin, E, eps, bound, upstream, dL_dx, work);
  else
    hipLaunchKernelGGL(view_loss_rows_kernel<0>, grid, dim3(256), 0, s, x, gt, (int)row_begin, E, eps, bound, upstream, dL_dx, work);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "view_loss_grad_rows");
}

int dgs_l2_ema_epoch(const float* work, const int32_t* pos, int32_t n, const uint32_t* const* skip_flags,
                     const int32_t* group_begin, int32_t n_groups, float* l2_ema, dgs_stream_t stream) {
  if (work == nullptr || pos == nullptr || l2_ema == nullptr) return dgs_fail_arg("l2_ema_epoch: null pointer");
  if (n < 1 || n > DGS_MAX_K) return dgs_fail_arg("l2_ema_epoch: n must be in 1..DGS_MAX_K");
  if (n_groups < 0 || n_groups > n || (n_groups > 0 && (skip_flags == nullptr || group_begin == nullptr)))
    return dgs_fail_arg("l2_ema_epoch: 0..n groups, with their skip words and row ranges");
  EmaGroups g;
  memset(&g, 0, sizeof(g));
  g.n_groups = n_groups > 0 ? n_groups : 1;       // no groups: one group of all rows that is never skipped
  g.begin[1] = n;
  for (int i = 0; i < n_groups; i++) {
    if (group_begin[i] < 0 || group_begin[i + 1] <= group_begin[i] || group_begin[i + 1] > n)
      return dgs_fail_arg("l2_ema_epoch: group_begin must rise from 0 to n");
    g.skip[i] = skip_flags[i];
    g.begin[i] = group_begin[i];
    g.begin[i + 1] = group_begin[i + 1];
  }
  if (n_groups > 0 && (group_begin[0] != 0 || group_begin[n_groups] != n))
    return dgs_fail_arg("l2_ema_epoch: group_begin must rise from 0 to n");
  hipLaunchKernelGGL(l2_ema_epoch_kernel, dim3(1), dim3(DGS_MAX_K), 0, reinterpret_cast<hipStream_t>(stream), work, pos,
                     (int)n, g, l2_ema);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "l2_ema_epoch");
}

size_t dgs_image_metrics_tmp_bytes(int32_t W, int32_t H) {
  if (W < 1 || H < 1) return 0;
  return (size_t)3 * ((W + MT - 1) / MT) * ((H + MT - 1) / MT) * 2 * sizeof(double);
}

int dgs_image_metrics(const float* a, const float* b, int32_t W, int32_t H, void* tmp, float* out, dgs_stream_t stream) {
  if (a == nullptr || b == nullptr || tmp == nullptr || out == nullptr || W < 1 || H < 1)
    return dgs_fail_arg("image_metrics: null pointer or empty image");
  const int gx = (W + MT - 1) / MT, gy = (H + MT - 1) / MT;
  if (gy > 65535) return dgs_fail_arg("image_metrics: image too tall");
  // the window of utils/loss_utils.py:23-25 with its roundings: fp32 samples of exp(-(x - 5)^2 / (2 sigma^2)), their fp32
  // sum, an fp32 division
  SsimWindow win;
  float sum = 0.0f;
  for (int i = 0; i < 2 * MR + 1; i++) {
    win.w[i] = (float)exp(-(double)((i - MR) * (i - MR)) / (2.0 * 1.5 * 1.5));
    sum += win.w[i];
  }
  for (int i = 0; i < 2 * MR + 1; i++) win.w[i] = win.w[i] / sum;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* partials = reinterpret_cast<double*>(tmp);
  hipLaunchKernelGGL(metrics_tile_kernel, dim3(gx, gy, 3), dim3(256), 0, s, a, b, (int)H, (int)W, win, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "image_metrics");
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3(1), dim3(256), 0, s, partials, gx * gy, 3, (double)W * (double)H, out);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "image_metrics");
}

}  // extern "C"

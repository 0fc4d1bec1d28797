// loss.hip -- the image-space kernels of a training step: the fused blur loss (blur image, both loss values and
// dL/dsubframes in one pass; whole view and one rank's slice of a subframe-sharded view) and the densification statistics.
// Built with FMA contraction (no extra flags in deblurgs_amd/build.py): densify_stats_kernel's gx*gx + gy*gy rounds once.
#include "dgs_common.h"

namespace {

// ------------------------------------------------------------------------------------------- fused blur loss (f1)
// train.py:143-165 with utils/loss_utils.py:17-18 (l1_loss) and :80-93 (batchwise_smoothness_loss):
//   blur = mean_k sub_k;  L = mean|blur - gt| + lambda_t * mean|sub_{k+1} - sub_k|
//   dL/dsub_k = sign(blur-gt)/(E*K) + lambda_t * [sign(sub_k - sub_{k-1}) - sign(sub_{k+1} - sub_k)] / (E*(K-1))
// with E = C*H*W.  One thread per (channel, pixel) element; replaces ~20 elementwise launches and ~1.5 GB of
// traffic between the fused forward and backward.

// The end of every blur-loss kernel: the block's two sums in a fixed order (lane order by DPP, then the four waves in
// index order), published as deterministic totals (dgs_totals_publish); the last block to arrive converts them.
// losses is an 8-word work area zeroed by the launcher: [0] L1, [1] smoothness, [2..7] the totals' own words.
__device__ __forceinline__ void loss_block_totals(float l1, float sm, float* __restrict__ losses, size_t E, int K) {
  __shared__ float red[2][4];
  l1 = dgs_wave_sum63(l1);
  sm = dgs_wave_sum63(sm);
  const int lane = dgs_lane(), w = threadIdx.x >> 6;
  if (lane == 63) {
    red[0][w] = l1;
    red[1][w] = sm;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const float c = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  unsigned long long t0, t1;
  bool bad;
  if (dgs_totals_publish(a, c, losses, t0, t1, bad)) {
    const float nanv = __int_as_float(0x7fc00000);
    losses[0] = bad ? nanv : (float)(((double)t0 / DGS_TOTALS_FX) / (double)E);
    losses[1] = bad ? nanv : ((K > 1) ? (float)(((double)t1 / DGS_TOTALS_FX) / ((double)E * (double)(K - 1))) : 0.0f);
  }
}

// MODE 0: blur + loss values (forward).  MODE 1: dL/dsubframes, multiplied by the upstream scalar *scale read
// from device memory (backward; no host sync, no extra elementwise pass over [K,3,H,W]).  MODE 2: both at once.
template <int MODE, int V>  // V = elements per thread (4 -> 16-byte loads/stores when E % 4 == 0, else 1)
__global__ void __launch_bounds__(256)
blur_loss_kernel(const float* __restrict__ sub, const float* __restrict__ gt, int K, size_t E, float lambda_t,
                 const float* __restrict__ lambda_dev, const float* __restrict__ scale, float* __restrict__ blur,
                 float* __restrict__ dsub, float* __restrict__ losses) {
  if (lambda_dev != nullptr) lambda_t = lambda_dev[0];   // graph replay: the scheduled weight lives in device memory
  typedef float vec __attribute__((ext_vector_type(V)));
  float l1 = 0.0f, sm = 0.0f;
  // grid-stride loop: the launcher caps the grid (the loss totals cost three same-address atomics per block)
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; e < E; e += (size_t)gridDim.x * 256 * V) {
    auto ld = [](const float* p) { return *reinterpret_cast<const vec*>(p); };
    if (MODE == 0) {
      // forward: ONE pass over the K subframes (sum for the blur and the adjacent differences together), unrolled so
      // that several 16-byte loads per lane are in flight
      vec prev = ld(sub + e);
      vec acc = prev;
#pragma unroll 4
      for (int k = 1; k < K; k++) {
        const vec nxt = ld(sub + (size_t)k * E + e);
        const vec dd = nxt - prev;
        acc += nxt;
#pragma unroll
        for (int i = 0; i < V; i++) sm += fabsf(dd[i]);
        prev = nxt;
      }
      const vec b = acc / (float)K;
      *reinterpret_cast<vec*>(blur + e) = b;
      const vec d = b - ld(gt + e);
#pragma unroll
      for (int i = 0; i < V; i++) l1 += fabsf(d[i]);
    } else {
      vec b;
      if (MODE == 1 && blur != nullptr) {
        b = ld(blur + e);   // backward: the forward's blur is handed back in, no second summation
      } else {
        vec acc = ld(sub + e);
#pragma unroll 4
        for (int k = 1; k < K; k++) acc += ld(sub + (size_t)k * E + e);
        b = acc / (float)K;
        if (MODE == 2) *reinterpret_cast<vec*>(blur + e) = b;
      }
      const vec d = b - ld(gt + e);
      const float up = (scale != nullptr) ? scale[0] : 1.0f;
      const float c_l1 = up / ((float)E * (float)K);
      const float ws = (K > 1) ? up * lambda_t / ((float)E * (float)(K - 1)) : 0.0f;
      vec g_l1;
#pragma unroll
      for (int i = 0; i < V; i++) {
        l1 += fabsf(d[i]);
        g_l1[i] = c_l1 * dgs_sgn(d[i]);
      }
      vec prev = ld(sub + e);
      vec s_prev = (vec)(0.0f);  // sign(x_k - x_{k-1})
#pragma unroll 4
      for (int k = 0; k < K; k++) {
        vec s_next = (vec)(0.0f);
        vec nxt = prev;
        if (k + 1 < K) {
          nxt = ld(sub + (size_t)(k + 1) * E + e);
          const vec dd = nxt - prev;
#pragma unroll
          for (int i = 0; i < V; i++) {
            sm += fabsf(dd[i]);
            s_next[i] = dgs_sgn(dd[i]);
          }
        }
        *reinterpret_cast<vec*>(dsub + (size_t)k * E + e) = g_l1 + ws * (s_prev - s_next);
        s_prev = s_next;
        prev = nxt;
      }
    }
  }
  if (MODE == 1) return;
  loss_block_totals(l1, sm, losses, E, K);
}

// Forward + backward at once (MODE 2's results, bit for bit) for K <= KMAX with the K subframe values of an element
// held in registers: every subframe value is read ONCE (MODE 2 streams the subframes twice: 1.1 GB instead of 0.77 GB
// at the metric configuration).
template <int KMAX, int V>
__global__ void __launch_bounds__(256)
blur_loss_all_kernel(const float* __restrict__ sub, const float* __restrict__ gt, int K, size_t E, float lambda_t,
                     const float* __restrict__ lambda_dev, const float* __restrict__ scale, float* __restrict__ blur,
                     float* __restrict__ dsub, float* __restrict__ losses) {
  if (lambda_dev != nullptr) lambda_t = lambda_dev[0];
  typedef float vec __attribute__((ext_vector_type(V)));
  float l1 = 0.0f, sm = 0.0f;
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; e < E; e += (size_t)gridDim.x * 256 * V) {
    vec x[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++)
      if (k < K) x[k] = *reinterpret_cast<const vec*>(sub + (size_t)k * E + e);
    vec acc = x[0];
#pragma unroll
    for (int k = 1; k < KMAX; k++)
      if (k < K) acc += x[k];
    const vec b = acc / (float)K;
    *reinterpret_cast<vec*>(blur + e) = b;
    const vec d = b - *reinterpret_cast<const vec*>(gt + e);
    const float up = (scale != nullptr) ? scale[0] : 1.0f;
    const float c_l1 = up / ((float)E * (float)K);
    const float ws = (K > 1) ? up * lambda_t / ((float)E * (float)(K - 1)) : 0.0f;
    vec g_l1;
#pragma unroll
    for (int i = 0; i < V; i++) {
      l1 += fabsf(d[i]);
      g_l1[i] = c_l1 * dgs_sgn(d[i]);
    }
    vec s_prev = (vec)(0.0f);
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      if (k < K) {
        vec s_next = (vec)(0.0f);
        if (k + 1 < K) {
          const vec dd = x[k + 1 < KMAX ? k + 1 : k] - x[k];
#pragma unroll
          for (int i = 0; i < V; i++) {
            sm += fabsf(dd[i]);
            s_next[i] = dgs_sgn(dd[i]);
          }
        }
        *reinterpret_cast<vec*>(dsub + (size_t)k * E + e) = g_l1 + ws * (s_prev - s_next);
        s_prev = s_next;
      }
    }
  }
  loss_block_totals(l1, sm, losses, E, K);
}

// The loss block of ONE RANK of a subframe-sharded view (deblurgs_amd/sharding.py; new work: the reference is
// single-GPU).  The rank holds Kl consecutive subframes of the view's K; `blur` is the view's blur image (mean over all K
// subframes: the ranks' partial sums were all-reduced), prev / next the neighbouring ranks' boundary subframes (NULL at
// the ends of the view).  Same arithmetic as blur_loss_all_kernel for the subframes held here:
//   dL/dsub_k = sign(blur - gt) / (E K) + lambda_t [sign(sub_k - sub_{k-1}) - sign(sub_{k+1} - sub_k)] / (E (K - 1)),
// losses[0] = mean |blur - gt| (the same on every rank), losses[1] = this rank's share of the smoothness value: the
// differences whose LEFT frame it holds, / (E (K - 1)) -- the caller sums the shares over the ranks.
template <int KMAX, int V>
__global__ void __launch_bounds__(256)
blur_loss_slice_kernel(const float* __restrict__ sub, const float* __restrict__ prev, const float* __restrict__ next,
                       const float* __restrict__ blur, const float* __restrict__ gt, int Kl, int K, size_t E,
                       float lambda_t, float* __restrict__ dsub, float* __restrict__ losses) {
  typedef float vec __attribute__((ext_vector_type(V)));
  float l1 = 0.0f, sm = 0.0f;
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; e < E; e += (size_t)gridDim.x * 256 * V) {
    vec x[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++)
      if (k < Kl) x[k] = *reinterpret_cast<const vec*>(sub + (size_t)k * E + e);
    const vec d = *reinterpret_cast<const vec*>(blur + e) - *reinterpret_cast<const vec*>(gt + e);
    const float c_l1 = 1.0f / ((float)E * (float)K);
    const float ws = (K > 1) ? lambda_t / ((float)E * (float)(K - 1)) : 0.0f;
    vec g_l1;
#pragma unroll
    for (int i = 0; i < V; i++) {
      l1 += fabsf(d[i]);
      g_l1[i] = c_l1 * dgs_sgn(d[i]);
    }
    vec s_prev = (vec)(0.0f);
    if (prev != nullptr) {   // the difference across the lower rank boundary belongs to the rank below: sign only
      const vec dd = x[0] - *reinterpret_cast<const vec*>(prev + e);
#pragma unroll
      for (int i = 0; i < V; i++) s_prev[i] = dgs_sgn(dd[i]);
    }
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      if (k < Kl) {
        vec s_next = (vec)(0.0f);
        const bool inner = k + 1 < Kl;
        if (inner || next != nullptr) {
          const vec nx = inner ? x[k + 1 < KMAX ? k + 1 : k] : *reinterpret_cast<const vec*>(next + e);
          const vec dd = nx - x[k];
#pragma unroll
          for (int i = 0; i < V; i++) {
            sm += fabsf(dd[i]);
            s_next[i] = dgs_sgn(dd[i]);
          }
        }
        *reinterpret_cast<vec*>(dsub + (size_t)k * E + e) = g_l1 + ws * (s_prev - s_next);
        s_prev = s_next;
      }
    }
  }
  loss_block_totals(l1, sm, losses, E, K);
}

// train.py:188-193 + scene/gaussian_model.py:456-458 for the K subframes of one step, in subframe order
__global__ void __launch_bounds__(256)
densify_stats_kernel(const float* __restrict__ vgrad, const int32_t* __restrict__ radii, int K, int K_total, int P,
                     float* __restrict__ max_radii2D, float* __restrict__ accum, float* __restrict__ denom,
                     const uint32_t* __restrict__ skip) {
  if (skip != nullptr && skip[0] != 0u) return;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  float mr = max_radii2D[g], ac = accum[g], dn = denom[g];
  const float inc = (float)(1.0 / (double)K_total);
  for (int k = 0; k < K; k++) {
    const size_t o = (size_t)k * P + g;
    const int r = radii[o];
    if (r > 0) {
      mr = fmaxf(mr, (float)r);
      const float gx = vgrad[3 * o], gy = vgrad[3 * o + 1];
      ac += sqrtf(gx * gx + gy * gy);
      dn += inc;
    }
  }
  max_radii2D[g] = mr;
  accum[g] = ac;
  denom[g] = dn;
}

// The launch shape of a blur-loss kernel: the 16-byte path when E % 4 == 0 and every pointer (or-ed into `pointers`)
// is 16-byte aligned, else one element per thread; at most DGS_LOSS_BLOCKS blocks (2 per CU; every thread keeps K
// 16-byte loads in flight): enough to saturate HBM, few enough that the per-block same-address atomics of the loss
// totals (~58 ns per block: 0.35 ms with 6075 blocks at 1080p, still 0.11 ms of the 800x800 case's kernel with 1875)
// disappear.  Measured 2048 / 1024 / 512 blocks: 1.204 / 1.157 / 1.144 ms per cfg2 step, 11.99 / 12.01 / 11.91 ms at
// the metric config.  The totals depend on the grid, which is a function of E only -- still bitwise reproducible
#ifndef DGS_LOSS_BLOCKS
#define DGS_LOSS_BLOCKS 512
#endif
struct LossShape {
  bool v4;
  dim3 grid;
};
LossShape loss_shape(size_t E, uintptr_t pointers) {
  LossShape sh;
  sh.v4 = (E % 4 == 0) && (pointers % 16 == 0);
  const size_t want = (E / (sh.v4 ? 4 : 1) + 255) / 256;
  sh.grid = dim3((uint32_t)(want < DGS_LOSS_BLOCKS ? (want == 0 ? 1 : want) : DGS_LOSS_BLOCKS));
  return sh;
}
uintptr_t bits(const void* p) { return reinterpret_cast<uintptr_t>(p); }

hipError_t launch_blur_loss(const float* sub, const float* gt, int K, int C, int HW, float lambda_t,
                            const float* lambda_dev, const float* scale, float* blur, float* dsub, float* losses,
                            hipStream_t s) {
  const size_t E = (size_t)C * HW;
  if (losses != nullptr) {
    hipError_t e = dgs_launch_clear_words(reinterpret_cast<uint32_t*>(losses), 8, s);   // results + accumulators + arrival counter
    if (e != hipSuccess) return e;
  }
  const LossShape sh = loss_shape(E, bits(sub) | bits(gt) | bits(blur) | bits(dsub));
#define DGS_BL(MODE)                                                                                              \
  do {                                                                                                            \
    if (sh.v4)                                                                                                       \
      hipLaunchKernelGGL((blur_loss_kernel<MODE, 4>), sh.grid, dim3(256), 0, s, sub, gt, K, E, lambda_t, lambda_dev, scale, blur, \
                         dsub, losses);                                                                           \
    else                                                                                                          \
      hipLaunchKernelGGL((blur_loss_kernel<MODE, 1>), sh.grid, dim3(256), 0, s, sub, gt, K, E, lambda_t, lambda_dev, scale, blur, \
                         dsub, losses);                                                                           \
  } while (0)
  if (dsub == nullptr)
    DGS_BL(0);
  else if (losses == nullptr)
    DGS_BL(1);
  else if (sh.v4 && K <= 16)
    hipLaunchKernelGGL((blur_loss_all_kernel<16, 4>), sh.grid, dim3(256), 0, s, sub, gt, K, E, lambda_t, lambda_dev, scale, blur, dsub,
                       losses);
  else if (sh.v4 && K <= 32)
    hipLaunchKernelGGL((blur_loss_all_kernel<32, 2>), sh.grid, dim3(256), 0, s, sub, gt, K, E, lambda_t, lambda_dev, scale, blur, dsub,
                       losses);
  else
    DGS_BL(2);
#undef DGS_BL
  return hipGetLastError();
}

int blur_loss_impl(const float* subframes, const float* gt, int32_t K, int32_t C, int32_t HW, float lambda_t,
                   const float* lambda_dev, const float* upstream, float* blur, float* dL_dsubframes, float* losses,
                   dgs_stream_t stream) {
  const bool fwd = (blur != nullptr && losses != nullptr);
  // losses given: blur is an output (forward, or forward + backward when dL_dsubframes is given too);
  // losses NULL: backward only, blur (optional) is the forward's blur handed back in
  if (subframes == nullptr || gt == nullptr || K < 1 || C < 1 || HW < 1 || (!fwd && dL_dsubframes == nullptr) ||
      (losses != nullptr && blur == nullptr))
    return dgs_fail_arg("blur_loss_grad: bad argument");
  hipError_t e = launch_blur_loss(subframes, gt, K, C, HW, lambda_t, lambda_dev, upstream, blur, dL_dsubframes, losses,
                                  reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "blur_loss_grad");
}

}  // namespace

extern "C" {

int dgs_blur_loss_grad(const float* subframes, const float* gt, int32_t K, int32_t C, int32_t HW, float lambda_t,
                       const float* upstream, float* blur, float* dL_dsubframes, float* losses, dgs_stream_t stream) {
  return blur_loss_impl(subframes, gt, K, C, HW, lambda_t, nullptr, upstream, blur, dL_dsubframes, losses, stream);
}
int dgs_blur_loss_grad_dev(const float* subframes, const float* gt, int32_t K, int32_t C, int32_t HW,
                           const float* lambda_t_dev, const float* upstream, float* blur, float* dL_dsubframes,
                           float* losses, dgs_stream_t stream) {
  if (lambda_t_dev == nullptr) return dgs_fail_arg("blur_loss_grad_dev: lambda_t_dev is null");
  return blur_loss_impl(subframes, gt, K, C, HW, 0.0f, lambda_t_dev, upstream, blur, dL_dsubframes, losses, stream);
}

int dgs_blur_loss_slice_grad(const float* subframes, const float* prev_last, const float* next_first, const float* blur,
                             const float* gt, int32_t K_local, int32_t K_total, int32_t C, int32_t HW, float lambda_t,
                             float* dL_dsubframes, float* losses, dgs_stream_t stream) {
  if (subframes == nullptr || blur == nullptr || gt == nullptr || dL_dsubframes == nullptr || losses == nullptr ||
      K_local < 1 || K_total < K_local || K_local > 32 || C < 1 || HW < 1)
    return dgs_fail_arg("blur_loss_slice_grad: bad argument (1 <= K_local <= 32, K_local <= K_total)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t E = (size_t)C * HW;
  hipError_t e = dgs_launch_clear_words(reinterpret_cast<uint32_t*>(losses), 8, s);
  if (e != hipSuccess) return dgs_fail_hip(e, "blur_loss_slice_grad");
  const LossShape sh = loss_shape(E, bits(subframes) | bits(blur) | bits(gt) | bits(dL_dsubframes) | bits(prev_last) |
                                         bits(next_first));
#define DGS_BLS(KMAX, V)                                                                                              \
  hipLaunchKernelGGL((blur_loss_slice_kernel<KMAX, V>), sh.grid, dim3(256), 0, s, subframes, prev_last, next_first, blur, gt, \
                     K_local, K_total, E, lambda_t, dL_dsubframes, losses)
  if (sh.v4) {
    if (K_local <= 4) DGS_BLS(4, 4); else if (K_local <= 16) DGS_BLS(16, 4); else DGS_BLS(32, 2);
  } else {
    if (K_local <= 4) DGS_BLS(4, 1); else if (K_local <= 16) DGS_BLS(16, 1); else DGS_BLS(32, 1);
  }
#undef DGS_BLS
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "blur_loss_slice_grad");
}

int dgs_densify_stats(const float* viewspace_grad, const int32_t* radii, int32_t K, int32_t K_total, int32_t P,
                      float* max_radii2D, float* xyz_gradient_accum, float* denom, const uint32_t* skip_flag,
                      dgs_stream_t stream) {
  if (K_total <= 0) K_total = K;
  if (K < 1 || K_total < K || P < 0 || (P > 0 && (viewspace_grad == nullptr || radii == nullptr || max_radii2D == nullptr ||
                                   xyz_gradient_accum == nullptr || denom == nullptr)))
    return dgs_fail_arg("densify_stats: bad argument");
  if (P == 0) return DGS_OK;
  hipLaunchKernelGGL(densify_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     viewspace_grad, radii, K, K_total, P, max_radii2D, xyz_gradient_accum, denom, skip_flag);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "densify_stats");
}

}  // extern "C"

// report.hip -- what the reference's drivers make on the host to LOOK at a result (test.py:122-126,
// utils/visualization.py:262-291, utils/colorize.py:63-107), on the device:
//   * dgs_order_stats / dgs_percentiles: exact order statistics of n floats by radix select -- four most-significant-first
//     8-bit passes over an order-preserving 32-bit key, one data pass for all ranks -- where the reference sorts
//     (np.percentile, torch.sort); numpy's linear percentile formed from the two selected neighbours in float64;
//   * dgs_report_images: the rounded 8-bit render(s), the 8-bit ground truth and the L1 error map of a view in one pass
//     (the sequential fp32 mean of the K subframes when the blurred image is asked for);
//   * dgs_scalar_colorize: colorize_np once its range is known -- two float64 device words -- through a 256-entry table.
// Built with -ffp-contract=off (deblurgs_amd/build.py): every statement rounds once, as the torch / numpy expression it
// restates does.  Plain loads and stores, LDS integer atomics for the block histograms; no global atomics, no float
// atomics, nothing kept between calls, no device word read by the host.
#include <math.h>
#include <stdio.h>

#include "dgs_common.h"

namespace {

// ------------------------------------------------------------------------------------------- radix select
constexpr int OS_THREADS = 256;
constexpr int OS_MAX_RANKS = 8;              // 4 order statistics, or the 2 x 4 neighbours of 4 percentiles
constexpr uint32_t OS_MAX_BLOCKS = 2048;
constexpr uint64_t OS_BLOCK_ELEMS = 8192;    // elements a block takes before the grid stops growing with n: keeps the
                                             // table the one-block pick kernel sums short (254 blocks at 1920 x 1080)
constexpr size_t OS_HIST_OFFSET = 256;       // bytes of tmp in front of the block histograms (OsState)
constexpr int OS_PICK_THREADS = 1024;        // 256 digits x 4 slices of the blocks

struct OsState {                 // device words at the start of tmp, written by the pick kernel only
  uint32_t prefix[OS_MAX_RANKS]; // the key bits fixed so far (lower bits 0); after the last pass: the key
  uint32_t rank[OS_MAX_RANKS];   // the rank among the elements that share the prefix
};
struct OsRanks {
  uint32_t r[OS_MAX_RANKS];
};
struct OsFinish {                // what the last pick does with the keys
  float* out32;                  // order statistics: m floats (or null)
  double* out64;                 // percentiles: mq doubles (or null) from the rank pairs (2 t, 2 t + 1)
  int mq;
  double g[4];
};

__host__ __device__ inline uint32_t os_blocks(uint64_t n) {
  const uint64_t want = (n + OS_BLOCK_ELEMS - 1) / OS_BLOCK_ELEMS;
  return (uint32_t)(want < 1 ? 1 : (want < (uint64_t)OS_MAX_BLOCKS ? want : (uint64_t)OS_MAX_BLOCKS));
}

// order-preserving key: negative floats reversed below the positive ones, every NaN last
__device__ __forceinline__ uint32_t os_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float os_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);      // (0xFFFFFFFF -> 0x7FFFFFFF, a quiet NaN)
}

// One count per valid lane into h[d], aggregated per wave first: lanes that share a digit elect their lowest lane, which
// adds the group's size -- an all-equal input (every lane in one bin) costs one LDS atomic per wave, not 64 on one word.
// The common cases leave early: no valid lane; all valid lanes on one digit (as the depth order's histogram in
// binning.hip tests it); otherwise the groups are matched digit bit by digit bit (binning.hip's ranking).
// Called in wave-uniform control flow only.
__device__ __forceinline__ void os_count(uint32_t* __restrict__ h, uint32_t d, bool valid, int lane) {
  const uint64_t vm = __ballot(valid);
  if (vm == 0ull) return;
  const int first = __builtin_ctzll(vm);
  const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, first);
  if (__ballot(valid && d != d0) == 0ull) {
    if (lane == first) atomicAdd(&h[d0], (uint32_t)__builtin_popcountll(vm));
    return;
  }
  uint64_t peers = vm;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = ((d >> b) & 1u) != 0u;
    const uint64_t m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  if (valid && lane == __builtin_ctzll(peers)) atomicAdd(&h[d], (uint32_t)__builtin_popcountll(peers));
}

// Pass `pass` (0 = the top 8 bits): per block the histogram [m_eff][256] of digit (key >> shift) & 255 over the elements
// whose bits above the digit equal rank j's prefix, written to hist[block][j][256] with plain stores.  Pass 0 has no prefix
// yet: one histogram (m_eff = 1) serves every rank.  x + head is 16-byte aligned and holds nvec float4; the head elements
// in front and the n - head - 4 nvec behind it (at most 3 each) are block 0's, by scalar loads.
__global__ void __launch_bounds__(OS_THREADS)
os_hist_kernel(const float* __restrict__ x, uint64_t n, uint32_t head, uint64_t nvec, const OsState* __restrict__ state,
               int pass, int m_eff, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[OS_MAX_RANKS * 256];
  __shared__ uint32_t s_pre[OS_MAX_RANKS];
  const int t = (int)threadIdx.x, lane = dgs_lane();
  for (int i = t; i < m_eff * 256; i += OS_THREADS) h[i] = 0u;
  if (t < m_eff) s_pre[t] = pass > 0 ? state->prefix[t] : 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
  // (the loop bound is the same for every lane of a wave: os_count holds ballots)
  for (uint64_t base = (uint64_t)blockIdx.x * OS_THREADS; base < nvec; base += (uint64_t)gridDim.x * OS_THREADS) {
    const uint64_t idx = base + (uint64_t)t;
    const bool ok = idx < nvec;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ok) q = xv[idx];
    const uint32_t key[4] = {os_key(q.x), os_key(q.y), os_key(q.z), os_key(q.w)};
    for (int j = 0; j < m_eff; j++) {
      const uint32_t pre = s_pre[j];
#pragma unroll
      for (int e = 0; e < 4; e++)
        os_count(h + j * 256, (key[e] >> shift) & 255u, ok && ((key[e] ^ pre) & hi_mask) == 0u, lane);
    }
  }
  if (blockIdx.x == 0 && t < DGS_WAVE) {
    const uint64_t body_end = (uint64_t)head + 4ull * nvec;
    const uint32_t ends = head + (uint32_t)(n - body_end);        // at most 6
    const bool ok = (uint32_t)t < ends;
    const uint64_t e = (uint32_t)t < head ? (uint64_t)t : body_end + (uint64_t)((uint32_t)t - head);
    const uint32_t key = ok ? os_key(x[e]) : 0u;
    for (int j = 0; j < m_eff; j++)
      os_count(h + j * 256, (key >> shift) & 255u, ok && ((key ^ s_pre[j]) & hi_mask) == 0u, lane);
  }
  __syncthreads();
  uint32_t* __restrict__ dst = hist + (size_t)blockIdx.x * (size_t)m_eff * 256;
  for (int i = t; i < m_eff * 256; i += OS_THREADS) dst[i] = h[i];
}

// One block: per histogram the sum over the blocks (integer sums, slice by slice in block order), an inclusive scan of
// the 256 counts, and per rank the digit whose run holds it -- the new prefix and the rank inside that run go to the
// device words of `state`.  After pass 3 the prefixes are the keys: the floats (order statistics) or numpy's linear
// interpolation of the rank pairs (percentiles) leave.
__global__ void __launch_bounds__(OS_PICK_THREADS)
os_pick_kernel(const uint32_t* __restrict__ hist, uint32_t nb, OsState* __restrict__ state, OsRanks ranks, int pass, int m,
               OsFinish fin) {
  __shared__ uint32_t part[4][256];
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t scan[2][256];
  __shared__ uint32_t s_pre[OS_MAX_RANKS], s_rank[OS_MAX_RANKS], s_key[OS_MAX_RANKS];
  const int t = (int)threadIdx.x, slice = t >> 8, d = t & 255;
  const int m_eff = pass == 0 ? 1 : m;
  const int shift = 24 - 8 * pass;
  if (t < m) {
    s_pre[t] = pass == 0 ? 0u : state->prefix[t];
    s_rank[t] = pass == 0 ? ranks.r[t] : state->rank[t];
  }
  __syncthreads();      // (every read of `state` is done before anything below writes it)
  for (int jh = 0; jh < m_eff; jh++) {
    uint32_t sum = 0u;
    for (uint32_t b = (uint32_t)slice; b < nb; b += 4u) sum += hist[((size_t)b * (size_t)m_eff + (size_t)jh) * 256 + (size_t)d];
    part[slice][d] = sum;
    __syncthreads();
    if (t < 256) {
      const uint32_t c = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
      cnt[t] = c;
      scan[0][t] = c;
    }
    __syncthreads();
    int src = 0;
    for (int off = 1; off < 256; off <<= 1) {
      if (t < 256) scan[src ^ 1][t] = scan[src][t] + (t >= off ? scan[src][t - off] : 0u);
      __syncthreads();
      src ^= 1;
    }
    if (t < 256) {
      const uint32_t c = cnt[t], incl = scan[src][t], excl = incl - c;
      const int j0 = pass == 0 ? 0 : jh, j1 = pass == 0 ? m : jh + 1;
      for (int j = j0; j < j1; j++) {
        const uint32_t r = s_rank[j];
        if (c > 0u && r >= excl && r - excl < c) {       // exactly one digit: the ranks are below the counts' total
          const uint32_t pre = s_pre[j] | ((uint32_t)t << shift);
          state->prefix[j] = pre;
          state->rank[j] = r - excl;
          s_key[j] = pre;
        }
      }
    }
    __syncthreads();
  }
  if (pass != 3) return;
  if (fin.out32 != nullptr && t < m) fin.out32[t] = os_unkey(s_key[t]);
  if (fin.out64 != nullptr && t < fin.mq) {
    // numpy's _lerp on two float32 neighbours and a float64 weight: the difference is formed in float32, the rest in
    // float64; the second form where the weight is at least a half
    const float a = os_unkey(s_key[2 * t]), b = os_unkey(s_key[2 * t + 1]);
    const float diff = b - a;
    const double g = fin.g[t];
    const double up = (double)diff * g;
    double r = (double)a + up;
    if (g >= 0.5) {
      const double down = (double)diff * (1.0 - g);
      r = (double)b - down;
    }
    fin.out64[t] = r;
  }
}

// the four passes of a select of m ranks (validated by the caller); the keys end in tmp's state words
int os_select(const float* x, uint64_t n, const OsRanks& ranks, int m, void* tmp, const OsFinish& fin, hipStream_t s,
              const char* what) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
  uint64_t head = ((16u - (uint32_t)(addr & 15u)) & 15u) / 4u;
  if (head > n) head = n;
  const uint64_t nvec = (n - head) / 4;
  const uint32_t nb = os_blocks(n);
  OsState* state = reinterpret_cast<OsState*>(tmp);
  uint32_t* hist = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(tmp) + OS_HIST_OFFSET);
  OsFinish none = {};
  for (int pass = 0; pass < 4; pass++) {
    hipLaunchKernelGGL(os_hist_kernel, dim3(nb), dim3(OS_THREADS), 0, s, x, n, (uint32_t)head, nvec,
                       (const OsState*)state, pass, pass == 0 ? 1 : m, hist);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dgs_fail_hip(e, what);
    hipLaunchKernelGGL(os_pick_kernel, dim3(1), dim3(OS_PICK_THREADS), 0, s, (const uint32_t*)hist, nb, state, ranks, pass,
                       m, pass == 3 ? fin : none);
    e = hipGetLastError();
    if (e != hipSuccess) return dgs_fail_hip(e, what);
  }
  return DGS_OK;
}

// ------------------------------------------------------------------------------------------- report images
// four consecutive floats (one 16-byte load where the address allows, scalar loads otherwise and for a row's last quad)
__device__ __forceinline__ void load4(const float* __restrict__ s, int nv, float v[4]) {
  if (nv == 4 && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(s);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = i < nv ? s[i] : 0.0f;
  }
}
// four pixels' interleaved bytes (three dword stores where the address allows, byte stores otherwise)
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ dst, int nv, const uint32_t lv[3][4]) {
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

// tone_map as frame_level (frames.hip) and view_loss_image (metrics.hip) evaluate it -- same expression, same powf; a NaN
// input stays NaN, as torch's clamp_min passes it on (fmaxf alone would make it eps)
template <int GAMMA>
__device__ __forceinline__ float report_tone(float xv, float eps, float bound, float inv_span, float ex) {
  if (!GAMMA) return xv;
  const float u = (xv - bound) / inv_span;
  const float uc = fmaxf(u, eps);
  const float y = powf(uc, ex);
  return (xv != xv) ? xv : y;
}
// torchvision's save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two roundings, then truncation.  fmaxf drops a
// NaN operand: a NaN gives 0.
__device__ __forceinline__ uint32_t report_level(float y) {
  const float a = y * 255.0f;
  const float b = a + 0.5f;
  return (uint32_t)fminf(fmaxf(b, 0.0f), 255.0f);
}

// Thread t: pixels [4 t, 4 t + 4) of the flattened H W plane of output image g = blockIdx.y.  mean: the K subframes are
// added in order, then divided by (float)K; else image g is subframe g.
template <int GAMMA>
__global__ void __launch_bounds__(256)
report_images_kernel(const float* __restrict__ x, int K, int mean, size_t plane, float eps, float bound,
                     const float* __restrict__ gt, uint8_t* __restrict__ out_u8, uint8_t* __restrict__ gt_u8,
                     float* __restrict__ err) {
  const size_t quad = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (quad >= (plane + 3) / 4) return;
  const size_t p0 = 4 * quad;
  const int nv = (plane - p0 < 4) ? (int)(plane - p0) : 4;
  const int g = (int)blockIdx.y;
  const int k0 = mean ? 0 : g, kn = mean ? K : 1;
  const float inv_span = 1.0f - 2.0f * bound;
  const float ex = (float)(1.0 / 2.2);
  const float fK = (float)K;
  uint32_t lv[3][4], glv[3][4];
  float ad[3][4];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float acc[4];
    load4(x + ((size_t)k0 * 3 + (size_t)c) * plane + p0, nv, acc);
    for (int k = 1; k < kn; k++) {
      float v[4];
      load4(x + ((size_t)(k0 + k) * 3 + (size_t)c) * plane + p0, nv, v);
#pragma unroll
      for (int i = 0; i < 4; i++) acc[i] = acc[i] + v[i];
    }
    float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (gt != nullptr) load4(gt + ((size_t)g * 3 + (size_t)c) * plane + p0, nv, gv);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float s = mean ? acc[i] / fK : acc[i];
      const float y = report_tone<GAMMA>(s, eps, bound, inv_span, ex);
      lv[c][i] = report_level(y);
      glv[c][i] = report_level(gv[i]);
      ad[c][i] = fabsf(gv[i] - y);
    }
  }
  store_rgb4(out_u8 + ((size_t)g * plane + p0) * 3, nv, lv);
  if (gt_u8 != nullptr) store_rgb4(gt_u8 + ((size_t)g * plane + p0) * 3, nv, glv);
  if (err != nullptr) {
    float e4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) e4[i] = ((ad[0][i] + ad[1][i]) + ad[2][i]) / 3.0f;
    float* d = err + (size_t)g * plane + p0;
    if (nv == 4 && (reinterpret_cast<uintptr_t>(d) & 15u) == 0) {
      *reinterpret_cast<float4*>(d) = make_float4(e4[0], e4[1], e4[2], e4[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (i < nv) d[i] = e4[i];
    }
  }
}

// ------------------------------------------------------------------------------------------- scalar colours
// colorize_np (utils/colorize.py:87-92) after its range: np.clip(x, vmin, vmax), (x - vmin) / (vmax - vmin), then the colour
// map's own indexing of a float in [0, 1] (matplotlib Colormap.__call__: int(d * 256), 256 -> 255).  vmin / vmax are
// float64 scalars (np.percentile's results), and numpy 2 promotes a float32 array against them to float64: the whole
// chain is float64 here.  (The numpy 1.x the reference was written against kept float32 there, which can move a value
// by one table entry.)  np.clip passes a NaN on, fmax / fmin would drop it: tested apart.  Thread t: values [4 t, 4 t + 4).
__global__ void __launch_bounds__(256)
scalar_colorize_kernel(const float* __restrict__ x, size_t n, const double* __restrict__ lo_hi,
                       const uint32_t* __restrict__ lut, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const double lo = lo_hi[0], hi = lo_hi[1];
  const double span = hi - lo;
  const bool flat = !(hi != lo) || (span != span);
  for (size_t quad = (size_t)blockIdx.x * 256 + threadIdx.x; quad < (n + 3) / 4; quad += (size_t)gridDim.x * 256) {
    const size_t p0 = 4 * quad;
    const int nv = (n - p0 < 4) ? (int)(n - p0) : 4;
    float v[4];
    load4(x + p0, nv, v);
    uint32_t lv[3][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double xd = (double)v[i];
      const double c = fmin(fmax(xd, lo), hi);
      const double d = (c - lo) / span;
      int idx = (int)(d * 256.0);
      idx = idx > 255 ? 255 : (idx < 0 ? 0 : idx);
      const uint32_t rgba = (flat || xd != xd || d != d) ? 0u : s_lut[idx];
      lv[0][i] = rgba & 255u;
      lv[1][i] = (rgba >> 8) & 255u;
      lv[2][i] = (rgba >> 16) & 255u;
    }
    store_rgb4(out + p0 * 3, nv, lv);
  }
}

const char* os_check(const float* x, uint64_t n, int32_t m, const void* host, const void* out, const void* tmp) {
  if (x == nullptr || host == nullptr || out == nullptr || tmp == nullptr) return "null pointer";
  if (n < 1) return "n must be at least 1";
  if (n > 0xFFFFFFFFull) return "n must be at most 2^32 - 1";
  if (m < 1 || m > 4) return "m must be in 1..4";
  if ((reinterpret_cast<uintptr_t>(x) & 3u) != 0 || (reinterpret_cast<uintptr_t>(tmp) & 3u) != 0)
    return "x and tmp must be 4-byte aligned";
  return nullptr;
}

}  // namespace

extern "C" {

size_t dgs_order_stats_tmp_bytes(uint64_t n, int32_t m) {
  if (n < 1 || n > 0xFFFFFFFFull || m < 1 || m > 4) return 0;
  // the state words, then one histogram per block and rank -- of 2 m ranks, the neighbours dgs_percentiles selects
  return OS_HIST_OFFSET + (size_t)os_blocks(n) * (size_t)(2 * m) * 256 * sizeof(uint32_t);
}

int dgs_order_stats(const float* x, uint64_t n, const uint64_t* ranks_host, int32_t m, float* out, void* tmp,
                    dgs_stream_t stream) {
  char msg[96];
  if (const char* bad = os_check(x, n, m, ranks_host, out, tmp)) {
    snprintf(msg, sizeof msg, "order_stats: %s", bad);
    return dgs_fail_arg(msg);
  }
  OsRanks ranks = {};
  for (int j = 0; j < m; j++) {
    if (ranks_host[j] >= n) return dgs_fail_arg("order_stats: every rank must be below n");
    ranks.r[j] = (uint32_t)ranks_host[j];
  }
  OsFinish fin = {};
  fin.out32 = out;
  return os_select(x, n, ranks, m, tmp, fin, reinterpret_cast<hipStream_t>(stream), "order_stats");
}

int dgs_percentiles(const float* x, uint64_t n, const double* q_host, int32_t m, double* out, void* tmp,
                    dgs_stream_t stream) {
  char msg[96];
  if (const char* bad = os_check(x, n, m, q_host, out, tmp)) {
    snprintf(msg, sizeof msg, "percentiles: %s", bad);
    return dgs_fail_arg(msg);
  }
  if ((reinterpret_cast<uintptr_t>(out) & 7u) != 0) return dgs_fail_arg("percentiles: out must be 8-byte aligned");
  OsRanks ranks = {};
  OsFinish fin = {};
  fin.out64 = out;
  fin.mq = m;
  for (int j = 0; j < m; j++) {
    const double q = q_host[j];
    if (!(q >= 0.0 && q <= 100.0)) return dgs_fail_arg("percentiles: q must be in [0, 100]");
    // numpy's linear method (_get_indexes, _get_gamma): the virtual index v = (n - 1) * (q / 100) in double, its floor and
    // the fraction above it -- and from v = n - 1 on both neighbours are the last element and the weight is v - (-1), the
    // index numpy has replaced the floor by when it forms it (the second form of the interpolation then returns
    // b - 0 * (1 - g): b itself, a -0.0 included)
    const double v = (double)(n - 1) * (q / 100.0);
    uint64_t i = n - 1, above = n - 1;
    double g = v + 1.0;
    if (v < (double)(n - 1)) {
      const double lower = floor(v);
      i = (uint64_t)lower;
      above = i + 1;
      g = v - lower;
    }
    ranks.r[2 * j] = (uint32_t)i;
    ranks.r[2 * j + 1] = (uint32_t)above;
    fin.g[j] = g;
  }
  return os_select(x, n, ranks, 2 * m, tmp, fin, reinterpret_cast<hipStream_t>(stream), "percentiles");
}

int dgs_report_images(const float* x, int32_t K, int32_t mean, int32_t H, int32_t W, int32_t tone_mapping, float eps,
                      float bound, const float* gt, uint8_t* out_u8, uint8_t* gt_u8, float* err, dgs_stream_t stream) {
  if (x == nullptr || out_u8 == nullptr) return dgs_fail_arg("report_images: null pointer");
  if (gt == nullptr && (gt_u8 != nullptr || err != nullptr))
    return dgs_fail_arg("report_images: gt_u8 and err need gt (null pointer)");
  if (K < 1 || K > 65535) return dgs_fail_arg("report_images: K must be in 1..65535");
  if (mean != 0 && mean != 1) return dgs_fail_arg("report_images: mean must be 0 or 1");
  if (H < 1 || W < 1) return dgs_fail_arg("report_images: empty image");
  if ((uint64_t)H * (uint64_t)W > (1ull << 36)) return dgs_fail_arg("report_images: image above 2^36 pixels");
  if (tone_mapping != DGS_TONE_IDENTITY && tone_mapping != DGS_TONE_GAMMA)
    return dgs_fail_arg("report_images: tone_mapping must be DGS_TONE_IDENTITY or DGS_TONE_GAMMA");
  if (tone_mapping == DGS_TONE_GAMMA && !(bound < 0.5f)) return dgs_fail_arg("report_images: bound must be below 0.5");
  if ((reinterpret_cast<uintptr_t>(x) & 3u) != 0 || (reinterpret_cast<uintptr_t>(gt) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(err) & 3u) != 0)
    return dgs_fail_arg("report_images: float pointers must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t plane = (size_t)H * (size_t)W;
  const size_t quads = (plane + 3) / 4;
  const dim3 grid((uint32_t)((quads + 255) / 256), (uint32_t)(mean ? 1 : K));
  if (tone_mapping == DGS_TONE_GAMMA)
    hipLaunchKernelGGL(report_images_kernel<1>, grid, dim3(256), 0, s, x, (int)K, (int)mean, plane, eps, bound, gt, out_u8,
                       gt_u8, err);
  else
    hipLaunchKernelGGL(report_images_kernel<0>, grid, dim3(256), 0, s, x, (int)K, (int)mean, plane, eps, bound, gt, out_u8,
                       gt_u8, err);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "report_images");
}

int dgs_scalar_colorize(const float* x, uint64_t n, const double* lo_hi, const uint8_t* lut, uint8_t* out,
                        dgs_stream_t stream) {
  if (x == nullptr || lo_hi == nullptr || lut == nullptr || out == nullptr)
    return dgs_fail_arg("scalar_colorize: null pointer");
  if (n < 1) return dgs_fail_arg("scalar_colorize: n must be at least 1");
  if ((reinterpret_cast<uintptr_t>(lut) & 3u) != 0)
    return dgs_fail_arg("scalar_colorize: lut must be 4-byte aligned (one RGBA word per entry)");
  if ((reinterpret_cast<uintptr_t>(lo_hi) & 7u) != 0 || (reinterpret_cast<uintptr_t>(x) & 3u) != 0)
    return dgs_fail_arg("scalar_colorize: lo_hi must be 8-byte aligned, x 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t want = ((n + 3) / 4 + 255) / 256;
  const dim3 grid((uint32_t)(want < 8192 ? want : 8192));
  hipLaunchKernelGGL(scalar_colorize_kernel, grid, dim3(256), 0, s, x, (size_t)n, lo_hi,
                     reinterpret_cast<const uint32_t*>(lut), out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "scalar_colorize");
}

}  // extern "C"

// lpips.hip -- LPIPS with the AlexNet backbone, the third number of the reference's evaluation (test.py:120,
// lpipsPyTorch/modules/{lpips,networks,utils}.py), with the VGG16 backbone, the one metrics.py:74 reports, and with
// SqueezeNet 1.1, all with caller-supplied weights:
//   * conv_kernel: ONE implicit-GEMM fp32 convolution for all five layers on the f32-input matrix cores
//     (v_mfma_f32_32x32x2_f32), with bias + ReLU in the epilogue and the z-score of the input fused into the first
//     layer's gather;
//   * maxpool_kernel: 3 x 3 stride 2, floor, no padding;
//   * conv3x3_kernel: VGG's 3 x 3 / stride 1 / pad 1 convolutions from an input halo tile in LDS, on the same matrix
//     cores with the same epilogue; maxpool2x2_kernel: VGG's 2 x 2 stride 2 pool;
//   * fire_kernel: a SqueezeNet Fire module (squeeze 1 x 1, expand 1 x 1 and 3 x 3, concatenated) in ONE launch, the
//     squeeze map of a tile and its halo kept in LDS; maxpool3x3s2_ceil_kernel: SqueezeNet's ceil-mode pool
//     (net_type='squeeze', networks.py:69-77);
//   * layer_distance_kernel + lpips_finish_kernel: per tap the channel-normalised squared difference under the "lin"
//     weights, reduced over space in block order.
// The host side knows a backbone as a layer program -- a constant table of (operation, shape, tap, pool that follows):
// ALEX, VGG, SQUEEZE -- and has ONE plan function (lpips_plan: every layer's sizes, the taps' table, the two ping-pong
// buffers and the partials) and ONE driver (lpips_run: layer, layer distance where the layer is a tap, pool, ...,
// finish) for all three; dgs_lpips_{alex,vgg,squeeze} only flatten their weight structs for it.
// Built with -ffp-contract=off (deblurgs_amd/build.py): the compensated sum of the convolution below is only what it says
// while the compiler forms no FMA across its statements, and (x - mean) / std and the distance's sums round once per
// statement, as the torch expressions do.
//
// The arithmetic of an output element never depends on where its image stands in the call: every element is the same
// k-ordered chain whatever block, wave or lane holds it, every spatial sum is cut into blocks by the image size alone.
// So a pair's six numbers are bitwise those of a call on that pair alone, lpips(x, x) is exactly 0 and
// lpips(x, y) == lpips(y, x) ((a - b)^2 == (b - a)^2).  No float atomics anywhere.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "dgs_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int LP_BK = 32;         // k per LDS tile, and per accumulator chain (see conv_kernel)
constexpr int LP_BN = 128;        // output pixels per block
constexpr int LP_MIN = 31;        // smallest image: conv1 7 x 7, pool 3 x 3, conv2 3 x 3, pool 1 x 1

struct ConvArgs {
  const float* in0;     // images [0, n_half) [n_half,Cin,IH,IW]
  const float* in1;     // images [n_half, n_img)
  int n_half;
  const float* w;       // [Cout, K] row-major, K = Cin KH KW in (ci, ky, kx) order: the weight tensor as it is
  const float* bias;    // [Cout]
  float* out;           // [n_img, Cout, OH, OW]
  int Cin, IH, IW, Cout, OH, OW, KH, KW, stride, pad, K, N;   // N = n_img OH OW
};

// C[Cout x N] = W[Cout x K] . patches[K x N]: a block computes a (WM TM 32) x 128 tile of C with four waves, wave
// (wm, wn) a TM x TN grid of 32 x 32 MFMA tiles.  Per 32 k: the W tile goes to LDS transposed (s_a[k][m]), the patch
// values are gathered on the fly into s_b[k][n] (0 where the window leaves the image or k, n pass their ends), then
// 16 k-steps of v_mfma_f32_32x32x2_f32 -- lane l feeds A[m = l & 31][k = l >> 5] and B[k = l >> 5][n = l & 31], one
// ds_read_b32 each, 32 consecutive floats per lane group: conflict-free.
// Numerics: the MFMA is an exact k-ordered fmaf chain.  One chain over all of K (up to 3456 terms) drifts by several
// ulp, which the thin last taps of a small image show (one pixel, 256 channels: no averaging); so every 32-k tile starts
// a fresh chain from 0 and the tiles' partial sums are added with a compensated (Kahan) fp32 sum -- four VALU operations
// per accumulator register and tile, next to 16 MFMAs.  Everything stays fp32.
// (k -> (ci, ky, kx) costs two integer divisions: the first 32 threads do them once per tile, two tiles ahead, into a
// double-buffered LDS table.)
template <int WM, int WN, int TM, int TN, bool ZSCORE>
__global__ void __launch_bounds__(256) conv_kernel(const ConvArgs g) {
  constexpr int BM = WM * TM * 32;
  static_assert(WM * WN == 4 && WN * TN * 32 == LP_BN, "four waves, 128 pixels");
  __shared__ float s_a[LP_BK][BM + 1];
  __shared__ float s_b[LP_BK][LP_BN];
  __shared__ int s_koff[2][LP_BK], s_kinfo[2][LP_BK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * LP_BN;
  const int ohw = g.OH * g.OW, khw = g.KH * g.KW, ihw = g.IH * g.IW;

  // the output pixel whose patches this thread gathers
  const int n_mine = n0 + (t & (LP_BN - 1));
  const bool n_ok = n_mine < g.N;
  int img = 0, iy0 = 0, ix0 = 0;
  if (n_ok) {
    img = n_mine / ohw;
    const int p = n_mine - img * ohw;
    const int oy = p / g.OW;
    iy0 = oy * g.stride - g.pad;
    ix0 = (p - oy * g.OW) * g.stride - g.pad;
  }
  const float* src = (img < g.n_half) ? g.in0 + (size_t)img * g.Cin * ihw : g.in1 + (size_t)(img - g.n_half) * g.Cin * ihw;
  const int pix0 = iy0 * g.IW + ix0;

  auto fill_table = [&](int kt, int b) {
    if (t < LP_BK) {
      const int k = kt * LP_BK + t;
      int off = 0, info = -1;
      if (k < g.K) {
        const int ci = k / khw, r = k - ci * khw;
        const int ky = r / g.KW, kx = r - ky * g.KW;
        off = ci * ihw + ky * g.IW + kx;
        info = (ci << 8) | (ky << 4) | kx;
      }
      s_koff[b][t] = off;
      s_kinfo[b][t] = info;
    }
  };

  f32x16 tot[TM][TN], comp[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        tot[i][j][r] = 0.0f;
        comp[i][j][r] = 0.0f;
      }

  // Software pipeline: the global loads of tile kt + 1 are issued into registers before the MFMAs of tile kt and stored to
  // LDS after them, so their latency hides behind the matrix work (without it the gather, two loads in flight per
  // thread, took five times the MFMA time).  The k table of a tile is written two tiles ahead of its use.
  float ra[BM / 8], rb[LP_BK / 2];
  unsigned zs_ci = 0;   // ZSCORE: 2 bits per staged patch value: 0 = not from the image (stays 0), else channel + 1
  auto load_tile = [&](int kt) {
    const int b = kt & 1;
    const int k = kt * LP_BK + (t & 31);   // W tile: 32 consecutive k of one row per lane group
#pragma unroll
    for (int i = 0; i < BM / 8; i++) {
      const int m = m0 + (t >> 5) + 8 * i;
      ra[i] = (m < g.Cout && k < g.K) ? g.w[(size_t)m * g.K + k] : 0.0f;
    }
    zs_ci = 0;
#pragma unroll
    for (int i = 0; i < LP_BK / 2; i++) {  // patch tile: this thread's pixel at 16 of the 32 k
      const int k_l = (t >> 7) + 2 * i;
      const int info = s_kinfo[b][k_l], off = s_koff[b][k_l];
      const int iy = iy0 + ((info >> 4) & 15), ix = ix0 + (info & 15);
      const bool in = n_ok && info >= 0 && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
      rb[i] = in ? src[off + pix0] : 0.0f;
      if (ZSCORE && in) zs_ci |= (unsigned)((info >> 8) + 1) << (2 * i);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < BM / 8; i++) s_a[t & 31][(t >> 5) + 8 * i] = ra[i];
#pragma unroll
    for (int i = 0; i < LP_BK / 2; i++) {
      float v = rb[i];
      if (ZSCORE) {  // networks.py:41-51; a value from outside the image stays 0: the padding pads the z-scored image
        const unsigned c = (zs_ci >> (2 * i)) & 3u;
        const float mean = c == 1 ? -.030f : (c == 2 ? -.088f : -.188f);
        const float sd = c == 1 ? .458f : (c == 2 ? .448f : .450f);
        v = (c != 0) ? (v - mean) / sd : 0.0f;
      }
      s_b[(t >> 7) + 2 * i][t & (LP_BN - 1)] = v;
    }
  };

  const int n_kt = (g.K + LP_BK - 1) / LP_BK;
  fill_table(0, 0);
  __syncthreads();
  load_tile(0);
  if (n_kt > 1) fill_table(1, 1);
  for (int kt = 0; kt < n_kt; kt++) {
    store_tile();
    __syncthreads();
    if (kt + 1 < n_kt) load_tile(kt + 1);
    if (kt + 2 < n_kt) fill_table(kt + 2, kt & 1);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < LP_BK; kk += 2) {
      const int kr = kk + (lane >> 5);
      float a[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) a[i] = s_a[kr][(wm * TM + i) * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < TN; j++) bv[j] = s_b[kr][(wn * TN + j) * 32 + (lane & 31)];
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++) {  // Kahan: tot += acc with the rounding error of the addition carried in comp
        const f32x16 y = acc[i][j] - comp[i][j];
        const f32x16 s = tot[i][j] + y;
        comp[i][j] = (s - tot[i][j]) - y;
        tot[i][j] = s;
      }
    __syncthreads();
  }

  // bias + ReLU (a NaN passes, as torch's relu passes it).  C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) +
  // 4 (lane >> 5): per register the 32 lanes of a group write 32 consecutive pixels of one channel.
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
    if (n >= g.N) continue;
    const int im = n / ohw, p = n - im * ohw;
    float* dst = g.out + (size_t)im * g.Cout * ohw + p;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < g.Cout) {
          const float v = tot[i][j][r] + g.bias[m];
          dst[(size_t)m * ohw] = (v < 0.0f) ? 0.0f : v;
        }
      }
  }
}

// max_pool2d(kernel 3, stride 2): out[i][y][x] = max over in[i][2y .. 2y + 2][2x .. 2x + 2], planes = n_img C.  Every window
// lies inside the image (floor, no padding); a NaN in the window is the result, as torch gives it.
__global__ void __launch_bounds__(256)
maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int IH, int IW, int PH, int PW) {
  const size_t total = planes * (size_t)PH * (size_t)PW;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t plane = e / ((size_t)PH * PW);
    const int p = (int)(e - plane * ((size_t)PH * PW));
    const int y = p / PW, x = p - y * PW;
    const float* s = in + plane * (size_t)IH * IW + (size_t)(2 * y) * IW + 2 * x;
    float m = s[0];
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
      for (int dx = 0; dx < 3; dx++) {
        const float v = s[dy * IW + dx];
        m = (v > m || v != v) ? v : m;
      }
    out[e] = m;
  }
}

// ---- VGG16: every convolution is 3 x 3, stride 1, pad 1, so the patches need not be gathered element by element
constexpr int V_ROWS = 4, V_COLS = 32;           // output pixels of a block: one rectangle of one image
constexpr int V_PITCH = V_COLS + 2;              // halo row pitch, floats
constexpr int V_CH = (V_ROWS + 2) * V_PITCH;     // halo of one channel: 204 floats
constexpr int V_MIN = 16;                        // smallest image: four floor pools leave 1 x 1

// relu(conv2d(x, w, b, stride 1, pad 1)), 3 x 3: a block owns BM = WM TM 32 output channels by 4 rows x 32 columns of ONE
// image (tiles never straddle images or wrap rows); wave (wm, wn) a TM x TN grid of 32 x 32 MFMA tiles, an MFMA tile 32
// channels by the 32 columns of one row.  Per chunk of CC input channels the 6 x 34 halo of each channel goes to LDS
// once (s_h[ci][row][col], zeros outside the image and past Cin; first layer: z-scored inside the image only) together
// with the matching slab of the [Cout,Cin,3,3] weights, transposed (s_w[(ky, kx)][ci][m], pitch BM + 1).  Every staged
// halo value is used nine times: for (ky, kx) the B operand of lane l is s_h[ci = 2 j + (l >> 5)][row + ky][kx + (l & 31)]
// -- one ds_read_b32 whose two lane groups each read 32 consecutive floats, conflict-free whatever the pitch (a group is
// served on its own, bank = dword address mod 32).  The pitch is 34 = no padding at all: a channel's halo, and the
// chunk's, is one dense run of floats which the threads write in index order, 32 consecutive dwords per lane group, so
// the ds_write_b32 are conflict-free too.  The A operand is s_w[(ky, kx)][ci][32 consecutive m].  No im2col copy, no k
// table, no bounds test between the barrier and the last MFMA of a chunk.
// Pipeline: LDS is double-buffered and there is ONE barrier per chunk -- the global loads of chunk c + 1 are issued into
// registers before the MFMAs of chunk c and stored after them into the other buffer, which every wave left before the
// barrier of chunk c.
// CC: 8 for the 128-channel tile (it runs at one wave per SIMD whatever the chunk -- three accumulator sets of 64
// registers -- and the longer chunk halves the compensated sums, the zeroing and the barriers per MFMA: 87 360 B of LDS),
// 4 for the 64-channel tile (25 248 B; with 8 it would lose its second wave per SIMD to the staging registers).
// Numerics: per chunk one chain of L = 9 CC terms (72 / 36) from 0 in the k order (ky, kx, ci) -- for each of the nine
// weights in row-major order the chunk's channels in order (terms past Cin are 0 x 0); the chunks' sums are added in
// channel order with conv_kernel's compensated sum; then bias, then ReLU (a NaN passes).  An element's arithmetic depends
// on the layer shape and the image size only, never on n_img or on the image's place in the call.
template <int WM, int WN, int TM, int TN, int CC, bool ZSCORE>
__global__ void __launch_bounds__(256) conv3x3_kernel(const ConvArgs g, const int tiles_x, const int tiles_per_img) {
  constexpr int BM = WM * TM * 32, BMP = BM + 1;
  constexpr int V_L = 9 * CC, V_HALO = CC * V_CH, V_NH = (V_HALO + 255) / 256;
  constexpr int NW = BM * V_L / 256;             // weights a thread stages per chunk
  static_assert(WM * WN == 4 && WN * TN == V_ROWS && (BM * V_L) % 256 == 0, "four waves, four rows");
  __shared__ float s_w[2][V_L * BMP];
  __shared__ float s_h[2][V_HALO];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int img = blockIdx.x / tiles_per_img, tile = blockIdx.x - img * tiles_per_img;
  const int ty = tile / tiles_x;
  const int y0 = ty * V_ROWS, x0 = (tile - ty * tiles_x) * V_COLS;
  const int m0 = blockIdx.y * BM;
  const int ihw = g.IH * g.IW;
  const float* src = (img < g.n_half) ? g.in0 + (size_t)img * g.Cin * ihw : g.in1 + (size_t)(img - g.n_half) * g.Cin * ihw;

  // this thread's halo elements: where they lie in the image does not change from chunk to chunk
  int h_off[V_NH], h_ci[V_NH];   // h_ci < 0: outside the image (or past the halo's end): stays 0
#pragma unroll
  for (int i = 0; i < V_NH; i++) {
    const int e = t + 256 * i;
    const int ci = e / V_CH, rem = e - ci * V_CH;
    const int r = rem / V_PITCH, c = rem - r * V_PITCH;
    const int iy = y0 - 1 + r, ix = x0 - 1 + c;
    const bool in = e < V_HALO && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
    h_ci[i] = in ? ci : -1;
    h_off[i] = in ? ci * ihw + iy * g.IW + ix : 0;
  }

  f32x16 tot[TM][TN], comp[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        tot[i][j][r] = 0.0f;
        comp[i][j][r] = 0.0f;
      }

  float rw[NW], rh[V_NH];
  auto load_chunk = [&](int c0) {   // c0: the chunk's first input channel
#pragma unroll
    for (int i = 0; i < NW; i++) {  // 36 consecutive floats of the weight tensor per output channel
      const int e = t + 256 * i;
      const int ml = e / V_L, r = e - ml * V_L;
      const int m = m0 + ml;
      rw[i] = (m < g.Cout && c0 + r / 9 < g.Cin) ? g.w[(size_t)m * g.K + c0 * 9 + r] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < V_NH; i++) {
      const int ci = h_ci[i];
      float v = (ci >= 0 && c0 + ci < g.Cin) ? src[(size_t)c0 * ihw + h_off[i]] : 0.0f;
      if (ZSCORE) {  // networks.py:41-51, conv_kernel's expression; outside the image the halo stays 0
        const float mean = ci == 0 ? -.030f : (ci == 1 ? -.088f : -.188f);
        const float sd = ci == 0 ? .458f : (ci == 1 ? .448f : .450f);
        v = (ci >= 0 && ci < g.Cin) ? (v - mean) / sd : 0.0f;
      }
      rh[i] = v;
    }
  };
  auto store_chunk = [&](int b) {
#pragma unroll
    for (int i = 0; i < NW; i++) {
      const int e = t + 256 * i;
      const int ml = e / V_L, r = e - ml * V_L;
      const int ci = r / 9, tap = r - ci * 9;
      s_w[b][(tap * CC + ci) * BMP + ml] = rw[i];
    }
#pragma unroll
    for (int i = 0; i < V_NH; i++)
      if (t + 256 * i < V_HALO) s_h[b][t + 256 * i] = rh[i];
  };

  const int n_chunks = (g.Cin + CC - 1) / CC;
  load_chunk(0);
  for (int c = 0; c < n_chunks; c++) {
    const int b = c & 1;
    store_chunk(b);
    __syncthreads();
    if (c + 1 < n_chunks) load_chunk((c + 1) * CC);

    const float* wb = s_w[b] + (lane >> 5) * BMP + wm * TM * 32 + (lane & 31);
    const float* hb = s_h[b] + (lane >> 5) * V_CH + wn * TN * V_PITCH + (lane & 31);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
    // k-step s = (weight s / (CC / 2), channel pair s % (CC / 2)); the operands of step s + 1 are read from LDS before
    // the MFMAs of step s, so that at one wave per SIMD the ds_read latency hides behind them
    constexpr int STEPS = 9 * CC / 2;
    float a[2][TM], bv[2][TN];
    auto read_step = [&](int s, int p) {
      const int tap = s / (CC / 2), cc = 2 * (s - tap * (CC / 2));
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int i = 0; i < TM; i++) a[p][i] = wb[(tap * CC + cc) * BMP + i * 32];
#pragma unroll
      for (int j = 0; j < TN; j++) bv[p][j] = hb[cc * V_CH + (j + ky) * V_PITCH + kx];
    };
    read_step(0, 0);
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
      if (s + 1 < STEPS) read_step(s + 1, (s + 1) & 1);
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][i], bv[s & 1][j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++) {  // Kahan, as conv_kernel
        const f32x16 y = acc[i][j] - comp[i][j];
        const f32x16 s = tot[i][j] + y;
        comp[i][j] = (s - tot[i][j]) - y;
        tot[i][j] = s;
      }
  }

  // bias + ReLU; C/D layout as in conv_kernel: per register a lane group writes 32 consecutive pixels of one channel
  const int ohw = g.OH * g.OW;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int y = y0 + wn * TN + j, x = x0 + (lane & 31);
    if (y >= g.OH || x >= g.OW) continue;
    float* dst = g.out + (size_t)img * g.Cout * ohw + y * g.OW + x;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < g.Cout) {
          const float v = tot[i][j][r] + g.bias[m];
          dst[(size_t)m * ohw] = (v < 0.0f) ? 0.0f : v;
        }
      }
  }
}

// max_pool2d(kernel 2, stride 2): floor, no padding; a NaN in the window is the result (the window in row-major order,
// torch's update rule).  A thread makes two neighbouring outputs; vec (IW a multiple of 4, `in` 16-byte and `out`
// 8-byte aligned): from two 16-byte loads, one 8-byte store.
__device__ __forceinline__ float lp_max4(float a, float b, float c, float d) {
  float m = a;
  m = (b > m || b != b) ? b : m;
  m = (c > m || c != c) ? c : m;
  m = (d > m || d != d) ? d : m;
  return m;
}

__global__ void __launch_bounds__(256)
maxpool2x2_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int IH, int IW, int PH, int PW, int vec) {
  const int PW2 = (PW + 1) / 2;
  const size_t per_plane = (size_t)PH * PW2, total = planes * per_plane;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t plane = e / per_plane;
    const int p = (int)(e - plane * per_plane);
    const int y = p / PW2, x = 2 * (p - y * PW2);
    const float* s = in + plane * (size_t)IH * IW + (size_t)(2 * y) * IW + 2 * x;
    float* d = out + plane * (size_t)PH * PW + (size_t)y * PW + x;
    if (vec) {
      const float4 r0 = *reinterpret_cast<const float4*>(s), r1 = *reinterpret_cast<const float4*>(s + IW);
      *reinterpret_cast<float2*>(d) = make_float2(lp_max4(r0.x, r0.y, r1.x, r1.y), lp_max4(r0.z, r0.w, r1.z, r1.w));
    } else {
      d[0] = lp_max4(s[0], s[1], s[IW], s[IW + 1]);
      if (x + 1 < PW) d[1] = lp_max4(s[2], s[3], s[IW + 2], s[IW + 3]);
    }
  }
}

// ---- SqueezeNet 1.1: a Fire module in one launch, and the ceil-mode pool
constexpr int F_S_MAX = 64;                      // deepest squeeze map the kernel holds in LDS
constexpr int F_BM = 64;                         // expand channels of a stage-2 slab
constexpr int F_CC = 8;                          // squeeze channels per 3 x 3 weight chunk
constexpr int F_WP = F_BM + 1;                   // pitch of the staged expand weights
constexpr int F_WROWS = 9 * F_CC;                // k rows of a staged expand-weight chunk (72; the 1 x 1 slab uses <= 64)
constexpr int F_NT = (V_CH + 31) / 32;           // 32-pixel MFMA column tiles that cover the 204 halo pixels: 7
constexpr int Q_MIN = 17;                        // smallest image: 8 x 8 after the first convolution, pools to 4, 2, 1

struct FireArgs {
  const float* in0;     // images [0, n_half) [n_half,Cin,IH,IW]
  const float* in1;     // images [n_half, n_img)
  int n_half;
  const float *sw, *sb; // squeeze [S,Cin], [S]
  const float *w1, *b1; // expand 1 x 1 [E1,S], [E1]
  const float *w3, *b3; // expand 3 x 3 [E3,S,3,3], [E3]
  float* sq_out;        // [n_img,S,IH,IW] or nullptr
  float* out;           // [n_img,E1+E3,IH,IW]
  int Cin, IH, IW, S, E1, E3, tiles_x, tiles_per_img;
};

// out = cat(relu(conv1x1(s, w1, b1)), relu(conv3x3(s, w3, b3, pad 1))), s = relu(conv1x1(in, sw, sb)): a block owns 4 rows x 32
// columns of ONE image (conv3x3_kernel's tile) and the expand slabs j = blockIdx.y, blockIdx.y + gridDim.y, ... (slab j:
// channels [64 j, 64 j + 64) of BOTH expands, so blocks of one grid row carry equal work when E1 = E3).
// Stage 1: the squeeze map of the tile and its 1-pixel halo, S x 204 values, as C[S x 204] = sw[S x Cin] . in[Cin x 204]
// on v_mfma_f32_32x32x2_f32: MT = 1 (S <= 32) or 2 row tiles of 32 squeeze channels by seven column tiles of 32 halo
// pixels (the halo in its dense [row][34] order; columns 204 .. 223 of the seventh are computed and dropped), wave w the
// column tiles w and w + 4.  The input goes through LDS in chunks of CK channels (s_in[k][204], zeros outside the image
// and past Cin: conv3x3_kernel's staging, double-buffered, one barrier per chunk) with the matching columns of sw
// transposed (s_w1[k][m]).  With bias and ReLU the map is written to s_sq[m][204] -- conv3x3_kernel's s_h with the whole
// squeeze depth as its one chunk -- and never to HBM (sq_out, for the tests: each element once, by the block whose
// interior holds it, grid row 0).  A halo position OUTSIDE the image holds 0, not relu(bias): the 3 x 3 expand's zero
// padding pads the squeeze output.  Rows S .. 32 MT - 1 hold 0.  A halo pixel is recomputed by up to four blocks: its
// value is the same chain whichever column of whichever tile holds it.
// Stage 2: per slab the 1 x 1 expand (weights s_w2[ci][m], B operand s_sq[ci][row + 1][1 + 32 columns]) and the 3 x 3
// expand in chunks of 8 squeeze channels (weights s_w2[(ky, kx)][ci][m], B operand s_sq[c0 + ci][row + ky][kx + 32
// columns]: conv3x3_kernel's reads); wave w makes row w of the tile, 64 channels = two MFMA row tiles.  The expand weights
// are double-buffered in the LDS the stage-1 staging has left, loaded into registers one item ahead, one barrier per item.
// Results go to channels [0, E1) and [E1, E1 + E3) of `out`: no concatenation pass.
// All ds_read_b32 / ds_write_b32 touch 32 consecutive floats per lane group: conflict-free (s_w1's transposed write: pitch
// 65 at CK = 32, 34 at CK = 16: the 32 lanes of a group fall on 32 banks).
// LDS: MT = 2, CK = 32: s_sq 52 224 B + staging 69 120 B = 121 344 B; MT = 1, CK = 16: 26 112 B + 37 440 B = 63 552 B.
// Both instantiations run at one wave per SIMD (the compiler takes more than 256 registers; held to 256 the MT = 1
// instantiation spills 129), so a CU holds one block of either.
// Numerics, fp32 throughout.  Stage 1: per chunk of CK input channels (CK = 16 where S <= 32, else 32) one fmaf chain of
// L1 = CK terms from 0 in channel order (terms past Cin are 0 x 0); the chunks' sums are added in channel order with
// conv_kernel's compensated sum; then bias, then ReLU (a NaN passes).  Stage 2, 1 x 1 expand: ONE fmaf chain of
// L2a = S terms from 0 in channel order (S + 1 for odd S: a last 0 x 0), then bias, then ReLU.  Stage 2, 3 x 3 expand: per
// chunk of 8 squeeze channels one chain of L2b = 72 terms from 0 in the k order (ky, kx, ci) -- conv3x3_kernel's --, the
// chunks' sums added in channel order with the compensated sum, then bias, then ReLU.  An element's arithmetic depends on
// the layer shape and the image size only, never on n_img, the image's place in the call, the pixel's place in a tile,
// or the number of grid rows.
template <int MT, int CK>
__global__ void __launch_bounds__(256) fire_kernel(const FireArgs g) {
  constexpr int BM1 = MT * 32, P1 = BM1 + (CK == 32 ? 1 : 2);
  constexpr int IN_FLOATS = CK * V_CH + 32;      // + 32: the seventh column tile reads 20 floats past the last channel
  constexpr int NH = (CK * V_CH + 255) / 256, NW1 = BM1 * CK / 256, NW2 = F_BM * F_WROWS / 256;
  constexpr int STAGE1 = 2 * IN_FLOATS + 2 * CK * P1, STAGE2 = 2 * F_WROWS * F_WP;
  static_assert((BM1 * CK) % 256 == 0 && (F_BM * F_WROWS) % 256 == 0 && BM1 >= F_CC, "staging loops");
  __shared__ float s_sq[BM1 * V_CH];
  __shared__ float s_stage[STAGE1 > STAGE2 ? STAGE1 : STAGE2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, lh = lane >> 5;
  const int img = blockIdx.x / g.tiles_per_img, tile = blockIdx.x - img * g.tiles_per_img;
  const int ty = tile / g.tiles_x;
  const int y0 = ty * V_ROWS, x0 = (tile - ty * g.tiles_x) * V_COLS;
  const int ihw = g.IH * g.IW;
  const float* src = (img < g.n_half) ? g.in0 + (size_t)img * g.Cin * ihw : g.in1 + (size_t)(img - g.n_half) * g.Cin * ihw;

  // ---- stage 1
  {
    float* s_in = s_stage;                       // [2][IN_FLOATS]
    float* s_w1 = s_stage + 2 * IN_FLOATS;       // [2][CK * P1]
    int h_off[NH];                               // < 0: outside the image (or past the halo's end): stays 0
#pragma unroll
    for (int i = 0; i < NH; i++) {
      const int e = t + 256 * i;
      const int ci = e / V_CH, rem = e - ci * V_CH;
      const int r = rem / V_PITCH, c = rem - r * V_PITCH;
      const int iy = y0 - 1 + r, ix = x0 - 1 + c;
      const bool in = e < CK * V_CH && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
      h_off[i] = in ? ci * ihw + iy * g.IW + ix : -1;
    }
    float rw[NW1], rh[NH];
    auto load_chunk = [&](int c0) {
#pragma unroll
      for (int i = 0; i < NW1; i++) {            // CK consecutive floats of a squeeze-weight row per CK threads
        const int e = t + 256 * i;
        const int ml = e / CK, k = e - ml * CK;
        rw[i] = (ml < g.S && c0 + k < g.Cin) ? g.sw[(size_t)ml * g.Cin + c0 + k] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < NH; i++) {
        const int ci = (t + 256 * i) / V_CH;
        rh[i] = (h_off[i] >= 0 && c0 + ci < g.Cin) ? src[(size_t)c0 * ihw + h_off[i]] : 0.0f;
      }
    };
    auto store_chunk = [&](int b) {
#pragma unroll
      for (int i = 0; i < NW1; i++) {
        const int e = t + 256 * i;
        const int ml = e / CK, k = e - ml * CK;
        s_w1[b * CK * P1 + k * P1 + ml] = rw[i];
      }
#pragma unroll
      for (int i = 0; i < NH; i++)
        if (t + 256 * i < CK * V_CH) s_in[b * IN_FLOATS + t + 256 * i] = rh[i];
    };

    const bool two = wave + 4 < F_NT;            // waves 0..2 own two column tiles, wave 3 one
    f32x16 tot[MT][2], comp[MT][2];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          tot[i][j][r] = 0.0f;
          comp[i][j][r] = 0.0f;
        }
    const int n_chunks = (g.Cin + CK - 1) / CK;
    load_chunk(0);
    for (int c = 0; c < n_chunks; c++) {
      const int b = c & 1;
      store_chunk(b);
      __syncthreads();
      if (c + 1 < n_chunks) load_chunk((c + 1) * CK);
      const float* wb = s_w1 + b * CK * P1 + lh * P1 + l31;
      const float* hb = s_in + b * IN_FLOATS + lh * V_CH + wave * 32 + l31;
      f32x16 acc[MT][2];
#pragma unroll
      for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
#pragma unroll
      for (int kk = 0; kk < CK; kk += 2) {
        float a[MT], bv[2];
#pragma unroll
        for (int i = 0; i < MT; i++) a[i] = wb[kk * P1 + i * 32];
        bv[0] = hb[kk * V_CH];
        bv[1] = two ? hb[kk * V_CH + 128] : 0.0f;
#pragma unroll
        for (int i = 0; i < MT; i++) {
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[0], acc[i][0], 0, 0, 0);
          if (two) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[1], acc[i][1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {  // Kahan, as conv_kernel
          const f32x16 y = acc[i][j] - comp[i][j];
          const f32x16 s = tot[i][j] + y;
          comp[i][j] = (s - tot[i][j]) - y;
          tot[i][j] = s;
        }
    }
    // bias + ReLU into s_sq; C/D layout: column (halo pixel) = lane & 31, row (squeeze channel) = (r & 3) + 8 (r >> 2) +
    // 4 (lane >> 5): per register a lane group writes 32 consecutive floats
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int hp = (wave + 4 * j) * 32 + l31;
      if ((j == 1 && !two) || hp >= V_CH) continue;
      const int hr = hp / V_PITCH, hc = hp - hr * V_PITCH;
      const int iy = y0 - 1 + hr, ix = x0 - 1 + hc;
      const bool in = (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
      const bool mine = in && g.sq_out != nullptr && blockIdx.y == 0 && hr >= 1 && hr <= V_ROWS && hc >= 1 && hc <= V_COLS;
#pragma unroll
      for (int i = 0; i < MT; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          float v = 0.0f;
          if (in && m < g.S) {
            v = tot[i][j][r] + g.sb[m];
            v = (v < 0.0f) ? 0.0f : v;
          }
          s_sq[m * V_CH + hp] = v;
          if (mine && m < g.S) g.sq_out[((size_t)img * g.S + m) * ihw + iy * g.IW + ix] = v;
        }
    }
  }
  __syncthreads();   // s_sq is complete, and every wave has left the stage-1 staging that the expand weights now overwrite

  // ---- stage 2: items of this block in order: per slab j the 1 x 1 expand (p = 0, if 64 j < E1), then the chunks
  // p = 1 .. nc of the 3 x 3 expand (if 64 j < E3)
  const int n1 = (g.E1 + F_BM - 1) / F_BM, n3 = (g.E3 + F_BM - 1) / F_BM, nsl = n1 > n3 ? n1 : n3;
  const int nc = (g.S + F_CC - 1) / F_CC, s_even = g.S + (g.S & 1);
  const int step = gridDim.y;
  auto advance = [&](int& j, int& p) {           // the next item (j >= nsl: none)
    do {
      if (p < nc) {
        p++;
      } else {
        p = 0;
        j += step;
      }
    } while (j < nsl && !(p == 0 ? j < n1 : j < n3));
  };
  float rw[NW2];
  auto load_item = [&](int j, int p) {
    const int m0 = j * F_BM;
    if (p == 0) {   // [64, S] of w1 is one dense run: thread t takes floats t, t + 256, ...
#pragma unroll
      for (int i = 0; i < NW2; i++) {
        const int e = t + 256 * i;
        const int ml = e / g.S;
        rw[i] = (e < F_BM * g.S && m0 + ml < g.E1) ? g.w1[(size_t)m0 * g.S + e] : 0.0f;
      }
    } else {        // 72 consecutive floats of the weight tensor per output channel (conv3x3_kernel's load)
      const int c0 = (p - 1) * F_CC;
#pragma unroll
      for (int i = 0; i < NW2; i++) {
        const int e = t + 256 * i;
        const int ml = e / F_WROWS, r = e - ml * F_WROWS;
        rw[i] = (m0 + ml < g.E3 && c0 + r / 9 < g.S) ? g.w3[((size_t)(m0 + ml) * g.S + c0) * 9 + r] : 0.0f;
      }
    }
  };
  auto store_item = [&](int p, int b) {
    float* w = s_stage + b * F_WROWS * F_WP;
    if (p == 0) {
#pragma unroll
      for (int i = 0; i < NW2; i++) {
        const int e = t + 256 * i;
        const int ml = e / g.S, ci = e - ml * g.S;
        if (e < F_BM * g.S) w[ci * F_WP + ml] = rw[i];
      }
      if (s_even != g.S && t < F_BM) w[g.S * F_WP + t] = 0.0f;   // odd S: the chain's last term is 0 x 0
    } else {
#pragma unroll
      for (int i = 0; i < NW2; i++) {
        const int e = t + 256 * i;
        const int ml = e / F_WROWS, r = e - ml * F_WROWS;
        const int ci = r / 9, tap = r - ci * 9;
        w[(tap * F_CC + ci) * F_WP + ml] = rw[i];
      }
    }
  };
  // bias + ReLU of wave `wave`'s row to channels choff + m0 .. of `out` (C/D layout as above: 32 consecutive pixels of one
  // channel per lane group and register)
  auto write_out = [&](const f32x16 (&val)[2], const float* bias, int m0, int E, int choff) {
    const int y = y0 + wave, x = x0 + l31;
    if (y >= g.IH || x >= g.IW) return;
    float* dst = g.out + ((size_t)img * (g.E1 + g.E3) + choff) * ihw + y * g.IW + x;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < E) {
          const float v = val[i][r] + bias[m];
          dst[(size_t)m * ihw] = (v < 0.0f) ? 0.0f : v;
        }
      }
  };

  f32x16 tot[2], comp[2];
  int j = blockIdx.y, p = 0, b = 0;
  if (!(j < n1)) advance(j, p);
  if (j < nsl) load_item(j, p);
  while (j < nsl) {
    store_item(p, b);
    __syncthreads();
    int jn = j, pn = p;
    advance(jn, pn);
    if (jn < nsl) load_item(jn, pn);
    const float* wb = s_stage + b * F_WROWS * F_WP + lh * F_WP + l31;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][r] = 0.0f;
    if (p == 0) {
      const float* hb = s_sq + lh * V_CH + (wave + 1) * V_PITCH + 1 + l31;
      for (int k = 0; k < s_even; k += 2) {
        const float a0 = wb[k * F_WP], a1 = wb[k * F_WP + 32], bv = hb[k * V_CH];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1], 0, 0, 0);
      }
      write_out(acc, g.b1, j * F_BM, g.E1, 0);
    } else {
      if (p == 1) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            tot[i][r] = 0.0f;
            comp[i][r] = 0.0f;
          }
      }
      const float* hb = s_sq + ((p - 1) * F_CC + lh) * V_CH + wave * V_PITCH + l31;
      // k-step s = (weight s / 4, channel pair s % 4); the operands of step s + 1 are read before the MFMAs of step s
      constexpr int STEPS = 9 * F_CC / 2;
      float a[2][2], bv[2];
      auto read_step = [&](int s, int q) {
        const int tap = s / (F_CC / 2), cc = 2 * (s - tap * (F_CC / 2));
        const int ky = tap / 3, kx = tap - 3 * ky;
        a[q][0] = wb[(tap * F_CC + cc) * F_WP];
        a[q][1] = wb[(tap * F_CC + cc) * F_WP + 32];
        bv[q] = hb[cc * V_CH + ky * V_PITCH + kx];
      };
      read_step(0, 0);
#pragma unroll
      for (int s = 0; s < STEPS; s++) {
        if (s + 1 < STEPS) read_step(s + 1, (s + 1) & 1);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][0], bv[s & 1], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][1], bv[s & 1], acc[1], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; i++) {  // Kahan, as conv_kernel
        const f32x16 y = acc[i] - comp[i];
        const f32x16 s = tot[i] + y;
        comp[i] = (s - tot[i]) - y;
        tot[i] = s;
      }
      if (p == nc) write_out(tot, g.b3, j * F_BM, g.E3, g.E1);
    }
    j = jn, p = pn, b ^= 1;
  }
}

// max_pool2d(kernel 3, stride 2, ceil_mode): out[i][y][x] = max over in[i][2y .. min(2y + 2, IH - 1)][2x .. min(2x + 2,
// IW - 1)], PH = IH / 2, PW = IW / 2 (IH, IW >= 2: torch drops a window that would start outside the input, so an even
// size ends with a window of two).  A NaN in the part inside the image is the result.
__global__ void __launch_bounds__(256)
maxpool3x3s2_ceil_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int IH, int IW, int PH, int PW) {
  const size_t total = planes * (size_t)PH * (size_t)PW;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t plane = e / ((size_t)PH * PW);
    const int p = (int)(e - plane * ((size_t)PH * PW));
    const int y = p / PW, x = p - y * PW;
    const float* s = in + plane * (size_t)IH * IW + (size_t)(2 * y) * IW + 2 * x;
    const int nh = (2 * y + 3 <= IH) ? 3 : IH - 2 * y, nw = (2 * x + 3 <= IW) ? 3 : IW - 2 * x;
    float m = s[0];
    for (int dy = 0; dy < nh; dy++)
      for (int dx = 0; dx < nw; dx++) {
        const float v = s[dy * IW + dx];
        m = (v > m || v != v) ? v : m;
      }
    out[e] = m;
  }
}

// sum over the 256 threads of a block in a fixed order (as metrics.hip's); valid in thread 0
__device__ __forceinline__ double lp_block_sum_256(double v, double* red) {
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

// One tap of one pair (blockIdx.y): f [2 n_pairs, C, HW], image `pair` against image n_pairs + pair.  A thread per pixel:
// na = sqrt(sum_c a_c^2) + 1e-10 and nb alike (utils.py:6-8), then sum_c lin_c (a_c / na - b_c / nb)^2, channels in
// order, fp32; the block adds its 256 pixels in a fixed tree and writes partials[pair][block].
__global__ void __launch_bounds__(256)
layer_distance_kernel(const float* __restrict__ f, int n_pairs, int C, int HW, const float* __restrict__ lin,
                      double* __restrict__ partials) {
  __shared__ double red[256];
  const int pair = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const float* a = f + (size_t)pair * C * HW;
  const float* b = f + (size_t)(n_pairs + pair) * C * HW;
  float s = 0.0f;
  if (p < HW) {
    float sa = 0.0f, sb = 0.0f;
    for (int c = 0; c < C; c++) {
      const float va = a[(size_t)c * HW + p], vb = b[(size_t)c * HW + p];
      sa += va * va;
      sb += vb * vb;
    }
    const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
    for (int c = 0; c < C; c++) {
      const float d = a[(size_t)c * HW + p] / na - b[(size_t)c * HW + p] / nb;
      s += lin[c] * (d * d);
    }
  }
  const double tot = lp_block_sum_256((double)s, red);
  if (threadIdx.x == 0) partials[(size_t)pair * gridDim.x + blockIdx.x] = tot;
}

constexpr int LP_MAX_TAPS = 7;
struct LpipsTaps {
  size_t first[LP_MAX_TAPS];   // where a tap's partials start (in doubles); pair i's blocks at first + i * blocks
  int blocks[LP_MAX_TAPS];
  double hw[LP_MAX_TAPS];
  int n;                       // taps of the backbone: 5 (alex, vgg) or 7 (squeeze)
};

// One block per pair: per tap the blocks' sums in index order / HW; out[pair] = (total, layer 1..n)
__global__ void __launch_bounds__(256) lpips_finish_kernel(const double* __restrict__ partials, LpipsTaps taps, float* __restrict__ out) {
  __shared__ double red[256];
  const int pair = blockIdx.x;
  double total = 0.0;
  const size_t row = (size_t)(taps.n + 1) * pair;
  for (int l = 0; l < taps.n; l++) {
    const double* src = partials + taps.first[l] + (size_t)pair * taps.blocks[l];
    double s = 0.0;
    for (int i = threadIdx.x; i < taps.blocks[l]; i += 256) s += src[i];
    s = lp_block_sum_256(s, red);
    const double mean = s / taps.hw[l];
    total += mean;
    if (threadIdx.x == 0) out[row + 1 + l] = (float)mean;
  }
  if (threadIdx.x == 0) out[row] = (float)total;
}

// ---- host side
size_t lp_align(size_t x) { return (x + 255) & ~(size_t)255; }

hipError_t launch_conv(const ConvArgs& g, bool zscore, hipStream_t s) {
  const unsigned gx = (unsigned)((g.N + LP_BN - 1) / LP_BN);
  if (g.Cout <= 64) {  // 64 x 128 tiles: wave w takes pixels 32 w .. 32 w + 31
    const dim3 grid(gx, (unsigned)((g.Cout + 63) / 64));
    if (zscore)
      hipLaunchKernelGGL((conv_kernel<1, 4, 2, 1, true>), grid, dim3(256), 0, s, g);
    else
      hipLaunchKernelGGL((conv_kernel<1, 4, 2, 1, false>), grid, dim3(256), 0, s, g);
  } else {             // 128 x 128 tiles: 2 x 2 waves of 2 x 2 MFMA tiles
    const dim3 grid(gx, (unsigned)((g.Cout + 127) / 128));
    if (zscore)
      hipLaunchKernelGGL((conv_kernel<2, 2, 2, 2, true>), grid, dim3(256), 0, s, g);
    else
      hipLaunchKernelGGL((conv_kernel<2, 2, 2, 2, false>), grid, dim3(256), 0, s, g);
  }
  return hipGetLastError();
}

// Which convolution kernel a VGG layer runs on: a function of the layer shape only (DESIGN.md 7 has the per-layer timings
// behind it).  The halo-tile kernel won every layer but the first by 8 % and more in every round; on 3 -> 64 channels
// (14 GFLOP, 1 GB written: bound by the store) it was not on one side of the generic kernel in every round, and a layer
// it has not won stays on the generic kernel.
bool vgg_layer_on_conv3x3(int Cin, int Cout) {
  (void)Cout;
  return Cin > 3;
}

hipError_t launch_conv3x3(const ConvArgs& g, int n_img, bool zscore, hipStream_t s) {
  const int tiles_x = (g.OW + V_COLS - 1) / V_COLS, tiles_per_img = tiles_x * ((g.OH + V_ROWS - 1) / V_ROWS);
  const unsigned gx = (unsigned)((size_t)n_img * tiles_per_img);
  if (g.Cout <= 64) {  // 64 channels: wave w takes row w
    const dim3 grid(gx, (unsigned)((g.Cout + 63) / 64));
    if (zscore)
      hipLaunchKernelGGL((conv3x3_kernel<1, 4, 2, 1, 4, true>), grid, dim3(256), 0, s, g, tiles_x, tiles_per_img);
    else
      hipLaunchKernelGGL((conv3x3_kernel<1, 4, 2, 1, 4, false>), grid, dim3(256), 0, s, g, tiles_x, tiles_per_img);
  } else {             // 128 channels: 2 x 2 waves of 2 x 2 MFMA tiles (64 channels by two rows)
    const dim3 grid(gx, (unsigned)((g.Cout + 127) / 128));
    if (zscore)
      hipLaunchKernelGGL((conv3x3_kernel<2, 2, 2, 2, 8, true>), grid, dim3(256), 0, s, g, tiles_x, tiles_per_img);
    else
      hipLaunchKernelGGL((conv3x3_kernel<2, 2, 2, 2, 8, false>), grid, dim3(256), 0, s, g, tiles_x, tiles_per_img);
  }
  return hipGetLastError();
}

size_t conv3x3_tiles(int64_t n_img, int64_t H, int64_t W) {
  return (size_t)(n_img * ((H + V_ROWS - 1) / V_ROWS) * ((W + V_COLS - 1) / V_COLS));
}

hipError_t launch_maxpool2x2(const float* in, size_t planes, int IH, int IW, float* out, hipStream_t s) {
  const int PH = IH / 2, PW = IW / 2;
  const size_t total = planes * (size_t)PH * ((PW + 1) / 2), want = (total + 255) / 256;
  const int vec = (IW % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0) ? 1 : 0;
  hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)(want < (1u << 20) ? want : (1u << 20))), dim3(256), 0, s, in, out, planes,
                     IH, IW, PH, PW, vec);
  return hipGetLastError();
}

size_t fire_tiles(int64_t n_img, int64_t H, int64_t W) { return conv3x3_tiles(n_img, H, W); }

// Grid rows (how many blocks share the expand slabs of one tile; each repeats stage 1): per pixel stage 1 is Cin S
// multiply-adds (x 1.75 for the halo and the dropped columns) against S (E1 + 9 E3) of stage 2 -- 0.17 to 0.35 of it for
// the eight SqueezeNet modules -- so one row wherever the tiles alone fill the device, and more only below 256 tiles per
// image (Fires 5 .. 8 at 1080p have 68).  A function of the layer shape and the image size only.
int fire_grid_rows(int E1, int E3, int tiles_per_img) {
  const int n1 = (E1 + F_BM - 1) / F_BM, n3 = (E3 + F_BM - 1) / F_BM, nsl = n1 > n3 ? n1 : n3;
  const int want = (256 + tiles_per_img - 1) / tiles_per_img;
  return want < nsl ? want : nsl;
}

hipError_t launch_fire(FireArgs& g, int n_img, hipStream_t s) {
  g.tiles_x = (g.IW + V_COLS - 1) / V_COLS;
  g.tiles_per_img = g.tiles_x * ((g.IH + V_ROWS - 1) / V_ROWS);
  const dim3 grid((unsigned)((size_t)n_img * g.tiles_per_img), (unsigned)fire_grid_rows(g.E1, g.E3, g.tiles_per_img));
  if (g.S <= 32)
    hipLaunchKernelGGL((fire_kernel<1, 16>), grid, dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((fire_kernel<2, 32>), grid, dim3(256), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_maxpool_ceil(const float* in, size_t planes, int IH, int IW, float* out, hipStream_t s) {
  const int PH = IH / 2, PW = IW / 2;
  const size_t total = planes * (size_t)PH * PW, want = (total + 255) / 256;
  hipLaunchKernelGGL(maxpool3x3s2_ceil_kernel, dim3((unsigned)(want < (1u << 20) ? want : (1u << 20))), dim3(256), 0, s, in, out,
                     planes, IH, IW, PH, PW);
  return hipGetLastError();
}

hipError_t launch_maxpool_floor(const float* in, size_t planes, int IH, int IW, float* out, hipStream_t s) {
  const int PH = (IH - 3) / 2 + 1, PW = (IW - 3) / 2 + 1;
  const size_t total = planes * PH * PW, want = (total + 255) / 256;
  hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)(want < (1u << 20) ? want : (1u << 20))), dim3(256), 0, s, in, out, planes,
                     IH, IW, PH, PW);
  return hipGetLastError();
}

bool fire_weights_null(const DgsFireWeights& f) {
  return f.squeeze_w == nullptr || f.squeeze_b == nullptr || f.expand1_w == nullptr || f.expand1_b == nullptr ||
         f.expand3_w == nullptr || f.expand3_b == nullptr;
}

// ---- the layer program: a backbone is a table of layers, and ONE plan function and ONE driver walk it
enum LayerOp { OP_CONV, OP_CONV3X3, OP_FIRE };   // generic convolution; 3 x 3 / 1 / pad 1 (vgg_layer_on_conv3x3 picks the kernel); Fire
enum PoolOp { POOL_NONE, POOL_3X3S2_FLOOR, POOL_2X2, POOL_3X3S2_CEIL };

struct Layer {
  LayerOp op;
  int Cin, Cout, k, stride, pad;   // a Fire module: Cout = 2 E, and 3, 1, 1 -- the map keeps its size
  int S;                           // a Fire module's squeeze depth, else 0
  int tap;                         // the tap this layer's output is, or -1
  PoolOp pool;                     // the pool that follows
};
constexpr Layer conv(int Cin, int Cout, int k, int stride, int pad, int tap, PoolOp pool) {
  return {OP_CONV, Cin, Cout, k, stride, pad, 0, tap, pool};
}
constexpr Layer conv3x3(int Cin, int Cout, int tap, PoolOp pool) { return {OP_CONV3X3, Cin, Cout, 3, 1, 1, 0, tap, pool}; }
constexpr Layer fire(int Cin, int S, int E, int tap, PoolOp pool) { return {OP_FIRE, Cin, 2 * E, 3, 1, 1, S, tap, pool}; }

constexpr int LP_MAX_LAYERS = 13;
struct Backbone {
  const char *name, *n_weights;   // for the error texts: "alex", "fifteen"
  int min_size, n_layers, n_taps;
  bool equal_bufs;   // both scratch buffers take the largest map of the program (else each the largest map written to it)
  bool map_limit;    // refuse a first layer whose output has 2^31 elements or more per image
  Layer layers[LP_MAX_LAYERS];
};

// AlexNet (networks.py:80-85): five convolutions on the generic kernel, each a tap; 3 x 3 / 2 pools after the first two
const Backbone ALEX = {"alex", "fifteen", LP_MIN, 5, 5, false, false,
                       {conv(3, 64, 11, 4, 2, 0, POOL_3X3S2_FLOOR), conv(64, 192, 5, 1, 2, 1, POOL_3X3S2_FLOOR),
                        conv(192, 384, 3, 1, 1, 2, POOL_NONE), conv(384, 256, 3, 1, 1, 3, POOL_NONE),
                        conv(256, 256, 3, 1, 1, 4, POOL_NONE)}};
// VGG16 (networks.py:88-96): thirteen 3 x 3 convolutions; taps after convolutions 2, 4, 7, 10 (each before its 2 x 2
// pool) and 13
const Backbone VGG = {"vgg", "thirty-one", V_MIN, 13, 5, true, true,
                      {conv3x3(3, 64, -1, POOL_NONE), conv3x3(64, 64, 0, POOL_2X2), conv3x3(64, 128, -1, POOL_NONE),
                       conv3x3(128, 128, 1, POOL_2X2), conv3x3(128, 256, -1, POOL_NONE), conv3x3(256, 256, -1, POOL_NONE),
                       conv3x3(256, 256, 2, POOL_2X2), conv3x3(256, 512, -1, POOL_NONE), conv3x3(512, 512, -1, POOL_NONE),
                       conv3x3(512, 512, 3, POOL_2X2), conv3x3(512, 512, -1, POOL_NONE), conv3x3(512, 512, -1, POOL_NONE),
                       conv3x3(512, 512, 4, POOL_NONE)}};
// SqueezeNet 1.1 (networks.py:69-77): conv 3 x 3 / 2 (no padding), ReLU, pool, Fire 1, Fire 2, pool, Fire 3, Fire 4,
// pool, Fire 5 .. 8; pools 3 x 3 / 2 in ceil mode; taps: the first ReLU and Fires 2, 4, 5, 6, 7, 8 (each before its pool).
// Its two buffers both take the first convolution's output, though the second never holds that much: 529,328,896 bytes
// for one 1080p pair is what include/dgs_hip.h promises.
const Backbone SQUEEZE = {"squeeze", "fifty-seven", Q_MIN, 9, 7, true, true,
                          {conv(3, 64, 3, 2, 0, 0, POOL_3X3S2_CEIL), fire(64, 16, 64, -1, POOL_NONE),
                           fire(128, 16, 64, 1, POOL_3X3S2_CEIL), fire(128, 32, 128, -1, POOL_NONE),
                           fire(256, 32, 128, 2, POOL_3X3S2_CEIL), fire(256, 48, 192, 3, POOL_NONE),
                           fire(384, 48, 192, 4, POOL_NONE), fire(384, 64, 256, 5, POOL_NONE), fire(512, 64, 256, 6, POOL_NONE)}};

int pooled(PoolOp pool, int n) { return pool == POOL_NONE ? n : pool == POOL_3X3S2_FLOOR ? (n - 3) / 2 + 1 : n / 2; }

struct LpipsPlan {
  int ih[LP_MAX_LAYERS], iw[LP_MAX_LAYERS], oh[LP_MAX_LAYERS], ow[LP_MAX_LAYERS];   // every layer's input and output size
  size_t off_b, off_partials, total_bytes;   // buffer A at 0, buffer B, the taps' partials
  LpipsTaps taps;
};

// Walks the program once, in the driver's order: every map goes to the buffer that does not hold its input, A first.
// false: an image below the backbone's smallest, no pairs, or sizes the kernels' 32-bit arithmetic does not cover
bool lpips_plan(const Backbone& B, int W, int H, int n_pairs, LpipsPlan& P) {
  if (W < B.min_size || H < B.min_size || n_pairs < 1 || n_pairs > 65535 || W > 65536 || H > 65536) return false;
  const size_t n_img = 2 * (size_t)n_pairs, limit = (size_t)1 << 31;
  size_t need[2] = {0, 0}, partial = 0;   // floats of the two buffers, doubles of the partials
  int h = H, w = W, which = 0;
  auto written = [&](int C) {
    const size_t map = n_img * C * (size_t)h * w;
    need[which] = map > need[which] ? map : need[which];
    which ^= 1;
  };
  for (int l = 0; l < B.n_layers; l++) {
    const Layer& y = B.layers[l];
    P.ih[l] = h, P.iw[l] = w;
    h = (h + 2 * y.pad - y.k) / y.stride + 1;
    w = (w + 2 * y.pad - y.k) / y.stride + 1;
    P.oh[l] = h, P.ow[l] = w;
    written(y.Cout);
    if (y.tap >= 0) {
      P.taps.first[y.tap] = partial;
      P.taps.blocks[y.tap] = (int)(((size_t)h * w + 255) / 256);
      P.taps.hw[y.tap] = (double)h * (double)w;
      partial += (size_t)n_pairs * P.taps.blocks[y.tap];
    }
    if (y.pool != POOL_NONE) {
      h = pooled(y.pool, h), w = pooled(y.pool, w);
      written(y.Cout);
    }
  }
  P.taps.n = B.n_taps;
  // (int32 arithmetic of the kernels: elements of one input image, pixels of a call, elements of one image's largest map)
  const size_t px0 = (size_t)P.oh[0] * P.ow[0];
  if ((size_t)3 * H * W >= limit || n_img * px0 >= limit || (B.map_limit && B.layers[0].Cout * px0 >= limit)) return false;
  if (B.equal_bufs) need[0] = need[1] = need[0] > need[1] ? need[0] : need[1];
  P.off_b = lp_align(need[0] * sizeof(float));
  P.off_partials = P.off_b + lp_align(need[1] * sizeof(float));
  P.total_bytes = P.off_partials + lp_align(partial * sizeof(double));
  return true;
}

struct LpipsWeights {   // the three ABI structs, flattened by their entry points
  const float* layer[LP_MAX_LAYERS][6];   // a convolution's (w, bias), a Fire module's six in DgsFireWeights' order
  const float* lin[LP_MAX_TAPS];
};

int lpips_refuse(const Backbone& B, const char* fmt, ...) {
  char what[128], msg[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(what, sizeof what, fmt, ap);
  va_end(ap);
  snprintf(msg, sizeof msg, "lpips_%s: %s", B.name, what);
  return dgs_fail_arg(msg);
}

// out[pair] = (total, layer 1 .. n_taps) of the pairs (a[i], b[i]).  The first layer reads the two arrays and z-scores
// them in its gather; every later map is one array of 2 n_pairs images, the b half behind the a half.
int lpips_run(const Backbone& B, const float* a, const float* b, int n_pairs, int W, int H, const LpipsWeights* w, void* tmp,
              float* out, dgs_stream_t stream) {
  if (a == nullptr || b == nullptr || w == nullptr || tmp == nullptr || out == nullptr) return lpips_refuse(B, "null pointer");
  bool hole = false;
  for (int l = 0; l < B.n_layers; l++)
    for (int i = 0; i < (B.layers[l].op == OP_FIRE ? 6 : 2); i++) hole |= w->layer[l][i] == nullptr;
  for (int t = 0; t < B.n_taps; t++) hole |= w->lin[t] == nullptr;
  if (hole) return lpips_refuse(B, "null pointer among the %s weight pointers", B.n_weights);
  if (n_pairs < 1) return lpips_refuse(B, "n_pairs must be at least 1");
  if (W < B.min_size || H < B.min_size)
    return lpips_refuse(B, "the smallest image the network accepts is %d x %d (W and H >= %d)", B.min_size, B.min_size, B.min_size);
  LpipsPlan P;
  if (!lpips_plan(B, W, H, n_pairs, P)) return lpips_refuse(B, "more than 65535 pairs or more pixels than one call covers");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>(tmp);
  float* bufs[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + P.off_b)};
  double* partials = reinterpret_cast<double*>(base + P.off_partials);
  const int n_img = 2 * n_pairs;
  auto fail = [&](hipError_t e, const char* stage) {
    char where[64];
    snprintf(where, sizeof where, "lpips_%s (%s)", B.name, stage);
    return dgs_fail_hip(e, where);
  };

  const float* cur = nullptr;   // the map the next kernel reads
  int which = 0;                // the buffer the next kernel writes
  for (int l = 0; l < B.n_layers; l++) {
    const Layer& y = B.layers[l];
    const float* const* p = w->layer[l];
    const int ih = P.ih[l], iw = P.iw[l], oh = P.oh[l], ow = P.ow[l];
    float* dst = bufs[which];
    which ^= 1;
    hipError_t e;
    if (y.op == OP_FIRE) {   // (never the first layer: it reads one array)
      FireArgs g;
      g.in0 = cur, g.in1 = cur, g.n_half = n_img;
      g.sw = p[0], g.sb = p[1], g.w1 = p[2], g.b1 = p[3], g.w3 = p[4], g.b3 = p[5];
      g.sq_out = nullptr, g.out = dst;
      g.Cin = y.Cin, g.IH = ih, g.IW = iw, g.S = y.S, g.E1 = y.Cout / 2, g.E3 = y.Cout / 2;
      e = launch_fire(g, n_img, s);
    } else {
      ConvArgs g;
      g.in0 = (l == 0) ? a : cur;
      g.in1 = (l == 0) ? b : cur + (size_t)n_pairs * y.Cin * ih * iw;
      g.n_half = n_pairs;
      g.w = p[0], g.bias = p[1], g.out = dst;
      g.Cin = y.Cin, g.IH = ih, g.IW = iw, g.Cout = y.Cout, g.OH = oh, g.OW = ow;
      g.KH = y.k, g.KW = y.k, g.stride = y.stride, g.pad = y.pad, g.K = y.Cin * y.k * y.k, g.N = n_img * oh * ow;
      e = (y.op == OP_CONV3X3 && vgg_layer_on_conv3x3(y.Cin, y.Cout)) ? launch_conv3x3(g, n_img, l == 0, s) : launch_conv(g, l == 0, s);
    }
    if (e != hipSuccess) return fail(e, y.op == OP_FIRE ? "Fire module" : "convolution");
    cur = dst;
    if (y.tap >= 0) {
      hipLaunchKernelGGL(layer_distance_kernel, dim3((unsigned)P.taps.blocks[y.tap], (unsigned)n_pairs), dim3(256), 0, s, cur,
                         (int)n_pairs, y.Cout, oh * ow, w->lin[y.tap], partials + P.taps.first[y.tap]);
      e = hipGetLastError();
      if (e != hipSuccess) return fail(e, "layer distance");
    }
    if (y.pool != POOL_NONE) {
      const size_t planes = (size_t)n_img * y.Cout;
      dst = bufs[which];
      which ^= 1;
      e = y.pool == POOL_2X2          ? launch_maxpool2x2(cur, planes, oh, ow, dst, s)
          : y.pool == POOL_3X3S2_CEIL ? launch_maxpool_ceil(cur, planes, oh, ow, dst, s)
                                      : launch_maxpool_floor(cur, planes, oh, ow, dst, s);
      if (e != hipSuccess) return fail(e, "max-pool");
      cur = dst;
    }
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, partials, P.taps, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : fail(e, "finish");
}

}  // namespace

extern "C" {

int dgs_fire_bias_relu(const float* in, int32_t n_img, int32_t Cin, int32_t IH, int32_t IW, int32_t S, int32_t E1, int32_t E3,
                       const DgsFireWeights* w, float* squeeze_out, float* out, dgs_stream_t stream) {
  if (in == nullptr || w == nullptr || out == nullptr || fire_weights_null(*w)) return dgs_fail_arg("fire_bias_relu: null pointer");
  if (n_img < 1 || Cin < 1 || E1 < 1 || E3 < 1 || IH < 1 || IW < 1) return dgs_fail_arg("fire_bias_relu: empty input or output");
  if (S < 1 || S > F_S_MAX) return dgs_fail_arg("fire_bias_relu: the squeeze depth S is 1..64 (the squeeze map stays in LDS)");
  if ((int64_t)Cin * IH * IW >= (1ll << 31) || ((int64_t)E1 + E3) * IH * IW >= (1ll << 31) || (int64_t)n_img * IH * IW >= (1ll << 31) ||
      fire_tiles(n_img, IH, IW) >= ((size_t)1 << 31) || E1 >= (1 << 24) || E3 >= (1 << 24) || Cin >= (1 << 24))
    return dgs_fail_arg("fire_bias_relu: sizes beyond the kernel's 32-bit index arithmetic");
  FireArgs g;
  g.in0 = in, g.in1 = in, g.n_half = n_img;
  g.sw = w->squeeze_w, g.sb = w->squeeze_b, g.w1 = w->expand1_w, g.b1 = w->expand1_b, g.w3 = w->expand3_w, g.b3 = w->expand3_b;
  g.sq_out = squeeze_out, g.out = out;
  g.Cin = Cin, g.IH = IH, g.IW = IW, g.S = S, g.E1 = E1, g.E3 = E3;
  const hipError_t e = launch_fire(g, n_img, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "fire_bias_relu");
}

int dgs_maxpool3x3s2_ceil(const float* in, uint64_t planes, int32_t IH, int32_t IW, float* out, dgs_stream_t stream) {
  if (in == nullptr || out == nullptr) return dgs_fail_arg("maxpool3x3s2_ceil: null pointer");
  if (planes < 1 || IH < 2 || IW < 2) return dgs_fail_arg("maxpool3x3s2_ceil: no planes, or planes below 2 x 2");
  if ((int64_t)IH * IW >= (1ll << 31) || planes >= (1ull << 40))
    return dgs_fail_arg("maxpool3x3s2_ceil: sizes beyond the kernel's index arithmetic");
  const hipError_t e = launch_maxpool_ceil(in, (size_t)planes, IH, IW, out, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "maxpool3x3s2_ceil");
}

int dgs_conv2d_bias_relu(const float* in, int32_t n_img, int32_t Cin, int32_t IH, int32_t IW, const float* weight,
                         const float* bias, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t zscore,
                         float* out, dgs_stream_t stream) {
  if (in == nullptr || weight == nullptr || bias == nullptr || out == nullptr) return dgs_fail_arg("conv2d_bias_relu: null pointer");
  if (n_img < 1 || Cin < 1 || Cout < 1 || IH < 1 || IW < 1) return dgs_fail_arg("conv2d_bias_relu: empty input or output");
  if (KH < 1 || KW < 1 || KH > 15 || KW > 15 || stride < 1 || pad < 0 || pad >= KH || pad >= KW)
    return dgs_fail_arg("conv2d_bias_relu: kernel sizes are 1..15, stride >= 1, 0 <= pad < kernel size");
  if (zscore != 0 && (zscore != 1 || Cin != 3)) return dgs_fail_arg("conv2d_bias_relu: zscore is 0 or 1, and 1 needs Cin = 3");
  if (IH + 2 * (int64_t)pad < KH || IW + 2 * (int64_t)pad < KW) return dgs_fail_arg("conv2d_bias_relu: image smaller than the kernel");
  const int64_t OH = (IH + 2 * (int64_t)pad - KH) / stride + 1, OW = (IW + 2 * (int64_t)pad - KW) / stride + 1;
  if ((int64_t)Cin * IH * IW >= (1ll << 31) || (int64_t)Cin * KH * KW >= (1ll << 23) || (int64_t)n_img * OH * OW >= (1ll << 31) ||
      Cout > 65535 * 64)
    return dgs_fail_arg("conv2d_bias_relu: sizes beyond the kernel's 32-bit index arithmetic");
  ConvArgs g;
  g.in0 = in;
  g.in1 = in;
  g.n_half = n_img;
  g.w = weight;
  g.bias = bias;
  g.out = out;
  g.Cin = Cin, g.IH = IH, g.IW = IW, g.Cout = Cout, g.OH = (int)OH, g.OW = (int)OW;
  g.KH = KH, g.KW = KW, g.stride = stride, g.pad = pad, g.K = Cin * KH * KW, g.N = (int)(n_img * OH * OW);
  const hipError_t e = launch_conv(g, zscore != 0, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "conv2d_bias_relu");
}

int dgs_conv3x3_bias_relu(const float* in, int32_t n_img, int32_t Cin, int32_t IH, int32_t IW, const float* weight,
                          const float* bias, int32_t Cout, int32_t zscore, float* out, dgs_stream_t stream) {
  if (in == nullptr || weight == nullptr || bias == nullptr || out == nullptr) return dgs_fail_arg("conv3x3_bias_relu: null pointer");
  if (n_img < 1 || Cin < 1 || Cout < 1 || IH < 1 || IW < 1) return dgs_fail_arg("conv3x3_bias_relu: empty input or output");
  if (zscore != 0 && (zscore != 1 || Cin != 3)) return dgs_fail_arg("conv3x3_bias_relu: zscore is 0 or 1, and 1 needs Cin = 3");
  if ((int64_t)Cin * IH * IW >= (1ll << 31) || (int64_t)Cout * IH * IW >= (1ll << 31) || (int64_t)Cin * 9 >= (1ll << 23) ||
      (int64_t)n_img * IH * IW >= (1ll << 31) || conv3x3_tiles(n_img, IH, IW) >= ((size_t)1 << 31) || Cout > 65535 * 64)
    return dgs_fail_arg("conv3x3_bias_relu: sizes beyond the kernel's 32-bit index arithmetic");
  ConvArgs g;
  g.in0 = in;
  g.in1 = in;
  g.n_half = n_img;
  g.w = weight;
  g.bias = bias;
  g.out = out;
  g.Cin = Cin, g.IH = IH, g.IW = IW, g.Cout = Cout, g.OH = IH, g.OW = IW;
  g.KH = 3, g.KW = 3, g.stride = 1, g.pad = 1, g.K = Cin * 9, g.N = n_img * IH * IW;
  const hipError_t e = launch_conv3x3(g, n_img, zscore != 0, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "conv3x3_bias_relu");
}

int dgs_maxpool2x2(const float* in, uint64_t planes, int32_t IH, int32_t IW, float* out, dgs_stream_t stream) {
  if (in == nullptr || out == nullptr) return dgs_fail_arg("maxpool2x2: null pointer");
  if (planes < 1 || IH < 2 || IW < 2) return dgs_fail_arg("maxpool2x2: no planes, or planes below 2 x 2");
  if ((int64_t)IH * IW >= (1ll << 31) || planes >= (1ull << 40)) return dgs_fail_arg("maxpool2x2: sizes beyond the kernel's index arithmetic");
  const hipError_t e = launch_maxpool2x2(in, (size_t)planes, IH, IW, out, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "maxpool2x2");
}

// ---- the three backbones: scratch sizes, and the entry points that flatten their weight structs for lpips_run
size_t dgs_lpips_alex_tmp_bytes(int32_t W, int32_t H, int32_t n_pairs) {
  LpipsPlan P;
  return lpips_plan(ALEX, W, H, n_pairs, P) ? P.total_bytes : 0;
}

size_t dgs_lpips_vgg_tmp_bytes(int32_t W, int32_t H, int32_t n_pairs) {
  LpipsPlan P;
  return lpips_plan(VGG, W, H, n_pairs, P) ? P.total_bytes : 0;
}

size_t dgs_lpips_squeeze_tmp_bytes(int32_t W, int32_t H, int32_t n_pairs) {
  LpipsPlan P;
  return lpips_plan(SQUEEZE, W, H, n_pairs, P) ? P.total_bytes : 0;
}

int dgs_lpips_alex(const float* a, const float* b, int32_t n_pairs, int32_t W, int32_t H, const DgsLpipsAlexWeights* w,
                   void* tmp, float* out, dgs_stream_t stream) {
  LpipsWeights f;
  for (int l = 0; w != nullptr && l < 5; l++) f.layer[l][0] = w->conv_w[l], f.layer[l][1] = w->conv_b[l], f.lin[l] = w->lin[l];
  return lpips_run(ALEX, a, b, n_pairs, W, H, w != nullptr ? &f : nullptr, tmp, out, stream);
}

int dgs_lpips_vgg(const float* a, const float* b, int32_t n_pairs, int32_t W, int32_t H, const DgsLpipsVggWeights* w, void* tmp,
                  float* out, dgs_stream_t stream) {
  LpipsWeights f;
  for (int l = 0; w != nullptr && l < 13; l++) f.layer[l][0] = w->conv_w[l], f.layer[l][1] = w->conv_b[l];
  for (int t = 0; w != nullptr && t < 5; t++) f.lin[t] = w->lin[t];
  return lpips_run(VGG, a, b, n_pairs, W, H, w != nullptr ? &f : nullptr, tmp, out, stream);
}

int dgs_lpips_squeeze(const float* a, const float* b, int32_t n_pairs, int32_t W, int32_t H, const DgsLpipsSqueezeWeights* w,
                      void* tmp, float* out, dgs_stream_t stream) {
  LpipsWeights f;
  if (w != nullptr) {
    f.layer[0][0] = w->conv_w, f.layer[0][1] = w->conv_b;
    for (int i = 0; i < 8; i++) {
      const DgsFireWeights& m = w->fire[i];
      const float* six[6] = {m.squeeze_w, m.squeeze_b, m.expand1_w, m.expand1_b, m.expand3_w, m.expand3_b};
      for (int j = 0; j < 6; j++) f.layer[1 + i][j] = six[j];
    }
    for (int t = 0; t < 7; t++) f.lin[t] = w->lin[t];
  }
  return lpips_run(SQUEEZE, a, b, n_pairs, W, H, w != nullptr ? &f : nullptr, tmp, out, stream);
}

}  // extern "C"

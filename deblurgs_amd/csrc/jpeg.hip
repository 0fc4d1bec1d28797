// jpeg.hip -- finished baseline .jpg files from 8-bit images on the device (deblurgs_amd/jpeg.py, deblurgs_amd/video.py).
//
// dgs_jpeg_encode turns n images u8 [h,w,c] (c = 1 gray, c = 3 RGB) into n complete JFIF files -- SOI, APP0, DQT, SOF0, four
// DHT, DRI, SOS, the scan with one restart interval per MCU row, EOI -- in two launches on the caller's stream.  Integers
// only; include/dgs_hip.h states the arithmetic, tests/jpeg_cases.py restates it in numpy and the bytes are equal.
//
//   1 jpeg_row_kernel       one block of 256 threads per (image, MCU row): the restart interval, which starts byte-aligned
//                           with DC predictors 0 and so depends on no other block.  The row is taken JPEG_UNIT MCUs at a time
//                           (32; 16 at 4:2:0: 256 pixels either way, at most 96 blocks of 8 x 8):
//                             colour     a thread per pixel: Y Cb Cr in 16-bit fixed point into three LDS planes; a pixel
//                                        right of or below the image reads the last column / row (padding at full resolution)
//                             transform  a thread per (block, row), then per (block, column): two 8-term integer dot products
//                                        per output against the table M, in place in LDS as int16; 4:2:0 chroma samples are
//                                        the rounded mean of 2 x 2 taken while the row pass reads.  The column pass quantises:
//                                        (|F| + 4q) / 8q by a 32-bit reciprocal that is exact for these operands.
//                             lengths    a WAVE per block, a lane per zig-zag position: one __ballot gives the non-zero mask,
//                                        every lane finds the non-zero level before it with a count of leading zeros and so
//                                        knows its run, its ZRLs, its code and its bits alone; lane 0 codes the DC difference
//                                        (against the DC of the component's previous block, still in LDS), lane 63 the EOB.
//                                        A wave prefix sum gives the bit offsets inside the block, a second one over the
//                                        blocks' totals the offset of each block.
//                             packing    the same codes again, ORed (LDS atomicOr: any order) into a zeroed bit buffer,
//                                        most significant bit first.  The bits of the unit's last, incomplete byte are
//                                        carried into the next unit; the last unit is padded with 1-bits.
//                             stuffing   a thread per byte: 1 + (byte == 0xFF) output bytes, a block prefix sum, plain byte
//                                        stores into the row's slot in tmp.
//                           The row's byte count goes to tmp.
//   2 jpeg_assemble_kernel  one block per (image, MCU row): the sum of the byte counts of the rows before it (+ 2 each for
//                           their RST markers) is its offset; it copies its bytes (dword stores between a byte head and tail),
//                           appends RST(r & 7) or, after the last row, EOI and sizes[i].  The block of row 0 also writes the
//                           header.  Nothing past sizes[i] is written.
// No allocation, no host synchronisation, nothing kept between calls, no float, no global atomics: capturable.
#include "dgs_common.h"

namespace {

constexpr int JPEG_T = 256;
constexpr int JPEG_UNIT = 32;             // MCUs of a row a block takes at a time (JPEG_UNIT / 2 at 4:2:0)
constexpr int JPEG_UNIT_PX = 256;         // = JPEG_UNIT * 8 = JPEG_UNIT / 2 * 16
constexpr int JPEG_UNIT_BLOCKS = 96;      // 32 (gray), 32 * 3 (4:4:4), 16 * 6 (4:2:0)
// The longest code sequence of a block: a DC code of 11 bits (chroma category 11) + 11 magnitude bits, and 63 AC codes of
// 16 + 10 bits each: 22 + 63 * 26 = 1660 bits, 208 bytes when rounded up.  AC levels stay inside category 10: a row of M
// with u > 0 sums to zero, so its dot product with samples in -128..127 is at most 255 (sum |M| / 2) = 255 * 11584, which
// after the second pass against the all-positive row 0 gives |F| <= 8159 and |level| <= 1020 at q = 1; the DC level reaches
// -1024 and a DC difference 2040, category 11.
constexpr int JPEG_BLOCK_BYTES = 208;
constexpr int JPEG_BITBUF_WORDS = JPEG_UNIT_BLOCKS * JPEG_BLOCK_BYTES / 4 + 4;      // + the carried bits and a spill word
constexpr int JPEG_HEAD_RGB = 625;        // SOI 2, APP0 18, DQT 134, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
constexpr int JPEG_HEAD_GRAY = 334;       // SOI 2, APP0 18, DQT 69, SOF0 13, DHT 33 + 183, DRI 6, SOS 10

__constant__ uint8_t jpeg_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 and K.2, natural order
__constant__ uint8_t jpeg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61,  12, 12, 14, 19, 26, 58, 60, 55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51, 87, 80, 62,  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3 - K.6: codes per length 1..16 and the symbols in code order; [0] luma, [1] chroma
__constant__ uint8_t jpeg_dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                            {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
__constant__ uint8_t jpeg_ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                            {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
__constant__ uint8_t jpeg_ac_vals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct JpegArgs {
  const uint8_t* images;
  size_t image_stride;
  uint8_t* files;
  size_t file_stride;
  uint64_t* sizes;
  uint8_t* rows;            // [n, mrows] x row_slot stuffed bytes of the restart intervals (16-byte aligned)
  uint32_t* row_bytes;      // [n, mrows]
  size_t row_slot;
  int32_t w, h, c, quality;
  int32_t mcu;              // MCU side in pixels: 8, or 16 at 4:2:0
  int32_t bpm;              // blocks per MCU: 1, 3 or 6
  int32_t unit;             // MCUs per pass of the row kernel
  int32_t mcus_x, mrows, head;
};

// q of dgs_hip.h for table t (0 luma, 1 chroma) at natural index k
__device__ __forceinline__ uint32_t jpeg_quant(int quality, int t, int k) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int q = ((int)jpeg_base[t][k] * s + 50) / 100;
  return (uint32_t)(q < 1 ? 1 : (q > 255 ? 255 : q));
}

// M[u][x] = rint(8192 c(u) / 2 cos((2x + 1) u pi / 16)) (tests/test_jpeg_host.py holds the literals against the formula)
__device__ __forceinline__ void jpeg_dot8(const int (&s)[8], int (&o)[8], int round, int shift) {
  const int M[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,    //
                     4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,   //
                     3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,    //
                     3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,   //
                     2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,    //
                     2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,   //
                     1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,    //
                     799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
#pragma unroll
  for (int u = 0; u < 8; u++) {
    int acc = round;
#pragma unroll
    for (int x = 0; x < 8; x++) acc += M[u * 8 + x] * s[x];
    o[u] = acc >> shift;
  }
}

__device__ __forceinline__ uint32_t jpeg_wave_scan(uint32_t v) {
  const int lane = dgs_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, (unsigned)d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// what lane `lane` of a block's wave emits: nzrl ZRL codes, then nb bits of val (a code and its magnitude bits)
struct JpegLane {
  uint32_t val;
  int nb, nzrl;
};
// v: the level at zig-zag position `lane` (lane 0: the DC difference); mask: the non-zero AC positions
__device__ __forceinline__ JpegLane jpeg_lane_code(int lane, int v, unsigned long long mask, const uint32_t* dc,
                                                   const uint32_t* ac) {
  JpegLane c = {0u, 0, 0};
  const uint32_t mag = (uint32_t)(v < 0 ? -v : v);
  const int size = mag == 0u ? 0 : 32 - __clz((int)mag);
  const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
  if (lane == 0) {
    const uint32_t e = dc[size];
    c.val = ((e & 0xFFFFu) << size) | extra;
    c.nb = (int)(e >> 16) + size;
  } else if (v != 0) {
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int prev = below != 0ull ? 63 - __clzll((long long)below) : 0;
    const int run = lane - prev - 1;
    const uint32_t e = ac[((run & 15) << 4) | size];
    c.nzrl = run >> 4;
    c.val = ((e & 0xFFFFu) << size) | extra;
    c.nb = (int)(e >> 16) + size;
  } else if (lane == 63) {      // the last coefficient is zero: EOB
    const uint32_t e = ac[0];
    c.val = e & 0xFFFFu;
    c.nb = (int)(e >> 16);
  }
  return c;
}

// n bits (1..32) of val at bit `pos` of a stream whose first bit is bit 31 of word 0
__device__ __forceinline__ void jpeg_put(uint32_t* w, uint32_t pos, uint32_t val, int n) {
  const uint32_t i = pos >> 5;
  const int space = 32 - (int)(pos & 31u);
  if (n <= space) {
    atomicOr(&w[i], val << (space - n));
  } else {
    atomicOr(&w[i], val >> (n - space));
    atomicOr(&w[i + 1u], val << (32 - (n - space)));
  }
}
__device__ __forceinline__ uint32_t jpeg_byte(const uint32_t* w, uint32_t j) { return (w[j >> 2] >> (24u - 8u * (j & 3u))) & 255u; }

// ------------------------------------------------------------------------------------------- 1: one restart interval
__global__ void __launch_bounds__(JPEG_T)
jpeg_row_kernel(const JpegArgs a) {
  __shared__ uint8_t plane[3][JPEG_UNIT_PX * 16];
  __shared__ int16_t lev[JPEG_UNIT_BLOCKS * 64];
  __shared__ uint32_t bits[JPEG_BITBUF_WORDS];
  __shared__ uint32_t ac_tab[2][256], dc_tab[2][16], qmagic[2][64];
  __shared__ uint16_t qv[2][64];
  __shared__ uint32_t blen[JPEG_UNIT_BLOCKS], boff[JPEG_UNIT_BLOCKS], wtot[JPEG_T / 64];
  __shared__ int pred[3];
  __shared__ uint32_t sh_total, sh_carry;
  const int tid = (int)threadIdx.x, lane = dgs_lane(), wave = tid >> 6;
  const uint32_t img = blockIdx.x / (uint32_t)a.mrows, mrow = blockIdx.x % (uint32_t)a.mrows;
  const uint8_t* image = a.images + (size_t)img * a.image_stride;
  uint8_t* out = a.rows + ((size_t)img * a.mrows + mrow) * a.row_slot;
  const int bpm = a.bpm, mcu = a.mcu;

  // ---- tables: canonical codes as length << 16 | code, quantisers and their reciprocals
  for (int i = tid; i < 512; i += JPEG_T) ac_tab[i >> 8][i & 255] = 0u;
  for (int i = tid; i < JPEG_BITBUF_WORDS; i += JPEG_T) bits[i] = 0u;
  if (tid < 128) {
    const uint32_t q = jpeg_quant(a.quality, tid >> 6, tid & 63);
    qv[tid >> 6][tid & 63] = (uint16_t)q;
    // floor(n / d) = (n m) >> 32 with m = floor(2^32 / d) + 1 while n d < 2^32: here n < 2^14 and d = 8q <= 2040
    qmagic[tid >> 6][tid & 63] = (uint32_t)(0x100000000ull / (8u * q)) + 1u;
  }
  if (tid < 3) pred[tid] = 0;
  __syncthreads();
  if (tid < 4) {
    const int t = tid & 1, is_ac = tid >> 1;
    const uint8_t* nb = is_ac ? jpeg_ac_bits[t] : jpeg_dc_bits[t];
    uint32_t code = 0u;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
      for (int i = 0; i < (int)nb[len - 1]; i++, k++, code++) {
        if (is_ac) ac_tab[t][jpeg_ac_vals[t][k]] = ((uint32_t)len << 16) | code;
        else dc_tab[t][k] = ((uint32_t)len << 16) | code;      // (the DC symbols are 0..11 in code order)
      }
      code <<= 1;
    }
  }
  __syncthreads();

  uint32_t cbits = 0u;          // bits of an incomplete byte carried over from the unit before
  uint32_t used_words = 0u;     // words of the bit buffer to clear before the next unit
  uint32_t outpos = 0u;
  for (int m0 = 0; m0 < a.mcus_x; m0 += a.unit) {
    const int nm = a.mcus_x - m0 < a.unit ? a.mcus_x - m0 : a.unit;
    const int nblk = nm * bpm, pw = nm * mcu;

    // ---- colour: pixels past the right or bottom edge read the last column / row
    for (int i = tid; i < JPEG_UNIT_PX * mcu; i += JPEG_T) {
      const int y = i >> 8, x = i & 255;
      if (x < pw) {
        const int gx = m0 * mcu + x, gy = (int)mrow * mcu + y;
        const uint8_t* p = image + ((size_t)(gy < a.h ? gy : a.h - 1) * (size_t)a.w + (size_t)(gx < a.w ? gx : a.w - 1)) * (size_t)a.c;
        if (a.c == 1) {
          plane[0][i] = p[0];
        } else {
          const int R = p[0], G = p[1], B = p[2];
          const int cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
          const int cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
          plane[0][i] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
          plane[1][i] = (uint8_t)(cb < 0 ? 0 : (cb > 255 ? 255 : cb));
          plane[2][i] = (uint8_t)(cr < 0 ? 0 : (cr > 255 ? 255 : cr));
        }
      }
    }
    for (uint32_t i = (uint32_t)tid; i < used_words; i += JPEG_T) bits[i] = 0u;
    __syncthreads();
    if (tid == 0 && cbits != 0u) bits[0] = sh_carry << (32u - cbits);

    // ---- row pass: t[y][u] = (sum_x M[u][x] (sample - 128) + 512) >> 10
    for (int task = tid; task < nblk * 8; task += JPEG_T) {
      const int b = task >> 3, r = task & 7, mi = b / bpm, j = b - mi * bpm;
      int s[8], o[8];
      if (bpm == 6 && j >= 4) {         // 4:2:0 chroma: the rounded mean of 2 x 2
        const uint8_t* p = plane[j - 3] + (2 * r) * JPEG_UNIT_PX + mi * 16;
#pragma unroll
        for (int x = 0; x < 8; x++)
          s[x] = ((p[2 * x] + p[2 * x + 1] + p[JPEG_UNIT_PX + 2 * x] + p[JPEG_UNIT_PX + 2 * x + 1] + 2) >> 2) - 128;
      } else {
        const uint8_t* p = bpm == 6 ? plane[0] + ((j >> 1) * 8 + r) * JPEG_UNIT_PX + mi * 16 + (j & 1) * 8
                                    : plane[j] + r * JPEG_UNIT_PX + mi * 8;
#pragma unroll
        for (int x = 0; x < 8; x++) s[x] = (int)p[x] - 128;
      }
      jpeg_dot8(s, o, 512, 10);
#pragma unroll
      for (int u = 0; u < 8; u++) lev[b * 64 + r * 8 + u] = (int16_t)o[u];
    }
    __syncthreads();
    // ---- column pass, in place: F[v][u] = (sum_y M[v][y] t[y][u] + 4096) >> 13, level = sign(F) (|F| + 4q) / 8q
    for (int task = tid; task < nblk * 8; task += JPEG_T) {
      const int b = task >> 3, u = task & 7, j = b % bpm;
      const int t = (bpm == 1 || j == 0 || (bpm == 6 && j < 4)) ? 0 : 1;
      int s[8], o[8];
#pragma unroll
      for (int y = 0; y < 8; y++) s[y] = lev[b * 64 + y * 8 + u];
      jpeg_dot8(s, o, 4096, 13);
#pragma unroll
      for (int v = 0; v < 8; v++) {
        const int F = o[v];
        const uint32_t n = (uint32_t)(F < 0 ? -F : F) + 4u * qv[t][v * 8 + u];
        const int l = (int)__umulhi(n, qmagic[t][v * 8 + u]);
        lev[b * 64 + v * 8 + u] = (int16_t)(F < 0 ? -l : l);
      }
    }
    __syncthreads();

    // ---- a wave per block, a lane per zig-zag position: the bits of the block, then the codes themselves
    for (int pass = 0; pass < 2; pass++) {
      for (int b = wave; b < nblk; b += JPEG_T / 64) {
        const int mi = b / bpm, j = b - mi * bpm;
        const int comp = bpm == 1 ? 0 : (bpm == 3 ? j : (j < 4 ? 0 : j - 3));
        const int t = comp == 0 ? 0 : 1;
        int v = lev[b * 64 + jpeg_zigzag[lane]];
        if (lane == 0) {
          const bool first = mi == 0 && (bpm != 6 || j == 0 || j >= 4);
          const int back = bpm == 1 ? 1 : (bpm == 3 ? 3 : (j >= 4 ? 6 : (j > 0 ? 1 : 3)));
          v -= first ? pred[comp] : (int)lev[(b - back) * 64];
        }
        const unsigned long long mask = __ballot(lane != 0 && v != 0);
        const JpegLane c = jpeg_lane_code(lane, v, mask, dc_tab[t], ac_tab[t]);
        const uint32_t zrl = ac_tab[t][0xF0];
        const uint32_t nbits = (uint32_t)c.nzrl * (zrl >> 16) + (uint32_t)c.nb;
        const uint32_t incl = jpeg_wave_scan(nbits);
        if (pass == 0) {
          if (lane == 63) blen[b] = incl;
        } else {
          uint32_t pos = boff[b] + incl - nbits;
          for (int z = 0; z < c.nzrl; z++, pos += zrl >> 16) jpeg_put(bits, pos, zrl & 0xFFFFu, (int)(zrl >> 16));
          if (c.nb != 0) jpeg_put(bits, pos, c.val, c.nb);
        }
      }
      __syncthreads();
      if (pass == 0) {
        if (wave == 0) {        // exclusive prefix sum over the (at most 96) blocks
          const uint32_t v0 = lane < nblk ? blen[lane] : 0u, v1 = lane + 64 < nblk ? blen[lane + 64] : 0u;
          const uint32_t s0 = jpeg_wave_scan(v0), s1 = jpeg_wave_scan(v1);
          const uint32_t t0 = __shfl(s0, 63, 64);
          if (lane < nblk) boff[lane] = cbits + s0 - v0;
          if (lane + 64 < nblk) boff[lane + 64] = cbits + t0 + s1 - v1;
          if (lane == 63) sh_total = cbits + t0 + s1;
        }
        __syncthreads();
      }
    }
    // (all lengths and codes are read: the levels may go, but first the predictors of the next unit)
    uint32_t totbits = sh_total;
    const bool last = m0 + a.unit >= a.mcus_x;
    if (tid == 0) {
      for (int cc = 0; cc < (bpm == 1 ? 1 : 3); cc++) pred[cc] = lev[(bpm == 1 ? nblk - 1 : nblk - 3 + cc) * 64];
      const uint32_t pad = (8u - (totbits & 7u)) & 7u;
      if (last && pad != 0u) jpeg_put(bits, totbits, (1u << pad) - 1u, (int)pad);
    }
    if (last) totbits = (totbits + 7u) & ~7u;
    const uint32_t nfull = totbits >> 3;
    __syncthreads();
    cbits = totbits & 7u;
    if (tid == 0 && cbits != 0u) sh_carry = jpeg_byte(bits, nfull) >> (8u - cbits);

    // ---- byte stuffing: 0xFF is followed by 0x00
    for (uint32_t base = 0u; base < nfull; base += JPEG_T) {
      const uint32_t jb = base + (uint32_t)tid;
      const uint32_t byte = jb < nfull ? jpeg_byte(bits, jb) : 0u;
      const uint32_t cnt = jb < nfull ? (byte == 255u ? 2u : 1u) : 0u;
      uint32_t incl = jpeg_wave_scan(cnt);
      if (lane == 63) wtot[wave] = incl;
      __syncthreads();
      uint32_t all = 0u;
      for (int u = 0; u < JPEG_T / 64; u++) {
        if (u < wave) incl += wtot[u];
        all += wtot[u];
      }
      if (cnt != 0u) {
        out[outpos + incl - cnt] = (uint8_t)byte;
        if (cnt == 2u) out[outpos + incl - 1u] = 0;
      }
      outpos += all;
      __syncthreads();
    }
    used_words = (totbits + 63u) >> 5;
    __syncthreads();
  }
  if (tid == 0) a.row_bytes[(size_t)img * a.mrows + mrow] = outpos;
}

// ------------------------------------------------------------------------------------------- 2: header, rows, markers
__device__ __forceinline__ int jpeg_marker(uint8_t* p, int at, int marker, int length) {
  p[at] = 0xFF;
  p[at + 1] = (uint8_t)marker;
  p[at + 2] = (uint8_t)(length >> 8);
  p[at + 3] = (uint8_t)length;
  return at + 4;
}

__device__ int jpeg_write_header(uint8_t* p, const JpegArgs& a) {
  const int nc = a.c == 1 ? 1 : 3;
  int at = 0;
  p[at++] = 0xFF;
  p[at++] = 0xD8;
  at = jpeg_marker(p, at, 0xE0, 16);
  const uint8_t app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 14; i++) p[at++] = app0[i];
  at = jpeg_marker(p, at, 0xDB, 2 + 65 * (nc == 1 ? 1 : 2));
  for (int t = 0; t < (nc == 1 ? 1 : 2); t++) {
    p[at++] = (uint8_t)t;
    for (int k = 0; k < 64; k++) p[at++] = (uint8_t)jpeg_quant(a.quality, t, jpeg_zigzag[k]);
  }
  at = jpeg_marker(p, at, 0xC0, 8 + 3 * nc);
  p[at++] = 8;
  p[at++] = (uint8_t)(a.h >> 8);
  p[at++] = (uint8_t)a.h;
  p[at++] = (uint8_t)(a.w >> 8);
  p[at++] = (uint8_t)a.w;
  p[at++] = (uint8_t)nc;
  for (int cc = 0; cc < nc; cc++) {
    p[at++] = (uint8_t)(cc + 1);
    p[at++] = (cc == 0 && a.bpm == 6) ? 0x22 : 0x11;
    p[at++] = cc == 0 ? 0 : 1;
  }
  for (int t = 0; t < (nc == 1 ? 1 : 2); t++) {
    at = jpeg_marker(p, at, 0xC4, 2 + 1 + 16 + 12);
    p[at++] = (uint8_t)t;
    for (int i = 0; i < 16; i++) p[at++] = jpeg_dc_bits[t][i];
    for (int i = 0; i < 12; i++) p[at++] = (uint8_t)i;
    at = jpeg_marker(p, at, 0xC4, 2 + 1 + 16 + 162);
    p[at++] = (uint8_t)(0x10 | t);
    for (int i = 0; i < 16; i++) p[at++] = jpeg_ac_bits[t][i];
    for (int i = 0; i < 162; i++) p[at++] = jpeg_ac_vals[t][i];
  }
  at = jpeg_marker(p, at, 0xDD, 4);
  p[at++] = (uint8_t)(a.mcus_x >> 8);
  p[at++] = (uint8_t)a.mcus_x;
  at = jpeg_marker(p, at, 0xDA, 6 + 2 * nc);
  p[at++] = (uint8_t)nc;
  for (int cc = 0; cc < nc; cc++) {
    p[at++] = (uint8_t)(cc + 1);
    p[at++] = cc == 0 ? 0x00 : 0x11;
  }
  p[at++] = 0;
  p[at++] = 63;
  p[at++] = 0;
  return at;
}

__global__ void __launch_bounds__(JPEG_T)
jpeg_assemble_kernel(const JpegArgs a) {
  __shared__ unsigned long long sh_before;
  __shared__ uint8_t hdr[640];
  const uint32_t tid = threadIdx.x;
  const uint32_t img = blockIdx.x / (uint32_t)a.mrows, mrow = blockIdx.x % (uint32_t)a.mrows;
  const uint32_t* row_bytes = a.row_bytes + (size_t)img * a.mrows;
  uint8_t* file = a.files + (size_t)img * a.file_stride;
  if (tid == 0u) sh_before = 0ull;
  __syncthreads();
  unsigned long long before = 0ull;
  for (uint32_t r = tid; r < mrow; r += JPEG_T) before += (unsigned long long)row_bytes[r] + 2ull;
  if (before != 0ull) atomicAdd(&sh_before, before);      // (an LDS integer sum: any order)
  if (mrow == 0u && tid == 0u) jpeg_write_header(hdr, a);
  __syncthreads();
  if (mrow == 0u)
    for (uint32_t i = tid; i < (uint32_t)a.head; i += JPEG_T) file[i] = hdr[i];
  const uint32_t nb = row_bytes[mrow];
  const uint8_t* src = a.rows + ((size_t)img * a.mrows + mrow) * a.row_slot;
  const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
  uint8_t* dst = file + (size_t)a.head + (size_t)sh_before;
  uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
  if (head > nb) head = nb;
  const uint32_t nd = (nb - head) >> 2;
  const uint32_t tail0 = head + 4u * nd;
  if (tid < head) dst[tid] = src[tid];
  if (tid < nb - tail0) dst[tail0 + tid] = src[tail0 + tid];
  const uint32_t sh = 8u * head;
  uint32_t* dstw = reinterpret_cast<uint32_t*>(dst + head);
  for (uint32_t q = tid; q < nd; q += JPEG_T) {       // (srcw[q + 1] stays inside the slot: it ends with 16 spare bytes)
    const uint32_t lo = srcw[q];
    dstw[q] = sh == 0u ? lo : (lo >> sh) | (srcw[q + 1u] << (32u - sh));
  }
  if (tid == 0u) {
    dst[nb] = 0xFF;
    if (mrow + 1u < (uint32_t)a.mrows) {
      dst[nb + 1u] = (uint8_t)(0xD0u + (mrow & 7u));
    } else {
      dst[nb + 1u] = 0xD9;
      a.sizes[img] = (uint64_t)a.head + sh_before + nb + 2ull;
    }
  }
}

// ------------------------------------------------------------------------------------------- host
struct JpegGeometry {
  int32_t mcu, bpm, unit, mcus_x, mrows, head;
  uint64_t blocks;      // of one image
  uint64_t row_slot;    // tmp bytes of one restart interval
};

inline bool jpeg_geometry(int32_t w, int32_t h, int32_t c, int32_t subsampling, JpegGeometry& g) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || (c != 1 && c != 3)) return false;
  if (subsampling != DGS_JPEG_444 && subsampling != DGS_JPEG_420) return false;
  const bool s420 = c == 3 && subsampling == DGS_JPEG_420;
  g.mcu = s420 ? 16 : 8;
  g.bpm = c == 1 ? 1 : (s420 ? 6 : 3);
  g.unit = s420 ? JPEG_UNIT / 2 : JPEG_UNIT;
  g.mcus_x = (w + g.mcu - 1) / g.mcu;
  g.mrows = (h + g.mcu - 1) / g.mcu;
  g.head = c == 1 ? JPEG_HEAD_GRAY : JPEG_HEAD_RGB;
  g.blocks = (uint64_t)g.mcus_x * (uint64_t)g.mrows * (uint64_t)g.bpm;
  g.row_slot = (uint64_t)g.mcus_x * (uint64_t)g.bpm * (2ull * JPEG_BLOCK_BYTES) + 16ull;      // a multiple of 16
  return true;
}

}  // namespace

extern "C" {

// The header, then per block the longest code sequence (1660 bits, rounded up to 208 bytes: a row is padded to a byte once,
// so its bytes are at most the sum of its blocks' rounded bytes) doubled because every byte may be 0xFF and take a 0x00,
// then two bytes per MCU row (its RST marker; the last row has none, which leaves room for EOI):
//   625 (334 gray) + 416 blocks + 2 MCU rows + 2
size_t dgs_jpeg_bound(int32_t w, int32_t h, int32_t channels, int32_t subsampling) {
  JpegGeometry g;
  if (!jpeg_geometry(w, h, channels, subsampling, g)) return 0;
  return (size_t)((uint64_t)g.head + 2ull * JPEG_BLOCK_BYTES * g.blocks + 2ull * (uint64_t)g.mrows + 2ull);
}

size_t dgs_jpeg_tmp_bytes(int32_t n, int32_t w, int32_t h, int32_t channels, int32_t subsampling) {
  JpegGeometry g;
  if (n < 0 || !jpeg_geometry(w, h, channels, subsampling, g)) return 0;
  // (n < 2^31, mrows < 2^13, row_slot < 2^24: below 2^63)
  return (size_t)(32ull + (uint64_t)n * (uint64_t)g.mrows * (g.row_slot + 4ull));
}

int dgs_jpeg_encode(const uint8_t* images, int32_t n, int32_t w, int32_t h, int32_t channels, size_t image_stride,
                    int32_t quality, int32_t subsampling, uint8_t* files, size_t file_stride, uint64_t* sizes, void* tmp,
                    dgs_stream_t stream) {
  if (channels != 1 && channels != 3) return dgs_fail_arg("jpeg_encode: channels must be 1 or 3");
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return dgs_fail_arg("jpeg_encode: w and h must be 1..65535");
  if (subsampling != DGS_JPEG_444 && subsampling != DGS_JPEG_420)
    return dgs_fail_arg("jpeg_encode: subsampling must be DGS_JPEG_444 or DGS_JPEG_420");
  if (quality < 1 || quality > 100) return dgs_fail_arg("jpeg_encode: quality must be 1..100");
  if (n < 0) return dgs_fail_arg("jpeg_encode: n must not be negative");
  if (n == 0) return DGS_OK;
  if (images == nullptr || files == nullptr || sizes == nullptr || tmp == nullptr)
    return dgs_fail_arg("jpeg_encode: null pointer");
  JpegGeometry g;
  jpeg_geometry(w, h, channels, subsampling, g);
  if ((uint64_t)image_stride < (uint64_t)h * (uint64_t)w * (uint64_t)channels)
    return dgs_fail_arg("jpeg_encode: image_stride is below h w channels");
  if ((uint64_t)file_stride < (uint64_t)dgs_jpeg_bound(w, h, channels, subsampling))
    return dgs_fail_arg("jpeg_encode: file_stride is below dgs_jpeg_bound");
  if ((reinterpret_cast<uintptr_t>(sizes) & 7u) != 0) return dgs_fail_arg("jpeg_encode: sizes must be 8-byte aligned");
  if ((uint64_t)n * (uint64_t)g.mrows > 0x7fffffffull) return dgs_fail_arg("jpeg_encode: more than 2^31 - 1 blocks");
  JpegArgs a;
  a.images = images;
  a.image_stride = image_stride;
  a.files = files;
  a.file_stride = file_stride;
  a.sizes = sizes;
  a.rows = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(tmp) + 15u) & ~(uintptr_t)15u);
  a.row_slot = (size_t)g.row_slot;
  a.row_bytes = reinterpret_cast<uint32_t*>(a.rows + (size_t)n * (size_t)g.mrows * a.row_slot);
  a.w = w;
  a.h = h;
  a.c = channels;
  a.quality = quality;
  a.mcu = g.mcu;
  a.bpm = g.bpm;
  a.unit = g.unit;
  a.mcus_x = g.mcus_x;
  a.mrows = g.mrows;
  a.head = g.head;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((uint32_t)((uint64_t)n * (uint64_t)g.mrows));
  hipLaunchKernelGGL(jpeg_row_kernel, grid, dim3(JPEG_T), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "jpeg_encode (rows)");
  hipLaunchKernelGGL(jpeg_assemble_kernel, grid, dim3(JPEG_T), 0, st, a);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "jpeg_encode (assemble)");
}

}  // extern "C"

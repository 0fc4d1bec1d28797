// png.hip -- finished .png files from 8-bit images on the device (deblurgs_amd/png.py): row filters, deflate, checksums.
//
// dgs_png_encode turns n images u8 [h,w,c] into n complete files -- signature, IHDR, ONE IDAT holding a zlib stream, IEND,
// every CRC -- in four launches on the caller's stream; the host reads sizes[i] and copies that many bytes.  Integers only.
//
//   1 png_filter_kernel    one block of 256 threads per image row.  The row and the row above it are read with 16-byte loads
//                          (byte loads at a misaligned head and tail) into LDS, FILTER_CH bytes at a time; every thread forms
//                          the five PNG candidates (None, Sub, Up, Average, Paeth; bpp = c, the row above row 0 is zeros) of
//                          its bytes and adds |residual as int8| into five 64-bit LDS sums (integer adds: any order).  The
//                          smallest sum wins, the lowest filter type on a tie.  A second pass over the same LDS bytes (rows
//                          wider than FILTER_CH are loaded again) writes the filter byte and the residuals into the filtered
//                          stream, F = h (1 + w c) bytes per image in tmp, as dwords staged in LDS.
//   2 png_deflate_kernel   one block of DGS_PNG_SEGMENT / 64 threads per segment of DGS_PNG_SEGMENT filtered bytes; a
//                          segment never refers to a byte before it.  Tokens are zlib's Z_RLE: a literal, then matches of
//                          distance 1 and length 3..258 while the byte repeats, a tail shorter than 3 as literals.
//                            run flags     byte != previous byte, one __ballot (64-bit mask) per 64 positions, kept in LDS;
//                                          one thread per mask word then scans (max forwards, min backwards) for the nearest
//                                          run start before / after each word, so every position finds its run's start and
//                                          end from two words and decides ITS token alone: none, a literal or a match.
//                            histogram     LDS integer adds, per SEGMENT (a code per segment, not per image: no second
//                                          pass over the image and no dependency between blocks).
//                            codes         the used symbols are ranked by (count, symbol) in parallel; ONE lane builds the
//                                          minimum-redundancy lengths in place (Moffat & Katajainen), limits them to 15 bits
//                                          by the count-per-length adjustment (complete by construction: it stops when the
//                                          Kraft sum is exactly 2^15), assigns canonical codes, run-length codes the lengths
//                                          (symbols 16 / 17 / 18), builds the 7-bit-limited code-length code the same way and
//                                          writes the block header.  The distance code is one code of length 1.
//                            offsets       bits per position -> wave prefix sums (__shfl_up) -> one block prefix sum over
//                                          the waves' totals.
//                            packing       atomicOr into zeroed LDS words (an OR: any order); no position is claimed by a
//                                          counter.
//                          A segment whose compressed form, marker included, is not smaller than 5 + len becomes a stored
//                          block.  A non-final compressed segment ends with an empty stored block (000, pad, 00 00 FF FF) so
//                          that the next starts on a byte; the last block of the image carries BFINAL.  The block also leaves
//                          the segment's byte count, the raw CRC-32 remainder of its output bytes and its Adler-32 pair
//                          (sum d, sum (len - i) d) in tmp.
//   3 png_assemble_kernel  one block per image: prefix sum of the byte counts; Adler-32 of the filtered stream as
//                          A = 1 + sum a_s, B = F + sum (b_s + after_s a_s) mod 65521; the IDAT CRC by the combine rule --
//                          each segment's remainder times x^(8 bytes after it) mod the polynomial, XORed (CRC without its
//                          initial and final inversion is linear; the inversion is added as 0xFFFFFFFF x^(8 n)) -- then the
//                          signature, IHDR, the IDAT frame, Adler, CRCs, IEND and the file size as a uint64.
//   4 png_copy_kernel      one block per segment copies its bytes behind the zlib header (dword stores between a byte head
//                          and tail: nothing past sizes[i] is written).
// No allocation, no host synchronisation, nothing kept between calls, no float, no float atomics: capturable.
#include "dgs_common.h"

#include <stdio.h>

namespace {

constexpr int PNG_S = DGS_PNG_SEGMENT;
constexpr int PNG_T = PNG_S / 64;          // threads of a deflate block: one per 64-bit word of run flags
constexpr int PNG_NWAVE = PNG_T / 64;
// (a stored block holds at most 65535 bytes and a block at most 1024 threads: 65536 would need two stored blocks a segment)
static_assert(PNG_S == 16384 || PNG_S == 32768, "DGS_PNG_SEGMENT must be 16384 or 32768");
constexpr int PNG_SLOT = PNG_S + 16;       // tmp bytes per segment's output: 5 + PNG_S and a dword of slack, 16-byte multiple
constexpr int PNG_OUT_WORDS = PNG_SLOT / 4;
constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr int FILTER_T = 256;
constexpr int FILTER_CH = 16384;           // row bytes staged in LDS at a time
constexpr int PNG_HEAD = 43;               // signature 8 + IHDR 25 + IDAT length and type 8 + zlib header 2
constexpr int PNG_LITLEN = 286;

// ------------------------------------------------------------------------------------------- CRC-32 as polynomial algebra
// reflected representation: bit 31 is x^0.  a * b mod P.
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
  }
  return p;
}
// x^(8 nbytes) mod P
__host__ __device__ inline uint32_t crc_xpow8(uint64_t nbytes) {
  uint64_t e = nbytes * 8u;
  uint32_t r = 0x80000000u, base = 0x40000000u;
  while (e != 0) {
    if (e & 1u) r = crc_mul(r, base);
    base = crc_mul(base, base);
    e >>= 1;
  }
  return r;
}
// one byte into the raw remainder (no initial or final inversion: linear in the message)
__host__ __device__ inline uint32_t crc_byte(uint32_t c, uint32_t byte) {
  c ^= byte;
  for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
  return c;
}
// the CRC-32 of a message of n bytes from its raw remainder
__host__ __device__ inline uint32_t crc_finish(uint32_t raw, uint64_t n) {
  return raw ^ crc_mul(0xFFFFFFFFu, crc_xpow8(n)) ^ 0xFFFFFFFFu;
}

// ------------------------------------------------------------------------------------------- code construction (one lane)
struct CodeWork {
  uint32_t freq[288];       // literal/length histogram of the segment
  uint32_t A[288];          // counts in rank order, then lengths (in place)
  uint16_t order[288];      // symbols by (count, symbol) ascending
  uint16_t code[288];       // canonical codes, bit-reversed (deflate packs codes from their most significant bit)
  uint8_t len[288];
  uint32_t cl_freq[19];
  uint16_t cl_code[19];
  uint8_t cl_len[19];
  uint8_t seq_sym[296];     // the run-length coded code lengths: symbol and extra-bits value
  uint8_t seq_ext[296];
  int32_t n_seq;
  int32_t cnt[36];          // codes per length
  uint32_t next_code[17];
};

__host__ __device__ inline void put_bits(uint32_t* out, uint32_t& pos, uint32_t val, int n) {
  const uint64_t v = (uint64_t)val << (pos & 31u);
  out[pos >> 5] |= (uint32_t)v;
  if ((v >> 32) != 0) out[(pos >> 5) + 1] |= (uint32_t)(v >> 32);
  pos += (uint32_t)n;
}

__host__ __device__ inline uint32_t reverse_bits(uint32_t c, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; i++) r |= ((c >> i) & 1u) << (n - 1 - i);
  return r;
}

// Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": A holds n >= 2 counts in ascending order and
// leaves the code length of each (descending).
__host__ __device__ inline void min_redundancy(uint32_t* A, int n) {
  A[0] += A[1];
  int root = 0, leaf = 2, next;
  for (next = 1; next < n - 1; next++) {
    if (leaf >= n || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= n || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  A[n - 2] = 0;
  for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
  int avbl = 1, used = 0, dpth = 0;
  root = n - 2;
  next = n - 1;
  while (avbl > 0) {
    while (root >= 0 && (int)A[root] == dpth) {
      used++;
      root--;
    }
    while (avbl > used) {
      A[next--] = (uint32_t)dpth;
      avbl--;
    }
    avbl = 2 * used;
    dpth++;
    used = 0;
  }
}

// lengths of the n used symbols order[0..n) (counts A[0..n) ascending), limited to maxlen bits, complete: the Kraft sum of
// the clamped lengths is brought down to exactly 2^maxlen one unit at a time (a code of maxlen bits leaves, the longest
// shorter code splits in two).  len[] of unused symbols is left as it is (zero).
__host__ __device__ inline void limited_lengths(CodeWork& w, int n, int maxlen, uint8_t* len) {
  if (n == 1) {
    len[w.order[0]] = 1;
    return;
  }
  min_redundancy(w.A, n);
  for (int i = 0; i < 36; i++) w.cnt[i] = 0;
  for (int i = 0; i < n; i++) w.cnt[w.A[i] < 35u ? w.A[i] : 35u]++;
  for (int i = maxlen + 1; i < 36; i++) w.cnt[maxlen] += w.cnt[i];
  uint32_t total = 0;
  for (int i = maxlen; i > 0; i--) total += (uint32_t)w.cnt[i] << (maxlen - i);
  while (total > (1u << maxlen)) {      // (a Huffman code is complete: the clamped sum starts at or above 2^maxlen)
    w.cnt[maxlen]--;
    for (int i = maxlen - 1; i > 0; i--)
      if (w.cnt[i] != 0) {
        w.cnt[i]--;
        w.cnt[i + 1] += 2;
        break;
      }
    total--;
  }
  int j = n;
  for (int i = 1; i <= maxlen; i++)
    for (int l = w.cnt[i]; l > 0; l--) len[w.order[--j]] = (uint8_t)i;
}

__host__ __device__ inline void canonical_codes(CodeWork& w, const uint8_t* len, int nsym, int maxlen, uint16_t* code) {
  for (int i = 0; i <= maxlen; i++) w.cnt[i] = 0;
  for (int s = 0; s < nsym; s++) w.cnt[len[s]]++;
  w.cnt[0] = 0;
  uint32_t c = 0;
  for (int l = 1; l <= maxlen; l++) {
    c = (c + (uint32_t)w.cnt[l - 1]) << 1;
    w.next_code[l] = c;
  }
  for (int s = 0; s < nsym; s++)
    if (len[s] != 0) code[s] = (uint16_t)reverse_bits(w.next_code[len[s]]++, len[s]);
}

__host__ __device__ inline void seq_emit(CodeWork& w, int sym, int ext) {
  w.seq_sym[w.n_seq] = (uint8_t)sym;
  w.seq_ext[w.n_seq] = (uint8_t)ext;
  w.n_seq++;
  w.cl_freq[sym]++;
}

// w.freq and w.order[0..n_used) are set.  Builds both codes and writes the dynamic block's header into the zeroed words
// `out`; returns its length in bits.
__host__ __device__ inline uint32_t build_block_header(CodeWork& w, int n_used, bool final_block, uint32_t* out) {
  for (int i = 0; i < n_used; i++) w.A[i] = w.freq[w.order[i]];
  for (int s = 0; s < 288; s++) w.len[s] = 0;
  limited_lengths(w, n_used, 15, w.len);
  canonical_codes(w, w.len, PNG_LITLEN, 15, w.code);
  int hlit = PNG_LITLEN;
  while (hlit > 257 && w.len[hlit - 1] == 0) hlit--;
  // the hlit literal/length lengths and the one distance length (1), run-length coded as one sequence
  const int total = hlit + 1;
  w.n_seq = 0;
  for (int i = 0; i < 19; i++) {
    w.cl_freq[i] = 0;
    w.cl_len[i] = 0;
  }
  int i = 0;
  while (i < total) {
    const int v = i < hlit ? w.len[i] : 1;
    int run = 1;
    while (i + run < total && (i + run < hlit ? w.len[i + run] : 1) == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        seq_emit(w, 18, r - 11);
        run -= r;
      }
      if (run >= 3) {
        seq_emit(w, 17, run - 3);
        run = 0;
      }
      for (; run > 0; run--) seq_emit(w, 0, 0);
    } else {
      seq_emit(w, v, 0);
      run--;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        seq_emit(w, 16, r - 3);
        run -= r;
      }
      for (; run > 0; run--) seq_emit(w, v, 0);
    }
  }
  // the code-length code: 19 symbols, at most 7 bits, complete (a lone symbol gets a partner of length 1)
  int n_cl = 0;
  for (int s = 0; s < 19; s++) {
    if (w.cl_freq[s] == 0) continue;
    int k = n_cl++;
    while (k > 0 && w.cl_freq[w.order[k - 1]] > w.cl_freq[s]) {
      w.order[k] = w.order[k - 1];
      k--;
    }
    w.order[k] = (uint16_t)s;
  }
  if (n_cl == 1) {
    w.cl_len[w.order[0]] = 1;
    w.cl_len[w.order[0] == 0 ? 1 : 0] = 1;
  } else {
    for (int k = 0; k < n_cl; k++) w.A[k] = w.cl_freq[w.order[k]];
    limited_lengths(w, n_cl, 7, w.cl_len);
  }
  canonical_codes(w, w.cl_len, 19, 7, w.cl_code);
  const uint8_t perm[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 19;
  while (hclen > 4 && w.cl_len[perm[hclen - 1]] == 0) hclen--;
  uint32_t pos = 0;
  put_bits(out, pos, final_block ? 1u : 0u, 1);
  put_bits(out, pos, 2u, 2);
  put_bits(out, pos, (uint32_t)(hlit - 257), 5);
  put_bits(out, pos, 0u, 5);
  put_bits(out, pos, (uint32_t)(hclen - 4), 4);
  for (int k = 0; k < hclen; k++) put_bits(out, pos, w.cl_len[perm[k]], 3);
  for (int k = 0; k < w.n_seq; k++) {
    const int s = w.seq_sym[k];
    put_bits(out, pos, w.cl_code[s], w.cl_len[s]);
    if (s == 16) put_bits(out, pos, w.seq_ext[k], 2);
    if (s == 17) put_bits(out, pos, w.seq_ext[k], 3);
    if (s == 18) put_bits(out, pos, w.seq_ext[k], 7);
  }
  return pos;
}

// the literal/length symbol and extra bits of a match of `glen` bytes (3..258)
__host__ __device__ inline void length_symbol(int glen, int& sym, uint32_t& ext, int& next) {
  const int l = glen - 3;
  ext = 0;
  next = 0;
  if (glen == 258) {
    sym = 285;
  } else if (l < 8) {
    sym = 257 + l;
  } else {
    int n = 3;
    while ((l >> (n + 1)) != 0) n++;
    next = n - 2;
    sym = 261 + 4 * next + ((l >> next) & 3);
    ext = (uint32_t)l & ((1u << next) - 1u);
  }
}

// ------------------------------------------------------------------------------------------- arguments
struct PngArgs {
  const uint8_t* images;
  size_t image_stride;
  uint8_t* files;
  size_t file_stride;
  uint64_t* sizes;
  uint8_t* filt;         // [n] x filt_stride filtered bytes (16-byte aligned, stride a multiple of 16)
  size_t filt_stride;
  uint8_t* slots;        // [n, nseg] x PNG_SLOT output bytes of the segments
  uint4* meta;           // [n, nseg]: bytes, raw CRC remainder, Adler a, Adler b
  uint32_t* prefix;      // [n, nseg]: bytes of the segments before
  int32_t w, h, c;
  uint32_t rowbytes, F, nseg;
};

// ------------------------------------------------------------------------------------------- LDS staging
// global [src, src + n) -> lds[m ..], m = src & 15 (returned): 16-byte loads where a whole aligned quad lies inside
__device__ __forceinline__ uint32_t load_to_lds(uint8_t* lds, const uint8_t* src, uint32_t n) {
  const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint8_t* base = src - m;
  const uint32_t nq = (m + n + 15u) >> 4;
  for (uint32_t q = threadIdx.x; q < nq; q += blockDim.x) {
    const uint32_t lo = q << 4;
    if (lo >= m && lo + 16u <= m + n) {
      *reinterpret_cast<uint4*>(lds + lo) = *reinterpret_cast<const uint4*>(base + lo);
    } else {
      for (uint32_t t = 0; t < 16u; t++) {
        const uint32_t p = lo + t;
        if (p >= m && p < m + n) lds[p] = base[p];
      }
    }
  }
  return m;
}
// lds[m .. m + n) -> global [dst, dst + n), m = dst & 3: dword stores where a whole aligned dword lies inside
__device__ __forceinline__ void store_from_lds(const uint8_t* lds, uint32_t m, uint8_t* dst, uint32_t n) {
  uint8_t* base = dst - m;
  const uint32_t nd = (m + n + 3u) >> 2;
  for (uint32_t d = threadIdx.x; d < nd; d += blockDim.x) {
    const uint32_t lo = d << 2;
    if (lo >= m && lo + 4u <= m + n) {
      *reinterpret_cast<uint32_t*>(base + lo) = *reinterpret_cast<const uint32_t*>(lds + lo);
    } else {
      for (uint32_t t = 0; t < 4u; t++) {
        const uint32_t p = lo + t;
        if (p >= m && p < m + n) base[p] = lds[p];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- 1: row filter
__device__ __forceinline__ uint32_t abs_int8(uint32_t r) {
  r &= 255u;
  return r < 128u ? r : 256u - r;
}
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ void __launch_bounds__(FILTER_T)
png_filter_kernel(const PngArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cur[FILTER_CH + 48];
  __shared__ __attribute__((aligned(16))) uint8_t up[FILTER_CH + 48];
  __shared__ __attribute__((aligned(16))) uint8_t ob[FILTER_CH + 16];
  __shared__ unsigned long long sums[5];
  __shared__ int choice_s;
  const uint32_t tid = threadIdx.x;
  const uint32_t row = blockIdx.x % (uint32_t)a.h, img = blockIdx.x / (uint32_t)a.h;
  const uint32_t rb = a.rowbytes, bpp = (uint32_t)a.c;
  const uint8_t* src = a.images + (size_t)img * a.image_stride + (size_t)row * rb;
  uint8_t* dst = a.filt + (size_t)img * a.filt_stride + (size_t)row * (rb + 1u);
  const uint32_t nchunk = (rb + FILTER_CH - 1u) / FILTER_CH;
  const bool has_up = row > 0u;
  if (tid < 5u) sums[tid] = 0ull;
  unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  int choice = 0;
  for (int pass = 0; pass < 2; pass++) {
    for (uint32_t k = 0; k < nchunk; k++) {
      const uint32_t off = k * FILTER_CH;
      const uint32_t len = rb - off < (uint32_t)FILTER_CH ? rb - off : (uint32_t)FILTER_CH;
      const uint32_t lead = k > 0u ? bpp : 0u;      // the left neighbours of the chunk's first pixel
      const uint8_t* csrc = src + off - lead;
      const uint32_t mc = (uint32_t)(reinterpret_cast<uintptr_t>(csrc) & 15u);
      const uint32_t mu = (uint32_t)(reinterpret_cast<uintptr_t>(csrc - rb) & 15u);
      if (pass == 0 || nchunk > 1u) {
        __syncthreads();
        load_to_lds(cur, csrc, len + lead);
        if (has_up) load_to_lds(up, csrc - rb, len + lead);
        __syncthreads();
      }
      const uint8_t* pc = cur + mc + lead;
      const uint8_t* pu = up + mu + lead;
      if (pass == 0) {
        for (uint32_t j = tid; j < len; j += FILTER_T) {
          const bool left = off + j >= bpp;
          const int x = pc[j];
          const int A = left ? pc[j - bpp] : 0;
          const int B = has_up ? pu[j] : 0;
          const int C = (has_up && left) ? pu[j - bpp] : 0;
          s0 += abs_int8((uint32_t)x);
          s1 += abs_int8((uint32_t)(x - A));
          s2 += abs_int8((uint32_t)(x - B));
          s3 += abs_int8((uint32_t)(x - ((A + B) >> 1)));
          s4 += abs_int8((uint32_t)(x - paeth(A, B, C)));
        }
      } else {
        uint8_t* dstk = dst + (k == 0u ? 0u : 1u + off);
        const uint32_t mo = (uint32_t)(reinterpret_cast<uintptr_t>(dstk) & 3u);
        const uint32_t shift = k == 0u ? 1u : 0u;     // chunk 0 starts with the filter byte
        if (k == 0u && tid == 0u) ob[mo] = (uint8_t)choice;
        for (uint32_t j = tid; j < len; j += FILTER_T) {
          const bool left = off + j >= bpp;
          const int x = pc[j];
          const int A = left ? pc[j - bpp] : 0;
          const int B = has_up ? pu[j] : 0;
          const int C = (has_up && left) ? pu[j - bpp] : 0;
          int pred = 0;
          if (choice == 1) pred = A;
          if (choice == 2) pred = B;
          if (choice == 3) pred = (A + B) >> 1;
          if (choice == 4) pred = paeth(A, B, C);
          ob[mo + shift + j] = (uint8_t)(x - pred);
        }
        __syncthreads();
        store_from_lds(ob, mo, dstk, len + shift);
        __syncthreads();
      }
    }
    if (pass == 0) {
      atomicAdd(&sums[0], s0);
      atomicAdd(&sums[1], s1);
      atomicAdd(&sums[2], s2);
      atomicAdd(&sums[3], s3);
      atomicAdd(&sums[4], s4);
      __syncthreads();
      if (tid == 0u) {
        int best = 0;
        for (int f = 1; f < 5; f++)
          if (sums[f] < sums[best]) best = f;
        choice_s = best;
      }
      __syncthreads();
      choice = choice_s;
    }
  }
}

// ------------------------------------------------------------------------------------------- 2: segment deflate
struct OpAdd {
  __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x + y; }
};
struct OpMax {
  __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x > y ? x : y; }
};
struct OpMin {
  __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x < y ? x : y; }
};

template <typename Op>
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, Op op) {
  const int lane = dgs_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, (unsigned)d, 64);
    if (lane >= d) v = op(v, o);
  }
  return v;
}
// inclusive scan over the threads of the block (every thread calls it); wtot: one LDS word per wave
template <typename Op>
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, Op op, uint32_t* wtot) {
  v = wave_scan_incl(v, op);
  const int wave = (int)(threadIdx.x >> 6);
  if (dgs_lane() == 63) wtot[wave] = v;
  __syncthreads();
  for (int u = 0; u < wave; u++) v = op(wtot[u], v);
  __syncthreads();
  return v;
}

struct SegState {
  const uint8_t* seg;
  const unsigned long long* mask;
  const uint32_t* lastset;
  const uint32_t* firstset;
  int L;
};

// the token position i emits: sym < 0 none, sym < 256 a literal, else a match of distance 1 (length symbol + extra bits)
__device__ __forceinline__ void token_at(const SegState& st, int i, int& sym, uint32_t& ext, int& next) {
  const int w = i >> 6, b = i & 63;
  const unsigned long long m = st.mask[w];
  const unsigned long long keep = (2ull << b) - 1ull;       // bits 0..b (b = 63: all)
  const unsigned long long below = m & keep, above = m & ~keep;
  const int start = below != 0ull ? (w << 6) + 63 - __clzll((long long)below) : (w > 0 ? (int)st.lastset[w - 1] : 0);
  const int end = above != 0ull ? (w << 6) + __ffsll((unsigned long long)above) - 1
                                : (w + 1 < PNG_T ? (int)st.firstset[w + 1] : st.L);
  const int j = i - start;
  sym = st.seg[i];
  ext = 0;
  next = 0;
  if (j == 0) return;
  const int r = end - start - 1;            // the bytes of the run after its literal
  const int q = (j - 1) / 258, within = (j - 1) - q * 258;
  const int rest = r - q * 258;
  const int glen = rest < 258 ? rest : 258;
  if (glen < 3) return;                     // a tail of one or two bytes: literals
  if (within != 0) {
    sym = -1;
    return;
  }
  length_symbol(glen, sym, ext, next);
}

__device__ __forceinline__ void put_bits_atomic(uint32_t* out, uint32_t pos, uint32_t val) {
  const uint64_t v = (uint64_t)val << (pos & 31u);
  if ((uint32_t)v != 0u) atomicOr(&out[pos >> 5], (uint32_t)v);
  if ((v >> 32) != 0) atomicOr(&out[(pos >> 5) + 1], (uint32_t)(v >> 32));
}

__global__ void __launch_bounds__(PNG_T)
png_deflate_kernel(const PngArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t seg[PNG_S + 16];
  __shared__ __attribute__((aligned(16))) uint32_t out[PNG_OUT_WORDS];
  __shared__ unsigned long long mask[PNG_T];
  __shared__ uint32_t lastset[PNG_T], firstset[PNG_T], part[PNG_T], wtot[16], crc_tab[256];
  __shared__ CodeWork cw;
  __shared__ uint32_t sh_nused, sh_hdr_bits, sh_tok_bits, sh_adler_a, sh_adler_b, sh_crc;
  const int tid = (int)threadIdx.x, lane = dgs_lane(), wave = tid >> 6;
  const uint32_t img = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  const uint32_t off = s * (uint32_t)PNG_S;
  const int L = (int)(a.F - off < (uint32_t)PNG_S ? a.F - off : (uint32_t)PNG_S);
  const bool last = s == a.nseg - 1u;
  const uint8_t* src = a.filt + (size_t)img * a.filt_stride + off;

  // ---- the segment, zeroed work areas, the CRC table
  for (int q = tid; q < (L + 15) / 16; q += PNG_T)
    *reinterpret_cast<uint4*>(seg + 16 * q) = *reinterpret_cast<const uint4*>(src + 16 * q);
  for (int q = tid; q < PNG_OUT_WORDS; q += PNG_T) out[q] = 0u;
  for (int q = tid; q < 288; q += PNG_T) cw.freq[q] = 0u;
  for (int e = tid; e < 256; e += PNG_T) crc_tab[e] = crc_byte(0u, (uint32_t)e);
  if (tid == 0) {
    sh_nused = 0u;
    sh_adler_a = 0u;
    sh_adler_b = 0u;
    sh_crc = 0u;
  }
  __syncthreads();

  // ---- run flags (position L carries a flag that ends the last run) and the Adler pair
  uint32_t a_sum = 0u, b_sum = 0u;
  for (int it = 0; it < 64; it++) {
    const int i = it * PNG_T + tid;
    bool f = i == L;
    if (i < L) {
      const uint32_t d = seg[i];
      f = i == 0 || d != seg[i - 1];
      a_sum += d;
      b_sum += (uint32_t)(L - i) * d;
    }
    const unsigned long long m = __ballot(f);
    if (lane == 0) mask[i >> 6] = m;
  }
  a_sum = wave_scan_incl(a_sum, OpAdd());
  b_sum = wave_scan_incl(b_sum % ADLER_MOD, OpAdd());
  if (lane == 63) {
    atomicAdd(&sh_adler_a, a_sum);
    atomicAdd(&sh_adler_b, b_sum);
  }
  __syncthreads();

  // ---- nearest run start at or before the end of word w, and at or after the start of word w
  {
    const unsigned long long m = mask[tid];
    const uint32_t hi = m != 0ull ? (uint32_t)(tid * 64 + 63 - __clzll((long long)m)) : 0u;
    lastset[tid] = block_scan_incl(hi, OpMax(), wtot);
    const int w = PNG_T - 1 - tid;
    const unsigned long long mr = mask[w];
    const uint32_t lo = mr != 0ull ? (uint32_t)(w * 64 + __ffsll((unsigned long long)mr) - 1) : 0xFFFFFFFFu;
    const uint32_t r = block_scan_incl(lo, OpMin(), wtot);
    firstset[w] = r < (uint32_t)L ? r : (uint32_t)L;
  }
  __syncthreads();
  SegState st;
  st.seg = seg;
  st.mask = mask;
  st.lastset = lastset;
  st.firstset = firstset;
  st.L = L;

  // ---- histogram
  for (int it = 0; it < 64; it++) {
    const int i = it * PNG_T + tid;
    if (i < L) {
      int sym, next;
      uint32_t ext;
      token_at(st, i, sym, ext, next);
      if (sym >= 0) atomicAdd(&cw.freq[sym], 1u);
    }
  }
  if (tid == 0) atomicAdd(&cw.freq[256], 1u);
  __syncthreads();

  // ---- rank the used symbols by (count, symbol); one lane builds the codes and the header
  for (int sy = tid; sy < PNG_LITLEN; sy += PNG_T) {
    const uint32_t f = cw.freq[sy];
    if (f != 0u) {
      int rank = 0;
      for (int u = 0; u < PNG_LITLEN; u++) {
        const uint32_t fu = cw.freq[u];
        rank += (fu != 0u && (fu < f || (fu == f && u < sy))) ? 1 : 0;
      }
      cw.order[rank] = (uint16_t)sy;
      atomicAdd(&sh_nused, 1u);
    }
  }
  __syncthreads();
  if (tid == 0) sh_hdr_bits = build_block_header(cw, (int)sh_nused, last, out);
  __syncthreads();
  const uint32_t hdr_bits = sh_hdr_bits;

  // ---- bits per position -> offsets
  for (int it = 0; it < 64; it++) {
    const int i = it * PNG_T + tid;
    uint32_t nbits = 0u;
    if (i < L) {
      int sym, next;
      uint32_t ext;
      token_at(st, i, sym, ext, next);
      if (sym >= 0) nbits = (uint32_t)cw.len[sym] + (uint32_t)next + (sym > 256 ? 1u : 0u);
    }
    const uint32_t incl = wave_scan_incl(nbits, OpAdd());
    if (lane == 63) part[it * PNG_NWAVE + wave] = incl;
  }
  __syncthreads();
  {
    const uint32_t v = part[tid];
    const uint32_t incl = block_scan_incl(v, OpAdd(), wtot);
    part[tid] = incl - v;
    if (tid == PNG_T - 1) sh_tok_bits = incl;
  }
  __syncthreads();
  const uint32_t tok_bits = sh_tok_bits;
  const uint32_t total_bits = hdr_bits + tok_bits + (uint32_t)cw.len[256];
  const uint32_t comp_bytes = last ? (total_bits + 7u) / 8u : (total_bits + 3u + 7u) / 8u + 4u;
  const bool stored = comp_bytes >= 5u + (uint32_t)L;
  const uint32_t nbytes = stored ? 5u + (uint32_t)L : comp_bytes;

  if (!stored) {
    for (int it = 0; it < 64; it++) {
      const int i = it * PNG_T + tid;
      uint32_t nbits = 0u, val = 0u;
      if (i < L) {
        int sym, next;
        uint32_t ext;
        token_at(st, i, sym, ext, next);
        if (sym >= 0) {
          const uint32_t cl = cw.len[sym];
          val = (uint32_t)cw.code[sym] | (ext << cl);     // (the distance code is one zero bit)
          nbits = cl + (uint32_t)next + (sym > 256 ? 1u : 0u);
        }
      }
      const uint32_t incl = wave_scan_incl(nbits, OpAdd());
      if (nbits != 0u) put_bits_atomic(out, hdr_bits + part[it * PNG_NWAVE + wave] + incl - nbits, val);
    }
    if (tid == 0) {
      put_bits_atomic(out, hdr_bits + tok_bits, cw.code[256]);
      if (!last) {      // the empty stored block: 000, padding, LEN = 0x0000, NLEN = 0xFFFF
        for (uint32_t p = comp_bytes - 2u; p < comp_bytes; p++) atomicOr(&out[p >> 2], 0xFFu << (8u * (p & 3u)));
      }
    }
  } else {
    uint8_t* ob = reinterpret_cast<uint8_t*>(out);
    if (tid == 0) {
      ob[0] = last ? 1 : 0;
      ob[1] = (uint8_t)(L & 255);
      ob[2] = (uint8_t)(L >> 8);
      ob[3] = (uint8_t)(~L & 255);
      ob[4] = (uint8_t)((~L >> 8) & 255);
    }
    for (int i = tid; i < L; i += PNG_T) ob[5 + i] = seg[i];
  }
  __syncthreads();

  // ---- the raw CRC remainder of the output bytes: a chunk per thread, shifted to the end of the segment, XORed
  {
    const uint8_t* ob = reinterpret_cast<const uint8_t*>(out);
    const uint32_t cb = ((nbytes + PNG_T - 1u) / PNG_T + 3u) & ~3u;
    const uint32_t b0 = (uint32_t)tid * cb;
    if (b0 < nbytes) {
      const uint32_t b1 = b0 + cb < nbytes ? b0 + cb : nbytes;
      uint32_t c = 0u;
      for (uint32_t p = b0; p < b1; p++) c = crc_tab[(c ^ ob[p]) & 255u] ^ (c >> 8);
      if (b1 < nbytes) c = crc_mul(c, crc_xpow8(nbytes - b1));
      atomicXor(&sh_crc, c);
    }
  }
  __syncthreads();
  uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + ((size_t)img * a.nseg + s) * PNG_SLOT);
  for (uint32_t q = (uint32_t)tid; q < (nbytes + 3u) / 4u; q += PNG_T) slot[q] = out[q];
  if (tid == 0)
    a.meta[(size_t)img * a.nseg + s] = make_uint4(nbytes, sh_crc, sh_adler_a % ADLER_MOD, sh_adler_b % ADLER_MOD);
}

// ------------------------------------------------------------------------------------------- 3: assembly
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

__global__ void __launch_bounds__(256)
png_assemble_kernel(const PngArgs a) {
  __shared__ uint32_t wtot[4];
  __shared__ uint32_t chunk_total, sh_cx;
  __shared__ unsigned long long sh_sa, sh_sb;
  const uint32_t tid = threadIdx.x, img = blockIdx.x;
  const uint4* meta = a.meta + (size_t)img * a.nseg;
  uint32_t* prefix = a.prefix + (size_t)img * a.nseg;
  uint8_t* file = a.files + (size_t)img * a.file_stride;
  if (tid == 0u) {
    sh_cx = 0u;
    sh_sa = 0ull;
    sh_sb = 0ull;
  }
  uint32_t Z = 0u;      // deflate bytes of the image
  for (uint32_t base = 0; base < a.nseg; base += 256u) {
    const uint32_t s = base + tid;
    const uint32_t v = s < a.nseg ? meta[s].x : 0u;
    const uint32_t incl = block_scan_incl(v, OpAdd(), wtot);
    if (s < a.nseg) prefix[s] = Z + incl - v;
    if (tid == 255u) chunk_total = incl;
    __syncthreads();
    Z += chunk_total;
    __syncthreads();
  }
  unsigned long long sa = 0ull, sb = 0ull;
  uint32_t cx = 0u;
  for (uint32_t s = tid; s < a.nseg; s += 256u) {       // (prefix[s] is this thread's own write)
    const uint4 m = meta[s];
    const uint64_t seg_end = (uint64_t)(s + 1u) * PNG_S;
    const uint32_t after_filt = seg_end < a.F ? a.F - (uint32_t)seg_end : 0u;
    sa += m.z;
    sb += (unsigned long long)m.w + (unsigned long long)(after_filt % ADLER_MOD) * m.z;
    cx ^= crc_mul(m.y, crc_xpow8((uint64_t)(Z - prefix[s] - m.x) + 4u));     // the Adler-32 follows the last segment
  }
  atomicAdd(&sh_sa, sa);
  atomicAdd(&sh_sb, sb);
  atomicXor(&sh_cx, cx);
  __syncthreads();
  if (tid != 0u) return;
  const uint32_t adler = (uint32_t)(((a.F % ADLER_MOD) + sh_sb) % ADLER_MOD) << 16 | (uint32_t)((1ull + sh_sa) % ADLER_MOD);
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  for (int i = 0; i < 8; i++) file[i] = sig[i];
  // IHDR
  uint8_t* p = file + 8;
  put_be32(p, 13u);
  p[4] = 'I';
  p[5] = 'H';
  p[6] = 'D';
  p[7] = 'R';
  put_be32(p + 8, (uint32_t)a.w);
  put_be32(p + 12, (uint32_t)a.h);
  p[16] = 8;
  p[17] = a.c == 1 ? 0 : (a.c == 2 ? 4 : (a.c == 3 ? 2 : 6));
  p[18] = 0;
  p[19] = 0;
  p[20] = 0;
  uint32_t c = 0u;
  for (int i = 4; i < 21; i++) c = crc_byte(c, p[i]);
  put_be32(p + 21, crc_finish(c, 17u));
  // IDAT: length, type, zlib header; the segments are copied in by png_copy_kernel
  p = file + 33;
  put_be32(p, 2u + Z + 4u);
  p[4] = 'I';
  p[5] = 'D';
  p[6] = 'A';
  p[7] = 'T';
  p[8] = 0x78;
  p[9] = 0x01;
  c = 0u;
  for (int i = 4; i < 10; i++) c = crc_byte(c, p[i]);
  c = crc_mul(c, crc_xpow8((uint64_t)Z + 4u)) ^ sh_cx;
  uint32_t ca = 0u;
  for (int i = 0; i < 4; i++) ca = crc_byte(ca, (adler >> (24 - 8 * i)) & 255u);
  c ^= ca;
  p = file + PNG_HEAD + Z;
  put_be32(p, adler);
  put_be32(p + 4, crc_finish(c, (uint64_t)Z + 10u));
  const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
  for (int i = 0; i < 12; i++) p[8 + i] = iend[i];
  a.sizes[img] = (uint64_t)PNG_HEAD + Z + 20u;
}

// ------------------------------------------------------------------------------------------- 4: segments into the file
__global__ void __launch_bounds__(256)
png_copy_kernel(const PngArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t img = blockIdx.x / a.nseg, s = blockIdx.x % a.nseg;
  const size_t idx = (size_t)img * a.nseg + s;
  const uint32_t nb = a.meta[idx].x;
  const uint8_t* src = a.slots + idx * PNG_SLOT;
  const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
  uint8_t* dst = a.files + (size_t)img * a.file_stride + PNG_HEAD + a.prefix[idx];
  uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
  if (head > nb) head = nb;
  const uint32_t nd = (nb - head) >> 2;
  const uint32_t tail0 = head + 4u * nd;
  if (tid < head) dst[tid] = src[tid];
  if (tid < nb - tail0) dst[tail0 + tid] = src[tail0 + tid];
  const uint32_t sh = 8u * (head & 3u), w0 = head >> 2;
  uint32_t* dstw = reinterpret_cast<uint32_t*>(dst + head);
  for (uint32_t q = tid; q < nd; q += 256u) {
    const uint32_t lo = srcw[w0 + q];
    dstw[q] = sh == 0u ? lo : (lo >> sh) | (srcw[w0 + q + 1u] << (32u - sh));
  }
}

// ------------------------------------------------------------------------------------------- host
// F = h (1 + w c), 0 where the arguments are refused
inline uint64_t png_filtered_bytes(int32_t w, int32_t h, int32_t c) {
  if (w < 1 || h < 1 || c < 1 || c > 4) return 0;
  const uint64_t rb = (uint64_t)w * (uint64_t)c;
  if (rb >= (1ull << 31)) return 0;
  const uint64_t F = (uint64_t)h * (1ull + rb);
  return F < (1ull << 31) ? F : 0;
}
inline uint64_t png_segments(uint64_t F) { return (F + PNG_S - 1) / PNG_S; }
inline uint64_t round16(uint64_t v) { return (v + 15ull) & ~15ull; }

}  // namespace

extern "C" {

size_t dgs_png_bound(int32_t w, int32_t h, int32_t channels) {
  const uint64_t F = png_filtered_bytes(w, h, channels);
  if (F == 0) return 0;
  return (size_t)(63ull + F + 5ull * png_segments(F));
}

size_t dgs_png_tmp_bytes(int32_t n, int32_t w, int32_t h, int32_t channels) {
  const uint64_t F = png_filtered_bytes(w, h, channels);
  if (F == 0 || n < 0) return 0;
  const uint64_t nseg = png_segments(F);
  // (n < 2^31, F < 2^31, nseg <= 2^17: every product stays below 2^63)
  return (size_t)(16ull + (uint64_t)n * (round16(F) + nseg * (uint64_t)PNG_SLOT + nseg * 16ull) +
                  round16((uint64_t)n * nseg * 4ull));
}

int dgs_png_encode(const uint8_t* images, int32_t n, int32_t w, int32_t h, int32_t channels, size_t image_stride,
                   uint8_t* files, size_t file_stride, uint64_t* sizes, void* tmp, dgs_stream_t stream) {
  if (channels < 1 || channels > 4) return dgs_fail_arg("png_encode: channels must be 1, 2, 3 or 4");
  if (w < 1 || h < 1) return dgs_fail_arg("png_encode: w and h must be at least 1");
  const uint64_t F = png_filtered_bytes(w, h, channels);
  if (F == 0) return dgs_fail_arg("png_encode: the filtered stream h (1 + w channels) must stay below 2^31 bytes");
  if (n < 0) return dgs_fail_arg("png_encode: n must not be negative");
  if (n == 0) return DGS_OK;
  if (images == nullptr || files == nullptr || sizes == nullptr || tmp == nullptr)
    return dgs_fail_arg("png_encode: null pointer");
  const uint64_t rb = (uint64_t)w * (uint64_t)channels;
  if ((uint64_t)image_stride < (uint64_t)h * rb) return dgs_fail_arg("png_encode: image_stride is below h w channels");
  if ((uint64_t)file_stride < (uint64_t)dgs_png_bound(w, h, channels))
    return dgs_fail_arg("png_encode: file_stride is below dgs_png_bound");
  if ((reinterpret_cast<uintptr_t>(sizes) & 7u) != 0) return dgs_fail_arg("png_encode: sizes must be 8-byte aligned");
  const uint64_t nseg = png_segments(F);
  if ((uint64_t)n * (uint64_t)h > 0x7fffffffull || (uint64_t)n * nseg > 0x7fffffffull)
    return dgs_fail_arg("png_encode: more than 2^31 - 1 blocks");
  PngArgs a;
  a.images = images;
  a.image_stride = image_stride;
  a.files = files;
  a.file_stride = file_stride;
  a.sizes = sizes;
  uint8_t* base = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(tmp) + 15u) & ~(uintptr_t)15u);
  a.filt = base;
  a.filt_stride = (size_t)round16(F);
  a.slots = a.filt + (size_t)n * a.filt_stride;
  a.meta = reinterpret_cast<uint4*>(a.slots + (size_t)n * nseg * PNG_SLOT);
  a.prefix = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.meta) + (size_t)n * nseg * 16u);
  a.w = w;
  a.h = h;
  a.c = channels;
  a.rowbytes = (uint32_t)rb;
  a.F = (uint32_t)F;
  a.nseg = (uint32_t)nseg;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(png_filter_kernel, dim3((uint32_t)((uint64_t)n * (uint64_t)h)), dim3(FILTER_T), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "png_encode (filter)");
  hipLaunchKernelGGL(png_deflate_kernel, dim3((uint32_t)((uint64_t)n * nseg)), dim3(PNG_T), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "png_encode (deflate)");
  hipLaunchKernelGGL(png_assemble_kernel, dim3((uint32_t)n), dim3(256), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "png_encode (assemble)");
  hipLaunchKernelGGL(png_copy_kernel, dim3((uint32_t)((uint64_t)n * nseg)), dim3(256), 0, st, a);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "png_encode (copy)");
}

}  // extern "C"

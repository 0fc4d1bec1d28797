// jpeg_decode_core.h -- the parts of the JPEG decoder (jpeg_decode.hip, include/dgs_hip.h "JPEG files decoded on the device")
// that run on the host as well as on the device: the parser that turns a file's bytes into a DgsJpegPlan, the geometry of
// the coefficient buffer, and the entropy decoder of ONE restart interval.  Plain C++ with no HIP call and no allocation, so
// the same text compiles with the host compiler alone (tests/jpeg_decode_host_main.cpp runs it under AddressSanitizer and
// UndefinedBehaviorSanitizer over truncated and mutated files) and into the entropy kernel.
//
// The parser treats the file as hostile: every read is bounded by the file's size, every table id, count and length is
// checked before it is used.  The interval decoder treats the SCAN as hostile and the plan as the parser's: it reads only
// bytes of [begin, end) and writes only coefficients of the blocks of its own MCUs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dgs_hip.h"

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

// zig-zag position -> natural index (T.81 figure A.6)
#define JD_ZIGZAG_LITERALS                                                                                                  \
  0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, \
      42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,   \
      62, 63

// ---- geometry: where the blocks of a component live -------------------------------------------------------------------
// Component c is a grid of bx[c] x by[c] blocks (the MCU grid times its sampling factors: the padding the scan codes
// included); its blocks are stored row by row from block index first[c] of the image's slot.  total <= dgs_jpeg_decode's
// per-image bound channels * (2 ceil(w / 16)) * (2 ceil(h / 16)).
struct JdGeometry {
  int32_t ncomp, hs, vs, mcus_x, mcus_y;
  uint32_t mcus;           // mcus_x * mcus_y
  uint32_t bx[3], by[3], first[3], total;
};

JD_HD uint64_t jd_block_bound(int32_t w, int32_t h, int32_t channels) {
  return (uint64_t)channels * (2ull * (uint64_t)((w + 15) / 16)) * (2ull * (uint64_t)((h + 15) / 16));
}

// a[c] by selects: c is a run-time value, and an indexed load would put the struct into scratch memory on the device
JD_HD uint32_t jd_pick(const uint32_t (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// false: not a geometry the decoder has (the parser refuses such files; the kernels refuse such plans)
JD_HD bool jd_geometry(int32_t w, int32_t h, int32_t channels, int32_t hs, int32_t vs, JdGeometry& g) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || (channels != 1 && channels != 3)) return false;
  if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
  if (channels == 1 && hs != 1) return false;
  g.ncomp = channels;
  g.hs = hs;
  g.vs = vs;
  g.mcus_x = (w + 8 * hs - 1) / (8 * hs);
  g.mcus_y = (h + 8 * vs - 1) / (8 * vs);
  g.mcus = (uint32_t)g.mcus_x * (uint32_t)g.mcus_y;
  uint32_t at = 0;
  for (int c = 0; c < 3; c++) {
    const bool live = c < channels;
    g.bx[c] = live ? (uint32_t)g.mcus_x * (uint32_t)(c == 0 ? hs : 1) : 0u;
    g.by[c] = live ? (uint32_t)g.mcus_y * (uint32_t)(c == 0 ? vs : 1) : 0u;
    g.first[c] = at;
    at += g.bx[c] * g.by[c];      // (at most 3 * 8192 * 8192)
  }
  g.total = at;
  return true;
}

// The plan against the call that was handed it.  Everything the kernels index with is checked here, so a plan that did
// not come from dgs_jpeg_decode_plan costs its image a status, not a fault.
JD_HD bool jd_plan_fits(const DgsJpegPlan& p, int32_t w, int32_t h, int32_t channels, JdGeometry& g) {
  if (p.magic != DGS_JPEG_PLAN_MAGIC || p.w != w || p.h != h || p.channels != channels) return false;
  if (!jd_geometry(w, h, channels, p.hs, p.vs, g)) return false;
  if (p.mcus_x != g.mcus_x || p.mcus_y != g.mcus_y || p.restart_interval < 0 || p.n_intervals < 1) return false;
  const uint32_t want = p.restart_interval == 0
                            ? 1u
                            : (g.mcus + (uint32_t)p.restart_interval - 1u) / (uint32_t)p.restart_interval;
  if ((uint32_t)p.n_intervals != want) return false;
  if (p.scan_begin > p.scan_end || p.scan_end > p.file_bytes) return false;
  if ((uint64_t)p.plan_bytes < sizeof(DgsJpegPlan) + 4ull * ((uint64_t)p.n_intervals + 1ull)) return false;
  return true;
}

JD_HD const uint32_t* jd_interval_table(const DgsJpegPlan* p) {
  return reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(p) + sizeof(DgsJpegPlan));
}

// ---- the bit reader: most significant bit first, refilled with aligned word loads -------------------------------------
// acc holds `nbits` valid bits at its top, zeros below.  base must be 4-byte aligned; pos and end are offsets from it.
// A 0xFF is data only when 0x00 follows (the pair gives one 0xFF byte); any other pair is a marker, which ends the data
// of the interval like the end of the range does.  Bits wanted past the end read as 0 and are an error once CONSUMED.
struct JdBits {
  const uint8_t* base;
  uint32_t pos, end;
  uint64_t acc;
  int32_t nbits;
};

JD_HD uint32_t jd_bswap(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xFF00u) | ((w << 8) & 0xFF0000u) | (w << 24); }

JD_HD void jd_refill(JdBits& b) {
  while (b.nbits <= 32 && b.pos < b.end) {
    if ((b.pos & 3u) == 0u && b.end - b.pos >= 4u) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(b.base + b.pos);
      if (((~w - 0x01010101u) & w & 0x80808080u) == 0u) {       // no byte of w is 0xFF
        b.acc |= (uint64_t)jd_bswap(w) << (32 - b.nbits);
        b.nbits += 32;
        b.pos += 4u;
        continue;
      }
    }
    const uint32_t v = b.base[b.pos];
    if (v == 0xFFu) {
      if (b.end - b.pos < 2u || b.base[b.pos + 1u] != 0u) {      // a marker, or a lone 0xFF at the end: no more data
        b.pos = b.end;
        break;
      }
      b.pos += 2u;
    } else {
      b.pos += 1u;
    }
    b.acc |= (uint64_t)v << (56 - b.nbits);
    b.nbits += 8;
  }
}
JD_HD uint32_t jd_peek(const JdBits& b, int n) { return (uint32_t)(b.acc >> (64 - n)); }      // n = 1..32
JD_HD bool jd_skip(JdBits& b, int n) {
  if (n > b.nbits) return false;
  b.acc <<= n;
  b.nbits -= n;
  return true;
}

// One Huffman symbol (T.81 F.2.2.3 with a lookahead of DGS_JPEG_LOOK bits): 0..255, or the negative of a
// DGS_JPEG_S_* status.  At least 16 bits have been asked of the refill before the call.
JD_HD int32_t jd_symbol(JdBits& b, const DgsJpegHuff& t) {
  const uint32_t e = t.look[jd_peek(b, DGS_JPEG_LOOK)];
  if (e != 0u) return jd_skip(b, (int)(e >> 8)) ? (int32_t)(e & 255u) : -DGS_JPEG_S_OUT_OF_BYTES;
  const int32_t c16 = (int32_t)jd_peek(b, 16);
  for (int l = DGS_JPEG_LOOK + 1; l <= 16; l++) {     // the slow path: the first length whose largest code is not below
    const int32_t code = c16 >> (16 - l);
    if (code <= t.maxcode[l]) {
      if (!jd_skip(b, l)) return -DGS_JPEG_S_OUT_OF_BYTES;
      return (int32_t)t.vals[(uint32_t)(code + t.valoff[l]) & 255u];
    }
  }
  return b.nbits < 16 ? -DGS_JPEG_S_OUT_OF_BYTES : -DGS_JPEG_S_BAD_CODE;
}

// s magnitude bits and EXTEND (F.12): 1 <= s <= 15
JD_HD bool jd_receive_extend(JdBits& b, int s, int32_t& v) {
  const int32_t r = (int32_t)jd_peek(b, s);
  if (!jd_skip(b, s)) return false;
  v = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
  return true;
}

// The blocks of restart interval `interval`: MCUs [interval * dri, min(that + dri, mcus)) (all of them without DRI), the
// blocks of an MCU in the order of the scan (luma left to right, top to bottom, then Cb, then Cr).  coef: the image's
// slot, int16 [g.total][64] in natural order, zero where nothing is stored.  huff: the six tables (DC of components
// 0..2, AC of components 0..2) -- the plan's, or the kernel's copy of them.  file: the file's first byte, 4-byte aligned.
// Returns 0 or a DGS_JPEG_S_* status; the blocks decoded before an error keep what was stored.
JD_HD int32_t jd_decode_interval(const DgsJpegPlan& p, const JdGeometry& g, const uint32_t* interval_at,
                                 const DgsJpegHuff* huff, const uint8_t* file, uint32_t interval, int16_t* coef) {
  const uint8_t zigzag[64] = {JD_ZIGZAG_LITERALS};
  const uint32_t dri = p.restart_interval == 0 ? g.mcus : (uint32_t)p.restart_interval;
  const uint64_t m0 = (uint64_t)interval * dri;
  if (m0 >= g.mcus) return DGS_JPEG_S_PLAN;
  const uint32_t m1 = (uint32_t)(m0 + dri < g.mcus ? m0 + dri : g.mcus);
  JdBits b;
  b.base = file;
  b.pos = interval_at[interval];
  const uint32_t next = interval_at[interval + 1u];
  if (next < 2u || b.pos < p.scan_begin || b.pos > next - 2u || next - 2u > p.scan_end) return DGS_JPEG_S_PLAN;
  b.end = next - 2u;            // (the two bytes before the next interval are its RST marker; EOI after the last)
  b.acc = 0;
  b.nbits = 0;
  uint32_t pred[3] = {0u, 0u, 0u};      // (unsigned: a hostile scan may wrap them; read and written by selects: jd_pick)
  uint32_t mx = (uint32_t)m0 % (uint32_t)g.mcus_x, my = (uint32_t)m0 / (uint32_t)g.mcus_x;
  for (uint32_t m = (uint32_t)m0; m < m1; m++) {
    for (int c = 0; c < g.ncomp; c++) {
      const int nh = c == 0 ? g.hs : 1, nv = c == 0 ? g.vs : 1;
      for (int v = 0; v < nv; v++) {
        for (int h = 0; h < nh; h++) {
          // (my < mcus_y and mx < mcus_x because m < mcus: the block is one of g.total)
          const uint32_t blk = jd_pick(g.first, c) + (my * (uint32_t)nv + (uint32_t)v) * jd_pick(g.bx, c) + mx * (uint32_t)nh + (uint32_t)h;
          int16_t* out = coef + (size_t)blk * 64u;
          jd_refill(b);
          int32_t s = jd_symbol(b, huff[c]);
          if (s < 0) return -s;
          if (s > 11) return DGS_JPEG_S_DC_CATEGORY;
          if (s != 0) {
            int32_t diff;
            if (!jd_receive_extend(b, s, diff)) return DGS_JPEG_S_OUT_OF_BYTES;
            const uint32_t dc = jd_pick(pred, c) + (uint32_t)diff;
            pred[0] = c == 0 ? dc : pred[0];
            pred[1] = c == 1 ? dc : pred[1];
            pred[2] = c == 2 ? dc : pred[2];
          }
          const int16_t dc16 = (int16_t)jd_pick(pred, c);
          if (dc16 != 0) out[0] = dc16;
          for (int k = 1; k < 64;) {
            jd_refill(b);
            const int32_t rs = jd_symbol(b, huff[3 + c]);
            if (rs < 0) return -rs;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;       // EOB
              k += 16;                  // ZRL
              if (k > 63) return DGS_JPEG_S_INDEX;
              continue;
            }
            k += r;
            if (k > 63) return DGS_JPEG_S_INDEX;
            int32_t level;
            if (!jd_receive_extend(b, s, level)) return DGS_JPEG_S_OUT_OF_BYTES;
            if (level != 0) out[zigzag[k]] = (int16_t)level;
            k++;
          }
        }
      }
    }
    if (++mx == (uint32_t)g.mcus_x) {
      mx = 0u;
      my++;
    }
  }
  return DGS_JPEG_S_OK;
}

// ---- the parser (host only) -------------------------------------------------------------------------------------------
struct JdParse {            // what the headers say, before the scan is walked
  int32_t w, h, channels, hs, vs, dri, n_intervals;
  uint32_t scan_begin;
  uint8_t tq[3], td[3], ta[3];
  const char* why;          // the reason of a refusal
};

struct JdTables {
  uint8_t quant[4][64];     // zig-zag order, as DQT holds them
  uint8_t counts[8][16];    // DC 0..3, AC 0..3
  uint8_t vals[8][256];
  bool have_q[4], have_h[8];
};

inline int jd_refuse(JdParse& o, int code, const char* why) {
  o.why = why;
  return code;
}

// The kernel's form of one table (Annex C codes, F.2.2.3 maxcode / valptr); false: the counts do not make a prefix code
inline bool jd_make_huff(const uint8_t* counts, const uint8_t* vals, DgsJpegHuff& t) {
  for (int i = 0; i < (1 << DGS_JPEG_LOOK); i++) t.look[i] = 0;
  for (int i = 0; i < 256; i++) t.vals[i] = vals[i];
  int32_t code = 0, k = 0;
  for (int l = 1; l <= 16; l++) {
    const int32_t n = counts[l - 1];
    if (code + n > (1 << l)) return false;
    t.valoff[l] = k - code;
    t.maxcode[l] = n != 0 ? code + n - 1 : -1;
    if (l <= DGS_JPEG_LOOK) {
      for (int32_t i = 0; i < n; i++) {
        const int32_t first = (code + i) << (DGS_JPEG_LOOK - l);
        for (int32_t j = 0; j < (1 << (DGS_JPEG_LOOK - l)); j++) t.look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
      }
    }
    code = (code + n) << 1;
    k += n;
  }
  t.maxcode[0] = t.maxcode[17] = -1;
  t.valoff[0] = t.valoff[17] = 0;
  return true;
}

inline uint32_t jd_be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

// Everything up to the first byte of the scan.  DGS_OK, DGS_E_JPEG_UNSUPPORTED or DGS_E_JPEG_CORRUPT (o.why says why).
inline int jd_parse_headers(const uint8_t* d, size_t size, JdParse& o, JdTables& t) {
  o = JdParse();
  t = JdTables();
  if (size > 0x7fffffffu) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a file of 2 GiB or more");
  if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: no SOI marker");
  size_t at = 2;
  bool have_sof = false;
  uint8_t ids[3] = {0, 0, 0};
  for (;;) {
    if (at + 2 > size) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: the file ends before a scan");
    if (d[at] != 0xFF) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a segment does not start with a marker");
    while (at + 1 < size && d[at + 1] == 0xFF) at++;       // fill bytes
    if (at + 2 > size) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: the file ends before a scan");
    const uint32_t m = d[at + 1];
    at += 2;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;       // markers that stand alone
    if (m == 0xD9) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: EOI before a scan");
    if (at + 2 > size) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a segment header runs past the end");
    const size_t len = jd_be16(d + at);
    if (len < 2 || at + len > size) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a segment length runs past the end");
    const uint8_t* s = d + at + 2;
    const size_t n = len - 2;
    at += len;
    if (m == 0xC0) {
      if (have_sof) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: two frame headers");
      if (n < 6) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: SOF0 is too short");
      if (s[0] != 8) return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: sample precision other than 8 bits");
      o.h = (int32_t)jd_be16(s + 1);
      o.w = (int32_t)jd_be16(s + 3);
      const int nc = s[5];
      if (n != (size_t)(6 + 3 * nc)) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: SOF0 length disagrees with its components");
      if (o.w == 0 || o.h == 0) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a zero dimension");
      if (nc == 4) return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: 4 components (CMYK / YCCK)");
      if (nc != 1 && nc != 3) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a component count other than 1, 3 or 4");
      o.channels = nc;
      int fh[3] = {1, 1, 1}, fv[3] = {1, 1, 1};
      for (int c = 0; c < nc; c++) {
        ids[c] = s[6 + 3 * c];
        fh[c] = s[7 + 3 * c] >> 4;
        fv[c] = s[7 + 3 * c] & 15;
        o.tq[c] = s[8 + 3 * c];
        if (fh[c] < 1 || fh[c] > 4 || fv[c] < 1 || fv[c] > 4)
          return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a sampling factor outside 1..4");
        if (o.tq[c] > 3) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a quantisation table id above 3");
        for (int k = 0; k < c; k++)
          if (ids[k] == ids[c]) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: two components share an id");
      }
      if (nc == 1) {
        o.hs = o.vs = 1;          // (a lone component is coded block by block whatever its factors say)
      } else {
        if (fh[1] != 1 || fv[1] != 1 || fh[2] != 1 || fv[2] != 1 ||
            !((fh[0] == 1 && fv[0] == 1) || (fh[0] == 2 && fv[0] == 1) || (fh[0] == 2 && fv[0] == 2)))
          return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: sampling factors other than 4:4:4, 4:2:2 and 4:2:0");
        o.hs = fh[0];
        o.vs = fv[0];
        if (ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B')
          return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: component ids R, G, B (no colour transform)");
      }
      have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED,
                       m == 0xC2 ? "jpeg: a progressive file (SOF2)"
                                 : (m == 0xC1 ? "jpeg: extended sequential (SOF1)"
                                              : "jpeg: a frame type above SOF2 (lossless, hierarchical or arithmetic)"));
    } else if (m == 0xCC) {
      return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: arithmetic coding conditioning (DAC)");
    } else if (m == 0xDB) {
      size_t k = 0;
      while (k < n) {
        const int pq = s[k] >> 4, id = s[k] & 15;
        if (id > 3) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a DQT table id above 3");
        if (pq == 1) return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: a 16-bit quantisation table");
        if (pq != 0) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a DQT precision other than 0 and 1");
        if (k + 65 > n) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a DQT table runs past its segment");
        for (int i = 0; i < 64; i++) t.quant[id][i] = s[k + 1 + i];
        t.have_q[id] = true;
        k += 65;
      }
    } else if (m == 0xC4) {
      size_t k = 0;
      while (k < n) {
        const int tc = s[k] >> 4, id = s[k] & 15;
        if (tc > 1 || id > 3) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a DHT class above 1 or table id above 3");
        if (k + 17 > n) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a DHT table runs past its segment");
        uint32_t total = 0;
        for (int i = 0; i < 16; i++) total += s[k + 1 + i];
        if (total > 256) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: DHT counts sum past 256");
        if (k + 17 + total > n) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a DHT table runs past its segment");
        const int slot = tc * 4 + id;
        for (int i = 0; i < 16; i++) t.counts[slot][i] = s[k + 1 + i];
        for (uint32_t i = 0; i < 256; i++) t.vals[slot][i] = i < total ? s[k + 17 + i] : 0;
        t.have_h[slot] = true;
        k += 17 + total;
      }
    } else if (m == 0xDD) {
      if (n != 2) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: DRI length is not 4");
      o.dri = (int32_t)jd_be16(s);
    } else if (m == 0xEE) {
      if (n >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e' && s[11] == 0)
        return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: Adobe APP14 with transform 0 (no colour transform)");
    } else if (m == 0xDA) {
      if (!have_sof) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a scan before the frame header");
      if (n < 1 || n != (size_t)(4 + 2 * s[0])) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: SOS length disagrees with its components");
      if (s[0] < 1 || s[0] > 4) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a scan of no or more than 4 components");
      if (s[0] != o.channels) return jd_refuse(o, DGS_E_JPEG_UNSUPPORTED, "jpeg: several scans (the first does not hold every component)");
      for (int c = 0; c < o.channels; c++) {
        if (s[1 + 2 * c] != ids[c]) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: the scan names a component the frame does not have, or another order");
        o.td[c] = s[2 + 2 * c] >> 4;
        o.ta[c] = s[2 + 2 * c] & 15;
        if (o.td[c] > 3 || o.ta[c] > 3) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: the scan names a Huffman table id above 3");
        if (!t.have_h[o.td[c]] || !t.have_h[4 + o.ta[c]])
          return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: the scan refers to a Huffman table that is not defined");
        if (!t.have_q[o.tq[c]]) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a component refers to a quantisation table that is not defined");
      }
      const uint8_t* tail = s + 1 + 2 * o.channels;
      if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0)
        return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: a baseline scan with a spectral selection or approximation");
      JdGeometry g;
      if (!jd_geometry(o.w, o.h, o.channels, o.hs, o.vs, g)) return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: no such geometry");
      o.n_intervals = o.dri == 0 ? 1 : (int32_t)((g.mcus + (uint32_t)o.dri - 1u) / (uint32_t)o.dri);
      o.scan_begin = (uint32_t)at;
      // a block takes at least two bits (a DC code and EOB) and a restart marker two bytes: a header that promises more
      // than the rest of the file can hold is refused before anyone sizes a buffer by it
      if ((uint64_t)g.total > 4ull * (uint64_t)(size - at) + 4ull)
        return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: the scan is too short for the picture");
      if (2ull * ((uint64_t)o.n_intervals - 1ull) > (uint64_t)(size - at))
        return jd_refuse(o, DGS_E_JPEG_CORRUPT, "jpeg: fewer restart intervals than DRI and the MCU count give");
      return DGS_OK;
    }
    // APPn, COM and everything else with a length: skipped
  }
}

inline size_t jd_plan_bytes(int32_t n_intervals) {
  return (sizeof(DgsJpegPlan) + 4u * ((size_t)n_intervals + 1u) + 7u) & ~(size_t)7u;
}

// The whole plan.  plan: plan_bytes bytes, 8-byte aligned, at least jd_plan_bytes of the file's interval count.
inline int jd_parse(const uint8_t* d, size_t size, void* plan, size_t plan_bytes, const char** why) {
  JdParse o;
  JdTables t;
  int rc = jd_parse_headers(d, size, o, t);
  *why = o.why;
  if (rc != DGS_OK) return rc;
  if (plan_bytes < jd_plan_bytes(o.n_intervals)) {
    *why = "jpeg: the plan buffer is smaller than dgs_jpeg_decode_plan_bytes";
    return DGS_E_CAPACITY;
  }
  DgsJpegPlan* p = static_cast<DgsJpegPlan*>(plan);
  uint8_t* raw = static_cast<uint8_t*>(plan);
  for (size_t i = 0; i < jd_plan_bytes(o.n_intervals); i++) raw[i] = 0;
  p->magic = DGS_JPEG_PLAN_MAGIC;
  p->plan_bytes = (uint32_t)jd_plan_bytes(o.n_intervals);
  p->file_bytes = (uint32_t)size;
  p->w = o.w;
  p->h = o.h;
  p->channels = o.channels;
  p->hs = o.hs;
  p->vs = o.vs;
  JdGeometry g;
  jd_geometry(o.w, o.h, o.channels, o.hs, o.vs, g);
  p->mcus_x = g.mcus_x;
  p->mcus_y = g.mcus_y;
  p->restart_interval = o.dri;
  p->n_intervals = o.n_intervals;
  p->scan_begin = o.scan_begin;
  const uint8_t zigzag[64] = {JD_ZIGZAG_LITERALS};
  for (int c = 0; c < o.channels; c++) {
    for (int k = 0; k < 64; k++) p->quant[c][zigzag[k]] = t.quant[o.tq[c]][k];
    if (!jd_make_huff(t.counts[o.td[c]], t.vals[o.td[c]], p->huff[c]) ||
        !jd_make_huff(t.counts[4 + o.ta[c]], t.vals[4 + o.ta[c]], p->huff[3 + c])) {
      *why = "jpeg: DHT counts that make no prefix code";
      return DGS_E_JPEG_CORRUPT;
    }
  }
  // the scan: up to the first marker that is neither a stuffed 0xFF nor RSTm; every RSTm starts an interval
  uint32_t* at_of = reinterpret_cast<uint32_t*>(raw + sizeof(DgsJpegPlan));
  size_t at = o.scan_begin;
  uint32_t found = 0;
  at_of[0] = o.scan_begin;
  for (;;) {
    while (at < size && d[at] != 0xFF) at++;
    if (at + 1 >= size) {
      *why = "jpeg: the scan runs to the end of the file (no EOI)";
      return DGS_E_JPEG_CORRUPT;
    }
    size_t m_at = at + 1;
    while (m_at < size && d[m_at] == 0xFF) m_at++;      // fill bytes before a marker
    if (m_at >= size) {
      *why = "jpeg: the scan runs to the end of the file (no EOI)";
      return DGS_E_JPEG_CORRUPT;
    }
    const uint32_t m = d[m_at];
    if (m == 0) {
      at = m_at + 1;
      continue;
    }
    if (m >= 0xD0 && m <= 0xD7) {
      if (m != 0xD0 + (found & 7u)) {
        *why = "jpeg: restart markers out of order";
        return DGS_E_JPEG_CORRUPT;
      }
      found++;
      if (found >= (uint32_t)o.n_intervals) {
        *why = "jpeg: more restart intervals than DRI and the MCU count give";
        return DGS_E_JPEG_CORRUPT;
      }
      at_of[found] = (uint32_t)(m_at + 1);
      at = m_at + 1;
      continue;
    }
    if (found + 1 != (uint32_t)o.n_intervals) {
      *why = "jpeg: fewer restart intervals than DRI and the MCU count give";
      return DGS_E_JPEG_CORRUPT;
    }
    p->scan_end = (uint32_t)at;
    at_of[o.n_intervals] = (uint32_t)at + 2u;
    at = m_at - 1;          // at the 0xFF of the marker that ended the scan
    break;
  }
  // what follows the scan: EOI, or segments up to it; another scan is one more than this decoder takes
  for (;;) {
    if (at + 2 > size) {
      *why = "jpeg: no EOI";
      return DGS_E_JPEG_CORRUPT;
    }
    if (d[at] != 0xFF) {
      *why = "jpeg: a segment does not start with a marker";
      return DGS_E_JPEG_CORRUPT;
    }
    const uint32_t m = d[at + 1];
    if (m == 0xFF) {
      at++;
      continue;
    }
    if (m == 0xD9) return DGS_OK;
    if (m == 0xDA) {
      *why = "jpeg: several scans";
      return DGS_E_JPEG_UNSUPPORTED;
    }
    if (m == 0xDC) {
      *why = "jpeg: the height comes after the scan (DNL)";
      return DGS_E_JPEG_UNSUPPORTED;
    }
    if (at + 4 > size) {
      *why = "jpeg: a segment header runs past the end";
      return DGS_E_JPEG_CORRUPT;
    }
    const size_t len = jd_be16(d + at + 2);
    if (len < 2 || at + 2 + len > size) {
      *why = "jpeg: a segment length runs past the end";
      return DGS_E_JPEG_CORRUPT;
    }
    at += 2 + len;
  }
}

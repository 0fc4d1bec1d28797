// jpeg_decode.hip -- baseline .jpg files to 8-bit images on the device (deblurgs_amd/jpeg.py decode, scene.py device_jpeg,
// video.py read_frames): libjpeg's pixels, bit for bit.  include/dgs_hip.h states the rules, tests/jpeg_decode_cases.py
// restates them in numpy.  The parser (host) and the entropy decoder of one restart interval (host and device) are
// csrc/jpeg_decode_core.h.
//
// dgs_jpeg_decode: n files and their plans, in one device buffer, to n images u8 [h,w,c], in five enqueues on the caller's
// stream -- the clears of status and of the coefficient buffer, then
//   1 jd_entropy_kernel   one LANE per restart interval, one wave per block, 64 intervals of one image.  The image's six
//                         Huffman tables (DgsJpegHuff: 8-bit lookahead, maxcode / offset for longer codes) are copied to LDS
//                         first.  A lane owns a byte range of the scan and the blocks of its MCUs; it stores the non-zero
//                         coefficients, int16 in natural order, and on a malformed stream raises status[image] (an integer
//                         atomicMax: the largest code wins whatever the order) and stops.  A file without DRI is ONE
//                         interval: one lane decodes its whole scan (parallel decoding inside an interval is not built).
//   2 jd_idct_kernel      8 lanes per 8 x 8 block, 32 blocks per workgroup: lane = row loads 8 coefficients (one 16-byte
//                         load) and dequantises into LDS; lane = column runs the 1-D routine (DESCALE 11) and writes the
//                         column back; lane = row runs it again (DESCALE 18), adds 128, clamps and stores 8 bytes of the
//                         component's plane.  LDS rows of a block are padded to 72 words: the column accesses of the four
//                         blocks of a 32-lane group fall on 32 different banks.
//   3 jd_pixel_kernel     4 pixels per lane in flat order: fancy upsampling of Cb and Cr where the luma factors are 2 x 1
//                         or 2 x 2, YCbCr -> RGB, three dword stores (one for gray).  An image whose status is not 0 is
//                         written as zeros.
// Every kernel checks the plan against the call before it indexes with anything the plan says (jd_image).
// Integers only, no float, no global atomics but the status maximum: the bytes are a function of the files.
#include "dgs_common.h"
#include "jpeg_decode_core.h"

static_assert(sizeof(DgsJpegHuff) == 912 && sizeof(DgsJpegPlan) == 5728 && sizeof(DgsJpegPlan) % 8 == 0,
              "DgsJpegPlan is a fixed layout (include/dgs_hip.h, deblurgs_amd/jpeg.py)");

namespace {

constexpr int JD_T = 256;
constexpr int JD_IDCT_BLOCKS = JD_T / 8;      // 8 x 8 blocks per workgroup of the transform
constexpr int JD_WS = 72;                     // words per block in LDS: 64 + 8 of padding

struct JdArgs {
  const uint8_t* blob;
  size_t blob_bytes;
  const uint64_t* index;
  uint8_t* images;
  size_t image_stride;
  int32_t* status;
  int16_t* coef;            // [n][slot][64]
  uint8_t* planes;          // [n][slot * 64]
  uint32_t slot;            // blocks per image: jd_block_bound
  uint32_t per_image;       // workgroups per image of the kernel being launched
  int32_t n, w, h, c, max_intervals;
};

// The plan and file of image img, or nullptr where they do not fit the call and the buffer (DGS_JPEG_S_PLAN).
__device__ __forceinline__ const DgsJpegPlan* jd_image(const JdArgs& a, uint32_t img, JdGeometry& g, const uint8_t*& file) {
  const uint64_t file_at = a.index[2u * img], plan_at = a.index[2u * img + 1u];
  if ((plan_at & 7u) != 0u || plan_at > a.blob_bytes || a.blob_bytes - plan_at < sizeof(DgsJpegPlan)) return nullptr;
  const DgsJpegPlan* p = reinterpret_cast<const DgsJpegPlan*>(a.blob + plan_at);
  if (!jd_plan_fits(*p, a.w, a.h, a.c, g)) return nullptr;
  if (p->plan_bytes > a.blob_bytes - plan_at || p->n_intervals > a.max_intervals || g.total > a.slot) return nullptr;
  if ((file_at & 3u) != 0u || file_at > a.blob_bytes || p->file_bytes > a.blob_bytes - file_at) return nullptr;
  file = a.blob + file_at;
  return p;
}

// ------------------------------------------------------------------------------------------- 1: restart intervals
__global__ void __launch_bounds__(64)
jd_entropy_kernel(const JdArgs a) {
  __shared__ DgsJpegHuff huff[6];
  const uint32_t img = blockIdx.x / a.per_image, first = (blockIdx.x % a.per_image) * 64u;
  JdGeometry g;
  const uint8_t* file = nullptr;
  const DgsJpegPlan* p = jd_image(a, img, g, file);
  if (p == nullptr) {       // (the whole block leaves: nobody waits at the barrier below)
    if (first == 0u && threadIdx.x == 0u) atomicMax(&a.status[img], DGS_JPEG_S_PLAN);
    return;
  }
  if (first >= (uint32_t)p->n_intervals) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(p->huff);
  uint32_t* dst = reinterpret_cast<uint32_t*>(huff);
  for (uint32_t i = threadIdx.x; i < sizeof(huff) / 4u; i += 64u) dst[i] = src[i];
  __syncthreads();
  const uint32_t interval = first + threadIdx.x;
  if (interval >= (uint32_t)p->n_intervals) return;
  const int32_t s = jd_decode_interval(*p, g, jd_interval_table(p), huff, file, interval,
                                       a.coef + (size_t)img * a.slot * 64u);
  if (s != DGS_JPEG_S_OK) atomicMax(&a.status[img], s);
}

// ------------------------------------------------------------------------------------------- 2: dequantise, transform
// libjpeg's jidctint 1-D routine (include/dgs_hip.h rule 2); the products of a malformed file may wrap (-fwrapv)
__device__ __forceinline__ void jd_idct8(int32_t (&i)[8], int n) {
  int32_t z1 = (i[2] + i[6]) * 4433;
  const int32_t t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
  const int32_t t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int32_t pa = i[7], pb = i[5], pc = i[3], pd = i[1];
  z1 = pa + pd;
  int32_t z2 = pb + pc, z3 = pa + pc, z4 = pb + pd;
  const int32_t z5 = (z3 + z4) * 9633;
  pa *= 2446;
  pb *= 16819;
  pc *= 25172;
  pd *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  pa += z1 + z3;
  pb += z2 + z4;
  pc += z2 + z3;
  pd += z1 + z4;
  const int32_t r = 1 << (n - 1);
  i[0] = (t10 + pd + r) >> n;
  i[7] = (t10 - pd + r) >> n;
  i[1] = (t11 + pc + r) >> n;
  i[6] = (t11 - pc + r) >> n;
  i[2] = (t12 + pb + r) >> n;
  i[5] = (t12 - pb + r) >> n;
  i[3] = (t13 + pa + r) >> n;
  i[4] = (t13 - pa + r) >> n;
}

__global__ void __launch_bounds__(JD_T)
jd_idct_kernel(const JdArgs a) {
  __shared__ int32_t ws[JD_IDCT_BLOCKS][JD_WS];
  const int grp = (int)threadIdx.x >> 3, l = (int)threadIdx.x & 7;
  const uint32_t img = blockIdx.x / a.per_image;
  const uint32_t blk = (blockIdx.x % a.per_image) * (uint32_t)JD_IDCT_BLOCKS + (uint32_t)grp;
  JdGeometry g;
  const uint8_t* file = nullptr;
  const DgsJpegPlan* p = jd_image(a, img, g, file);
  const bool live = p != nullptr && blk < g.total;      // (no early return: the barriers below are the workgroup's)
  const int c = !live ? 0 : (g.ncomp == 3 && blk >= g.first[2] ? 2 : (g.ncomp == 3 && blk >= g.first[1] ? 1 : 0));
  int32_t v[8];
  if (live) {     // lane = row: 8 coefficients, 8 table entries
    const uint4 raw = *reinterpret_cast<const uint4*>(a.coef + ((size_t)img * a.slot + blk) * 64u + (size_t)l * 8u);
    const uint2 q = *reinterpret_cast<const uint2*>(&p->quant[c][l * 8]);
    const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int32_t coef = (int32_t)(int16_t)(rw[j >> 1] >> (16 * (j & 1)));
      const int32_t qj = (int32_t)(((j < 4 ? q.x : q.y) >> (8 * (j & 3))) & 255u);
      ws[grp][l * 8 + j] = coef * qj;
    }
  }
  __syncthreads();
  if (live) {     // lane = column
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = ws[grp][r * 8 + l];
    jd_idct8(v, 11);
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; r++) ws[grp][r * 8 + l] = v[r];
  }
  __syncthreads();
  if (live) {     // lane = row
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = ws[grp][l * 8 + j];
    jd_idct8(v, 18);
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int32_t s = v[j] + 128;
      const uint32_t b = (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
      if (j < 4) lo |= b << (8 * j);
      else hi |= b << (8 * (j - 4));
    }
    const uint32_t first = jd_pick(g.first, c), nbx = jd_pick(g.bx, c);
    const uint32_t k = blk - first, by = k / nbx, bx = k - by * nbx;
    uint8_t* plane = a.planes + ((size_t)img * a.slot + first) * 64u;
    *reinterpret_cast<uint2*>(plane + ((size_t)by * 8u + (size_t)l) * ((size_t)nbx * 8u) + (size_t)bx * 8u) = make_uint2(lo, hi);
  }
}

// ------------------------------------------------------------------------------------------- 3: upsampling, colour
// The chroma sample of output pixel (x, y): rule 3.  P: the component's plane, `stride` bytes per row; dw x dh: the part
// of it that is picture (never read beyond).
__device__ __forceinline__ int32_t jd_chroma(const uint8_t* P, size_t stride, int32_t dw, int32_t dh, int32_t hs, int32_t vs,
                                             int32_t x, int32_t y) {
  if (hs == 1) return P[(size_t)y * stride + (size_t)x];
  const int32_t cx = x >> 1;
  if (vs == 1) {
    const uint8_t* row = P + (size_t)y * stride;
    const int32_t s = row[cx];
    if (dw <= 2) return s;
    if ((x & 1) == 0) return cx == 0 ? s : (3 * s + row[cx - 1] + 1) >> 2;
    return cx == dw - 1 ? s : (3 * s + row[cx + 1] + 2) >> 2;
  }
  const int32_t r = y >> 1;
  const uint8_t* row = P + (size_t)r * stride;
  if (dw <= 2) return row[cx];
  const int32_t nb = (y & 1) != 0 ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
  const uint8_t* nbr = P + (size_t)nb * stride;
  const int32_t s = 3 * row[cx] + nbr[cx];
  if ((x & 1) == 0) return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * row[cx - 1] + nbr[cx - 1] + 8) >> 4;
  return cx == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * row[cx + 1] + nbr[cx + 1] + 7) >> 4;
}

__device__ __forceinline__ uint32_t jd_clamp8(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ void __launch_bounds__(JD_T)
jd_pixel_kernel(const JdArgs a) {
  const uint32_t img = blockIdx.x / a.per_image;
  const uint32_t hw = (uint32_t)a.h * (uint32_t)a.w;                     // (at most 65535^2: fits)
  const uint64_t first = ((uint64_t)(blockIdx.x % a.per_image) * JD_T + threadIdx.x) * 4ull;
  if (first >= hw) return;
  JdGeometry g;
  const uint8_t* file = nullptr;
  const DgsJpegPlan* p = jd_image(a, img, g, file);
  const bool ok = p != nullptr && a.status[img] == DGS_JPEG_S_OK;
  const uint32_t count = hw - (uint32_t)first < 4u ? hw - (uint32_t)first : 4u;
  uint8_t px[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) {
    const uint8_t* Y = a.planes + (size_t)img * a.slot * 64u;
    const size_t sy = (size_t)g.bx[0] * 8u;
    int32_t y = (int32_t)((uint32_t)first / (uint32_t)a.w), x = (int32_t)((uint32_t)first - (uint32_t)y * (uint32_t)a.w);
    const uint8_t* Cb = Y + (size_t)g.first[1] * 64u;
    const uint8_t* Cr = Y + (size_t)g.first[2] * 64u;
    const size_t sc = (size_t)g.bx[1] * 8u;
    const int32_t dw = (a.w + g.hs - 1) / g.hs, dh = (a.h + g.vs - 1) / g.vs;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
      if (j >= count) break;
      const int32_t lum = Y[(size_t)y * sy + (size_t)x];
      if (a.c == 1) {
        px[j] = (uint8_t)lum;
      } else {
        const int32_t cb = jd_chroma(Cb, sc, dw, dh, g.hs, g.vs, x, y) - 128;
        const int32_t cr = jd_chroma(Cr, sc, dw, dh, g.hs, g.vs, x, y) - 128;
        px[3 * j] = (uint8_t)jd_clamp8(lum + ((91881 * cr + 32768) >> 16));
        px[3 * j + 1] = (uint8_t)jd_clamp8(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        px[3 * j + 2] = (uint8_t)jd_clamp8(lum + ((116130 * cb + 32768) >> 16));
      }
      if (++x == a.w) {
        x = 0;
        y++;
      }
    }
  }
  uint8_t* out = a.images + (size_t)img * a.image_stride + (size_t)first * (size_t)a.c;      // 4-byte aligned
  if (count == 4u) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
#pragma unroll
    for (int k = 0; k < 3; k++)
      if (k < a.c) o[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
  } else {
    for (uint32_t k = 0; k < count * (uint32_t)a.c; k++) out[k] = px[k];
  }
}

inline bool jd_call_shape(int32_t n, int32_t w, int32_t h, int32_t c, uint64_t& slot) {
  if (n < 0 || w < 1 || h < 1 || w > 65535 || h > 65535 || (c != 1 && c != 3)) return false;
  slot = jd_block_bound(w, h, c);
  return (uint64_t)n * slot <= 0x7fffffffull;
}

}  // namespace

extern "C" {

int dgs_jpeg_decode_plan_bytes(const uint8_t* data, size_t size, size_t* plan_bytes) {
  if (data == nullptr || plan_bytes == nullptr) return dgs_fail_arg("jpeg_decode_plan_bytes: null pointer");
  JdParse o;
  JdTables t;
  const int rc = jd_parse_headers(data, size, o, t);
  if (rc != DGS_OK) return dgs_fail_code(rc, o.why);
  *plan_bytes = jd_plan_bytes(o.n_intervals);
  return DGS_OK;
}

int dgs_jpeg_decode_plan(const uint8_t* data, size_t size, void* plan, size_t plan_bytes) {
  if (data == nullptr || plan == nullptr) return dgs_fail_arg("jpeg_decode_plan: null pointer");
  if ((reinterpret_cast<uintptr_t>(plan) & 7u) != 0) return dgs_fail_arg("jpeg_decode_plan: plan must be 8-byte aligned");
  const char* why = "";
  const int rc = jd_parse(data, size, plan, plan_bytes, &why);
  return rc == DGS_OK ? DGS_OK : dgs_fail_code(rc, why);
}

// 32 bytes of alignment slack, then per block 64 int16 coefficients and 64 plane bytes.  0 for arguments the call refuses.
size_t dgs_jpeg_decode_tmp_bytes(int32_t n, int32_t w, int32_t h, int32_t channels) {
  uint64_t slot;
  if (!jd_call_shape(n, w, h, channels, slot)) return 0;
  return (size_t)(32ull + (uint64_t)n * slot * 192ull);
}

int dgs_jpeg_decode(const uint8_t* blob, size_t blob_bytes, const uint64_t* index, int32_t n, int32_t w, int32_t h,
                    int32_t channels, int32_t max_intervals, uint8_t* images, size_t image_stride, int32_t* status,
                    void* tmp, dgs_stream_t stream) {
  if (channels != 1 && channels != 3) return dgs_fail_arg("jpeg_decode: channels must be 1 or 3");
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return dgs_fail_arg("jpeg_decode: w and h must be 1..65535");
  if (n < 0) return dgs_fail_arg("jpeg_decode: n must not be negative");
  if (n == 0) return DGS_OK;
  if (blob == nullptr || index == nullptr || images == nullptr || status == nullptr || tmp == nullptr)
    return dgs_fail_arg("jpeg_decode: null pointer");
  if ((reinterpret_cast<uintptr_t>(blob) & 15u) != 0) return dgs_fail_arg("jpeg_decode: blob must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(index) & 7u) != 0) return dgs_fail_arg("jpeg_decode: index must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(status) & 3u) != 0) return dgs_fail_arg("jpeg_decode: status must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(images) & 3u) != 0 || (image_stride & 3u) != 0)
    return dgs_fail_arg("jpeg_decode: images must be 4-byte aligned and image_stride a multiple of 4");
  if ((uint64_t)image_stride < (uint64_t)h * (uint64_t)w * (uint64_t)channels)
    return dgs_fail_arg("jpeg_decode: image_stride is below h w channels");
  if (max_intervals < 1) return dgs_fail_arg("jpeg_decode: max_intervals must be at least 1");
  uint64_t slot;
  if (!jd_call_shape(n, w, h, channels, slot)) return dgs_fail_arg("jpeg_decode: more than 2^31 - 1 blocks");
  JdArgs a;
  a.blob = blob;
  a.blob_bytes = blob_bytes;
  a.index = index;
  a.images = images;
  a.image_stride = image_stride;
  a.status = status;
  a.coef = reinterpret_cast<int16_t*>((reinterpret_cast<uintptr_t>(tmp) + 15u) & ~(uintptr_t)15u);
  a.planes = reinterpret_cast<uint8_t*>(a.coef) + (size_t)n * (size_t)slot * 128u;
  a.slot = (uint32_t)slot;
  a.n = n;
  a.w = w;
  a.h = h;
  a.c = channels;
  a.max_intervals = max_intervals;
  const uint64_t entropy_blocks = ((uint64_t)max_intervals + 63ull) / 64ull;
  const uint64_t idct_blocks = (slot + JD_IDCT_BLOCKS - 1) / JD_IDCT_BLOCKS;
  const uint64_t pixel_blocks = (((uint64_t)h * (uint64_t)w + 3ull) / 4ull + JD_T - 1) / JD_T;
  if ((uint64_t)n * entropy_blocks > 0x7fffffffull || (uint64_t)n * pixel_blocks > 0x7fffffffull)
    return dgs_fail_arg("jpeg_decode: more than 2^31 - 1 workgroups");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(status, 0, (size_t)n * 4u, st);
  if (e != hipSuccess) return dgs_fail_hip(e, "jpeg_decode (clear status)");
  e = hipMemsetAsync(a.coef, 0, (size_t)n * (size_t)slot * 128u, st);
  if (e != hipSuccess) return dgs_fail_hip(e, "jpeg_decode (clear coefficients)");
  a.per_image = (uint32_t)entropy_blocks;
  hipLaunchKernelGGL(jd_entropy_kernel, dim3((uint32_t)((uint64_t)n * entropy_blocks)), dim3(64), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "jpeg_decode (entropy)");
  a.per_image = (uint32_t)idct_blocks;
  hipLaunchKernelGGL(jd_idct_kernel, dim3((uint32_t)((uint64_t)n * idct_blocks)), dim3(JD_T), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return dgs_fail_hip(e, "jpeg_decode (transform)");
  a.per_image = (uint32_t)pixel_blocks;
  hipLaunchKernelGGL(jd_pixel_kernel, dim3((uint32_t)((uint64_t)n * pixel_blocks)), dim3(JD_T), 0, st, a);
  e = hipGetLastError();
  return e == hipSuccess ? DGS_OK : dgs_fail_hip(e, "jpeg_decode (pixels)");
}

}  // extern "C"

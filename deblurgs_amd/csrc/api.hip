// api.hip -- the rasteriser's part of the extern "C" surface of libdgs_hip.so (include/dgs_hip.h): argument checks, blob
// carving, stage sequencing (replaces Rasterizer::forward / ::backward, rasterizer_impl.cu:198-463, and the torch glue
// in rasterize_points.cu:35-239), the backward in parts, contexts and stage timing.  Host code only: every kernel lives in
// the file of its stage (the image-space loss kernels in loss.hip), and the other files report errors through
// dgs_fail_arg / dgs_fail_hip below.
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <new>

#include "dgs_common.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* a = "") {
  snprintf(g_err, sizeof(g_err), fmt, a);
  return code;
}
int fail_hip(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return DGS_E_HIP;
}

constexpr size_t ALIGN = 256;
size_t up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

int sort_bits_for(int W, int H, int K) {
  const uint32_t T = (uint32_t)((W + DGS_TILE - 1) / DGS_TILE) * (uint32_t)((H + DGS_TILE - 1) / DGS_TILE);
  return 32 + (int)dgs_higher_msb(T * (uint32_t)K);  // rasterizer_impl.cu:306, with K*T tiles
}

// forward_only: the image blob holds the tile ranges alone (final_T / n_contrib are not stored: offsets 0, size 0)
DgsLayout make_layout(int P, int W, int H, int K, uint64_t R, bool wide_records, bool forward_only = false) {
  DgsLayout L = {};
  const size_t KP = (size_t)K * (size_t)P;
  const size_t N = (size_t)W * (size_t)H;
  const size_t T = (size_t)((W + DGS_TILE - 1) / DGS_TILE) * (size_t)((H + DGS_TILE - 1) / DGS_TILE);
  size_t o = 0;
  L.geom_rows = o;      o += up(KP * sizeof(DgsRow));
  L.cov3D = o;          o += up((size_t)P * 6 * 4);
  L.pre_sigmoid = o;    o += up(KP * 3 * 4);
  L.tiles_touched = o;  o += up(KP * 4);
  L.point_offsets = o;  o += up(KP * 4);
  L.scan_tmp = o;       o += up(dgs_scan_tmp_words(KP) * 4);
  L.num_rendered = o;   o += up(32);
  L.gsort_keys = o;     o += up(KP * 4);
  L.gsort_keys_alt = o; o += up(KP * 4);
  L.gsort_vals = o;     o += up(KP * 4);
  L.gsort_vals_alt = o; o += up(KP * 4);
  L.tt_sorted = o;      o += up(KP * 4);
  L.offs_sorted = o;    o += up(KP * 4);
  L.tt_tight = o;       o += up(KP * 4);
  L.offs_tight = o;     o += up(KP * 4);
  L.gsort_tmp = o;      o += up(dgs_depth_sort_tmp_words(K, (uint32_t)P) * 4);
  L.cull_rec = o;       o += up(KP * 16);
  L.cull_cnt = o;       o += up(KP * 4);
  L.geom_total = o;
  o = 0;
  L.final_T = o;        o += forward_only ? 0 : up((size_t)K * N * 4);
  L.n_contrib = o;      o += forward_only ? 0 : up((size_t)K * N * 4);
  L.ranges = o;         o += up((size_t)K * T * 8);
  L.image_total = o;
  o = 0;
  L.keys_sorted = o;    o += up(R * 8);
  L.point_list = o;     o += up(R * 4);
  L.keys_unsorted = o;  o += up(R * 8);
  L.vals_unsorted = o;  o += up(R * 4);
  L.sort_tmp = o;       o += up(dgs_sort_tmp_words(R) * 4);
  L.binning_total = o;
  L.sort_bits = sort_bits_for(W, H, K);
  L.sort_passes = dgs_sort_num_passes(32, L.sort_bits);
  // compact keys (tile_cull only): tile | Gaussian | emission index in one 64-bit word when the three fit
  const bool compact = !wide_records;   // DgsProblem.wide_records: keep key + value arrays
  const int u_bits = (int)dgs_higher_msb64(R), g_bits = (int)dgs_higher_msb((uint32_t)(P > 0 ? P : 1));
  L.pack_g_shift = 0;
  L.pack_tile_shift = 0;
  if (compact && R > 0 && u_bits + g_bits + (L.sort_bits - 32) <= 64) {
    L.pack_g_shift = u_bits;
    L.pack_tile_shift = u_bits + g_bits;
  }
  return L;
}

// need_opacity = false: the backward of activated-value problems (raw_params = 0) -- the reference's backward entry point
// is not handed the opacities either (rasterize_points.cu:125-152: it reads them from the geometry state)
int check_problem(const DgsProblem* p, bool need_opacity = true) {
  if (p == nullptr) return fail(DGS_E_ARG, "null DgsProblem");
  if (p->P < 0 || p->W <= 0 || p->H <= 0) return fail(DGS_E_ARG, "bad P/W/H");
  // tile coordinates are packed into 12 bits each by the duplication kernels (and tile counts stay below 2^24)
  if (p->W > 4095 * DGS_TILE || p->H > 4095 * DGS_TILE) return fail(DGS_E_ARG, "W / H above 65520 pixels");
  if (p->K < 1 || p->K > DGS_MAX_K) return fail(DGS_E_ARG, "K must be in [1, DGS_MAX_K]");
  if (p->D < 0 || p->D > 3) return fail(DGS_E_ARG, "SH degree must be 0..3");
  if (p->forward_only != 0 && p->forward_only != 1) return fail(DGS_E_ARG, "forward_only must be 0 or 1");
  if (p->P == 0) return DGS_OK;
  if (p->means3D == nullptr || (need_opacity && p->opacities == nullptr))
    return fail(DGS_E_ARG, "means3D / opacities are null");
  if ((p->shs == nullptr) == (p->colors_precomp == nullptr))
    return fail(DGS_E_ARG, "Please provide excatly one of either SHs or precomputed colors!");
  if (((p->scales == nullptr || p->rotations == nullptr) && p->cov3D_precomp == nullptr) ||
      ((p->scales != nullptr || p->rotations != nullptr) && p->cov3D_precomp != nullptr))
    return fail(DGS_E_ARG, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  if (p->shs != nullptr && p->M < (p->D + 1) * (p->D + 1)) return fail(DGS_E_ARG, "M < (D+1)^2");
  if (p->raw_params != 0 && p->raw_params != 1 && p->raw_params != 3)
    return fail(DGS_E_ARG, "raw_params must be 0, 1 or 3 (1 | isotropic scale)");
  if (p->raw_params) {
    if (p->shs == nullptr || p->scales == nullptr || p->rotations == nullptr)
      return fail(DGS_E_ARG, "raw_params needs shs (dc), scales and rotations");
    if (p->M > 1 && p->shs_rest == nullptr) return fail(DGS_E_ARG, "raw_params with M > 1 needs shs_rest");
  } else if (p->shs_rest != nullptr) {
    return fail(DGS_E_ARG, "shs_rest is only meaningful with raw_params");
  }
  if (p->viewmatrix == nullptr || p->projmatrix == nullptr || p->campos == nullptr || p->bg == nullptr)
    return fail(DGS_E_ARG, "viewmatrix / projmatrix / campos / bg are null");
  if ((uint64_t)p->K * (uint64_t)p->P >= (1ull << 32)) return fail(DGS_E_ARG, "K*P must be < 2^32");
  return DGS_OK;
}

DgsView make_view(const DgsProblem* p, const DgsLayout& L) {
  DgsView v;
  v.P = p->P; v.D = p->D; v.M = p->M; v.W = p->W; v.H = p->H; v.K = p->K;
  v.gx = (p->W + DGS_TILE - 1) / DGS_TILE;
  v.gy = (p->H + DGS_TILE - 1) / DGS_TILE;
  v.T = v.gx * v.gy;
  v.tanfovx = p->tanfovx; v.tanfovy = p->tanfovy;
  v.focal_y = p->H / (2.0f * p->tanfovy);  // rasterizer_impl.cu:227-228
  v.focal_x = p->W / (2.0f * p->tanfovx);
  v.scale_modifier = p->scale_modifier;
  v.z_far = p->z_far;
  v.use_sigmoid = p->use_sigmoid; v.prefiltered = p->prefiltered;
  v.tile_cull = p->tile_cull != 0;
  v.raw_params = (p->raw_params & 1) != 0;
  v.iso_scale = (p->raw_params & 2) != 0;
  v.pack_g_shift = v.tile_cull ? L.pack_g_shift : 0;      // (both 0 in a layout made without R)
  v.pack_tile_shift = v.tile_cull ? L.pack_tile_shift : 0;
  v.scale_lb = p->scale_lb;
  return v;
}

void carve(const DgsProblem* p, const DgsLayout& L, DgsCarve* c) {
  char* g = reinterpret_cast<char*>(p->geom_state);
  char* im = reinterpret_cast<char*>(p->image_state);
  char* b = reinterpret_cast<char*>(p->binning_state);
  c->rows = reinterpret_cast<DgsRow*>(g + L.geom_rows);
  c->cov3D = p->forward_only ? nullptr : reinterpret_cast<float*>(g + L.cov3D);   // (not stored by an inference call)
  c->pre_sigmoid = p->forward_only ? nullptr : reinterpret_cast<float*>(g + L.pre_sigmoid);
  c->tiles_touched = reinterpret_cast<uint32_t*>(g + L.tiles_touched);
  c->point_offsets = reinterpret_cast<uint32_t*>(g + L.point_offsets);
  c->scan_tmp = reinterpret_cast<uint32_t*>(g + L.scan_tmp);
  c->num_rendered = reinterpret_cast<uint32_t*>(g + L.num_rendered);
  c->gsort_keys = reinterpret_cast<uint32_t*>(g + L.gsort_keys);
  c->gsort_keys_alt = reinterpret_cast<uint32_t*>(g + L.gsort_keys_alt);
  c->gsort_vals = reinterpret_cast<uint32_t*>(g + L.gsort_vals);
  c->gsort_vals_alt = reinterpret_cast<uint32_t*>(g + L.gsort_vals_alt);
  c->tt_sorted = reinterpret_cast<uint32_t*>(g + L.tt_sorted);
  c->offs_sorted = reinterpret_cast<uint32_t*>(g + L.offs_sorted);
  c->tt_tight = reinterpret_cast<uint32_t*>(g + L.tt_tight);
  c->offs_tight = reinterpret_cast<uint32_t*>(g + L.offs_tight);
  c->gsort_tmp = reinterpret_cast<uint32_t*>(g + L.gsort_tmp);
  c->cull_rec = reinterpret_cast<uint4*>(g + L.cull_rec);
  c->cull_cnt = reinterpret_cast<uint32_t*>(g + L.cull_cnt);
  c->final_T = p->forward_only ? nullptr : reinterpret_cast<float*>(im + L.final_T);
  c->n_contrib = p->forward_only ? nullptr : reinterpret_cast<uint32_t*>(im + L.n_contrib);
  c->ranges = reinterpret_cast<uint2*>(im + L.ranges);
  c->keys_sorted = b ? reinterpret_cast<uint64_t*>(b + L.keys_sorted) : nullptr;
  c->point_list = b ? reinterpret_cast<uint32_t*>(b + L.point_list) : nullptr;
  c->keys_unsorted = b ? reinterpret_cast<uint64_t*>(b + L.keys_unsorted) : nullptr;
  c->vals_unsorted = b ? reinterpret_cast<uint32_t*>(b + L.vals_unsorted) : nullptr;
  c->sort_tmp = b ? reinterpret_cast<uint32_t*>(b + L.sort_tmp) : nullptr;
}

// DgsBackwardIO.scratch: contribution rows [R], their per-pair totals by natural index [K*P] (64 bytes each), the
// pose-gradient partials (f64)
struct ScratchLayout {
  size_t sums, partials, total;
};
ScratchLayout scratch_layout(uint64_t R, int P, int K) {
  const size_t sums = up((size_t)R * DGS_CONTRIB_F * 4);
  const size_t partials = sums + up((size_t)K * (size_t)P * DGS_SUMS_F * 4);
  return {sums, partials, partials + up((size_t)dgs_geometry_bwd_blocks(P) * (size_t)K * 24 * 8) + ALIGN};
}

// What a call with P > 0 works on: the blob layout for its R, the carved pointers, the kernels' view of the problem and,
// for a backward, the three parts of its scratch.
struct Call {
  DgsLayout L;
  DgsCarve c;
  DgsView v;
  float* contrib = nullptr;
  float* sums = nullptr;
  double* partials = nullptr;
};
enum { NEED_IMAGE = 1, NEED_BINNING = 2 };
// Fills `k` for a layout sized by R and checks the caller's capacities: geom_state always, image_state / binning_state
// (the latter only when R > 0) as `need` says, the scratch of `io` when one is given.  Touches no HIP call.
int prepare(const DgsProblem* p, uint64_t R, int need, const DgsBackwardIO* io, Call* k) {
  k->L = make_layout(p->P, p->W, p->H, p->K, R, p->wide_records != 0, p->forward_only != 0);
  if (p->geom_state == nullptr || p->geom_bytes < k->L.geom_total) return fail(DGS_E_CAPACITY, "geom_state too small");
  if ((need & NEED_IMAGE) && (p->image_state == nullptr || p->image_bytes < k->L.image_total))
    return fail(DGS_E_CAPACITY, "image_state too small");
  if ((need & NEED_BINNING) && R > 0 && (p->binning_state == nullptr || p->binning_bytes < k->L.binning_total))
    return fail(DGS_E_CAPACITY, "binning_state too small");
  carve(p, k->L, &k->c);
  k->v = make_view(p, k->L);
  if (io != nullptr) {
    const ScratchLayout sl = scratch_layout(R, p->P, p->K);
    if (io->scratch == nullptr || io->scratch_bytes < sl.total) return fail(DGS_E_CAPACITY, "backward scratch too small");
    char* base = reinterpret_cast<char*>(io->scratch);
    k->contrib = reinterpret_cast<float*>(base);
    k->sums = reinterpret_cast<float*>(base + sl.sums);
    k->partials = reinterpret_cast<double*>(base + sl.partials);
  }
  return DGS_OK;
}

// ------------------------------------------------------------------------------------------------ context
// Everything that outlives a call lives here, owned by the caller (include/dgs_hip.h, ABI 14): the side stream + events of
// the backward in parts (created on first use, on the device that is current then), its policy, the stage timers.
constexpr int PROF_MAX = 16384;
struct Prof {
  bool on = false;
  int n = 0;
  hipEvent_t* beg = nullptr;   // PROF_MAX each, allocated when the timers are first switched on
  hipEvent_t* end = nullptr;
  int* stage = nullptr;
  int created = 0;
};
}  // namespace

struct DgsContext {
  std::mutex mu;               // one enqueue sequence at a time per context
  DgsContextOptions opt;
  bool side_ready = false;
  int side_device = -1;
  hipStream_t s2 = nullptr;
  hipEvent_t done[DGS_MAX_BWD_PARTS] = {}, join = nullptr;
  Prof prof;
};

namespace {

int prof_begin(DgsContext* ctx, int stage, hipStream_t s) {
  if (ctx == nullptr || !ctx->prof.on) return -1;
  Prof& pr = ctx->prof;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (pr.n >= PROF_MAX) return -1;
  const int i = pr.n++;
  if (i >= pr.created) {
    (void)hipEventCreate(&pr.beg[i]);
    (void)hipEventCreate(&pr.end[i]);
    pr.created = i + 1;
  }
  pr.stage[i] = stage;
  (void)hipEventRecord(pr.beg[i], s);
  return i;
}
void prof_end(DgsContext* ctx, int i, hipStream_t s) {
  if (i >= 0) (void)hipEventRecord(ctx->prof.end[i], s);
}

struct StageTimer {
  DgsContext* ctx;
  int id;
  hipStream_t s;
  StageTimer(DgsContext* c, int stage, hipStream_t st) : ctx(c), id(prof_begin(c, stage, st)), s(st) {}
  ~StageTimer() { prof_end(ctx, id, s); }
};

#define DGS_STAGE(stage_id, where, expr)                                   \
  do {                                                                      \
    hipError_t e__;                                                         \
    {                                                                       \
      StageTimer tm__(p->context, stage_id, s);                                         \
      e__ = (expr);                                                         \
    }                                                                       \
    if (e__ != hipSuccess) return fail_hip(e__, where);                     \
    if (p->debug) {                                                         \
      e__ = hipStreamSynchronize(s);                                        \
      if (e__ != hipSuccess) return fail_hip(e__, where " (debug sync)");   \
    }                                                                       \
  } while (0)

}  // namespace

// error reporting for the other translation units of the library (dgs_common.h)
int dgs_fail_arg(const char* msg) { return fail(DGS_E_ARG, "%s", msg); }
int dgs_fail_hip(hipError_t e, const char* where) { return fail_hip(e, where); }
int dgs_fail_code(int code, const char* msg) { return fail(code, "%s", msg); }

extern "C" {

int dgs_abi_version(void) { return DGS_ABI_VERSION; }
const char* dgs_last_error(void) { return g_err; }

size_t dgs_geom_state_bytes(int32_t P, int32_t K) { return make_layout(P, 16, 16, K, 0, false).geom_total; }
size_t dgs_image_state_bytes(int32_t W, int32_t H, int32_t K) { return make_layout(0, W, H, K, 0, false).image_total; }
size_t dgs_image_state_bytes_forward_only(int32_t W, int32_t H, int32_t K) {
  return make_layout(0, W, H, K, 0, false, true).image_total;
}
size_t dgs_binning_state_bytes(uint64_t R, int32_t W, int32_t H, int32_t K) {
  return make_layout(0, W, H, K, R, false).binning_total;
}
size_t dgs_backward_scratch_bytes(uint64_t R, int32_t P, int32_t K) { return scratch_layout(R, P, K).total; }
int dgs_layout(int32_t P, int32_t W, int32_t H, int32_t K, uint64_t R, int32_t wide_records, DgsLayout* out) {
  if (out == nullptr) return fail(DGS_E_ARG, "null DgsLayout");
  *out = make_layout(P, W, H, K, R, wide_records != 0);
  return DGS_OK;
}
int dgs_backward_scratch_layout(uint64_t R, int32_t P, int32_t K, size_t* sums_offset, size_t* partials_offset) {
  const ScratchLayout sl = scratch_layout(R, P, K);
  if (sums_offset) *sums_offset = sl.sums;
  if (partials_offset) *partials_offset = sl.partials;
  return DGS_OK;
}

// order the (k, Gaussian) pairs by (k, depth bits, index): segmented stable sort of the depth keys preprocess wrote;
// the result (flat indices) lands in c.gsort_vals
// (tile_cull: its last pass also writes the visibility flags in that order)
static hipError_t launch_depth_order(const DgsProblem* p, const DgsCarve& c, hipStream_t s, bool carry_counts = false) {
  const bool cull = p->tile_cull != 0;
  // (status word [6]: "a visible depth key needs more than 27 bits", zeroed with the other status words before preprocess)
  return dgs_launch_depth_sort(c.gsort_keys, c.gsort_keys_alt, c.gsort_vals, c.gsort_vals_alt, p->K, (uint32_t)p->P,
                               c.gsort_tmp, cull ? c.tt_sorted : nullptr, c.num_rendered + 6, s,
                               carry_counts ? c.cull_cnt : nullptr, carry_counts ? c.tt_tight : nullptr,
                               /* drop_invisible = */ cull);
}

// tile_cull: per-slot test in natural order (independent of the depth order), then records and counts into depth order and
// the scan of the counts (total -> status words [2], [3])
static hipError_t launch_tile_cull(const DgsView& v, const DgsCarve& c, hipStream_t s) {
  hipError_t e = dgs_launch_cull_count(v, c, s);
  if (e != hipSuccess) return e;
  return dgs_launch_cull_offsets(v, c, c.num_rendered + 2, s);
}
// the surviving-tile counts ride through the depth sort in the top byte of its 32-bit values when the flat (subframe,
// Gaussian) index fits 24 bits: COUNT first (natural order), then the depth order, then only the scan
static bool counts_ride_with_the_sort(const DgsProblem* p) { return (uint64_t)p->K * (uint64_t)p->P <= (1ull << 24); }

// copy_count = false: the caller (the capacity-mode forward) publishes the count words itself, from its finalize kernel
static int forward_geometry_impl(const DgsProblem* p, const DgsForwardOut* out, dgs_stream_t stream, bool copy_count) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = check_problem(p);
  if (rc != DGS_OK) return rc;
  if (out == nullptr || out->num_rendered_host == nullptr)
    return fail(DGS_E_ARG, "DgsForwardOut: num_rendered_host is null");
  if (p->P == 0) {  // rasterize_points.cu:85 -- nothing to launch
    out->num_rendered_host[0] = 0;
    out->num_rendered_host[1] = 0;
    return DGS_OK;
  }
  if (out->radii == nullptr) return fail(DGS_E_ARG, "DgsForwardOut: radii is null");
  Call k;
  rc = prepare(p, 0, 0, nullptr, &k);
  if (rc != DGS_OK) return rc;
  const DgsCarve& c = k.c;
  const DgsView& v = k.v;
  hipError_t e = dgs_launch_clear_words(c.num_rendered, 8, s);   // (a kernel, not a memset node: see finalize_count_kernel)
  if (e != hipSuccess) return fail_hip(e, "clear status");
  DGS_STAGE(DGS_STAGE_PREPROCESS, "preprocess", dgs_launch_preprocess(*p, v, c, out->radii, s));
  if (!v.tile_cull) {
    DGS_STAGE(DGS_STAGE_SCAN, "scan",
              dgs_launch_scan(c.tiles_touched, c.point_offsets, (uint64_t)p->K * p->P, c.scan_tmp, c.num_rendered, s));
  } else {
    // tile_cull: R is the number of surviving duplicates: per-slot test in natural order, depth ordering (which also
    // lays the per-pair records and counts out in its order), scan of the counts.  Status words [0], [1] stay 0.
    if (counts_ride_with_the_sort(p)) {
      DGS_STAGE(DGS_STAGE_TILE_CULL, "tile cull", dgs_launch_cull_count(v, c, s));
      DGS_STAGE(DGS_STAGE_DEPTH_ORDER, "depth order", launch_depth_order(p, c, s, true));
      DGS_STAGE(DGS_STAGE_SCAN, "scan", dgs_launch_cull_offsets(v, c, c.num_rendered + 2, s, true));
    } else {
      DGS_STAGE(DGS_STAGE_DEPTH_ORDER, "depth order", launch_depth_order(p, c, s));
      DGS_STAGE(DGS_STAGE_TILE_CULL, "tile cull", launch_tile_cull(v, c, s));
    }
  }
  // two words: R and the high half of the 64-bit total (non-zero = the u32 duplicate offsets overflowed)
  if (copy_count)
    e = hipMemcpyAsync(out->num_rendered_host, c.num_rendered + (v.tile_cull ? 2 : 0), 2 * sizeof(uint32_t),
                       hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return fail_hip(e, "copy num_rendered");
  return DGS_OK;
}

int dgs_forward_geometry(const DgsProblem* p, const DgsForwardOut* out, dgs_stream_t stream) {
  return forward_geometry_impl(p, out, stream, true);
}

// R = the exact duplicate count (two-phase forward), or the capacity of the duplicate arrays when `speculative`
// (then the kernels read the count from c.num_rendered[4], set by finalize_count)
static int forward_render_impl(const DgsProblem* p, const DgsForwardOut* out, uint32_t R, bool speculative,
                               hipStream_t s, int phases = 3) {   // 1 = duplicate lists + sort + ranges, 2 = compositing
  int rc = check_problem(p);
  if (rc != DGS_OK) return rc;
  if (out == nullptr || out->out_color == nullptr) return fail(DGS_E_ARG, "DgsForwardOut: out_color is null");
  if (out->debug_contrib_checksum != nullptr && (p->tile_cull || p->forward_only || out->out_depth == nullptr))
    return fail(DGS_E_ARG, "debug_contrib_checksum needs tile_cull = 0 (positions in the reference's lists), out_depth and a "
                           "problem that keeps its state");
  const size_t N = (size_t)p->W * p->H;
  if (p->P == 0) {  // the reference returns zero-filled images when P == 0 (rasterize_points.cu:70-71,85)
    hipError_t e = hipMemsetAsync(out->out_color, 0, (size_t)p->K * 3 * N * 4, s);
    if (e == hipSuccess && out->out_depth != nullptr) e = hipMemsetAsync(out->out_depth, 0, (size_t)p->K * N * 4, s);
    return e == hipSuccess ? DGS_OK : fail_hip(e, "memset outputs");
  }
  Call k;
  rc = prepare(p, R, NEED_IMAGE | NEED_BINNING, nullptr, &k);
  if (rc != DGS_OK) return rc;
  const DgsLayout& L = k.L;
  const DgsCarve& c = k.c;
  const DgsView& v = k.v;
  const int key_lo = v.pack_tile_shift > 0 ? v.pack_tile_shift : 32;   // first tile bit of the key
  const uint32_t* n_dev = speculative ? c.num_rendered + 4 : nullptr;
  if ((phases & 1) && (R > 0 || v.tile_cull)) {  // tile_cull with R == 0 still marks the visible pairs as "no surviving tile"
    // choose the sort's input pair so that the result always lands in keys_sorted / point_list
    DgsCarve cd = c;
    const bool even = (L.sort_passes % 2) == 0;
    if (even) {
      cd.keys_unsorted = c.keys_sorted;
      cd.vals_unsorted = c.point_list;
    }
    if (!v.tile_cull) {
      // (1) order the (k, Gaussian) pairs by (k, depth bits, index)
      DGS_STAGE(DGS_STAGE_DEPTH_ORDER, "depth order", launch_depth_order(p, c, s));
      const uint32_t* order = c.gsort_vals;
      // (2) duplicate in that order, (3) stable sort on the tile bits only
      DGS_STAGE(DGS_STAGE_DUPLICATE, "duplicateWithKeys",
                dgs_launch_duplicate_sorted(v, cd, order, c.tt_sorted, c.offs_sorted, c.scan_tmp, R, s));
    } else {
      // the ordering and the surviving-tile offsets were produced by dgs_forward_geometry
      const uint32_t* order = c.gsort_vals;
      DGS_STAGE(DGS_STAGE_DUPLICATE, "duplicateWithKeys", dgs_launch_duplicate_tight(v, cd, order, R, s));
    }
    int in_alt = 0;
    uint64_t* kalt = even ? c.keys_unsorted : c.keys_sorted;
    uint32_t* valt = even ? c.vals_unsorted : c.point_list;
    const bool packed = v.pack_tile_shift > 0;
    DGS_STAGE(DGS_STAGE_SORT, "radix sort",
              dgs_launch_sort(cd.keys_unsorted, packed ? nullptr : cd.vals_unsorted, kalt, packed ? nullptr : valt, R,
                              key_lo, key_lo + (L.sort_bits - 32), c.sort_tmp, &in_alt, s, n_dev));
  }
  if (phases & 1) DGS_STAGE(DGS_STAGE_RANGES, "identifyTileRanges", dgs_launch_ranges(v, c, R, s, n_dev, key_lo));
  if (phases & 2)
    DGS_STAGE(DGS_STAGE_COMPOSITE_FWD, "composite forward",
              dgs_launch_composite_fwd(v, c, p->bg, out->out_color, out->out_depth, s,   // (c.final_T == NULL: inference)
                                       out->debug_contrib_checksum));
  return DGS_OK;
}

int dgs_forward_render(const DgsProblem* p, const DgsForwardOut* out, uint32_t R, dgs_stream_t stream) {
  return forward_render_impl(p, out, R, false, reinterpret_cast<hipStream_t>(stream));
}

static int forward_capacity_impl(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream,
                                 int phases) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // The count words reach the host from the finalize kernel itself when num_rendered_host is device-accessible pinned
  // memory (hipHostMalloc / torch pin_memory: the usual case) -- no copy node in the launch chain; otherwise by copies.
  uint32_t* host_dev = nullptr;
  Call k;
  {   // arguments first: an invalid call is refused before anything touches the HIP runtime
    const int rc0 = check_problem(p);
    if (rc0 != DGS_OK) return rc0;
    if (out == nullptr || out->num_rendered_host == nullptr)
      return fail(DGS_E_ARG, "DgsForwardOut: num_rendered_host is null");
    if (p->P > 0) {
      if (out->radii == nullptr) return fail(DGS_E_ARG, "DgsForwardOut: radii is null");
      const int rc1 = prepare(p, capacity, ((phases & 2) ? NEED_IMAGE : 0) | NEED_BINNING, nullptr, &k);
      if (rc1 != DGS_OK) return rc1;
    }
  }
  if (p->P > 0) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, out->num_rendered_host, 0) == hipSuccess && dp != nullptr)
      host_dev = reinterpret_cast<uint32_t*>(dp);
    else
      (void)hipGetLastError();   // not mapped: the copies below
  }
  int rc = forward_geometry_impl(p, out, stream, host_dev == nullptr);
  if (rc != DGS_OK) return rc;
  if (p->P > 0) {
    const DgsCarve& c = k.c;   // (only the status words are used: their place does not depend on the layout's R)
    hipError_t e = dgs_launch_finalize_count(c, p->tile_cull != 0, capacity, out->drop_counter, out->status_dev, host_dev,
                                             out->status_host_indirect, s);
    if (host_dev == nullptr) {
      if (e == hipSuccess && out->drop_counter != nullptr)   // [4] = overflowed forwards so far (caller's running counter)
        e = hipMemcpyAsync(out->num_rendered_host + 4, out->drop_counter, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess)   // [2] = overflow flag, [3] = the count the lists were built with (0 on overflow)
        e = hipMemcpyAsync(out->num_rendered_host + 2, c.num_rendered + 5, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess)
        e = hipMemcpyAsync(out->num_rendered_host + 3, c.num_rendered + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    }
    if (e != hipSuccess) return fail_hip(e, "finalize count");
  } else {
    out->num_rendered_host[2] = 0;
    out->num_rendered_host[3] = 0;
  }
  return forward_render_impl(p, out, capacity, true, s, phases);
}
int dgs_forward(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream) {
  return forward_capacity_impl(p, out, capacity, stream, 3);
}
int dgs_forward_lists(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream) {
  return forward_capacity_impl(p, out, capacity, stream, 1);
}
int dgs_forward_composite(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream) {
  return forward_render_impl(p, out, capacity, true, reinterpret_cast<hipStream_t>(stream), 2);
}

// ---- the compositing backward in parts, each part's row totals next to the next part's compositing
// composite_bwd is bound by VALU issue and the LDS, contrib_reduce by scattered HBM writes: side by side they share the
// device well.  The subframes are cut into (up to) three parts; their compositing kernels run back to back on the
// caller's stream, and the row totals of every part but the last run on a side stream owned by the library, each as soon as
// its part's compositing is done; the caller's stream waits for the side stream before the last part's totals, so all of
// the call's work is ordered before whatever the caller enqueues next.  The kernels and every sum are the ones of the single
// launch: bit-identical results (tools/grad_hash.py).  Only for an eagerly enqueued call (backward_impl: never inside a stream
// capture); measured at the metric configuration: the eager step 10.4-10.6 ms against 10.7-10.9 replayed or eager with one
// launch.
// Policy and streams come from the caller's DgsContext (no context: always one launch).
constexpr int BWD_MAX_PARTS = DGS_MAX_BWD_PARTS;
constexpr uint64_t BWD_OVERLAP_MIN_PAIRS = 4000000;   // below this the extra launches and events cost more than they hide

// the context's side stream and events, created on first use on the device that is current (mutex held by the caller)
static hipError_t side_stream(DgsContext* ctx) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (ctx->side_ready) return dev == ctx->side_device ? hipSuccess : hipErrorInvalidDevice;   // one context, one device
  e = hipStreamCreateWithFlags(&ctx->s2, hipStreamNonBlocking);
  for (int i = 0; i < BWD_MAX_PARTS && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ctx->done[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->join, hipEventDisableTiming);
  if (e != hipSuccess) {   // give back what was created: the next large backward tries again from nothing
    for (int i = 0; i < BWD_MAX_PARTS; i++) {
      if (ctx->done[i] != nullptr) (void)hipEventDestroy(ctx->done[i]);
      ctx->done[i] = nullptr;
    }
    if (ctx->join != nullptr) (void)hipEventDestroy(ctx->join);
    if (ctx->s2 != nullptr) (void)hipStreamDestroy(ctx->s2);
    ctx->join = nullptr;
    ctx->s2 = nullptr;
    return e;
  }
  ctx->side_device = dev;
  ctx->side_ready = true;
  return hipSuccess;
}

// cut[0..n]: part i = subframes [cut[i], cut[i+1]).  Default for K >= 6: a first part of two thirds of the subframes -- its
// totals, which take about twice as long beside compositing as alone, then have the compositing of all the others to run
// beside --, a second one of most of the rest and a last one of one subframe (its totals are the only ones nothing runs next
// to): K = 15 -> 10, 4, 1; K = 31 -> 21, 9, 1.  (Measured for the eagerly enqueued step, the only place the parts run, on three
// boxes: 10,4,1 10.40-10.44 against 7,6,2 10.47-10.55 ms; 10,4,1 10.86, 12,2,1 10.80-10.82, 12,3 10.84-10.90, 7,6,2 10.91-10.95,
// 13,2 10.94, 14,1 11.03; on the third 12,2,1 and 7,6,2 were equal within its noise, and K = 31 lost 0.5 % with 26,4,1 against
// 14,13,4 -- profiles/r05_ab_logs.txt, calls 31-34)
static int bwd_parts(const DgsContextOptions& opt, int K, int* cut, bool force) {
  int n = 0;
  cut[0] = 0;
  if (opt.bwd_n_parts > 0) {
    for (int i = 0; i < opt.bwd_n_parts && i < BWD_MAX_PARTS - 1 && n < BWD_MAX_PARTS - 1; i++) {
      const int len = opt.bwd_parts[i];
      if (len <= 0 || cut[n] + len >= K) break;
      cut[n + 1] = cut[n] + len;
      n++;
    }
  } else if (K >= 6) {
    cut[1] = (2 * K + 1) / 3;
    cut[2] = K - 1;
    n = 2;
  } else if (force && K >= 2) {
    cut[1] = (K + 1) / 2;
    n = 1;
  }
  cut[++n] = K;
  return n;
}

static hipError_t backward_composite_overlapped(const DgsProblem* p, const DgsBackwardIO* io, const Call& k, hipStream_t s,
                                                const int* cut, int n) {
  const DgsCarve& c = k.c;
  const DgsView& v = k.v;
  DgsContext* ctx = p->context;
  hipStream_t s2 = ctx->s2;
  hipError_t e = hipSuccess;
  bool forked = false;
  for (int i = 0; i < n && e == hipSuccess; i++) {
    e = dgs_launch_composite_bwd(v, c, p->bg, io->dL_dout_color, io->dL_dout_depth, k.contrib, s, cut[i], cut[i + 1]);
    if (i + 1 < n) {
      if (e == hipSuccess) e = hipEventRecord(ctx->done[i], s);
      if (e == hipSuccess) e = hipStreamWaitEvent(s2, ctx->done[i], 0);
      if (e == hipSuccess) {
        forked = true;
        e = dgs_launch_geometry_bwd(*p, v, c, *io, k.contrib, k.sums, k.partials, s2, 1, 0, 0, cut[i], cut[i + 1]);
      }
    }
  }
  // the join is enqueued also when something failed half-way: whatever already sits on the side stream is ordered before
  // the caller's next work on `s`
  if (forked) {
    hipError_t j = hipEventRecord(ctx->join, s2);
    if (j == hipSuccess) j = hipStreamWaitEvent(s, ctx->join, 0);
    if (j != hipSuccess && e == hipSuccess) e = j;
    if (j != hipSuccess) (void)hipStreamSynchronize(s2);
  }
  if (e == hipSuccess) e = dgs_launch_geometry_bwd(*p, v, c, *io, k.contrib, k.sums, k.partials, s, 1, 0, 0, cut[n - 1], cut[n]);
  return e;
}

// The argument and capacity checks every backward entry point starts with, then its Call.  all_grads: dgs_backward and its
// parts write every gradient of the cloud and need all the outputs; false: the camera only (dgs_backward_pose_only: the
// pose matrices).  P == 0: *empty is set -- nothing to launch -- after the matrix gradients were zeroed (if zero_pose).
static int backward_prepare(const DgsProblem* p, const DgsBackwardIO* io, bool all_grads, bool zero_pose, int32_t g_begin,
                            int32_t g_end, hipStream_t s, Call* k, bool* empty) {
  *empty = false;
  int rc = check_problem(p, p != nullptr && p->raw_params != 0);
  if (rc != DGS_OK) return rc;
  if (p->forward_only)
    return fail(DGS_E_ARG, "%s: the problem is forward_only (nothing was kept for a backward)",
                all_grads ? "backward" : "backward_pose_only");
  if (io == nullptr) return fail(DGS_E_ARG, "null DgsBackwardIO");
  if (io->dL_dviewmatrix == nullptr || io->dL_dprojmatrix == nullptr)
    return fail(DGS_E_ARG, "dL_dviewmatrix / dL_dprojmatrix are null");
  if (p->P == 0) {
    *empty = true;
    if (!zero_pose) return DGS_OK;
    hipError_t e = hipMemsetAsync(io->dL_dviewmatrix, 0, (size_t)p->K * 64, s);
    if (e == hipSuccess) e = hipMemsetAsync(io->dL_dprojmatrix, 0, (size_t)p->K * 64, s);
    return e == hipSuccess ? DGS_OK : fail_hip(e, "memset grads");
  }
  if (!all_grads) {
    if (io->dL_dout_color == nullptr || io->radii == nullptr)
      return fail(DGS_E_ARG, "DgsBackwardIO: dL_dout_color / radii are null");
  } else {
    if (io->dL_dout_color == nullptr || io->radii == nullptr || io->dL_dmeans3D == nullptr ||
        (io->dL_dmeans2D == nullptr && io->stats_max_radii2D == nullptr) || io->dL_dcolors == nullptr ||
        io->dL_dopacity == nullptr || io->dL_dcov3D == nullptr)
      return fail(DGS_E_ARG, "DgsBackwardIO: a required pointer is null");
    if (p->shs != nullptr && io->dL_dsh == nullptr) return fail(DGS_E_ARG, "dL_dsh is null");
    if (p->raw_params && p->M > 1 && io->dL_dsh_rest == nullptr) return fail(DGS_E_ARG, "dL_dsh_rest is null");
    if (p->scales != nullptr && (io->dL_dscales == nullptr || io->dL_drotations == nullptr))
      return fail(DGS_E_ARG, "dL_dscales / dL_drotations are null");
    if (g_begin < 0 || g_end > p->P || g_begin > g_end || (g_begin % 256) != 0)
      return fail(DGS_E_ARG, "backward: bad Gaussian range (g_begin must be a multiple of 256)");
  }
  return prepare(p, io->num_rendered, NEED_IMAGE | NEED_BINNING, io, k);
}

// which != 0: 1 = compositing backward + per-pair totals, 2 = per-Gaussian kernel for [g_begin, g_end), 4 = pose sums
static int backward_impl(const DgsProblem* p, const DgsBackwardIO* io, int which, int32_t g_begin, int32_t g_end,
                         hipStream_t s) {
  Call k;
  bool empty;
  const int rc = backward_prepare(p, io, true, (which & 4) != 0, g_begin, g_end, s, &k, &empty);
  if (rc != DGS_OK || empty) return rc;
  const uint64_t R = io->num_rendered;
  // (with the stage timers on -- dgs_profile_begin -- the two kernels run one after the other: their event pairs then time
  // what they say; so does debug mode, which synchronises after every stage)
  // ... and never inside a stream capture (unless DGS_BWD_OVERLAP=3 asks for it): on this runtime (ROCm 7.2) an executable
  // graph with a kernel on a forked branch does not give back all device memory when it is destroyed -- 4 MB per
  // capture / instantiate / destroy cycle in plain HIP (tools/graph_fork_leak.hip), and with torch's graph pools the
  // step's released buffers stay in use as well: ~0.9 GB per re-capture at 1.2 M Gaussians (tools/soak.py)
  int cut[BWD_MAX_PARTS + 1], parts = 1;
  DgsContext* ctx = p->context;
  const int omode = ctx != nullptr ? ctx->opt.bwd_overlap : 0;
  std::unique_lock<std::mutex> side_lock;
  if ((which & 1) && k.v.tile_cull && !p->debug && omode != 0 && !ctx->prof.on && (R >= BWD_OVERLAP_MIN_PAIRS || omode >= 2)) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (omode != 3 && hipStreamIsCapturing(s, &cs) != hipSuccess) cs = hipStreamCaptureStatusActive;   // (unknown: stay serial)
    if (cs == hipStreamCaptureStatusNone) parts = bwd_parts(ctx->opt, p->K, cut, omode >= 2);
    if (parts > 1) {
      side_lock = std::unique_lock<std::mutex>(ctx->mu);
      if (side_stream(ctx) != hipSuccess) {   // no side stream to be had: the single launch
        (void)hipGetLastError();
        side_lock.unlock();
        parts = 1;
      }
    }
  }
  if (parts > 1) {
    hipError_t e = backward_composite_overlapped(p, io, k, s, cut, parts);
    side_lock.unlock();
    if (e != hipSuccess) return fail_hip(e, "composite backward (parts)");
  } else if (which & 1) {
    DGS_STAGE(DGS_STAGE_COMPOSITE_BWD, "composite backward",
              dgs_launch_composite_bwd(k.v, k.c, p->bg, io->dL_dout_color, io->dL_dout_depth, k.contrib, s));
    DGS_STAGE(DGS_STAGE_CONTRIB_REDUCE, "contribution-row totals",
              dgs_launch_geometry_bwd(*p, k.v, k.c, *io, k.contrib, k.sums, k.partials, s, 1, 0, 0));
  }
  if (which & 6)
    DGS_STAGE(DGS_STAGE_GEOMETRY_BWD, "geometry backward",
              dgs_launch_geometry_bwd(*p, k.v, k.c, *io, k.contrib, k.sums, k.partials, s, which & 6, g_begin, g_end));
  return DGS_OK;
}

int dgs_backward(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream) {
  return backward_impl(p, io, 7, 0, p != nullptr ? p->P : 0, reinterpret_cast<hipStream_t>(stream));
}
int dgs_backward_composite(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream) {
  return backward_impl(p, io, 1, 0, 0, reinterpret_cast<hipStream_t>(stream));
}
int dgs_backward_geometry(const DgsProblem* p, const DgsBackwardIO* io, int32_t g_begin, int32_t g_end,
                          dgs_stream_t stream) {
  return backward_impl(p, io, 2, g_begin, g_end, reinterpret_cast<hipStream_t>(stream));
}
int32_t dgs_backward_parts(const DgsContext* ctx, int32_t K, uint64_t num_rendered, int32_t tile_cull) {
  const int omode = ctx != nullptr ? ctx->opt.bwd_overlap : 0;
  if (K < 1 || !tile_cull || omode == 0 || (num_rendered < BWD_OVERLAP_MIN_PAIRS && omode < 2)) return 1;
  int cut[BWD_MAX_PARTS + 1];
  return bwd_parts(ctx->opt, K, cut, omode >= 2);
}
int dgs_backward_pose(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream) {
  return backward_impl(p, io, 4, 0, 0, reinterpret_cast<hipStream_t>(stream));
}

// The backward of a caller that optimises the CAMERA only (the test-view pose fit, test.py:131-186): the compositing
// backward and the per-pair totals as dgs_backward runs them, then geometry_pose_bwd_kernel instead of the per-Gaussian
// kernel.  Always one launch chain on `s`: the context's side stream is never used.
int dgs_backward_pose_only(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Call k;
  bool empty;
  const int rc = backward_prepare(p, io, false, true, 0, 0, s, &k, &empty);
  if (rc != DGS_OK || empty) return rc;
  DGS_STAGE(DGS_STAGE_COMPOSITE_BWD, "composite backward",
            dgs_launch_composite_bwd(k.v, k.c, p->bg, io->dL_dout_color, io->dL_dout_depth, k.contrib, s, 0, -1, true));
  DGS_STAGE(DGS_STAGE_CONTRIB_REDUCE, "contribution-row totals",
            dgs_launch_geometry_pose_bwd(*p, k.v, k.c, *io, k.contrib, k.sums, k.partials, s, 1));
  DGS_STAGE(DGS_STAGE_GEOMETRY_BWD, "geometry backward (pose only)",
            dgs_launch_geometry_pose_bwd(*p, k.v, k.c, *io, k.contrib, k.sums, k.partials, s, 2));
  return DGS_OK;
}

int dgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, dgs_stream_t stream) {
  (void)projmatrix;  // in_frustum only uses the view depth (auxiliary.h:159)
  if (P < 0 || (P > 0 && (means3D == nullptr || viewmatrix == nullptr || present == nullptr)))
    return fail(DGS_E_ARG, "mark_visible: null pointer");
  if (P == 0) return DGS_OK;
  hipError_t e = dgs_launch_mark_visible(P, means3D, viewmatrix, present, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : fail_hip(e, "mark_visible");
}

int dgs_cloud_activations(int32_t P, const float* scaling, const float* rotation, const float* opacity, float scale_lb,
                          float* out_scaling, float* out_rotation, float* out_opacity, dgs_stream_t stream) {
  if (P < 0 || (out_scaling != nullptr && scaling == nullptr) || (out_rotation != nullptr && rotation == nullptr) ||
      (out_opacity != nullptr && opacity == nullptr))
    return fail(DGS_E_ARG, "cloud_activations: an output is requested without its input");
  if (P == 0) return DGS_OK;
  hipError_t e = dgs_launch_cloud_activations(P, scaling, rotation, opacity, scale_lb, out_scaling, out_rotation,
                                              out_opacity, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : fail_hip(e, "cloud_activations");
}

size_t dgs_scan_tmp_bytes(uint64_t n) { return dgs_scan_tmp_words(n) * 4; }
int dgs_exclusive_scan_u32(const uint32_t* in, uint32_t* out, uint64_t n, void* tmp, uint32_t* total_out,
                           dgs_stream_t stream) {
  hipError_t e = dgs_launch_scan(in, out, n, reinterpret_cast<uint32_t*>(tmp), total_out,
                                 reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? DGS_OK : fail_hip(e, "scan");
}
size_t dgs_sort_tmp_bytes(uint64_t n) { return dgs_sort_tmp_words(n) * 4; }
int dgs_sort_pairs(uint64_t* keys, uint32_t* vals, uint64_t* keys_alt, uint32_t* vals_alt, uint64_t n,
                   int32_t begin_bit, int32_t end_bit, void* tmp, int32_t* result_in_alt, dgs_stream_t stream) {
  if (n >= (1ull << 32)) return fail(DGS_E_ARG, "sort: n must be < 2^32");
  if (begin_bit < 0 || end_bit > 64 || end_bit <= begin_bit) return fail(DGS_E_ARG, "sort: bad bit range");
  int alt = 0;
  hipError_t e = dgs_launch_sort(keys, vals, keys_alt, vals_alt, n, begin_bit, end_bit, reinterpret_cast<uint32_t*>(tmp), &alt,
                                 reinterpret_cast<hipStream_t>(stream));
  if (result_in_alt) *result_in_alt = alt;
  return e == hipSuccess ? DGS_OK : fail_hip(e, "sort");
}

size_t dgs_depth_order_tmp_bytes(int32_t K, int32_t P) {
  return (K > 0 && P > 0) ? dgs_depth_sort_tmp_words(K, (uint32_t)P) * 4 + 256 : 256;
}
int dgs_depth_order(uint32_t* keys, uint32_t* keys_alt, uint32_t* order, uint32_t* order_alt, int32_t K, int32_t P,
                    void* tmp, uint32_t* visible, dgs_stream_t stream) {
  if (K < 0 || P < 0) return fail(DGS_E_ARG, "depth_order: bad size");
  if (K == 0 || P == 0) return DGS_OK;
  if (keys == nullptr || keys_alt == nullptr || order == nullptr || order_alt == nullptr || tmp == nullptr)
    return fail(DGS_E_ARG, "depth_order: null buffer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the last 256 bytes of tmp hold the "a key needs the fourth pass" word
  uint32_t* words = reinterpret_cast<uint32_t*>(tmp);
  uint32_t* flag = words + dgs_depth_sort_tmp_words(K, (uint32_t)P);
  hipError_t e = hipMemsetAsync(flag, 0, 4, s);
  if (e == hipSuccess) e = dgs_launch_depth_sort(keys, keys_alt, order, order_alt, K, (uint32_t)P, words, visible, flag, s);
  return e == hipSuccess ? DGS_OK : fail_hip(e, "depth_order");
}

// device-side address of a pointer that is either device memory or mapped pinned host memory; nullptr otherwise (pageable)
static void* device_view(const void* ptr) {
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, const_cast<void*>(ptr), 0) == hipSuccess && dp != nullptr) return dp;
  (void)hipGetLastError();
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) == hipSuccess && at.type == hipMemoryTypeDevice) return const_cast<void*>(ptr);
  (void)hipGetLastError();
  return nullptr;
}

int dgs_copy_words(void* dst, const void* src, int32_t n_words, dgs_stream_t stream) {
  if (n_words < 0 || n_words > 4096 || (n_words > 0 && (dst == nullptr || src == nullptr)))
    return fail(DGS_E_ARG, "copy_words: bad argument (at most 4096 words)");
  if (n_words == 0) return DGS_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  void* d = device_view(dst);
  void* sp = device_view(src);
  hipError_t e;
  if (d != nullptr && sp != nullptr)   // both reachable from a kernel (system-scope stores + fence: dst may be pinned host)
    e = dgs_launch_copy_words(reinterpret_cast<uint32_t*>(d), reinterpret_cast<const uint32_t*>(sp), n_words, s);
  else                                 // a pageable end: the runtime's copy
    e = hipMemcpyAsync(dst, src, (size_t)n_words * 4, hipMemcpyDefault, s);
  return e == hipSuccess ? DGS_OK : fail_hip(e, "copy_words");
}

int dgs_context_create(const DgsContextOptions* options, DgsContext** out) {
  if (out == nullptr) return fail(DGS_E_ARG, "context_create: null output");
  *out = nullptr;
  DgsContextOptions o;
  memset(&o, 0, sizeof(o));
  o.bwd_overlap = 1;
  if (options != nullptr) o = *options;
  if (o.bwd_overlap < 0 || o.bwd_overlap > 3 || o.bwd_n_parts < 0 || o.bwd_n_parts > DGS_MAX_BWD_PARTS - 1)
    return fail(DGS_E_ARG, "context_create: bwd_overlap must be 0..3, bwd_n_parts 0..DGS_MAX_BWD_PARTS-1");
  for (int i = 0; i < o.bwd_n_parts; i++)
    if (o.bwd_parts[i] < 1) return fail(DGS_E_ARG, "context_create: a part must hold at least one subframe");
  DgsContext* c = new (std::nothrow) DgsContext();
  if (c == nullptr) return fail(DGS_E_ARG, "context_create: out of host memory");
  c->opt = o;
  *out = c;
  return DGS_OK;
}
int dgs_context_destroy(DgsContext* ctx) {
  if (ctx == nullptr) return DGS_OK;
  hipError_t e = hipSuccess;
  if (ctx->side_ready) {
    e = hipStreamSynchronize(ctx->s2);
    for (int i = 0; i < BWD_MAX_PARTS; i++) (void)hipEventDestroy(ctx->done[i]);
    (void)hipEventDestroy(ctx->join);
    (void)hipStreamDestroy(ctx->s2);
  }
  for (int i = 0; i < ctx->prof.created; i++) {
    (void)hipEventDestroy(ctx->prof.beg[i]);
    (void)hipEventDestroy(ctx->prof.end[i]);
  }
  delete[] ctx->prof.beg;
  delete[] ctx->prof.end;
  delete[] ctx->prof.stage;
  delete ctx;
  return e == hipSuccess ? DGS_OK : fail_hip(e, "context_destroy");
}

int dgs_profile_enable(DgsContext* ctx, int32_t on) {
  if (ctx == nullptr) return fail(DGS_E_ARG, "profile_enable: null context");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (on) {   // (each array on its own: a call that ran out of host memory half-way is completed by the next one)
    if (ctx->prof.beg == nullptr) ctx->prof.beg = new (std::nothrow) hipEvent_t[PROF_MAX];
    if (ctx->prof.end == nullptr) ctx->prof.end = new (std::nothrow) hipEvent_t[PROF_MAX];
    if (ctx->prof.stage == nullptr) ctx->prof.stage = new (std::nothrow) int[PROF_MAX];
    if (ctx->prof.beg == nullptr || ctx->prof.end == nullptr || ctx->prof.stage == nullptr)
      return fail(DGS_E_ARG, "profile_enable: out of host memory");
  }
  ctx->prof.on = on != 0;
  return DGS_OK;
}
int dgs_profile_reset(DgsContext* ctx) {
  if (ctx == nullptr) return fail(DGS_E_ARG, "profile_reset: null context");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->prof.n = 0;
  return DGS_OK;
}
int dgs_profile_read(DgsContext* ctx, float* ms, int32_t* calls, int32_t n) {
  if (ctx == nullptr) return fail(DGS_E_ARG, "profile_read: null context");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Prof& pr = ctx->prof;
  for (int i = 0; i < n; i++) {
    if (ms) ms[i] = 0.0f;
    if (calls) calls[i] = 0;
  }
  for (int i = 0; i < pr.n; i++) {
    hipError_t e = hipEventSynchronize(pr.end[i]);
    if (e != hipSuccess) return fail_hip(e, "profile_read");
    float t = 0.0f;
    e = hipEventElapsedTime(&t, pr.beg[i], pr.end[i]);
    if (e != hipSuccess) return fail_hip(e, "profile_read");
    const int st = pr.stage[i];
    if (st >= 0 && st < n) {
      if (ms) ms[st] += t;
      if (calls) calls[st] += 1;
    }
  }
  return DGS_OK;
}

#ifndef DGS_BUILD_ID
#define DGS_BUILD_ID "unstamped"
#endif
const char* dgs_build_id(void) { return DGS_BUILD_ID; }

}  // extern "C"

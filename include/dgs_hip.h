/* dgs_hip.h -- C ABI of libdgs_hip.so: the MI355X (gfx950) differentiable Gaussian-splat rasteriser for
 * DeblurGS's blur-integration loop.
 *
 * This is the drop-in boundary for the reference's pybind module `diff_gaussian_rasterization._C`
 * (/root/reference/submodules/diff-gaussian-rasterization/ext.cpp:15-19,
 *  rasterize_points.h:18-73).  Differences, all deliberate:
 *   - plain C: raw device pointers, sizes and a HIP stream handle; no torch types.  The caller owns every
 *     byte (inputs, outputs, gradients, the three state blobs and the backward scratch); the library never
 *     allocates device memory.  Blob sizes come from the dgs_*_bytes() queries, and the carving of a blob
 *     into sub-arrays is a pure function of (P, W, H, K, R, wide_records, forward_only), replayed identically by forward and backward
 *     (the reference does the same with GeometryState/ImageState/BinningState::fromChunk,
 *     rasterizer_impl.cu:155-194,389-391).
 *   - the duplicates are generated in (k, depth, index) order (a 15 M-pair sort of the Gaussians) so that the
 *     R-pair sort only has to order the bits(K*T) tile bits; sorted keys / point list are bit-identical to the
 *     reference's single (tile | depth) sort.
 *   - K >= 1 subframes per call ("K-fused"): one launch chain rasterises all K poses of a blurry view
 *     (scene/motion.py:141-143 calls render() K times).  K = 1 is exactly `_C.rasterize_gaussians`.
 *   - the forward is split in two calls around the one host read of num_rendered
 *     (rasterizer_impl.cu:286-287): dgs_forward_geometry -> caller sizes the binning blob ->
 *     dgs_forward_render.
 * Every entry point returns 0 on success or a negative DGS_E_* code; dgs_last_error() gives the text.
 * All kernels are enqueued on the given stream; nothing here synchronises unless `debug` is set.
 *   - NO PROCESS STATE (ABI 14): the library reads no environment variable and keeps no global but the thread-local
 *     text of dgs_last_error().  What outlives a call -- the side stream and events the backward of a large view forks
 *     part of its work onto, the policy for that fork, the stage timers -- lives in a DgsContext the CALLER creates,
 *     hands over in DgsProblem.context and destroys; with context = NULL every call is one launch chain on the given
 *     stream and nothing else.  (The reference keeps its state in caller tensors only, rasterize_points.cu:27-33.)
 */
#ifndef DGS_HIP_H_INCLUDED
#define DGS_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGS_ABI_VERSION 15
#define DGS_MAX_K 128 /* subframes per fused call */

#define DGS_OK 0
#define DGS_E_ARG (-1)      /* bad shape / null pointer / exclusive-argument violation */
#define DGS_E_CAPACITY (-2) /* a caller-provided blob is too small */
#define DGS_E_HIP (-3)      /* a HIP runtime error (text in dgs_last_error) */

typedef void* dgs_stream_t; /* hipStream_t */

/* ---- caller-owned context (ABI 14) ---------------------------------------------------------------------------
 * Everything the library keeps between calls.  dgs_context_create, on the CURRENT device: one non-blocking side stream,
 * DGS_MAX_BWD_PARTS + 1 events (no device memory), the options below, and the stage timers of dgs_profile_*.  A context
 * serialises the calls that use it (a mutex around each enqueue sequence); use one per host thread that enqueues
 * concurrently.  It must outlive every call it was handed to and be destroyed on a quiet device. */
#define DGS_MAX_BWD_PARTS 8
typedef struct DgsContextOptions {
  int32_t bwd_overlap; /* the compositing backward in parts, each part's row totals on the side stream next to the next
                        * part's compositing (dgs_backward): 0 = never; 1 = for large views (tile_cull, K >= 6, >= 4 M
                        * duplicates), never inside a stream capture (the default); 2 = for any view with K >= 2 (tests);
                        * 3 = as 2, also inside a stream capture (measurements only: a forked executable graph does not
                        * return its memory on ROCm 7.2, tools/graph_fork_leak.hip) */
  int32_t bwd_n_parts; /* 0 = the library's cut (K = 15: 10, 4, 1); n >= 1: bwd_parts[0..n-1] subframes per part, what is
                        * left of K after them is the last part (entries that do not fit K are dropped) */
  int32_t bwd_parts[DGS_MAX_BWD_PARTS - 1];
} DgsContextOptions;
typedef struct DgsContext DgsContext; /* opaque */
/* options = NULL: {1, 0, {}}. */
int dgs_context_create(const DgsContextOptions* options, DgsContext** out);
int dgs_context_destroy(DgsContext* ctx); /* NULL is a no-op */

/* Arguments shared by forward and backward: replaces the 22 / 25 positional arguments of
 * RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA (rasterize_points.cu:35-59,125-152). */
typedef struct DgsProblem {
  int32_t P;       /* Gaussians */
  int32_t D;       /* active SH degree 0..3 */
  int32_t M;       /* SH coefficients per Gaussian, (max_sh_degree+1)^2; 0 when colors_precomp is used */
  int32_t W, H;    /* image size */
  int32_t K;       /* subframes (poses) in this call, 1..DGS_MAX_K */
  float tanfovx, tanfovy;
  float scale_modifier;
  float z_near, z_far; /* z_near is plumbed but unused, as in the reference */
  int32_t use_sigmoid; /* colour activation: 0 = relu(x+0.5), 1 = sigmoid (forward.cu:63-80) */
  int32_t prefiltered;
  int32_t debug;       /* sync + check after every stage (auxiliary.h:179-186) */
  int32_t tile_cull;   /* 0: one duplicate per tile of the 3-sigma rectangle, the reference's exact lists
                        *    (rasterizer_impl.cu:76-108); 1: drop the duplicates whose Gaussian cannot reach
                        *    alpha >= 1/255 at any pixel of the tile (pairs the reference skips at every pixel,
                        *    forward.cu:356-358), so R is smaller and the outputs are unchanged.  Must be the same
                        *    in the forward and backward calls of one problem. */
  int32_t raw_params;  /* 0: opacities / scales / rotations / shs are activated values, as the reference's render() passes
                        *    them (gaussian_renderer/__init__.py:60-77).  1: they are the cloud's raw parameters and the
                        *    kernels apply the reference's activations themselves (scene/gaussian_model.py:36-50,
                        *    scene/gaussian_activation.py): opacity clamp(x, 0, 1), scale exp(x) + scale_lb, rotation
                        *    x / max(|x|, 1e-12), SH = [shs (dc, [P,1,3]) | shs_rest ([P,M-1,3])]; the backward then
                        *    returns gradients with respect to the raw parameters.  3 (= 1 | 2): the same with ONE shared
                        *    scale per Gaussian, column 0 of `scales` used for all three axes (use_isotrophic,
                        *    scene/gaussian_model.py:115-118); dL_dscales then carries the summed gradient in column 0
                        *    and zeros in columns 1, 2. */
  float scale_lb;
  int32_t wide_records; /* tile_cull only.  0 (default): a duplicate is ONE 64-bit word, tile | Gaussian | emission index,
                         *    whenever the three fit (DgsLayout.pack_*), and the value arrays stay unused; 1: always keep
                         *    the key (tile << 32 | emission index) and the Gaussian index in separate arrays.  Part of
                         *    the blob carving: must be the same in the forward and backward calls of one problem. */
  int32_t forward_only; /* 1: an inference call -- the reference's test.py:117 / render_spiral.py:29 call render() under
                         *    no_grad --: nothing is kept for a backward.  The compositing does not store final_T /
                         *    n_contrib, preprocess does not store cov3D / the colour-activation mask, image_state needs
                         *    only dgs_image_state_bytes_forward_only(W,H,K) bytes (the tile ranges; a full-size blob is
                         *    accepted too), and dgs_backward* on such a problem returns DGS_E_ARG.  Outputs are
                         *    bit-identical to forward_only = 0. */
  /* inputs, device pointers, fp32 contiguous */
  const float* means3D;        /* [P,3] */
  const float* shs;            /* [P,M,3] or NULL */
  const float* shs_rest;       /* raw_params = 1 only: [P,M-1,3] (then shs is [P,1,3]); else NULL */
  const float* colors_precomp; /* [P,3]   or NULL   (exactly one of shs / colors_precomp) */
  const float* opacities;      /* [P]; may be NULL in the backward calls of a raw_params = 0 problem (the reference's backward
                                * is not handed them either, rasterize_points.cu:125-152) */
  const float* scales;         /* [P,3] or NULL */
  const float* rotations;      /* [P,4] or NULL */
  const float* cov3D_precomp;  /* [P,6] or NULL   (exactly one of scales+rotations / cov3D_precomp) */
  const float* viewmatrix;     /* [K,4,4] row-vector convention, flat index 4r+c (auxiliary.h:58-66) */
  const float* projmatrix;     /* [K,4,4] full projection = view @ proj */
  const float* campos;         /* [K,3] */
  const float* bg;             /* [3] */
  /* state blobs kept alive by the caller between forward and backward */
  void* geom_state;    size_t geom_bytes;    /* >= dgs_geom_state_bytes(P,K) */
  void* image_state;   size_t image_bytes;   /* >= dgs_image_state_bytes(W,H,K) */
  void* binning_state; size_t binning_bytes; /* >= dgs_binning_state_bytes(R,W,H,K); unused by dgs_forward_geometry */
  DgsContext* context; /* caller-owned (dgs_context_create) or NULL: no side stream, no stage timers -- every call is one
                        * launch chain on `stream`.  Not part of the blob carving; may differ between forward and backward. */
} DgsProblem;

typedef struct DgsForwardOut {
  float* out_color;   /* [K,3,H,W] */
  float* out_depth;   /* [K,1,H,W], or NULL: the caller does not consume the depth image (the default training loss
                       * never reads it) -- the depth channel then drops out of the compositing */
  int32_t* radii;     /* [K,P] */
  uint32_t* num_rendered_host; /* pinned host uint32[2] (dgs_forward: [5]): dgs_forward_geometry enqueues an async copy
                                * of {R, overflow}; overflow != 0 means the duplicate count exceeded 32 bits */
  uint32_t* drop_counter;      /* dgs_forward only, optional device word owned by the caller: incremented by every
                                * forward whose capacity overflowed and copied to num_rendered_host[4].  A caller that
                                * replays a captured graph reads its running value instead of one flag per replay. */
  uint32_t* status_dev;        /* dgs_forward only, optional DEVICE uint32[4] owned by the caller and outliving the state
                                * blobs: receives the same four words as num_rendered_host[0..3] ({count, its high word,
                                * overflow flag, count the lists were built with}).  Every replay of a captured graph copies
                                * into the SAME pinned num_rendered_host block; a caller that runs several replays ahead
                                * enqueues its own copy of status_dev into a per-step pinned slot right behind each replay
                                * and so reads the words of exactly that replay. */
  const uint64_t* status_host_indirect; /* dgs_forward only, optional DEVICE uint64: the address of a device-accessible
                                * PINNED HOST uint32[5] that this forward's finalize kernel writes the five words of
                                * num_rendered_host into, read from device memory when the kernel runs.  A caller that
                                * replays a captured graph stores a different block's address there before every replay
                                * (through its own device-side scalar block): every replay then reports into a pinned
                                * slot of its own without any copy behind it. */
  uint32_t* debug_contrib_checksum; /* optional [K, H*W], tile_cull = 0 only: per pixel, the wrap-around sum of
                                * pos * 2654435761 over the 1-based positions pos (inside the tile's list) of the pairs that
                                * contribute to the pixel.  What the parity tests compare with the CPU oracle's to find the
                                * pixels where the two traversals took a different per-pair decision (an exp() ulp at one of
                                * the three thresholds of forward.cu:354-368); NULL (the product): the compositing kernel
                                * without that sum. */
} DgsForwardOut;

typedef struct DgsBackwardIO {
  uint32_t num_rendered;      /* R returned by the forward */
  const int32_t* radii;       /* [K,P] from the forward */
  const float* dL_dout_color; /* [K,3,H,W] */
  const float* dL_dout_depth; /* [K,1,H,W] or NULL (= zeros) */
  void* scratch; size_t scratch_bytes; /* >= dgs_backward_scratch_bytes(R,P,K) */
  /* gradients, fully overwritten (no zero-fill needed).  Per-Gaussian grads are summed over the K
   * subframes; the screen-space and pose grads stay per subframe because densification and the trajectory
   * consume them per subframe (train.py:188-193, scene/motion.py:248-294). */
  float* dL_dmeans3D;  /* [P,3] */
  float* dL_dmeans2D;  /* [K,P,3] NDC-scaled screen gradient, .z = 0 (backward.cu:628-629); NULL allowed with stats_* */
  float* dL_dsh;       /* [P,M,3]  (NULL when colors_precomp was used); [P,1,3] with raw_params */
  float* dL_dsh_rest;  /* raw_params = 1 only: [P,M-1,3] */
  float* dL_dcolors;   /* [P,3]    (written always; the grad of colors_precomp when that was used) */
  float* dL_dopacity;  /* [P] */
  float* dL_dscales;   /* [P,3]  (NULL when cov3D_precomp was used) */
  float* dL_drotations;/* [P,4]  (NULL when cov3D_precomp was used) */
  float* dL_dcov3D;    /* [P,6] */
  float* dL_dviewmatrix; /* [K,4,4] */
  float* dL_dprojmatrix; /* [K,4,4] */
  /* raw_params = 1 only: adds opacity_hinge_scale * d/dx hinge_l2 terms to dL_dopacity, i.e. the gradient of the
   * training loss's lambda_hinge * hinge_l2(_opacity) (utils/loss_utils.py:96-104, train.py:156-163) with
   * opacity_hinge_scale = lambda_hinge / P; 0 = off.  Saves the caller a dozen elementwise launches per step. */
  float opacity_hinge_scale;
  /* Optional fused densification statistics (train.py:188-193, scene/gaussian_model.py:456-458): when
   * stats_max_radii2D is non-NULL the per-Gaussian kernel updates the three [P] accumulators in place exactly as
   * dgs_densify_stats(dL_dmeans2D, radii, K, stats_K_total, ...) would right after this backward (same operations,
   * subframe order; nothing is touched when the forward's overflow flag is set), and dL_dmeans2D may then be NULL:
   * the [K,P,3] screen gradient is neither written nor re-read.  stats_K_total: len(render_pkgs) of the whole view
   * (0 = K). */
  float* stats_max_radii2D;
  float* stats_grad_accum;
  float* stats_denom;
  int32_t stats_K_total;
} DgsBackwardIO;

/* Byte offsets of the sub-arrays inside the three blobs (for debuggers and the parity tests).
 * Element types: rows f32[12] = {x, y, conic.x, conic.y, conic.z, opacity, r, g, b, depth, u32 (unused),
 * i32 radius}; keys u64 = ((k*T + tile) << 32) | depth_bits; ranges uint2 per (k, tile). */
typedef struct DgsLayout {
  /* geometry blob */
  size_t geom_rows;      /* f32 [K,P,12] */
  size_t cov3D;          /* f32 [P,6] */
  size_t pre_sigmoid;    /* f32 [K,P,3]  pre-activation colour (sigmoid) or 0/1 clamp mask (relu) */
  size_t tiles_touched;  /* u32 [K*P] */
  size_t point_offsets;  /* u32 [K*P] tile_cull = 0 only, by natural (k, Gaussian) index: index of the pair's first
                          * duplicate = first contribution row of the backward (duplicates are laid out in (k, depth,
                          * index) order; undefined for invisible pairs).  With tile culling the backward uses
                          * offs_tight (same order as tt_tight) and the emission index in the low key word. */
  size_t scan_tmp;       /* u32 scan block sums */
  size_t num_rendered;   /* u32 [8] status words: [0],[1] rectangle total lo/hi (tile_cull = 0), [2],[3] surviving total lo/hi
                          * (tile_cull = 1), [4] the count the lists were built with, [5] overflow flag (capacity mode) */
  size_t gsort_keys;     /* u32 [K,P] bits(depth) - bits(0.2f) (0xFFFFFFFF = invisible): keys of the segmented depth sort */
  size_t gsort_keys_alt; /* u32 [K,P] its ping-pong buffer */
  size_t gsort_vals;     /* u32 [K*P] flat (k, Gaussian) indices in (k, depth, index) order (the sort's result).  tile_cull = 1:
                          * the invisible pairs are dropped by the first sort pass -- every subframe's segment holds its
                          * visible pairs first (tt_sorted = 1) and UNDEFINED indices behind them (tt_sorted = 0) */
  size_t gsort_vals_alt; /* u32 [K*P] */
  size_t tt_sorted;      /* u32 [K*P] tiles_touched in (k, depth, index) order (tile_cull: 1 / 0 = visible / not) */
  size_t offs_sorted;    /* u32 [K*P] its exclusive prefix sum (tile_cull = 0 only) */
  size_t tt_tight;       /* u32 [K*P] tile_cull: surviving tiles per (k, Gaussian), same order */
  size_t offs_tight;     /* u32 [K*P] its exclusive prefix sum (its total is R under tile_cull) */
  size_t gsort_tmp;      /* u32 radix tables of the Gaussian sort */
  size_t cull_rec;       /* u32 [K*P,4] tile_cull: per (k, Gaussian), natural order: rectangle (minx | miny << 12 | (width-1) << 24, or
                          * bit 31 = more than 64 tiles), surviving tiles, hit bits of the rectangle's first 64 tiles (u64) */
  size_t cull_cnt;       /* u32 [K*P] tile_cull: the surviving-tile counts alone, natural order */
  size_t geom_total;
  /* image blob */
  size_t final_T;        /* f32 [K,H*W] */
  size_t n_contrib;      /* u32 [K,H*W] */
  size_t ranges;         /* u32 [K*T,2] */
  size_t image_total;
  /* binning blob */
  size_t keys_sorted;    /* u64 [R] */
  size_t point_list;     /* u32 [R] sorted Gaussian ids */
  size_t keys_unsorted;  /* u64 [R] (also the sort's ping-pong buffer) */
  size_t vals_unsorted;  /* u32 [R] */
  size_t sort_tmp;       /* u32 radix histogram table */
  size_t binning_total;
  int32_t sort_bits;     /* 32 + bits(K*T): width of the reference-compatible key */
  int32_t sort_passes;   /* digit passes of the duplicate sort (over the tile bits only) */
  /* tile_cull = 1 with wide_records = 0 only, when bits(K*T) + bits(P) + bits(R) <= 64 (else both are 0 and keys /
   * point_list are as above):
   * the key is the whole record, (tile << pack_tile_shift) | (Gaussian << pack_g_shift) | emission index, point_list /
   * vals_unsorted stay unused and the sort moves 8 instead of 12 bytes per duplicate and pass. */
  int32_t pack_g_shift;
  int32_t pack_tile_shift;
} DgsLayout;

int dgs_abi_version(void);
const char* dgs_last_error(void);
/* SHA-256 (64 hex digits) over the sources this binary was built from -- every .hip and .h file of deblurgs_amd/csrc, include/dgs_hip.h --
 * and the compiler flag table of deblurgs_amd/build.py, computed by the build and compiled in.  A loader that has the
 * sources at hand (deblurgs_amd/_lib.py) recomputes it and refuses a stale binary; bench.py prints it. */
const char* dgs_build_id(void);

size_t dgs_geom_state_bytes(int32_t P, int32_t K);
size_t dgs_image_state_bytes(int32_t W, int32_t H, int32_t K);
size_t dgs_image_state_bytes_forward_only(int32_t W, int32_t H, int32_t K); /* DgsProblem.forward_only = 1: tile ranges only */
size_t dgs_binning_state_bytes(uint64_t R, int32_t W, int32_t H, int32_t K);
size_t dgs_backward_scratch_bytes(uint64_t R, int32_t P, int32_t K);
/* wide_records: DgsProblem.wide_records of the problem the layout is for (it only decides pack_g_shift / pack_tile_shift;
 * the offsets and totals do not depend on it). */
int dgs_layout(int32_t P, int32_t W, int32_t H, int32_t K, uint64_t R, int32_t wide_records, DgsLayout* out);
/* Byte offsets inside DgsBackwardIO.scratch (for debuggers and the parity tests): contribution rows f32 [R,12] at 0
 * ([S_wx, S_wy, S_xx, S_xy, S_yy, S_w, dL_dr, dL_dg, dL_db, dL_ddepth, -, -] per duplicate, in emission order), their
 * per-(subframe, Gaussian) totals f32 [K*P,16] at *sums_offset (the same 12 columns in 64-byte slots, the last 4 floats
 * unused; natural index k*P + g; defined for visible pairs only; the
 * reference's per-Gaussian sinks follow from them as dL_dconic = -0.5 (S_xx, S_xy, S_yy), dL_dopacity = S_w / opacity,
 * backward.cu:620-637), the per-block pose-gradient partials at *partials_offset. */
int dgs_backward_scratch_layout(uint64_t R, int32_t P, int32_t K, size_t* sums_offset, size_t* partials_offset);

/* Replaces Rasterizer::forward up to the host read of num_rendered (rasterizer_impl.cu:198-287):
 * preprocess for all K subframes + prefix sum, then an async copy of R to out->num_rendered_host. */
int dgs_forward_geometry(const DgsProblem* p, const DgsForwardOut* out, dgs_stream_t stream);
/* Replaces the rest of Rasterizer::forward (rasterizer_impl.cu:289-345): duplicateWithKeys, the stable
 * radix sort, identifyTileRanges and the per-tile alpha compositing, for all K subframes. */
int dgs_forward_render(const DgsProblem* p, const DgsForwardOut* out, uint32_t num_rendered, dgs_stream_t stream);
/* Single-call forward for callers that size the duplicate arrays AHEAD of the count (from the previous step's count,
 * say): dgs_forward_geometry + dgs_forward_render without the host read in between.  binning_state must hold
 * dgs_binning_state_bytes(capacity, ...).  num_rendered_host (pinned, >= 4 words) receives asynchronously
 * [0] the true duplicate count, [1] its u32-overflow word, [2] overflow flag (count > capacity or [1] != 0: the lists
 * were NOT built, the outputs are meaningless and dgs_backward on this state returns garbage-but-in-bounds results;
 * re-run with a larger capacity), [3] the count the lists were built with, [4] the running drop_counter (if given) --
 * written by the forward's finalize kernel itself when the block is device-accessible pinned memory (no copy in the
 * launch chain), by asynchronous copies otherwise.
 * The same flag is the device word at
 * geom_state + DgsLayout.num_rendered + 20 bytes, which dgs_adam_step / dgs_densify_stats accept as `skip_flag` so that
 * a whole training step can be enqueued without any host synchronisation and still never apply a truncated gradient.
 * dgs_backward takes num_rendered = capacity for such a state. */
int dgs_forward(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream);
/* dgs_forward in two parts, for callers that pipeline subframe groups over streams: dgs_forward_lists (preprocess, depth
 * order, tile culling, duplication, sort, tile ranges: the HBM-bound half) and dgs_forward_composite (the per-tile
 * compositing of the lists the first call built: the VALU-bound half).  Same arguments as dgs_forward. */
int dgs_forward_lists(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream);
int dgs_forward_composite(const DgsProblem* p, const DgsForwardOut* out, uint32_t capacity, dgs_stream_t stream);
/* Replaces Rasterizer::backward (rasterizer_impl.cu:350-463).
 * With a context (DgsProblem.context) whose bwd_overlap allows it, an EAGERLY enqueued call for a large view (tile_cull,
 * K >= 6, >= 4 M duplicates) runs the compositing backward in up to three parts of the subframes and the per-pair totals
 * of every part but the last on the context's side stream, forked from and joined back into `stream` inside the call
 * (events; joined also when an enqueue fails half-way): ordering on `stream` is unchanged, results are bit-identical.
 * Not while `stream` is being captured (unless bwd_overlap = 3), not while the context's stage timers are on, not in
 * debug mode, never without a context. */
int dgs_backward(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream);
/* dgs_backward in three parts, for callers that overlap the gradient all-reduce of a sharded run with the backward's
 * tail: dgs_backward_composite (compositing backward + per-(subframe, Gaussian) totals), then dgs_backward_geometry for
 * consecutive Gaussian-index chunks [g_begin, g_end) (g_begin a multiple of 256; each call writes exactly those rows of
 * the per-Gaussian outputs, so chunk i can be all-reduced on another stream while chunk i + 1 runs), then
 * dgs_backward_pose (dL_dviewmatrix / dL_dprojmatrix from the partial sums all chunks left).  Bit-identical to
 * dgs_backward for any chunking. */
int dgs_backward_composite(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream);
int dgs_backward_geometry(const DgsProblem* p, const DgsBackwardIO* io, int32_t g_begin, int32_t g_end,
                          dgs_stream_t stream);
int dgs_backward_pose(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream);
/* How many parts an eagerly enqueued dgs_backward / dgs_backward_composite of such a view runs its compositing in with
 * this context (1 = one launch: no context, small view, K < 6, no tile culling, or bwd_overlap = 0).  For callers that
 * choose between replaying a captured step (always one launch) and enqueueing it eagerly: deblurgs_amd/fused_step.py does. */
int32_t dgs_backward_parts(const DgsContext* ctx, int32_t K, uint64_t num_rendered, int32_t tile_cull);
/* ABI 15.  The backward of a caller that optimises the CAMERAS only -- the test-view pose fit of the reference's evaluation
 * (test.py:131-186: one render, a loss, a backward into the camera, one Adam step on a quaternion and a translation,
 * tens of thousands of times per evaluation).  Reads what dgs_backward reads -- the state blobs, num_rendered, radii,
 * dL_dout_color, optional dL_dout_depth, scratch (>= dgs_backward_scratch_bytes) -- and writes ONLY dL_dviewmatrix and
 * dL_dprojmatrix [K,4,4]: the compositing backward without its colour sums, the per-pair totals of the columns that are
 * left, then a per-Gaussian kernel that keeps the pose terms alone (no SH backward, no covariance -> scale / rotation
 * chain, no per-Gaussian store).  The two matrices agree with dgs_backward's to fp32 rounding -- the same expressions
 * compiled into two kernels contract different multiplies into FMAs: 3e-6 .. 9e-6 of the largest entry measured, held to
 * 1e-4 by the tests -- NOT bit for bit; they are bit-reproducible from call to call.  The scratch holds this call's own
 * row layout afterwards (eight columns per row), not dgs_backward's.  Every other gradient pointer and every stats_* field of `io` may be NULL and is never
 * dereferenced.  Any K in 1..DGS_MAX_K, both tile_cull values, raw_params 0 / 1 / 3, colors_precomp, cov3D_precomp;
 * DGS_E_ARG for a forward_only problem and for a NULL pose output.  On a state whose lists were truncated (status word
 * [5], capacity mode) the kernels return at once and the outputs are meaningless, as dgs_backward's are: the caller
 * discards the step (skip_flag).  Always one launch chain on `stream`: the context's side stream is never used, so the
 * call can be captured into a graph with no fork. */
int dgs_backward_pose_only(const DgsProblem* p, const DgsBackwardIO* io, dgs_stream_t stream);
/* Replaces Rasterizer::markVisible (rasterizer_impl.cu:141-153); present is bool[P] as bytes. */
int dgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, dgs_stream_t stream);

/* Stand-alone building blocks, exported so the parity tests can pin them against numpy
 * (cub::DeviceScan::InclusiveSum / cub::DeviceRadixSort::SortPairs call sites,
 * rasterizer_impl.cu:166,188-191,283,309-314). */
size_t dgs_scan_tmp_bytes(uint64_t n);
/* total_out (optional) receives uint32[2] = {sum mod 2^32, high 32 bits of the 64-bit sum} */
int dgs_exclusive_scan_u32(const uint32_t* in, uint32_t* out, uint64_t n, void* tmp, uint32_t* total_out,
                           dgs_stream_t stream);
size_t dgs_sort_tmp_bytes(uint64_t n);
/* Stable LSD radix sort of (u64 key, u32 value) pairs on key bits [begin_bit, end_bit).  Both buffer pairs are
 * clobbered; *result_in_alt tells which pair holds the result (0: keys/vals, 1: keys_alt/vals_alt). */
int dgs_sort_pairs(uint64_t* keys, uint32_t* vals, uint64_t* keys_alt, uint32_t* vals_alt, uint64_t n,
                   int32_t begin_bit, int32_t end_bit, void* tmp, int32_t* result_in_alt, dgs_stream_t stream);

/* The depth order of the fused rasteriser on its own (the stage between preprocess and duplicateWithKeys; the reference
 * sorts depth inside its one 64-bit cub sort, rasterizer_impl.cu:306-314): K independent stable sorts of P u32 keys,
 * key = bits(view depth) - bits(0.2f) for a visible (subframe, Gaussian) pair, 0xFFFFFFFF for an invisible one.
 * order[K*P] receives the flat indices k * P + g in (k, key, g) order; visible (optional, [K*P]) 1 / 0 in that order.
 * keys, keys_alt, order_alt are clobbered; tmp: dgs_depth_order_tmp_bytes(K, P) bytes.  Three 9-bit passes when every
 * visible key is below 2^27 - 1 (depth < 13107), a fourth one otherwise -- decided on the device. */
size_t dgs_depth_order_tmp_bytes(int32_t K, int32_t P);
int dgs_depth_order(uint32_t* keys, uint32_t* keys_alt, uint32_t* order, uint32_t* order_alt, int32_t K, int32_t P,
                    void* tmp, uint32_t* visible, dgs_stream_t stream);

/* Fused loss-gradient image (train.py:143-165, utils/loss_utils.py:17-18,80-93): from the K rendered subframes
 * and the target, produces blur = mean_k, the L1 and temporal-smoothness loss values and/or dL/dsubframes in one pass.
 * `losses` is an 8-float (32-byte) work area whose first two words receive {l1, smooth}; the totals are formed with
 * integer (2^-24 fixed-point) atomics and are therefore bitwise reproducible; a NaN / Inf among the inputs, or a total
 * beyond the fixed-point range (2^40), makes both values NaN.  Forward call: blur + losses non-null, dL_dsubframes NULL.  Backward call: losses
 * NULL, dL_dsubframes non-null, `upstream` = device pointer to the scalar dL/d(l1 + lambda_t*smooth) (NULL = 1); blur
 * is then an optional INPUT (the forward call's blur, which saves re-summing the K subframes; NULL = recompute).
 * All three outputs non-null computes everything at once. */
int dgs_blur_loss_grad(const float* subframes, const float* gt, int32_t K, int32_t C, int32_t HW, float lambda_t,
                       const float* upstream, float* blur, float* dL_dsubframes, float* losses, dgs_stream_t stream);

/* The same with lambda_t read from device memory when the kernel runs: the scheduled weight of a captured (hipGraph)
 * training step changes between replays without re-capturing. */
int dgs_blur_loss_grad_dev(const float* subframes, const float* gt, int32_t K, int32_t C, int32_t HW,
                           const float* lambda_t_dev, const float* upstream, float* blur, float* dL_dsubframes,
                           float* losses, dgs_stream_t stream);

/* Multi-GPU runs, "subframes" sharding (new work, the reference is single-GPU): the loss block of ONE RANK, which
 * holds K_local consecutive subframes [K_local,C,HW] of a view's K_total.  blur [C,HW] = the view's blur image (mean over
 * all K_total subframes, after the ranks' partial sums have been all-reduced), prev_last / next_first [C,HW] = the boundary
 * subframes of the neighbouring ranks (NULL at the ends of the view).  Writes dL/dsubframes of the local subframes (the
 * formula of dgs_blur_loss_grad with K = K_total) and, in the 8-float work area `losses`: [0] mean |blur - gt| (the same
 * on every rank), [1] this rank's share of the temporal-smoothness value (the differences whose LEFT frame it holds,
 * over E (K_total - 1)): the caller sums the shares over the ranks.  Same deterministic fixed-point totals.  K_local <= 32. */
int dgs_blur_loss_slice_grad(const float* subframes, const float* prev_last, const float* next_first, const float* blur,
                             const float* gt, int32_t K_local, int32_t K_total, int32_t C, int32_t HW, float lambda_t,
                             float* dL_dsubframes, float* losses, dgs_stream_t stream);

/* A few words (n_words <= 4096) copied BY A KERNEL on `stream`: dst and src may each be device memory or pinned host
 * memory (hipHostMalloc / torch pin_memory / hipHostRegister: resolved through hipHostGetDevicePointer; the kernel stores
 * with system scope and fences, so a pinned destination is complete when the stream reaches the caller's next event).  What a captured training step's per-step scalars travel
 * with: an asynchronous host-to-device copy in front of every graph launch costs a hand-over between the copy engine and
 * the compute queue (tens of microseconds); a kernel in front of the graph costs one launch.  Pageable host memory falls
 * back to hipMemcpyAsync. */
int dgs_copy_words(void* dst_dev, const void* src, int32_t n_words, dgs_stream_t stream);

/* Densification-statistic consumers of the rasteriser's per-subframe outputs (train.py:188-193 with
 * scene/gaussian_model.py:456-458), for all K subframes in one pass and in subframe order:
 *   visible = radii[k] > 0;  max_radii2D = max(max_radii2D, radii[k]);
 *   xyz_gradient_accum += || viewspace_grad[k][:, :2] ||;  denom += 1/K_total.
 * viewspace_grad is the [K,P,3] gradient of the means2D carrier, radii is [K,P]; the three accumulators are [P].
 * K_total = len(render_pkgs) of the whole view (train.py:192): K itself (pass 0) unless the view's subframes are
 * split over ranks and this call covers only a rank's share. */
int dgs_densify_stats(const float* viewspace_grad, const int32_t* radii, int32_t K, int32_t K_total, int32_t P,
                      float* max_radii2D, float* xyz_gradient_accum, float* denom, const uint32_t* skip_flag,
                      dgs_stream_t stream);

/* ---- optimiser step and densification of the Gaussian cloud ----------------------------------
 * Multi-tensor Adam: all parameter groups in one launch.  Replaces torch.optim.Adam(l, lr=0.0, eps=1e-15).step()
 * over the six per-Gaussian groups (scene/gaussian_model.py:170-195, train.py:203-208) with the same arithmetic
 * (torch/optim/adam.py, single-tensor path: lerp, mul+addcmul, sqrt/div/add, addcdiv; bias corrections in double).
 * `step` is the 1-based count of THIS update (state["step"] after its increment).  A group whose grad is NULL is
 * skipped, like a parameter whose .grad is None.  clip_value > 0 clamps the gradient first
 * (torch.nn.utils.clip_grad_value_, train.py:204-205); the gradient buffer itself is left untouched.
 * skip_flag (optional device word, see dgs_forward): non-zero = the launch leaves parameters and moments untouched. */
#define DGS_ADAM_MAX_GROUPS 16
typedef struct DgsAdamGroup {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  uint64_t numel;
  double lr;      /* python floats stay double up to the point where torch casts them (step_size, 1 - beta) */
  int32_t step;
} DgsAdamGroup;
int dgs_adam_step(const DgsAdamGroup* groups, int32_t n_groups, double beta1, double beta2, double eps,
                  double clip_value, const uint32_t* skip_flag, dgs_stream_t stream);

/* densify_and_prune (scene/gaussian_model.py:436-448 = densify_and_clone :419-434, densify_and_split :389-417,
 * prune_points :336-349 with the optimiser-state surgery of :315-334 / :359-387) as plan + apply.
 * Arrays of the cloud, in the order xyz[P,3], f_dc[P,3], f_rest[P,n_rest], opacity[P,1], scaling[P,3],
 * rotation[P,4] (raw parameters), with the two Adam moments of each (exp_avg / exp_avg_sq may be NULL in the
 * source = no optimiser state yet = zeros). */
typedef struct DgsCloudArrays {
  float* param[6];
  float* exp_avg[6];
  float* exp_avg_sq[6];
} DgsCloudArrays;
/* For captured (hipGraph) training steps: the per-group scalars that depend on the step count and the learning rate --
 * out[2 i] = -(lr_i / (1 - beta1^step_i)), out[2 i + 1] = sqrt(1 - beta2^step_i), exactly as dgs_adam_step forms them --
 * are computed on the host by dgs_adam_scalars, copied by the caller into device memory before every replay, and read
 * from there (dev_scalars, same group order) by the kernel that dgs_adam_step_dev enqueues; the lr / step fields of the
 * groups passed to dgs_adam_step_dev itself are not used. */
int dgs_adam_scalars(const DgsAdamGroup* groups, int32_t n_groups, double beta1, double beta2, float* out);
int dgs_adam_step_dev(const DgsAdamGroup* groups, int32_t n_groups, double beta1, double beta2, double eps,
                      double clip_value, const uint32_t* skip_flag, const float* dev_scalars, dgs_stream_t stream);

/* Adam over a whole EPOCH of the test-view pose fit in one launch (evaluation.EpochPoseFit).  The groups are [n, w]
 * tensors (numel = n w, w <= 64; at most 4 groups) whose row r receives a non-zero gradient at exactly one of the epoch's
 * n_steps dense steps -- step pos[r] (device int32 [n]; a value outside [0, n_steps) counts as 0) -- and zeros at all
 * others.  Adam is elementwise and the rows never interact, so the n_steps updates of an element are applied one after
 * the other by one thread: the statements of dgs_adam_step each time (a zero-gradient step is that update with g = 0:
 * the moments decay, the parameter moves by its momentum), step j with scalars[j] -- device floats [n_steps, 2 n_groups],
 * row j = what dgs_adam_scalars writes for step j's count and learning rates.  The lr / step fields are not used.
 *   peek: for rows [row_begin, row_end), the parameters after the pos[r] zero-gradient steps that precede the row's
 *         turn -- what the row's gradient has to be evaluated at -- written to peek_out[i] (host array of n_groups device
 *         tensors shaped like the parameters; only the rows of the range are written).  Reads no gradient, changes no state.
 *   step: for rows [row_begin, row_end), from the epoch-start state: pos[r] zero-gradient steps, the step with row r of
 *         `grad`, n_steps - 1 - pos[r] more zero-gradient steps; parameter and both moments written.  Bit-identical to
 *         n_steps dgs_adam_step_dev launches on dense gradients that are zero outside row order[j] at step j.
 *         skip_flag (optional device word): non-zero = nothing is written for the whole epoch. */
int dgs_adam_epoch_peek(const DgsAdamGroup* groups, int32_t n_groups, float* const* peek_out, int32_t n, int32_t row_begin,
                        int32_t row_end, const int32_t* pos, const float* scalars, int32_t n_steps, double beta1,
                        double beta2, double eps, dgs_stream_t stream);
int dgs_adam_epoch_step(const DgsAdamGroup* groups, int32_t n_groups, int32_t n, int32_t row_begin, int32_t row_end,
                        const int32_t* pos, const float* scalars, int32_t n_steps, double beta1, double beta2, double eps,
                        const uint32_t* skip_flag, dgs_stream_t stream);

/* Multi-GPU runs (new work, the reference is single-GPU): the local half of a direct reduce-scatter over
 * point-to-point transfers.  `own` [n] is this rank's shard of the gradient bucket, `recv` [world, stride] holds the copy
 * received from every peer in row s = its rank (row `rank` is not read); own <- ((row_0 + row_1) + row_2) + ... with `own`
 * standing in for row `rank`, added IN RANK ORDER so every rank computes the same bits for a given set of inputs, then
 * divided by `divisor` (1 = sum, world = mean).  stride >= n, world <= 64. */
int dgs_rank_ordered_sum(const float* recv, uint64_t stride, float* own, uint64_t n, int32_t world, int32_t rank,
                         float divisor, dgs_stream_t stream);

size_t dgs_densify_tmp_bytes(int32_t P);
/* plan: per Gaussian, grads = xyz_gradient_accum / denom (NaN -> 0); clone if |grads| >= grad_threshold and
 * max(exp(scaling)+scale_lb) <= size_threshold (= percent_dense * extent); split if grads >= grad_threshold and
 * max(...) > size_threshold; every Gaussian whose clamp(opacity, 0, 1) < min_opacity is pruned together with its
 * clone / children (they inherit its opacity).  flags and offsets are u32 [4,P] (keep, clone, split, split-selected
 * before the opacity prune) and their exclusive scans; counts_host (pinned, u32[4]) receives the four totals by an
 * async copy: {n_keep, n_clone, n_split, m_all}.  The new cloud has n_keep + n_clone + 2 n_split Gaussians. */
int dgs_densify_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling,
                     const float* opacity, float grad_threshold, float size_threshold, float min_opacity,
                     float scale_lb, int32_t isotropic, uint32_t* flags, uint32_t* offsets, uint32_t* counts_dev,
                     uint32_t* counts_host, void* tmp, dgs_stream_t stream);
/* apply: writes the new cloud in the reference's order [surviving originals | clones | children copy 0 | children
 * copy 1]; clones and children get zero Adam moments; a child is xyz + R(rotation) (std * z), scaling
 * log(max(std / 1.6 - scale_lb, 0.001)) with std = exp(scaling) + scale_lb, and z = noise[c * m_all + rank] the
 * caller's standard-normal samples [2 m_all, 3] (the reference draws torch.normal(0, stds) for every selected
 * Gaussian and copy before the opacity prune).  isotropic != 0 (both calls): std = exp(scaling[:, 0]) + scale_lb for all
 * three axes (use_isotrophic clouds): size test, child offsets and all three child scaling columns use it; survivors
 * and clones copy the raw rows unchanged.  counts = the host copy {n_keep, n_clone, n_split, m_all}. */
int dgs_densify_apply(int32_t P, int32_t n_rest, const uint32_t* counts, const uint32_t* flags, const uint32_t* offsets,
                      const DgsCloudArrays* src, const DgsCloudArrays* dst, const float* noise, float scale_lb,
                      int32_t isotropic, dgs_stream_t stream);

/* ---- initialisation: mean squared distance to the 3 nearest neighbours -------------------------
 * Replaces simple_knn._C.distCUDA2 (submodules/simple-knn/spatial.cu:15-26, simple_knn.cu:138-221), which
 * create_from_pcd uses for the initial scales (scene/gaussian_model.py:148-156): mean_dist2[i] = mean of the three
 * smallest |p_j - p_i|^2 over j != i (exact search; duplicates count with distance 0; fewer than three neighbours
 * leave FLT_MAX terms, i.e. +inf, like the reference).  points is [P,3] fp32, tmp >= dgs_knn_tmp_bytes(P). */
size_t dgs_knn_tmp_bytes(int32_t P);
int dgs_knn_mean_dist2(int32_t P, const float* points, float* mean_dist2, void* tmp, dgs_stream_t stream);

/* Pose path of the blur-integration loop on device: Bezier curves in se(3) evaluated at the K
 * subframe times nu, se3_exp_map, and the three camera tensors render() reads -- scene/bezier.py:54-83,
 * utils/pytorch3d_functions.py:373-457, scene/motion.py:248-294, scene/cameras.py:63-74 -- as one kernel, and its
 * backward from dL/d{world_view, full_proj} to the control points and nu.  ctrl_* are [C+1,3] (one curve),
 * proj is the transposed projection matrix [4,4] (row-vector convention), outputs are [K,4,4], [K,4,4], [K,3].
 * quaternion != 0: curve_type "quarternion_cartesian" (scene/motion.py:191-194,242-246): ctrl_rot is [C+1,4], a
 * quaternion curve (x, y, z, w) that is normalised and turned into the c2w rotation, ctrl_trans the camera origin. */
/* Subframe times of one view from its alignment parameters (scene/motion.py:209-219):
 * nu = sort(clamp(cat(0, sigmoid(raw) [+ uniform / n_subframes - 1 / (2 n_subframes)], 1), 0, 1)), f values from the
 * f - 2 raw ones (uniform: optional [f-2] samples of U(0,1), the reference's curve_random_sample); src[r] = index of
 * the candidate that landed at sorted position r (stable ascending sort).  Backward: dL/draw from dL/dnu (zero where
 * the clamp was active, end points carry no parameter).  f <= DGS_MAX_K. */
int dgs_alignment_forward(const float* raw, const float* uniform, int32_t f, int32_t n_subframes, float* nu,
                          int32_t* src, dgs_stream_t stream);
int dgs_alignment_backward(const float* raw, const float* uniform, int32_t f, int32_t n_subframes, const int32_t* src,
                           const float* dL_dnu, float* dL_draw, dgs_stream_t stream);
size_t dgs_pose_scratch_bytes(int32_t K);
int dgs_pose_forward(const float* ctrl_trans, const float* ctrl_rot, const float* nu, const float* proj, int32_t C,
                     int32_t K, int32_t quaternion, float* view, float* full, float* campos, dgs_stream_t stream);
int dgs_pose_backward(const float* ctrl_trans, const float* ctrl_rot, const float* nu, const float* proj, int32_t C,
                      int32_t K, int32_t quaternion, const float* dL_dview, const float* dL_dfull, void* scratch,
                      float* dL_dctrl_trans, float* dL_dctrl_rot, float* dL_dnu, dgs_stream_t stream);

/* ---- evaluation protocol (ABI 15; test.py:72-186 of the reference) ------------------------------------------------
 * The pose chain of the test-view fit for ONE view (OptimPoseModel.forward, test.py:72-91): rot [n,4] quaternions in
 * (x, y, z, w) order, trans [n,3];  q = rot[idx] + 1e-8, unit quaternion, rotation matrix (the arithmetic of the
 * "quarternion_cartesian" curve of dgs_pose_forward), world_view[:3,:3] = R, world_view[3,:3] = trans[idx],
 * full_proj = world_view @ proj (proj: the transposed projection matrix, as for dgs_pose_forward),
 * camera_center = inverse(world_view)[3,:3].  Outputs view / full [4,4], campos [3].  The view's index is read from
 * device memory when the kernel runs (idx_dev, one int32; a captured step serves every view) or, with idx_dev = NULL,
 * taken from `idx`; a device-side index outside [0, n) selects view 0.
 * Backward: dL/d{world_view, full_proj} -> dL_drot [n,4], dL_dtrans [n,3], FULLY written: row idx receives the gradient,
 * every other row zeros (the dense gradient torch leaves on an indexed parameter, which a dense Adam then consumes).  The
 * camera centre carries no gradient (the rasteriser returns none for campos). */
int dgs_testpose_forward(const float* rot, const float* trans, const int32_t* idx_dev, int32_t idx, int32_t n,
                         const float* proj, float* view, float* full, float* campos, dgs_stream_t stream);
int dgs_testpose_backward(const float* rot, const float* trans, const int32_t* idx_dev, int32_t idx, int32_t n,
                          const float* proj, const float* dL_dview, const float* dL_dfull, float* dL_drot,
                          float* dL_dtrans, dgs_stream_t stream);
/* The same chain for the views [row_begin, row_end) of rot [n,4] / trans [n,3] at once (at most DGS_MAX_K of them): slot
 * k = row - row_begin of view / full [G,4,4] and campos [G,3]; backward from dL_dview / dL_dfull [G,4,4] into rows
 * [row_begin, row_end) of dL_drot [n,4] / dL_dtrans [n,3] -- the other rows are NOT written.  One body with the
 * single-view kernels: every row's results are theirs bit for bit. */
int dgs_testpose_forward_rows(const float* rot, const float* trans, int32_t n, int32_t row_begin, int32_t row_end,
                              const float* proj, float* view, float* full, float* campos, dgs_stream_t stream);
int dgs_testpose_backward_rows(const float* rot, const float* trans, int32_t n, int32_t row_begin, int32_t row_end,
                               const float* proj, const float* dL_dview, const float* dL_dfull, float* dL_drot,
                               float* dL_dtrans, dgs_stream_t stream);

/* The loss of one step of that fit (test.py:171-178) for one image x [C,HW]:
 *   y = clamp(tone_map(x), 0, 1);  l1 = mean |y - gt|;  mse = mean (y - gt)^2;  dL_dx = upstream * d l1 / dx
 * tone_map: DGS_TONE_IDENTITY, or DGS_TONE_GAMMA = max((x - bound) / (1 - 2 bound), eps) ^ (1 / 2.2) (scene/tonemapping.py).
 * Derivative conventions are torch's: clamp and clamp_min pass the gradient where the input is inside or ON the bound,
 * sign(0) = 0.  gt: the image (n_gt = 1, gt_index_dev = NULL), or with gt_index_dev (one device int32, read when the
 * kernel runs) image gt_index_dev[0] of a stack [n_gt,C,HW]; an index outside [0, n_gt) selects image 0, as an index
 * outside [0, n) selects view 0 in dgs_testpose_*: nothing is read out of bounds.  upstream: optional device scalar (NULL = 1).  dL_dx [C,HW] and `work` are each optional (not both
 * NULL).  work: a 12-word (48-byte, 8-byte aligned) area -- [0] l1, [1] mse as fp32, words [8..9] / [10..11] the same two
 * values as fp64, the rest scratch of the deterministic fixed-point totals (same scheme and the same NaN rule as
 * dgs_blur_loss_grad).  l2_ema (optional device float, needs work): l2_ema = 0.6 l2_ema + 0.4 mse, the reference's
 * l2_error_ema, kept on the device; left alone when skip_flag (optional, see dgs_forward) is non-zero. */
#define DGS_TONE_IDENTITY 0
#define DGS_TONE_GAMMA 1
int dgs_view_loss_grad(const float* x, const float* gt, const int32_t* gt_index_dev, int32_t n_gt, int32_t C, int32_t HW,
                       int32_t tone_mapping, float eps, float bound, const float* upstream, float* dL_dx, float* work,
                       float* l2_ema, const uint32_t* skip_flag, dgs_stream_t stream);
/* That loss for G = row_end - row_begin images in one launch (at most DGS_MAX_K): image k of x [G,C,HW] against image
 * row_begin + k of the stack gt [n_gt,C,HW], gradient image k of dL_dx [G,C,HW] (optional), work area k of work [G,12].
 * Every image gets the block grid dgs_view_loss_grad gives it (a function of C HW only), with the image index on the
 * grid's second axis, and its own 1 / (C HW): its totals, values and gradient are those of a dgs_view_loss_grad call on
 * it, bit for bit (a NaN in one image reaches that image's values only). */
int dgs_view_loss_grad_rows(const float* x, const float* gt, int32_t n_gt, int32_t row_begin, int32_t row_end, int32_t C,
                            int32_t HW, int32_t tone_mapping, float eps, float bound, const float* upstream, float* dL_dx,
                            float* work, dgs_stream_t stream);
/* l2_error_ema over an epoch: l2_ema = 0.6 l2_ema + 0.4 mse_j for the epoch's views IN THE ORDER OF THEIR TURNS, by one
 * thread.  work [n,12]: the views' work areas by row (word [1] = mse); pos (device int32 [n]): the turn of row r, i.e.
 * the inverse of the epoch's order (what dgs_adam_epoch_* read; a position outside [0, n) drops its row).  n <= DGS_MAX_K.
 * Groups (optional, n_groups = 0: none): host arrays skip_flags [n_groups] of device words and group_begin
 * [n_groups + 1] rising from 0 to n; the rows [group_begin[g], group_begin[g + 1]) do not count when *skip_flags[g] is
 * non-zero (a NULL word never skips). */
int dgs_l2_ema_epoch(const float* work, const int32_t* pos, int32_t n, const uint32_t* const* skip_flags,
                     const int32_t* group_begin, int32_t n_groups, float* l2_ema, dgs_stream_t stream);

/* PSNR and SSIM of two [3,H,W] images as the reference's evaluation computes them (test.py:118-119):
 * out[0] = mean over the three channels of 20 log10(1 / sqrt(mse_c)) (utils/image_utils.py:17-19),
 * out[1] = mean of the SSIM map with the 11 x 11 Gaussian window, sigma 1.5, zero padding, per channel
 * (utils/loss_utils.py:23-63).  Forward only; one launch over 16 x 16 tiles (separable window through LDS, fp64
 * arithmetic) plus a reduction in block order: deterministic.  tmp >= dgs_image_metrics_tmp_bytes(W, H).  `out` is FIVE
 * floats: the two values above, then the three per-channel PSNRs out[0] is the mean of.  Identical images give
 * {+inf, 1, +inf, +inf, +inf}. */
size_t dgs_image_metrics_tmp_bytes(int32_t W, int32_t H);
int dgs_image_metrics(const float* a, const float* b, int32_t W, int32_t H, void* tmp, float* out, dgs_stream_t stream);

/* ---- camera-path frames (additions to ABI 15; render_spiral.py:27-35, render_trainview.py:33-52 of the reference) ----
 * K rendered frames color [K,3,H,W] (fp32, the rasteriser's output) -> packed 8-bit frames out [K,h,w,3] of the window
 * rows [y0, y0 + h) x columns [x0, x0 + w), in one pass:  y = tone_map(x) (DGS_TONE_*, the expression and the powf of
 * dgs_view_loss_grad), then (uint8)(min(max(y, 0), 1) * 255.0f) -- numpy's (y.clip(0, 1) * 255.0).astype(uint8), whose cast
 * truncates.  A NaN input writes 0 (numpy leaves that cast undefined).  `out` needs no alignment.  Errors: K < 1 (or above
 * 65535), an empty window or one that leaves the image (or is taller than 65535 rows), a tone id that is neither,
 * bound >= 0.5 with DGS_TONE_GAMMA. */
int dgs_frames_finish(const float* color, int32_t K, int32_t H, int32_t W, int32_t tone_mapping, float eps, float bound,
                      int32_t y0, int32_t x0, int32_t h, int32_t w, uint8_t* out, dgs_stream_t stream);
/* lo_hi[0] = min, lo_hi[1] = max of n floats, left in device memory: per-block fminf / fmaxf, then one block over the
 * blocks' results -- two launches, a block count that depends on n only.  NaNs do not count (torch.min / torch.max return
 * NaN when one is present; the rasteriser's depth holds none); n NaNs leave (+inf, -inf).
 * tmp >= dgs_depth_range_tmp_bytes(n), 4-byte aligned. */
size_t dgs_depth_range_tmp_bytes(uint64_t n);
int dgs_depth_range(const float* depth, uint64_t n, float* lo_hi, void* tmp, dgs_stream_t stream);
/* depth_colorize (utils/export_utils.py:44-65) with its default clip_percentage = 1, the range read from the two device
 * words dgs_depth_range left:  lo = max(z_near, lo_hi[0]), hi = min(z_far, lo_hi[1]), d = clip((x - lo) / (hi - lo), 0, 1),
 * out[e] = lut[min((int)(d * 256), 255)] -- the colour map's own indexing of a float in [0, 1].  lut [256,4] and out [n,4]
 * are RGBA bytes, both 4-byte aligned; the table holds (colour * 255) truncated.  hi == lo or a NaN writes (0, 0, 0, 0), the
 * colour the map gives a value it cannot place. */
int dgs_depth_colorize(const float* depth, uint64_t n, const float* lo_hi, float z_near, float z_far, const uint8_t* lut,
                       uint8_t* out, dgs_stream_t stream);

/* ---- visual reports (additions to ABI 15; test.py:122-126, utils/visualization.py:262-291, utils/colorize.py:63-107 of
 * the reference) ----  Raw device pointers and a stream, nothing kept between calls, no global or float atomics, no
 * device word read by the host; every argument is checked before the first HIP call.
 *
 * Exact order statistics by radix select: out[j] = the element np.sort(x)[ranks[j]] holds, x float32 [n], 1 <= n <= 2^32 - 1,
 * 1 <= m <= 4 host ranks below n.  Four most-significant-first 8-bit passes over the order-preserving key (sign set: ~bits;
 * else bits | 0x80000000; a NaN: 0xFFFFFFFF, so NaNs come last as numpy sorts them; a returned NaN is the quiet positive
 * one); one data pass serves all m ranks.  -0.0 sorts before +0.0 (numpy holds them equal: either may stand at a rank).
 * tmp >= dgs_order_stats_tmp_bytes(n, m) bytes, 4-byte aligned: a function of n and m only (it serves dgs_percentiles
 * with the same n and m too). */
size_t dgs_order_stats_tmp_bytes(uint64_t n, int32_t m);
int dgs_order_stats(const float* x, uint64_t n, const uint64_t* ranks_host, int32_t m, float* out, void* tmp,
                    dgs_stream_t stream);
/* numpy's np.percentile(x, q_tuple) (method "linear", float32 x, float64 results) for 1 <= m <= 4 percentages in
 * [0, 100]: the host forms v = (n - 1) (q / 100) in double, i = floor(v), g = v - i (from v = n - 1 on: i = i + 1 = n - 1
 * and g = v + 1, as numpy forms them there); the device selects a = x_(i) and b = x_(i + 1) (one select of 2 m ranks),
 * d = (float)(b - a), out[j] = (double)a + (double)d g, or (double)b - (double)d (1 - g) when g >= 0.5.
 * out: m float64 device words, 8-byte aligned. */
int dgs_percentiles(const float* x, uint64_t n, const double* q_host, int32_t m, double* out, void* tmp,
                    dgs_stream_t stream);
/* The 8-bit images and the L1 error map of a report in one pass.  x [K,3,H,W] linear renders.  mean = 1: ONE image
 * y = tone_map(s), s = (((x_0 + x_1) + ...) + x_{K-1}) / (float)K summed in order in fp32, gt [3,H,W]; mean = 0: K images
 * y_k = tone_map(x_k), gt [K,3,H,W] (G = 1 or K images leave).  tone_map: DGS_TONE_*, dgs_frames_finish's expression (a
 * NaN input stays NaN).  out_u8 [G,H,W,3] = (uint8)clamp(y * 255 + 0.5, 0, 255), torchvision's save_image rounding, a NaN
 * gives 0; gt_u8 [G,H,W,3] (or NULL) the same of gt itself; err [G,H,W] (or NULL) = ((|gt_r - y_r| + |gt_g - y_g|) +
 * |gt_b - y_b|) / 3.0f with y unclamped: torch.abs(gt - image).permute(1, 2, 0).mean(-1).  gt may be NULL (then gt_u8 and
 * err must be): subframes.  No pointer needs more than its type's alignment. */
int dgs_report_images(const float* x, int32_t K, int32_t mean, int32_t H, int32_t W, int32_t tone_mapping, float eps,
                      float bound, const float* gt, uint8_t* out_u8, uint8_t* gt_u8, float* err, dgs_stream_t stream);
/* colorize_np (utils/colorize.py:87-92) once the range is known: lo_hi two float64 device words (8-byte aligned),
 * c = min(max((double)x, lo), hi), d = (c - lo) / (hi - lo), out[e] = the first three bytes of lut[min((int)(d * 256), 255)]
 * -- float64 throughout, as numpy 2 promotes a float32 array against float64 scalars.  lut [256,4] RGBA bytes, 4-byte
 * aligned; out [n,3] bytes, any alignment.  hi == lo or a NaN in the chain writes (0, 0, 0). */
int dgs_scalar_colorize(const float* x, uint64_t n, const double* lo_hi, const uint8_t* lut, uint8_t* out,
                        dgs_stream_t stream);

/* ---- LPIPS (additions to ABI 15; test.py:120, lpipsPyTorch/modules/{lpips,networks,utils}.py of the reference) ----
 * The reference's third evaluation number, lpips(image, gt_image, net_type='alex'), with CALLER-SUPPLIED weights: the
 * library ships none and fetches none.  The AlexNet `features` shapes and the z-score constants are fixed in the library:
 *   conv_w[0..4]  [64,3,11,11] [192,64,5,5] [384,192,3,3] [256,384,3,3] [256,256,3,3]   (torchvision features.0/3/6/8/10)
 *   conv_b[0..4]  [64] [192] [384] [256] [256]
 *   lin[0..4]     [1,C,1,1], C = 64, 192, 384, 256, 256                                  (LPIPS v0.1 lin{i}.model.1.weight)
 * all fp32, contiguous, in device memory. */
typedef struct DgsLpipsAlexWeights {
  const float* conv_w[5];
  const float* conv_b[5];
  const float* lin[5];
} DgsLpipsAlexWeights;
/* a, b [n_pairs,3,H,W] fp32, used as they come (no rescaling); out [n_pairs,6] = per pair (total, layer 1..5):
 * z-score (x - (-.030, -.088, -.188)) / (.458, .448, .450) before the first convolution (whose zero padding so pads the
 * z-scored image); conv 11x11 /4 pad 2, ReLU, max-pool 3x3 /2, conv 5x5 pad 2, ReLU, max-pool 3x3 /2, three conv 3x3 pad 1
 * each with a ReLU; per ReLU output (before its pool): every pixel's channel vector / (sqrt(sum c^2) + 1e-10), the squared
 * difference of the two maps under the lin weights, the spatial mean; total = the sum of the five.  (The reference's
 * function sums a batch into one number; this returns the pairs one by one.)  fp32 throughout; the convolutions run on the
 * f32-input matrix cores (dgs_conv2d_bias_relu).  Stream-explicit, caller-owned memory, no host synchronisation, no
 * float atomics: a pair's six numbers do not depend on the other pairs of the call or on n_pairs, two runs are bitwise
 * equal, lpips(x, x) is exactly 0 in all six and lpips(x, y) == lpips(y, x) bitwise.
 * tmp >= dgs_lpips_alex_tmp_bytes(W, H, n_pairs) bytes (0: arguments the call refuses), 256-byte aligned.  Refused before
 * any HIP call: a NULL pointer (the fifteen of `w` included), n_pairs < 1 (or above 65535), W or H below 31 -- the
 * smallest image the network accepts, as the reference raises at 30. */
size_t dgs_lpips_alex_tmp_bytes(int32_t W, int32_t H, int32_t n_pairs);
int dgs_lpips_alex(const float* a, const float* b, int32_t n_pairs, int32_t W, int32_t H, const DgsLpipsAlexWeights* w,
                   void* tmp, float* out, dgs_stream_t stream);
/* The convolution of the above on its own: out [n_img,Cout,OH,OW] = relu(conv2d(in [n_img,Cin,IH,IW], weight
 * [Cout,Cin,KH,KW], bias [Cout], stride, zero padding pad)), OH = (IH + 2 pad - KH) / stride + 1.  An implicit GEMM
 * C[Cout x N] = W[Cout x K] . patches[K x N], K = Cin KH KW in the weight's own order, N over the output pixels of all
 * images, patches gathered on the fly, on v_mfma_f32_32x32x2_f32.  Every output element is: per 32 consecutive k one
 * k-ordered fmaf chain from 0, the chains' results added in order with a compensated (Kahan) fp32 sum, + bias, ReLU
 * (a NaN passes) -- whatever its place in the call.  zscore = 1 (Cin = 3): the input is z-scored as above on the way in,
 * the padding stays 0.  KH, KW in 1..15, pad below both.  `out` must not overlap `in`. */
int dgs_conv2d_bias_relu(const float* in, int32_t n_img, int32_t Cin, int32_t IH, int32_t IW, const float* weight,
                         const float* bias, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t zscore,
                         float* out, dgs_stream_t stream);

/* ---- LPIPS with the VGG16 backbone (additions to ABI 15; metrics.py:74, networks.py:88-96 of the reference) ----
 * lpips(x, y, net_type='vgg'), again with CALLER-SUPPLIED weights.  torchvision's VGG16 `features` shapes:
 *   conv_w[0..12]  [Cout,Cin,3,3], Cout = 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512, Cin = 3 and then
 *                  the Cout before                                 (features.0/2/5/7/10/12/14/17/19/21/24/26/28)
 *   conv_b[0..12]  [Cout]
 *   lin[0..4]      [1,C,1,1], C = 64, 128, 256, 512, 512           (LPIPS v0.1 lin{i}.model.1.weight of vgg.pth)
 * all fp32, contiguous, in device memory. */
typedef struct DgsLpipsVggWeights {
  const float* conv_w[13];
  const float* conv_b[13];
  const float* lin[5];
} DgsLpipsVggWeights;
/* As dgs_lpips_alex, with the network z-score, then thirteen conv 3x3 pad 1 each with a ReLU, a max-pool 2x2 /2 (floor)
 * after convolutions 2, 4, 7 and 10; taps: the ReLU outputs of convolutions 2, 4, 7, 10 (each before its pool) and 13.
 * out [n_pairs,6] = per pair (total, layer 1..5).  Every contract of dgs_lpips_alex holds: stream-explicit, caller-owned
 * memory, no host synchronisation, no float atomics, a pair's six numbers independent of the other pairs and of n_pairs,
 * two runs bitwise equal, lpips(x, x) exactly 0 and lpips(x, y) == lpips(y, x) bitwise.
 * tmp >= dgs_lpips_vgg_tmp_bytes(W, H, n_pairs) bytes (0: arguments the call refuses), 256-byte aligned: two ping-pong
 * buffers of the largest layer output [2 n_pairs,64,H,W] and the distance partials -- 2,123,452,928 bytes for one
 * 1920 x 1080 pair.  Refused before any HIP call: a NULL pointer (the thirty-one of `w` included), n_pairs < 1 (or above
 * 65535), W or H below 16 -- the smallest image the network accepts, as the reference raises at 15 -- and 64 H W or
 * 2 n_pairs H W of 2^31 and more. */
size_t dgs_lpips_vgg_tmp_bytes(int32_t W, int32_t H, int32_t n_pairs);
int dgs_lpips_vgg(const float* a, const float* b, int32_t n_pairs, int32_t W, int32_t H, const DgsLpipsVggWeights* w,
                  void* tmp, float* out, dgs_stream_t stream);
/* The 3 x 3 convolution of the above on its own: out [n_img,Cout,IH,IW] = relu(conv2d(in [n_img,Cin,IH,IW], weight
 * [Cout,Cin,3,3], bias [Cout], stride 1, zero padding 1)) on v_mfma_f32_32x32x2_f32, the operands read from an input halo
 * tile in LDS (no patch gather).  Every output element is: per chunk of CC input channels (CC = 4 where Cout <= 64, else
 * 8) one fmaf chain of L = 9 CC terms (36 / 72) from 0 in the k order (ky, kx, ci) -- for each of the nine weights in
 * row-major order the chunk's channels in order, a term past Cin being 0 x 0 --, the chunks' results added in channel
 * order with a compensated (Kahan) fp32 sum, + bias, ReLU (a NaN passes) -- whatever its place in the call.  zscore = 1 (Cin = 3): as dgs_conv2d_bias_relu's.  `out` must not
 * overlap `in`. */
int dgs_conv3x3_bias_relu(const float* in, int32_t n_img, int32_t Cin, int32_t IH, int32_t IW, const float* weight,
                          const float* bias, int32_t Cout, int32_t zscore, float* out, dgs_stream_t stream);
/* max_pool2d(kernel 2, stride 2) of `planes` planes [IH,IW] -> [IH / 2, IW / 2] (floor, no padding; IH, IW >= 2); a NaN in
 * a window is its result.  `out` must not overlap `in`. */
int dgs_maxpool2x2(const float* in, uint64_t planes, int32_t IH, int32_t IW, float* out, dgs_stream_t stream);

/* ---- LPIPS with the SqueezeNet 1.1 backbone (additions to ABI 15; networks.py:69-77 of the reference) ----
 * lpips(x, y, net_type='squeeze'), again with CALLER-SUPPLIED weights.  torchvision's squeezenet1_1().features shapes:
 *   conv_w, conv_b   [64,3,3,3], [64]                                                        (features.0)
 *   fire[0..7]       the Fire modules features.3/4/6/7/9/10/11/12, (Cin, S, E) = (64,16,64) (128,16,64) (128,32,128)
 *                    (256,32,128) (256,48,192) (384,48,192) (384,64,256) (512,64,256): squeeze_w [S,Cin,1,1], squeeze_b [S],
 *                    expand1_w [E,S,1,1], expand1_b [E], expand3_w [E,S,3,3], expand3_b [E]
 *   lin[0..6]        [1,C,1,1], C = 64, 128, 256, 384, 384, 512, 512   (LPIPS v0.1 lin{i}.model.1.weight of squeeze.pth)
 * all fp32, contiguous, in device memory. */
typedef struct DgsFireWeights {
  const float* squeeze_w;
  const float* squeeze_b;
  const float* expand1_w;
  const float* expand1_b;
  const float* expand3_w;
  const float* expand3_b;
} DgsFireWeights;
typedef struct DgsLpipsSqueezeWeights {
  const float* conv_w;
  const float* conv_b;
  DgsFireWeights fire[8];
  const float* lin[7];
} DgsLpipsSqueezeWeights;
/* As dgs_lpips_alex, with the network z-score, then conv 3x3 /2 without padding, ReLU, max-pool, Fire 1, Fire 2, max-pool,
 * Fire 3, Fire 4, max-pool, Fire 5 .. 8; the max-pools are 3x3 /2 in ceil mode; taps: the first ReLU and the outputs of
 * Fires 2, 4, 5, 6, 7, 8 (each before the pool that follows it) -- `features` modules 2, 5, 8, 10, 11, 12, 13 counted from
 * 1.  out [n_pairs,8] = per pair (total, layer 1..7).  The first convolution runs on dgs_conv2d_bias_relu's kernel, every
 * Fire module in one launch of dgs_fire_bias_relu's.  Every contract of dgs_lpips_vgg holds: stream-explicit, caller-owned
 * memory, no host synchronisation, no float atomics, a pair's eight numbers independent of the other pairs and of
 * n_pairs, two runs bitwise equal, lpips(x, x) exactly 0 in all eight and lpips(x, y) == lpips(y, x) bitwise.
 * tmp >= dgs_lpips_squeeze_tmp_bytes(W, H, n_pairs) bytes (0: arguments the call refuses), 256-byte aligned: two ping-pong
 * buffers of the first convolution's output [2 n_pairs,64,(H-3)/2+1,(W-3)/2+1] and the distance partials -- 529,328,896
 * bytes for one 1920 x 1080 pair.  Refused before any HIP call: a NULL pointer (the fifty-seven of `w` included),
 * n_pairs < 1 (or above 65535), W or H below 17 -- the smallest image the network accepts, as the reference raises at
 * 16 -- and 3 H W, 64 h0 w0 or 2 n_pairs h0 w0 of 2^31 and more (h0 = (H-3)/2+1, w0 = (W-3)/2+1). */
size_t dgs_lpips_squeeze_tmp_bytes(int32_t W, int32_t H, int32_t n_pairs);
int dgs_lpips_squeeze(const float* a, const float* b, int32_t n_pairs, int32_t W, int32_t H, const DgsLpipsSqueezeWeights* w,
                      void* tmp, float* out, dgs_stream_t stream);
/* A Fire module on its own, in one launch: out [n_img,E1+E3,IH,IW] = cat(relu(conv1x1(s, expand1)), relu(conv3x3(s,
 * expand3, zero padding 1))) with s = relu(conv1x1(in [n_img,Cin,IH,IW], squeeze)) [n_img,S,IH,IW], on
 * v_mfma_f32_32x32x2_f32.  s is computed per output tile (4 rows x 32 columns, with its 1-pixel halo) and kept in LDS;
 * both expands write straight into their channel ranges of `out`.  Any Cin >= 1, 1 <= S <= 64 (a larger S is refused),
 * E1, E3 >= 1.  squeeze_out non-NULL: s is also stored there (each element once); `out` is bit-identical either way.
 * Every element, fp32 throughout, whatever its place in the call or in a tile:
 *   s:           per chunk of CK input channels (CK = 16 where S <= 32, else 32) one fmaf chain of L1 = CK terms from 0 in
 *                channel order (a term past Cin being 0 x 0), the chunks' results added in channel order with a
 *                compensated (Kahan) fp32 sum, + bias, ReLU (a NaN passes);
 *   1 x 1 part:  ONE fmaf chain of L2a = S terms from 0 in channel order (S + 1 for odd S: a last 0 x 0), + bias, ReLU;
 *   3 x 3 part:  per chunk of 8 squeeze channels one fmaf chain of L2b = 72 terms from 0 in the k order (ky, kx, ci) -- for
 *                each of the nine weights in row-major order the chunk's channels in order, a term past S being 0 x 0 --,
 *                the chunks' results added in channel order with the compensated sum, + bias, ReLU; the zero padding
 *                pads s (a position outside the image is 0, not relu(bias)).
 * Refused before any HIP call: a NULL pointer (squeeze_out excepted; the six of `w` included), an empty size, S above 64,
 * and Cin IH IW, (E1 + E3) IH IW or n_img IH IW of 2^31 and more.  `out` and squeeze_out must not overlap `in`. */
int dgs_fire_bias_relu(const float* in, int32_t n_img, int32_t Cin, int32_t IH, int32_t IW, int32_t S, int32_t E1, int32_t E3,
                       const DgsFireWeights* w, float* squeeze_out, float* out, dgs_stream_t stream);
/* max_pool2d(kernel 3, stride 2, ceil_mode=True) of `planes` planes [IH,IW] -> [IH / 2, IW / 2] (IH, IW >= 2: a window
 * that would start outside the input is dropped, so an even size ends with a window of two rows or columns); the maximum
 * over the part of a window inside the plane, a NaN in that part is its result.  `out` must not overlap `in`. */
int dgs_maxpool3x3s2_ceil(const float* in, uint64_t planes, int32_t IH, int32_t IW, float* out, dgs_stream_t stream);

/* ---- tile-list profile (addition to ABI 15; no counterpart in the reference) ----
 * How long are the tile lists of a forward, how far did the forward walk them, and how uneven is that work: the figures
 * behind any decision about splitting long lists or balancing tiles.  Reads what a forward left in the image blob:
 *   ranges     u32 [K*T,2], the blob's `ranges` (DgsLayout.ranges; offset 0 of a forward_only blob), T = ceil(W/16) ceil(H/16)
 *   n_contrib  u32 [K,H*W], the blob's `n_contrib`, or NULL (a forward_only blob has none): the walked figures are then 0
 * Per (subframe, tile), into per_tile u32 [K*T,2] when it is not NULL:
 *   length = ranges.y - ranges.x
 *   walked = the largest n_contrib among the tile's pixels INSIDE the image: the list position after which the forward had
 *            nothing left to do for the tile (its wave stops there), so the work the tile really cost
 * summary u64 [K+1, DGS_LIST_PROFILE_WORDS]: row k < K is subframe k, row K all subframes together.  Words of a row:
 *   0 tiles          1 nonempty (length > 0)   2 total = sum of length   3 max_length
 *   4 batches = sum of ceil(length / 64), the compositing kernels' unit of work
 *   5 walked_total   6 walked_max              7 walked_batches = sum of ceil(walked / 64)
 *   8..40  hist_length[33]:  bucket 0 counts the tiles with length 0, bucket b >= 1 those with length in [2^(b-1), 2^b)
 *   41..73 hist_walked[33]:  the same of walked
 * One wave64 per tile with the compositing kernels' pixel mapping (four loads per lane, a cross-lane max); a block adds
 * its 32 tiles in LDS with integer atomics and stores one partial row into tmp, a second launch adds the partial rows.
 * Integers only, no global and no float atomics: the result is bitwise reproducible.  Two launches on `stream`, no host
 * synchronisation, no allocation, nothing kept between calls: capturable.  tmp >= dgs_list_profile_tmp_bytes(W, H, K)
 * bytes (0 for sizes the call refuses); ranges, per_tile, summary and tmp 8-byte aligned.  Refused before anything is
 * enqueued: a NULL ranges / summary / tmp, W or H outside 1..65536, K outside 1..DGS_MAX_K, a misaligned pointer. */
#define DGS_LIST_PROFILE_WORDS 74
size_t dgs_list_profile_tmp_bytes(int32_t W, int32_t H, int32_t K);
int dgs_list_profile(const uint32_t* ranges, const uint32_t* n_contrib, int32_t W, int32_t H, int32_t K, uint32_t* per_tile,
                     uint64_t* summary, void* tmp, dgs_stream_t stream);

/* ---- photometric registration (additions to ABI 15; the reference shells out to COLMAP for this step, test.py:188-398) ----
 * Two integer kernels on the 8-bit frames dgs_frames_finish makes; every result is exact and bitwise reproducible.  No
 * atomics, no host synchronisation, no allocation, nothing kept between calls: capturable.
 *
 * dgs_box_reduce_u8: in u8 [G,H,W,3] (any alignment) -> out u32 [G,pitch], h = H / s, w = W / s (floor: trailing rows and
 * columns are dropped), pitch = (h w + 3) & ~3 dwords.  Output pixel (y, x) of image g is dword y w + x of row g:
 * r | g << 8 | b << 16, top byte 0, each channel (sum of its s s bytes + s s / 2) / (s s) in integer arithmetic; the pad
 * dwords of a row are written as 0.  s = 1 packs.  Refused before anything is enqueued: a NULL pointer, G outside 1..65535,
 * s outside 1..64, H / s or W / s below 1, more than 2^30 output pixels per image, an `out` that is not 16-byte aligned. */
int dgs_box_reduce_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t s, uint32_t* out, dgs_stream_t stream);

/* dgs_sad_matrix: a u32 [na,L], b u32 [nb,L] (L dwords per image, a multiple of 4; both 16-byte aligned; all four bytes of
 * a dword count).  group == 0: out u64 [na,nb], out[i][j] = sum over the 4 L bytes of |a_i - b_j|.  group == m > 0 (nb must
 * equal na m): out u64 [na,m], out[i][j] scores a_i against b_{i m + j}.
 * First launch: a block takes DGS_SAD_TILE_A images of `a` (1 when grouped) and a tile of `b` over one chunk of
 * DGS_SAD_CHUNK_DWORDS dwords -- 16-byte loads, the `a` quads in registers, every quad of `b` loaded once per a-tile,
 * v_sad_u8 -- and stores one u32 partial per pair into tmp [chunk][row][column]; second launch: the 64-bit sums.  The
 * number of blocks is a function of (na, nb, group, L) only; tmp's contents before the call do not matter.
 * tmp >= dgs_sad_matrix_tmp_bytes(na, nb, L) bytes (0 for arguments the call refuses), 4-byte aligned; out 8-byte aligned.
 * Refused before anything is enqueued: a NULL pointer, na or nb below 1, L below 4, no multiple of 4 or above 2^40, a negative
 * group or nb != na group, a misaligned pointer, more than 2^31 - 1 blocks. */
#define DGS_SAD_CHUNK_DWORDS 16384
#define DGS_SAD_TILE_A 4
size_t dgs_sad_matrix_tmp_bytes(int32_t na, int32_t nb, uint64_t L);
int dgs_sad_matrix(const uint32_t* a, int32_t na, const uint32_t* b, int32_t nb, int32_t group, uint64_t L, uint64_t* out,
                   void* tmp, dgs_stream_t stream);

/* ---- scene loading (additions to ABI 15; utils/general_utils.py:23-29 PILtoTorch, scene/dataset_readers.py:164-209) ----
 * dgs_resample_ksize / dgs_resample_coeffs: HOST ONLY (no HIP call).  Pillow's precompute_coeffs + normalize_coeffs_8bpc
 * for the antialiased bicubic filter (a = -0.5, support 2) on one axis, in double: scale = in / out, fs = max(scale, 1),
 * support = 2 fs, ksize = (int)ceil(support) * 2 + 1 (what dgs_resample_ksize returns; 0 for sizes the call refuses).  Per
 * output index xx: center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center +
 * support + 0.5), in) - xmin, w[x] = bicubic((x + xmin - center + 0.5) (1 / fs)) for x < xmax, each divided by their
 * sequential sum when that is not 0, kk[xx][x] = (int)(+-0.5 + w[x] 2^22) with the sign of w[x], the rest of the row 0;
 * bounds[xx] = (xmin, xmax).  kk int32 [out, ksize] (kk_capacity: the int32 entries the caller's array holds), bounds int32
 * [out, 2], both caller-owned HOST arrays.  Refused: a NULL pointer, a size outside 1..65536, in / out outside [1/64, 64],
 * kk_capacity below out ksize. */
int32_t dgs_resample_ksize(int32_t in_size, int32_t out_size);
int dgs_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* kk, uint64_t kk_capacity, int32_t* bounds);

/* dgs_resize_u8: Pillow's ImagingResample (Image.resize, BICUBIC) of G 8-bit images in one launch.  in u8 [G,H,W,C],
 * pixel-interleaved as np.asarray(image) gives it, C = 1 or 3, any alignment.  kk_h / bounds_h: the DEVICE copies of
 * dgs_resample_coeffs(W, w), kk_v / bounds_v of (H, h); the pair of an axis whose size does not change is not read (may be
 * NULL) and that pass is skipped.  Horizontal pass first: every sample starts at 2^21, adds pixel * kk in 32-bit integers,
 * >> 22 (arithmetic), clamped to 0..255 and ROUNDED TO A BYTE; then the vertical pass the same way on those bytes.
 * Outputs, either may be NULL but not both: out_u8 u8 [G,h,w,C] (any alignment) and out_f32 float planar [C,h,w] per image,
 * image g at out_f32 + g f32_image_stride floats (>= C h w: a caller writes straight into its slice of a larger stack),
 * value (float)byte / 255.0f -- torch.from_numpy(u8) / 255.0 bit for bit.
 * A block owns an output tile (16 x 64 pixels, shrunk where the input rows it needs do not fit 32 KiB of LDS), resamples
 * those rows horizontally into LDS as bytes and runs the vertical pass out of LDS; no temporary, nothing kept between calls,
 * no atomics: capturable.  Every index derived from the tables is clamped to the buffers.  Refused before anything is
 * enqueued: a NULL input, both outputs NULL, G below 1, C outside {1, 3}, a size outside 1..65536, a ratio outside
 * [1/64, 64] on an axis, a NULL table of an axis that is resampled, a table or out_f32 that is not 4-byte aligned, a float
 * image stride below C h w, more than 2^31 - 1 blocks. */
int dgs_resize_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, const int32_t* kk_h,
                  const int32_t* bounds_h, const int32_t* kk_v, const int32_t* bounds_v, uint8_t* out_u8, float* out_f32,
                  uint64_t f32_image_stride, dgs_stream_t stream);

/* dgs_resize_rgba_u8: Pillow's Image.resize (BICUBIC) of G RGBA images in one launch (additions to ABI 15).  in u8
 * [G,H,W,4], any alignment; the tables and the outputs as dgs_resize_u8's with C = 4: out_u8 u8 [G,h,w,4], out_f32 float
 * planar [4,h,w] per image at f32_image_stride floats (>= 4 h w).  Pillow does not resample four independent channels: it
 * converts to premultiplied alpha (per colour byte t = c a + 128, ((t >> 8) + t) >> 8), resamples the four bytes as
 * dgs_resize_u8 does, and converts back (the colour copied where the resampled alpha is 0 or 255, min(255, 255 c / a)
 * elsewhere).  When neither size changes the call is a copy / conversion WITHOUT that round trip, as Pillow's is (the colour
 * under alpha 0 survives).  The same kernel template as dgs_resize_u8 with a fourth channel (the result tile is 4 KiB of LDS
 * instead of 3).  Refusals as dgs_resize_u8's (no C), each with its own message. */
int dgs_resize_rgba_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t h, int32_t w, const int32_t* kk_h,
                       const int32_t* bounds_h, const int32_t* kk_v, const int32_t* bounds_v, uint8_t* out_u8, float* out_f32,
                       uint64_t f32_image_stride, dgs_stream_t stream);

/* dgs_rgba_over_u8: the composite of the reference's Blender reader (scene/dataset_readers.py:335-341) of G RGBA images
 * over a black (white = 0) or white background in one launch.  in u8 [G,H,W,4], any alignment.  Per colour byte
 *     (uint8)(int)(((c / 255.0) * (a / 255.0) + bg * (1.0 - a / 255.0)) * 255.0)
 * in IEEE double, one rounding per operation, in this order (bg = 0.0 or 1.0, its product kept): numpy's float64 expression
 * and its cast to np.byte, i.e. truncation.  It differs from the exact integer floor in 154 (black) / 152 (white) of the
 * 65 536 (c, a) pairs and from a float32 evaluation in 154 / 391.  Outputs, either may be NULL but not both: out_u8 u8
 * [G,H,W,3] (any alignment) and out_f32 float planar [3,H,W] per image, image g at out_f32 + g f32_image_stride floats
 * (>= 3 H W), value (float)byte / 255.0f.  No temporary, nothing kept between calls, no atomics: capturable.  Refused before
 * anything is enqueued: a NULL input, both outputs NULL, G below 1, a size outside 1..65536, an out_f32 that is not 4-byte
 * aligned, a float image stride below 3 H W, more than 2^31 - 1 blocks. */
int dgs_rgba_over_u8(const uint8_t* in, int32_t G, int32_t H, int32_t W, int32_t white, uint8_t* out_u8, float* out_f32,
                     uint64_t f32_image_stride, dgs_stream_t stream);

/* dgs_depth_bound_keys: the per-(camera, point) part of get_bds in double.  points double [n,3], w2c double [m,3,4] (rows
 * of the world-to-camera matrix [R | t]), both on the device; w, h, fx, fy: the FIRST camera's, used for every camera as the
 * reference does.  With cam = R p + t: u = cam.x / fx, v = cam.y / fy, d = cam.z - cam.x (w / 2) / fx - cam.y (h / 2) / fy,
 * px = u / d, py = v / d (the reference multiplies the row vector by inv(K), not K: restated, not repaired); the pair
 * counts when cam.z > 0.01 && 0 <= px < w && 0 <= py < h.  keys float [m,n]: (float)cam.z of a pair that counts, a quiet NaN
 * otherwise (NaNs sort last in dgs_order_stats); counts u32 [m]: the pairs that count (zeroed by the call's first launch,
 * then one integer atomicAdd per block).  Two launches, capturable.  Refused before anything is enqueued: a NULL pointer,
 * n below 1, m outside 1..65535, a w, h, fx or fy that is not positive and finite, a misaligned pointer. */
int dgs_depth_bound_keys(const double* points, int32_t n, const double* w2c, int32_t m, double w, double h, double fx,
                         double fy, float* keys, uint32_t* counts, dgs_stream_t stream);

/* ---- PNG files made on the device (additions to ABI 15) ----
 * dgs_png_encode: n 8-bit images -> n finished .png files, every byte made on the device: signature, IHDR, ONE IDAT holding
 * a zlib stream, IEND and every CRC.  channels 1 / 2 / 3 / 4 is colour type 0 / 4 / 2 / 6 (gray, gray + alpha, RGB, RGBA), bit
 * depth 8, no interlace, no ancillary chunk.  Image i is h w channels contiguous bytes at images + i image_stride, any
 * alignment; file i starts at files + i file_stride (file_stride >= dgs_png_bound, any alignment) and sizes[i] (a device
 * uint64, 8-byte aligned) is its length; the bytes of the slot past sizes[i] are not written.  The host reads a size, copies
 * that many bytes and writes them.
 *   row filter   per row the candidate (None, Sub, Up, Average, Paeth; bpp = channels; the row above row 0 is zeros) with the
 *                smallest sum of |residual as int8| over the row, the lowest filter type on a tie.  The filtered stream is
 *                F = h (1 + w channels) bytes.
 *   deflate      the filtered stream is cut into segments of DGS_PNG_SEGMENT bytes, each compressed on its own (no reference
 *                to an earlier byte) with zlib's Z_RLE tokens -- a literal, then matches of distance 1 and length 3..258
 *                while the byte repeats, a tail shorter than 3 as literals -- and dynamic Huffman codes (BTYPE 10) built from
 *                the SEGMENT's own histogram: literal/length lengths limited to 15 bits, the code-length code to 7, both
 *                complete; one distance code of length 1.  A segment whose compressed form, marker included, is not smaller
 *                than 5 + len is a stored block.  A non-final compressed segment is followed by an empty stored block, so
 *                the next starts on a byte; the last block carries BFINAL.
 *   checksums    Adler-32 from per-segment (sum, weighted sum) pairs, each chunk's CRC-32 from per-segment remainders
 *                shifted by x^(8 bytes after it) mod the polynomial (the published combine rule).
 * Four launches on the caller's stream, integers only, every sum an integer sum or an OR: the bytes are a function of the
 * arguments.  tmp: dgs_png_tmp_bytes(n, w, h, channels) bytes of the caller's, any alignment; nothing is allocated, no host
 * synchronisation, nothing kept between calls: capturable.  dgs_png_bound = 63 + F + 5 ceil(F / DGS_PNG_SEGMENT): 8 signature
 * + 25 IHDR + 12 IDAT framing + 2 zlib header + 4 Adler + 12 IEND, and the stored-block fallback of every segment; 0 for
 * arguments the call refuses.  n = 0 succeeds without a launch.  Refused before anything is enqueued: channels outside 1..4,
 * w or h below 1, F >= 2^31, a negative n, a NULL pointer, an image_stride below h w channels, a file_stride below the bound,
 * a misaligned sizes, more than 2^31 - 1 blocks. */
#define DGS_PNG_SEGMENT 16384
size_t dgs_png_bound(int32_t w, int32_t h, int32_t channels);
size_t dgs_png_tmp_bytes(int32_t n, int32_t w, int32_t h, int32_t channels);
int dgs_png_encode(const uint8_t* images, int32_t n, int32_t w, int32_t h, int32_t channels, size_t image_stride,
                   uint8_t* files, size_t file_stride, uint64_t* sizes, void* tmp, dgs_stream_t stream);

/* ---- JPEG files made on the device (additions to ABI 15) ----
 * dgs_jpeg_encode: n 8-bit images -> n finished baseline JFIF files (the frames of a Motion-JPEG AVI, deblurgs_amd/video.py,
 * or lone .jpg files).  The calling rules are dgs_png_encode's: image i is h w channels contiguous bytes at images +
 * i image_stride, file i starts at files + i file_stride (file_stride >= dgs_jpeg_bound, any alignment), sizes[i] (a device
 * uint64, 8-byte aligned) is its length and the bytes of the slot past it are not written; tmp is dgs_jpeg_tmp_bytes bytes of
 * the caller's, any alignment; nothing is allocated, no host synchronisation, nothing kept between calls: capturable.  Two
 * launches.  channels 1 is gray (subsampling is ignored, the MCU is one block), 3 is RGB; subsampling DGS_JPEG_444 or
 * DGS_JPEG_420; quality 1..100; w, h 1..65535.
 * The bytes are a function of the pixels, in integers (arithmetic shifts, everything fits int32):
 *   colour     Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *              Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16, Cb and Cr clipped to 0..255; gray: Y = the byte
 *   padding    to a multiple of the MCU (8; 16 at 4:2:0) by repeating the last column, then the last row, at full resolution
 *   4:2:0      Cb, Cr = (a + b + c + d + 2) >> 2 over each 2 x 2
 *   transform  samples - 128; M[u][x] = rint(8192 c(u) / 2 cos((2x + 1) u pi / 16)), c(0) = sqrt(1/2), c(u) = 1 otherwise;
 *              t[y][u] = (sum_x M[u][x] b[y][x] + 512) >> 10, F[v][u] = (sum_y M[v][y] t[y][u] + 4096) >> 13: 8 x the coefficient
 *   quantiser  Annex K.1 / K.2 base tables, s = 5000 / quality below 50, else 200 - 2 quality, q = clip((base s + 50) / 100,
 *              1, 255), level = sign(F) ((|F| + 4 q) / (8 q))  (integer divisions)
 *   entropy    baseline sequential, the Annex K.3 - K.6 Huffman tables, zig-zag order, ZRL for runs above 15, EOB unless
 *              coefficient 63 is non-zero; the restart interval is one MCU row: its bits start on a byte with DC predictors 0
 *              and are padded with 1-bits, every 0xFF is followed by 0x00, row r (all but the last) by RST(r & 7)
 *   file       SOI, APP0 "JFIF" 1.01 (no units, density 1:1), one DQT (both tables, zig-zag order; one for gray), SOF0
 *              (component ids 1, 2, 3, luma sampling 0x22 or 0x11, table selectors 0, 1, 1), four DHT (luma DC, luma AC, chroma
 *              DC, chroma AC; two for gray), DRI = MCUs per row, SOS, the scan, EOI
 * dgs_jpeg_bound = 625 (334 gray) + 416 blocks + 2 MCU rows + 2: the header; per 8 x 8 block the longest code sequence
 * (22 + 63 * 26 = 1660 bits, 208 bytes) doubled for stuffing; an RST marker per MCU row; EOI.  0 for arguments the call
 * refuses.  n = 0 succeeds without a launch.  Refused before anything is enqueued: channels other than 1 and 3, w or h
 * outside 1..65535, another subsampling, a quality outside 1..100, a negative n, a NULL pointer, an image_stride below
 * h w channels, a file_stride below the bound, a misaligned sizes, more than 2^31 - 1 blocks. */
#define DGS_JPEG_444 0
#define DGS_JPEG_420 1
size_t dgs_jpeg_bound(int32_t w, int32_t h, int32_t channels, int32_t subsampling);
size_t dgs_jpeg_tmp_bytes(int32_t n, int32_t w, int32_t h, int32_t channels, int32_t subsampling);
int dgs_jpeg_encode(const uint8_t* images, int32_t n, int32_t w, int32_t h, int32_t channels, size_t image_stride,
                    int32_t quality, int32_t subsampling, uint8_t* files, size_t file_stride, uint64_t* sizes, void* tmp,
                    dgs_stream_t stream);

/* ---- JPEG files decoded on the device (additions to ABI 15) ----
 * The pixels are libjpeg's (Pillow's `np.asarray(Image.open(f))`), bit for bit, for the files below; all arithmetic is
 * integer, all shifts arithmetic, everything fits int32.  tests/jpeg_decode_cases.py restates the rules in numpy.
 *   1 entropy    T.81 Annex F baseline: canonical Huffman codes from the DHT counts (Annex C), EXTEND (F.12), ZRL (0xF0) and
 *                EOB, coefficients de-zigzagged to natural order, one DC predictor per component, reset to 0 at every RSTm;
 *                FF 00 is a stuffed FF; an RSTm marker ends an interval at a byte boundary
 *   2 transform  libjpeg's jidctint ("islow"): coefficient times 8-bit table entry; with DESCALE(x, n) = (x + (1 << (n-1))) >> n
 *                the 1-D routine below runs over the 8 columns with n = 11, then over the 8 rows of that result with n = 18;
 *                then + 128, clamped to 0..255.  The routine, on i0..i7:
 *                  z1 = (i2 + i6) 4433, t2 = z1 - i6 15137, t3 = z1 + i2 6270, t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13,
 *                  t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
 *                  a = i7, b = i5, c = i3, d = i1, z1 = a + d, z2 = b + c, z3 = a + c, z4 = b + d, z5 = (z3 + z4) 9633,
 *                  a *= 2446, b *= 16819, c *= 25172, d *= 12299, z1 *= -7373, z2 *= -20995, z3 = z3 (-16069) + z5,
 *                  z4 = z4 (-3196) + z5, a += z1 + z3, b += z2 + z4, c += z2 + z3, d += z1 + z4;
 *                  out0..7 = DESCALE of t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d
 *   3 upsampling libjpeg's "fancy" upsampling.  A component's plane is dh x dw, dh = ceil(h V / Vmax), dw = ceil(w H / Hmax);
 *                the padding of the transform beyond it is never read.  dw <= 2: every sample replicated, 2 x horizontally
 *                (and 2 x vertically at 2 x 2).  Otherwise at 2 x 1 (4:2:2): out[2x] = (3 P[x] + P[x-1] + 1) >> 2,
 *                out[2x+1] = (3 P[x] + P[x+1] + 2) >> 2, at the ends out[0] = P[0], out[2dw-1] = P[dw-1]; at 2 x 2 (4:2:0):
 *                output row 2r takes the neighbour row max(r-1, 0), row 2r+1 the row min(r+1, dh-1), S[x] = 3 P[r][x] +
 *                P[nbr][x], out[2x] = (3 S[x] + S[x-1] + 8) >> 4, out[2x+1] = (3 S[x] + S[x+1] + 7) >> 4, at the ends
 *                out[0] = (4 S[0] + 8) >> 4, out[2dw-1] = (4 S[dw-1] + 7) >> 4.  Cropped to h x w.
 *   4 colour     cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768)
 *                >> 16), B = Y + ((116130 cb + 32768) >> 16), each clamped to 0..255.  One component: the channel is Y.
 * Files taken: SOF0, 8 bits, ONE interleaved scan, 8-bit quantisation tables, 1 component or 3 with luma sampling 1 x 1,
 * 2 x 1 or 2 x 2 and chroma 1 x 1, with or without DRI, any valid DHT tables; APPn and COM are skipped.  Refused as
 * DGS_E_JPEG_UNSUPPORTED, the reason in dgs_last_error(): SOF1, SOF2 and above, several scans, a 16-bit DQT, 4 components,
 * other sampling factors, Adobe APP14 with transform 0, component ids 'R' 'G' 'B' (such files are not malformed: a caller
 * hands them to a host reader).  DGS_E_JPEG_CORRUPT: a stream that breaks the format -- a segment length past the end, DHT
 * counts that sum past 256 or make no prefix code, table ids out of range, references to tables that are not defined, a zero
 * dimension, restart markers out of order or a count of them that disagrees with DRI and the MCU count, a missing EOI, a
 * scan too short to hold a picture of the size the header claims.
 *
 * dgs_jpeg_decode_plan (HOST ONLY: no HIP call, nothing on the device is touched) parses one file of `size` bytes into
 * `plan`, plan_bytes bytes of the caller's, 8-byte aligned: a DgsJpegPlan followed by uint32 interval_at[n_intervals + 1].
 * Interval i is the bytes [interval_at[i], interval_at[i+1] - 2) of the file (the two bytes before the next interval are
 * its RSTm marker, those after the last interval the marker that ends the scan); the parser walks the scan once for EOI
 * and takes the offsets from that walk.  dgs_jpeg_decode_plan_bytes reads the headers only and gives the size to pass
 * (DGS_E_CAPACITY for a smaller one); both return the same code for the same file.
 *
 * dgs_jpeg_decode (enqueue only: no allocation, no synchronisation, nothing kept between calls, capturable): n files and
 * their plans, both inside ONE device buffer `blob` of blob_bytes bytes, 16-byte aligned: index (device uint64 [n,2],
 * 8-byte aligned, anywhere) holds for image i the offset in blob of its file (a multiple of 4) and of its plan (a multiple
 * of 8).  All n images are w x h x channels; tables, sampling and DRI are each plan's own.  Image i is written as h w
 * channels contiguous bytes (interleaved RGB, or gray) at images + i image_stride; images is 4-byte aligned and
 * image_stride a multiple of 4 (packed stores).  status (device int32 [n]) is 0 or a DGS_JPEG_S_* code; an image with a
 * non-zero status is written as zeros.  max_intervals: the largest n_intervals of the n plans (the entropy grid).  tmp:
 * dgs_jpeg_decode_tmp_bytes bytes, any alignment: int16 coefficients and 8-bit component planes of channels * (2 ceil(w /
 * 16)) * (2 ceil(h / 16)) blocks per image.  Five enqueues: the clears of status and of the coefficients, then
 *   entropy   one LANE per restart interval (a file without DRI is one interval: its scan is decoded by one lane), a wave
 *             of 64 per block, the image's six Huffman tables (8-bit lookahead, maxcode / offset for longer codes) in LDS;
 *             only non-zero coefficients are stored.  A lane stops with DGS_JPEG_S_BAD_CODE, _INDEX (a coefficient index
 *             past 63), _DC_CATEGORY (past 11) or _OUT_OF_BYTES; it reads no byte outside its interval and writes no
 *             coefficient outside the blocks of its MCUs, whatever the scan holds.
 *   transform 8 lanes per block: rule 2, columns then rows, the exchange through LDS; 8-bit planes.
 *   pixels    4 pixels per lane: rules 3 and 4, dword stores.
 * The kernels check the plan against the call (DGS_JPEG_S_PLAN: another size or channel count, geometry or interval count
 * that disagree, offsets outside blob): a plan that is not the parser's costs its image a status, never a stray access.
 * Refused before anything is enqueued (DGS_E_ARG): channels other than 1 and 3, w or h outside 1..65535, a negative n, a
 * NULL pointer, misaligned blob / index / images / status, an image_stride below h w channels or no multiple of 4,
 * max_intervals below 1, more than 2^31 - 1 blocks in all.  n = 0 succeeds without a launch. */
#define DGS_E_JPEG_UNSUPPORTED (-4) /* a valid file of a kind the device decoder does not take (text in dgs_last_error) */
#define DGS_E_JPEG_CORRUPT (-5)     /* a stream that breaks the format */
#define DGS_JPEG_S_OK 0
#define DGS_JPEG_S_PLAN 1
#define DGS_JPEG_S_BAD_CODE 2
#define DGS_JPEG_S_INDEX 3
#define DGS_JPEG_S_DC_CATEGORY 4
#define DGS_JPEG_S_OUT_OF_BYTES 5
#define DGS_JPEG_PLAN_MAGIC 0x4E4C504Au /* "JPLN" */
#define DGS_JPEG_LOOK 8                 /* bits of the Huffman lookahead */
typedef struct DgsJpegHuff {
  uint16_t look[1 << DGS_JPEG_LOOK]; /* by the next 8 bits: code length << 8 | symbol; 0: the code is longer than 8 bits */
  int32_t maxcode[18];               /* [l]: the largest code of length l, -1 where there is none (l = 1..16) */
  int32_t valoff[18];                /* [l]: index into vals of the first code of length l, minus that code */
  uint8_t vals[256];                 /* the symbols in code order */
} DgsJpegHuff;
typedef struct DgsJpegPlan {
  uint32_t magic;
  uint32_t plan_bytes; /* of this struct and the interval table after it, rounded up to 8 */
  uint32_t file_bytes;
  int32_t w, h, channels;
  int32_t hs, vs;            /* the luma sampling factors: 1 x 1, 2 x 1 or 2 x 2 (chroma is 1 x 1) */
  int32_t mcus_x, mcus_y;    /* ceil(w / 8 hs), ceil(h / 8 vs) */
  int32_t restart_interval;  /* DRI: MCUs per interval, 0 = none */
  int32_t n_intervals;       /* ceil(mcus_x mcus_y / restart_interval), 1 without DRI */
  uint32_t scan_begin;       /* the first byte after SOS */
  uint32_t scan_end;         /* the 0xFF of the marker that ends the scan */
  uint32_t reserved[2];
  uint8_t quant[3][64];      /* per component, natural order */
  DgsJpegHuff huff[6];       /* DC of components 0..2, AC of components 0..2 */
} DgsJpegPlan;
int dgs_jpeg_decode_plan_bytes(const uint8_t* data, size_t size, size_t* plan_bytes);
int dgs_jpeg_decode_plan(const uint8_t* data, size_t size, void* plan, size_t plan_bytes);
size_t dgs_jpeg_decode_tmp_bytes(int32_t n, int32_t w, int32_t h, int32_t channels);
int dgs_jpeg_decode(const uint8_t* blob, size_t blob_bytes, const uint64_t* index, int32_t n, int32_t w, int32_t h,
                    int32_t channels, int32_t max_intervals, uint8_t* images, size_t image_stride, int32_t* status,
                    void* tmp, dgs_stream_t stream);

/* ---- the training-progress visualiser's drawings (additions to ABI 15) ----
 * dgs_draw_prims: n records int32 [n,6] = (x0, y0, x1, y1, r, rgb), rgb = R | G << 8 | B << 16, painted into img, uint8
 * [H,W,3] on the device, in painter's order: a covered pixel takes the colour of the HIGHEST-index record that covers it,
 * every other byte of img is left as it was.
 *   r == 0   a one-pixel line from (x0, y0) to (x1, y1).  dx = |x1 - x0|, dy = |y1 - y0|; the major axis is y if dy > dx,
 *            else x; maj, min = the larger, the smaller of dx, dy.  Step i = 0 .. maj moves i pixels along the major axis
 *            from the start point and floor((2 min i + maj - 1) / (2 maj)) along the minor one (0 for a single point): the
 *            integer Bresenham walk with error term maj - 2 min, a tie staying with the start point -- so a line is not
 *            the same set of pixels as its reverse.  The UNCLIPPED line is walked; pixels outside the image are dropped.
 *   r > 0    the filled disc (x - x0)^2 + (y - y0)^2 <= r^2.  Needs x1 == x0, y1 == y0 and r <= 64: else skipped.
 *   r < 0    skipped.  A record with a |coordinate| above 2^29 is skipped too (the 64-bit products above stay exact).
 * owner: uint32 [H,W] scratch of the caller's; the call clears it itself (it may be passed dirty).  Three enqueues on the
 * caller's stream: the clear; one wave per record raising owner[pixel] to index + 1 with an integer atomicMax, the step
 * range clipped to the image before the loop (no lane loops more than max(W, H) / 64 + 1 times, wherever the endpoints lie);
 * a pass that writes the owner's colour.  The maximum does not depend on arrival order: the bytes are a function of the
 * arguments.  Nothing allocated, no host synchronisation, nothing kept between calls.  Refused before anything is enqueued:
 * a NULL pointer, W or H below 1, W H >= 2^31, a negative n, a misaligned prims or owner.  n = 0 succeeds and touches
 * nothing. */
int dgs_draw_prims(uint8_t* img, int32_t W, int32_t H, const int32_t* prims, int32_t n, uint32_t* owner,
                   dgs_stream_t stream);

/* dgs_cone_segments: draw_cone_on_render_img (utils/visualization.py:156-185) for C cameras, one thread each, in double
 * with the float inputs promoted.  view float [C,16] (row-major 4 x 4 world-view matrices: the upper 3 x 3 is the
 * camera-to-world rotation), campos float [C,3], render_view / render_proj float [16] (the world-view and full projection
 * matrices of the camera the image was rendered from), rgb int32 [C], prims_out int32 [C * 8, 6]: all on the device.  The
 * five vertices (0,0,0), (tanx, tany, 1), (tanx, -tany, 1), (-tanx, -tany, 1), (-tanx, tany, 1) times scale, w = 1, go to
 * the world by c2w^T and to ndc by render_proj (row vectors); pix = ((ndc.xy + 1) (W, H) - 1) / 2 truncated toward zero.
 * Camera c writes the records 8 c .. 8 c + 7 = the segments (0,1) (0,2) (0,3) (0,4) (1,2) (2,3) (3,4) (4,1) with r = 0 and
 * rgb[c].  All eight get r = -1 when z / w < 0.1 for any vertex of the camera-LOCAL cone taken through render_view (the
 * reference's test as written); a segment with an endpoint that is not finite or beyond 2^29 gets r = -1 (the reference
 * swallows cv2.line's exception).  One launch.  Refused before it: a NULL pointer, W or H below 1, C negative or above
 * 2^24, a misaligned pointer.  C = 0 succeeds without a launch. */
int dgs_cone_segments(int32_t C, const float* view, const float* campos, double tanx, double tany, double scale,
                      const float* render_view, const float* render_proj, int32_t W, int32_t H, const int32_t* rgb,
                      int32_t* prims_out, dgs_stream_t stream);

/* The cloud's activations as the raw_params kernels evaluate them -- clamp(opacity, 0, 1), exp(scaling) + scale_lb,
 * rotation / max(|rotation|, 1e-12): the reference's get_opacity / get_scaling / get_rotation getters
 * (scene/gaussian_model.py:114-137, scene/gaussian_activation.py:29-52) on device, bit-identical to what
 * dgs_forward_geometry uses with DgsProblem.raw_params = 1.  Any output pointer may be NULL (with its input). */
int dgs_cloud_activations(int32_t P, const float* scaling, const float* rotation, const float* opacity, float scale_lb,
                          float* out_scaling, float* out_rotation, float* out_opacity, dgs_stream_t stream);

/* Stage timing with HIP events recorded on the caller's stream (bench.py's roofline leg); the timers belong to the context
 * the timed calls are handed (DgsProblem.context). */
#define DGS_STAGE_PREPROCESS 0
#define DGS_STAGE_SCAN 1
#define DGS_STAGE_DUPLICATE 2
#define DGS_STAGE_SORT 3
#define DGS_STAGE_RANGES 4
#define DGS_STAGE_COMPOSITE_FWD 5
#define DGS_STAGE_COMPOSITE_BWD 6
#define DGS_STAGE_GEOMETRY_BWD 7
#define DGS_STAGE_DEPTH_ORDER 8 /* sort of the (k, Gaussian) pairs by depth that precedes the duplication */
#define DGS_STAGE_TILE_CULL 9   /* tile_cull: per-slot ellipse test + count, and the scan of the counts */
#define DGS_STAGE_CONTRIB_REDUCE 10 /* backward: per-(subframe, Gaussian) totals of the contribution rows (the second
                                     * stage of the atomics-free reduction; no counterpart in the reference) */
#define DGS_STAGE_COUNT 11
int dgs_profile_enable(DgsContext* ctx, int32_t on);
int dgs_profile_reset(DgsContext* ctx);
/* Synchronises on the recorded events; ms[i] = summed duration of stage i, calls[i] = launches timed. */
int dgs_profile_read(DgsContext* ctx, float* ms, int32_t* calls, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* DGS_HIP_H_INCLUDED */

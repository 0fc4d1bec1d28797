// C entry points over the reference rasteriser's three host calls (CudaRasterizer::Rasterizer::forward, ::backward,
// ::markVisible), so that its own kernels can run on the device next to the CPU oracle and the product's kernels.
//
// TEST INFRASTRUCTURE ONLY.  This file is the project's own text; the reference's rasterizer.h / rasterizer_impl.h are
// included at compile time only (oracle/ref_rasterizer.py compiles them from the reference tree into oracle/_ref/).
//
// Every pointer argument is a DEVICE pointer.  The three buffers the reference asks for through std::function<char*(size_t)>
// are grow-only hipMalloc blocks owned by a handle; after a forward the handle keeps the Geometry / Binning / Image state
// recovered with fromChunk, and dgs_ref_state() hands their pointers and counts out.  Calls return 0 (or num_rendered)
// on success and a negative number on failure; dgs_ref_last_error() has the text.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "rasterizer.h"
#include "rasterizer_impl.h"

namespace {

struct Block {
    char* ptr = nullptr;
    size_t cap = 0;
};

struct Handle {
    Block geom, binning, image;
    int P = 0, N = 0, R = -1, W = 0, H = 0;
    CudaRasterizer::GeometryState g{};
    CudaRasterizer::BinningState b{};
    CudaRasterizer::ImageState i{};
};

thread_local std::string g_err;

bool ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

// grow-only, zero-filled on every request (the reference's torch buffers are uninitialised; zeros make the words no kernel
// writes -- cov3D of a Gaussian culled at the near plane -- reproducible)
char* request(Block& blk, size_t n) {
    if (n > blk.cap) {
        if (blk.ptr) (void)hipFree(blk.ptr);
        blk.ptr = nullptr;
        blk.cap = 0;
        size_t cap = n + n / 4 + 256;
        if (hipMalloc(reinterpret_cast<void**>(&blk.ptr), cap) != hipSuccess) throw std::runtime_error("hipMalloc failed");
        blk.cap = cap;
    }
    if (hipMemset(blk.ptr, 0, blk.cap) != hipSuccess) throw std::runtime_error("hipMemset failed");
    return blk.ptr;
}

bool zero(float* p, size_t count) {
    if (p == nullptr || count == 0) return true;
    return ok(hipMemset(p, 0, count * sizeof(float)), "hipMemset(gradient)");
}

}  // namespace

extern "C" {

// field order is part of the ABI: oracle/ref_rasterizer.py mirrors it
struct DgsRefState {
    int32_t P, N, R, tiles;
    // geometry state [P]
    const float* depths;
    const float* pre_sigmoid;      // [P,3]
    const int32_t* internal_radii;
    const float* means2D;          // [P,2]
    const float* cov3D;            // [P,6]
    const float* conic_opacity;    // [P,4]
    const float* rgb;              // [P,3]
    const uint32_t* point_offsets;
    const uint32_t* tiles_touched;
    // binning state [R]
    const uint64_t* point_list_keys;
    const uint32_t* point_list;
    // image state
    const uint32_t* ranges;        // [tiles,2]
    const uint32_t* n_contrib;     // [N]
    const float* accum_alpha;      // [N]
};

const char* dgs_ref_last_error() { return g_err.c_str(); }

int dgs_ref_struct_size() { return static_cast<int>(sizeof(DgsRefState)); }

void* dgs_ref_create() { return new Handle(); }

void dgs_ref_destroy(void* hv) {
    Handle* h = static_cast<Handle*>(hv);
    if (!h) return;
    for (Block* blk : {&h->geom, &h->binning, &h->image})
        if (blk->ptr) (void)hipFree(blk->ptr);
    delete h;
}

int dgs_ref_forward(void* hv, int P, int D, int M, const float* background, int W, int H, const float* means3D,
                    const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                    float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                    const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, float z_near, float z_far,
                    float* out_color, float* out_depth, int* radii, int use_sigmoid) {
    Handle* h = static_cast<Handle*>(hv);
    if (!h || P <= 0 || W <= 0 || H <= 0 || !radii || !out_color || !out_depth) {
        g_err = "dgs_ref_forward: bad arguments (P == 0 is the caller's guard, as in the reference's binding)";
        return -1;
    }
    h->R = -1;
    int R = -1;
    try {
        R = CudaRasterizer::Rasterizer::forward(
            [h](size_t n) { return request(h->geom, n); }, [h](size_t n) { return request(h->binning, n); },
            [h](size_t n) { return request(h->image, n); }, P, D, M, background, W, H, means3D, shs, colors_precomp, opacities,
            scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, z_near,
            z_far, /*prefiltered=*/false, out_color, out_depth, radii, use_sigmoid != 0, /*debug=*/false);
    } catch (const std::exception& e) {
        g_err = std::string("forward: ") + e.what();
        return -2;
    }
    if (!ok(hipDeviceSynchronize(), "forward: synchronize") || !ok(hipGetLastError(), "forward: launch")) return -3;
    if (R < 0) {
        g_err = "forward: negative num_rendered";
        return -4;
    }
    h->P = P;
    h->N = W * H;
    h->W = W;
    h->H = H;
    h->R = R;
    char* c = h->geom.ptr;
    h->g = CudaRasterizer::GeometryState::fromChunk(c, P);
    c = h->binning.ptr;
    h->b = CudaRasterizer::BinningState::fromChunk(c, R);
    c = h->image.ptr;
    h->i = CudaRasterizer::ImageState::fromChunk(c, h->N);
    return R;
}

int dgs_ref_state(void* hv, DgsRefState* s) {
    Handle* h = static_cast<Handle*>(hv);
    if (!h || !s || h->R < 0) {
        g_err = "dgs_ref_state: no forward has completed on this handle";
        return -1;
    }
    s->P = h->P;
    s->N = h->N;
    s->R = h->R;
    s->tiles = ((h->W + 15) / 16) * ((h->H + 15) / 16);
    s->depths = h->g.depths;
    s->pre_sigmoid = h->g.pre_sigmoid;
    s->internal_radii = h->g.internal_radii;
    s->means2D = reinterpret_cast<const float*>(h->g.means2D);
    s->cov3D = h->g.cov3D;
    s->conic_opacity = reinterpret_cast<const float*>(h->g.conic_opacity);
    s->rgb = h->g.rgb;
    s->point_offsets = h->g.point_offsets;
    s->tiles_touched = h->g.tiles_touched;
    s->point_list_keys = h->b.point_list_keys;
    s->point_list = h->b.point_list;
    s->ranges = reinterpret_cast<const uint32_t*>(h->i.ranges);
    s->n_contrib = h->i.n_contrib;
    s->accum_alpha = h->i.accum_alpha;
    return 0;
}

// Backward of the forward this handle ran last.  Every gradient buffer is zero-filled here first: the reference accumulates
// into them with atomics.  Sizes: dL_dmean2D [P,3], dL_dconic [P,4], dL_dopacity [P], dL_dcolor [P,3], dL_dmean3D [P,3],
// dL_dcov3D [P,6], dL_dsh [P,M,3], dL_dscale [P,3], dL_drot [P,4], dL_ddepths [P], dL_dviewmatrix [16], dL_dprojmatrix [16].
int dgs_ref_backward(void* hv, int P, int D, int M, const float* background, int W, int H, const float* means3D,
                     const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                     const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                     const float* campos, float tan_fovx, float tan_fovy, float z_near, float z_far, const int* radii,
                     const float* dL_dpix, const float* dL_dpixdepth, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                     float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                     float* dL_ddepths, float* dL_dviewmatrix, float* dL_dprojmatrix, int use_sigmoid) {
    Handle* h = static_cast<Handle*>(hv);
    if (!h || h->R < 0 || P != h->P || W != h->W || H != h->H || !radii || !dL_dpix || !dL_dpixdepth || !dL_dmean2D ||
        !dL_dconic || !dL_dopacity || !dL_dcolor || !dL_dmean3D || !dL_dcov3D || !dL_dscale || !dL_drot || !dL_ddepths ||
        !dL_dviewmatrix || !dL_dprojmatrix || (M > 0 && !dL_dsh)) {
        g_err = "dgs_ref_backward: bad arguments, or no matching forward on this handle";
        return -1;
    }
    const size_t p = static_cast<size_t>(P);
    if (!(zero(dL_dmean2D, p * 3) && zero(dL_dconic, p * 4) && zero(dL_dopacity, p) && zero(dL_dcolor, p * 3) &&
          zero(dL_dmean3D, p * 3) && zero(dL_dcov3D, p * 6) && zero(dL_dsh, p * M * 3) && zero(dL_dscale, p * 3) &&
          zero(dL_drot, p * 4) && zero(dL_ddepths, p) && zero(dL_dviewmatrix, 16) && zero(dL_dprojmatrix, 16)))
        return -2;
    try {
        CudaRasterizer::Rasterizer::backward(P, D, M, h->R, background, W, H, means3D, shs, colors_precomp, scales,
                                             scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                                             tan_fovy, z_near, z_far, radii, h->geom.ptr, h->binning.ptr, h->image.ptr, dL_dpix,
                                             dL_dpixdepth, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D,
                                             dL_dsh, dL_dscale, dL_drot, dL_ddepths, dL_dviewmatrix, dL_dprojmatrix,
                                             use_sigmoid != 0, /*debug=*/false);
    } catch (const std::exception& e) {
        g_err = std::string("backward: ") + e.what();
        return -3;
    }
    if (!ok(hipDeviceSynchronize(), "backward: synchronize") || !ok(hipGetLastError(), "backward: launch")) return -4;
    return 0;
}

// device -> host copy of a state array (the front-end has raw device pointers, not tensors)
int dgs_ref_copy_out(void* dst_host, const void* src_device, size_t nbytes) {
    if (nbytes == 0) return 0;
    if (!dst_host || !src_device) {
        g_err = "dgs_ref_copy_out: null pointer";
        return -1;
    }
    return ok(hipMemcpy(dst_host, src_device, nbytes, hipMemcpyDeviceToHost), "copy_out") ? 0 : -2;
}

int dgs_ref_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, bool* present) {
    if (P <= 0 || !means3D || !viewmatrix || !projmatrix || !present) {
        g_err = "dgs_ref_mark_visible: bad arguments (P == 0 is the caller's guard)";
        return -1;
    }
    CudaRasterizer::Rasterizer::markVisible(P, const_cast<float*>(means3D), const_cast<float*>(viewmatrix),
                                            const_cast<float*>(projmatrix), present);
    if (!ok(hipDeviceSynchronize(), "mark_visible: synchronize") || !ok(hipGetLastError(), "mark_visible: launch")) return -2;
    return 0;
}

}  // extern "C"

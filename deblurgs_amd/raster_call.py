"""The rasteriser's C ABI (include/dgs_hip.h) as its Python callers speak it -- the operator
(diff_gaussian_rasterization), the training step without autograd (fused_step.FusedStep) and the test-view pose fits
(evaluation): filling DgsProblem (cloud_problem: from a GaussianCloud's raw parameters), DgsForwardOut and DgsBackwardIO,
the two forward protocols, the meaning of the pinned count words and of the skip word, the rounding of a learnt capacity,
and the layout of the flat gradient bucket.  Formats only: what to run when is the callers' business.
"""
import ctypes
import math
from typing import NamedTuple

import torch

from . import _lib


def _ptr(t, offset_elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_elems)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _set_blobs(p, geom=None, image=None, binning=None):
    for name, blob in (("geom", geom), ("image", image), ("binning", binning)):
        if blob is not None:
            setattr(p, name + "_state", _ptr(blob))
            setattr(p, name + "_bytes", blob.numel())


def problem(K, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
            settings, bg, tile_cull, wide_records, raw=None, forward_only=False, geom=None, image=None, binning=None):
    """A DgsProblem on the package's context of means3D's device.  settings: the fields of GaussianRasterizationSettings
    (image size, fields of view, scale_modifier, z range, use_sigmoid, sh_degree, prefiltered, debug); bg: its
    background as a contiguous fp32 device tensor that the caller keeps alive.
    raw = {"scale_lb": float, "sh_rest": [P,M-1,3] or None, optional "isotropic": bool}: the inputs are the cloud's raw
    parameters (DgsProblem.raw_params) and shs is the dc part [P,1,3]."""
    p = _lib.DgsProblem()
    p.context = _lib.context(means3D.device.index)   # the package's per-device context (side stream, stage timers)
    p.tile_cull, p.wide_records, p.forward_only = int(bool(tile_cull)), int(bool(wide_records)), int(bool(forward_only))
    rest = None if raw is None else raw["sh_rest"]
    if raw is None:
        p.M = 0 if shs is None else shs.shape[1]
    else:
        p.raw_params = 3 if raw.get("isotropic") else 1
        p.scale_lb = float(raw["scale_lb"])
        p.M = 1 + (0 if rest is None else rest.shape[1])
    p.P, p.D, p.K = means3D.shape[0], int(settings.sh_degree), K
    p.W, p.H = int(settings.image_width), int(settings.image_height)
    p.tanfovx, p.tanfovy = float(settings.tanfovx), float(settings.tanfovy)
    p.scale_modifier, p.z_near, p.z_far = float(settings.scale_modifier), float(settings.z_near), float(settings.z_far)
    p.use_sigmoid, p.prefiltered, p.debug = (int(bool(settings.use_sigmoid)), int(bool(settings.prefiltered)),
                                             int(bool(settings.debug)))
    p.means3D, p.shs, p.shs_rest, p.colors_precomp = _ptr(means3D), _ptr(shs), _ptr(rest), _ptr(colors_precomp)
    p.opacities, p.scales, p.rotations, p.cov3D_precomp = _ptr(opacities), _ptr(scales), _ptr(rotations), _ptr(cov3D_precomp)
    p.viewmatrix, p.projmatrix, p.campos, p.bg = _ptr(viewmatrix), _ptr(projmatrix), _ptr(campos), _ptr(bg)
    _set_blobs(p, geom, image, binning)
    return p


def cloud_problem(cloud, K, viewmatrix, projmatrix, campos, H, W, FoVx, FoVy, bg, tile_cull, geom, image, binning=None):
    """The DgsProblem of a K-camera call on a GaussianCloud's RAW parameters (the kernels apply the activations): compact
    duplicate records, scale_modifier 1, nothing prefiltered, no debug; the rest coefficients only if the cloud has any."""
    from .diff_gaussian_rasterization import GaussianRasterizationSettings      # (that module imports this one)
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(FoVx * 0.5), tanfovy=math.tan(FoVy * 0.5), bg=bg,
        scale_modifier=1.0, z_near=cloud.z_near, z_far=cloud.z_far, use_sigmoid=cloud.use_sigmoid,
        sh_degree=cloud.active_sh_degree, campos=campos, prefiltered=False, debug=False)
    rest = cloud._features_rest if cloud._features_rest.shape[1] > 0 else None
    raw = {"scale_lb": cloud.scale_lower_bound, "sh_rest": rest, "isotropic": getattr(cloud, "use_isotrophic", False)}
    return problem(K, cloud._xyz, cloud._features_dc, None, cloud._opacity, cloud._scaling, cloud._rotation, None,
                   viewmatrix, projmatrix, campos, settings, bg, tile_cull, 0, raw=raw, geom=geom, image=image,
                   binning=binning)


def forward_out(color, depth, radii, host, **pointers):
    """A DgsForwardOut: the images, the radii and the pinned count words (host).  `pointers` sets further fields by name
    from a tensor or a raw address: debug_contrib_checksum, or a captured step's drop_counter / status_dev /
    status_host_indirect."""
    out = _lib.DgsForwardOut()
    out.out_color, out.out_depth, out.radii, out.num_rendered_host = _ptr(color), _ptr(depth), _ptr(radii), _ptr(host)
    for name, v in pointers.items():
        setattr(out, name, v if isinstance(v, int) else _ptr(v))
    return out


class Counts(NamedTuple):
    """The pinned count words a forward leaves in DgsForwardOut.num_rendered_host."""
    counted: int      # [0] the (tile, Gaussian) duplicates counted
    overflow: bool    # [2] capacity mode: the count exceeded the capacity, the lists were not built
    built: int        # [3] the count the lists were built with


def counts(host):
    """Decodes the count words ([1], the high half of the count, must be zero)."""
    counted, hi, overflow, built = (int(x) & 0xFFFFFFFF for x in host[:4].tolist())
    if hi != 0:
        raise RuntimeError("num_rendered exceeds 32 bits: too many (tile, Gaussian) duplicates for one fused call; "
                           "render fewer subframes per call")
    return Counts(counted, bool(overflow), built)


def forward(device, prob, out, host, capacity=None):
    """The forward, with the geometry and image blobs already in `prob`; `host` holds out's count words.
    capacity None: the exact two-phase protocol -- dgs_forward_geometry, one blocking read of the count, the binning blob
    sized to it, dgs_forward_render.  capacity given: the binning blob is sized for that many duplicates up front and one
    dgs_forward runs with no host read; the count words arrive once the stream gets there (a count above the capacity
    sets the overflow word and the skip word instead of writing out of bounds).
    Returns (R the binning blob is laid out for, the binning blob)."""
    L = _lib.lib()
    stream = _stream(device)
    if capacity is None:
        _lib.check(L.dgs_forward_geometry(ctypes.byref(prob), ctypes.byref(out), stream), "dgs_forward_geometry")
        torch.cuda.current_stream(device).synchronize()   # the one host read of num_rendered (rasterizer_impl.cu:287)
        R = counts(host).counted
    else:
        R = int(capacity)
    binning = torch.empty(L.dgs_binning_state_bytes(R, prob.W, prob.H, prob.K), dtype=torch.uint8, device=device)
    _set_blobs(prob, binning=binning)
    if capacity is None:
        _lib.check(L.dgs_forward_render(ctypes.byref(prob), ctypes.byref(out), R, stream), "dgs_forward_render")
    else:
        _lib.check(L.dgs_forward(ctypes.byref(prob), ctypes.byref(out), R, stream), "dgs_forward")
    return R, binning


def round_capacity(cap):
    """cap rounded up to 1/32 of its leading power of two (at least 1024): steps of 3-6 %, so that small drifts of a
    duplicate count do not change the capacity -- and with it the size of every list and what a captured graph holds."""
    q = 1 << max(cap.bit_length() - 5, 10)
    return -(-cap // q) * q


def skip_word_offset(P, W, H, K):
    """Byte offset in the geometry blob of the skip word: status word [5], which a capacity-mode forward sets when its
    count overflowed and which dgs_adam_step / dgs_densify_stats take as `skip_flag` (the geometry blob's layout does not
    depend on R or on wide_records)."""
    return _lib.layout(P, W, H, K, 0, wide_records=False).num_rendered + 4 * 5


def backward_io(R, radii, dL_dout_color, dL_dout_depth, means3D, means2D, sh, opacity, scales, rotations, sh_rest=None,
                opacity_hinge_scale=0.0, stats=None, stats_K_total=0):
    """A DgsBackwardIO for the backward of a forward whose lists hold R duplicates and that wrote radii [K,P].
    means3D ... sh_rest: the caller's gradient outputs (None: not wanted).  The scratch blob and dL_dcolors [P,3], dL_dcov3D
    [P,6], dL_dviewmatrix / dL_dprojmatrix [K,4,4] are allocated here and returned with the struct by those names:
    (io, {"scratch": ..., "colors": ..., "cov3D": ..., "viewmatrix": ..., "projmatrix": ...}).
    stats = (max_radii2D, xyz_gradient_accum, denom): the backward updates the densification accumulators itself."""
    K, P = radii.shape
    f = dict(dtype=torch.float32, device=radii.device)
    scratch = torch.empty(_lib.lib().dgs_backward_scratch_bytes(R, P, K), dtype=torch.uint8, device=radii.device)
    colors, cov3D = torch.empty((P, 3), **f), torch.empty((P, 6), **f)
    view, proj = torch.empty((K, 4, 4), **f), torch.empty((K, 4, 4), **f)
    io = _lib.DgsBackwardIO()
    io.num_rendered = R
    io.radii, io.dL_dout_color, io.dL_dout_depth = _ptr(radii), _ptr(dL_dout_color), _ptr(dL_dout_depth)
    io.scratch, io.scratch_bytes = _ptr(scratch), scratch.numel()
    io.dL_dmeans3D, io.dL_dmeans2D, io.dL_dsh, io.dL_dsh_rest = _ptr(means3D), _ptr(means2D), _ptr(sh), _ptr(sh_rest)
    io.dL_dopacity, io.dL_dscales, io.dL_drotations = _ptr(opacity), _ptr(scales), _ptr(rotations)
    io.dL_dcolors, io.dL_dcov3D, io.dL_dviewmatrix, io.dL_dprojmatrix = _ptr(colors), _ptr(cov3D), _ptr(view), _ptr(proj)
    io.opacity_hinge_scale = opacity_hinge_scale
    if stats is not None:
        io.stats_max_radii2D, io.stats_grad_accum, io.stats_denom = (_ptr(t) for t in stats)
        io.stats_K_total = int(stats_K_total)
    return io, {"scratch": scratch, "colors": colors, "cov3D": cov3D, "viewmatrix": view, "projmatrix": proj}


class Bucket:
    """Layout of a flat fp32 gradient bucket: one segment per tensor, in order, each starting on a 16-byte boundary (the
    fused Adam reads float4).  The cloud's six per-Gaussian gradients live in one (cloud_bucket), in optimiser-group order,
    so that a data-parallel run reduces them with one collective and no packing."""

    def __init__(self, numels):
        self.numels = [int(n) for n in numels]
        self.offsets = [0]
        for n in self.numels:
            self.offsets.append(self.offsets[-1] + (n + 3) // 4 * 4)
        self.size = self.offsets.pop()

    def views(self, flat, shapes):
        """The segments of `flat`, as tensors of these shapes."""
        return [flat[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, shapes)]

    def chunk(self, flat, P, b0, b1):
        """The slices of `flat` that hold rows [b0, b1) of every segment (each segment has P rows)."""
        return [flat[o + b0 * (n // P):o + b1 * (n // P)] for o, n in zip(self.offsets, self.numels)]


def cloud_bucket(P, Mr):
    """xyz, f_dc, f_rest (Mr coefficients), opacity, scaling, rotation of P Gaussians."""
    return Bucket([3 * P, 3 * P, 3 * Mr * P, P, 3 * P, 4 * P])

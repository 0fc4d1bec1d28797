"""The per-Gaussian backward -- geometry_bwd_kernel<1|4|9|16> and pose_grad_reduce_kernel -- tested ALONE: the per-(subframe,
Gaussian) totals it reads are written into the backward's scratch blob by the test (tests/geometry_cases.py), which makes
the kernel a pure function of constructed inputs, and every output is held to float64 autograd through
oracle/torch_naive.py::preprocess at bars one to two orders of magnitude below the end-to-end ones (over_bar in
tests/geometry_cases.py: 4 x the float32-vs-float64 gap of the reference itself, floored at 2^-20 per column and
2^-18 per row; the two matrices per entry at 2^-19 of the absolute sum of their terms, the last column of dL_dprojmatrix at
PROJ_LAST_MULT times that).  No row is exempt.

One forward per case (tile culling off, so that tiles_touched > 0 exactly where radii > 0) is shared by its tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geometry_cases as GC
from helpers import _t, tile_cull
from geometry_cases import over_bar, proj_last_unraised

pytestmark = pytest.mark.gpu

NAMES = list(GC.CASES)
PERM_SEED = 11


class Geometry:
    """The forward of a case -- of its subframes `ks`, with its Gaussians in the order `perm` -- and the backward's
    problem, outputs and scratch, ready for run(S)."""

    def __init__(self, case, perm=None, ks=None):
        from deblurgs_amd import _lib, raster_call
        from deblurgs_amd import diff_gaussian_rasterization as dgr
        from deblurgs_amd.cloud import GaussianCloud
        sc, kw, raw = case["scene"], case["kw"], case["raw"]
        self.case, self.L, self.lib = case, _lib.lib(), _lib
        self.ks = list(range(sc["K"])) if ks is None else list(ks)
        self.perm = np.arange(sc["P"]) if perm is None else np.asarray(perm)
        K, P, dev = len(self.ks), sc["P"], torch.device("cuda")
        self.K, self.P = K, P
        g = lambda a: None if a is None else _t(np.ascontiguousarray(np.asarray(a)[self.perm]))
        view, proj, cam = (_t(sc[n][self.ks]) for n in ("viewmatrix", "projmatrix", "campos"))
        rs = dgr.GaussianRasterizationSettings(
            image_height=sc["H"], image_width=sc["W"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], bg=_t(sc["bg"]),
            scale_modifier=kw["scale_modifier"], z_near=sc["z_near"], z_far=sc["z_far"], use_sigmoid=kw["use_sigmoid"],
            sh_degree=kw["sh_degree"], campos=cam, prefiltered=False, debug=False)
        self.keep = [view, proj, cam, rs]
        f = dict(dtype=torch.float32, device=dev)
        with tile_cull(False), torch.no_grad():
            if raw is None:
                colors, cov = kw.get("colors_precomp"), kw.get("cov3D_precomp")
                args = [g(sc["means3D"]), None if colors is not None else g(sc["sh"]), g(colors),
                        g(sc["opacities"].reshape(-1)), None if cov is not None else g(sc["scales"]),
                        None if cov is not None else g(sc["rotations"]), g(cov)]
                R, _, _, radii, geom, binning, image = dgr._forward_impl(K, *args, view, proj, cam, rs)
                prob = raster_call.problem(K, *args, view, proj, cam, rs, dgr._bg(rs, dev), False, dgr.WIDE_RECORDS,
                                           geom=geom, image=image, binning=binning)
                M = 0 if args[1] is None else args[1].shape[1]
                self.out = dict(means3D=torch.empty((P, 3), **f), means2D=torch.empty((K, P, 3), **f),
                                sh=torch.empty((P, M, 3), **f) if M else None, opacity=torch.empty((P,), **f),
                                scales=None if cov is not None else torch.empty((P, 3), **f),
                                rotations=None if cov is not None else torch.empty((P, 4), **f))
                hinge = 0.0
            else:      # the cloud_problem path: raw parameters, dc | rest split, the activations inside the kernels
                cloud = GaussianCloud(g(raw["xyz"]), g(raw["f_dc"]), g(raw["f_rest"]), g(raw["scaling"]), g(raw["rotation"]),
                                      g(raw["opacity"]), sh_degree=int(round(sc["M"] ** 0.5)) - 1,
                                      active_sh_degree=kw["sh_degree"], z_near=sc["z_near"], z_far=sc["z_far"],
                                      scale_lb=raw["scale_lb"], use_isotrophic=raw["isotropic"])
                rawd = {"scale_lb": raw["scale_lb"], "sh_rest": cloud._features_rest.detach(), "isotropic": raw["isotropic"]}
                args = [cloud._xyz.detach(), cloud._features_dc.detach(), None, cloud._opacity.detach().reshape(-1),
                        cloud._scaling.detach(), cloud._rotation.detach(), None]
                R, _, _, radii, geom, binning, image = dgr._forward_impl(K, *args, view, proj, cam, rs, raw=rawd)
                prob = raster_call.cloud_problem(cloud, K, view, proj, cam, sc["H"], sc["W"], sc["FoVx"], sc["FoVy"],
                                                 dgr._bg(rs, dev), False, geom, image, binning)
                self.keep.append(cloud)
                Mr = cloud._features_rest.shape[1]
                self.out = dict(means3D=torch.empty((P, 3), **f), means2D=torch.empty((K, P, 3), **f),
                                sh=torch.empty((P, 1, 3), **f), sh_rest=torch.empty((P, Mr, 3), **f),
                                opacity=torch.empty((P,), **f), scales=torch.empty((P, 3), **f),
                                rotations=torch.empty((P, 4), **f))
                hinge = raw["hinge"]
            torch.cuda.synchronize()
            # 1. the device radii are the oracle's
            want = case["radii"][self.ks][:, self.perm]
            got = radii.cpu().numpy()
            assert np.array_equal(got, want), f"{int((got != want).sum())} radii differ from the oracle's"
            # 2. problem and io; 3. the compositing backward once, with a zero upstream gradient: the scratch is in the state
            # the per-Gaussian kernel normally finds it in (zero totals in the slots of the visible pairs)
            self.R = int(R)
            self.gC = torch.zeros((K, 3, sc["H"], sc["W"]), **f)
            self.io, self.own = raster_call.backward_io(self.R, radii, self.gC, None, opacity_hinge_scale=hinge, **self.out)
            self.prob, self.blobs, self.args, self.radii = prob, (geom, binning, image), args, radii
            self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            self.check(self.L.dgs_backward_composite(ctypes.byref(prob), ctypes.byref(self.io), self.stream), "composite")
            so, _ = _lib.backward_scratch_layout(self.R, P, K)
            assert so % 16 == 0 and so + K * P * 64 <= self.own["scratch"].numel()
            self.slots = self.own["scratch"][so:so + K * P * 64].view(torch.float32).reshape(K, P, 16)
            self.visible = torch.from_numpy(want > 0).to(dev)
            torch.cuda.synchronize()

    def check(self, rc, what):
        self.lib.check(rc, what)

    def run(self, S, chunks=None, nan_unread=False):
        """4. writes S [K',P,10] (the case's order of Gaussians and subframes; permuted and selected here) into columns
        0..9 of the slots; 5. dgs_backward_geometry over `chunks` (default: one call) and dgs_backward_pose; 6. the outputs
        as numpy, keyed as geometry_cases.reference keys them.  nan_unread: NaN in the slots of the invisible pairs and in
        columns 10..15 of every slot.  Every output buffer is filled with NaN first."""
        S = np.asarray(S, np.float32)[self.ks][:, self.perm]
        for t in list(self.out.values()) + [self.own[n] for n in ("colors", "cov3D", "viewmatrix", "projmatrix")]:
            if t is not None:
                t.fill_(float("nan"))
        self.slots[..., :10] = _t(S)
        self.slots[..., 10:] = float("nan") if nan_unread else 0.0
        if nan_unread:
            self.slots[~self.visible] = float("nan")
        for b0, b1 in ([(0, self.P)] if chunks is None else chunks):
            self.check(self.L.dgs_backward_geometry(ctypes.byref(self.prob), ctypes.byref(self.io), b0, b1, self.stream),
                       "dgs_backward_geometry")
        self.check(self.L.dgs_backward_pose(ctypes.byref(self.prob), ctypes.byref(self.io), self.stream), "dgs_backward_pose")
        torch.cuda.synchronize()
        n = lambda t: t.cpu().numpy().copy()
        o = self.out
        res = dict(dL_dmeans3D=n(o["means3D"]), dL_dopacity=n(o["opacity"]), dL_dmeans2D=n(o["means2D"]),
                   dL_dcolors=n(self.own["colors"]), dL_dcov3D=n(self.own["cov3D"]),
                   dL_dviewmatrix=n(self.own["viewmatrix"]), dL_dprojmatrix=n(self.own["projmatrix"]))
        if o.get("sh") is not None:
            res["dL_dsh"] = n(o["sh"]) if "sh_rest" not in o else np.concatenate([n(o["sh"]), n(o["sh_rest"])], axis=1)
        if o.get("scales") is not None:
            res["dL_dscales"], res["dL_drotations"] = n(o["scales"]), n(o["rotations"])
        return res


@functools.lru_cache(maxsize=None)
def geometry(name, permuted=False):
    case = GC.make(name)
    perm = np.random.default_rng(PERM_SEED).permutation(case["scene"]["P"]) if permuted else None
    return Geometry(case, perm=perm)


@functools.lru_cache(maxsize=None)
def refs(name):
    case = GC.make(name)
    return GC.reference(case, torch.float64), GC.reference(case, torch.float32)


@functools.lru_cache(maxsize=None)
def result(name):
    """(a)'s run: the case's totals, one call."""
    return geometry(name).run(GC.make(name)["S"])


def hold(name, out, keys, r64=None, r32=None, what=""):
    """Every key of `out` against the float64 reference under over_bar; prints the worst error over its bar per key."""
    if r64 is None:
        r64, r32 = refs(name)
    ratios = {key: over_bar(out[key], r64, r32, key) for key in keys}
    line = ", ".join(f"{k} {v:.3f}" for k, v in ratios.items())
    if "dL_dprojmatrix" in keys:
        line += f" (its last column over the unraised 2^-19 A_proj: {proj_last_unraised(out['dL_dprojmatrix'], r64):.3f})"
    print(f"\n[geometry bwd {name}{what}] error / bar: " + line)
    for key in keys:
        assert np.isfinite(out[key]).all(), f"{name}{what}: {key} is not finite"
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{name}{what}: above the bar (error / bar): {bad}"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def hinge_gradient(case):
    """The opacity hinge's own gradient, in the kernel's float32 operations."""
    raw = case["raw"]
    if raw is None or raw["hinge"] == 0.0:
        return np.zeros(case["scene"]["P"], np.float32)
    x = raw["opacity"].reshape(-1).astype(np.float32)
    t = np.where(x <= 0, np.float32(2.0) * x, np.where(x >= 1, np.float32(2.0) * (x - np.float32(1.0)), np.float32(0.0)))
    return (np.float32(raw["hinge"]) * t.astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
def test_against_float64(gpu, name):
    """(a), and (g) for `kmax` (K = DGS_MAX_K = 128: 72 000 bytes of LDS per block, accepted on gfx950): every output within
    its bar of the float64 reference; no row exempt.  The measured figures are in DESIGN.md section 5."""
    hold(name, result(name), GC.output_keys(GC.make(name)))


@pytest.mark.parametrize("name", NAMES)
def test_exact_zeros(gpu, name):
    """(b): dL_dmeans2D of invisible pairs, every output of a never-visible Gaussian but the hinge term, the SH gradients
    above the active degree, and everything for all-zero totals are zeros, not small numbers."""
    case, out = GC.make(name), result(name)
    vis, keys = case["visible"], GC.output_keys(case)
    never = ~vis.any(axis=0)
    hg = hinge_gradient(case)
    assert not out["dL_dmeans2D"][~vis].any(), "dL_dmeans2D of an invisible pair"
    assert not out["dL_dmeans2D"][..., 2].any()
    for key in keys[:-3]:
        got = out[key] if key != "dL_dopacity" else out[key] - hg
        if key == "dL_dopacity":
            assert same_bits(out[key][never], hg[never]), "dL_dopacity of a never-visible Gaussian"
        assert not got[never].any(), f"{key} of a never-visible Gaussian"
    ncoef = (case["kw"]["sh_degree"] + 1) ** 2
    if "dL_dsh" in out and ncoef < case["scene"]["M"]:
        assert not out["dL_dsh"][:, ncoef:].any(), "SH gradient above the active degree"
        assert out["dL_dsh"][:, :ncoef].any()
    zero = geometry(name).run(np.zeros_like(case["S"]))
    for key in keys:
        got = zero[key] if key != "dL_dopacity" else zero[key] - hg
        assert np.isfinite(zero[key]).all() and not got.any(), f"{key} for all-zero totals"
    assert same_bits(zero["dL_dopacity"], hg)


@pytest.mark.parametrize("name", NAMES)
def test_unread_slots_stay_unread(gpu, name):
    """(c): NaN in the slots of the invisible pairs and in columns 10..15 of every slot changes no bit of any output."""
    case, out = GC.make(name), result(name)
    nan = geometry(name).run(case["S"], nan_unread=True)
    for key in GC.output_keys(case):
        assert same_bits(nan[key], out[key]), f"{key} changed with NaN in slots the kernel must not use"


@pytest.mark.parametrize("name", NAMES)
def test_lane_independence(gpu, name):
    """(d): the Gaussians (inputs and totals) in another order, through a forward of their own: the per-Gaussian outputs
    and dL_dmeans2D are the permuted outputs bit for bit; the two matrices, whose sums run in another order, are held to
    (a)'s bar."""
    case, out = GC.make(name), result(name)
    gp = geometry(name, True)
    got = gp.run(case["S"])
    keys = GC.output_keys(case)
    for key in keys[:-3]:
        assert same_bits(got[key], out[key][gp.perm]), f"{key} depends on the lane"
    assert same_bits(got["dL_dmeans2D"], out["dL_dmeans2D"][:, gp.perm]), "dL_dmeans2D depends on the lane"
    hold(name, got, keys[-2:], what=" permuted")


@pytest.mark.parametrize("name", ["deg3", "raw"])
def test_subframe_independence(gpu, name):
    """(e): dL_dmeans2D[k], dL_dviewmatrix[k], dL_dprojmatrix[k] of the K-fused call are those of a one-subframe call given
    subframe k's view and totals, bit for bit; the K-fused per-Gaussian gradients are the float64 sum of the one-subframe
    ones within (a)'s bars (measured against that sum, with the bars of the case)."""
    case, out = GC.make(name), result(name)
    K = case["scene"]["K"]
    singles = [Geometry(case, ks=[k]).run(case["S"]) for k in range(K)]
    for k, one in enumerate(singles):
        for key in ("dL_dmeans2D", "dL_dviewmatrix", "dL_dprojmatrix"):
            assert same_bits(one[key][0], out[key][k]), f"{key}[{k}] differs between the fused and the one-subframe call"
    r64, r32 = refs(name)
    keys = GC.output_keys(case)[:-3]
    summed = dict(r64)
    for key in keys:
        summed[key] = sum(one[key].astype(np.float64) for one in singles)
    # the float32 evaluation's distance from the float64 reference, carried over to the new centre
    moved = dict(r32)
    for key in keys:
        moved[key] = summed[key] + (r32[key] - r64[key])
    hold(name, out, keys, summed, moved, what=" against the sum of its subframes")


def test_chunks(gpu):
    """(f): dgs_backward_geometry over [512, 700), [0, 256), [256, 512) in that order, then dgs_backward_pose: every output
    bit-identical to the single call."""
    case, out = GC.make("deg2"), result("deg2")
    got = geometry("deg2").run(case["S"], chunks=[(512, 700), (0, 256), (256, 512)])
    for key in GC.output_keys(case):
        assert same_bits(got[key], out[key]), f"{key} depends on the chunking"

"""Parity pin: the reference rasteriser's OWN kernels, compiled for gfx950 (oracle/ref_rasterizer.py -> oracle/_ref/), run
on the device next to the CPU oracle and the product's HIP kernels.

  R  the reference's kernels on the device (R_f32: built without FMA contraction; R_fma: with it)
  O  the CPU oracle (oracle/dgs_oracle.cpp), our restatement of those kernels
  H  the product's HIP kernels

Per scene: (a) geometry state R_f32 vs O, bitwise; (b) binning R vs O exact, then H vs R; (c) images R vs O and H vs R, off
the oracle's own margin mask; (d) backward R vs O and (e) H vs R with helpers.assert_grads_close.  The reference sums its
gradients with float atomics in an arbitrary order, so its noise is measured first (R_f32 twice, R_fma once: the largest
column-relative spread among the three, per key, from the reference alone); a key that misses its existing bar is held
to max(existing bar, POSE_NOISE_MULT x that spread) and the report says so.  (f) mark_visible, (g) P = 0.

DGS_REFPIN_REPORT=<file>: the printed figures are appended there as JSON lines."""
import functools
import json
import os

import numpy as np
import pytest

import posed_scenes
import ref_checks
import stack_scenes
from helpers import (GRAD_TOL, POSE_NOISE_MULT, ROW_TOL, OracleRun, assert_grads_close, hip_forward_backward, hip_forward_state,
                     oracle_forward, synthetic, unstable_pixels)
from oracle import ref_rasterizer as rr
from test_gpu_parity import FUZZ, GRAD_KEYS, _check_binning_bits, _grads, adversarial_sprinkles, small_scene

pytestmark = pytest.mark.gpu

if not rr.available():
    pytest.skip("foreign checkout: oracle/_ref/ holds no reference-kernel library and there is no reference tree to build "
                "one from (oracle/ref_rasterizer.py; DGS_REFERENCE_ROOT)", allow_module_level=True)


def _report(case, what, value):
    print(f"   [refpin] {case}: {what}: {value}")
    path = os.environ.get("DGS_REFPIN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "what": what, "value": value}, default=float) + "\n")


# ------------------------------------------------------------------------------------------------------ scenes
def _fuzz(i, subframes=None):
    P, W, H, K, seed, sigma, deg, kw = FUZZ[i]
    sc = adversarial_sprinkles(synthetic.make_scene(P, W, H, K=K, seed=seed, sigma_px=sigma, sh_degree=deg), seed)
    if subframes is not None:
        for key in ("viewmatrix", "projmatrix", "campos"):
            sc[key] = np.ascontiguousarray(sc[key][list(subframes)])
        sc["K"] = K = len(subframes)
    # (the sprinkles may all land in the explicit ill-conditioned set: the bars of test_fuzz_shapes_against_oracle)
    return dict(sc=sc, K=K, kw=dict(kw), grad_kw=dict(ill_frac=0.05, well_frac=0.9))


def _precomp():
    sc = small_scene(P=1800, W=144, H=104, K=1, seed=12)
    st = oracle_forward(sc, 0, render=False)
    cov = st["cov3D"].copy()
    cov[st["depths"] == 0] = np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32)      # culled at the near plane: never read
    col = np.random.default_rng(9).random((sc["P"], 3)).astype(np.float32)
    keys = ["dL_dmeans3D", "dL_dopacities", "dL_dmeans2D", "dL_dviewmatrix", "dL_dprojmatrix", "dL_dcolors_precomp",
            "dL_dcov3D_precomp"]
    return dict(sc=sc, K=1, kw=dict(colors_precomp=col, cov3D_precomp=cov), keys=keys)


def _long_lists():
    sc = small_scene(P=4000, W=96, H=64, K=1, seed=10, sigma_px=6.0)     # test_huge_gaussian_and_long_tile_lists
    sc["scales"][0] = 50.0
    sc["means3D"][0] = [0, 0, 5]
    sc["opacities"][0] = 0.3
    return dict(sc=sc, K=1, kw={}, min_list=257)


def _stack():
    sc, K = stack_scenes.make("batches")
    return dict(sc=sc, K=K, kw={}, grad_kw=stack_scenes.checker_kw("batches"))


CASES = {
    "small": lambda: dict(sc=small_scene(), K=3, kw={}),
    "seed12_sh_scales": lambda: dict(sc=small_scene(P=1800, W=144, H=104, K=1, seed=12), K=1, kw={}),
    "seed12_precomp": _precomp,
    "posed_pin": lambda: dict(sc=posed_scenes.make("pin"), K=2, kw={}),
    "stack_batches": _stack,
    # more than one 256-entry fetch round per tile in the reference's compositing loops (asserted on the oracle's ranges)
    "long_lists": _long_lists,
    "fuzz_subpixel": lambda: _fuzz(1),
    "fuzz_12px": lambda: _fuzz(2),
    "fuzz_deg3_wide": lambda: _fuzz(3),
    # 16 x 16: 1 % of a subframe is 2.56 pixels.  The oracle's margin mask has 2, 3, 1, 1, 1 pixels in the scene's five
    # subframes; subframe 1 (3 of 256 = 1.17 %) does not meet the condition under which the mask may be used, so the case runs
    # the four that do.
    "fuzz_one_tile_sigmoid": lambda: _fuzz(4, subframes=(0, 2, 3, 4)),
    "fuzz_sh_degree_1": lambda: _fuzz(5),
    "fuzz_sh_degree_0": lambda: _fuzz(6),
    "scale_modifier_0p7": lambda: dict(sc=small_scene(P=1500, W=96, H=64, K=1, seed=12), K=1, kw=dict(scale_modifier=0.7)),
    "ragged": lambda: dict(sc=small_scene(P=300, W=75, H=41, K=2, seed=7), K=2, kw={}),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The three parties' forwards of a scene, once: O (and its margin masks, from O alone), R_f32, H (tile_cull = 0)."""
    c = CASES[name]()
    sc, K, kw = c["sc"], c["K"], c["kw"]
    assert sc["K"] >= K
    sc["K"] = K
    run = OracleRun(sc, K, margin_masks=False, **kw)
    run.unstable = [unstable_pixels(st) for st in run.states]
    for k, un in enumerate(run.unstable):
        assert un.sum() <= stack_scenes.MARGIN_FRAC * un.size, f"{name}: margin mask of {int(un.sum())} pixels in subframe {k}"
    if c.get("min_list"):
        lens = run.states[0]["ranges"].astype(np.int64)
        assert (lens[:, 1] - lens[:, 0]).max() >= c["min_list"]
    c.update(name=name, run=run, O=run.states, R=[rr.forward(sc, k, variant="f32", **kw) for k in range(K)],
             H=hip_forward_state(sc, K, **kw), grads={})
    c.setdefault("keys", GRAD_KEYS)
    c.setdefault("grad_kw", {})
    return c


@pytest.fixture(params=list(CASES))
def case(gpu, request):
    return _case(request.param)


def test_build_info_matches_the_tree(gpu):
    """A library built from another recipe or wrapper than this tree's is a failure, not a skip."""
    info = rr.check_build_info()
    assert set(info) >= {"reference_sources", "recipe", "wrapper", "compiler"}
    for v in rr.VARIANTS:
        rr.lib(v)


# ------------------------------------------------------------------------------------------------ a, b, c: forward
def test_geometry_state_reference_vs_oracle_bitwise(case):
    """(a) R_f32 against O: radii, tiles_touched exactly equal; means2D, depths, conic_opacity, cov3D bitwise; the relu mask
    bitwise (pre-sigmoid colours within 1e-5 under use_sigmoid); rgb within 1e-6."""
    relu = not case["kw"].get("use_sigmoid", False)
    ref_checks.check_preprocess(case["R"], case["O"], min_visible=case.get("min_visible", 100), relu=relu)
    exact = {}
    for key in ("rgb", "pre_sigmoid"):      # held to a tolerance above; reported: are they bitwise equal as well?
        exact[key] = all(np.array_equal(r[key][o["radii"] > 0].view(np.uint32), o[key][o["radii"] > 0].view(np.uint32))
                         for r, o in zip(case["R"], case["O"]))
    _report(case["name"], "bitwise beyond the asserted fields", exact)


def test_binning_reference_vs_oracle_and_product_vs_reference(case):
    """(b) num_rendered, sorted keys, point_list, ranges of the non-empty tiles: R against O exact; then H (tile_cull = 0)
    against R through the product's checker with R in the oracle's place."""
    ref_checks.check_binning(case["R"], case["O"])
    _check_binning_bits(case["sc"], case["H"], case["R"])


def test_images_reference_vs_oracle_and_product_vs_reference(case):
    """(c) off the oracle's own margin mask: colour 1e-4, depth 1e-4 of z_far, n_contrib equal, final_T 1e-5; anywhere 2e-2."""
    masks, z_far = case["run"].unstable, case["sc"]["z_far"]
    inmask = []
    for r, o, un in zip(case["R"], case["O"], masks):
        differ = (np.abs(r["color"] - o["color"]).max(axis=0) > ref_checks.IMG_TOL) | \
                 (r["n_contrib"] != o["n_contrib"]).reshape(un.shape)
        inmask.append((int((differ & un).sum()), int(un.sum())))
    _report(case["name"], "in-mask pixels where R and O differ (of mask size), per subframe", inmask)
    ref_checks.check_images(case["R"], case["O"], masks, z_far)
    ref_checks.check_images(ref_checks.plain_images(case["H"]), case["R"], masks, z_far)


# --------------------------------------------------------------------------------------------------- d, e: backward
def _spread(runs, key):
    """Largest column-relative spread of `key` among runs of the reference alone: max over columns of
    max_g (max_run - min_run) / max_g |value|."""
    a = np.stack([np.asarray(r[key], np.float64) for r in runs])
    if key in ("dL_dviewmatrix", "dL_dprojmatrix"):       # per matrix, relative to its largest entry (helpers.relerr)
        a = a.reshape(a.shape[0], a.shape[1], -1)
        return float(((a.max(axis=0) - a.min(axis=0)).max(axis=1) / (np.abs(a[0]).max(axis=1) + 1e-30)).max())
    # rows = (subframe, Gaussian) for the per-subframe outputs, Gaussians otherwise; every component is a column
    a = a.reshape(a.shape[0], -1, a.shape[-1]) if key in ("dL_dmeans2D", "dL_dconic") else a.reshape(a.shape[0], a.shape[1], -1)
    colmax = np.abs(a[0]).max(axis=0)
    nz = colmax > 0
    return float(((a.max(axis=0) - a.min(axis=0)).max(axis=0)[nz] / colmax[nz]).max()) if nz.any() else 0.0


def _backward(case, depth):
    """Upstream gradients zeroed on the oracle's margin mask; O's three builds; R_f32 twice and R_fma once."""
    if depth not in case["grads"]:
        sc, K, kw, run = case["sc"], case["K"], case["kw"], case["run"]
        gC, gD = run.mask(*_grads(sc, K, depth=depth))
        ra = rr.forward_backward(sc, K, gC, gD, states=case["R"])
        rb = rr.forward_backward(sc, K, gC, gD, states=case["R"])
        rf = rr.forward_backward(sc, K, gC, gD, variant="fma", **kw)
        keys = list(case["keys"]) + ["dL_dconic", "dL_dcov3D"]
        spread = {key: _spread([ra, rb, rf], key) for key in keys}
        _report(case["name"], f"atomics spread per key (depth={depth})", spread)
        # (reported only: how much of it is the order of the atomics alone -- the uncontracted build against itself)
        _report(case["name"], f"of which R_f32 against R_f32 (depth={depth})", {key: _spread([ra, rb], key) for key in keys})
        case["grads"][depth] = dict(gC=gC, gD=gD, O=run.backward(gC, gD), Ra=ra, spread=spread, keys=keys)
    return case["grads"][depth]


def _assert_grads(name, what, got, ora, keys, spread, **kw):
    """helpers.assert_grads_close key by key, unchanged bars.  A key that fails them is held to max(existing bar,
    POSE_NOISE_MULT x the reference's own atomics spread of that key): the column bar, and the row bar in the checker's own
    ratio (ROW_TOL / GRAD_TOL = 10: a row is measured against >= ROW_FLOOR = 0.1 of the column scale)."""
    for key in keys:
        try:
            assert_grads_close(got, ora, [key], **kw)
        except AssertionError as first:
            tol = max(GRAD_TOL, POSE_NOISE_MULT * spread[key])
            _report(name, f"{what} {key}", dict(failed_existing_bar=str(first), spread=spread[key], bar_used=tol))
            if tol <= GRAD_TOL:
                raise
            assert_grads_close(got, ora, [key], tol=tol, row_tol=tol * (ROW_TOL / GRAD_TOL), **kw)


@pytest.mark.parametrize("depth", [True, False])
def test_backward_reference_vs_oracle(case, depth):
    """(d) R_f32 in the product's place of helpers.assert_grads_close, against O."""
    b = _backward(case, depth)
    _assert_grads(case["name"], "R vs O", b["Ra"], b["O"], b["keys"], b["spread"], **case["grad_kw"])


@pytest.mark.parametrize("depth", [True, False])
def test_backward_product_vs_reference(case, depth):
    """(e) H against R_f32: R's arrays stand where the oracle's stand in the checker; the conditioning yardstick (how far two
    correct fp32 builds move a row) is still the oracle's: its f32 and fma builds' offsets from its double build, carried
    over to R.

    Measured on the MI355X: every key of every scene meets the unchanged bars but dL_drotations of fuzz_deg3_wide without
    depth gradients (1.28e-4 per column on the well-conditioned rows; the reference's own spread on that key 8.6e-5, bar used
    max(1e-4, 4 x 8.6e-5) = 3.4e-4)."""
    b = _backward(case, depth)
    hip = hip_forward_backward(case["sc"], case["K"], b["gC"], b["gD"], **case["kw"])
    O = b["O"]
    ref = {"double": {}, "f32": {}, "fma": {}}
    for key in b["keys"]:
        r = np.asarray(b["Ra"][key], np.float64).reshape(O["double"][key].shape)
        ref["double"][key] = r
        ref["f32"][key] = r + (O["f32"][key] - O["double"][key])
        ref["fma"][key] = r + (O["fma"][key] - O["double"][key])
    _assert_grads(case["name"], "H vs R", hip, ref, b["keys"], b["spread"], **case["grad_kw"])


# ------------------------------------------------------------------------------------------------------------ f, g
def test_mark_visible_three_ways(gpu):
    """(f) a third of the cloud behind the camera: R, O and H agree exactly."""
    from helpers import hip_settings, _t
    from deblurgs_amd.diff_gaussian_rasterization import GaussianRasterizer
    from oracle import oracle
    sc = small_scene(P=500, W=64, H=64, K=1)
    sc["means3D"][::3, 2] *= -1
    o = oracle.mark_visible(sc["means3D"], sc["viewmatrix"][0])
    r = rr.mark_visible(sc["means3D"], sc["viewmatrix"][0], sc["projmatrix"][0])
    h = GaussianRasterizer(hip_settings(sc, 1)).markVisible(_t(sc["means3D"]), _t(sc["viewmatrix"][0]),
                                                            _t(sc["projmatrix"][0])).cpu().numpy()
    assert 100 < o.sum() < 400
    assert np.array_equal(r, o) and np.array_equal(h, r)


def test_empty_cloud(gpu):
    """(g) P = 0: the reference's binding returns before touching anything (zero images, no launch); the front-end applies
    that guard, and the product's zeros are checked against the front-end's."""
    import torch
    from helpers import hip_settings, _t
    from deblurgs_amd.diff_gaussian_rasterization import GaussianRasterizer
    sc = dict(small_scene(P=64, W=64, H=48, K=1, seed=8))
    empty = dict(sc, means3D=np.zeros((0, 3), np.float32), sh=np.zeros((0, 9, 3), np.float32),
                 opacities=np.zeros((0, 1), np.float32), scales=np.zeros((0, 3), np.float32),
                 rotations=np.zeros((0, 4), np.float32))
    r = rr.forward(empty, 0)
    assert r["num_rendered"] == 0 and not r["color"].any() and not r["depth"].any() and r["radii"].size == 0
    assert rr.mark_visible(empty["means3D"], sc["viewmatrix"][0], sc["projmatrix"][0]).size == 0
    e = torch.zeros((0, 3), device="cuda")
    c, d, rad = GaussianRasterizer(hip_settings(sc, 1))(
        e, e.clone(), torch.zeros((0, 1), device="cuda"), shs=torch.zeros((0, 9, 3), device="cuda"), scales=e.clone(),
        rotations=torch.zeros((0, 4), device="cuda"), viewmatrix=_t(sc["viewmatrix"][0]), projmatrix=_t(sc["projmatrix"][0]))
    assert np.array_equal(c.cpu().numpy(), r["color"]) and np.array_equal(d.cpu().numpy().reshape(r["depth"].shape), r["depth"])
    assert rad.numel() == 0

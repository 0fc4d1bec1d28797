"""GPU parity on the constructed tile-list scenes of tests/stack_scenes.py: the compositing kernels (csrc/composite.hip)
at their structural edges -- lists of exactly 63 / 64 / 65 / 127 / 128 / 129 entries, last contributors on both sides of a
batch boundary, quadrants that finish a batch before their neighbours, termination taken and never taken, empty and ragged
tiles, K * T of 1 and 5, splats grazing the quadrant boxes at the alpha threshold -- against the CPU oracle, against float64
autograd directly, and against themselves (tile culling on / off, forward-only, a dirty backward scratch, pose-only)."""
import ctypes

import numpy as np
import pytest

import stack_scenes as S
from helpers import (GRAD_TOL, OracleRun, _t, assert_grads_close, capped_exempt_masks, describe_exempt, exempt_cap,
                     hip_forward_backward, hip_forward_state, hip_settings, oracle, relerr, tile_cull)
from test_gpu_evaluation import pose_only_vs_full
from test_gpu_parity import DEPTH_TOL, IMG_TOL, _check_binning_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=S.NAMES)
def case(request, gpu):
    """A catalogue scene with its preconditions asserted, the oracle (margin masks), the HIP forward on the reference's
    lists with contributor checksums, and the exact disagreement masks."""
    name = request.param
    sc, K = S.make(name)
    run = OracleRun(sc, K)
    S.preconditions(name, run.states)
    hip = hip_forward_state(sc, K, checksum=True)
    return dict(name=name, sc=sc, K=K, run=run, hip=hip, cache={})


def _exact(case):
    """OracleRun(exact=True) of the scene, once: the masks are the pixels whose per-pair decisions differ (bounded by
    helpers.capped_exempt_masks)."""
    if "exact" not in case["cache"]:
        case["cache"]["exact"] = OracleRun(case["sc"], case["K"], exact=True)
    return case["cache"]["exact"]


# ------------------------------------------------------------------------------------------------------- forward
def test_forward_on_the_reference_lists(case):
    """tile_cull = 0: sort keys, point lists, tile ranges, radii and tile counts bit-equal to the oracle's; off the exempt
    pixels the last contributor is equal, final_T within 1e-5, colour and depth within the image bars."""
    sc, K, run, hip = case["sc"], case["K"], case["run"], case["hip"]
    _check_binning_bits(sc, hip, run.states)
    ex = _exact(case).unstable
    for k, o in enumerate(run.states):
        assert np.array_equal(hip["radii"][k], o["radii"]), "radii"
        assert np.array_equal(hip["tiles_touched"][k], o["tiles_touched"]), "tiles_touched"
        keep = ~ex[k]
        s = keep.reshape(-1)
        assert np.array_equal(hip["n_contrib"][k][s], o["n_contrib"][s]), f"n_contrib k={k}"
        assert np.abs(hip["final_T"][k][s] - o["final_T"][s]).max() <= 1e-5, f"final_T k={k}"
        dc = np.abs(hip["color"][k] - o["color"]).max(axis=0)
        dd = np.abs(hip["depth"][k][0] - o["depth"][0]) / sc["z_far"]
        assert dc[keep].max() <= IMG_TOL, f"colour k={k}: {dc[keep].max()}"
        assert dd[keep].max() <= DEPTH_TOL, f"depth k={k}: {dd[keep].max()}"


def test_exempt_set_is_the_oracles_own_doubt_and_nothing_else(case):
    """Every pixel where the HIP traversal took another per-pair decision than the oracle's lies inside the oracle's margin
    mask (a pair within a rounding error of a threshold), and there are at most max(2e-4 H W, 4) of them per subframe.  On
    `grazers` this is the test of the quadrant cull and of the tile cull's hit test: 66 + 68 quadrant boxes hold a pair
    whose best pixel has alpha in [1, 1.5) / 255 and really blends it; a wrongly dropped pair with alpha >= 1/255 + 5e-7
    is a checksum difference outside the margin mask."""
    run, hip = case["run"], case["hip"]
    masks = capped_exempt_masks(run.states, hip["contrib_checksum"], hip["n_contrib"], what=case["name"])
    for k, (ex, st) in enumerate(zip(masks, run.states)):
        print(f"[{case['name']} k={k}] exempt {int(ex.sum())}, margin {int(run.unstable[k].sum())}")
        assert ex.sum() <= exempt_cap(st)
        outside = ex & ~run.unstable[k]
        assert not outside.any(), (f"{case['name']} k={k}: a per-pair decision differs where the oracle has no doubt:\n   "
                                   + describe_exempt(st, outside, hip["contrib_checksum"][k], hip["n_contrib"][k]))


def test_forward_on_tile_culled_lists_is_bit_identical(case):
    cul = hip_forward_state(case["sc"], case["K"], cull=True)
    for key in ("radii", "color", "depth", "final_T"):       # (n_contrib is a position in the list, which culling shortens)
        assert np.array_equal(cul[key], case["hip"][key]), key
    assert (cul["n_contrib"] <= case["hip"]["n_contrib"]).all()


def _abi_forward(sc, K, cull, forward_only, with_depth):
    """One forward through the C ABI with DgsProblem.forward_only and DgsForwardOut.out_depth as given."""
    import torch
    from deblurgs_amd import _lib, raster_call
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    L = _lib.lib()
    dev = torch.device("cuda")
    rs = hip_settings(sc, K)._replace(campos=_t(sc["campos"][:K]))
    P, H, W = sc["P"], sc["H"], sc["W"]
    color = torch.full((K, 3, H, W), float("nan"), device=dev)
    depth = torch.full((K, 1, H, W), float("nan"), device=dev) if with_depth else None
    radii = torch.full((K, P), -7, dtype=torch.int32, device=dev)
    geom = torch.empty(L.dgs_geom_state_bytes(P, K), dtype=torch.uint8, device=dev)
    image = torch.empty(L.dgs_image_state_bytes_forward_only(W, H, K) if forward_only else L.dgs_image_state_bytes(W, H, K),
                        dtype=torch.uint8, device=dev)
    host = dgr._pinned_word(dev)
    out = raster_call.forward_out(color, depth, radii, host)
    args = [_t(sc["means3D"]), _t(sc["sh"]), None, _t(sc["opacities"]).reshape(-1), _t(sc["scales"]), _t(sc["rotations"]), None]
    cams = [_t(sc["viewmatrix"][:K]), _t(sc["projmatrix"][:K]), _t(sc["campos"][:K])]
    prob = raster_call.problem(K, *args, *cams, rs, dgr._bg(rs, dev), cull, dgr.WIDE_RECORDS, forward_only=forward_only,
                               geom=geom, image=image)
    raster_call.forward(dev, prob, out, host)
    torch.cuda.synchronize()
    return color.cpu().numpy(), None if depth is None else depth.cpu().numpy(), radii.cpu().numpy()


@pytest.mark.parametrize("cull", [True, False])
def test_forward_only_call_gives_the_same_bits(case, cull):
    """DgsProblem.forward_only (the inference call: no final_T / n_contrib kept), with and without the depth output."""
    hip = case["hip"]
    for forward_only, with_depth in ((True, True), (True, False), (False, False)):
        color, depth, radii = _abi_forward(case["sc"], case["K"], cull, forward_only, with_depth)
        assert np.array_equal(color, hip["color"]), (forward_only, with_depth)
        assert np.array_equal(radii, hip["radii"]), (forward_only, with_depth)
        if with_depth:
            assert np.array_equal(depth, hip["depth"]), (forward_only, with_depth)


# ------------------------------------------------------------------------------------------------------ backward
def _backward(case, depth, cull):
    """(masked upstream gradients, HIP forward + backward through the operator) of a scene, once per (depth, cull)."""
    key = ("bwd", depth, cull)
    if key not in case["cache"]:
        gC, gD = _exact(case).mask(*S.upstream(case["sc"], case["K"], depth=depth))
        with tile_cull(cull):
            hip = hip_forward_backward(case["sc"], case["K"], gC, gD)
        case["cache"][key] = (gC, gD, hip)
    return case["cache"][key]


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("depth", [True, False])
def test_backward_against_the_oracle(case, depth, cull):
    """Upstream gradients zero on the exempt pixels only; on the stack scenes every Gaussian is held to the flat 1e-4 / 1e-3
    bars (no ill-conditioned set: tests/test_stack_scenes_host.py shows the reference's own fp32 builds meet them)."""
    gC, gD, hip = _backward(case, depth, cull)
    okey = ("ora", depth)
    if okey not in case["cache"]:
        case["cache"][okey] = _exact(case).backward(gC, gD)
    ora = case["cache"][okey]
    kw = S.checker_kw(case["name"])
    for mode in ("f32", "fma"):     # the precondition of the bars: two fp32 builds of the reference meet them
        assert_grads_close(ora[mode], ora, S.CHECK_KEYS, **kw)
    assert np.array_equal(hip["radii"], np.stack([o["radii"] for o in case["run"].states]))
    assert_grads_close(hip, ora, S.CHECK_KEYS, **kw)


@pytest.mark.parametrize("depth", [True, False])
def test_backward_bits_do_not_depend_on_tile_culling(case, depth):
    a, b = _backward(case, depth, True)[2], _backward(case, depth, False)[2]
    for key in S.CHECK_KEYS + ["color", "depth"]:
        assert np.array_equal(a[key], b[key]), key


def test_backward_against_float64_autograd_directly(gpu):
    """The one place where a HIP gradient meets a high-precision reference without the fp32 oracle in between: `batches`,
    subframe 1 of the K = 3 call (the other subframes get a zero upstream gradient), against autograd through the dense
    float64 rasteriser.  relerr <= GRAD_TOL per tensor, the two analytic columns of dL_dprojmatrix each against its own
    largest entry.  The oracle's fp32 sits at <= 5.0e-6 of the same reference (tests/test_stack_scenes_host.py)."""
    sc, K = S.make("batches")
    k = 1
    run = OracleRun(sc, K, exact=True)
    un = run.unstable[k] | oracle.unstable(run.states[k])      # float64 decides differently where fp32 itself is in doubt
    gC, gD = S.upstream(sc, K, depth=True)
    for j in range(K):
        if j != k:
            gC[j] = 0.0
            gD[j] = 0.0
    gC[k][:, un] = 0.0
    gD[k][:, un] = 0.0
    hip = hip_forward_backward(sc, K, gC, gD)
    ref = S.float64_reference(sc, k, gC[k], gD[k])
    assert np.array_equal(ref["radii"], hip["radii"][k])
    assert np.abs(ref["color"] - hip["color"][k]).max(axis=0)[~un].max() <= IMG_TOL
    got = {key: hip[key] for key in S.GRAD_KEYS}
    for key in ("dL_dviewmatrix", "dL_dprojmatrix"):
        rest = np.delete(hip[key], k, axis=0)
        assert not rest.any(), f"{key}: subframes without an upstream gradient must get exact zeros"
        got[key] = hip[key][k]
    err = S.errors_to_float64(got, ref)
    print("[batches k=1] HIP against float64: " + ", ".join(f"{n} {e:.2e}" for n, e in err.items()))
    for key, e in err.items():
        assert e <= GRAD_TOL, f"{key}: {e:.3e}"


# ------------------------------------------------------------------------------- the backward's caller-owned scratch
def _backward_on_scratch(sc, K, cull, gC, gD, fills, pose_only):
    """One forward through the C ABI, then one backward (dgs_backward, or dgs_backward_pose_only) per entry of `fills` on
    the SAME forward state, the scratch blob filled with that byte beforehand and every gradient output with NaN.
    Returns one dict of outputs (numpy) per fill."""
    import torch
    from deblurgs_amd import _lib, raster_call
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    L = _lib.lib()
    dev = torch.device("cuda")
    rs = hip_settings(sc, K)._replace(campos=_t(sc["campos"][:K]))
    args = [_t(sc["means3D"]), _t(sc["sh"]), None, _t(sc["opacities"]).reshape(-1), _t(sc["scales"]), _t(sc["rotations"]), None]
    cams = [_t(sc["viewmatrix"][:K]), _t(sc["projmatrix"][:K]), _t(sc["campos"][:K])]
    with tile_cull(cull), torch.no_grad():
        R, color, depth, radii, geom, binning, image = dgr._forward_impl(K, *args, *cams, rs)
        prob = raster_call.problem(K, *args, *cams, rs, dgr._bg(rs, dev), cull, dgr.WIDE_RECORDS, geom=geom, image=image,
                                   binning=binning)
    R, P, M = int(R), sc["P"], sc["sh"].shape[1]
    gCt, gDt = _t(gC), (None if gD is None else _t(gD))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    outs = []
    for fill in fills:
        if pose_only:
            bufs = dict(means3D=None, means2D=None, sh=None, opacity=None, scales=None, rotations=None)
        else:
            bufs = dict(means3D=nan(P, 3), means2D=nan(K, P, 3), sh=nan(P, M, 3), opacity=nan(P), scales=nan(P, 3),
                        rotations=nan(P, 4))
        io, own = raster_call.backward_io(R, radii, gCt, gDt, **bufs)
        own["scratch"].fill_(fill)
        for n in ("colors", "cov3D", "viewmatrix", "projmatrix"):
            own[n].fill_(float("nan"))
        if pose_only:
            io.dL_dcolors = io.dL_dcov3D = None
            _lib.check(L.dgs_backward_pose_only(ctypes.byref(prob), ctypes.byref(io), stream), "dgs_backward_pose_only")
            names = {"viewmatrix": own["viewmatrix"], "projmatrix": own["projmatrix"]}
        else:
            _lib.check(L.dgs_backward(ctypes.byref(prob), ctypes.byref(io), stream), "dgs_backward")
            names = dict(bufs, **{n: own[n] for n in ("colors", "cov3D", "viewmatrix", "projmatrix")})
        torch.cuda.synchronize()
        outs.append({n: t.cpu().numpy().copy() for n, t in names.items()})
    return outs


@pytest.mark.parametrize("pose_only", [False, True])
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("depth", [True, False])
def test_backward_never_reads_a_stale_word_of_its_scratch(gpu, depth, cull, pose_only):
    """dgs_backward / dgs_backward_pose_only take a caller-owned, UNINITIALISED scratch blob.  The blob holds only
    floating-point words (contribution rows, their totals, the double partials of the pose gradients: csrc/api.hip,
    scratch_layout), so any byte pattern is a legal input.  On `batches` (K = 3; lists that end inside, at the end of and
    right behind a batch, entries no pixel reaches whose rows the kernel zero-fills instead of walking, an empty tile) a
    blob of zeros and a blob of 0xFF bytes (NaNs) must give the same bits, all finite, in every output -- each of which is
    handed in full of NaN, as the operator hands them in uninitialised."""
    sc, K = S.make("batches")
    gC, gD = S.upstream(sc, K, depth=depth)
    clean, dirty = _backward_on_scratch(sc, K, cull, gC, gD, (0x00, 0xFF), pose_only)
    for name in clean:
        assert np.isfinite(dirty[name]).all(), f"dL_d{name}: not finite on a dirty scratch"
        assert np.isfinite(clean[name]).all(), f"dL_d{name}: not finite"
        assert np.array_equal(clean[name].view(np.uint32), dirty[name].view(np.uint32)), f"dL_d{name}: depends on the scratch"
    assert np.abs(clean["viewmatrix"]).max() > 0


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("depth", [True, False])
def test_pose_only_backward_equals_the_full_backward_on_batches(gpu, depth, cull):
    """The rule of tests/test_gpu_evaluation.py::test_pose_only_backward_equals_the_full_backward on the constructed lists."""
    sc, K = S.make("batches")
    gC, gD = S.upstream(sc, K, depth=depth)
    full, outs = pose_only_vs_full(sc, K, cull, gC, gD)
    for i, name in enumerate(("dL_dviewmatrix", "dL_dprojmatrix")):
        assert np.isfinite(full[i]).all() and np.abs(full[i]).max() > 0
        e = relerr(outs[0][i], full[i])
        assert e <= GRAD_TOL, (name, e)
        assert np.array_equal(outs[0][i], outs[1][i]), name + ": two calls differ"
        assert np.array_equal(outs[0][i], outs[2][i]), name + ": NULL gradient pointers change the result"

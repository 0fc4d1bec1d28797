"""GPU tests of the evaluation protocol (ABI 15): the pose-only backward against the full one and against the CPU oracle,
the view-loss and metrics kernels against torch in float64 and the reference's fixture, the fused pose fit against the
same fit driven through render() + autograd + torch.optim.Adam, and evaluate()."""
import contextlib
import ctypes

import numpy as np
import pytest

from helpers import GRAD_TOL, _t, hip_settings, oracle_forward_backward, relerr, synthetic, tile_cull
from test_evaluation_host import CASES, EPS32, check_metrics, view_loss_case, view_loss_torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def small_scene(P=2500, W=160, H=120, K=3, seed=2, **kw):
    return synthetic.make_scene(P, W, H, K=K, seed=seed, **kw)


def _grads(sc, K, seed=5, depth=True):
    """The upstream gradients of tests/test_gpu_parity.py::test_backward_vs_oracle (same seed, same draws)."""
    rng = np.random.default_rng(seed)
    gC = rng.normal(size=(K, 3, sc["H"], sc["W"])).astype(np.float32)
    gD = (rng.normal(size=(K, 1, sc["H"], sc["W"])) * 0.05).astype(np.float32) if depth else None
    return gC, gD


def _precomp(sc, which):
    rng = np.random.default_rng(17)
    if which == "colors":
        return rng.uniform(0.0, 1.0, (sc["P"], 3)).astype(np.float32)
    s, q = sc["scales"].astype(np.float64), sc["rotations"].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    M = R * s[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32)


def pose_only_vs_full(sc, K, cull, gC, gD, sh_degree=None, use_sigmoid=False, colors=False, cov=False, raw=False):
    """One forward through the C ABI, then dgs_backward and (twice) dgs_backward_pose_only on the SAME state.  Every
    gradient buffer of the pose-only call but the two matrices is handed in filled with a sentinel.  Returns the two
    matrices of each call as numpy plus the sentinel buffers after the call."""
    import torch
    from deblurgs_amd import _lib, raster_call
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    from deblurgs_amd.cloud import GaussianCloud
    L = _lib.lib()
    dev = torch.device("cuda")
    rs = hip_settings(sc, K, sh_degree, use_sigmoid)._replace(campos=_t(sc["campos"][:K]))
    view, proj, cam = _t(sc["viewmatrix"][:K]), _t(sc["projmatrix"][:K]), _t(sc["campos"][:K])
    rawd = None
    if raw:
        c = GaussianCloud.from_scene(sc, "cuda")
        rest = c._features_rest if c._features_rest.shape[1] > 0 else None
        rawd = {"scale_lb": 0.0, "sh_rest": rest}
        args = [c._xyz.detach(), c._features_dc.detach(), None, c._opacity.detach().reshape(-1), c._scaling.detach(),
                c._rotation.detach(), None]
    else:
        args = [_t(sc["means3D"]), None if colors else _t(sc["sh"]), _t(_precomp(sc, "colors")) if colors else None,
                _t(sc["opacities"]).reshape(-1), None if cov else _t(sc["scales"]), None if cov else _t(sc["rotations"]),
                _t(_precomp(sc, "cov")) if cov else None]
    with tile_cull(cull), torch.no_grad():
        R, color, depth, radii, geom, binning, image = dgr._forward_impl(K, *args, view, proj, cam, rs, raw=rawd)
        prob = raster_call.problem(K, *args, view, proj, cam, rs, dgr._bg(rs, dev), cull, dgr.WIDE_RECORDS, raw=rawd,
                                   geom=geom, image=image, binning=binning)
    R, P = int(R), sc["P"]
    gCt, gDt = _t(gC[:K]), (None if gD is None else _t(gD[:K]))
    f = dict(dtype=torch.float32, device=dev)
    M = 0 if args[1] is None else args[1].shape[1]
    Mr = 0 if rawd is None or rawd["sh_rest"] is None else rawd["sh_rest"].shape[1]

    def bufs(fill):
        mk = (lambda *s: torch.full(s, fill, **f)) if fill is not None else (lambda *s: torch.empty(s, **f))
        return dict(means3D=mk(P, 3), means2D=mk(K, P, 3), sh=mk(P, max(M, 1), 3) if args[1] is not None else None,
                    sh_rest=mk(P, Mr, 3) if Mr > 0 else None, opacity=mk(P), scales=None if cov else mk(P, 3),
                    rotations=None if cov else mk(P, 4))

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    full_b = bufs(None)
    io, own = raster_call.backward_io(R, radii, gCt, gDt, **full_b)
    _lib.check(L.dgs_backward(ctypes.byref(prob), ctypes.byref(io), st), "dgs_backward")
    torch.cuda.synchronize()
    full = (own["viewmatrix"].cpu().numpy().copy(), own["projmatrix"].cpu().numpy().copy())
    outs = []
    sent = bufs(SENTINEL)
    for rep in range(2):
        io2, own2 = raster_call.backward_io(R, radii, gCt, gDt, **sent)
        own2["colors"].fill_(SENTINEL)
        own2["cov3D"].fill_(SENTINEL)
        io2.stats_max_radii2D = io2.stats_grad_accum = io2.stats_denom = None
        own2["viewmatrix"].fill_(SENTINEL)
        own2["projmatrix"].fill_(SENTINEL)
        _lib.check(L.dgs_backward_pose_only(ctypes.byref(prob), ctypes.byref(io2), st), "dgs_backward_pose_only")
        torch.cuda.synchronize()
        outs.append((own2["viewmatrix"].cpu().numpy().copy(), own2["projmatrix"].cpu().numpy().copy()))
        for name, t in list(sent.items()) + [("colors", own2["colors"]), ("cov3D", own2["cov3D"])]:
            if t is not None:
                assert bool((t == SENTINEL).all()), f"dgs_backward_pose_only wrote to dL_d{name}"
    # ... and with every other pointer NULL
    io3 = _lib.DgsBackwardIO()
    io3.num_rendered = R
    scratch = torch.empty(L.dgs_backward_scratch_bytes(R, P, K), dtype=torch.uint8, device=dev)
    gv, gp = torch.full((K, 4, 4), SENTINEL, **f), torch.full((K, 4, 4), SENTINEL, **f)
    io3.radii, io3.dL_dout_color = radii.data_ptr(), gCt.data_ptr()
    io3.dL_dout_depth = None if gDt is None else gDt.data_ptr()
    io3.scratch, io3.scratch_bytes = scratch.data_ptr(), scratch.numel()
    io3.dL_dviewmatrix, io3.dL_dprojmatrix = gv.data_ptr(), gp.data_ptr()
    _lib.check(L.dgs_backward_pose_only(ctypes.byref(prob), ctypes.byref(io3), st), "dgs_backward_pose_only (NULLs)")
    torch.cuda.synchronize()
    outs.append((gv.cpu().numpy(), gp.cpu().numpy()))
    return full, outs


CASES_POSE = [
    # K, tile_cull, depth gradient, keyword arguments
    (3, 1, True, {}),
    (3, 0, True, {}),
    (1, 1, True, {}),
    (1, 0, False, {}),
    (3, 1, False, {}),
    (3, 1, True, {"sh_degree": 0}),
    (3, 0, True, {"sh_degree": 3}),
    (1, 1, True, {"sh_degree": 3}),
    (3, 1, True, {"use_sigmoid": True}),
    (3, 1, True, {"colors": True}),
    (3, 0, False, {"cov": True}),
    (3, 1, True, {"raw": True}),
    (1, 0, True, {"raw": True}),
]


@pytest.mark.parametrize("K,cull,depth,kw", CASES_POSE)
def test_pose_only_backward_equals_the_full_backward(gpu, K, cull, depth, kw):
    """dL_dviewmatrix / dL_dprojmatrix of dgs_backward_pose_only against dgs_backward on the same forward state; nothing
    else written; two calls, and a call with every other gradient pointer NULL, give identical bits.

    The two are NOT bit-identical, and cannot be made so from this side: geometry_bwd.hip is built
    with SLP vectorisation, which packs pairs of scalar multiplies / adds chosen from ALL operations of the loop body
    into v_pk_* instructions before the backend contracts multiplies into FMAs; the full kernel's loop holds the
    dL_dcov3D / dL_dmean3D sums as well, so other pairs are packed and other multiplies fused than in the pose-only loop,
    and a few per-Gaussian terms round once instead of twice.  Measured on the MI355X over these 13 cases:
    dL_dviewmatrix 3.2e-6 ... 9.0e-6 of its largest entry apart (dL_dprojmatrix is printed by the run); the same test
    against a build of that file with -fno-slp-vectorize (or with -ffp-contract=off) gives 0 in all 13 -- at the price
    of changing every existing gradient's bits, which is why the product is not built that way.  The assertion is
    therefore the project's bar for these matrices, relerr <= GRAD_TOL (what the oracle test below holds both paths
    to)."""
    sc = small_scene(sh_degree=3) if kw.get("sh_degree") == 3 else small_scene()
    gC, gD = _grads(sc, 3, depth=depth)
    full, outs = pose_only_vs_full(sc, K, bool(cull), gC, gD, **kw)
    for i, name in enumerate(("dL_dviewmatrix", "dL_dprojmatrix")):
        assert np.isfinite(full[i]).all() and np.abs(full[i]).max() > 0
        e = relerr(outs[0][i], full[i])
        print(f"{name}: relerr pose-only vs full {e:.3e}")
        assert e <= GRAD_TOL, (name, e)
        assert np.array_equal(outs[0][i], outs[1][i]), name + ": two calls differ"
        assert np.array_equal(outs[0][i], outs[2][i]), name + ": NULL gradient pointers change the result"


@pytest.mark.parametrize("depth", [True, False])
def test_pose_only_backward_against_the_oracle(gpu, depth):
    """The scene, seeds, statistic and bar with which test_backward_vs_oracle passes for the full path."""
    sc = small_scene()
    gC, gD = _grads(sc, 3, depth=depth)
    ora = oracle_forward_backward(sc, 3, gC, gD)
    _, outs = pose_only_vs_full(sc, 3, True, gC, gD)
    for i, key in enumerate(("dL_dviewmatrix", "dL_dprojmatrix")):
        e = relerr(outs[0][i].reshape(ora[key].shape), ora[key])
        print(f"{key}: rel err vs oracle {e:.3e}")
        assert e <= GRAD_TOL, f"{key}: rel err {e:.3e}"


def test_pose_only_backward_honours_the_truncated_list_flag_and_never_forks(gpu):
    """Capacity mode with a capacity below the count: status word [5] is set, the kernels that would walk the truncated
    lists return at once and the call completes (its outputs are meaningless, as dgs_backward's are on such a state: the
    caller discards the step through the skip word).  With a context that forks every K >= 2 backward (bwd_overlap = 2)
    the pose-only call gives the same bits as with no context at all: it runs on the caller's stream alone."""
    import torch
    from deblurgs_amd import _lib, raster_call
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    L = _lib.lib()
    sc = small_scene()
    K, P = 3, sc["P"]
    gC, _ = _grads(sc, 3, depth=False)
    rs = hip_settings(sc, K)._replace(campos=_t(sc["campos"][:K]))
    args = [_t(sc["means3D"]), _t(sc["sh"]), None, _t(sc["opacities"]).reshape(-1), _t(sc["scales"]), _t(sc["rotations"]), None]
    cams = [_t(sc["viewmatrix"][:K]), _t(sc["projmatrix"][:K]), _t(sc["campos"][:K])]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    with tile_cull(True), torch.no_grad():
        R0 = int(dgr._forward_impl(K, *args, *cams, rs)[0])
        for cap, mode in ((R0 // 3, 1), (R0 + 1000, 1), (R0 + 1000, 2), (R0 + 1000, None)):
            with (_lib.context_options(bwd_overlap=mode) if mode is not None else contextlib.nullcontext()):
                R, color, depth, radii, geom, binning, image = dgr._forward_impl(K, *args, *cams, rs, capacity=cap)
                assert R.overflow == (cap < R0)
                prob = raster_call.problem(K, *args, *cams, rs, dgr._bg(rs, torch.device("cuda")), True, dgr.WIDE_RECORDS,
                                           geom=geom, image=image, binning=binning)
                if mode is None:
                    prob.context = None
                io, own = raster_call.backward_io(cap, radii, _t(gC), None, None, None, None, None, None, None)
                own["viewmatrix"].fill_(SENTINEL)
                own["projmatrix"].fill_(SENTINEL)
                _lib.check(L.dgs_backward_pose_only(ctypes.byref(prob), ctypes.byref(io), st), "dgs_backward_pose_only")
                torch.cuda.synchronize()
                res[(cap < R0, mode)] = (own["viewmatrix"].cpu().numpy(), own["projmatrix"].cpu().numpy())
    assert res[(True, 1)][0].shape == (K, 4, 4)          # (the truncated call returned DGS_OK and the device is alive)
    for i in range(2):
        assert np.abs(res[(False, 1)][i]).max() > 0 and not (res[(False, 1)][i] == SENTINEL).any()
        assert np.array_equal(res[(False, 1)][i], res[(False, 2)][i]) and np.array_equal(res[(False, 1)][i], res[(False, None)][i])


# ------------------------------------------------------------------------------------------------ view loss
def _ulp32(a):
    a = np.abs(np.asarray(a, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


@pytest.mark.parametrize("kind,bound", [("identity", 0.0), ("gamma", 0.0), ("gamma", 0.125)])
def test_view_loss_kernel_against_torch_in_float64(gpu, kind, bound):
    """dgs_view_loss_grad against the torch expression of tests/test_evaluation_host.py evaluated on the device in
    float64.  Losses: within 4 x the gap between torch's own fp32 and fp64 evaluation of the case.  Gradient: the pixels
    where |tone_map(x) - gt| or the distance to a clamp bound lies strictly between 0 and one fp32 ulp of the operand
    could legitimately decide differently in fp32 -- there must be NONE on these inputs (the edge cases sit exactly on
    the bounds) -- and then every pixel takes the same decision (zero / sign pattern equal) and, for the identity, whose
    gradient is +-upstream / E or 0, the same VALUE bit for bit.

    DEVIATION from "equal" for gamma, recorded in DESIGN.md section 4: there the gradient carries the factor
    (1 / 2.2) u^(1 / 2.2 - 1), which an fp32 kernel cannot produce with the bits of torch's float64 evaluation.  Its value
    is held to the fp32 rounding of that factor instead: the exponent is rounded to fp32 (relative 2^-24 |ln u| on the
    power), powf is good to 2 ulp, three more roundings follow -- (6 + |ln u|) 2^-23 relative; with a non-zero bound u
    itself carries the roundings of (x - bound) / (1 - 2 bound) and the derivative one more division: (9 + |ln u|) 2^-23.
    Measured worst error / bar on the MI355X: 0.25 (bound 0).  bound = 0.125 is exact in fp32 and fp64 alike."""
    import torch
    from deblurgs_amd import _lib
    L = _lib.lib()
    x, gt = view_loss_case(kind)
    E = x.size
    up = 0.75
    l1_64, mse_64, g64 = view_loss_torch(x, gt, kind, torch.float64, device="cuda", upstream=up, bound=bound)
    l1_32, mse_32, _ = view_loss_torch(x, gt, kind, torch.float32, device="cuda", upstream=up, bound=bound)
    # a stack of two images, the case second: the image index comes from device memory
    gts = torch.stack([torch.zeros(3, *x.shape[1:], device="cuda"), _t(gt)]).contiguous()
    idx = torch.tensor([1], dtype=torch.int32, device="cuda")
    xs, upt = _t(x), torch.tensor([up], dtype=torch.float32, device="cuda")
    dx = torch.full_like(xs, SENTINEL)
    work = torch.full((12,), 7.0, dtype=torch.float32, device="cuda")
    ema = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tone = _lib.TONE_GAMMA if kind == "gamma" else _lib.TONE_IDENTITY
    call = lambda e, s, w=work, n_gt=2: _lib.check(
        L.dgs_view_loss_grad(xs.data_ptr(), gts.data_ptr(), idx.data_ptr(), n_gt, 3, x[0].size, tone, EPS32, bound,
                             upt.data_ptr(), dx.data_ptr(), w.data_ptr(), e, s, st), "dgs_view_loss_grad")
    call(ema.data_ptr(), skip.data_ptr())
    torch.cuda.synchronize()
    vals64 = work[8:12].cpu().numpy().view(np.float64)
    for name, got, got32, w64, w32 in (("l1", vals64[0], float(work[0]), float(l1_64), float(l1_32)),
                                       ("mse", vals64[1], float(work[1]), float(mse_64), float(mse_32))):
        bar = 4.0 * abs(w32 - w64)
        print(f"{kind} bound {bound} {name}: kernel {got!r} torch64 {w64!r} torch32 {w32!r} |diff| {abs(got - w64):.3e} bar {bar:.3e}")
        assert abs(got - w64) <= bar, (name, got, w64, bar)
        assert got32 == np.float32(got)
    assert float(ema) == np.float32(np.float32(0.5) * np.float32(0.6) + np.float32(vals64[1]) * np.float32(0.4))
    skip.fill_(1)
    call(ema.data_ptr(), skip.data_ptr())                       # an overflowed step does not count in the EMA
    torch.cuda.synchronize()
    assert float(ema) == np.float32(np.float32(0.5) * np.float32(0.6) + np.float32(vals64[1]) * np.float32(0.4))
    # an index outside the stack selects image 0 (all zeros here) instead of reading out of bounds
    work0 = torch.zeros(12, dtype=torch.float32, device="cuda")
    keep = dx.clone()
    call(None, None, w=work0, n_gt=1)
    torch.cuda.synchronize()
    y0_32, _, _ = view_loss_torch(x, np.zeros_like(gt), kind, torch.float64, device="cuda", bound=bound)
    assert abs(float(work0[0]) - float(y0_32)) <= 1e-6
    dx.copy_(keep)
    # ---- the gradient image
    x64 = x.astype(np.float64)
    u64 = (x64 - bound) / (1.0 - 2.0 * bound)
    y0 = x64 if kind == "identity" else np.maximum(u64, EPS32) ** (1 / 2.2)
    y = np.clip(y0, 0.0, 1.0)
    d = np.abs(y - gt)
    near = (d > 0) & (d < _ulp32(np.maximum(y, gt)))
    for b in (0.0, 1.0):
        near |= (np.abs(y0 - b) > 0) & (np.abs(y0 - b) < _ulp32(np.maximum(np.abs(y0), b)))
    if kind == "gamma":
        near |= (np.abs(u64 - EPS32) > 0) & (np.abs(u64 - EPS32) < _ulp32(EPS32))
    print(f"{kind} bound {bound}: pixels within one fp32 ulp of a decision: {int(near.sum())}")
    assert int(near.sum()) == 0
    g = dx.cpu().numpy().astype(np.float64)
    ref = g64.cpu().numpy()
    assert np.array_equal(g == 0.0, ref == 0.0) and np.array_equal(np.sign(g), np.sign(ref))
    if kind == "identity":
        assert np.array_equal(dx.cpu().numpy(), ref.astype(np.float32))
    else:
        tol = ((6.0 if bound == 0.0 else 9.0) + np.abs(np.log(np.maximum(u64, EPS32)))) * 2.0 ** -23 * np.abs(ref)
        worst = float((np.abs(g - ref) / np.maximum(tol, 1e-300)).max())
        print(f"gamma bound {bound}: worst gradient error / its bar {worst:.3f}")
        assert np.all(np.abs(g - ref) <= tol)
    assert np.count_nonzero(g) > 0.4 * E


@pytest.mark.parametrize("H,W", [(7, 9), (20, 24), (300, 300)])
def test_view_loss_totals_over_one_block_many_blocks_and_the_capped_grid(gpu, H, W):
    """The totals of dgs_view_loss_grad (identity tone mapping) where the number of blocks changes who converts them:
    E = 189 (one block), 1440 (six blocks: the last to arrive converts), 270000 (> 1024 * 256: capped grid, a second
    trip of the stride loop).  The fp32 words are the rounding of the fp64 words, both agree with torch in float64
    within 4 x the gap between torch's own fp32 and fp64 evaluation (the bar of the test above), and a NaN in x turns
    all four values into NaN (torch's clamp passes a NaN on; the kernel's fminf / fmaxf clamp used to drop it and report
    the loss of a zero pixel instead)."""
    import torch
    from deblurgs_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(H * 1000 + W)
    x = rng.uniform(-0.2, 1.3, (3, H, W)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    x.reshape(-1)[0:4] = [0.0, 1.0, -0.5, 2.0]                     # on the clamp bounds and far outside
    gt.reshape(-1)[10:20] = np.clip(x.reshape(-1)[10:20], 0.0, 1.0)   # equal to gt
    l1_64, mse_64, _ = view_loss_torch(x, gt, "identity", torch.float64, device="cuda")
    l1_32, mse_32, _ = view_loss_torch(x, gt, "identity", torch.float32, device="cuda")
    xs, gts = _t(x), _t(gt)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def totals():
        work = torch.full((12,), 7.0, dtype=torch.float32, device="cuda")
        _lib.check(L.dgs_view_loss_grad(xs.data_ptr(), gts.data_ptr(), None, 1, 3, H * W, _lib.TONE_IDENTITY, EPS32, 0.0,
                                        None, None, work.data_ptr(), None, None, st), "dgs_view_loss_grad")
        torch.cuda.synchronize()
        return work[:2].cpu().numpy(), work[8:12].cpu().numpy().view(np.float64)

    v32, v64 = totals()
    for name, got, got32, w64, w32 in (("l1", v64[0], v32[0], float(l1_64), float(l1_32)),
                                       ("mse", v64[1], v32[1], float(mse_64), float(mse_32))):
        bar = 4.0 * abs(w32 - w64)
        print(f"E {x.size} {name}: kernel {got!r} torch64 {w64!r} torch32 {w32!r} |diff| {abs(got - w64):.3e} bar {bar:.3e}")
        assert got32 == np.float32(got)
        assert abs(got - w64) <= bar, (name, got, w64, bar)
    xs.view(-1)[x.size // 2] = float("nan")
    v32, v64 = totals()
    assert np.isnan(v32).all() and np.isnan(v64).all(), (v32, v64)


# ------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("name", sorted(CASES))
def test_image_metrics_kernel_against_the_reference_fixture(gpu, name):
    import torch
    from deblurgs_amd import metrics
    case = CASES[name]
    a, b = _t(case["a"]), _t(case["b"])
    both = metrics.psnr_ssim(a, b)
    p, s = metrics.psnr(a, b), metrics.ssim(a, b)
    torch.cuda.synchronize()
    assert tuple(p.shape) == (3, 1) and torch.equal(p.reshape(3), both[2:5]) and torch.equal(s, both[1])
    check_metrics(case, float(p.mean().item()), float(s.item()), "gpu " + name)
    check_metrics(case, float(both[0].item()), float(both[1].item()), "gpu (kernel's own channel mean) " + name)
    assert torch.equal(metrics.psnr_ssim(a, b), both)          # deterministic


# ------------------------------------------------------------------------------------------------ the fit
class _NoHostSync:
    """Inside the block every way torch offers to wait for the device raises: torch's own sync debug mode turns the
    implicit ones (.item(), .cpu(), a pageable copy) into errors, the explicit ones are patched."""

    def __enter__(self):
        import torch
        self.saved = [(torch.cuda, "synchronize", torch.cuda.synchronize),
                      (torch.cuda.Stream, "synchronize", torch.cuda.Stream.synchronize),
                      (torch.cuda.Event, "synchronize", torch.cuda.Event.synchronize)]

        def refuse(*a, **k):
            raise AssertionError("host synchronisation inside the fused fit loop")
        for obj, name, _ in self.saved:
            setattr(obj, name, refuse)
        self.mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        return self

    def __exit__(self, *exc):
        import torch
        torch.cuda.set_sync_debug_mode(self.mode)
        for obj, name, fn in self.saved:
            setattr(obj, name, fn)
        return False


def _fit_fixture(P=3000, W=144, H=96, seed=3, move=None):
    """A product cloud, three test views whose ground truth is the product's own render (gamma tone mapping) at known
    poses, and start poses off by a fixed rotation (0.4 degrees about a fixed axis) and translation.  move: a map from
    the scene to the scene the fixture is built on (tests/test_gpu_posed.py: the same cloud and views at a general pose)."""
    import torch
    from scipy.spatial.transform import Rotation
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses
    from deblurgs_amd.cloud import GaussianCloud
    torch.manual_seed(seed)
    sc = synthetic.make_scene(P, W, H, K=3, seed=seed, sigma_px=2.5)
    if move is not None:
        sc = move(sc)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:3].astype(np.float64)
    true_cams = [ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(3)]
    truth = ev.TestPoseModel(true_cams, device="cuda")
    with torch.no_grad():
        gts = torch.stack([tm(gaussian_renderer.render(truth(i), cloud, bg)["render"]).clamp(0.0, 1.0) for i in range(3)])
    dR = Rotation.from_rotvec(np.deg2rad(0.4) * np.array([0.6, -0.64, 0.48])).as_matrix()
    dT = np.array([0.03, -0.02, 0.04])
    start = [ev.TestCamera(V[i][:3, :3] @ dR, V[i][3, :3] + dT, sc["FoVx"], sc["FoVy"], W, H) for i in range(3)]
    return cloud, start, gts, bg, tm, truth


def _pose_error(model, truth, cloud):
    """How far the fitted cameras put the scene from where the true cameras put it: the mean distance between the cloud's
    points in the view space of the fitted and of the true pose, over the views.  (Rotation and translation errors taken
    one by one are no measure of a fit's progress: a small rotation of the camera and a sideways translation move the
    image almost alike, so a fit first trades one against the other -- the autograd fit does exactly the same.)"""
    import torch
    with torch.no_grad():
        x = torch.cat([cloud._xyz, torch.ones_like(cloud._xyz[:, :1])], dim=1)
        return float(np.mean([float(((x @ model(i).world_view_transform)[:, :3] -
                                     (x @ truth(i).world_view_transform)[:, :3]).norm(dim=1).mean())
                              for i in range(len(truth))]))


def test_fused_pose_fit_first_step_gradients_match_autograd(gpu):
    """dL/dq and dL/dt of the fused path against render() + losses + torch.autograd + the torch pose chain."""
    _check_first_step_gradients(_fit_fixture())


def _check_first_step_gradients(fixture):
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer
    cloud, start, gts, bg, tm, _ = fixture
    fit = ev.FusedPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=60)
    ref = ev.TestPoseModel(start, device="cuda")
    errs = []
    for idx in range(3):
        g_rot, g_trans, vals = fit.gradients(idx)
        for p in ref.parameters():
            p.grad = None
        image = gaussian_renderer.render(ref(idx), cloud, bg)["render"]
        l1, mse = ev.view_loss(image, gts[idx], tm)
        l1.backward()
        torch.cuda.synchronize()
        for name, a, b in (("dL/dq", g_rot, ref._rot.grad), ("dL/dt", g_trans, ref._trans.grad)):
            e = relerr(a.cpu().numpy(), b.cpu().numpy())
            print(f"view {idx} {name}: rel err {e:.3e}")
            errs.append(e)
            assert e <= GRAD_TOL, (idx, name, e)
            assert float(a[[i for i in range(3) if i != idx]].abs().max()) == 0.0      # the dense gradient's other rows
        assert abs(float(vals[0]) - float(l1)) <= 1e-6 and abs(float(vals[1]) - float(mse)) <= 1e-6
    return errs


def test_fused_pose_fit_against_the_autograd_fit(gpu):
    """S = 60 epochs of both fits from the same start, the same fixed view order, num_iter_per_view = S so that StepLR
    fires every 3 epochs.  The fused fit's final mean L1 must be no worse than what the autograd fit had reached after
    0.9 S epochs: the fused step costs at most a tenth of the iterations.  Both end closer to the true poses than they
    started, and the fused loop never synchronises with the host."""
    import torch
    from deblurgs_amd import evaluation as ev
    S, n = 60, 3
    cloud, start, gts, bg, tm, truth = _fit_fixture()
    orders = ev.epoch_orders(n, S, order=[2, 0, 1])
    # ---- the autograd fit (the path a user had before: render(), autograd, torch.optim.Adam)
    from autograd_pose_fit import AutogradPoseFit
    auto = AutogradPoseFit(cloud, start, list(gts), bg, tm, num_iter_per_view=S)
    err0 = _pose_error(auto.model, truth, cloud)
    curve_a = []
    for order in orders:
        curve_a.append(float(np.mean([float(auto.step(i)) for i in order])))
        auto.scheduler.step()
    err_a = _pose_error(auto.model, truth, cloud)
    for p in cloud.parameters():
        p.grad = None
    # ---- the fused fit
    fit = ev.FusedPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=S)
    steps = fit.schedule(orders)
    assert steps == S * n
    curve_dev = torch.zeros(steps, device="cuda")
    torch.cuda.synchronize()
    with _NoHostSync():
        for i in range(steps):
            fit.run(1)
            curve_dev[i:i + 1].copy_(fit.work[:1], non_blocking=True)
    torch.cuda.synchronize()
    assert fit.dropped() == 0 and fit.steps == steps
    curve_f = curve_dev.cpu().numpy().reshape(S, n).mean(axis=1)
    err_f = _pose_error(fit.model, truth, cloud)
    at = int(round(0.9 * S)) - 1                   # the autograd fit's epoch 0.9 S (1-based)
    msg = (f"fused final {curve_f[-1]:.6e} vs autograd after {at + 1} epochs {curve_a[at]:.6e} (autograd final "
           f"{curve_a[-1]:.6e}); pose error (mean view-space displacement) start {err0} autograd {err_a} fused {err_f}\n"
           f"autograd curve {np.array2string(np.array(curve_a), precision=5)}\nfused curve {np.array2string(curve_f, precision=5)}")
    print(msg)
    assert curve_f[-1] <= curve_a[at], msg
    assert err_a < err0 and err_f < err0, msg
    assert 0.0 < fit.psnr_ema() < 100.0
    # Adam's moments of ALL rows moved every step (dense Adam), and the schedule's last rates are the 20th stage's
    assert float(fit.exp_avg_sq[0].abs().min()) > 0.0
    assert ev.step_lrs(S, S)[-1][0] == pytest.approx(ev.ROT_LR * 0.9 ** 19, rel=1e-12)


def test_evaluate_returns_the_metrics_of_the_renders(gpu):
    """evaluate() on fitted cameras: the PSNR and SSIM that metrics.* give on render()'s images, bit for bit."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer, metrics
    cloud, start, gts, bg, tm, truth = _fit_fixture()
    cams = ev.optimize_test_pose(cloud, start, gts, bg, tm, num_iter_per_view=20, order=[0, 1, 2])
    assert len(cams) == 3 and not cams[0].world_view_transform.requires_grad
    psnr, ssim = ev.evaluate(cams, cloud, bg, gts, tm)
    want_p, want_s = 0.0, 0.0
    with torch.no_grad():
        for cam, gt in zip(cams, gts):
            image = tm(gaussian_renderer.render(cam, cloud, bg)["render"])
            want_p += metrics.psnr(image, gt).mean().item()
            want_s += metrics.ssim(image, gt).mean().item()
    assert psnr == want_p / 3 and ssim == want_s / 3
    assert 10.0 < psnr < 80.0 and 0.3 < ssim <= 1.0
    # the start poses score worse than the fitted ones
    with torch.no_grad():
        m0 = ev.TestPoseModel(start, device="cuda")
        p0, s0 = ev.evaluate([m0(i) for i in range(3)], cloud, bg, gts, tm)
    print(f"evaluate: fitted {psnr:.3f} dB / {ssim:.5f}, start poses {p0:.3f} dB / {s0:.5f}")
    assert psnr > p0

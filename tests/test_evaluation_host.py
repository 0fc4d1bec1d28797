"""CPU tests of the evaluation protocol (deblurgs_amd.evaluation / deblurgs_amd.metrics; test.py:39-186 of the
reference): the metrics against the reference's own functions (tests/golden/metrics_golden.npz, written by
tests/golden/make_golden_metrics.py), the pose chain of TestPoseModel against scipy and float64 torch, the fit's loss as
a torch expression (the yardstick tests/test_gpu_evaluation.py holds dgs_view_loss_grad to), the schedule helpers, and
the argument checks of the ABI 15 entry points, which run before any HIP call."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics_golden.npz")

# The reference prints SSIM with .3f and PSNR with .2f (test.py:429-439); a hundredth of that resolution cannot change a
# reported figure.
SSIM_FLOOR, PSNR_FLOOR = 1e-5, 1e-4
REF_NOISE_MULT = 4.0          # x |reference fp32 - reference fp64|: the reference's own rounding noise (helpers.POSE_NOISE_MULT)
EPS32 = float(np.float32(1e-8))   # ToneMapping's eps as fp32 arithmetic sees it: the same number in the fp32 and fp64 runs


def golden_cases():
    z = np.load(GOLDEN)
    for name in [str(n) for n in z["names"]]:
        yield name, dict(a=z[name + "_a"].astype(np.float32), b=z[name + "_b"].astype(np.float32),
                         psnr32=float(z[name + "_psnr32"]), psnr64=float(z[name + "_psnr64"]),
                         ssim32=float(z[name + "_ssim32"]), ssim64=float(z[name + "_ssim64"]))


def metric_bars(case):
    """(psnr bar, ssim bar) of a fixture case: 4 x the reference's fp32-to-fp64 gap, floored at a hundredth of the
    resolution the reference prints the metric at."""
    gp = abs(case["psnr32"] - case["psnr64"]) if np.isfinite(case["psnr64"]) else 0.0
    return (max(REF_NOISE_MULT * gp, PSNR_FLOOR), max(REF_NOISE_MULT * abs(case["ssim32"] - case["ssim64"]), SSIM_FLOOR))


def check_metrics(case, psnr, ssim, what):
    """psnr / ssim: python floats computed by the code under test; compared with the reference's fp64 values."""
    bar_p, bar_s = metric_bars(case)
    print(f"{what}: psnr {psnr!r} ref64 {case['psnr64']!r} bar {bar_p:.2e} | ssim {ssim!r} ref64 {case['ssim64']!r} bar {bar_s:.2e}")
    if np.isinf(case["psnr64"]):
        assert psnr == float("inf") and ssim == 1.0, what
        return
    assert abs(psnr - case["psnr64"]) <= bar_p, (what, psnr, case["psnr64"], bar_p)
    assert abs(ssim - case["ssim64"]) <= bar_s, (what, ssim, case["ssim64"], bar_s)


CASES = dict(golden_cases()) if os.path.exists(GOLDEN) else {}


def test_fixture_covers_the_cases_the_metrics_are_pinned_on():
    assert len(CASES) >= 8
    shapes = {n: c["a"].shape for n, c in CASES.items()}
    assert all(s[0] == 3 and s[1] <= 96 and s[2] <= 128 for s in shapes.values())
    assert shapes["odd_size"] == (3, 37, 53)
    assert np.array_equal(CASES["identical"]["a"], CASES["identical"]["b"])
    oor = CASES["out_of_range"]
    assert oor["a"].min() < 0.0 and oor["a"].max() > 1.0
    assert os.path.getsize(GOLDEN) < 200 * 1024


@pytest.mark.parametrize("name", sorted(CASES))
def test_metrics_on_cpu_match_the_reference(name):
    from deblurgs_amd import metrics
    case = CASES[name]
    a, b = torch.from_numpy(case["a"]), torch.from_numpy(case["b"])
    p = metrics.psnr(a, b)
    assert tuple(p.shape) == (3, 1)
    check_metrics(case, float(p.mean().item()), float(metrics.ssim(a, b).mean().item()), "cpu " + name)


def test_identical_images_give_ssim_one_and_infinite_psnr():
    from deblurgs_amd import metrics
    a = torch.from_numpy(CASES["identical"]["a"])
    assert float(metrics.ssim(a, a.clone())) == 1.0
    assert bool(torch.isinf(metrics.psnr(a, a.clone())).all())
    per_channel = metrics.ssim(a[None], a[None].clone(), size_average=False)      # the reference's batched form
    assert tuple(per_channel.shape) == (1,) and float(per_channel[0]) == 1.0


# ------------------------------------------------------------------------------------------------ pose chain
def _cams(n=4, seed=3, W=64, H=48):
    from scipy.spatial.transform import Rotation
    from deblurgs_amd.evaluation import TestCamera
    rng = np.random.default_rng(seed)
    Rs = Rotation.random(n, random_state=seed).as_matrix()
    return [TestCamera(Rs[i], rng.normal(0, 2.0, 3), 0.9, 0.7, W, H) for i in range(n)], Rs


def test_pose_model_forward_against_scipy_and_float64():
    """The rotation against scipy.spatial.transform.Rotation (roma, which the reference calls, is not installed: parity
    unpinned against roma, as for pose.py's conversions), camera_center and full_proj against their torch definitions
    (test.py:87-89) in float64."""
    from scipy.spatial.transform import Rotation
    from deblurgs_amd import pose
    from deblurgs_amd.evaluation import TestPoseModel
    cams, Rs = _cams()
    m = TestPoseModel(cams, device="cpu")
    assert tuple(m._rot.shape) == (4, 4) and tuple(m._trans.shape) == (4, 3) and m._rot.dtype == torch.float32
    q_ref = Rotation.from_matrix(Rs).as_quat()                         # (x, y, z, w)
    q = m._rot.detach().double().numpy()
    sign = np.sign((q * q_ref).sum(axis=1, keepdims=True))
    assert np.abs(q * sign - q_ref).max() <= 2e-7                      # fp32 storage of unit quaternions
    with torch.no_grad():
        m._rot.mul_(1.7)                                               # the chain normalises: the scale must not matter
    for i, c in enumerate(cams):
        cam = m(i)
        wv = cam.world_view_transform.detach().double()
        # fp32 chain: ~8 roundings of O(1) products per rotation entry
        R_ref = Rotation.from_quat(m._rot[i].detach().double().numpy() + 1e-8).as_matrix()
        assert np.abs(wv[:3, :3].numpy() - R_ref).max() <= 2e-6
        assert np.abs(wv[:3, :3].numpy() - Rs[i]).max() <= 2e-6
        assert torch.equal(wv[3, :3].float(), m._trans[i].detach()) and torch.equal(wv[:, 3], torch.tensor([0, 0, 0, 1.0]).double())
        wv64 = torch.eye(4, dtype=torch.float64)
        wv64[:3, :3] = torch.from_numpy(R_ref)
        wv64[3, :3] = m._trans[i].detach().double()
        proj64 = pose.get_projection_matrix(c.znear, c.zfar, c.FoVx, c.FoVy).transpose(0, 1).double()
        full64 = wv64 @ proj64
        center64 = torch.inverse(wv64)[3, :3]
        scale = float(full64.abs().max())
        assert float((cam.full_proj_transform.detach().double() - full64).abs().max()) <= 4e-6 * scale
        assert float((cam.camera_center.detach().double() - center64).abs().max()) <= 4e-6 * float(center64.abs().max())
        assert cam.image_width == 64 and cam.image_height == 48 and cam.FoVx == 0.9
    # gradients reach both parameters through the camera
    cam = m(2)
    (cam.world_view_transform.sum() + cam.full_proj_transform.sum()).backward()
    assert float(m._rot.grad[2].abs().max()) > 0 and float(m._trans.grad[2].abs().max()) > 0
    assert float(m._rot.grad[[0, 1, 3]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the fit's loss
def view_loss_case(kind, seed=0, H=60, W=80):
    """Seeded inputs of the view loss with the edge cases placed exactly: pixels below eps, outside [0, 1] after tone
    mapping, exactly on the clamp bounds and exactly equal to gt.  Returns (x, gt) as float32 numpy [3,H,W]."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.3, (3, H, W)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    f, g = x.reshape(-1), gt.reshape(-1)
    f[0:8] = [0.0, 1.0, EPS32, EPS32 / 2, -0.5, 2.0, 1.0, 0.0]      # on the bounds, at and below eps, far outside
    g[6], g[7] = 1.0, 0.0                                          # ... and equal to gt on a bound
    g[1] = 0.25
    f[100:140] = 1.0 + rng.uniform(0.0, 0.5, 40).astype(np.float32)   # clamped to 1 ...
    g[100:120] = 1.0                                                  # ... where gt is 1 as well: sign(0) = 0
    if kind == "identity":
        g[200:260] = np.clip(f[200:260], 0.0, 1.0)                    # equal to gt inside the range (identity is exact)
        f[300:310] = -rng.uniform(0.0, 0.2, 10).astype(np.float32)    # below 0: clamped, no gradient
    return x, gt


def view_loss_torch(x, gt, kind, dtype, device="cpu", eps=EPS32, bound=0.0, upstream=1.0):
    """The loss of test.py:171-178 for one image as a torch expression, with autograd's gradient: (l1, mse, dL/dx)."""
    from deblurgs_amd import losses
    from deblurgs_amd.evaluation import view_loss
    xt = torch.as_tensor(x, device=device).to(dtype).requires_grad_(True)
    gtt = torch.as_tensor(gt, device=device).to(dtype)
    l1, mse = view_loss(xt, gtt, losses.ToneMapping(kind, eps=eps, bound=bound))
    (l1 * upstream).backward()
    return l1.detach(), mse.detach(), xt.grad.detach()


@pytest.mark.parametrize("kind", ["identity", "gamma"])
def test_view_loss_torch_expression_and_its_conventions(kind):
    x, gt = view_loss_case(kind)
    E = x.size
    l1, mse, g = view_loss_torch(x, gt, kind, torch.float64)
    g = g.reshape(-1).numpy()
    y = np.clip(x.astype(np.float64) if kind == "identity" else np.maximum(x.astype(np.float64), EPS32) ** (1 / 2.2), 0, 1)
    assert abs(float(l1) - np.abs(y - gt).mean()) <= 1e-14 and abs(float(mse) - ((y - gt) ** 2).mean()) <= 1e-14
    assert g[5] == 0.0 and g[6] == 0.0 and g[7] == 0.0            # outside the clamp; equal to gt: sign(0) = 0
    assert np.all(g[100:120] == 0.0) and np.all(g[120:140] == 0.0)
    if kind == "identity":
        assert g[0] == -1.0 / E and g[1] == 1.0 / E               # ON the clamp bounds: the gradient passes
        assert g[4] == 0.0 and np.all(g[200:260] == 0.0) and np.all(g[300:310] == 0.0)
        inside = (x.reshape(-1) > 0) & (x.reshape(-1) < 1) & (y.reshape(-1) != gt.reshape(-1))
        assert np.all(np.abs(g[inside]) == 1.0 / E)
    else:
        assert g[2] != 0.0                                        # AT eps: clamp_min passes the gradient
        assert g[3] == 0.0 and g[4] == 0.0 and g[0] == 0.0        # below eps
        assert g[1] == (1 / 2.2) / E                              # x = 1: (1 / 2.2) 1^(1 / 2.2 - 1) on the upper bound
    # fp32 evaluation of the same expression: what the GPU test calibrates its loss bar with
    l1_32, mse_32, _ = view_loss_torch(x, gt, kind, torch.float32)
    assert abs(float(l1_32) - float(l1)) <= 1e-6 and abs(float(mse_32) - float(mse)) <= 1e-6


# ------------------------------------------------------------------------------------------------ schedule helpers
def test_step_lrs_follow_torch_steplr():
    from deblurgs_amd.evaluation import ROT_LR, TRANS_LR, step_lrs
    for num_iter, epochs in ((60, 60), (2000, 230), (7, 9)):
        p = [torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))]
        opt = torch.optim.Adam([{"params": [p[0]], "lr": ROT_LR}, {"params": [p[1]], "lr": TRANS_LR}], lr=5e-4, eps=1e-15)
        sch = torch.optim.lr_scheduler.StepLR(opt, step_size=max(num_iter // 20, 1), gamma=0.9)
        got = step_lrs(epochs, num_iter)
        for e in range(epochs):
            want = (opt.param_groups[0]["lr"], opt.param_groups[1]["lr"])
            assert got[e] == pytest.approx(want, rel=1e-12), (num_iter, e)
            opt.step()
            sch.step()
    assert got[0] == (ROT_LR, TRANS_LR)


def test_epoch_orders_shuffle_like_the_reference_and_accept_a_fixed_order():
    from deblurgs_amd.evaluation import epoch_orders
    rng = random.Random(11)
    want = []
    for _ in range(3):
        idx = list(range(5))
        rng.shuffle(idx)
        order = []
        while idx:
            order.append(idx.pop())           # test.py:163-165
        want.append(order)
    assert epoch_orders(5, 3, seed=11) == want
    assert epoch_orders(3, 2, order=[2, 0, 1]) == [[2, 0, 1], [2, 0, 1]]
    assert epoch_orders(3, 2, order=[[2, 0, 1], [0, 1, 2]]) == [[2, 0, 1], [0, 1, 2]]
    with pytest.raises(ValueError):
        epoch_orders(3, 2, order=[0, 1])


# ------------------------------------------------------------------------------------------------ ABI 15
NEW_SYMBOLS = ["dgs_backward_pose_only", "dgs_view_loss_grad", "dgs_image_metrics", "dgs_testpose_forward",
               "dgs_testpose_backward"]


def test_abi_15_and_its_new_symbols():
    from deblurgs_amd import _lib
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", text).group(1)) == 15 == _lib.ABI_VERSION
    L = _lib.lib()
    assert L.dgs_abi_version() == 15
    for s in NEW_SYMBOLS + ["dgs_image_metrics_tmp_bytes"]:
        assert hasattr(L, s) and s in _lib.EXPORTS, s
    assert L.dgs_image_metrics_tmp_bytes(1920, 1080) == 3 * 120 * 68 * 16
    # metrics.hip is part of the build (and so of the build id)
    from deblurgs_amd import build
    assert "metrics.hip" in build.SOURCES


def _valid_problem(addr):
    from deblurgs_amd import _lib
    p = _lib.DgsProblem()
    p.P, p.W, p.H, p.K, p.D, p.M = 10, 64, 64, 1, 2, 9
    for f in ("means3D", "shs", "scales", "rotations", "viewmatrix", "projmatrix", "campos", "bg"):
        setattr(p, f, addr)
    return p


def test_pose_only_backward_refuses_bad_problems_before_touching_hip():
    from deblurgs_amd import _lib
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(256)
    addr = ctypes.cast(dummy, ctypes.c_void_p)
    io = _lib.DgsBackwardIO()
    io.dL_dviewmatrix = io.dL_dprojmatrix = addr
    p = _valid_problem(addr)
    p.forward_only = 1
    assert L.dgs_backward_pose_only(ctypes.byref(p), ctypes.byref(io), None) == -1
    assert b"forward_only" in L.dgs_last_error()
    p.forward_only = 0
    io.dL_dviewmatrix = None
    assert L.dgs_backward_pose_only(ctypes.byref(p), ctypes.byref(io), None) == -1
    assert b"dL_dviewmatrix" in L.dgs_last_error()
    io.dL_dviewmatrix, io.dL_dprojmatrix = addr, None
    assert L.dgs_backward_pose_only(ctypes.byref(p), ctypes.byref(io), None) == -1
    assert L.dgs_backward_pose_only(ctypes.byref(p), None, None) == -1
    assert L.dgs_backward_pose_only(None, ctypes.byref(io), None) == -1
    # the other gradient pointers are NOT required: with both pose outputs the next complaint is about the inputs
    io.dL_dprojmatrix = addr
    assert L.dgs_backward_pose_only(ctypes.byref(p), ctypes.byref(io), None) == -1
    assert b"dL_dout_color" in L.dgs_last_error()
    io.dL_dout_color = io.radii = addr
    assert L.dgs_backward_pose_only(ctypes.byref(p), ctypes.byref(io), None) == -2     # DGS_E_CAPACITY: no state blobs
    p.K = 0
    assert L.dgs_backward_pose_only(ctypes.byref(p), ctypes.byref(io), None) == -1


def test_evaluation_entry_points_check_their_arguments_without_a_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(256)
    a = ctypes.cast(dummy, ctypes.c_void_p)
    assert L.dgs_view_loss_grad(None, a, None, 1, 3, 16, 0, 1e-8, 0.0, None, a, a, None, None, None) == -1
    assert L.dgs_view_loss_grad(a, a, None, 1, 3, 16, 0, 1e-8, 0.0, None, None, None, None, None, None) == -1   # no output
    assert L.dgs_view_loss_grad(a, a, None, 1, 3, 16, 7, 1e-8, 0.0, None, a, a, None, None, None) == -1
    assert b"tone_mapping" in L.dgs_last_error()
    assert L.dgs_view_loss_grad(a, a, None, 1, 3, 16, 1, 1e-8, 0.5, None, a, a, None, None, None) == -1
    assert L.dgs_view_loss_grad(a, a, None, 1, 3, 16, 0, 1e-8, 0.0, None, a, None, a, None, None) == -1         # ema, no work
    assert L.dgs_view_loss_grad(a, a, None, 0, 3, 16, 0, 1e-8, 0.0, None, a, a, None, None, None) == -1         # n_gt = 0
    assert L.dgs_image_metrics(a, None, 8, 8, a, a, None) == -1
    assert L.dgs_image_metrics(a, a, 0, 8, a, a, None) == -1
    assert L.dgs_testpose_forward(a, a, None, 3, 3, a, a, a, a, None) == -1                                  # idx out of range
    assert L.dgs_testpose_forward(a, None, None, 0, 3, a, a, a, a, None) == -1
    assert L.dgs_testpose_backward(a, a, None, 0, 0, a, a, a, a, a, None) == -1                              # n = 0
    assert L.dgs_testpose_backward(a, a, None, 0, 3, a, a, None, a, a, None) == -1


def test_fused_fit_refuses_what_it_does_not_implement():
    from deblurgs_amd import evaluation, losses
    with pytest.raises(NotImplementedError, match="tone mapping"):
        evaluation._tone_args(losses.ToneMapping("reverse_gamma"))
    assert evaluation._tone_args("gamma")[1:] == (1, 1e-8, 0.0)
    assert evaluation._tone_args(None)[1] == 0
    from deblurgs_amd import metrics
    with pytest.raises(RuntimeError, match="float32"):
        metrics.psnr_ssim(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8))      # the fused kernel itself takes device images only
    # what the reference's signatures accept beyond [3,H,W]: a batch, one channel, size_average=False
    a, b = torch.rand(2, 1, 16, 20), torch.rand(2, 1, 16, 20)
    assert tuple(metrics.ssim(a, b, size_average=False).shape) == (2,) and tuple(metrics.psnr(a, b).shape) == (2, 1)

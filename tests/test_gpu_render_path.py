"""GPU tests of camera-path rendering: the three kernels of csrc/frames.hip against numpy / torch (in fp32 where the
expression is exact, in float64 under a band rule where a powf or a division sits between), get_middle_cams, render_frames
against per-camera render() + dgs_frames_finish bit for bit, evaluate(views_per_call=...) and render_spiral.

The band rule: a value whose float64 result v (255 y for a frame, 256 d for a depth colour) lies within 1e-3 of an integer,
with y (d) strictly inside (0, 1), may come out one level off -- the fp32 chain (a correctly rounded division, a powf a few
ulp wide; at most ~1e-4 of a level) can land on the other side of the truncation there; every other value must be equal.
Values the clip pins to 0 or 1 are exact and are NOT in the band."""
import numpy as np
import pytest

from helpers import synthetic

pytestmark = pytest.mark.gpu

GUARD = 64
BAND = 1e-3


def _frames_input(K, H, W, seed):
    """uniform in [-0.15, 1.15] with sprinkled exact 0, 1, k/255, +-inf and NaN; returns (x fp32 numpy, NaN mask)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.15, 1.15, (K, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    m = max(n // 12, 6)
    pos = rng.permutation(n)[:6 * m].reshape(6, -1) if n >= 6 * m else rng.integers(0, n, (6, m))
    flat[pos[0]] = 0.0
    flat[pos[1]] = 1.0
    flat[pos[2]] = (rng.integers(0, 256, pos[2].size) / 255.0).astype(np.float32)
    flat[pos[3][: max(m // 4, 1)]] = np.inf
    flat[pos[4][: max(m // 4, 1)]] = -np.inf
    flat[pos[5][: max(m // 4, 1)]] = np.nan
    return x, np.isnan(x)


def _windows(H, W):
    from deblurgs_amd import render_path as rp
    odd = (H // 2, H // 2 + max(H // 3, 1), 1 if W > 1 else 0, (1 if W > 1 else 0) + 1)      # odd x0, w = 1
    return {"full": (0, H, 0, W), "r095": rp.center_crop_window(H, W, 0.95), "r05": rp.center_crop_window(H, W, 0.5), "odd": odd}


def _finish_guarded(x, tone_mapping, window, shift=0):
    """dgs_frames_finish into the middle of one allocation filled with 0xA5; returns the frames and checks both guards."""
    import torch
    from deblurgs_amd import render_path as rp
    K = x.shape[0]
    h, w = window[1] - window[0], window[3] - window[2]
    nbytes = K * h * w * 3
    buf = torch.full((GUARD + shift + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + shift: GUARD + shift + nbytes]
    rp.frames_finish(x, tone_mapping, window, out=out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD + shift] == 0xA5).all() and (host[GUARD + shift + nbytes:] == 0xA5).all(), "guard zone overwritten"
    assert host[GUARD + shift + nbytes:].size == GUARD
    return host[GUARD + shift: GUARD + shift + nbytes].reshape(K, h, w, 3)


def _crop_nhwc(a, window):
    h1, h2, w1, w2 = window
    return np.ascontiguousarray(a[:, :, h1:h2, w1:w2].transpose(0, 2, 3, 1))


@pytest.mark.parametrize("K,H,W", [(1, 5, 7), (3, 37, 53), (2, 64, 128)])
def test_frames_finish_identity_equals_numpy(gpu, K, H, W):
    """Every window; the output equals numpy's clip * 255 -> astype(uint8) of the fp32 values, NaN gives 0, and nothing
    outside the K h w 3 bytes is written -- with the destination 4-byte aligned and not."""
    import torch
    x, nan = _frames_input(K, H, W, seed=K * 1000 + W)
    xt = torch.from_numpy(x).cuda()
    for name, win in _windows(H, W).items():
        h, w = win[1] - win[0], win[3] - win[2]
        assert h >= 1 and w >= 1, (name, win)
        sub, sub_nan = _crop_nhwc(x, win), _crop_nhwc(nan, win)
        with np.errstate(invalid="ignore"):
            want = (np.where(sub_nan, np.float32(0.0), sub).clip(0.0, 1.0) * 255.0).astype(np.uint8)
        for shift in (0, 1):
            got = _finish_guarded(xt, None, win, shift)
            assert got.shape == (K, h, w, 3)
            assert (got[sub_nan] == 0).all(), (name, shift)
            bad = (got != want) & ~sub_nan
            assert not bad.any(), (name, win, shift, int(bad.sum()), sub[bad][:5], got[bad][:5], want[bad][:5])
    assert nan.any() and np.isinf(x).any()


def _band_compare(got, v64, inside, what):
    """got: integer levels; v64: the float64 value whose floor is expected (already clipped to its range); inside: where
    the unclipped quantity lies strictly inside (0, 1).  Returns the in-band share."""
    want = np.floor(v64).astype(np.int64)
    band = inside & (np.abs(v64 - np.rint(v64)) < BAND)
    diff = got.astype(np.int64) - want
    outside_bad = (diff != 0) & ~band
    share = float(band.mean())
    print(f"{what}: {band.sum()} of {band.size} values in the band ({100 * share:.3f} %), {int((diff != 0).sum())} differ, "
          f"{int(outside_bad.sum())} of them outside the band")
    assert not outside_bad.any(), (what, v64[outside_bad][:5], got[outside_bad][:5])
    assert (np.abs(diff[band]) <= 1).all(), what
    assert share <= 0.01, (what, share)
    return share


def _gamma64(x32, eps, bound):
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x32.astype(np.float64) - bound) / (1.0 - 2.0 * bound)
        return np.maximum(u, eps) ** (1.0 / 2.2)


@pytest.mark.parametrize("bound", [0.0, 0.05])
@pytest.mark.parametrize("K,H,W", [(1, 5, 7), (3, 37, 53), (2, 64, 128)])
def test_frames_finish_gamma_against_float64(gpu, K, H, W, bound):
    import torch
    from deblurgs_amd import losses
    tm = losses.ToneMapping("gamma", bound=bound)
    x, nan = _frames_input(K, H, W, seed=K * 2000 + W)
    xt = torch.from_numpy(x).cuda()
    shares = []
    for name, win in _windows(H, W).items():
        sub, sub_nan = _crop_nhwc(x, win), _crop_nhwc(nan, win)
        got = _finish_guarded(xt, tm, win, shift=0)
        assert (got[sub_nan] == 0).all(), name
        ok = ~sub_nan
        y = _gamma64(sub[ok], tm.eps, bound)
        shares.append(_band_compare(got[ok], 255.0 * np.clip(y, 0.0, 1.0), (y > 0.0) & (y < 1.0),
                                    f"gamma bound {bound} {K}x{H}x{W} {name}"))
    assert len(shares) == 4


@pytest.mark.parametrize("n", [1, 63, 257, 70_001])
def test_depth_range_and_colorize(gpu, n):
    """The two words equal torch.min / torch.max (a block, part of a block, more than one block, the grid-stride loop); the
    colours equal the table at the float64 index under the band rule -- with the range the data's own and with z_near /
    z_far cutting into it; a constant image gives the map's bad colour everywhere."""
    import torch
    from deblurgs_amd import render_path as rp
    rng = np.random.default_rng(n)
    d = rng.uniform(0.5, 30.0, n).astype(np.float32)
    dt = torch.from_numpy(d).cuda()
    lo_hi = rp.depth_range(dt)
    assert lo_hi.dtype == torch.float32 and tuple(lo_hi.shape) == (2,)
    assert float(lo_hi[0]) == float(torch.min(dt)) == float(d.min()) and float(lo_hi[1]) == float(torch.max(dt)) == float(d.max())
    lut = rp.jet_r_table().astype(np.int64)
    for z_near, z_far in ((0.2, 100.0), (2.0, 20.0)):
        got = rp.depth_colorize(dt, z_near, z_far).cpu().numpy()
        assert got.shape == (n, 4) and got.dtype == np.uint8
        lo = max(np.float32(z_near), d.min()).astype(np.float64)
        hi = min(np.float32(z_far), d.max()).astype(np.float64)
        if hi == lo:
            assert n == 1 and (got == 0).all()
            continue
        raw = (d.astype(np.float64) - lo) / (hi - lo)
        v = 256.0 * np.clip(raw, 0.0, 1.0)
        idx = np.minimum(np.floor(v).astype(np.int64), 255)
        band = (raw > 0.0) & (raw < 1.0) & (np.abs(v - np.rint(v)) < BAND)
        exact = (got == lut[idx]).all(axis=1)
        near = exact | (got == lut[np.clip(idx - 1, 0, 255)]).all(axis=1) | (got == lut[np.clip(idx + 1, 0, 255)]).all(axis=1)
        print(f"n {n} range ({z_near}, {z_far}): {band.sum()} in the band, {int((~exact).sum())} differ")
        assert (exact | band).all(), (d[~(exact | band)][:5], got[~(exact | band)][:5])
        assert near.all() and band.mean() <= 0.01 + 1.0 / n
    # NaNs do not count in the range and get the bad colour
    if n >= 63:
        with_nan = d.copy()
        with_nan[::7] = np.nan
        t = torch.from_numpy(with_nan).cuda()
        r = rp.depth_range(t).cpu().numpy()
        assert r[0] == np.nanmin(with_nan) and r[1] == np.nanmax(with_nan)
        c = rp.depth_colorize(t, 0.2, 100.0).cpu().numpy()
        assert (c[::7] == 0).all() and (c[1::7, 3] == 255).all()
        const = torch.full((n,), 3.25, device="cuda")
        assert (rp.depth_colorize(const, 0.2, 100.0).cpu().numpy() == 0).all()


def test_get_middle_cams_equals_the_trajectory_at_the_middle_nu(gpu):
    import torch
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    torch.manual_seed(4)
    ref = RefCamera(144, 96, 1.0, 0.7, device="cuda")
    for curve_type, f in (("se3", 7), ("quarternion_cartesian", 6)):
        kw = dict(init_se3=torch.randn(3, 6) * 0.05) if curve_type == "se3" else {}
        m = CameraMotionModule(ref, torch.rand(3, 3, 96, 144, device="cuda"), curve_order=4, num_subframes=f, device="cuda",
                               curve_type=curve_type, **kw)
        with torch.no_grad():
            m._nu.add_(torch.randn_like(m._nu) * 0.3)
        cams = m.get_middle_cams()
        assert len(cams) == 3
        for i, cam in enumerate(cams):
            nu = m._sample_nu_from_alignment(i)
            want = m.get_trajectory(i, nu[f // 2: f // 2 + 1])[0]
            for a, b in ((cam.world_view_transform, want.world_view_transform), (cam.full_proj_transform, want.full_proj_transform),
                         (cam.camera_center, want.camera_center)):
                assert torch.equal(a, b) and not a.requires_grad
            assert (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy) == (144, 96, 1.0, 0.7)


@pytest.fixture(scope="module")
def path_scene(gpu):
    """About 3000 Gaussians at 144 x 96, five cameras along the scene's trajectory, and per tone mapping the per-camera
    render() images (computed once, shared, never written to)."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer
    from deblurgs_amd.cloud import GaussianCloud
    P, W, H, n = 3000, 144, 96, 5
    sc = synthetic.make_scene(P, W, H, K=n, seed=3, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    with torch.no_grad():
        cams = [model(i) for i in range(n)]
        pkgs = [gaussian_renderer.render(c, cloud, bg) for c in cams]
        renders = torch.stack([p["render"] for p in pkgs]).contiguous()
        depths = torch.stack([p["depth"][0] for p in pkgs]).contiguous()
    return dict(cloud=cloud, bg=bg, cams=cams, renders=renders, depths=depths, H=H, W=W, n=n, sc=sc)


@pytest.mark.parametrize("kind", ["identity", "gamma"])
def test_render_frames_equals_per_camera_render_then_finish(path_scene, kind):
    import torch
    from deblurgs_amd import losses, render_path as rp
    s = path_scene
    tm = losses.ToneMapping(kind)
    window = rp.center_crop_window(s["H"], s["W"], 0.95)
    assert rp.frame_groups(s["cams"], 2) == [(0, 2), (2, 4), (4, 5)]
    frames = rp.render_frames(s["cams"], s["cloud"], s["bg"], tm, crop_ratio=0.95, frames_per_call=2)
    assert frames.dtype == np.uint8 and frames.shape == (s["n"], window[1] - window[0], window[3] - window[2], 3)
    # per-camera render() followed by dgs_frames_finish: bit for bit
    want = rp.frames_finish(s["renders"], tm, window).cpu().numpy()
    assert np.array_equal(frames, want)
    # the reference's torch / numpy expression
    sub = _crop_nhwc(s["renders"].cpu().numpy(), window)
    assert not np.isnan(sub).any()
    if kind == "identity":
        assert np.array_equal(frames, (sub.clip(0.0, 1.0) * 255.0).astype(np.uint8))
    else:
        y = _gamma64(sub, tm.eps, tm.bound)
        _band_compare(frames, 255.0 * np.clip(y, 0.0, 1.0), (y > 0.0) & (y < 1.0), "render_frames gamma")
    assert len(np.unique(frames)) > 50                       # (a picture, not a constant)
    # two runs, and other groupings: the same bytes
    assert np.array_equal(rp.render_frames(s["cams"], s["cloud"], s["bg"], tm, crop_ratio=0.95, frames_per_call=2), frames)
    for per_call in (1, 5):
        assert np.array_equal(rp.render_frames(s["cams"], s["cloud"], s["bg"], tm, crop_ratio=0.95, frames_per_call=per_call),
                              frames), per_call
    torch.cuda.synchronize()


def test_render_frames_depth_takes_its_range_over_the_whole_path(path_scene):
    from deblurgs_amd import render_path as rp
    s = path_scene
    want = rp.depth_colorize(s["depths"], s["cloud"].z_near, s["cloud"].z_far).cpu().numpy()
    outs = [rp.render_frames(s["cams"], s["cloud"], s["bg"], "identity", frames_per_call=k, depth=True) for k in (2, 5)]
    for frames, colours in outs:
        assert frames.shape == (s["n"], s["H"], s["W"], 3) and colours.shape == (s["n"], s["H"], s["W"], 4)
        assert np.array_equal(colours, want)
        assert np.array_equal(frames, outs[0][0])
    assert (want[..., 3] == 255).all() and len(np.unique(want[..., :3].reshape(-1, 3), axis=0)) > 20


def test_evaluate_with_views_per_call_returns_the_same_floats(path_scene):
    import torch
    from deblurgs_amd import evaluation as ev, losses
    s = path_scene
    tm = losses.ToneMapping("gamma")
    torch.manual_seed(0)
    gts = (tm(s["renders"]).clamp(0.0, 1.0) + 0.02 * torch.randn_like(s["renders"])).clamp(0.0, 1.0)
    one = ev.evaluate(s["cams"], s["cloud"], s["bg"], gts, tm)
    for per_call in (2, 5):
        assert ev.evaluate(s["cams"], s["cloud"], s["bg"], gts, tm, views_per_call=per_call) == one, per_call
    assert 10.0 < one[0] < 80.0 and 0.3 < one[1] <= 1.0


def test_render_spiral_and_trainview_end_to_end(path_scene):
    import torch
    from deblurgs_amd import gaussian_renderer, render_path as rp
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    s = path_scene
    sc, H, W = s["sc"], s["H"], s["W"]
    torch.manual_seed(7)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    gt = torch.rand(4, 3, H, W, device="cuda")
    m = CameraMotionModule(ref, gt, curve_order=3, num_subframes=5, init_se3=torch.randn(4, 6) * 0.01, device="cuda")
    written = []
    frames = rp.render_spiral(m, s["cloud"], s["bg"], "gamma", n_frames=6, spin_for=2, frames_per_call=4,
                              writer=lambda f, path, fps: written.append((f.shape, path, fps)), path="spiral.mp4")
    assert frames.shape == (12, H, W, 3) and frames.dtype == np.uint8 and written == [((12, H, W, 3), "spiral.mp4", 32)]
    # the look-at depth: the torch mean of the centre half of the pivot camera's depth render
    middle = m.get_middle_cams()
    pivot = rp.mean_camera_pose(np.stack([rp.cam_to_c2w(c) for c in middle]))
    with torch.no_grad():
        depth = gaussian_renderer.render(rp.c2w_to_cam(middle[0], pivot), s["cloud"], torch.zeros(3, device="cuda"))["depth"]
        z = depth[:, H // 4:H * 3 // 4, W // 4:W * 3 // 4].mean()
    assert float(rp.center_depth(depth)) == float(z) and 0.2 < float(z) < 100.0
    a = rp.spiral_path(m, s["cloud"], n_frames=6, spin_for=2)
    b = rp.spiral_path(m, None, n_frames=6, spin_for=2, lookat_depth=z.cpu().numpy())
    assert len(a) == len(b) == 12
    for ca, cb in zip(a, b):
        assert torch.equal(ca.world_view_transform, cb.world_view_transform)
        assert torch.equal(ca.full_proj_transform, cb.full_proj_transform)
    assert np.array_equal(rp.render_frames(a, s["cloud"], s["bg"], "gamma", frames_per_call=12), frames)
    # the training views beside their ground truth
    imgs, gts, both = rp.render_trainview(m, s["cloud"], s["bg"], "gamma", start_index=1, length=1, frames_per_call=2)
    win = rp.center_crop_window(H, W, 0.95)
    h, w = win[1] - win[0], win[3] - win[2]
    assert imgs.shape == gts.shape == (2, h, w, 3) and both.shape == (2, h, 2 * w, 3)
    assert np.array_equal(both[:, :, :w], gts) and np.array_equal(both[:, :, w:], imgs)
    assert np.array_equal(gts, (_crop_nhwc(gt[1:3].cpu().numpy(), win).clip(0.0, 1.0) * 255.0).astype(np.uint8))
    assert np.array_equal(imgs, rp.render_frames(middle[1:3], s["cloud"], s["bg"], "gamma", crop_ratio=0.95))

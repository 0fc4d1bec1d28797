"""GPU tests of the visual reports (csrc/report.hip, deblurgs_amd/report.py): the radix select against np.sort, the
percentiles against the restated numpy formula bit for bit, dgs_report_images against a float32 numpy restatement (exactly
with the identity tone mapping, under tests/test_gpu_render_path.py's band rule behind a powf), the colours against a
float64 restatement, and evaluate(vis_dir=...) / traj_render end to end on small scenes."""
import ctypes
import os

import numpy as np
import pytest

import report_cases as rc
from helpers import synthetic

pytestmark = pytest.mark.gpu

GUARD = 64
NS = (1, 2, 63, 257, 70_001, 600_001)


def _eq_sorted(got, want):
    """== against the sorted array's entry; NaN for NaN; a -0.0 may stand for 0.0 (== holds them equal already)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


# ------------------------------------------------------------------------------------------------- 1. order statistics
@pytest.mark.parametrize("n", NS)
def test_order_stats_equal_the_sorted_array(gpu, n):
    """Every input kind, the four ranks one by one and in one call; once more with x one float off 16-byte alignment."""
    import torch
    from deblurgs_amd import report
    ranks = rc.ranks_of(n)
    for name, x in rc.order_inputs(n).items():
        s = np.sort(x)
        want = s[ranks]
        xt = torch.from_numpy(x).cuda()
        together = report.order_stats(xt, ranks).cpu().numpy()
        assert _eq_sorted(together, want), (name, n, together, want)
        if name == "with NaNs" and n > 2:
            assert np.isnan(s[-1]) and np.isnan(together[1])                   # NaNs come last
        for j, r in enumerate(ranks):
            alone = report.order_stats(xt, [r]).cpu().numpy()
            assert alone.view(np.uint32)[0] == together.view(np.uint32)[j], (name, n, r)
        if name in ("normal x 1", "all equal", "with NaNs"):
            shifted = torch.empty(n + 1, dtype=torch.float32, device="cuda")
            shifted[1:].copy_(xt)
            assert shifted[1:].data_ptr() % 16 == 4
            off = report.order_stats(shifted[1:], ranks).cpu().numpy()
            assert np.array_equal(off.view(np.uint32), together.view(np.uint32)), (name, n)


@pytest.mark.parametrize("n", [257, 70_001])
def test_order_stats_leave_the_words_around_out_and_tmp_alone(gpu, n):
    import torch
    from deblurgs_amd import _lib
    from deblurgs_amd.raster_call import _stream
    L = _lib.lib()
    x = rc.normal_with_ties(n, 1.0)
    ranks = rc.ranks_of(n)
    xt = torch.from_numpy(x).cuda()
    nbytes = L.dgs_order_stats_tmp_bytes(n, 4)
    tmp = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((GUARD // 4 + 4 + GUARD // 4,), float("nan"), dtype=torch.float32, device="cuda")
    out.view(torch.int32).fill_(0x5A5A5A5A)
    rc_ = L.dgs_order_stats(ctypes.c_void_p(xt.data_ptr()), n, (ctypes.c_uint64 * 4)(*ranks), 4,
                            ctypes.c_void_p(out.data_ptr() + GUARD), ctypes.c_void_p(tmp.data_ptr() + GUARD),
                            _stream(xt.device))
    _lib.check(rc_, "dgs_order_stats")
    torch.cuda.synchronize()
    th, oh = tmp.cpu().numpy(), out.cpu().numpy()
    assert (th[:GUARD] == 0xA5).all() and (th[GUARD + nbytes:] == 0xA5).all(), "guard zone around tmp overwritten"
    words = oh.view(np.uint32)
    assert (words[:GUARD // 4] == 0x5A5A5A5A).all() and (words[GUARD // 4 + 4:] == 0x5A5A5A5A).all(), "guard around out"
    assert _eq_sorted(oh[GUARD // 4: GUARD // 4 + 4], np.sort(x)[ranks])


# ------------------------------------------------------------------------------------------------- 2. percentiles
@pytest.mark.parametrize("n", NS)
def test_percentiles_equal_the_restated_numpy_formula_bit_for_bit(gpu, n):
    import torch
    from deblurgs_amd import report
    for name, x in rc.order_inputs(n).items():
        if name == "with NaNs":
            continue
        s = rc.sort_like_device(x)              # np.sort(x), -0.0 in front of 0.0
        assert np.array_equal(s, np.sort(x))
        xt = torch.from_numpy(x).cuda()
        for qs in ((1.0, 100.0), (0.0, 37.5, 50.0, 99.0)):
            got = report.percentiles(xt, qs)
            assert got.dtype == torch.float64 and tuple(got.shape) == (len(qs),)
            want = np.array([rc.percentile_restated(s, q) for q in qs])
            assert rc.same_bits(got.cpu().numpy(), want), (name, n, qs, got.cpu().numpy(), want)
            if np.isfinite(x).all():      # (and the restatement is numpy's own result: pinned on the CPU, shown here once more)
                assert rc.same_bits_or_zeros(want, np.percentile(x, qs)), (name, n, qs)


# ------------------------------------------------------------------------------------------------- 3. report images
SIZES = [(1, 5, 7), (3, 37, 53), (2, 64, 128)]


def _expected_y(x, mean):
    return rc.sequential_mean(x)[None] if mean else x


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("K,H,W", SIZES)
def test_report_images_identity_equal_numpy(gpu, K, H, W, mean):
    import torch
    from deblurgs_amd import report
    x = rc.frames_input(K, H, W, seed=K * 1000 + W)
    G = 1 if mean else K
    gt = rc.gt_input(G, H, W, seed=K + W)
    y = _expected_y(x, mean)
    want_u8, want_gt, want_err = rc.rounded_bytes(y), rc.rounded_bytes(gt), rc.l1_error(gt, y)
    xt, gtt = torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda()
    out, gt_u8, err = report.report_images(xt, None, mean=mean, gt=gtt[0] if mean else gtt)
    assert out.shape == gt_u8.shape == (G, H, W, 3) and err.shape == (G, H, W)
    assert np.array_equal(out.cpu().numpy(), want_u8)
    assert np.array_equal(gt_u8.cpu().numpy(), want_gt)
    assert np.array_equal(err.cpu().numpy(), want_err, equal_nan=True)
    nan = np.isnan(y).transpose(0, 2, 3, 1)
    assert nan.any() and (out.cpu().numpy()[nan] == 0).all()                      # a NaN gives 0
    # without a ground truth (subframes): the same bytes, nothing else; and each optional output alone
    alone, none_gt, none_err = report.report_images(xt, None, mean=mean)
    assert none_gt is None and none_err is None and np.array_equal(alone.cpu().numpy(), want_u8)
    _, g_only, e_none = report.report_images(xt, None, mean=mean, gt=gtt[0] if mean else gtt, want_err=False)
    assert e_none is None and np.array_equal(g_only.cpu().numpy(), want_gt)
    _, g_none, e_only = report.report_images(xt, None, mean=mean, gt=gtt[0] if mean else gtt, want_gt_u8=False)
    assert g_none is None and np.array_equal(e_only.cpu().numpy(), want_err, equal_nan=True)


@pytest.mark.parametrize("bound", [0.0, 0.05])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("K,H,W", SIZES)
def test_report_images_gamma_against_float64(gpu, K, H, W, mean, bound):
    """Bytes under the band rule around 255 y + 0.5; the error map within 1e-6 of float64 (a few ulp of powf at 1.0 on
    three channels)."""
    import torch
    from deblurgs_amd import losses, report
    tm = losses.ToneMapping("gamma", bound=bound)
    x = rc.frames_input(K, H, W, seed=K * 2000 + W)
    G = 1 if mean else K
    gt = rc.gt_input(G, H, W, seed=K + W + 1)
    s = _expected_y(x, mean)                                      # float32, exact
    nan = np.isnan(s)
    xt, gtt = torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda()
    out, gt_u8, err = report.report_images(xt, tm, mean=mean, gt=gtt[0] if mean else gtt)
    got = out.cpu().numpy()
    assert (got[nan.transpose(0, 2, 3, 1)] == 0).all()
    assert np.array_equal(gt_u8.cpu().numpy(), rc.rounded_bytes(gt))               # no tone mapping on the ground truth
    y64 = rc.gamma64(s, tm.eps, bound)
    ok = ~nan
    # (y > 0 always: 255 y + 0.5 needs no clip below; from y = 1 on the clamp pins 255, exactly, and is NOT in the band)
    v = np.where(y64[ok] >= 1.0, 255.0, 255.0 * y64[ok] + 0.5)
    rc.band_compare(got.transpose(0, 3, 1, 2)[ok], v, (y64[ok] > 0.0) & (y64[ok] < 1.0),
                    f"report gamma bound {bound} mean {mean} {K}x{H}x{W}")
    with np.errstate(invalid="ignore", over="ignore"):
        e64 = np.abs(gt.astype(np.float64) - y64).sum(axis=1) / 3.0
    fin = np.isfinite(e64)
    gap = np.abs(err.cpu().numpy().astype(np.float64)[fin] - e64[fin]).max()
    print(f"error map against float64: {gap:.3e}")
    assert fin.mean() > 0.5 and gap <= 1e-6
    sub, _, _ = report.report_images(xt, tm, mean=mean)
    assert np.array_equal(sub.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------- 4. colours
def _error_like(H, W, seed):
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((H, W)) * 0.05).astype(np.float32)
    x.reshape(-1)[::11] = 0.0
    return x


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 53), (64, 128)])
def test_scalar_colorize_equals_the_float64_restatement(gpu, shape):
    import torch
    from deblurgs_amd import report
    x = _error_like(*shape, seed=shape[1])
    x.reshape(-1)[::13] = np.nan if x.size > 13 else x.reshape(-1)[0]
    xt = torch.from_numpy(x).cuda()
    clean = torch.from_numpy(np.nan_to_num(x, nan=0.0)).cuda()
    lo_hi = report.percentiles(clean, (1.0, 100.0))
    lo_hi[1:] += 1e-6
    lo, hi = lo_hi.cpu().numpy()
    for rounded in (True, False):
        lut = report.jet_table(rounded)
        got = report.scalar_colorize(xt, lo_hi, rounded).cpu().numpy()
        assert got.shape == shape + (3,) and got.dtype == np.uint8
        assert np.array_equal(got, rc.colorize_restated(x, lo, hi, lut)), (shape, rounded)
    if x.size > 13:
        assert (got.reshape(-1, 3)[::13] == 0).all()                                  # a NaN gives three zero bytes
    # an unaligned destination, its neighbours left alone
    buf = torch.full((GUARD + 1 + 3 * x.size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    report.scalar_colorize(xt, lo_hi, True, out=buf[GUARD + 1: GUARD + 1 + 3 * x.size])
    host = buf.cpu().numpy()
    assert (host[:GUARD + 1] == 0xA5).all() and (host[GUARD + 1 + 3 * x.size:] == 0xA5).all()
    assert np.array_equal(host[GUARD + 1: GUARD + 1 + 3 * x.size].reshape(shape + (3,)),
                          rc.colorize_restated(x, lo, hi, report.jet_table(True)))
    # hi == lo: the map cannot place anything
    flat = torch.tensor([0.25, 0.25], dtype=torch.float64, device="cuda")
    assert (report.scalar_colorize(clean, flat).cpu().numpy() == 0).all()


def test_colorize_end_to_end_equals_numpy_s_percentile_then_the_chain(gpu):
    import torch
    from deblurgs_amd import report
    x = _error_like(37, 53, seed=5)
    got = report.colorize(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (37, 53, 3)
    assert np.array_equal(got, rc.colorize_reference(x, report.jet_table(True)))
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 50
    ranged = report.colorize(torch.from_numpy(x).cuda(), range=(0.01, 0.1)).cpu().numpy()
    assert np.array_equal(ranged, rc.colorize_restated(x, 0.01, 0.1, report.jet_table(True)))
    # a constant map: vmax += 1e-6 keeps the range open, every value sits at its lower end (the map's first entry), as in
    # the reference; with the range closed by hand (hi == lo) the kernel writes zeros
    const = torch.full((37, 53), 0.125, device="cuda")
    assert np.array_equal(report.colorize(const).cpu().numpy(),
                          rc.colorize_reference(np.full((37, 53), 0.125, np.float32), report.jet_table(True)))
    closed = torch.tensor([0.125, 0.125], dtype=torch.float64, device="cuda")
    assert (report.scalar_colorize(const, closed).cpu().numpy() == 0).all()
    assert (report.colorize(const, range=(0.125, 0.125)).cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------- 5. depth colours
@pytest.mark.parametrize("n", [257, 70_001])
def test_depth_colorize_with_a_clip_percentage(gpu, n):
    """utils/export_utils.py:56-65 with numpy on the same data, the index band rule of tests/test_gpu_render_path.py's depth
    test (copied): equal outside 1e-3 of an index step, one entry off at most inside."""
    import torch
    from deblurgs_amd import render_path as rp, report
    rng = np.random.default_rng(n)
    d = rng.uniform(0.5, 30.0, n).astype(np.float32)
    d[:3] = [55.0, 60.0, 80.0]                                   # a tail the clip cuts off
    dt = torch.from_numpy(d).cuda()
    lut = rp.jet_r_table().astype(np.int64)
    for z_near, z_far, p in ((0.2, 100.0, 0.99), (2.0, 20.0, 0.99), (0.2, 100.0, 0.5)):
        got = report.depth_colorize(dt, z_near, z_far, clip_percentage=p).cpu().numpy()
        assert got.shape == (n, 4) and got.dtype == np.uint8
        cap = np.sort(d)[int((n - 1) * p)]
        lo = np.float64(max(np.float32(z_near), d.min()))
        hi = np.float64(min(np.float32(z_far), d.max(), cap))
        assert hi < d.max()
        raw = (d.astype(np.float64) - lo) / (hi - lo)
        v = 256.0 * np.clip(raw, 0.0, 1.0)
        idx = np.minimum(np.floor(v).astype(np.int64), 255)
        band = (raw > 0.0) & (raw < 1.0) & (np.abs(v - np.rint(v)) < rc.BAND)
        exact = (got == lut[idx]).all(axis=1)
        near = exact | (got == lut[np.clip(idx - 1, 0, 255)]).all(axis=1) | (got == lut[np.clip(idx + 1, 0, 255)]).all(axis=1)
        print(f"n {n} range ({z_near}, {z_far}) clip {p}: {band.sum()} in the band, {int((~exact).sum())} differ")
        assert (exact | band).all(), (d[~(exact | band)][:5], got[~(exact | band)][:5])
        assert near.all() and band.mean() <= 0.01 + 1.0 / n
    assert np.array_equal(report.depth_colorize(dt, 0.2, 100.0, clip_percentage=1.0).cpu().numpy(),
                          rp.depth_colorize(dt, 0.2, 100.0).cpu().numpy())


# ------------------------------------------------------------------------------------------------- 6. evaluate(vis_dir)
@pytest.fixture(scope="module")
def small_scene(gpu):
    """500 Gaussians at 64 x 48, three test cameras along the scene's trajectory, noisy ground truth (computed once,
    shared, never written to)."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses
    from deblurgs_amd.cloud import GaussianCloud
    P, W, H, n = 500, 64, 48, 3
    sc = synthetic.make_scene(P, W, H, K=n, seed=5, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    tm = losses.ToneMapping("gamma")
    with torch.no_grad():
        cams = [model(i) for i in range(n)]
        renders = torch.stack([gaussian_renderer.render(c, cloud, bg)["render"] for c in cams]).contiguous()
        torch.manual_seed(0)
        gts = (tm(renders).clamp(0.0, 1.0) + 0.03 * torch.randn_like(renders)).clamp(0.0, 1.0)
    return dict(cloud=cloud, bg=bg, cams=cams, renders=renders, gts=gts, tm=tm, H=H, W=W, n=n, sc=sc)


def _read_image(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_evaluate_writes_the_reference_s_three_files_per_view(small_scene, tmp_path):
    import torch
    from deblurgs_amd import evaluation as ev, report
    s = small_scene
    plain = ev.evaluate(s["cams"], s["cloud"], s["bg"], s["gts"], s["tm"])
    runs = {}
    for per_call in (None, 3):
        seen = {}
        floats = ev.evaluate(s["cams"], s["cloud"], s["bg"], s["gts"], s["tm"], views_per_call=per_call, vis_dir="vis",
                             writer=lambda p, a: seen.__setitem__(p, a.copy()))
        assert floats == plain and type(floats[0]) is float                          # the same Python floats
        runs[per_call] = seen
    names = [os.path.join("vis", f"{i:03d}_{kind}.png") for i in range(s["n"]) for kind in ("gt", "render", "error")]
    assert sorted(runs[None]) == sorted(names) and not os.path.exists("vis")
    for name in names:
        assert np.array_equal(runs[None][name], runs[3][name]), name
    lut = report.jet_table(True)
    for i in range(s["n"]):
        image = s["tm"](s["renders"][i])
        want = image.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()      # save_image's own
        assert np.array_equal(runs[None][os.path.join("vis", f"{i:03d}_render.png")], want), i
        want_gt = s["gts"][i].mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(runs[None][os.path.join("vis", f"{i:03d}_gt.png")], want_gt), i
        err = torch.abs(s["gts"][i] - image).permute(1, 2, 0).mean(dim=-1).cpu().numpy()
        assert np.array_equal(runs[None][os.path.join("vis", f"{i:03d}_error.png")], rc.colorize_reference(err, lut)), i
    # and as files: the directory is removed and recreated, the PNGs decode to the same bytes
    vis = tmp_path / "vis"
    vis.mkdir()
    (vis / "stale.png").write_bytes(b"x")
    assert ev.evaluate(s["cams"], s["cloud"], s["bg"], s["gts"], s["tm"], vis_dir=str(vis)) == plain
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert sorted(os.listdir(vis)) == sorted(os.path.basename(n)[:-4] + ".npy" for n in names)
        return
    assert sorted(os.listdir(vis)) == sorted(os.path.basename(n) for n in names)
    for name in names:
        assert np.array_equal(_read_image(str(vis / os.path.basename(name))), runs[None][name]), name


# ------------------------------------------------------------------------------------------------- 7. traj_render
def test_traj_render_writes_the_reference_s_files(small_scene, tmp_path):
    import torch
    from deblurgs_amd import report
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    s = small_scene
    sc, H, W = s["sc"], s["H"], s["W"]
    torch.manual_seed(11)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    gt = torch.rand(2, 3, H, W, device="cuda")
    m = CameraMotionModule(ref, gt, curve_order=3, num_subframes=5, init_se3=torch.randn(2, 6) * 0.01, device="cuda")
    m.link_gaussian(s["cloud"])
    bg = s["bg"]
    names = [n for i in range(2) for n in report.traj_render_names(i, 3)]
    assert names[:6] == ["000_00.png", "000_01.png", "000_02.png", "000_blur.png", "000_gt.png", "000_l1.png"]
    runs = []
    for two_calls in (None, True):
        seen = {}
        paths = report.traj_render(m, s["cloud"], str(tmp_path / "model"), 30, "identity", background=bg, _two_calls=two_calls,
                                   writer=lambda p, a: seen.__setitem__(os.path.basename(p), a.copy()))
        assert [os.path.basename(p) for p in paths] == names
        assert all(os.path.dirname(p) == str(tmp_path / "model") + "/traj_render_00030" for p in paths)
        runs.append(seen)
    assert not (tmp_path / "model").exists()                                            # a writer touches no directory
    for name in names:
        assert np.array_equal(runs[0][name], runs[1][name]), name                       # one call or two: the same bytes
    lut = report.jet_table(True)
    for i in range(2):
        with torch.no_grad():
            three = m.query(i, 3, background=bg)["subframes"]
            every = m.query(i, "all", background=bg)["subframes"]
        assert three.shape[0] == 3 and every.shape[0] >= 5
        finished = report.report_images(three.contiguous(), "identity")[0].cpu().numpy()
        for j in range(3):
            assert np.array_equal(runs[0][f"{i:03d}_{j:02d}.png"], finished[j]), (i, j)
        blurred = rc.sequential_mean(every.cpu().numpy())
        assert np.array_equal(runs[0][f"{i:03d}_blur.png"], rc.rounded_bytes(blurred[None])[0]), i
        g = gt[i].cpu().numpy()
        assert np.array_equal(runs[0][f"{i:03d}_gt.png"], rc.rounded_bytes(g[None])[0]), i
        err = rc.l1_error(g[None], blurred[None])[0]
        assert np.array_equal(runs[0][f"{i:03d}_l1.png"], rc.colorize_reference(err, lut)), i
    assert len(np.unique(runs[0]["000_blur.png"])) > 20                                 # (a picture, not a constant)
    # and as files, under {model_path}/traj_render_{iteration:05d}, removed and recreated
    out = tmp_path / "model" / "traj_render_00030"
    out.mkdir(parents=True)
    (out / "stale.png").write_bytes(b"x")
    paths = report.traj_render(m, s["cloud"], str(tmp_path / "model"), 30, "gamma", background=bg)
    ext = os.path.splitext(paths[0])[1]
    assert sorted(os.listdir(out)) == sorted(n[:-4] + ext for n in names)
    if ext == ".png":
        sub = report.report_images(m.query(1, 3, background=bg)["subframes"].detach().contiguous(), "gamma")[0].cpu().numpy()
        assert np.array_equal(_read_image(str(out / "001_02.png")), sub[2])

"""CPU tests of camera-path rendering (deblurgs_amd/render_path.py, csrc/frames.hip): the new entry points are exported,
bound and reject bad arguments before any HIP call; the path geometry, the crop windows and the jet_r table equal
tests/golden/paths_golden.npz (the reference's own functions, tests/golden/make_golden_paths.py); the spiral path has the
shape get_render_path gives it; the grouping of cameras into rasteriser calls."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "paths_golden.npz")
NEW_SYMBOLS = ("dgs_frames_finish", "dgs_depth_range_tmp_bytes", "dgs_depth_range", "dgs_depth_colorize")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_new_symbols_are_declared_exported_and_bound():
    from deblurgs_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s) and (s + "(") in header, s
        assert getattr(L, s).argtypes == _lib.EXPORTS[s][1]
    assert L.dgs_abi_version() == 15            # additions to ABI 15
    from deblurgs_amd import build
    assert build.SOURCES["frames.hip"] == ["-ffp-contract=off"]


def test_frames_finish_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096          # non-null dummies: only the argument logic runs
    ok = dict(color=a, K=2, H=10, W=12, tone=_lib.TONE_IDENTITY, eps=0.0, bound=0.0, y0=0, x0=0, h=10, w=12, out=a)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_frames_finish(v["color"], v["K"], v["H"], v["W"], v["tone"], v["eps"], v["bound"], v["y0"], v["x0"],
                                   v["h"], v["w"], v["out"], None)

    for kw, text in (({"color": None}, b"null"), ({"out": None}, b"null"), ({"K": 0}, b"K must be"), ({"K": -3}, b"K must be"),
                     ({"h": 0}, b"empty window"), ({"w": 0}, b"empty window"), ({"w": -1}, b"empty window"),
                     ({"y0": 1}, b"leaves the image"), ({"x0": 1}, b"leaves the image"), ({"y0": -1, "h": 5}, b"leaves the image"),
                     ({"x0": 11, "w": 2}, b"leaves the image"), ({"h": 11}, b"leaves the image"),
                     ({"x0": 2**31 - 1, "w": 2**31 - 1}, b"leaves the image"),
                     ({"H": 0}, b"empty image"), ({"tone": 2}, b"tone_mapping"), ({"tone": -1}, b"tone_mapping"),
                     ({"tone": _lib.TONE_GAMMA, "bound": 0.5}, b"bound"),
                     ({"tone": _lib.TONE_GAMMA, "bound": float("nan")}, b"bound")):
        assert call(**kw) == -1, kw
        assert text in L.dgs_last_error(), (kw, L.dgs_last_error())
    with pytest.raises(RuntimeError, match="dgs_frames_finish failed"):
        _lib.check(call(K=0), "dgs_frames_finish")


def test_depth_kernels_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096
    assert L.dgs_depth_range_tmp_bytes(0) == 0
    assert L.dgs_depth_range_tmp_bytes(1) == 8 and L.dgs_depth_range_tmp_bytes(257) == 16
    assert L.dgs_depth_range_tmp_bytes(10**12) == L.dgs_depth_range_tmp_bytes(10**7) == 8192     # capped block count
    for args, text in (((None, 5, a, a), b"null"), ((a, 5, None, a), b"null"), ((a, 5, a, None), b"null"),
                       ((a, 0, a, a), b"n must be")):
        assert L.dgs_depth_range(*args, None) == -1 and text in L.dgs_last_error(), args
    for args, text in (((None, 5, a, 0.0, 1.0, a, a), b"null"), ((a, 5, None, 0.0, 1.0, a, a), b"null"),
                       ((a, 5, a, 0.0, 1.0, None, a), b"null"), ((a, 5, a, 0.0, 1.0, a, None), b"null"),
                       ((a, 0, a, 0.0, 1.0, a, a), b"n must be"), ((a, 5, a, 0.0, 1.0, a + 1, a), b"aligned"),
                       ((a, 5, a, 0.0, 1.0, a, a + 2), b"aligned")):
        assert L.dgs_depth_colorize(*args, None) == -1 and text in L.dgs_last_error(), args


def test_wrappers_refuse_cpu_tensors_and_other_clip_percentages():
    import torch
    from deblurgs_amd import render_path as rp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rp.frames_finish(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rp.depth_range(torch.zeros(4))
    with pytest.raises(NotImplementedError, match="clip_percentage"):
        rp.depth_colorize(torch.zeros(1, 4, 4), clip_percentage=0.99)
    with pytest.raises(NotImplementedError, match="tone mappings"):
        rp._tone_args("reverse_gamma")


def test_geometry_helpers_equal_the_reference(golden):
    from deblurgs_amd import render_path as rp
    for name in ("tight", "wide", "one", "two"):
        got = rp.mean_camera_pose(golden[f"mean_{name}_in"])
        err = np.abs(got - golden[f"mean_{name}_out"]).max()
        assert err <= 1e-12, (name, err)
    eyes, lookats, ups = golden["eye_in"]
    for i in range(eyes.shape[0]):
        got = rp.c2w_from_eye(eyes[i], lookats[i], ups[i])
        assert np.abs(got - golden["eye_out"][i]).max() <= 1e-12, i


def test_mean_camera_pose_does_not_import_scipy():
    src = open(os.path.join(ROOT, "deblurgs_amd", "render_path.py")).read()
    assert "import scipy" not in src and "from scipy" not in src and "import matplotlib" not in src


def test_center_crop_window_equals_the_reference_windows(golden):
    from deblurgs_amd import render_path as rp
    table, ratios = golden["crop_table"], golden["crop_ratio"]
    assert len(table) >= 12
    for (H, W, h, w, h1, w1), ratio in zip(table.tolist(), ratios.tolist()):
        g = rp.center_crop_window(H, W, ratio)
        assert (g[1] - g[0], g[3] - g[2]) == (h, w), (H, W, ratio, g)
        if h and w:
            assert (g[0], g[2]) == (h1, w1), (H, W, ratio, g)
    assert rp.center_crop_window(1080, 1920, 1.0) == (0, 1080, 0, 1920)


def test_jet_r_table_equals_the_fixture_and_matplotlib(golden):
    from deblurgs_amd import render_path as rp
    lut = rp.jet_r_table()
    assert lut.dtype == np.uint8 and lut.shape == (256, 4)
    assert np.array_equal(lut, golden["jet_r"])
    assert tuple(lut[0]) == (127, 0, 0, 255) and tuple(lut[255]) == (0, 0, 127, 255)
    assert tuple(golden["jet_r_bad"]) == (0, 0, 0, 0)          # what the kernel writes for hi == lo / NaN
    try:
        import matplotlib
    except ImportError:
        return
    cm = matplotlib.colormaps["jet_r"]
    d = np.random.default_rng(0).random(50_000).astype(np.float32)
    d[:6] = [0.0, 1.0, 0.5, 1.0 / 256.0, 255.0 / 256.0, np.nextafter(np.float32(1.0), np.float32(0.0))]
    want = (cm(d) * 255).astype(np.uint8)
    assert np.array_equal(want, lut[np.minimum((d * np.float32(256.0)).astype(np.int64), 255)])


def _motion(n=4, seed=0):
    import torch
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    torch.manual_seed(seed)
    ref = RefCamera(64, 48, 1.0, 0.8, device="cpu")
    return CameraMotionModule(ref, torch.rand(n, 3, 48, 64), curve_order=3, num_subframes=7, device="cpu",
                              init_se3=torch.randn(n, 6) * 0.05)


def test_get_middle_cams_on_the_cpu():
    import torch
    m = _motion()
    cams = m.get_middle_cams()
    assert len(cams) == len(m) == 4
    for i, cam in enumerate(cams):
        nu = m._sample_nu_from_alignment(i)
        want = m.get_trajectory(i, nu[nu.shape[0] // 2: nu.shape[0] // 2 + 1])[0]
        assert torch.equal(cam.world_view_transform, want.world_view_transform)
        assert torch.equal(cam.full_proj_transform, want.full_proj_transform)
        assert not cam.world_view_transform.requires_grad
        assert (cam.image_width, cam.image_height) == (64, 48)


@pytest.mark.parametrize("n_frames,spin_for,depth", [(50, 2, 3.0), (7, 3, 0.8), (5, 1, 12.5)])
def test_spiral_path_geometry(n_frames, spin_for, depth):
    import torch
    from deblurgs_amd import render_path as rp
    m = _motion()
    angle = 5.0
    cams = rp.spiral_path(m, None, spin_angle=angle, n_frames=n_frames, spin_for=spin_for, lookat_depth=depth)
    n = n_frames * spin_for
    assert len(cams) == n
    pivot = rp.mean_camera_pose(np.stack([rp.cam_to_c2w(c) for c in m.get_middle_cams()]))
    eye, lookat = pivot[:3, 3], pivot[:3, 3] + depth * pivot[:3, 2]
    widest = np.tan(np.deg2rad(angle)) * depth
    want_r = np.linspace(widest / spin_for, widest, n)
    turn = np.tile(np.linspace(0.0, 2.0 * np.pi, n_frames), spin_for)
    for i, cam in enumerate(cams):
        assert cam.world_view_transform.dtype == torch.float32
        assert (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy) == (64, 48, 1.0, 0.8)
        # in float64, before the camera's matrices are rounded to fp32: the pose c2w_to_cam is handed
        local = np.array([np.cos(turn[i]) * want_r[i], np.sin(turn[i]) * want_r[i], 0.0, 1.0])
        e = (pivot @ local)[:3]
        c2w = rp.c2w_from_eye(e, lookat, pivot[:3, 1])
        to_point = lookat - e
        off_axis = np.linalg.norm(np.cross(c2w[:3, 2], to_point))           # distance of the look-at point from the +z ray
        assert off_axis <= 1e-9 and c2w[:3, 2] @ to_point > 0.0, (i, off_axis)
        in_plane = pivot[:3, :3].T @ (e - eye)
        assert abs(np.hypot(in_plane[0], in_plane[1]) - want_r[i]) <= 1e-9 and abs(in_plane[2]) <= 1e-9
        # the camera that came back carries that pose (fp32 matrices) ...
        got = rp.cam_to_c2w(cam)
        assert np.abs(got - c2w).max() <= 2e-6 * max(1.0, np.abs(c2w).max()), (i, np.abs(got - c2w).max())
        # ... and survives the round trip through its own c2w
        again = rp.c2w_to_cam(cam, got)
        for a, b in ((again.world_view_transform, cam.world_view_transform), (again.full_proj_transform, cam.full_proj_transform),
                     (again.camera_center, cam.camera_center)):
            assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
        assert torch.equal(again.world_view_transform[:3, :3], cam.world_view_transform[:3, :3])


class _Cam:
    def __init__(self, W, H, fx=1.0, fy=0.8):
        self.image_width, self.image_height, self.FoVx, self.FoVy = W, H, fx, fy


def test_frame_groups():
    from deblurgs_amd import _lib, render_path as rp
    same = [_Cam(144, 96) for _ in range(5)]
    assert rp.frame_groups(same, 2) == [(0, 2), (2, 4), (4, 5)]
    assert rp.frame_groups(same, 1) == [(i, i + 1) for i in range(5)]
    assert rp.frame_groups(same, 5) == rp.frame_groups(same, 99) == [(0, 5)]
    assert rp.frame_groups([], 4) == []
    mixed = [_Cam(144, 96), _Cam(144, 96), _Cam(144, 96), _Cam(96, 144), _Cam(96, 144), _Cam(144, 96), _Cam(144, 96, fx=1.1),
             _Cam(144, 96, fx=1.1)]
    assert rp.frame_groups(mixed, 2) == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 8)]
    assert rp.frame_groups(mixed, 8) == [(0, 3), (3, 5), (5, 6), (6, 8)]
    many = [_Cam(8, 8) for _ in range(2 * _lib.DGS_MAX_K + 3)]
    g = rp.frame_groups(many, 10_000)
    assert max(e - b for b, e in g) == _lib.DGS_MAX_K and g[-1] == (2 * _lib.DGS_MAX_K, 2 * _lib.DGS_MAX_K + 3)
    with pytest.raises(ValueError):
        rp.frame_groups(same, 0)
    assert isinstance(rp.FRAMES_PER_CALL, int) and 1 <= rp.FRAMES_PER_CALL <= _lib.DGS_MAX_K


def test_path_plan_refusals():
    """What render_frames, write_frames_png and write_frames_video start from (_path_plan), named as the caller."""
    import torch
    from deblurgs_amd import render_path as rp
    same = [_Cam(144, 96) for _ in range(5)]
    for who in ("render_frames", "write_frames_png", "write_frames_video"):
        with pytest.raises(ValueError, match="no cameras"):
            rp._path_plan([], 1.0, None, who)
        with pytest.raises(ValueError, match=f"{who}.*share one image size"):
            rp._path_plan(same + [_Cam(96, 144)], 1.0, None, who)
        with pytest.raises(ValueError, match="crop_ratio 0.0 leaves no pixel of a 144 x 96 image"):
            rp._path_plan(same, 0.0, None, who)
        with pytest.raises(ValueError, match="frames_per_call"):
            rp._path_plan(same, 1.0, 0, who)
        for cam in same:
            cam.world_view_transform = torch.eye(4)
        with pytest.raises(RuntimeError, match=f"{who} needs .* HIP device \\(no CPU fallback\\)"):
            rp._path_plan(iter(same), 0.5, 2, who)
    with pytest.raises(ValueError, match="no cameras"):
        rp.render_frames([], None, None)
    with pytest.raises(ValueError, match="no cameras"):
        rp.write_frames_png([], None, None, os.devnull)
    with pytest.raises(ValueError, match="no cameras"):
        rp.write_frames_video([], None, None, os.devnull, 32)


def test_write_frames(tmp_path):
    from deblurgs_amd import render_path as rp
    frames = (np.arange(2 * 5 * 7 * 3) % 256).astype(np.uint8).reshape(2, 5, 7, 3)
    paths = rp.write_frames(frames, str(tmp_path / "out"))
    try:
        from PIL import Image
    except ImportError:
        assert len(paths) == 1 and np.array_equal(np.load(paths[0]), frames)
        return
    assert len(paths) == 2
    assert np.array_equal(np.asarray(Image.open(paths[1])), frames[1])


def test_evaluate_takes_views_per_call():
    import inspect
    from deblurgs_amd import evaluation as ev
    assert inspect.signature(ev.evaluate).parameters["views_per_call"].default is None

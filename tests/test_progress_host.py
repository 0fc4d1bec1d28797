"""The host side of the training-progress visualiser (no GPU needed): exports and refusals of dgs_draw_prims /
dgs_cone_segments, the shot schedule, the view colours, the reference painter of tests/progress_cases.py against the closed
form include/dgs_hip.h states, the overview camera's search, and the refusal of CPU tensors.  The device is held to the
painter byte for byte in tests/test_gpu_progress.py."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import progress_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake(n=1):
    """A host buffer standing in for a device one: an argument check must answer before anything touches it."""
    return ctypes.cast((ctypes.c_uint8 * (64 * n))(), ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------- the two entry points
def test_new_symbols_load_and_the_abi_is_still_15():
    from deblurgs_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "dgs_draw_prims") and hasattr(L, "dgs_cone_segments")
    assert "dgs_draw_prims" in _lib.EXPORTS and "dgs_cone_segments" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", header).group(1)) == 15 == L.dgs_abi_version() == _lib.ABI_VERSION
    from deblurgs_amd import build
    assert "draw.hip" in build.SOURCES


def test_draw_prims_argument_errors_are_codes_with_text():
    from deblurgs_amd import _lib
    L = _lib.lib()
    img, prims, owner = _fake(), _fake(), _fake()
    bad = [((None, 8, 8, prims, 1, owner), "null pointer"), ((img, 8, 8, None, 1, owner), "null pointer"),
           ((img, 8, 8, prims, 1, None), "null pointer"), ((img, 0, 8, prims, 1, owner), "W and H"),
           ((img, 8, -1, prims, 1, owner), "W and H"), ((img, 65536, 32768, prims, 1, owner), "2^31"),
           ((img, 8, 8, prims, -1, owner), "negative"),
           ((img, 8, 8, ctypes.c_void_p(prims.value + 2), 1, owner), "aligned"),
           ((img, 8, 8, prims, 1, ctypes.c_void_p(owner.value + 1)), "aligned")]
    for args, text in bad:
        assert L.dgs_draw_prims(*args, None) != 0, args
        assert text in L.dgs_last_error().decode(), (args, L.dgs_last_error())
    assert L.dgs_draw_prims(img, 8, 8, prims, 0, owner, None) == 0          # n = 0: nothing is touched, nothing enqueued


def test_cone_segments_argument_errors_are_codes_with_text():
    from deblurgs_amd import _lib
    L = _lib.lib()
    good = [4, _fake(4), _fake(), 0.5, 0.4, 0.5, _fake(), _fake(), 64, 48, _fake(), _fake(16)]
    for at in (1, 2, 6, 7, 10, 11):
        args = list(good)
        args[at] = None
        assert L.dgs_cone_segments(*args, None) != 0 and "null pointer" in L.dgs_last_error().decode(), at
        args[at] = ctypes.c_void_p(good[at].value + 2)
        assert L.dgs_cone_segments(*args, None) != 0 and "aligned" in L.dgs_last_error().decode(), at
    for at, value, text in ((8, 0, "W and H"), (9, -3, "W and H"), (0, -1, "negative"), (0, (1 << 24) + 1, "2^24")):
        args = list(good)
        args[at] = value
        assert L.dgs_cone_segments(*args, None) != 0 and text in L.dgs_last_error().decode(), (at, value)
    args = list(good)
    args[0] = 0
    assert L.dgs_cone_segments(*args, None) == 0


# ------------------------------------------------------------------------------------------------- schedule and colours
def test_vis_iterations_equal_the_numpy_expression():
    from deblurgs_amd import progress
    n_iters, n_shots, alpha = 30000, 200, 1.7
    a = n_iters / n_shots ** (alpha)
    want = (a * (np.arange(1, n_shots + 1).astype(float)) ** alpha).astype(int)
    got = progress.vis_iterations(30000)
    assert np.array_equal(got, want) and got.dtype == want.dtype
    assert got[0] == 3 and got[-1] == 30000 and len(got) == 200 and (np.diff(got) > 0).all()
    assert np.array_equal(progress.vis_iterations(7000, 50, 2.0), (7000 / 50 ** 2.0 * np.arange(1, 51).astype(float) ** 2.0)
                          .astype(int))


def test_view_colours_endpoints_and_truncation():
    from deblurgs_amd import progress
    c = progress.view_colours(4)
    assert c.dtype == np.uint8 and c.shape == (4, 3)
    assert c[0].tolist() == [0, 255, 255] and c[-1].tolist() == [255, 255, 0]
    assert c[1].tolist() == [85, 255, 170] and c[2].tolist() == [170, 255, 85]          # 255 / 3 = 85 exactly
    c = progress.view_colours(8)                                                          # 255 t is no integer: truncated
    t = np.linspace(0, 1, 8)
    assert c[:, 0].tolist() == [int(255 * v) for v in t] and c[:, 0].tolist() != [int(round(255 * v)) for v in t]
    assert c[:, 2].tolist() == [int((1 - v) * 255) for v in t]
    # green is (1 - t) 255 + t 255 in floating point: a sum just below 255 truncates to 254, as it does in the reference
    assert c[:, 1].tolist() == [int((1 - v) * 255 + v * 255) for v in t] and set(c[:, 1].tolist()) <= {254, 255}
    assert progress.view_colours(1).tolist() == [[0, 255, 255]]
    assert progress.pack_rgb(c[-1]) == 255 | 255 << 8 and progress.pack_rgb(c).shape == (8,)


# ------------------------------------------------------------------------------------------------- the painter
def test_the_walk_equals_the_closed_form_on_random_segments():
    rng = np.random.default_rng(3)
    for _ in range(3000):
        span = int(rng.choice([3, 20, 300]))
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-span, span + 1, size=4))
        dx, dy = abs(x1 - x0), abs(y1 - y0)
        steep = dy > dx
        maj, mn = (dy, dx) if steep else (dx, dy)
        sx, sy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
        want = []
        for i in range(maj + 1):
            off = pc.closed_form_offset(maj, mn, i)
            want.append((x0 + sx * off, y0 + sy * i) if steep else (x0 + sx * i, y0 + sy * off))
        got = pc.walk(x0, y0, x1, y1)
        assert got == want, (x0, y0, x1, y1)
        assert got[0] == (x0, y0) and got[-1] == (x1, y1)


def test_ties_stay_with_the_start_point():
    assert pc.walk(0, 0, 4, 2) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]
    assert pc.walk(4, 2, 0, 0) == [(4, 2), (3, 2), (2, 1), (1, 1), (0, 0)]
    assert set(pc.walk(0, 0, 4, 2)) != set(pc.walk(4, 2, 0, 0))


def test_entering_the_canvas_by_the_invariant_equals_walking_there():
    rng = np.random.default_rng(4)
    for _ in range(60):
        inside = (int(rng.integers(0, pc.W)), int(rng.integers(0, pc.H)))
        away = (int(rng.integers(-20000, 20000)), int(rng.integers(-20000, 20000)))
        for a, b in ((inside, away), (away, inside)):
            plain = [(x, y) for x, y in pc.walk(*a, *b) if 0 <= x < pc.W and 0 <= y < pc.H]
            assert pc.line_pixels(*a, *b, pc.W, pc.H, far=64) == plain, (a, b)
            assert pc.line_pixels(*a, *b, pc.W, pc.H, far=1 << 40) == plain, (a, b)


def test_the_batched_painter_equals_the_painter():
    img = pc.canvas(5)
    segs = pc.draw_cases()["random"]
    segs = segs[segs[:, 4] == 0]
    assert len(segs) == 300
    assert np.array_equal(pc.paint_lines_batched(img, segs), pc.paint(img, segs))


def test_painter_s_order_and_skips():
    img = np.zeros((pc.H, pc.W, 3), dtype=np.uint8)
    out = pc.paint(img, pc.draw_cases()["three on one pixel"])
    assert out[10, 30].tolist() == [200, 100, 50] and out[12, 30].tolist() == [9, 8, 7] and out[10, 5].tolist() == [255, 0, 0]
    out = pc.paint(img, pc.draw_cases()["bad discs"])
    # (the radius-64 disc covers the whole canvas; the three records before it draw nothing; the radius-1 disc is 5 pixels)
    assert out[5, 5].tolist() == [5, 0, 0] and (out[..., 0] == 5).sum() == 5 and (out[..., 0] == 4).sum() == pc.W * pc.H - 5
    assert not pc.paint(img, pc.draw_cases()["beyond the limit"][:4]).any()
    assert pc.paint(img, pc.draw_cases()["far endpoints"]).any()


# ------------------------------------------------------------------------------------------------- the overview camera
def _ring(n=14, radius=3.0, seed=0):
    """Camera-to-world poses on a ring in the plane z = -4, all looking roughly at the origin."""
    from deblurgs_amd import render_path
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        a = 2 * math.pi * k / n
        eye = np.array([radius * math.cos(a), 0.6 * radius * math.sin(a), -4.0]) + 0.05 * rng.normal(size=3)
        out.append(render_path.c2w_from_eye(eye, 0.1 * rng.normal(size=3), [0.0, 1.0, 0.0]))
    return np.stack(out)


@pytest.mark.parametrize("radius", [0.2, 3.0, 9.0])
def test_overview_zoom_is_the_lowest_zoom_that_sees_every_centre(radius):
    from deblurgs_amd import progress, render_path
    ref = types.SimpleNamespace(image_width=64, image_height=48, FoVx=0.9, FoVy=0.7, znear=0.01, zfar=100.0)
    c2ws = _ring(radius=radius)
    lookat = np.array([0.05, -0.02, 1.0])
    zoom, c2w = progress.overview_zoom(c2ws, lookat, ref)
    mean = render_path.mean_camera_pose(c2ws)
    host = progress._shell(ref, "cpu")
    cam_at = lambda z: render_path.c2w_to_cam(host, progress.zoomed_c2w(mean, lookat, z))
    assert np.array_equal(c2w, progress.zoomed_c2w(mean, lookat, zoom))
    assert progress.centres_good(c2ws[:, :3, 3], cam_at(zoom)).all()
    assert 1.5 <= zoom < 100.0
    if not zoom < 1.5 + 1e-3:
        assert not progress.centres_good(c2ws[:, :3, 3], cam_at(zoom - 2e-3)).all()
    if radius == 0.2:
        assert zoom < 1.5 + 1e-3        # a tight ring is seen from the lower bound already
    if radius == 9.0:
        assert zoom > 1.5 + 1e-3


# ------------------------------------------------------------------------------------------------- no CPU fallback
def test_progress_functions_refuse_cpu_tensors(tmp_path):
    import torch
    from deblurgs_amd import progress
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    prims = torch.zeros(1, 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.draw(img, prims)
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.cone_segments(torch.zeros(1, 4, 4), torch.zeros(1, 3), 0.5, 0.5, 0.5, torch.eye(4), torch.eye(4), 8, 8,
                               torch.zeros(1, dtype=torch.int32))
    ref = RefCamera(16, 12, 0.9, 0.7, device="cpu")
    motion = CameraMotionModule(ref, torch.zeros(2, 3, 12, 16), curve_order=3, num_subframes=5, device="cpu")
    cloud = types.SimpleNamespace(_xyz=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.alignment_prims(motion, [0, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.alignment_plot(motion, [0, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.overview_camera(motion, cloud)
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.camera_overlay(motion, cloud, None, torch.zeros(3))
    with pytest.raises(RuntimeError, match="HIP device"):
        progress.ProgressVisualizer(motion, cloud, torch.zeros(3), str(tmp_path / "model"), 12)
    assert not (tmp_path / "model").exists()

"""GPU tests of the training-progress visualiser (csrc/draw.hip, deblurgs_amd/progress.py): dgs_draw_prims against the
numpy painter of tests/progress_cases.py byte for byte, dgs_cone_segments against a float64 numpy restatement of the
reference's lines, and camera_overlay / alignment_plot / ProgressVisualizer end to end on a tiny scene."""
import ctypes
import os

import numpy as np
import pytest

import progress_cases as pc
from helpers import synthetic

pytestmark = pytest.mark.gpu

CASES = pc.draw_cases()


def _draw_raw(img, prims, W, H):
    """dgs_draw_prims on a host image and record list with a DIRTY owner (every word 0xFFFFFFFF): the painted bytes."""
    import torch
    from deblurgs_amd import _lib
    from deblurgs_amd.raster_call import _stream
    dev = torch.from_numpy(img).cuda()
    recs = torch.from_numpy(np.ascontiguousarray(prims, dtype=np.int32)).cuda()
    owner = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().dgs_draw_prims(ctypes.c_void_p(dev.data_ptr()), W, H, ctypes.c_void_p(recs.data_ptr()),
                                         int(recs.shape[0]), ctypes.c_void_p(owner.data_ptr()), _stream(dev.device)),
               "dgs_draw_prims")
    return dev.cpu().numpy()


# ------------------------------------------------------------------------------------------------- 1. dgs_draw_prims
@pytest.mark.parametrize("name", sorted(CASES))
def test_draw_equals_the_painter_byte_for_byte(gpu, name):
    prims = CASES[name]
    img = pc.canvas(seed=len(name))
    want = pc.paint(img, prims)
    got = _draw_raw(img, prims, pc.W, pc.H)
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(axis=2))[:8])
    assert (want != img).any() == (name != "outside"), name       # every case but that one draws something


def test_draw_tie_cases_differ_as_the_rule_says(gpu):
    img = np.zeros((pc.H, pc.W, 3), dtype=np.uint8)
    fwd = _draw_raw(img, CASES["tie forward"], pc.W, pc.H).any(axis=2)
    bwd = _draw_raw(img, CASES["tie backward"], pc.W, pc.H).any(axis=2)
    assert sorted(map(tuple, np.argwhere(fwd)[:, ::-1].tolist())) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]
    assert sorted(map(tuple, np.argwhere(bwd)[:, ::-1].tolist())) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]


def test_draw_skips_what_it_must_and_leaves_the_image_alone(gpu):
    img = pc.canvas(seed=3)
    for name in ("beyond the limit", "negative radius"):
        prims = CASES[name]
        dead = np.array([pc.skipped(r) for r in prims.tolist()])
        assert dead.any() and not dead.all()
        assert np.array_equal(_draw_raw(img, prims[dead], pc.W, pc.H), img), name
        assert np.array_equal(_draw_raw(img, prims, pc.W, pc.H), pc.paint(img, prims[~dead])), name


def test_draw_highest_index_wins(gpu):
    img = np.zeros((pc.H, pc.W, 3), dtype=np.uint8)
    got = _draw_raw(img, CASES["three on one pixel"], pc.W, pc.H)
    assert got[10, 30].tolist() == [200, 100, 50] and got[12, 30].tolist() == [9, 8, 7] and got[10, 5].tolist() == [255, 0, 0]
    assert got[9, 29].tolist() == [9, 8, 7] and got[5, 30].tolist() == [0, 255, 0]


def test_draw_twice_gives_equal_bytes_and_the_wrapper_reuses_its_scratch(gpu):
    import torch
    from deblurgs_amd import progress
    img = pc.canvas(seed=9)
    prims = CASES["random"]
    want = pc.paint(img, prims)
    recs = torch.from_numpy(prims).cuda()
    outs = []
    for _ in range(2):
        dev = torch.from_numpy(img).cuda()
        assert progress.draw(dev, recs) is dev
        outs.append(dev.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want)
    owner = progress._owner_cache[str(recs.device)]
    progress.draw(torch.from_numpy(img).cuda(), recs[:0])                  # n = 0 touches nothing
    assert progress._owner_cache[str(recs.device)] is owner


def test_draw_a_full_hd_frame_with_4000_segments(gpu):
    W, H = 1920, 1080
    prims = pc.large_case(4000, W, H)
    img = pc.canvas(seed=1, w=W, h=H)
    want = pc.paint_lines_batched(img, prims)
    got = _draw_raw(img, prims, W, H)
    assert np.array_equal(got, want)
    assert (want != img).any(axis=2).sum() > 100000


# ------------------------------------------------------------------------------------------------- 2. dgs_cone_segments
def _motion(n_views, K, H, W, fovx, fovy, seed, spread=0.3):
    import torch
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    torch.manual_seed(seed)
    ref = RefCamera(W, H, fovx, fovy, device="cuda")
    gt = torch.rand(n_views, 3, H, W, device="cuda")
    se3 = torch.randn(n_views, 6) * torch.tensor([spread] * 3 + [0.2] * 3)
    return CameraMotionModule(ref, gt, curve_order=3, num_subframes=K, init_se3=se3, device="cuda")


def _render_cam(ref, eye, lookat):
    from deblurgs_amd import progress, render_path
    return render_path.c2w_to_cam(progress._shell(ref, "cuda"), render_path.c2w_from_eye(eye, lookat, [0.0, 1.0, 0.0]))


CONE_SEEDS = tuple(range(20, 29))       # 9 x 12 cameras x 10 coordinates: the 1-in-1000 cap allows one exempt coordinate


def test_cone_segments_equal_the_float64_restatement(gpu):
    import math
    import torch
    from deblurgs_amd import progress
    W, H, fovx, fovy, scale = 160, 120, 0.9, 0.7, 0.5
    total = exempt = 0
    for seed in CONE_SEEDS:
        motion = _motion(1, 5, H, W, fovx, fovy, seed)
        with torch.no_grad():
            view, _, campos = motion.get_trajectory_matrices(0, torch.linspace(0.0, 1.0, 12, device="cuda"))
        cam = _render_cam(motion.ref_cam, [0.4, -0.3, -4.0 - 0.1 * seed], [0.0, 0.0, 1.0])
        rgb = torch.arange(100, 112, dtype=torch.int32, device="cuda")
        got = progress.cone_segments(view, campos, math.tan(fovx / 2), math.tan(fovy / 2), scale, cam.world_view_transform,
                                     cam.full_proj_transform, W, H, rgb).cpu().numpy().reshape(12, 8, 6)
        pix, skip = pc.cone_reference(view.cpu().numpy(), campos.cpu().numpy(), math.tan(fovx / 2), math.tan(fovy / 2), scale,
                                      cam.world_view_transform.cpu().numpy(), cam.full_proj_transform.cpu().numpy(), W, H)
        assert not skip.any() and np.isfinite(pix).all()
        assert (got[:, :, 4] == 0).all() and (got[:, :, 5] == np.arange(100, 112)[:, None]).all()
        near = np.abs(pix - np.rint(pix)) <= 1e-7 * np.maximum(1.0, np.abs(pix))            # [12,5,2]
        want = pix.astype(int)
        total += near.size
        exempt += int(near.sum())
        for e, (i, j) in enumerate(pc.CONNECTIVITY):
            for at, v in ((0, i), (2, j)):
                same = (got[:, e, at:at + 2] == want[:, v]) | near[:, v]
                assert same.all(), (seed, e, got[:, e], want[:, v])
        assert (np.abs(want) < 4000).all() and (want[..., 0] >= 0).any()      # the cones are on or near the image
    print(f"cone endpoints: {exempt} of {total} coordinates within 1e-7 of an integer")
    assert exempt * 1000 <= total


def test_cone_segments_skip_test_is_the_reference_s(gpu):
    """The reference takes the camera-LOCAL cone through the render camera's view matrix: a render camera whose view matrix
    puts the local origin behind it trips the test for every camera, wherever the cameras are."""
    import math
    import torch
    from deblurgs_amd import progress
    W, H, fovx, fovy = 160, 120, 0.9, 0.7
    motion = _motion(1, 5, H, W, fovx, fovy, 3)
    with torch.no_grad():
        view, _, campos = motion.get_trajectory_matrices(0, torch.linspace(0.0, 1.0, 12, device="cuda"))
    cam = _render_cam(motion.ref_cam, [0.0, 0.0, 4.0], [0.0, 0.0, 9.0])
    rgb = torch.zeros(12, dtype=torch.int32, device="cuda")
    got = progress.cone_segments(view, campos, math.tan(fovx / 2), math.tan(fovy / 2), 0.5, cam.world_view_transform,
                                 cam.full_proj_transform, W, H, rgb).cpu().numpy()
    _, skip = pc.cone_reference(view.cpu().numpy(), campos.cpu().numpy(), math.tan(fovx / 2), math.tan(fovy / 2), 0.5,
                                cam.world_view_transform.cpu().numpy(), cam.full_proj_transform.cpu().numpy(), W, H)
    assert skip.all() and got.shape == (96, 6) and (got[:, 4] == -1).all()


# ------------------------------------------------------------------------------------------------- 3. overlay, plot, driver
@pytest.fixture(scope="module")
def tiny(gpu):
    """200 Gaussians at 64 x 48, a motion module of 4 views with K = 5 subframes (made once, shared, never written to)."""
    import torch
    from deblurgs_amd.cloud import GaussianCloud
    P, W, H = 200, 64, 48
    sc = synthetic.make_scene(P, W, H, K=3, seed=5, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    motion = _motion(4, 5, H, W, sc["FoVx"], sc["FoVy"], seed=11, spread=0.05)
    motion.link_gaussian(cloud)
    with torch.no_grad():
        motion._nu.add_(0.4 * torch.randn_like(motion._nu))                # an alignment that is no longer the initial one
    return dict(cloud=cloud, motion=motion, bg=torch.tensor([0.2, 0.3, 0.1], device="cuda"), W=W, H=H)


def test_camera_overlay_is_the_finished_render_painted_with_its_records(tiny):
    import torch
    from deblurgs_amd import gaussian_renderer, progress, render_path
    s = tiny
    cam = progress.overview_camera(s["motion"], s["cloud"])
    assert cam.world_view_transform.device.type == "cuda" and int(cam.image_width) == s["W"]
    got = progress.camera_overlay(s["motion"], s["cloud"], cam, s["bg"], "gamma")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (s["H"], s["W"], 3) and got.device.type == "cuda"
    with torch.no_grad():
        plain = render_path.frames_finish(gaussian_renderer.render(cam, s["cloud"], s["bg"])["render"][None], "gamma")[0]
    prims = progress.overlay_prims(s["motion"], cam).cpu().numpy()
    assert prims.shape == (4 * 5 * 8, 6)
    colours = progress.pack_rgb(progress.view_colours(4))
    assert (prims[:, 5].reshape(4, 40) == colours[:, None]).all()
    assert (prims[:, 4] == 0).any()                                       # the overview camera sees the cones
    want = pc.paint(plain.cpu().numpy(), prims)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != plain.cpu().numpy()).any()
    bare = progress.camera_overlay(s["motion"], s["cloud"], cam, s["bg"], "gamma", cones=False)
    assert torch.equal(bare, plain)
    first = progress.overview_camera(s["motion"], s["cloud"], vis_cam_idx=2)
    with torch.no_grad():
        wv, _, _ = s["motion"].get_trajectory_matrices(2, torch.zeros(1, device="cuda"))
    assert torch.equal(first.world_view_transform, wv[0])


def test_alignment_plot_is_the_painter_run_on_the_device_made_records(tiny):
    import torch
    from deblurgs_amd import progress
    s = tiny
    motion, size = s["motion"], (300, 360)
    indices = [0, 1, 3]
    prims = progress.alignment_prims(motion, indices, size)
    assert prims.dtype == torch.int32 and prims.device.type == "cuda"
    host = prims.cpu().numpy()
    K = 5
    assert len(host) == progress.alignment_prim_count(motion, indices) == 3 * (10 + 7 + K + K - 2)
    got = progress.alignment_plot(motion, indices, size)
    assert tuple(got.shape) == (300, 360, 3) and got.dtype == torch.uint8
    white = np.full((300, 360, 3), 255, dtype=np.uint8)
    assert np.array_equal(got.cpu().numpy(), pc.paint(white, host))
    per = 10 + 7 + K + K - 2
    for p, idx in enumerate(indices):
        X0, Y0, X1, Y1 = progress.panel_frame(p, size)
        block = host[p * per:(p + 1) * per]
        assert (block[:17, 4] <= 0).all() and (block[:17, 5] == progress.BLACK).all()
        assert block[:4, :4].tolist() == [[X0, Y0, X1, Y0], [X1, Y0, X1, Y1], [X1, Y1, X0, Y1], [X0, Y1, X0, Y0]]
        lit = "".join(n for n, r in zip("abcdefg", block[10:17, 4]) if r == 0)
        assert sorted(lit) == sorted(progress._SEGMENTS[str(idx)])
        with torch.no_grad():
            nu = motion._sample_nu_from_alignment(idx).cpu().numpy().astype(np.float64)
            pivots = torch.sigmoid(motion._nu[idx].sort().values).cpu().numpy().astype(np.float64)
        for values, rows, radius, rgb in ((nu, block[17:17 + K], 2, progress.BLUE), (pivots, block[17 + K:], 3, progress.RED)):
            m = len(values)
            assert len(rows) == m and (rows[:, 4] == radius).all() and (rows[:, 5] == rgb).all()
            assert (rows[:, 0] == rows[:, 2]).all() and (rows[:, 1] == rows[:, 3]).all()
            x = X0 + (values + 0.05) / 1.1 * (X1 - X0)
            y = Y1 - (np.linspace(0.0, 1.0, m) + 0.1) / 1.2 * (Y1 - Y0)
            assert (np.abs(rows[:, 0] - x) <= 1.0).all() and (np.abs(rows[:, 1] - y) <= 1.0).all()
            assert (rows[:, 0] > X0).all() and (rows[:, 0] < X1).all() and (rows[:, 1] > Y0).all() and (rows[:, 1] < Y1).all()
    # nine panels at most, and the default size
    assert progress.alignment_prim_count(motion, [0, 1, 2, 3] * 3) == 9 * per
    full = progress.alignment_plot(motion, [0, 1, 2, 3])
    assert tuple(full.shape) == (1000, 1200, 3)


def test_progress_visualizer_writes_its_files_at_the_shot_iterations(tiny, tmp_path):
    from deblurgs_amd import jpeg, progress, video
    s = tiny
    model = tmp_path / "model"
    (model / "vis_traj").mkdir(parents=True)
    (model / "vis_traj" / "stale.jpg").write_bytes(b"x")
    vis = progress.ProgressVisualizer(s["motion"], s["cloud"], s["bg"], str(model), 12, tone_mapping="gamma",
                                      n_visualize_shots=3, rng=np.random.default_rng(0))
    shots = [int(i) for i in progress.vis_iterations(12, 3)]
    assert len(set(shots)) == 3 and vis.vis_iters.tolist() == shots
    assert vis.selected_indice.tolist() == [0, 1, 2, 3] and vis.draw_camera
    assert os.listdir(model / "vis_traj") == [] and os.listdir(model / "vis_alignment") == []
    for it in range(1, 13):
        out = vis.run(it)
        assert (out is not None) == (it in shots)
        names = sorted(f"{i:05d}.jpg" for i in shots if i <= it)
        assert sorted(os.listdir(model / "vis_traj")) == names and sorted(os.listdir(model / "vis_alignment")) == names
    paths = vis.save_video()
    assert paths == [str(model / "vis_traj.avi"), str(model / "vis_alignment.avi")]
    for path, folder, (w, h) in zip(paths, ("vis_traj", "vis_alignment"), ((s["W"], s["H"]), (1200, 1000))):
        header, frames = video.parse_avi(open(path, "rb").read())
        assert len(frames) == 3 and header["avih"]["total_frames"] == 3
        assert (header["avih"]["width"], header["avih"]["height"]) == (w, h) and header["strh"]["rate"] == 20
        for frame, it in zip(frames, shots):
            data = open(model / folder / f"{it:05d}.jpg", "rb").read()
            assert frame == data
            kinds = [m for m, _ in jpeg.segments(data)]
            assert kinds[0] == jpeg.SOI and kinds[-1] == jpeg.EOI and 0xC0 in kinds
            assert video.jpeg_size(data) == (w, h)

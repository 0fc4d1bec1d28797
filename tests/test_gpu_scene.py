"""GPU tests of scene loading (deblurgs_amd/scene.py, csrc/scene.hip): dgs_resize_u8 against Pillow's recorded outputs byte
for byte, depth_bounds against the reference's float64 get_bds, and a dataset directory loaded, trained on for three steps."""
import os

import numpy as np
import pytest

import scene_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "scene_golden.npz"))


# ------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("case", sc.RESIZE_CASES, ids=lambda c: c.name)
def test_resize_equals_pillow_byte_for_byte(gpu, golden, case):
    import torch
    from deblurgs_amd import scene
    x = sc.resize_input(case)
    G, C, h, w = case.G, case.C, case.h, case.w
    buf = torch.zeros(x.size + 1, dtype=torch.uint8, device=gpu)           # the input starts at an ODD address
    buf[1:].copy_(torch.from_numpy(x).reshape(-1))
    src = buf[1:].view(G, case.H, case.W, C)
    assert src.data_ptr() % 2 == 1 and src.is_contiguous()
    want = torch.from_numpy(golden["resize_" + case.name])
    want_f = (want / 255.0).permute(0, 3, 1, 2).contiguous()
    size = (w, h)
    # both outputs at once
    out_f = torch.full((G, C, h, w), -1.0, device=gpu)
    out_u = torch.full((G, h, w, C), 7, dtype=torch.uint8, device=gpu)
    got_f, got_u = scene.resize_images(src, size, out=out_f, out_u8=out_u)
    assert got_f is out_f and got_u is out_u
    assert torch.equal(out_u.cpu(), want), int((out_u.cpu() != want).sum())
    assert torch.equal(out_f.cpu(), want_f)                                # bit for bit: from_numpy(u8) / 255.0
    # each alone
    only_f = scene.resize_images(src, size)
    assert only_f.dtype == torch.float32 and torch.equal(only_f.cpu(), want_f)
    only_u = scene.resize_images(src, size, out_u8=torch.empty((G, h, w, C), dtype=torch.uint8, device=gpu))
    assert torch.equal(only_u.cpu(), want)
    # into the middle of a larger stack, and with a stride of two images: the neighbours stay as they were
    stack = torch.full((G + 2, C, h, w), -3.0, device=gpu)
    scene.resize_images(src, size, out=stack[1:G + 1])
    host = stack.cpu()
    assert torch.equal(host[1:G + 1], want_f) and (host[0] == -3.0).all() and (host[-1] == -3.0).all()
    wide = torch.full((G, 2, C, h, w), -5.0, device=gpu)
    scene.resize_images(src, size, out=wide[:, 1])
    host = wide.cpu()
    assert torch.equal(host[:, 1], want_f) and (host[:, 0] == -5.0).all()
    assert (buf.cpu()[1:].reshape(x.shape).numpy() == x).all() and int(buf[0]) == 0          # the input is untouched


def test_pil_to_torch_for_rgb_and_l(gpu, golden):
    import torch
    from deblurgs_amd import scene
    for name in ("odd", "v_only_L"):
        case = next(c for c in sc.RESIZE_CASES if c.name == name)
        x = sc.resize_input(case)[0]
        got = scene.pil_to_torch(x if case.C == 3 else x[:, :, 0], (case.w, case.h))
        want = (torch.from_numpy(golden["resize_" + name][0]) / 255.0).permute(2, 0, 1)
        assert got.shape == (case.C, case.h, case.w) and torch.equal(got.cpu(), want)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        scene.pil_to_torch(np.zeros((8, 8, 5), np.uint8), (4, 4))


def test_pil_to_torch_rgba_takes_pillows_own_path(gpu):
    Image = pytest.importorskip("PIL.Image")
    import torch
    from deblurgs_amd import scene
    x = np.random.default_rng(3).integers(0, 256, (21, 33, 4), dtype=np.uint8)
    got = scene.pil_to_torch(x, (16, 10))
    want = (torch.from_numpy(np.array(Image.fromarray(x).resize((16, 10)))) / 255.0).permute(2, 0, 1)
    assert got.shape == (4, 10, 16) and torch.equal(got.cpu(), want)


def test_resize_wrapper_checks_its_tensors(gpu):
    import torch
    from deblurgs_amd import scene
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="out must be"):
        scene.resize_images(src, (4, 4), out=torch.zeros((2, 3, 4, 5), device=gpu))
    with pytest.raises(ValueError, match="out_u8 must be"):
        scene.resize_images(src, (4, 4), out_u8=torch.zeros((2, 4, 4, 1), dtype=torch.uint8, device=gpu))
    with pytest.raises(RuntimeError, match=r"\[1/64, 64\]"):
        scene.resize_images(torch.zeros((1, 130, 8, 3), dtype=torch.uint8, device=gpu), (8, 2))
    same = scene.resize_images(src + 9, (8, 8))                            # both passes skipped: a conversion
    assert torch.equal(same.cpu(), torch.full((2, 3, 8, 8), 9 / 255.0))


# ------------------------------------------------------------------------------------------------- depth bounds
_BOUNDS = sc.bounds_cases()


@pytest.mark.parametrize("case", _BOUNDS, ids=lambda c: c.name)
def test_depth_bounds_against_get_bds(gpu, golden, case):
    """The validity test runs in double on points kept 1e-9 away from every decision boundary, so the counted sets are the
    reference's; the only rounding is the float32 key of each of the two order statistics a percentile interpolates
    (relative 2^-24 each), and the interpolation is convex: |delta| <= 2^-24 far, asserted with a factor 2."""
    from deblurgs_amd import scene
    got, counts = scene.depth_bounds(case.cams, case.points, return_counts=True)
    want = golden["bds_" + case.name]
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(counts, sc.bounds_valid(case.cams, case.points).sum(axis=1))
    err = np.abs(got - want)
    print("depth_bounds", case.name, "max |delta| / far:", float((err / want[:, 1:2]).max()), "bar", 2.0 ** -23)
    assert (err <= 2.0 ** -23 * want[:, 1:2]).all(), float((err / want[:, 1:2]).max())
    # the cameras in groups of one and all at once: identical bits
    n = len(case.points)
    single = scene.depth_bounds(case.cams, case.points, key_budget_bytes=4 * n)
    whole = scene.depth_bounds(case.cams, case.points, key_budget_bytes=4 * n * len(case.cams))
    assert np.array_equal(single, got) and np.array_equal(whole, got)


def test_depth_bound_keys_are_depths_or_nans(gpu):
    import torch
    from deblurgs_amd import scene
    case = _BOUNDS[0]
    pts = torch.from_numpy(case.points).to(gpu)
    keys, counts = scene.depth_bound_keys(case.cams, pts)
    valid = sc.bounds_valid(case.cams, case.points)
    (z, _, _, _, _), _ = sc.bounds_quantities(case.cams, case.points)
    k = keys.cpu().numpy()
    assert np.array_equal(~np.isnan(k), valid) and np.array_equal(counts.cpu().numpy(), valid.sum(axis=1))
    assert np.array_equal(k[valid], z[valid].astype(np.float32))
    # the FIRST camera's intrinsics serve every camera: another first camera changes the sets
    other = case.cams[0]._replace(width=48, FovX=0.5)
    _, counts2 = scene.depth_bound_keys(case.cams, pts, first=other)
    assert np.array_equal(counts2.cpu().numpy(), sc.bounds_valid([other] + list(case.cams), case.points).sum(axis=1)[1:])


def test_depth_bounds_names_a_camera_that_sees_nothing(gpu):
    from deblurgs_amd import scene
    case = _BOUNDS[0]
    behind = case.points.copy()
    behind[:, 2] = -50.0 - np.abs(behind[:, 2])
    with pytest.raises(ValueError, match=r"camera 0 \(000\) sees none"):
        scene.depth_bounds(case.cams, behind)


# ------------------------------------------------------------------------------------------------- end to end
def _dataset(root, as_png=False):
    """A 4-image dataset from a synthetic scene: its four subframe cameras are the views, renders of its cloud the 96 x 64
    pictures, the first 300 Gaussian centres the COLMAP points.  Returns the uint8 sources by image name."""
    import torch
    from helpers import hip_forward_state, synthetic
    s = synthetic.make_scene(1500, 96, 64, K=4, seed=8, sigma_px=3.0)
    color = hip_forward_state(s, 4)["color"]
    u8 = (np.clip(color, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).transpose(0, 2, 3, 1)
    fx, fy = 96 / (2 * s["tanfovx"]), 64 / (2 * s["tanfovy"])
    names = ["003", "001", "002", "000"]                                   # the images file is not sorted
    images = []
    for k, name in enumerate(names):
        view = s["viewmatrix"][k].astype(np.float64)                       # row-vector world-to-view
        images.append((k + 1, [float(v) for v in sc.quat_of(view[:3, :3].T)], [float(v) for v in view[3, :3]], 1,
                       name + ".png", []))
    rng = np.random.default_rng(2)
    points = [(p + 1, [float(v) for v in s["means3D"][p]], [int(v) for v in rng.integers(0, 256, 3)],
               float(rng.uniform(0.1, 2.0)), []) for p in range(300)]
    sc.write_model(os.path.join(str(root), "sparse", "0"), [(1, "PINHOLE", 96, 64, [fx, fy, 48.0, 32.0])], images, points)
    os.makedirs(os.path.join(str(root), "images"))
    sources = {}
    for k, name in enumerate(names):
        sources[name] = np.ascontiguousarray(u8[k])
        if as_png:
            from PIL import Image
            Image.fromarray(sources[name]).save(os.path.join(str(root), "images", name + ".png"))
        else:
            np.save(os.path.join(str(root), "images", name + ".npy"), sources[name])
    torch.cuda.synchronize()
    return sources, points


def _train_three_steps(data):
    import torch
    from deblurgs_amd.training import TrainingLoop, default_optimization_params
    torch.manual_seed(0)
    motion = data.motion_module(curve_order=3, num_subframes=5)
    cloud = data.cloud(sh_degree=2)
    motion.link_gaussian(cloud)
    opt = default_optimization_params(iterations=10, curve_start_iter=2, densify_from_iter=100)
    loop = TrainingLoop(cloud, motion, opt, data.cameras_extent)
    for it in range(1, 4):
        out = loop.step(it, (it - 1) % len(data.image_names))
        assert torch.isfinite(out["loss"]), it
    return cloud


def _check_loaded(data, sources, device):
    import torch
    names = sorted(sources)
    assert data.image_names == names and data.test_images is None and data.test_c2w is None
    stack = np.stack([sources[n] for n in names])
    want = (torch.from_numpy(sc.resize_restated(stack, (48, 32))) / 255.0).permute(0, 3, 1, 2)
    assert data.gt_images.shape == (4, 3, 32, 48) and data.gt_images.device.type == "cuda"
    assert torch.equal(data.gt_images.cpu(), want)                         # the Pillow route, bit for bit
    assert (data.ref_cam.image_width, data.ref_cam.image_height) == (48, 32)
    rot, pos = data.init_c2w
    assert rot.shape == (4, 3, 3) and pos.shape == (4, 3) and rot.dtype == torch.float64
    assert data.cameras_extent > 0.0


def test_load_colmap_scene_end_to_end(gpu, tmp_path):
    from deblurgs_amd import scene
    sources, points = _dataset(tmp_path)
    before = sorted(os.listdir(os.path.join(str(tmp_path), "sparse", "0")))
    data = scene.load_colmap_scene(str(tmp_path), resolution=2, image_reader=np.load)
    _check_loaded(data, sources, gpu)
    assert data.points.dtype == np.float32 and data.points.shape == (300, 3) and data.colors.shape == (300, 3)
    assert np.array_equal(data.points, np.array([p[1] for p in points]).astype(np.float32))
    assert np.array_equal(data.colors, np.array([p[2] for p in points]) / 255.0)
    cloud = _train_three_steps(data)
    assert cloud._xyz.shape[0] == 300
    assert sorted(os.listdir(os.path.join(str(tmp_path), "sparse", "0"))) == before            # nothing is written
    # the default reader finds the .npy pictures too; a held-out split shares the training size
    data = scene.load_colmap_scene(str(tmp_path), resolution=2, eval=True, llffhold=2)
    assert data.image_names == ["001", "003"] and data.test_names == ["000", "002"]
    assert data.test_images.shape == (2, 3, 32, 48) and data.test_c2w[0].shape == (2, 3, 3)


def test_load_colmap_scene_random_init(gpu, tmp_path):
    from deblurgs_amd import scene
    sources, _ = _dataset(tmp_path)
    np.random.seed(5)
    data = scene.load_colmap_scene(str(tmp_path), resolution=2, random_init=True, image_reader=np.load, num_random_points=3000)
    _check_loaded(data, sources, gpu)
    assert data.points.shape == (3000, 3) and np.isfinite(data.points).all() and data.points.flags.c_contiguous
    assert np.array_equal(data.colors, np.full((3000, 3), 2 / 255.0))      # 0.01 through RGB2SH / SH2RGB and the ply's uint8
    np.random.seed(5)
    again = scene.load_colmap_scene(str(tmp_path), resolution=2, random_init=True, image_reader=np.load, num_random_points=3000)
    assert np.array_equal(again.points, data.points)
    assert again.cameras_extent == scene.nerfpp_radius(scene.camera_centers(data.train_cameras))
    _train_three_steps(data)


def test_load_colmap_scene_reads_png_through_pil(gpu, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import torch
    from deblurgs_amd import scene
    sources, _ = _dataset(tmp_path, as_png=True)
    data = scene.load_colmap_scene(str(tmp_path), resolution=2)
    _check_loaded(data, sources, gpu)
    names = sorted(sources)
    pil = np.stack([np.asarray(Image.fromarray(sources[n]).resize((48, 32))) for n in names])
    assert torch.equal(data.gt_images.cpu(), (torch.from_numpy(pil) / 255.0).permute(0, 3, 1, 2))

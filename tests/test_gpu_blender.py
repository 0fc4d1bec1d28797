"""GPU tests of Blender scene loading (deblurgs_amd/scene.py, csrc/scene.hip): dgs_rgba_over_u8 on every (colour, alpha)
pair against the golden float64 tables, dgs_resize_rgba_u8 against PIL's recorded RGBA resizes byte for byte, the RGBA
routes of pil_to_torch and _load_images, and a NeRF-synthetic directory loaded and trained on for three steps.  Every
comparison is an equality of bytes or of bits."""
import os
import sys

import numpy as np
import pytest

import blender_cases as bc
import scene_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "blender_golden.npz"))


def _at_odd_address(x, device):
    import torch
    buf = torch.zeros(x.size + 1, dtype=torch.uint8, device=device)
    buf[1:].copy_(torch.from_numpy(x).reshape(-1))
    src = buf[1:].view(*x.shape)
    assert src.data_ptr() % 2 == 1 and src.is_contiguous()
    return buf, src


def _planes(u8):
    """torch.from_numpy(bytes) / 255.0 as float planes [G,C,H,W]."""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(u8)) / 255.0).permute(0, 3, 1, 2).contiguous()


def _check_outputs(fn, src, want_u8, device):
    """fn(src, out=, out_u8=) under resize_images' output rules: both outputs at once, each alone, the middle of a larger
    stack and a stride of two images."""
    import torch
    G, h, w, C = want_u8.shape
    want = torch.from_numpy(want_u8)
    want_f = _planes(want_u8)
    out_f = torch.full((G, C, h, w), -1.0, device=device)
    out_u = torch.full((G, h, w, C), 7, dtype=torch.uint8, device=device)
    got_f, got_u = fn(src, out=out_f, out_u8=out_u)
    assert got_f is out_f and got_u is out_u
    assert torch.equal(out_u.cpu(), want), int((out_u.cpu() != want).sum())
    assert torch.equal(out_f.cpu(), want_f)                                # bit for bit: from_numpy(u8) / 255.0
    only_f = fn(src)
    assert only_f.dtype == torch.float32 and torch.equal(only_f.cpu(), want_f)
    only_u = fn(src, out_u8=torch.empty((G, h, w, C), dtype=torch.uint8, device=device))
    assert torch.equal(only_u.cpu(), want)
    odd_u = torch.full((G * h * w * C + 1,), 7, dtype=torch.uint8, device=device)      # a byte output at an odd address
    fn(src, out_u8=odd_u[1:])
    assert torch.equal(odd_u[1:].cpu().view(G, h, w, C), want) and int(odd_u[0]) == 7
    stack = torch.full((G + 2, C, h, w), -3.0, device=device)
    fn(src, out=stack[1:G + 1])
    host = stack.cpu()
    assert torch.equal(host[1:G + 1], want_f) and (host[0] == -3.0).all() and (host[-1] == -3.0).all()
    wide = torch.full((G, 2, C, h, w), -5.0, device=device)
    fn(src, out=wide[:, 1])
    host = wide.cpu()
    assert torch.equal(host[:, 1], want_f) and (host[:, 0] == -5.0).all()


# ------------------------------------------------------------------------------------------------- composite
@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
def test_composite_equals_the_float64_expression_on_every_pair(gpu, golden, white):
    import torch
    from deblurgs_amd import scene
    table = golden["over_white" if white else "over_black"]
    x = bc.over_pairs()[None]                                              # [1,256,256,4]: alpha by row, colour by column
    buf, src = _at_odd_address(x, gpu)
    want = np.stack([table, np.roll(table, -85, axis=1), np.roll(table, -170, axis=1)], axis=-1)[None]
    assert np.array_equal(want, bc.over_from_table(table, x))              # channel k carries colour (c + 85 k) % 256
    got = scene.rgba_over(src, white, out_u8=torch.empty((1, 256, 256, 3), dtype=torch.uint8, device=gpu)).cpu().numpy()
    print("bytes that differ from the golden table:", int((got != want).sum()), "of", want.size)
    _check_outputs(lambda s, **kw: scene.rgba_over(s, white, **kw), src, want, gpu)
    assert (buf.cpu()[1:].reshape(x.shape).numpy() == x).all() and int(buf[0]) == 0          # the input is untouched


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("aligned", [False, True], ids=["odd_address", "aligned"])
def test_composite_tail_and_image_stride(gpu, golden, white, aligned):
    """G = 3 images of 5 x 7: 105 pixels -- a tail of the 4 pixels a thread takes, planes of 35 floats that no group of 4
    pixels lines up with, and an image stride.  From an aligned address (the 16-byte loads) and from an odd one."""
    import torch
    from deblurgs_amd import scene
    table = golden["over_white" if white else "over_black"]
    x = np.random.default_rng(31).integers(0, 256, (3, 5, 7, 4), dtype=np.uint8)
    x[0, 0, :3, 3] = (0, 255, 1)
    if aligned:
        buf = src = torch.from_numpy(x).to(gpu)
        assert src.data_ptr() % 16 == 0
    else:
        buf, src = _at_odd_address(x, gpu)
    _check_outputs(lambda s, **kw: scene.rgba_over(s, white, **kw), src, bc.over_from_table(table, x), gpu)
    single = scene.rgba_over(src[1], white)                                # one [H,W,4] image
    assert single.shape == (1, 3, 5, 7) and torch.equal(single.cpu(), _planes(bc.over_from_table(table, x[1:2])))
    assert (buf.cpu().numpy().reshape(-1)[-x.size:].reshape(x.shape) == x).all()


def test_composite_crosses_block_borders(gpu, golden):
    """2 images of 33 x 47: 3102 pixels, four blocks of 1024, the image border inside a block."""
    import torch
    from deblurgs_amd import scene
    x = np.random.default_rng(32).integers(0, 256, (2, 33, 47, 4), dtype=np.uint8)
    for white in (False, True):
        want = bc.over_from_table(golden["over_white" if white else "over_black"], x)
        _check_outputs(lambda s, **kw: scene.rgba_over(s, white, **kw), torch.from_numpy(x).to(gpu), want, gpu)


def test_composite_wrapper_checks_its_tensors(gpu):
    import torch
    from deblurgs_amd import scene
    src = torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match=r"uint8 \[G,H,W,4\]"):
        scene.rgba_over(src[..., :3], False)
    with pytest.raises(ValueError, match=r"uint8 \[G,H,W,4\]"):
        scene.resize_rgba_images(src[..., :3], (4, 4))
    with pytest.raises(ValueError, match="out must be"):
        scene.rgba_over(src, False, out=torch.zeros((2, 4, 8, 8), device=gpu))
    with pytest.raises(ValueError, match="out_u8 must be"):
        scene.rgba_over(src, False, out_u8=torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=gpu))
    with pytest.raises(RuntimeError, match=r"\[1/64, 64\]"):
        scene.resize_rgba_images(torch.zeros((1, 130, 8, 4), dtype=torch.uint8, device=gpu), (8, 2))


# ------------------------------------------------------------------------------------------------- RGBA resize
@pytest.mark.parametrize("case", bc.RGBA_CASES, ids=lambda c: c.name)
def test_rgba_resize_equals_pillow_byte_for_byte(gpu, golden, case):
    import torch
    from deblurgs_amd import scene
    x = bc.rgba_input(case)
    buf, src = _at_odd_address(x, gpu)
    want = golden["rgba_" + case.name]
    got = scene.resize_rgba_images(src, (case.w, case.h), out_u8=torch.empty(want.shape, dtype=torch.uint8, device=gpu))
    got = got.cpu().numpy()
    print(case.name, "bytes that differ from PIL's:", int((got != want).sum()), "of", want.size)
    _check_outputs(lambda s, **kw: scene.resize_rgba_images(s, (case.w, case.h), **kw), src, want, gpu)
    if case.name == "same":
        assert tuple(got[0, 0, 0]) == (9, 8, 7, 0)                         # the colour under alpha 0 survives the copy
    assert (buf.cpu()[1:].reshape(x.shape).numpy() == x).all() and int(buf[0]) == 0          # the input is untouched


def test_pil_to_torch_rgba_needs_no_pil(gpu, golden, monkeypatch):
    import torch
    from deblurgs_amd import scene
    case = next(c for c in bc.RGBA_CASES if c.name == "odd")
    x = bc.rgba_input(case)[0]
    want = _planes(golden["rgba_odd"])[0]
    with_pil = scene.pil_to_torch(x, (case.w, case.h))
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError):
        from PIL import Image  # noqa: F401
    got = scene.pil_to_torch(x, (case.w, case.h))
    assert got.shape == (4, case.h, case.w) and got.device.type == "cuda"
    assert torch.equal(got.cpu(), want) and torch.equal(with_pil.cpu(), want)
    with pytest.raises(RuntimeError, match="LA"):                           # two channels stay on the host route
        scene.pil_to_torch(x[:, :, :2], (case.w, case.h))


def test_load_images_keeps_rgba_in_its_batches(gpu, tmp_path, monkeypatch):
    """A mixed list of RGB and RGBA pictures: what the route of one image at a time gave, pil_to_torch(img)[:3], and what
    the restatements of Pillow give."""
    import torch
    from deblurgs_amd import scene
    rng = np.random.default_rng(12)
    images, cams = [], []
    for i, C in enumerate((3, 4, 4, 3, 4, 4, 4)):
        img = bc.rgba_input(bc.RgbaCase("odd", 37, 53, 18, 26, 1, ""))[0] if i == 1 else \
            rng.integers(0, 256, (37, 53, C), dtype=np.uint8)
        path = str(tmp_path / f"{i:03d}.npy")
        np.save(path, img)
        images.append(img)
        cams.append(sc.Cam(1, np.eye(3), np.zeros(3), 0.8, 1.1, path, f"{i:03d}", 53, 37))
    uploads = []
    real = scene.resize_rgba_images

    def counted(src, *a, **kw):
        uploads.append(int(src.shape[0]))
        return real(src, *a, **kw)
    monkeypatch.setattr(scene, "resize_rgba_images", counted)
    for resolution, size in ((2, (26, 18)), (1, (53, 37))):
        uploads.clear()
        got = scene._load_images(cams, resolution, np.load, gpu, "training")
        assert uploads == [2, 3]                                           # the RGBA pictures travel in groups
        assert got.shape == (7, 3, size[1], size[0]) and got.dtype == torch.float32
        for i, img in enumerate(images):
            assert torch.equal(got[i], scene.pil_to_torch(img, size)[:3]), i
            restated = bc.resize_rgba_restated(img[None], size) if img.shape[2] == 4 else sc.resize_restated(img[None], size)
            assert torch.equal(got[i].cpu(), _planes(restated)[0, :3]), i
    np.save(cams[3].image_path, images[3][:-1])
    with pytest.raises(ValueError, match="share one size"):
        scene._load_images(cams, 2, np.load, gpu, "training")


# ------------------------------------------------------------------------------------------------- end to end
def _train_three_steps(data):
    import torch
    from deblurgs_amd.training import TrainingLoop, default_optimization_params
    torch.manual_seed(0)
    motion = data.motion_module(curve_order=3, num_subframes=5)
    cloud = data.cloud(sh_degree=2)
    motion.link_gaussian(cloud)
    opt = default_optimization_params(iterations=10, curve_start_iter=2, densify_from_iter=100)
    loop = TrainingLoop(cloud, motion, opt, data.cameras_extent, white_background=data.white_background)
    for it in range(1, 4):
        out = loop.step(it, (it - 1) % len(data.image_names))
        assert torch.isfinite(out["loss"]), it
    return cloud


def _want_images(golden, sources, white, size=None):
    over = bc.over_from_table(golden["over_white" if white else "over_black"], np.stack(sources))
    return _planes(over if size is None else sc.resize_restated(over, size))


def test_load_blender_scene_end_to_end(gpu, tmp_path, golden):
    import torch
    from deblurgs_amd import scene
    sources = bc.write_blender_dir(tmp_path)                               # 4 train and 2 test views, 40 x 32 RGBA
    before = sorted(os.listdir(str(tmp_path)))
    train, test = list(sources["train"].values()), list(sources["test"].values())
    for white in (True, False):
        np.random.seed(5)
        data = scene.load_blender_scene(str(tmp_path), white_background=white, resolution=1, num_random_points=3000)
        assert data.white_background is white and data.test_images is None and data.test_c2w is None
        assert data.image_names == ["r_0", "r_1", "r_2", "r_3", "r_0", "r_1"] and data.test_names == []
        assert data.gt_images.shape == (6, 3, 32, 40) and data.gt_images.device.type == "cuda"
        assert torch.equal(data.gt_images.cpu(), _want_images(golden, train + test, white))
        half = scene.load_blender_scene(str(tmp_path), white_background=white, resolution=2, eval=True, num_random_points=3000)
        assert torch.equal(half.gt_images.cpu(), _want_images(golden, train, white, (20, 16)))
        assert torch.equal(half.test_images.cpu(), _want_images(golden, test, white, (20, 16)))
    assert not torch.equal(_want_images(golden, train, True), _want_images(golden, train, False))
    # the eval split, the poses, the field of view
    assert half.image_names == ["r_0", "r_1", "r_2", "r_3"] and half.test_names == ["r_0", "r_1"]
    assert (half.ref_cam.image_width, half.ref_cam.image_height) == (20, 16)
    rot, pos = half.init_c2w
    assert rot.dtype == torch.float64 and np.array_equal(rot.numpy(), golden["cam_R"])
    assert np.array_equal(pos.numpy(), np.stack([-golden["cam_T"][i] @ golden["cam_R"][i].T for i in range(4)]))
    assert np.abs(np.linalg.norm(pos.numpy(), axis=1) - 4.0).max() <= 1e-12
    assert half.test_c2w[0].shape == (2, 3, 3) and len(half.test_cameras) == 2
    fov_x, fov_y = golden["cam_fov"]
    assert all(c.FovX == fov_x and c.FovY == fov_y and (c.width, c.height) == (40, 32) for c in half.train_cameras)
    # the random cloud of the six views, the radius from the cameras alone
    cams = data.train_cameras
    assert len(cams) == 6 and data.points.shape == (3000, 3) and data.points.dtype == np.float32
    np.random.seed(5)
    xyz, rgb = scene.blender_random_cloud(cams, 3000)
    assert np.array_equal(data.points, xyz.astype(np.float32)) and np.array_equal(data.colors, np.full((3000, 3), 127 / 255.0))
    assert data.cameras_extent == scene.nerfpp_radius(scene.camera_centers(cams)) > 0.0
    assert (data.ref_cam.image_width, data.ref_cam.image_height) == (40, 32)
    cloud = _train_three_steps(data)
    assert cloud._xyz.shape[0] == 3000
    assert sorted(os.listdir(str(tmp_path))) == before                     # nothing is written
    # an RGB picture among the RGBA ones skips the composite: alpha 255 is the identity
    rgb_dir = tmp_path / "rgb"
    mixed = bc.write_blender_dir(rgb_dir, rgb_views=(("train", "r_2"),))
    opaque = [np.concatenate([v[:, :, :3], np.full_like(v[:, :, 3:], 255)], axis=2) if k == "r_2" else v
              for k, v in mixed["train"].items()]
    got = scene.load_blender_scene(str(rgb_dir), white_background=True, resolution=2, eval=True, num_random_points=3000)
    assert torch.equal(got.gt_images.cpu(), _want_images(golden, opaque, True, (20, 16)))


def test_load_blender_scene_reads_points3d_ply(gpu, tmp_path):
    from deblurgs_amd import scene
    bc.write_blender_dir(tmp_path)
    rng = np.random.default_rng(9)
    v = np.zeros(50, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                            ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k in ("x", "y", "z"):
        v[k] = rng.normal(0, 0.5, 50).astype(np.float32)
    for k in ("red", "green", "blue"):
        v[k] = rng.integers(0, 256, 50)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 50\n" + \
        "".join(f"property {'uchar' if v.dtype[n] == np.uint8 else 'float'} {n}\n" for n in v.dtype.names) + "end_header\n"
    with open(str(tmp_path / "points3d.ply"), "wb") as f:
        f.write(header.encode("ascii") + v.tobytes())
    state = np.random.get_state()[1].copy()
    data = scene.load_blender_scene(str(tmp_path), resolution=4)
    assert np.array_equal(np.random.get_state()[1], state)                 # no draw from the global generator
    assert np.array_equal(data.points, np.stack([v["x"], v["y"], v["z"]], axis=1)) and data.points.flags.c_contiguous
    assert np.array_equal(data.colors, np.stack([v["red"], v["green"], v["blue"]], axis=1) / 255.0)
    assert data.gt_images.shape == (6, 3, 8, 10) and data.white_background is False


def test_load_scene_picks_the_reader(gpu, tmp_path, monkeypatch):
    import torch
    from deblurgs_amd import scene
    blender = tmp_path / "blender"
    bc.write_blender_dir(blender)
    np.random.seed(5)
    data = scene.load_scene(str(blender), white_background=True, eval=True, resolution=2, num_random_points=3000)
    np.random.seed(5)
    want = scene.load_blender_scene(str(blender), white_background=True, eval=True, resolution=2, num_random_points=3000)
    assert data.white_background is True and torch.equal(data.gt_images, want.gt_images)
    assert np.array_equal(data.points, want.points) and data.test_names == ["r_0", "r_1"]
    # a `sparse` directory wins, as in the reference -- even next to a transforms file
    calls = []
    monkeypatch.setattr(scene, "load_colmap_scene", lambda path, **kw: calls.append((path, kw)) or "colmap")
    os.makedirs(str(blender / "sparse"))
    assert scene.load_scene(str(blender), resolution=2) == "colmap" and calls == [(str(blender), {"resolution": 2})]
    bounds = tmp_path / "llff"
    os.makedirs(str(bounds))
    np.save(str(bounds / "poses_bounds.npy"), np.zeros((2, 17)))
    assert scene.load_scene(str(bounds)) == "colmap" and len(calls) == 2

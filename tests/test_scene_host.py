"""CPU tests of scene loading (deblurgs_amd/scene.py, colmap_io.py, csrc/scene.hip): the new entry points are declared,
exported, bound and refuse bad arguments before any HIP call; the coefficient tables (host code of the library) against the
numpy restatement of Pillow; the restatement against the Pillow golden; the COLMAP readers, the resolution rule, the scene
radius, the random initialisation, the split and the prune against the reference's recorded results."""
import math
import os
import re

import numpy as np
import pytest

import scene_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_resample_ksize", "dgs_resample_coeffs", "dgs_resize_u8", "dgs_depth_bound_keys")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "scene_golden.npz"))


def test_new_symbols_are_declared_exported_and_bound():
    from deblurgs_amd import _lib, build
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s) and (s + "(") in header, s
        assert getattr(L, s).argtypes == _lib.EXPORTS[s][1]
    assert L.dgs_abi_version() == 15 and _lib.ABI_VERSION == 15            # additions to ABI 15
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", header).group(1)) == 15
    assert build.SOURCES.get("scene.hip") == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(ROOT, "deblurgs_amd", "csrc", "scene.hip"))


# ------------------------------------------------------------------------------------------------- coefficient tables
def _axis_pairs():
    pairs = set(sc.EXTRA_COEFF_SIZES)
    for c in sc.RESIZE_CASES:
        pairs.update(((c.W, c.w), (c.H, c.h)))
    return sorted(pairs)


@pytest.mark.parametrize("sizes", _axis_pairs(), ids=lambda s: f"{s[0]}to{s[1]}")
def test_resample_coeffs_equal_the_restatement(sizes):
    from deblurgs_amd import _lib, scene
    kk, bounds = scene.resample_coeffs(*sizes)
    want_kk, want_bounds = sc.resample_coeffs(*sizes)
    assert _lib.lib().dgs_resample_ksize(*sizes) == sc.resample_ksize(*sizes) == want_kk.shape[1]
    assert kk.dtype == np.int32 and kk.shape == want_kk.shape and np.array_equal(kk, want_kk)
    assert np.array_equal(bounds, want_bounds)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= sizes[0]).all() and (bounds[:, 1] <= kk.shape[1]).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()     # what the kernel's row range relies on
    assert (np.abs(kk.sum(axis=1) - (1 << 22)) <= kk.shape[1]).all()                           # taps sum to 1 up to their rounding


def test_resample_coeffs_argument_errors():
    from deblurgs_amd import _lib
    L = _lib.lib()
    kk = np.zeros(4096, np.int32)
    bounds = np.zeros(4096, np.int32)

    def call(i=37, o=18, k=kk.ctypes.data, cap=kk.size, b=bounds.ctypes.data):
        return L.dgs_resample_coeffs(i, o, k, cap, b)

    assert call() == 0
    for kw, text in (({"k": None}, b"null"), ({"b": None}, b"null"), ({"i": 0}, b"1..65536"), ({"o": 0}, b"1..65536"),
                     ({"o": -3}, b"1..65536"), ({"i": 65537}, b"1..65536"), ({"i": 650, "o": 10}, b"[1/64, 64]"),
                     ({"i": 10, "o": 641}, b"[1/64, 64]"), ({"cap": 18 * 11 - 1}, b"fewer than"), ({"cap": 0}, b"fewer than")):
        assert call(**kw) == -1, kw
        assert text in L.dgs_last_error(), (kw, L.dgs_last_error())
    assert call(i=640, o=10, cap=10 * 257) == 0 and call(i=10, o=640) == 0          # the ends of the range are inside it
    assert L.dgs_resample_ksize(640, 10) == 257 and L.dgs_resample_ksize(10, 640) == 5
    assert L.dgs_resample_ksize(650, 10) == L.dgs_resample_ksize(0, 10) == L.dgs_resample_ksize(10, 0) == 0
    with pytest.raises(RuntimeError, match="dgs_resample_coeffs failed"):
        from deblurgs_amd import scene
        scene.resample_coeffs(650, 10)


def test_resize_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096          # non-null, aligned dummies: only the argument logic runs
    ok = dict(src=a + 1, G=2, H=37, W=53, C=3, h=18, w=26, kh=a, bh=a, kv=a, bv=a, u8=a + 3, f32=a, stride=3 * 18 * 26)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_resize_u8(v["src"], v["G"], v["H"], v["W"], v["C"], v["h"], v["w"], v["kh"], v["bh"], v["kv"], v["bv"],
                               v["u8"], v["f32"], v["stride"], None)

    for kw, text in (({"src": None}, b"null input"), ({"u8": None, "f32": None}, b"both outputs"),
                     ({"G": 0}, b"G must be"), ({"G": -1}, b"G must be"),
                     ({"C": 0}, b"C must be 1 or 3"), ({"C": 2}, b"C must be 1 or 3"), ({"C": 4}, b"C must be 1 or 3"),
                     ({"H": 0}, b"1..65536"), ({"w": 0}, b"1..65536"), ({"W": 70000}, b"1..65536"), ({"h": -2}, b"1..65536"),
                     ({"H": 1300, "h": 20}, b"[1/64, 64]"), ({"W": 10, "w": 700}, b"[1/64, 64]"),
                     ({"kh": None}, b"null horizontal"), ({"bh": None}, b"null horizontal"),
                     ({"kv": None}, b"null vertical"), ({"bv": None}, b"null vertical"),
                     ({"kh": a + 2}, b"4-byte aligned"), ({"bv": a + 1}, b"4-byte aligned"), ({"f32": a + 2}, b"4-byte aligned"),
                     ({"stride": 3 * 18 * 26 - 1}, b"stride")):
        assert call(**kw) == -1, kw
        assert text in L.dgs_last_error(), (kw, L.dgs_last_error())
    with pytest.raises(RuntimeError, match="dgs_resize_u8 failed"):
        _lib.check(call(C=2), "dgs_resize_u8")


def test_depth_bound_keys_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096
    ok = dict(pts=a, n=500, w2c=a, m=3, w=96.0, h=64.0, fx=80.0, fy=75.0, keys=a, counts=a)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_depth_bound_keys(v["pts"], v["n"], v["w2c"], v["m"], v["w"], v["h"], v["fx"], v["fy"], v["keys"],
                                      v["counts"], None)

    for kw, text in (({"pts": None}, b"null"), ({"w2c": None}, b"null"), ({"keys": None}, b"null"), ({"counts": None}, b"null"),
                     ({"n": 0}, b"n must be"), ({"n": -4}, b"n must be"), ({"m": 0}, b"m must be"), ({"m": -1}, b"m must be"),
                     ({"m": 65536}, b"m must be"), ({"w": 0.0}, b"positive and finite"), ({"fx": -1.0}, b"positive and finite"),
                     ({"fy": float("nan")}, b"positive and finite"), ({"h": float("inf")}, b"positive and finite"),
                     ({"pts": a + 4}, b"8-byte aligned"), ({"w2c": a + 2}, b"8-byte aligned"),
                     ({"keys": a + 2}, b"4-byte aligned"), ({"counts": a + 1}, b"4-byte aligned")):
        assert call(**kw) == -1, kw
        assert text in L.dgs_last_error(), (kw, L.dgs_last_error())


def test_wrappers_refuse_the_cpu(tmp_path):
    import torch
    from deblurgs_amd import scene
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.resize_images(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.pil_to_torch(np.zeros((8, 8, 3), np.uint8), (4, 4), device="cpu")
    case = sc.bounds_cases()[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.depth_bounds(case.cams, case.points, device="cpu")
    _write_dataset(tmp_path)
    with pytest.raises(RuntimeError, match="needs a tensor on a HIP device"):
        scene.load_colmap_scene(str(tmp_path), device="cpu")


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", sc.RESIZE_CASES, ids=lambda c: c.name)
def test_restatement_equals_the_pillow_golden(case, golden):
    x = sc.resize_input(case)
    assert x.shape == (case.G, case.H, case.W, case.C)
    extreme = np.isin(x, (0, 255)).all(axis=(2, 3)).sum(axis=1)                  # rows drawn from {0, 255}
    assert (extreme >= case.H / 6).all() and (extreme <= case.H / 2 + 1).all(), extreme      # about a third, in whole bands
    clamps = [0, 0]
    got = sc.resize_restated(x, (case.w, case.h), clamps)
    want = golden["resize_" + case.name]
    assert got.shape == want.shape == (case.G, case.h, case.w, case.C)
    assert np.array_equal(got, want), int((got != want).sum())
    if sc.CLAMPS_FIRE[case.name]:
        assert clamps[0] > 0 and clamps[1] > 0, clamps                           # both clamps fire
    else:
        assert clamps == [0, 0]
    try:
        import PIL
        from PIL import Image
    except ImportError:
        return
    if PIL.__version__ == str(golden["pillow_version"]):
        for g in range(case.G):
            ref = np.asarray(Image.fromarray(x[g] if case.C == 3 else x[g, :, :, 0]).resize((case.w, case.h)))
            assert np.array_equal(ref.reshape(case.h, case.w, case.C), got[g])


# ------------------------------------------------------------------------------------------------- COLMAP readers
def _check_images(images, g, prefix):
    ids = list(images)
    assert ids == g[prefix + "img_ids"].tolist()                                 # and in the file's order
    assert np.array_equal(np.stack([images[i].qvec for i in ids]), g[prefix + "img_qvec"])
    assert np.array_equal(np.stack([images[i].tvec for i in ids]), g[prefix + "img_tvec"])
    assert [images[i].camera_id for i in ids] == g[prefix + "img_cam"].tolist()
    assert [images[i].name for i in ids] == g[prefix + "img_names"].tolist()
    assert [len(images[i].point3D_ids) for i in ids] == g[prefix + "img_npts"].tolist()
    assert np.array_equal(np.concatenate([images[i].xys.reshape(-1, 2) for i in ids]), g[prefix + "img_xys"])
    assert np.array_equal(np.concatenate([images[i].point3D_ids for i in ids]), g[prefix + "img_pids"])
    assert all(images[i].xys.shape == (len(images[i].point3D_ids), 2) for i in ids)


def _check_cameras(cameras, g, prefix):
    ids = list(cameras)
    assert ids == g[prefix + "cam_ids"].tolist()
    assert [cameras[i].model for i in ids] == g[prefix + "cam_models"].tolist()
    assert [[cameras[i].width, cameras[i].height] for i in ids] == g[prefix + "cam_sizes"].tolist()
    assert np.array_equal(np.concatenate([cameras[i].params for i in ids]), g[prefix + "cam_params"])


def _check_points(points, g, prefix):
    assert np.array_equal(points.xyz, g[prefix + "pts_xyz"]) and np.array_equal(points.rgb, g[prefix + "pts_rgb"])
    assert np.array_equal(points.error, g[prefix + "pts_err"]) and points.error.shape == (len(points.ids), 1)
    assert points.xyz.dtype == points.rgb.dtype == points.error.dtype == np.float64


def test_colmap_readers_equal_the_golden_parse(tmp_path, golden):
    from deblurgs_amd import colmap_io
    cameras, images, points = sc.reader_model()
    b, t, p = str(tmp_path / "bin"), str(tmp_path / "txt"), str(tmp_path / "pinhole")
    sc.write_model(b, cameras, images, points, binary=True)
    sc.write_model(t, cameras, images, points, binary=False)
    sc.write_model(p, [c for c in cameras if c[1] == "PINHOLE"], images, points, binary=False)
    _check_cameras(colmap_io.read_cameras_binary(os.path.join(b, "cameras.bin")), golden, "bin_")
    _check_images(colmap_io.read_images_binary(os.path.join(b, "images.bin")), golden, "bin_")
    _check_points(colmap_io.read_points3D_binary(os.path.join(b, "points3D.bin")), golden, "bin_")
    _check_cameras(colmap_io.read_cameras_text(os.path.join(t, "cameras.txt")), golden, "bin_")     # (the text round-trips)
    _check_cameras(colmap_io.read_cameras_text(os.path.join(p, "cameras.txt")), golden, "txt_")
    _check_images(colmap_io.read_images_text(os.path.join(t, "images.txt")), golden, "txt_")
    _check_points(colmap_io.read_points3D_text(os.path.join(t, "points3D.txt")), golden, "txt_")
    assert [int(i) for i in colmap_io.read_points3D_binary(os.path.join(b, "points3D.bin")).ids] == [q[0] for q in points]
    # the directory reader: .bin first, .txt where the binary file is missing or broken
    os.remove(os.path.join(b, "cameras.bin"))
    with open(os.path.join(b, "points3D.bin"), "wb") as f:
        f.write(b"\x05\0\0\0\0\0\0\0junk")
    with pytest.raises(FileNotFoundError, match="cameras"):
        colmap_io.read_model(b)
    for stem in ("cameras", "points3D"):
        os.replace(os.path.join(t, stem + ".txt"), os.path.join(b, stem + ".txt"))
    cams, imgs, pts = colmap_io.read_model(b)
    _check_cameras(cams, golden, "bin_")
    _check_images(imgs, golden, "bin_")
    _check_points(pts, golden, "txt_")
    rot = np.stack([colmap_io.qvec2rotmat(im[1]) for im in images])
    assert np.abs(rot - golden["qvec_rotmat"]).max() <= 4 * np.finfo(np.float64).eps
    assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14


def test_every_camera_model_has_its_parameter_count(tmp_path):
    from deblurgs_amd import colmap_io
    assert colmap_io.MODEL_IDS == sc.MODEL_IDS
    want = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "OPENCV_FISHEYE": 8,
            "FULL_OPENCV": 12, "FOV": 5, "SIMPLE_RADIAL_FISHEYE": 4, "RADIAL_FISHEYE": 5, "THIN_PRISM_FISHEYE": 12}
    assert colmap_io.MODEL_PARAMS == want
    cameras = [(i + 1, name, 10 + i, 20 + i, [float(i) + 0.25 * k for k in range(n)]) for i, (name, n) in enumerate(want.items())]
    for binary in (True, False):
        d = str(tmp_path / ("b" if binary else "t"))
        sc.write_model(d, cameras, [], [], binary=binary)
        got = (colmap_io.read_cameras_binary if binary else colmap_io.read_cameras_text)(
            os.path.join(d, "cameras.bin" if binary else "cameras.txt"))
        assert [(c.id, c.model, c.width, c.height, list(c.params)) for c in got.values()] == cameras


# ------------------------------------------------------------------------------------------------- host restatements
def test_training_resolution_equals_loadcam(golden):
    from deblurgs_amd import scene
    got = [scene.training_resolution(w, h, r) for w, h, r in sc.RESOLUTION_TABLE]
    assert np.array_equal(np.array(got, dtype=np.int64), golden["resolutions"])
    assert scene.training_resolution(101, 67, 2) == (50, 34)                 # round(): 50.5 -> 50, 33.5 -> 34
    assert scene.training_resolution(1234, 821, 800) == (800, int(821 / (1234 / 800)))      # int(): truncation
    assert scene.training_resolution(3840, 2160, -1) == (1600, 900) and scene.training_resolution(1600, 1066, -1) == (1600, 1066)
    assert scene.training_resolution(96, 64, 2, resolution_scale=2.0) == (24, 16)


def test_nerfpp_radius_equals_the_golden_exactly(golden):
    from deblurgs_amd import scene
    cams = sc.make_cameras(7, 90)
    pts32 = np.random.default_rng(91).normal(0.0, 2.0, (400, 3)).astype(np.float32)
    centers = golden["radius_centers"]
    assert centers.dtype == np.float32
    assert scene.nerfpp_radius(centers, pts32) == golden["radius_points"]
    assert scene.nerfpp_radius(centers) == golden["radius_cameras"]
    assert golden["radius_points"] != golden["radius_cameras"]
    mine = scene.camera_centers(cams)
    assert mine.dtype == np.float32 and np.abs(mine - centers).max() <= 1e-6
    true = np.stack([-c.R @ c.T for c in cams])
    assert np.abs(mine - true).max() <= 1e-6


def test_random_frustum_points_equal_the_golden_bit_for_bit(golden):
    from deblurgs_amd import scene
    cams = sc.make_cameras(7, 90)
    bds = np.stack([np.linspace(0.5, 1.5, 7), np.linspace(4.0, 9.0, 7)], axis=1)
    np.random.seed(3)
    got = scene.random_frustum_points(cams, near=1.2, far=6.0, num_pcd=900, bds=bds)
    assert got.dtype == np.float64 and got.shape == golden["random_pcd_bds"].shape == (900, 3)
    assert np.array_equal(got, golden["random_pcd_bds"])
    np.random.seed(3)
    assert np.array_equal(scene.random_frustum_points(cams[:3], near=2.0, far=8.0, num_pcd=300), golden["random_pcd_plain"])
    np.random.seed(4)
    assert not np.array_equal(scene.random_frustum_points(cams[:3], near=2.0, far=8.0, num_pcd=300), golden["random_pcd_plain"])
    with pytest.raises(ValueError, match="zero slice step"):
        scene.random_frustum_points(cams[:3], num_pcd=10 ** 7)


def test_bounds_cases_meet_their_preconditions_and_the_golden(golden):
    """The cases module asserts the margins and the 20 visible points; here the float64 restatement of the test is held
    against get_bds itself: the same points pass, so np.percentile of their depths is the golden."""
    for case in sc.bounds_cases():
        (z, _, _, _, _), _ = sc.bounds_quantities(case.cams, case.points)
        valid = sc.bounds_valid(case.cams, case.points)
        want = golden["bds_" + case.name]
        assert want.shape == (len(case.cams), 2) and want.dtype == np.float64
        for i in range(len(case.cams)):
            d = z[i][valid[i]]
            got = [np.percentile(d, 0.1), np.percentile(d, 99.9)]
            assert np.abs(np.array(got) - want[i]).max() <= 1e-12 * want[i, 1], (case.name, i)


# ------------------------------------------------------------------------------------------------- split, prune, loader
def _write_dataset(root, names=None, binary=True, n_points=300, camera_model="PINHOLE", hold=None):
    cameras, images, points = sc.scene_model(n_points=n_points, names=names, camera_model=camera_model)
    sc.write_model(os.path.join(str(root), "sparse", "0"), cameras, images, points, binary=binary)
    os.makedirs(os.path.join(str(root), "images"), exist_ok=True)
    if hold is not None:
        open(os.path.join(str(root), f"hold={hold}"), "w").close()
    return cameras, images, points


@pytest.mark.parametrize("binary", [True, False], ids=["bin", "txt"])
def test_cameras_split_and_hold_file(tmp_path, binary):
    from deblurgs_amd import colmap_io, scene
    names = ["007", "002", "010", "004"]
    _, images, _ = _write_dataset(tmp_path, names=names, binary=binary)
    cams = scene.read_cameras(str(tmp_path))
    assert [c.image_name for c in cams] == [im[4].split(".")[0] for im in images]           # the file's order
    by_name = {im[4].split(".")[0]: im for im in images}
    for c in cams:
        im = by_name[c.image_name]
        assert np.array_equal(c.R, colmap_io.qvec2rotmat(im[1]).T) and np.array_equal(c.T, np.array(im[2]))
        assert (c.width, c.height) == (96, 64)
        assert c.FovX == 2 * math.atan(96 / (2 * 95.0)) and c.FovY == 2 * math.atan(64 / (2 * 93.0))
        assert c.image_path == os.path.join(str(tmp_path), "images", c.image_name + ".png")
    train, test = scene.split_cameras(cams, str(tmp_path))
    assert [c.image_name for c in train] == sorted(names) and test == []
    train, test = scene.split_cameras(cams, str(tmp_path), eval=True, llffhold=2)
    assert [c.image_name for c in train] == ["007"] and [c.image_name for c in test] == ["002", "004", "010"]
    with pytest.raises(ValueError, match="the other is off"):
        scene.split_cameras(cams, str(tmp_path), eval=True)
    with pytest.raises(ValueError, match="the other is off"):
        scene.split_cameras(cams, str(tmp_path), llffhold=2)
    open(os.path.join(str(tmp_path), "hold=5"), "w").close()                                # the indicator file
    train, test = scene.split_cameras(cams, str(tmp_path), eval=True)
    assert [c.image_name for c in test] == ["010"] and len(train) == 3
    with pytest.raises(ValueError, match="the other is off"):
        scene.split_cameras(cams, str(tmp_path))                                            # the file alone, as in the reference
    train, test = scene.split_cameras(cams, str(tmp_path), eval=True, llffhold=7)           # an explicit value wins
    assert [c.image_name for c in test] == ["007"]
    open(os.path.join(str(tmp_path), "hold=3"), "w").close()
    with pytest.raises(ValueError, match="more than one llffhold"):
        scene.split_cameras(cams, str(tmp_path), eval=True)


def test_split_takes_int_of_the_image_name(tmp_path):
    from deblurgs_amd import scene
    _write_dataset(tmp_path, names=["a1", "a2", "a3", "a4"])
    cams = scene.read_cameras(str(tmp_path))
    with pytest.raises(ValueError, match=r"int\(image_name\)"):
        scene.split_cameras(cams, str(tmp_path), eval=True, llffhold=2)


def test_error_prune_and_text_fallback(tmp_path):
    from deblurgs_amd import scene
    _, _, points = _write_dataset(tmp_path, binary=False)
    xyz, rgb = scene.read_points(str(tmp_path))
    assert xyz.shape == rgb.shape == (300, 3) and np.array_equal(xyz, np.array([p[1] for p in points]))
    err = np.array([p[3] for p in points])
    xyz2, rgb2 = scene.read_points(str(tmp_path), num_initial_pcd=120)
    keep = err < np.percentile(err, 120 / 300 * 100)
    assert keep.sum() == 120 and np.array_equal(xyz2, xyz[keep]) and np.array_equal(rgb2, rgb[keep])
    xyz3, _ = scene.read_points(str(tmp_path), num_initial_pcd=1000)                        # the percentile caps at 100:
    assert len(xyz3) == 299                                                                 # `<` drops the largest error


def test_unsupported_camera_model_is_named(tmp_path):
    from deblurgs_amd import scene
    cameras, images, points = sc.scene_model()
    cameras = [(1, "OPENCV", 96, 64, [95.0, 93.0, 48.0, 32.0, 0.1, 0.0, 0.0, 0.0])]
    sc.write_model(os.path.join(str(tmp_path), "sparse", "0"), cameras, images, points)
    with pytest.raises(ValueError, match="OPENCV"):
        scene.read_cameras(str(tmp_path))


def test_simple_pinhole_uses_one_focal_length(tmp_path):
    from deblurgs_amd import scene
    _write_dataset(tmp_path, camera_model="SIMPLE_PINHOLE")
    c = scene.read_cameras(str(tmp_path))[0]
    assert c.FovX == 2 * math.atan(96 / (2 * 95.0)) and c.FovY == 2 * math.atan(64 / (2 * 95.0))

"""CPU tests of Blender scene loading (deblurgs_amd/scene.py, csrc/scene.hip): dgs_rgba_over_u8 and dgs_resize_rgba_u8 are
declared, exported, bound and refuse bad arguments before any HIP call; the golden composite tables against the float64
expression and its look-alikes; the numpy restatement of Pillow's RGBA resize against PIL's golden bytes; the transforms
reader, the split, the dispatch and the random initialisation against the golden."""
import json
import os
import re

import numpy as np
import pytest

import blender_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_rgba_over_u8", "dgs_resize_rgba_u8")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "blender_golden.npz"))


def test_new_symbols_are_declared_exported_and_bound():
    from deblurgs_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s) and (s + "(") in header, s
        assert getattr(L, s).argtypes == _lib.EXPORTS[s][1]
    assert L.dgs_abi_version() == 15 and _lib.ABI_VERSION == 15            # additions to ABI 15
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", header).group(1)) == 15


# ------------------------------------------------------------------------------------------------- argument errors
def test_rgba_over_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096          # non-null, aligned dummies: only the argument logic runs
    ok = dict(src=a + 1, G=2, H=37, W=53, white=1, u8=a + 3, f32=a, stride=3 * 37 * 53)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_rgba_over_u8(v["src"], v["G"], v["H"], v["W"], v["white"], v["u8"], v["f32"], v["stride"], None)

    for kw, text in (({"src": None}, b"null input"), ({"u8": None, "f32": None}, b"both outputs"),
                     ({"G": 0}, b"G must be"), ({"G": -1}, b"G must be"),
                     ({"H": 0}, b"1..65536"), ({"W": 0}, b"1..65536"), ({"W": 70000}, b"1..65536"), ({"H": -2}, b"1..65536"),
                     ({"f32": a + 2}, b"4-byte aligned"), ({"stride": 3 * 37 * 53 - 1}, b"stride")):
        assert call(**kw) == -1, kw
        assert b"rgba_over_u8" in L.dgs_last_error() and text in L.dgs_last_error(), (kw, L.dgs_last_error())
    with pytest.raises(RuntimeError, match="dgs_rgba_over_u8 failed"):
        _lib.check(call(G=0), "dgs_rgba_over_u8")


def test_resize_rgba_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096
    ok = dict(src=a + 1, G=2, H=37, W=53, h=18, w=26, kh=a, bh=a, kv=a, bv=a, u8=a + 3, f32=a, stride=4 * 18 * 26)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_resize_rgba_u8(v["src"], v["G"], v["H"], v["W"], v["h"], v["w"], v["kh"], v["bh"], v["kv"], v["bv"],
                                    v["u8"], v["f32"], v["stride"], None)

    seen = set()
    for kw, text in (({"src": None}, b"null input"), ({"u8": None, "f32": None}, b"both outputs"),
                     ({"G": 0}, b"G must be"), ({"G": -1}, b"G must be"),
                     ({"H": 0}, b"1..65536"), ({"w": 0}, b"1..65536"), ({"W": 70000}, b"1..65536"), ({"h": -2}, b"1..65536"),
                     ({"H": 1300, "h": 20}, b"[1/64, 64]"), ({"W": 10, "w": 700}, b"[1/64, 64]"),
                     ({"kh": None}, b"null horizontal"), ({"bh": None}, b"null horizontal"),
                     ({"kv": None}, b"null vertical"), ({"bv": None}, b"null vertical"),
                     ({"kh": a + 2}, b"4-byte aligned"), ({"bv": a + 1}, b"4-byte aligned"), ({"f32": a + 2}, b"4-byte aligned"),
                     ({"stride": 4 * 18 * 26 - 1}, b"stride is below 4 * h * w")):
        assert call(**kw) == -1, kw
        assert b"resize_rgba_u8: " in L.dgs_last_error() and text in L.dgs_last_error(), (kw, L.dgs_last_error())
        seen.add(text)
    assert len(seen) == 9                                                   # each failure has its own message
    # the three-channel entry point still refuses four channels, with the message it has always had
    assert L.dgs_resize_u8(a + 1, 2, 37, 53, 4, 18, 26, a, a, a, a, a + 3, a, 4 * 18 * 26, None) == -1
    assert b"resize_u8: C must be 1 or 3" in L.dgs_last_error()


def test_wrappers_refuse_the_cpu(tmp_path):
    import torch
    from deblurgs_amd import scene
    x = torch.zeros(1, 8, 8, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.rgba_over(x, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.rgba_over(x.numpy(), False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.resize_rgba_images(x, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.pil_to_torch(np.zeros((8, 8, 4), np.uint8), (4, 4), device="cpu")
    bc.write_blender_dir(tmp_path)
    with pytest.raises(RuntimeError, match="needs a tensor on a HIP device"):
        scene.load_blender_scene(str(tmp_path), device="cpu")
    with pytest.raises(RuntimeError, match="needs a tensor on a HIP device"):
        scene.load_scene(str(tmp_path), device="cpu")                       # (dispatched to the Blender loader)


# ------------------------------------------------------------------------------------------------- the composite tables
@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
def test_golden_composite_tables(golden, white):
    """The counts are preconditions of the GPU test: a kernel that takes the integer floor, or evaluates in float32, gives
    other bytes than the golden in that many of the 65 536 pairs."""
    table = golden["over_white" if white else "over_black"]
    assert table.shape == (256, 256) and table.dtype == np.uint8
    a, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    value = ((c / 255.0) * (a / 255.0) + (1.0 if white else 0.0) * (1.0 - a / 255.0)) * 255.0      # float64, here
    assert value.dtype == np.float64 and value.min() >= 0.0 and value.max() < 256.0
    assert np.array_equal(table, np.trunc(value).astype(np.int64).astype(np.uint8))
    assert np.array_equal(table, bc.over_table(white))
    assert np.array_equal(table[255], np.arange(256)) and (table[0] == (255 if white else 0)).all()
    floor_differs = int((table != bc.over_floor_table(white)).sum())
    float32_differs = int((table != bc.over_table(white, np.float32)).sum())
    print("differs from the integer floor:", floor_differs, " from float32:", float32_differs)
    assert floor_differs == bc.FLOOR_DIFFERS[int(white)]
    assert float32_differs == bc.FLOAT32_DIFFERS[int(white)]
    pairs = bc.over_pairs()                                                 # the GPU test's image, from the table
    assert np.array_equal(bc.over_from_table(table, pairs), bc.over_restated(pairs, white))


# ------------------------------------------------------------------------------------------------- the RGBA restatement
@pytest.mark.parametrize("case", bc.RGBA_CASES, ids=lambda c: c.name)
def test_rgba_restatement_equals_the_pillow_golden(case, golden):
    x = bc.rgba_input(case)
    assert x.shape == (case.G, case.H, case.W, 4) and x.dtype == np.uint8
    clipped = [0]
    got = bc.resize_rgba_restated(x, (case.w, case.h), clipped)
    want = golden["rgba_" + case.name]
    assert got.shape == want.shape == (case.G, case.h, case.w, 4)
    assert np.array_equal(got, want), int((got != want).sum())
    zero, full, between = bc.rgba_counts(want)
    print(case.name, "alpha 0:", zero, " alpha 255:", full, " between:", between, " clipped colour bytes:", clipped[0])
    assert zero > 0 and full > 0 and between > 0
    if case.name == "same":                                                 # a copy: nothing is divided, nothing clipped
        assert clipped[0] == 0 and np.array_equal(want, x)
        assert tuple(want[0, 0, 0]) == (9, 8, 7, 0)                         # the colour under alpha 0 survives
    else:
        assert clipped[0] > 0                                               # 255 c // a exceeds 255 somewhere
        # resampling four independent channels is another picture
        import scene_cases as sc
        assert not np.array_equal(sc.resize_restated(x, (case.w, case.h)), want)
    try:
        import PIL
        from PIL import Image
    except ImportError:
        return
    if PIL.__version__ == str(golden["pillow_version"]):
        for g in range(case.G):
            assert np.array_equal(np.asarray(Image.fromarray(x[g], "RGBA").resize((case.w, case.h))), got[g])


# ------------------------------------------------------------------------------------------------- the readers
def test_read_blender_cameras_equal_the_golden(tmp_path, golden):
    from deblurgs_amd import scene
    sources = bc.write_blender_dir(tmp_path)                                # 40 x 32 pictures: FovY differs from FovX
    cams = scene.read_blender_cameras(str(tmp_path), "transforms_train.json")
    assert [c.image_name for c in cams] == list(sources["train"]) == ["r_0", "r_1", "r_2", "r_3"]
    assert [c.uid for c in cams] == [0, 1, 2, 3]
    assert np.array_equal(np.stack([c.R for c in cams]), golden["cam_R"])
    assert np.array_equal(np.stack([c.T for c in cams]), golden["cam_T"])
    fov_x, fov_y = golden["cam_fov"]
    assert all(c.FovX == fov_x == bc.CAMERA_ANGLE_X and c.FovY == fov_y for c in cams) and fov_x != fov_y
    assert all((c.width, c.height) == (40, 32) for c in cams)
    assert cams[1].image_path == os.path.join(str(tmp_path), "./train/r_1.png")
    # R is a camera-to-world rotation in COLMAP's axes: the camera looks down +z at the origin from 4 units away
    for c in cams:
        assert np.abs(c.R @ c.R.T - np.eye(3)).max() <= 1e-12
        centre = -c.R @ c.T
        assert abs(np.linalg.norm(centre) - 4.0) <= 1e-12 and np.abs(centre + 4.0 * c.R[:, 2]).max() <= 1e-12
    # an explicit reader and another extension
    seen = []

    def reader(path):
        seen.append(path)
        return np.load(path)
    cams = scene.read_blender_cameras(str(tmp_path), "transforms_test.json", extension=".npy", image_reader=reader)
    assert len(cams) == 2 and seen == [os.path.join(str(tmp_path), f"./test/r_{i}.npy") for i in range(2)]
    with pytest.raises(FileNotFoundError):
        scene.read_blender_cameras(str(tmp_path), "transforms_val.json")


def test_blender_split_follows_eval(tmp_path):
    from deblurgs_amd import scene
    bc.write_blender_dir(tmp_path)
    train = scene.read_blender_cameras(str(tmp_path), "transforms_train.json")
    test = scene.read_blender_cameras(str(tmp_path), "transforms_test.json")
    a, b = scene.split_blender(train, test, eval=True)
    assert a == train and b == test
    a, b = scene.split_blender(train, test, eval=False)
    assert a == train + test and b == [] and len(a) == 6                    # the test views are appended, not sorted in
    assert len(train) == 4                                                  # (the arguments are not extended in place)


def test_load_scene_raises_on_an_unrecognised_directory(tmp_path):
    from deblurgs_amd import scene
    os.makedirs(str(tmp_path / "images"))
    with open(str(tmp_path / "transforms.json"), "w") as f:
        json.dump({}, f)
    with pytest.raises(ValueError, match=re.escape(str(tmp_path))):
        scene.load_scene(str(tmp_path))
    fields = scene.SceneData.__dataclass_fields__
    assert list(fields)[-1] == "white_background" and fields["white_background"].default is False


def test_blender_random_cloud_equals_the_golden_bit_for_bit(tmp_path, golden):
    from deblurgs_amd import scene
    bc.write_blender_dir(tmp_path)
    cams = scene.read_blender_cameras(str(tmp_path), "transforms_train.json")
    np.random.seed(7)
    xyz, rgb = scene.blender_random_cloud(cams, 3000)
    assert xyz.dtype == rgb.dtype == np.float64 and xyz.shape == rgb.shape == (3000, 3)
    assert np.array_equal(xyz, golden["cloud_xyz"]) and np.array_equal(rgb, golden["cloud_rgb"])
    assert rgb.min() >= 127.5 and rgb.max() < 127.5 + 0.2822                # SH2RGB of a draw below 1 / 255: grey 127
    points, colors = scene._ply_round_trip(xyz, rgb)
    assert points.dtype == np.float32 and np.array_equal(colors, np.full((3000, 3), 127 / 255.0))
    np.random.seed(8)
    assert not np.array_equal(scene.blender_random_cloud(cams, 3000)[0], golden["cloud_xyz"])


def test_read_ply_points_reads_the_storeply_layout(tmp_path):
    from deblurgs_amd import scene
    rng = np.random.default_rng(5)
    dtype = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
             ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.zeros(17, dtype=dtype)
    for k in ("x", "y", "z"):
        v[k] = rng.normal(0, 2, 17).astype(np.float32)
    for k in ("red", "green", "blue"):
        v[k] = rng.integers(0, 256, 17)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 17\n" + \
        "".join(f"property {'float' if t == '<f4' else 'uchar'} {n}\n" for n, t in dtype) + "end_header\n"
    path = str(tmp_path / "points3d.ply")
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + v.tobytes())
    xyz, rgb = scene.read_ply_points(path)
    assert xyz.dtype == np.float32 and np.array_equal(xyz, np.stack([v["x"], v["y"], v["z"]], axis=1))
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, np.stack([v["red"], v["green"], v["blue"]], axis=1))
    with open(path, "w") as f:
        f.write(header.replace("binary_little_endian", "ascii"))
        for row in v:
            f.write(" ".join(repr(float(row[k])) if t == "<f4" else str(int(row[k])) for k, t in dtype) + "\n")
    xyz2, rgb2 = scene.read_ply_points(path)
    assert np.array_equal(xyz2, xyz) and np.array_equal(rgb2, rgb)
    with open(path, "w") as f:
        f.write("plx\n")
    with pytest.raises(ValueError, match="not a PLY file"):
        scene.read_ply_points(path)

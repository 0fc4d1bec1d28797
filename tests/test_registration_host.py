"""CPU tests of the test-pose seeding (deblurgs_amd/registration.py, csrc/register.hip): the new entry points are declared,
exported, bound and refuse bad arguments before any HIP call; the size query; the candidate poses and the pattern-search
lattice, which are host code."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_box_reduce_u8", "dgs_sad_matrix_tmp_bytes", "dgs_sad_matrix")


def test_new_symbols_are_declared_exported_and_bound():
    from deblurgs_amd import _lib, build, registration as reg
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s) and (s + "(") in header, s
        assert getattr(L, s).argtypes == _lib.EXPORTS[s][1]
    assert L.dgs_abi_version() == 15            # additions to ABI 15
    assert "register.hip" in build.SOURCES
    assert int(re.search(r"#define DGS_SAD_CHUNK_DWORDS (\d+)", header).group(1)) == reg.SAD_CHUNK
    assert int(re.search(r"#define DGS_SAD_TILE_A (\d+)", header).group(1)) == reg.SAD_TILE_A
    assert reg.SAD_CHUNK % 4 == 0 and reg.SAD_CHUNK <= 2 ** 20         # 4 * 255 * chunk < 2^32: uint32 partials


def test_box_reduce_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096          # non-null, 16-byte aligned dummies: only the argument logic runs
    ok = dict(src=a + 1, G=2, H=17, W=23, s=3, out=a)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_box_reduce_u8(v["src"], v["G"], v["H"], v["W"], v["s"], v["out"], None)

    for kw, text in (({"G": 0}, b"G must be"), ({"G": -1}, b"G must be"),
                     ({"H": 2}, b"empty output"), ({"W": 2}, b"empty output"), ({"H": 0}, b"empty output"),
                     ({"W": -5}, b"empty output"), ({"s": 0}, b"s must be"), ({"s": -1}, b"s must be"),
                     ({"s": 65, "H": 100, "W": 100}, b"s must be"),
                     ({"src": None}, b"null"), ({"out": None}, b"null"),
                     ({"out": a + 4}, b"16-byte aligned"), ({"out": a + 8}, b"16-byte aligned")):
        assert call(**kw) == -1, kw
        assert text in L.dgs_last_error(), (kw, L.dgs_last_error())
    with pytest.raises(RuntimeError, match="dgs_box_reduce_u8 failed"):
        _lib.check(call(G=0), "dgs_box_reduce_u8")


def test_sad_matrix_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096
    ok = dict(a=a, na=3, b=a, nb=36, group=12, L=1028, out=a, tmp=a)

    def call(**kw):
        v = dict(ok, **kw)
        return L.dgs_sad_matrix(v["a"], v["na"], v["b"], v["nb"], v["group"], v["L"], v["out"], v["tmp"], None)

    for kw, text in (({"a": None}, b"null"), ({"b": None}, b"null"), ({"out": None}, b"null"), ({"tmp": None}, b"null"),
                     ({"na": 0}, b"at least 1"), ({"nb": 0, "group": 0}, b"at least 1"), ({"na": -2}, b"at least 1"),
                     ({"L": 0}, b"multiple of 4"), ({"L": 1026}, b"multiple of 4"), ({"L": 3}, b"multiple of 4"),
                     ({"group": -1}, b"group"), ({"group": 11}, b"na * m"), ({"nb": 35}, b"na * m"),
                     ({"a": a + 4}, b"16-byte aligned"), ({"b": a + 8}, b"16-byte aligned"),
                     ({"out": a + 4}, b"aligned"), ({"tmp": a + 2}, b"aligned")):
        assert call(**kw) == -1, kw
        assert text in L.dgs_last_error(), (kw, L.dgs_last_error())


def test_sad_matrix_tmp_bytes_is_monotone_and_a_function_of_its_arguments():
    from deblurgs_amd import _lib, registration as reg
    L = _lib.lib()
    c = reg.SAD_CHUNK
    sizes = [L.dgs_sad_matrix_tmp_bytes(5, 7, n) for n in (4, 8, c - 4, c, c + 4, 3 * c + 4, 100 * c)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert sizes[3] == sizes[0] == 5 * 7 * 4 and sizes[4] == 2 * sizes[3] and sizes[5] == 4 * sizes[3]
    for args in ((1, 1, 4), (17, 1, 1024), (3, 36, 4_300_000)):
        assert L.dgs_sad_matrix_tmp_bytes(*args) == L.dgs_sad_matrix_tmp_bytes(*args) > 0
        L.dgs_sad_matrix(None, 1, None, 1, 0, 4, None, None, None)           # a refused call in between changes nothing
        assert L.dgs_sad_matrix_tmp_bytes(*args) == -(-args[2] // c) * args[0] * args[1] * 4
    assert L.dgs_sad_matrix_tmp_bytes(0, 1, 4) == L.dgs_sad_matrix_tmp_bytes(1, 1, 6) == L.dgs_sad_matrix_tmp_bytes(1, 1, 0) == 0


def test_wrappers_refuse_cpu_tensors():
    import torch
    from deblurgs_amd import registration as reg
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.box_reduce_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.sad_matrix(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------- candidate poses
def _motion(n=3, seed=0):
    """Three views on the CPU (fused=False paths), their trajectories well apart: rotations of ~0.3 rad between views."""
    import torch
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    torch.manual_seed(seed)
    ref = RefCamera(64, 48, 1.0, 0.8, device="cpu")
    init = torch.randn(n, 6) * 0.05 + torch.arange(n)[:, None] * torch.tensor([0.2, -0.1, 0.05, 0.25, -0.15, 0.1])
    return CameraMotionModule(ref, torch.rand(n, 3, 48, 64), curve_order=3, num_subframes=7, device="cpu", init_se3=init)


@pytest.mark.parametrize("subframes,between", [(3, 1), (2, 2), (4, 0)])
def test_candidate_cameras_count_and_table(subframes, between):
    import torch
    from deblurgs_amd import registration as reg
    m = _motion()
    cams, table = reg.candidate_cameras(m, subframes=subframes, between=between)
    assert len(cams) == len(table) == 3 * subframes + 2 * between
    want = [("trajectory", i, k) for i in range(3) for k in range(subframes)] + \
           [("between", i, j) for i in range(2) for j in range(1, between + 1)]
    assert [tuple(r) for r in table] == want
    nu = torch.linspace(0.0, 1.0, subframes)
    for i in range(3):
        for k, cam in enumerate(m.get_trajectory(i, nu)):
            got = cams[i * subframes + k]
            assert torch.equal(got.world_view_transform, cam.world_view_transform.detach())
            assert torch.equal(got.full_proj_transform, cam.full_proj_transform.detach())
            assert not got.world_view_transform.requires_grad
    for cam in cams:
        assert (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy) == (64, 48, 1.0, 0.8)
        assert cam.world_view_transform.dtype == torch.float32


def test_candidate_cameras_honours_exclude():
    from deblurgs_amd import registration as reg
    m = _motion()
    cams, table = reg.candidate_cameras(m, subframes=3, between=1, exclude=(1,))
    assert [tuple(r) for r in table] == [("trajectory", 0, 0), ("trajectory", 0, 1), ("trajectory", 0, 2), ("trajectory", 2, 0),
                                         ("trajectory", 2, 1), ("trajectory", 2, 2), ("between", 0, 1)]
    assert len(cams) == 7
    one, t1 = reg.candidate_cameras(m, subframes=3, between=1, exclude=(0, 2))
    assert len(one) == 3 and all(r[0] == "trajectory" and r[1] == 1 for r in t1)
    with pytest.raises(ValueError):
        reg.candidate_cameras(m, exclude=(0, 1, 2))


def test_between_pose_is_the_se3_midpoint():
    from deblurgs_amd import registration as reg, render_path as rp
    m = _motion()
    cams, table = reg.candidate_cameras(m, subframes=3, between=1)
    middle = [rp.cam_to_c2w(c) for c in m.get_middle_cams()]
    for v in range(2):
        mid = rp.cam_to_c2w(cams[table.index(("between", v, 1))])
        first = np.linalg.inv(middle[v]) @ mid                # a -> midpoint
        second = np.linalg.inv(mid) @ middle[v + 1]           # midpoint -> b
        assert np.abs(first - second).max() <= 1e-6, np.abs(first - second).max()
        assert np.abs(first - np.eye(4)).max() > 1e-2         # (the two views are apart: the midpoint is not an end)
    # the interpolation itself, in float64 on exactly rigid poses (the cameras' matrices above are rounded to fp32)
    from scipy.spatial.transform import Rotation
    a, rel = _pose(3), np.eye(4)
    rel[:3, :3] = Rotation.from_rotvec([0.3, -0.2, 0.4]).as_matrix()
    rel[:3, 3] = [0.5, -1.0, 2.0]
    b = a @ rel
    third = reg._se3_between(a, b, 1.0 / 3.0)
    step = np.linalg.inv(a) @ third
    assert np.abs(a @ step @ step @ step - b).max() <= 1e-9


def test_candidate_cameras_are_deterministic_under_curve_random_sample():
    import torch
    from deblurgs_amd import registration as reg
    m = _motion()
    m.curve_random_sample = True
    first, _ = reg.candidate_cameras(m, subframes=3, between=2)
    second, _ = reg.candidate_cameras(m, subframes=3, between=2)
    assert m.curve_random_sample is True
    for a, b in zip(first, second):
        assert torch.equal(a.world_view_transform, b.world_view_transform)
        assert torch.equal(a.full_proj_transform, b.full_proj_transform)
        assert torch.equal(a.camera_center, b.camera_center)


# ------------------------------------------------------------------------------------------------- the lattice
def _pose(seed=1):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    c2w = np.eye(4)
    c2w[:3, :3] = Rotation.from_rotvec(rng.normal(size=3)).as_matrix()
    c2w[:3, 3] = rng.normal(size=3) * 3.0
    return c2w


def test_seed_lattice_order_and_geometry():
    from deblurgs_amd import registration as reg
    c2w = _pose()
    ts, rs = 0.37, 0.021
    lat = reg.seed_lattice(c2w, ts, rs)
    assert lat.shape == (12, 4, 4) and lat.dtype == np.float64
    assert reg.LATTICE == ("+tx", "-tx", "+ty", "-ty", "+tz", "-tz", "+rx", "-rx", "+ry", "-ry", "+rz", "-rz")
    inv = np.linalg.inv(c2w)
    for k, name in enumerate(reg.LATTICE):
        sign, kind, axis = (1.0 if name[0] == "+" else -1.0), name[1], "xyz".index(name[2])
        rel = inv @ lat[k]                                     # the step in the camera's own frame
        e = np.zeros(3)
        e[axis] = 1.0
        if kind == "t":
            assert np.abs(rel[:3, :3] - np.eye(3)).max() <= 1e-12
            assert np.abs(rel[:3, 3] - sign * ts * e).max() <= 1e-12
            assert abs(np.linalg.norm(lat[k][:3, 3] - c2w[:3, 3]) - ts) <= 1e-12       # the centre moves by exactly ts
            assert np.abs(lat[k][:3, 3] - (c2w[:3, 3] + sign * ts * c2w[:3, axis])).max() <= 1e-12
        else:
            assert np.abs(lat[k][:3, 3] - c2w[:3, 3]).max() == 0.0                      # the centre stays
            R = rel[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
            assert np.abs(R @ e - e).max() <= 1e-12                                     # about the camera's own axis
            angle = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
            assert abs(angle - rs) <= 1e-9
            vee = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
            assert np.sign(vee[axis]) == sign
        assert np.array_equal(lat[k][3], [0.0, 0.0, 0.0, 1.0])


def test_seed_lattice_plus_and_minus_compose_to_the_identity():
    from deblurgs_amd import registration as reg
    c2w = _pose(2)
    for ts, rs in ((0.37, 0.021), (1e-9, 1e-9), (5.0, 1.2)):
        lat = reg.seed_lattice(c2w, ts, rs)
        inv = np.linalg.inv(c2w)
        for k in range(0, 12, 2):
            both = (inv @ lat[k]) @ (inv @ lat[k + 1])
            assert np.abs(both - np.eye(4)).max() <= 1e-12, (k, ts, rs)


def test_default_steps_and_the_single_view_rule():
    from deblurgs_amd import registration as reg
    from scipy.spatial.transform import Rotation
    poses = np.tile(np.eye(4), (4, 1, 1))
    for i, (d, ang) in enumerate(((0.0, 0.0), (1.0, 0.1), (3.0, 0.3), (7.0, 0.7))):
        poses[i, :3, 3] = [d, 0.0, 0.0]
        poses[i, :3, :3] = Rotation.from_rotvec([0.0, ang, 0.0]).as_matrix()
    ts, rs = reg.default_steps(poses)
    assert abs(ts - 0.25 * 2.0) <= 1e-12 and abs(rs - 0.25 * 0.2) <= 1e-9       # medians of (1, 2, 4) and (0.1, 0.2, 0.4)
    with pytest.raises(ValueError, match="single training view"):
        reg.default_steps(poses[:1])


def test_seed_test_poses_checks_the_image_size_before_anything_else():
    import torch
    from deblurgs_amd import registration as reg
    m = _motion()
    with pytest.raises(ValueError, match="ref_cam"):
        reg.seed_test_poses(m, None, torch.zeros(2, 3, 48, 60), torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.seed_test_poses(m, None, torch.zeros(2, 3, 48, 64), torch.zeros(3))


def test_initialize_test_pose_is_part_of_the_evaluation_module():
    import inspect
    from deblurgs_amd import evaluation as ev
    lines = [ln for ln in ev.__doc__.splitlines() if "initialize_test_pose" in ln]
    assert lines and not any("out of scope" in ln for ln in lines)
    doc = ev.initialize_test_pose.__doc__
    assert "COLMAP" in doc and "photometric" in doc
    assert list(inspect.signature(ev.initialize_test_pose).parameters)[:5] == ["motion", "cloud", "test_images", "bg",
                                                                               "tone_mapping"]

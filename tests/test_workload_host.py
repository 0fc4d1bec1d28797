"""CPU tests of the scene-shaped workload: the `surfaces` layout of synthetic.make_scene (deterministic, well-formed, and
shaped like a trained scene where the uniform layout gives every tile the same list) and the declaration of the device
tile-list profile (dgs_list_profile) in the header and the ctypes table.  The shape is measured with the OpenMP oracle's
list building alone (no rendering)."""
import os
import re

import numpy as np
import pytest

import helpers
from helpers import synthetic
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("means3D", "scales", "rotations", "opacities", "sh", "bg", "viewmatrix", "projmatrix", "campos", "se3", "nu",
          "ctrl_trans", "ctrl_rot", "projection_matrix")


def _same(a, b):
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
            assert a[key].tobytes() == b[key].tobytes(), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("seed", [0, 1])
def test_uniform_layout_is_unchanged(seed):
    a = synthetic.make_scene(3000, 176, 112, K=3, seed=seed)
    b = synthetic.make_scene(3000, 176, 112, K=3, seed=seed, layout="uniform")
    _same(a, b)
    # the draws of the default path, restated: the order of the rng calls is part of the contract
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, 10.0, 3000)
    u = rng.uniform(-1.15, 1.15, 3000)
    assert np.array_equal(a["means3D"][:, 2], z.astype(np.float32))
    assert np.array_equal(a["means3D"][:, 0], (u * a["tanfovx"] * z).astype(np.float32))


def test_make_config_passes_the_layout_through():
    a = synthetic.make_config("cfg1", layout="surfaces", layout_args=dict(n_surfaces=3))
    b = synthetic.make_scene(1000, 256, 256, K=1, curve_order=3, layout="surfaces", layout_args=dict(n_surfaces=3))
    _same(a, b)
    _same(synthetic.make_config("cfg1"), synthetic.make_scene(1000, 256, 256, K=1, curve_order=3))


def test_surfaces_layout_is_well_formed():
    P = 5000
    uni = synthetic.make_scene(P, 176, 112, K=2, seed=0)
    a = synthetic.make_scene(P, 176, 112, K=2, seed=0, layout="surfaces")
    _same(a, synthetic.make_scene(P, 176, 112, K=2, seed=0, layout="surfaces"))
    other = synthetic.make_scene(P, 176, 112, K=2, seed=1, layout="surfaces")
    assert a["means3D"].tobytes() != other["means3D"].tobytes() and a["scales"].tobytes() != other["scales"].tobytes()
    assert set(a) == set(uni)
    for key in uni:
        if isinstance(uni[key], np.ndarray):
            assert a[key].dtype == uni[key].dtype and a[key].shape == uni[key].shape, key
            assert np.isfinite(a[key]).all(), key
        else:
            assert type(a[key]) is type(uni[key]) and (key in ("P", "W", "H", "K", "M", "sh_degree") or a[key] == uni[key]), key
    for key in ARRAYS:
        assert key in a
    assert np.abs(np.linalg.norm(a["rotations"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert (a["scales"] > 0).all()
    assert (a["opacities"] > 0).all() and (a["opacities"] <= 1).all()
    assert (a["means3D"][:, 2] >= 1.0).all()        # (the camera sits within a few cm of the identity pose)
    # camera, trajectory, SH-independent parts are made as for the uniform layout
    for key in ("viewmatrix", "projmatrix", "campos", "se3", "nu", "projection_matrix"):
        assert a[key].tobytes() == uni[key].tobytes(), key
    with pytest.raises(ValueError):
        synthetic.make_scene(100, 64, 64, layout="spiral")
    with pytest.raises(ValueError):
        synthetic.make_scene(100, 64, 64, layout="surfaces", layout_args=dict(n_patches=3))
    with pytest.raises(ValueError):
        synthetic.make_scene(100, 64, 64, layout_args=dict(n_surfaces=3))


def _list_shape(scene):
    st = helpers.oracle_forward(scene, 0, render=False)
    length = (st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0].astype(np.int64))
    R = int(length.sum())
    assert R == st["num_rendered"]
    mean = R / length.size
    nonempty = length[length > 0]
    return dict(R=R, max=int(length.max()), share_long=float(length[length > 4 * mean].sum() / R),
                share_short=float((nonempty <= 64).sum() / nonempty.size), big=int((st["radii"] > 100).sum()),
                nonempty=float(nonempty.size / length.size),
                pct=[int(v) for v in np.percentile(nonempty, (50, 90, 99))])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_surfaces_scene_shape_at_the_metric_size(seed):
    """P = 1 M, 1920 x 1080, subframe 0, the reference's rectangle lists: the surfaces scene carries about the uniform
    scene's R in lists that are nothing like the uniform scene's."""
    oracle.use_openmp(True)
    try:
        uni = _list_shape(synthetic.make_scene(1_000_000, 1920, 1080, K=1, seed=seed))
        sur = _list_shape(synthetic.make_scene(1_000_000, 1920, 1080, K=1, seed=seed, layout="surfaces"))
    finally:
        oracle.use_openmp(False)
    print(f"\nseed {seed}: uniform {uni}\n         surfaces {sur}")
    assert abs(sur["R"] - uni["R"]) <= 0.15 * uni["R"]
    assert sur["max"] >= 8 * uni["max"]
    assert sur["share_long"] >= 0.3
    assert sur["share_short"] >= 0.3
    assert sur["big"] >= 500


def test_list_profile_entry_point_is_declared():
    from deblurgs_amd import _lib
    assert _lib.ABI_VERSION == 15
    for name in ("dgs_list_profile", "dgs_list_profile_tmp_bytes"):
        assert name in _lib.EXPORTS
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+dgs_list_profile\s*\(", code) and re.search(r"\bsize_t\s+dgs_list_profile_tmp_bytes\s*\(", code)
    assert re.search(r"#define DGS_ABI_VERSION 15\b", text)
    words = int(re.search(r"#define DGS_LIST_PROFILE_WORDS (\d+)", text).group(1))
    assert words == 8 + 2 * 33
    from deblurgs_amd import workload
    assert workload.WORDS == words and len(workload.SCALARS) == 8

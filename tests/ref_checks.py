"""The stage checkers of the parity tests in a layout-neutral form: both sides are lists of per-subframe dicts with the
oracle's plain keys (radii, tiles_touched, means2D, depths, conic_opacity, rgb, pre_sigmoid, cov3D, num_rendered, keys,
point_list, ranges, color, depth, n_contrib, final_T).  tests/test_gpu_parity.py adapts the product's packed layout to
it; tests/test_gpu_reference_kernels.py feeds it the reference's own kernels.  `got` is the side under test, `ref` the
side it is held to."""
import numpy as np

IMG_TOL = 1e-4      # abs, colour (values O(1))
DEPTH_TOL = 1e-4    # relative to z_far-scale depths
ANYWHERE_TOL = 2e-2  # a flipped threshold moves one pair's weight only
FINAL_T_TOL = 1e-5
RGB_TOL = 1e-6
PRE_SIGMOID_TOL = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_preprocess(got, ref, min_visible=100, relu=True):
    """Geometry state: radii and tiles_touched exactly equal; means2D, depths, conic_opacity, cov3D bitwise equal (same IEEE
    operations in the same order, no FMA contraction); rgb within 1e-6; the relu clamp mask equal (or, with the sigmoid
    activation, the pre-activation colours within 1e-5)."""
    for k, (g, o) in enumerate(zip(got, ref)):
        vis = o["radii"] > 0
        assert vis.sum() > min_visible
        assert np.array_equal(g["radii"], o["radii"]), "radii"
        assert np.array_equal(g["tiles_touched"], o["tiles_touched"]), "tiles_touched"
        assert np.array_equal(_bits(g["means2D"][vis]), _bits(o["means2D"][vis])), "means2D bits"
        assert np.array_equal(_bits(g["depths"][vis]), _bits(o["depths"][vis])), "depth bits"
        assert np.array_equal(_bits(g["conic_opacity"][vis]), _bits(o["conic_opacity"][vis])), "conic bits"
        assert np.abs(g["rgb"][vis] - o["rgb"][vis]).max() <= RGB_TOL, "rgb"
        if relu:
            assert np.array_equal(g["pre_sigmoid"][vis], o["pre_sigmoid"][vis]), "relu mask"
        else:   # sigmoid activation: the pre-activation colours, an SH sum like rgb
            assert np.abs(g["pre_sigmoid"][vis] - o["pre_sigmoid"][vis]).max() <= PRE_SIGMOID_TOL, "pre-sigmoid colours"
    wrote = np.any(ref[0]["cov3D"] != 0, axis=1)     # the oracle fills cov3D only past the near-plane cull
    assert np.array_equal(_bits(got[0]["cov3D"][wrote]), _bits(ref[0]["cov3D"][wrote])), "cov3D bits"


def check_binning(got, ref):
    """Per subframe: num_rendered, the sorted 64-bit keys (tile << 32 | depth bits), point_list, and the ranges of the
    non-empty tiles exactly equal; an empty tile has a range of length zero."""
    for k, (g, o) in enumerate(zip(got, ref)):
        assert int(g["num_rendered"]) == int(o["num_rendered"]), "num_rendered"
        assert np.array_equal(g["keys"], o["keys"]), "sort keys"
        assert np.array_equal(g["point_list"], o["point_list"]), "point_list"
        rng, want = np.asarray(g["ranges"]).astype(np.int64), np.asarray(o["ranges"]).astype(np.int64)
        nonempty = want[:, 1] > want[:, 0]
        assert np.array_equal(rng[nonempty], want[nonempty]), "tile ranges"
        assert np.all(rng[~nonempty, 1] - rng[~nonempty, 0] == 0)


def check_images(got, ref, masks, z_far):
    """Off masks[k] ([H,W] bool): colour within IMG_TOL, depth within DEPTH_TOL (of z_far), n_contrib equal, final_T within
    1e-5.  Anywhere: colour and depth within 2e-2."""
    for k, (g, o) in enumerate(zip(got, ref)):
        unstable = masks[k]
        dc = np.abs(g["color"] - o["color"]).max(axis=0)
        dd = np.abs(np.asarray(g["depth"])[0] - np.asarray(o["depth"])[0]) / z_far
        assert dc[~unstable].max() <= IMG_TOL, f"colour k={k}: {dc[~unstable].max()}"
        assert dd[~unstable].max() <= DEPTH_TOL, f"depth k={k}: {dd[~unstable].max()}"
        assert dc.max() <= ANYWHERE_TOL and dd.max() <= ANYWHERE_TOL
        s = ~unstable.reshape(-1)
        assert np.array_equal(np.asarray(g["n_contrib"]).reshape(-1)[s], np.asarray(o["n_contrib"]).reshape(-1)[s]), "n_contrib"
        assert np.abs(np.asarray(g["final_T"]).reshape(-1)[s] - np.asarray(o["final_T"]).reshape(-1)[s]).max() <= FINAL_T_TOL, \
            "final_T"


# ---------------------------------------------------------------- the product's packed layout in the plain keys
def plain_geometry(hip):
    """Per-subframe geometry dicts of a helpers.hip_forward_state result (48-byte rows: means2D | conic_opacity | rgb | depth)."""
    out = []
    for k in range(hip["K"]):
        rows = hip["rows"][k]
        out.append(dict(radii=hip["radii"][k], tiles_touched=hip["tiles_touched"][k], means2D=rows[:, 0:2], depths=rows[:, 9],
                        conic_opacity=rows[:, 2:6], rgb=rows[:, 6:9], pre_sigmoid=hip["pre_sigmoid"][k], cov3D=hip["cov3D"]))
    return out


def plain_binning(hip, counts):
    """Per-subframe binning dicts of a tile_cull = 0 helpers.hip_forward_state result, given the per-subframe duplicate
    counts: the fused key carries k * T on top of the tile id and the ranges index the concatenated list."""
    out, off, T = [], 0, hip["T"]
    for k, R in enumerate(counts):
        rng = hip["ranges"][k].astype(np.int64)
        rel = np.where((rng[:, 1] != rng[:, 0])[:, None], rng - off, 0)      # (an empty tile keeps its zero length)
        out.append(dict(num_rendered=R, keys=hip["keys"][off:off + R] - (np.uint64(k * T) << np.uint64(32)),
                        point_list=hip["point_list"][off:off + R], ranges=rel))
        off += R
    return out


def plain_images(hip):
    return [dict(color=hip["color"][k], depth=hip["depth"][k], n_contrib=hip["n_contrib"][k], final_T=hip["final_T"][k])
            for k in range(hip["K"])]

"""GPU parity tests at a general camera pose and at the frustum border (tests/posed_scenes.py): the checkers of
tests/test_gpu_parity.py, tests/test_gpu_evaluation.py and tests/test_gpu_configs.py, unchanged and with their default
bars, on a scene whose view matrix is a 1.04 rad rotation with the camera 6 units from the origin, with 600 splats around
the frustum -- beyond the 1.3 tanfov guard band (clamped t.x / t.y, x/y_grad_mul = 0: preprocess.hip, both kernels of
geometry_bwd.hip) and in the unclamped off-screen band -- and 150 Gaussians behind the camera, inside the near plane and
just past it.  tests/test_posed_scenes_host.py proves on the oracle that those branches are populated and
well-conditioned, and that a wrong camera centre moves the gradients by a hundred times the bar on this scene."""
import numpy as np
import pytest

import posed_scenes as PS
from helpers import (CLOUD_KEYS, GRAD_TOL, OracleRun, _t, assert_grads_close, cloud_grads_from_activated,
                     hip_cloud_forward_backward, hip_forward_backward, hip_forward_state, hip_settings, oracle_forward,
                     oracle_forward_backward, relerr, tile_cull)
from test_gpu_configs import kernel_activated_scene
from test_gpu_evaluation import _check_first_step_gradients, _fit_fixture, pose_only_vs_full
from test_gpu_parity import (GRAD_KEYS, _check_binning_bits, _check_forward_images, _check_preprocess_bits,
                             _check_tile_cull_subset, _grads, sharp_backward_check)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def posed(gpu):
    sc = PS.make("main")
    return sc, hip_forward_state(sc, sc["K"]), [oracle_forward(sc, k) for k in range(sc["K"])]


def test_preprocess_bit_exact(posed):
    """Radii, tiles touched, means2D, conic, depth and cov3D bits: the clamped t.x / t.y enter the conic and the radius."""
    sc, hip, ora = posed
    _check_preprocess_bits(sc, hip, ora)
    for k, o in enumerate(ora):
        c = PS.classes(sc, k)
        assert (o["radii"][c["clamped"]] > 0).sum() >= 200 and not o["radii"][c["near_culled"]].any()


def test_binning_bit_exact(posed):
    """Duplicate offsets, sort keys, point lists and tile ranges: the band's rectangles are clipped at the image border."""
    _check_binning_bits(*posed)


def test_tile_cull_lists_are_the_contributing_subset(posed):
    """The tile-culled lists against the rectangle lists (tests/test_gpu_parity.py, same statement): an order-preserving
    subset that drops no contributing duplicate and leaves images, radii and transmittance unchanged by a bit.  (How much
    of the rectangle lists survives is a property of the scene, not asserted here.)"""
    _check_tile_cull_subset(posed[0], ratio=(0.0, 1.0 + 1e-9))


def test_forward_images(posed):
    _check_forward_images(*posed)


@pytest.mark.parametrize("depth", [True, False])
def test_backward_vs_oracle(gpu, depth):
    """Every gradient under the per-component / per-Gaussian checker with its default bars.  Measured on the MI355X: every
    column within 2.3e-6 and every row within 6.8e-6, no exempt pixel, all 1890 active Gaussians well-conditioned; with
    x_grad_mul forced to 1 in geometry_bwd_kernel the dL_dmeans3D columns are 1.3e-2 ... 2.5e-2 off."""
    sc = PS.make("main")
    hip, run, _ = sharp_backward_check(sc, sc["K"], depth=depth)
    for k in range(sc["K"]):
        assert np.array_equal(hip["radii"][k], run.states[k]["radii"])


def test_backward_vs_oracle_sh_degree_3(gpu):
    """The MAXC > 9 instantiation of the geometry backward; the 16-coefficient SH direction runs through a campos six
    units from the origin."""
    sc = PS.make("main", sh_degree=3)
    assert sc["sh"].shape[1] == 16
    sharp_backward_check(sc, sc["K"])


@pytest.mark.parametrize("depth", [False, True])
def test_tile_cull_gradients_bitwise_equal(gpu, depth):
    sc = PS.make("main")
    gC, gD = _grads(sc, sc["K"], depth=depth)
    with tile_cull(False):
        a = hip_forward_backward(sc, sc["K"], gC, gD)
    with tile_cull(True):
        b = hip_forward_backward(sc, sc["K"], gC, gD)
    for key in GRAD_KEYS:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("cull", [True, False])
def test_pose_only_backward(gpu, cull):
    """dgs_backward_pose_only (its own restatement of the clamp and of the zero x/y_grad_mul) against dgs_backward on the
    same state and against the oracle, statistic and bar of tests/test_gpu_evaluation.py: relerr <= GRAD_TOL, K = 2.
    Measured on the MI355X (dL_dviewmatrix, dL_dprojmatrix), the same with both tile_cull settings: pose-only against
    full 3.6e-7, 1.1e-7; against the oracle 2.0e-6, 6.0e-7.  (With y_grad_mul forced to 1 in the pose-only kernel:
    dL_dviewmatrix 0.12 from the full backward.)"""
    sc = PS.make("main")
    K = sc["K"]
    gC, gD = _grads(sc, K)
    ora = oracle_forward_backward(sc, K, gC, gD)
    full, outs = pose_only_vs_full(sc, K, cull, gC, gD)
    for i, key in enumerate(("dL_dviewmatrix", "dL_dprojmatrix")):
        assert np.isfinite(full[i]).all() and np.abs(full[i]).max() > 0
        e_full, e_ora = relerr(outs[0][i], full[i]), relerr(outs[0][i].reshape(ora[key].shape), ora[key])
        print(f"\n[posed, tile_cull {cull}] {key}: pose-only vs full {e_full:.3e}, vs oracle {e_ora:.3e}")
        assert e_full <= GRAD_TOL, (key, e_full)
        assert e_ora <= GRAD_TOL, (key, e_ora)
        assert np.array_equal(outs[0][i], outs[1][i]) and np.array_equal(outs[0][i], outs[2][i]), key


def test_mark_visible(posed):
    """markVisible against numpy, z_view > 0.2 in float64 (no Gaussian of the scene lies within 1e-5 of the plane)."""
    from deblurgs_amd.diff_gaussian_rasterization import GaussianRasterizer
    sc = posed[0]
    for k in range(sc["K"]):
        z = PS.camera_space(sc, k)[:, 2]
        assert np.abs(z - PS.Z_NEAR_CULL).min() > 1e-5
        want = z > PS.Z_NEAR_CULL
        assert (~want).sum() >= 80 and (want & (z <= 0.26)).sum() >= 20
        vis = GaussianRasterizer(hip_settings(sc, 1)).markVisible(_t(sc["means3D"]), _t(sc["viewmatrix"][k]),
                                                                  _t(sc["projmatrix"][k]))
        assert np.array_equal(vis.cpu().numpy(), want), k


def test_raw_parameter_path(gpu):
    """The product path (GaussianCloud's raw parameters, activations inside the kernels, tile culling) against the oracle's
    gradients chained to the raw parameters: tests/test_gpu_configs.py's statement, default bars."""
    sc = PS.make("main")
    K = sc["K"]
    act = kernel_activated_scene(sc)
    run = OracleRun(act, K, exact=True)
    gC, gD = run.mask(*_grads(sc, K))
    hip = hip_cloud_forward_backward(sc, K, gC, gD, cull=True)
    for k in range(K):
        assert np.array_equal(hip["radii"][k], run.states[k]["radii"])
    assert_grads_close(hip, cloud_grads_from_activated(act, run.backward(gC, gD)), CLOUD_KEYS)


def test_fused_pose_fit_first_step_gradients_match_autograd_at_a_general_pose(gpu):
    """FusedPoseFit.gradients(idx) against render() + autograd (tests/test_gpu_evaluation.py's fixture, statement and bar)
    with the cloud and the three views moved by posed_scenes.rigid_move: the quaternion and translation the pose chain
    differentiates are those of a 1 rad rotation, where composing the update on the wrong side of the base rotation
    shows.  Measured on the MI355X (dL/dq, dL/dt): view 0 1.0e-5, 8.2e-6; view 1 3.3e-6, 3.6e-6; view 2 2.1e-5, 2.1e-5."""
    fixture = _fit_fixture(move=PS.rigid_move)
    for cam in fixture[1]:
        assert PS.rotation_angle(cam.R) >= 0.5
    _check_first_step_gradients(fixture)

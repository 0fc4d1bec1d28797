"""Host side of the posed scenes (tests/posed_scenes.py), on the CPU oracle alone: the main scene populates the branches
it was built for (clamped and off-screen splats with a gradient, near-culled Gaussians without one, all of them
well-conditioned) at a general pose, it tells a wrong camera centre from the right one by three orders of magnitude above
the gradient bar, the checker the GPU tests apply is met by the reference's own fp32 builds, and the oracle itself is
pinned to float64 autograd at such a pose with clamped Gaussians (tests/test_oracle_golden.py pins it at the identity pose
and inside the guard band only)."""
import numpy as np
import pytest

import posed_scenes as PS
import stack_scenes as S
from helpers import GRAD_TOL, OracleRun, assert_grads_close, grad_errors, oracle, oracle_forward

F64_BAR = 2e-4     # the bar of test_oracle_golden.py::test_oracle_backward_matches_float64_autograd


@pytest.fixture(scope="module")
def main():
    sc = PS.make("main")
    K = sc["K"]
    run = OracleRun(sc, K)
    gC, gD = run.mask(*S.upstream(sc, K))
    return sc, K, run, gC, gD, run.backward(gC, gD), [oracle.backward(run.states[k], gC[k], gD[k]) for k in range(K)]


def test_main_scene_populates_the_pose_and_border_branches(main):
    """Per subframe: >= 200 clamped Gaussians (|t.x / t.z| > 1.3 tanfovx or the same in y) with a non-zero dL_dmeans3D,
    >= 200 active Gaussians in the unclamped off-screen band, >= 80 Gaussians culled by z <= 0.2 with exactly zero gradient
    rows; none of the active band Gaussians ill-conditioned (noise as assert_grads_close computes it) for any chain output;
    view rotation >= 0.5 rad and |campos| >= 3.  Measured (subframe 0, 1): 368, 375 clamped and 367, 361 off-screen
    Gaussians with a gradient; 100, 110 near-culled; 755 active band Gaussians in all, their largest noise 4.0e-6
    (dL_drotations), none above WELL_ROW; rotation 1.041, 1.046 rad; |campos| 6.17."""
    sc, K, run, gC, gD, ora, per_k = main
    info = PS.conditions(sc, run, ora, per_k)
    print("\n[posed main] " + ", ".join(f"{k}: {v}" for k, v in info.items()))


def test_reference_builds_pass_the_checker_the_gpu_test_applies(main):
    """The oracle's fp32-accumulating and FMA-contracted builds against its double-accumulating build under
    assert_grads_close with its default ILL_FRAC / WELL_FRAC: were the band to push the scene's ill-conditioned share
    past them, no kernel could be held to the bars of tests/test_gpu_posed.py."""
    sc, K, run, gC, gD, ora, _ = main
    for mode in ("f32", "fma"):
        assert_grads_close(ora[mode], ora, S.CHECK_KEYS)


def test_main_scene_tells_a_wrong_camera_centre(main):
    """The oracle backward with campos = -viewmatrix[3,:3] (right only when R = I) against the true one, in the column
    measure of grad_errors: both dL_dsh and dL_dmeans3D must move by >= 100 x GRAD_TOL.  Measured (subframe 0, 1): dL_dsh
    2.0, 1.9; dL_dmeans3D 2.1e-2, 3.1e-2.  The same cloud before rigid_move: 1.5e-4, 9.4e-5 and 4.7e-6, 6.7e-6 -- at or
    below the bar.  (dL_dmeans3D feels campos only through the view-dependent SH coefficients, which posed_scenes.make
    scales by SH_REST_GAIN; with make_scene's own N(0, 0.05) draws it measured 0.7e-2 ... 1.3e-2, on either side of the
    1e-2 asked for here.)"""
    sc, K, run, gC, gD, _, per_k = main
    for k in range(K):
        st = dict(run.states[k])
        st["inputs"] = dict(st["inputs"], campos=np.ascontiguousarray(-sc["viewmatrix"][k][3, :3], dtype=np.float32))
        bad = oracle.backward(st, gC[k], gD[k])
        for key in ("dL_dsh", "dL_dmeans3D"):
            e = grad_errors(bad[key], per_k[k][key])["col"]
            print(f"\n[posed main k={k}] campos = -t: {key} moves by {e:.2e}")
            assert e >= 100 * GRAD_TOL, f"k={k} {key}: {e:.2e}"


@pytest.fixture(scope="module", params=[0, 1])
def pin(request):
    """Subframe k of the 400-Gaussian posed border scene through the oracle and through float64 autograd with the clamp
    written the reference's way and written plainly; upstream gradients zero on the oracle's margin mask."""
    k = request.param
    sc = PS.make("pin")
    st = oracle_forward(sc, k)
    un = oracle.unstable(st)
    gC, gD = (g[k] for g in S.upstream(sc, sc["K"]))
    gC[:, un] = 0.0
    gD[:, un] = 0.0
    gr = oracle.backward(st, gC, gD)
    gr = dict(gr, dL_dopacities=gr["dL_dopacity"])
    clamped = PS.classes(sc, k)["clamped"] & (np.abs(gr["dL_dmeans3D"]).max(axis=1) > 0)
    return k, sc, st, un, gr, clamped, S.float64_reference(sc, k, gC, gD, reference_clamp=True), S.float64_reference(sc, k, gC, gD)


def test_oracle_matches_float64_autograd_at_a_general_pose_with_clamped_gaussians(pin):
    """Image, radii, the five per-Gaussian gradients, dL_dviewmatrix and the two analytic columns of dL_dprojmatrix of the
    oracle against float64 autograd through oracle/torch_naive.py with reference_clamp=True, bar 2e-4 of each tensor's
    largest entry.  Measured (image; means3D, opacities, sh, scales, rotations, view, proj column 0, 1):
      k = 0: 5.0e-6; 1.2e-5, 5.8e-6, 4.5e-6, 5.1e-6, 2.0e-6, 1.7e-6, 9.3e-6, 1.6e-5   (78 clamped Gaussians with a gradient)
      k = 1: 5.3e-6; 3.2e-6, 9.6e-6, 3.8e-6, 5.3e-6, 3.8e-6, 6.6e-7, 4.7e-6, 1.3e-6   (77)
    and dL_dmeans3D on the clamped rows alone 1.8e-7, 1.4e-7 of the tensor's largest entry."""
    k, sc, st, un, gr, clamped, ref, _ = pin
    assert clamped.sum() >= 20, f"only {int(clamped.sum())} clamped Gaussians receive a gradient"
    assert PS.rotation_angle(sc["viewmatrix"][k][:3, :3]) >= 0.5
    assert np.array_equal(ref["radii"], st["radii"])
    img = float(np.abs(ref["color"] - st["color"]).max(axis=0)[~un].max())
    err = S.errors_to_float64(gr, ref)
    print(f"\n[posed pin k={k}] clamped with a gradient {int(clamped.sum())}, margin {int(un.sum())}, image {img:.2e}, "
          + ", ".join(f"{n} {e:.2e}" for n, e in err.items()))
    assert img <= F64_BAR
    for key, e in err.items():
        assert e <= F64_BAR, f"{key}: {e:.3e}"
    rows = np.abs(gr["dL_dmeans3D"] - ref["dL_dmeans3D"])[clamped].max() / np.abs(ref["dL_dmeans3D"]).max()
    print(f"[posed pin k={k}] dL_dmeans3D on the clamped rows: {rows:.2e}")
    assert rows <= F64_BAR


def test_plain_autograd_differs_on_the_clamped_rows(pin):
    """With reference_clamp off autograd differentiates clamp(x / z) * z through z, which the reference's backward does
    not: the clamped rows of dL_dmeans3D differ by >= 1e-3 of the tensor's largest entry, i.e. they carry weight far
    above the bar and the agreement above is not vacuous.  Measured (k = 0, 1): clamped rows 1.9e-2, 7.1e-3; the other rows
    1.2e-5, 3.2e-6; dL_dviewmatrix 0.15, 0.14."""
    k, sc, st, un, gr, clamped, _, plain = pin
    d = np.abs(gr["dL_dmeans3D"] - plain["dL_dmeans3D"])
    on, off = d[clamped].max() / np.abs(plain["dL_dmeans3D"]).max(), d[~clamped].max() / np.abs(plain["dL_dmeans3D"]).max()
    view = S.errors_to_float64(gr, plain)["dL_dviewmatrix"]
    print(f"\n[posed pin k={k}] plain autograd: dL_dmeans3D clamped rows {on:.2e}, other rows {off:.2e}, dL_dviewmatrix {view:.2e}")
    assert on >= 1e-3
    assert off <= F64_BAR

"""Posed scenes shared by tests/test_posed_scenes_host.py and tests/test_gpu_posed.py (no test lives here): a scene of
synthetic.make_scene taken away from the two properties every other parity scene has.

  * The camera of make_scene sits at the identity pose (viewmatrix = I + O(1e-2)), where a transposed W in the covariance
    chain, campos = -t instead of -R^T t, a pose update composed on the wrong side or an SH direction from the wrong origin
    are second-order or vanish.  rigid_move() moves the world and the cameras together by a large rigid transform: the
    picture stays (up to the SH colours, whose coefficients are not rotated), the matrices become general.
  * No Gaussian of make_scene lies outside the guard band |t.x / t.z| <= 1.3 tanfovx of the covariance Jacobian
    (forward.cu computeCov2D, backward.cu computeCov2DCUDA: the clamp of t.x, t.y and x_grad_mul / y_grad_mul = 0), and
    none that is off screen (1 < |ndc| <= 1.3) is large enough to reach the image.  border_band() puts splats there that
    are, and culled() puts Gaussians behind the camera, inside the near plane and just beyond it.

conditions(scene, run, ora) asserts, on the ORACLE alone, that a scene really populates those branches; numpy only."""
import numpy as np

from helpers import CHAIN_KEYS, ILL_ROW, WELL_ROW, row_errors, row_reference, synthetic

ROTVEC = 1.1 * np.array([0.5, -0.7, 0.4])      # 1.04 rad about a general axis
TRANS = np.array([3.0, -2.0, 5.0])
GUARD = 1.3                                    # the reference's guard band, in units of tanfov
Z_NEAR_CULL = 0.2                              # in_frustum: p_view.z <= 0.2 is culled
SH_REST_GAIN = 4.0                             # make_scene draws the view-dependent SH coefficients from N(0, 0.05): a colour that
                                               # hardly depends on the direction mean - campos cannot tell a wrong campos


def _rotmat(rotvec):
    """Rodrigues: rotation vector -> [3,3] matrix acting on column vectors, float64."""
    rotvec = np.asarray(rotvec, np.float64)
    ang = float(np.linalg.norm(rotvec))
    if ang == 0.0:
        return np.eye(3)
    x, y, z = rotvec / ang
    S = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], np.float64)
    return np.eye(3) + np.sin(ang) * S + (1.0 - np.cos(ang)) * (S @ S)


def _quat(rotvec):
    """Rotation vector -> unit quaternion (r, x, y, z), float64."""
    rotvec = np.asarray(rotvec, np.float64)
    ang = float(np.linalg.norm(rotvec))
    if ang == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * rotvec / ang])


def _quat_mul(a, b):
    """Hamilton product a * b of (r, x, y, z) quaternions; a [4], b [P,4]: the rotation of b followed by that of a."""
    ar, ax, ay, az = a
    br, bx, by, bz = b.T
    return np.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                     ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], axis=1)


def rigid_move(scene, rotvec=ROTVEC, t=TRANS):
    """The scene with world and cameras moved together by p' = R_g p + t; in the row-vector convention p' = p @ G with
    G[:3,:3] = R_g^T, G[3,:3] = t.  Means go through G, Gaussian quaternions are left-multiplied by R_g's,
    viewmatrix[k] = G^-1 @ viewmatrix[k] (float64, then float32), projmatrix[k] = viewmatrix[k] @ projection_matrix
    (float32), campos[k] = inv(viewmatrix[k])[3,:3].  Camera-space positions and covariances are those of `scene` up to
    float32 rounding; the SH coefficients are left as they are, so the colours -- evaluated along mean - campos in the
    moved world frame -- are another scene's, not the same picture."""
    Rg = _rotmat(rotvec)
    G = np.eye(4)
    G[:3, :3] = Rg.T
    G[3, :3] = np.asarray(t, np.float64)
    Ginv = np.linalg.inv(G)
    out = dict(scene)
    out["means3D"] = (scene["means3D"].astype(np.float64) @ Rg.T + G[3, :3]).astype(np.float32)
    out["rotations"] = _quat_mul(_quat(rotvec), scene["rotations"].astype(np.float64)).astype(np.float32)
    K = scene["viewmatrix"].shape[0]
    view = np.stack([(Ginv @ scene["viewmatrix"][k].astype(np.float64)).astype(np.float32) for k in range(K)])
    proj_T = scene["projection_matrix"].astype(np.float32)
    out["viewmatrix"] = view
    out["projmatrix"] = np.stack([view[k] @ proj_T for k in range(K)]).astype(np.float32)
    out["campos"] = np.stack([np.linalg.inv(view[k])[3, :3] for k in range(K)]).astype(np.float32)
    return out


def _place(scene, idx, ndcx, ndcy, z, sigma_px, rng, jitter=0.25):
    """Gaussians idx at camera-space (identity pose) NDC (ndcx, ndcy) and depth z, sigma_px pixels wide times a per-axis
    exp(N(0, jitter)); rotations are left as drawn."""
    focal = scene["W"] / (2.0 * scene["tanfovx"])
    scene["means3D"][idx] = np.stack([ndcx * scene["tanfovx"] * z, ndcy * scene["tanfovy"] * z, z], axis=1)
    scene["scales"][idx] = (np.abs(z) * sigma_px / focal)[:, None] * np.exp(rng.normal(0.0, jitter, (len(idx), 3)))


def border_band(scene, n, rng, ndc_range=(1.02, 1.7), sigma_clip=(2.0, 40.0), corner_frac=0.15):
    """Overwrites the first n Gaussians of a scene at the IDENTITY pose (call before rigid_move) by a band around the
    frustum: |ndc| ~ U[ndc_range] on a random side (left, right, top, bottom), the other coordinate ~ U[-1, 1]; corner_frac
    of them outside in x AND y; z ~ U[1.5, 8]; pixel sigma = the gap to the image edge / U[1, 2] clipped to sigma_clip (so
    that 3 sigma reaches 1.5 ... 3 gaps: into the image) times a per-axis exp(N(0, 0.25)); opacity ~ U[0.3, 0.9].  With the
    default range 3 in 5 lie beyond the guard band (clamped t.x / t.y, zero x/y_grad_mul), the others in the unclamped
    off-screen band 1 < |ndc| <= 1.3."""
    out = dict(scene)
    for key in ("means3D", "scales", "opacities"):
        out[key] = scene[key].copy()
    idx = np.arange(n)
    out_c = rng.uniform(ndc_range[0], ndc_range[1], n) * rng.choice([-1.0, 1.0], n)
    in_c = rng.uniform(-1.0, 1.0, n)
    horizontal = rng.random(n) < 0.5                    # outside in x (left / right) or in y (top / bottom)
    corner = rng.random(n) < corner_frac
    out_c2 = rng.uniform(ndc_range[0], ndc_range[1], n) * rng.choice([-1.0, 1.0], n)
    ndcx = np.where(horizontal, out_c, np.where(corner, out_c2, in_c))
    ndcy = np.where(horizontal, np.where(corner, out_c2, in_c), out_c)
    z = rng.uniform(1.5, 8.0, n)
    gap = np.hypot(np.maximum(np.abs(ndcx) - 1.0, 0.0) * 0.5 * scene["W"], np.maximum(np.abs(ndcy) - 1.0, 0.0) * 0.5 * scene["H"])
    sigma = np.clip(gap / rng.uniform(1.0, 2.0, n), sigma_clip[0], sigma_clip[1])
    _place(out, idx, ndcx, ndcy, z, sigma, rng)
    out["opacities"][idx, 0] = rng.uniform(0.3, 0.9, n)
    return out


def culled(scene, n_behind, n_near, rng):
    """Overwrites the LAST n_behind + n_near Gaussians of a scene at the identity pose: n_behind with camera-space
    z ~ U[-5, 0.2] anywhere in view (behind the camera or inside the near plane: radii = 0, no gradient), n_near with
    z in (0.2, 0.25] within half the view of the optical axis (the first depths the near cull lets through).  The near
    ones are 8 pixels wide and faint (opacity ~ U[0.01, 0.03]): d mean2D / d mean3D = focal / z is twenty times the
    scene's typical one there, and at the cloud's own size and opacity fifty such rows would set the scale of every
    column of dL_dmeans3D a thousand times above the other Gaussians' gradients -- which the column and row measures of
    the checker would then no longer see."""
    out = dict(scene)
    for key in ("means3D", "scales", "opacities"):
        out[key] = scene[key].copy()
    P = scene["P"]
    idx = np.arange(P - n_behind - n_near, P - n_near)
    _place(out, idx, rng.uniform(-1.0, 1.0, n_behind), rng.uniform(-1.0, 1.0, n_behind), rng.uniform(-5.0, 0.2, n_behind),
           np.full(n_behind, 2.5), rng)
    idx = np.arange(P - n_near, P)
    _place(out, idx, rng.uniform(-0.5, 0.5, n_near), rng.uniform(-0.5, 0.5, n_near), 0.25 - rng.uniform(0.0, 0.05, n_near),
           np.full(n_near, 8.0), rng)
    out["opacities"][idx, 0] = rng.uniform(0.01, 0.03, n_near)
    return out


# P, W, H, K, make_scene keywords, band size, culled (behind, near): the smallest shapes at which every branch is populated.
# Both draw near-isotropic splats (sigma_log 0.4).  With make_scene's default 0.8 the pin scene holds a 70-pixel splat
# (Gaussian 264) that carries the largest dL_drotations of subframe 0 and on whose row the oracle's OWN three builds sit
# 1.9e-4 ... 4.2e-4 from float64 autograd at the identity pose as well: an ill-conditioned row that says nothing about
# the pose or the clamp, above the 2e-4 bar the oracle is pinned to.
MAIN = (2400, 160, 112, 2, dict(sigma_px=2.5, sigma_log=0.4), 600, (100, 50))
PIN = (400, 80, 64, 2, dict(seed=3, sigma_log=0.4), 120, (30, 15))
N_BAND = {"main": MAIN[5], "pin": PIN[5]}


def make(which="main", band=True, move=True, **over):
    """The main scene (2400 Gaussians, 160 x 112, K = 2, 600 in the border band, 100 + 50 culled / near) or the oracle-pin
    scene (400, 80 x 64, K = 2, 120 in the band, 30 + 15); over: make_scene keywords (sh_degree = 3)."""
    P, W, H, K, kw, n, (n_behind, n_near) = MAIN if which == "main" else PIN
    kw = dict(kw, **over)
    sc = synthetic.make_scene(P, W, H, K=K, **kw)
    sc["sh"][:, 1:] *= SH_REST_GAIN
    if band:
        rng = np.random.default_rng(1000 + kw.get("seed", 0))
        sc = culled(border_band(sc, n, rng), n_behind, n_near, rng)
    return rigid_move(sc) if move else sc


def camera_space(scene, k):
    """float64 camera-space means of subframe k."""
    ph = np.concatenate([scene["means3D"].astype(np.float64), np.ones((scene["P"], 1))], axis=1)
    return ph @ scene["viewmatrix"][k].astype(np.float64)[:, :3]


def classes(scene, k):
    """Per Gaussian, for subframe k: `clamped` (past the near cull and |t.x / t.z| > 1.3 tanfovx or |t.y / t.z| > 1.3
    tanfovy), `offscreen` (past the near cull, outside the image, inside the guard band in both axes) and `near_culled`
    (z <= 0.2)."""
    p = camera_space(scene, k)
    front = p[:, 2] > Z_NEAR_CULL
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.abs(p[:, 0] / p[:, 2]) / scene["tanfovx"]
        v = np.abs(p[:, 1] / p[:, 2]) / scene["tanfovy"]
    m = np.maximum(u, v)
    return dict(clamped=front & (m > GUARD), offscreen=front & (m > 1.0) & (m <= GUARD), near_culled=~front)


def rotation_angle(R):
    return float(np.arccos(np.clip((np.trace(np.asarray(R, np.float64)) - 1.0) * 0.5, -1.0, 1.0)))


def noise_rows(ora, key):
    """Per Gaussian, how far two correct fp32 builds of the reference move its row of ora[.][key]: the noise of
    helpers.assert_grads_close, max(|f32 - double|, |fma - double|) in its row measure."""
    b = ora["double"][key]
    ref = row_reference(b)
    return np.maximum(row_errors(ora["f32"][key], b, _ref=ref)[0], row_errors(ora["fma"][key], b, _ref=ref)[0])


def conditions(scene, run, ora, per_subframe, min_clamped=200, min_offscreen=200, min_culled=80):
    """Asserts that the posed scene populates the branches it was built for.  run: helpers.OracleRun of the scene; ora:
    run.backward(...) of the masked upstream gradients (K-summed, three builds); per_subframe: [K] oracle.backward(...)
    of the same upstream gradients, one subframe each.  Returns the measured counts."""
    K = run.K
    info = dict(clamped_active=[], offscreen_active=[], near_culled=[], angle=[], campos=[])
    band = np.zeros(scene["P"], bool)
    for k in range(K):
        c = classes(scene, k)
        g = per_subframe[k]
        active = np.abs(g["dL_dmeans3D"]).max(axis=1) > 0
        radii = run.states[k]["radii"]
        info["clamped_active"].append(int((c["clamped"] & active).sum()))
        info["offscreen_active"].append(int((c["offscreen"] & active).sum()))
        info["near_culled"].append(int(c["near_culled"].sum()))
        band |= (c["clamped"] | c["offscreen"]) & active
        assert not radii[c["near_culled"]].any(), f"k={k}: a Gaussian with z <= 0.2 is visible"
        for key in ("dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dcov3D", "dL_dmeans2D"):
            assert not g[key][c["near_culled"]].any(), f"k={k}: {key} of a near-culled Gaussian is not zero"
        info["angle"].append(rotation_angle(scene["viewmatrix"][k][:3, :3]))
        info["campos"].append(float(np.linalg.norm(scene["campos"][k])))
    info["band"] = int(band.sum())
    info["band_noise_max"], info["band_above_well"] = {}, {}
    for key in sorted(CHAIN_KEYS & set(ora["double"])):
        noise = noise_rows(ora, key)
        info["band_noise_max"][key] = float(noise[band].max())
        info["band_above_well"][key] = int((noise[band] > WELL_ROW).sum())
        assert not (noise[band] > ILL_ROW).any(), f"{key}: {int((noise[band] > ILL_ROW).sum())} band Gaussians are ill-conditioned"
    for k in range(K):
        assert info["clamped_active"][k] >= min_clamped, f"k={k}: {info['clamped_active'][k]} clamped Gaussians with a gradient"
        assert info["offscreen_active"][k] >= min_offscreen, f"k={k}: {info['offscreen_active'][k]} active off-screen Gaussians"
        assert info["near_culled"][k] >= min_culled, f"k={k}: {info['near_culled'][k]} Gaussians with z <= 0.2"
        assert info["angle"][k] >= 0.5 and info["campos"][k] >= 3.0, (k, info["angle"][k], info["campos"][k])
    return info

"""Deterministic synthetic Gaussian clouds and SE(3)-Bezier trajectories (BASELINE.md
section 3).  There is no dataset on the GPU box, so bench.py, the parity tests and smoke() all draw their
inputs from here.  Pure numpy: the same bytes feed the CPU oracle and the HIP path.
"""
import math

import numpy as np

SH_C0 = 0.28209479177387814

# BASELINE.json configs (P, W, H, K, curve_order); "metric" is the configuration the headline metric is quoted on.
CONFIGS = {
    "cfg1": dict(P=1_000, W=256, H=256, K=1, C=3),
    "cfg2": dict(P=100_000, W=800, H=800, K=9, C=9),
    "cfg3": dict(P=1_000_000, W=1600, H=1200, K=15, C=3),
    "metric": dict(P=1_000_000, W=1920, H=1080, K=15, C=3),
    "cfg5": dict(P=5_000_000, W=3840, H=2160, K=31, C=5),
}


def projection_matrix(znear, zfar, fovx, fovy):
    """utils/graphics_utils.py:51-71 in float32 steps (torch.zeros(4,4) is float32 there)."""
    tan_y = math.tan(fovy / 2)
    tan_x = math.tan(fovx / 2)
    top, right = tan_y * znear, tan_x * znear
    bottom, left = -top, -right
    P = np.zeros((4, 4), np.float32)
    P[0, 0] = 2.0 * znear / (right - left)
    P[1, 1] = 2.0 * znear / (top - bottom)
    P[0, 2] = (right + left) / (right - left)
    P[1, 2] = (top + bottom) / (top - bottom)
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def _hat(v):
    x, y, z = v
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], np.float64)


def se3_exp_np(log_transform, eps=1e-4):
    """float64 numpy restatement of utils/pytorch3d_functions.py:373-457 for one 6-vector -> 4x4 (row-vector form)."""
    lt, lr = np.asarray(log_transform[:3], np.float64), np.asarray(log_transform[3:], np.float64)
    ang = math.sqrt(max(float(lr @ lr), eps))
    S = _hat(lr)
    S2 = S @ S
    R = (math.sin(ang) / ang) * S + ((1 - math.cos(ang)) / ang ** 2) * S2 + np.eye(3)
    V = np.eye(3) + S * ((1 - math.cos(ang)) / ang ** 2) + S2 * ((ang - math.sin(ang)) / ang ** 3)
    out = np.zeros((4, 4), np.float64)
    out[:3, :3] = R
    out[:3, 3] = V @ lt
    out[3, 3] = 1.0
    return out.T


def bezier_np(ctrl, t):
    """scene/bezier.py:54-83: ctrl [C+1,d], t [K] -> [K,d]; control point 0 is reached at t = 1."""
    C = ctrl.shape[0] - 1
    k = np.arange(C + 1)
    coeff = (t[:, None] ** (C - k)[None]) * ((1 - t)[:, None] ** k[None]) * np.array([math.comb(C, i) for i in k])
    return coeff @ ctrl


def make_camera(W, H, fovx_deg=60.0, znear=0.01, zfar=100.0):
    tanfovx = math.tan(math.radians(fovx_deg) * 0.5)
    tanfovy = tanfovx * H / W
    fovx = 2 * math.atan(tanfovx)
    fovy = 2 * math.atan(tanfovy)
    proj = projection_matrix(znear, zfar, fovx, fovy).T.copy()  # stored transposed like scene/cameras.py:58
    return dict(W=W, H=H, tanfovx=tanfovx, tanfovy=tanfovy, FoVx=fovx, FoVy=fovy, znear=znear, zfar=zfar,
                projection_matrix=proj)


def make_trajectory(K, curve_order, proj_T, seed=0, trans_sigma=0.01, rot_sigma=0.002):
    """K subframe cameras along an SE(3) Bezier around the identity pose (scene/motion.py:248-294)."""
    rng = np.random.default_rng(seed + 1000)
    ctrl_t = rng.normal(0.0, trans_sigma, (curve_order + 1, 3))
    ctrl_r = rng.normal(0.0, rot_sigma, (curve_order + 1, 3))
    nu = np.linspace(0.0, 1.0, K) if K > 1 else np.zeros(1)
    se3 = np.concatenate([bezier_np(ctrl_t, nu), bezier_np(ctrl_r, nu)], axis=1)
    view = np.zeros((K, 4, 4), np.float32)
    full = np.zeros((K, 4, 4), np.float32)
    campos = np.zeros((K, 3), np.float32)
    for k in range(K):
        c2w = se3_exp_np(se3[k])
        rot = c2w[:3, :3].T
        trans = c2w[3, :3]
        wv = np.eye(4, dtype=np.float32)
        wv[:3, :3] = rot.astype(np.float32)
        wv[3, :3] = (-trans @ rot).astype(np.float32)
        view[k] = wv
        full[k] = wv @ proj_T.astype(np.float32)
        campos[k] = np.linalg.inv(wv)[3, :3]
    return dict(viewmatrix=view, projmatrix=full, campos=campos, se3=se3.astype(np.float32), nu=nu.astype(np.float32),
                ctrl_trans=ctrl_t.astype(np.float32), ctrl_rot=ctrl_r.astype(np.float32))


LAYOUTS = ("uniform", "surfaces")
# layout="surfaces": the defaults of layout_args (see _surfaces_cloud)
SURFACES_DEFAULTS = dict(n_surfaces=16, child_frac=0.3, centre=0.9, z_range=(1.5, 9.0), extent=(0.05, 0.22), slope=0.3,
                         share_log=1.0, z_noise=0.01, sigma_min_px=1.0, sigma_tail=2.5, sigma_max_px=60.0, thin=0.1,
                         scale_log=0.3, clone_frac=1.0 / 3.0, clone_offset=0.05, split_shrink=1.6, split_offset=1.0,
                         opaque_frac=0.6, opaque=(0.7, 1.0), faint=(0.02, 0.2))


def _surfaces_cloud(rng, P, tanfovx, tanfovy, focal, args):
    """The cloud of layout="surfaces": a scene-shaped load -- clustered surfaces, empty regions, clone / split clusters
    as densification leaves them, and a heavy tail of splat sizes -- where the uniform layout gives every tile the same
    list.  All draws come from `rng` in the order written here.

      surfaces   n_surfaces patches: centre (u0, v0) ~ U[-centre, centre]^2 in NDC, depth z0 ~ U[z_range], NDC
                 half-extents a_u, a_v ~ U[extent], slopes s_u, s_v ~ N(0, slope); a patch's share of the base points
                 is proportional to a_u a_v exp(N(0, share_log))
      base       round((1 - child_frac) P) points, assigned to patches by those shares; with du, dv ~ U[-1, 1]:
                 u = u0 + a_u du, v = v0 + a_v dv, z = max(z0 (1 + s_u a_u du + s_v a_v dv) + N(0, z_noise) z0, 1),
                 mean = (u tanfovx z, v tanfovy z, z)
      scales     sigma_px = min(sigma_min_px U(0,1)^(-1 / sigma_tail), sigma_max_px): a power-law tail; per axis
                 z sigma_px / focal (1, 1, thin) exp(N(0, scale_log)): flat surfels
      rotations  normalised N(0, 1)^4: the thin axis points anywhere, edge-on to the camera included
      children   the other P - base points draw a parent among the base points with probability proportional to its
                 sigma_px; the first clone_frac of them are clones (parent scale, offset N(0,1)^3 clone_offset x the
                 parent's largest scale), the rest splits (parent scale / split_shrink, offset N(0,1)^3 split_offset x
                 the parent's largest scale); every child takes its parent's rotation; child z is clamped to >= 1
      opacity    bimodal: opaque_frac of the points U[opaque], the others U[faint]
    """
    a = dict(SURFACES_DEFAULTS)
    unknown = set(args or {}) - set(a)
    if unknown:
        raise ValueError(f"unknown layout_args {sorted(unknown)}; known: {sorted(a)}")
    a.update(args or {})
    S = int(a["n_surfaces"])
    if S < 1 or not 0.0 <= a["child_frac"] < 1.0:
        raise ValueError("layout_args: n_surfaces >= 1 and 0 <= child_frac < 1")
    n_base = max(1, min(P, int(round((1.0 - a["child_frac"]) * P))))
    n_child = P - n_base
    u0 = rng.uniform(-a["centre"], a["centre"], S)
    v0 = rng.uniform(-a["centre"], a["centre"], S)
    z0 = rng.uniform(a["z_range"][0], a["z_range"][1], S)
    a_u = rng.uniform(a["extent"][0], a["extent"][1], S)
    a_v = rng.uniform(a["extent"][0], a["extent"][1], S)
    s_u = rng.normal(0.0, a["slope"], S)
    s_v = rng.normal(0.0, a["slope"], S)
    share = a_u * a_v * np.exp(rng.normal(0.0, a["share_log"], S))
    surf = rng.choice(S, size=n_base, p=share / share.sum())
    du = rng.uniform(-1.0, 1.0, n_base)
    dv = rng.uniform(-1.0, 1.0, n_base)
    u = u0[surf] + a_u[surf] * du
    v = v0[surf] + a_v[surf] * dv
    z = z0[surf] * (1.0 + s_u[surf] * a_u[surf] * du + s_v[surf] * a_v[surf] * dv) \
        + rng.normal(0.0, a["z_noise"], n_base) * z0[surf]
    z = np.maximum(z, 1.0)
    mean_b = np.stack([u * tanfovx * z, v * tanfovy * z, z], axis=1)
    sigma_px = np.minimum(a["sigma_min_px"] * (1.0 - rng.uniform(0.0, 1.0, n_base)) ** (-1.0 / a["sigma_tail"]),
                          a["sigma_max_px"])
    scale_b = (z * sigma_px / focal)[:, None] * np.array([1.0, 1.0, a["thin"]]) \
        * np.exp(rng.normal(0.0, a["scale_log"], (n_base, 3)))
    q = rng.normal(0.0, 1.0, (n_base, 4))
    rot_b = q / np.linalg.norm(q, axis=1, keepdims=True)
    if n_child > 0:
        parent = rng.choice(n_base, size=n_child, p=sigma_px / sigma_px.sum())
        n_clone = int(round(a["clone_frac"] * n_child))
        clone = np.arange(n_child) < n_clone
        big = scale_b[parent].max(axis=1, keepdims=True)
        offset = rng.normal(0.0, 1.0, (n_child, 3)) * big * np.where(clone, a["clone_offset"], a["split_offset"])[:, None]
        mean_c = mean_b[parent] + offset
        mean_c[:, 2] = np.maximum(mean_c[:, 2], 1.0)
        scale_c = scale_b[parent] / np.where(clone, 1.0, a["split_shrink"])[:, None]
        means = np.concatenate([mean_b, mean_c])
        scales = np.concatenate([scale_b, scale_c])
        rotations = np.concatenate([rot_b, rot_b[parent]])
    else:
        means, scales, rotations = mean_b, scale_b, rot_b
    opaque = rng.uniform(0.0, 1.0, P) < a["opaque_frac"]
    opacities = np.where(opaque, rng.uniform(a["opaque"][0], a["opaque"][1], P),
                         rng.uniform(a["faint"][0], a["faint"][1], P))
    return (means.astype(np.float32), scales.astype(np.float32), rotations.astype(np.float32),
            opacities.reshape(P, 1).astype(np.float32))


def make_scene(P, W, H, K=1, curve_order=3, sh_degree=2, seed=0, sigma_px=1.5, sigma_log=0.8, max_sh_degree=None, *,
               layout="uniform", layout_args=None):
    """Synthetic cloud + camera + trajectory.  layout="uniform" (default): exactly as SURVEY.md section 8d prescribes --
    means uniform over the view, log-normal scales: every tile gets the same list.  layout="surfaces": a scene-shaped
    cloud (clustered surfaces, empty regions, clone / split clusters, a power-law tail of splat sizes; the recipe and the
    parameters layout_args may override are _surfaces_cloud's and SURFACES_DEFAULTS); sigma_px / sigma_log do not apply to
    it.  Camera, trajectory, SH and bg are made the same way for both, and both return the same keys, dtypes and shapes."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS} (got {layout!r})")
    if layout == "uniform" and layout_args is not None:
        raise ValueError("layout_args belongs to layout='surfaces'")
    rng = np.random.default_rng(seed)
    cam = make_camera(W, H)
    tanfovx, tanfovy = cam["tanfovx"], cam["tanfovy"]
    focal = W / (2.0 * tanfovx)
    if layout == "surfaces":
        means3D, scales, rotations, opacities = _surfaces_cloud(rng, P, tanfovx, tanfovy, focal, layout_args)
    else:
        z = rng.uniform(1.0, 10.0, P)
        u = rng.uniform(-1.15, 1.15, P)
        v = rng.uniform(-1.15, 1.15, P)
        means3D = np.stack([u * tanfovx * z, v * tanfovy * z, z], axis=1).astype(np.float32)
        sig = np.exp(rng.normal(math.log(sigma_px), sigma_log, (P, 3)))
        scales = (z[:, None] * sig / focal).astype(np.float32)
        q = rng.normal(0.0, 1.0, (P, 4))
        rotations = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        opacities = rng.uniform(0.05, 1.0, (P, 1)).astype(np.float32)
    Dmax = sh_degree if max_sh_degree is None else max_sh_degree
    M = (Dmax + 1) ** 2
    sh = np.zeros((P, M, 3), np.float32)
    sh[:, 0, :] = rng.normal(0.0, 1.0, (P, 3)) / SH_C0 * 0.3
    if M > 1:
        sh[:, 1:, :] = rng.normal(0.0, 0.05, (P, M - 1, 3))
    bg = rng.random(3).astype(np.float32)
    traj = make_trajectory(K, curve_order, cam["projection_matrix"], seed=seed)
    scene = dict(P=P, W=W, H=H, K=K, sh_degree=sh_degree, M=M, means3D=means3D, scales=scales, rotations=rotations,
                 opacities=opacities, sh=sh, bg=bg, z_near=0.2, z_far=100.0, scale_modifier=1.0)
    scene.update(cam)
    scene.update(traj)
    return scene


def make_config(name, seed=0, **over):
    cfg = dict(CONFIGS[name])
    cfg.update(over)
    extra = {k: over[k] for k in ("sigma_px", "sigma_log", "layout", "layout_args") if k in over}
    return make_scene(cfg["P"], cfg["W"], cfg["H"], K=cfg["K"], curve_order=cfg["C"], seed=seed,
                      sh_degree=over.get("sh_degree", 2), **extra)

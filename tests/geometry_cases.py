"""Cases and float64 reference of the per-Gaussian backward tested ALONE (tests/test_geometry_cases_host.py,
tests/test_gpu_geometry_bwd.py; no test lives here, and nothing here needs a GPU).

geometry_bwd_kernel<1|4|9|16> + pose_grad_reduce_kernel (deblurgs_amd/csrc/geometry_bwd.hip) read one 64-byte slot of
totals per (subframe, Gaussian) pair from the backward's scratch blob.  With those slots written by the test the kernel is
a pure function of constructed inputs: a linear functional of the totals S [K,P,10] whose coefficients are the derivatives
of the forward's per-pair quantities -- which oracle/torch_naive.py::preprocess gives under autograd in float64.

  make(name)             the scene (float32 arrays, as helpers' scenes), the call's keywords, the totals S, the oracle's
                         visibility [K,P], and for the raw-parameter cases the cloud's raw tensors
  reference(case, dtype) every output of dgs_backward_geometry + dgs_backward_pose for those totals
  conditions(case)       asserts, on the oracle and the float64 forward alone, that the case populates the branches it was
                         built for and that no decision of the forward sits where fp32 and float64 could take it differently

Cameras.  Three rigid poses in a base world whose y axis they share: A at the origin looking down +z; B, A turned by 180
degrees about y, at (0, 0, 10) looking back at A; C, A turned by 90 degrees, at (-5, 0, 5) looking down +x.  All three see
the region around (0, 0, 5); beyond B only A sees, behind A only B, far along +x only C, and a strip near (5.3, y, 10.6) is
seen by A and C.  Subframe k takes the pose ORDER names, moved sideways in its own frame by a fraction of a unit and turned
by a few hundredths of a radian, so that no two matrices are equal; for K >= 4 the first subframe is moved by 3 units to its
left and the last by 3 units along y, which gives each a strip of the far field that no other subframe sees (the "first" /
"last" groups).
The whole scene then goes through posed_scenes.rigid_move: general matrices.

Totals.  S = N(0, 1) * 10 ** U(-3, 0) per pair; a few pairs all-zero; for every column some Gaussians whose pairs hold that
column alone; pairs closer than NEAR_Z to their camera are scaled by (z / NEAR_Z) ** 2 -- d pixel / d mean = focal / z
there is tens of times the scene's typical one, and at full size a handful of such pairs would set the scale of every
column, which the column and row measures would then no longer see past (posed_scenes.culled makes its near splats faint
for the same reason).
"""
import functools

import numpy as np
import torch

import posed_scenes as PS
from helpers import GRAD_TOL, ROW_FLOOR, grad_errors, oracle_forward, row_errors, synthetic
from oracle import torch_naive as tn

W, H = 96, 64
NEAR_Z = 1.5
ORDER = {1: "A", 2: "AB", 3: "ABC", 4: "ABAC"}        # K >= 5: "ABACB" repeated
BLOCK = 256                                            # threads of a geometry_bwd_kernel block, 4 waves of 64
COND_MAX = 1e3                                         # float64 2-D covariance (with the +0.3 low-pass) of every visible pair
Z_MARGIN, BAND_MARGIN, CLAMP_MARGIN = 1e-3, 1e-4, 1e-4

BIG = frozenset({"patterns", "blocks", "guard"})
CASES = {
    # P, K, active SH degree D, SH degree of the storage Dmax, what conditions() requires, further keywords.  The image is
    # 96 x 64 (kmax: 32 x 32).  `require`: the visibility patterns need K >= 3 (and more than one Gaussian), the block
    # conditions a second block; k1, k2 and tiny_1 carry only the conditions every case carries (stable decisions,
    # condition number, the clamped share of the colours).
    "deg0": dict(P=700, K=5, D=0, require=BIG),
    "deg1": dict(P=700, K=5, D=1, require=BIG),
    "deg2": dict(P=700, K=5, D=2, require=BIG),
    "deg3": dict(P=700, K=5, D=3, require=BIG),
    "deg1_of_3": dict(P=700, K=3, D=1, Dmax=3, require=BIG),
    "sigmoid_deg3": dict(P=700, K=3, D=3, use_sigmoid=True, require=BIG),
    "sigmoid_deg2": dict(P=700, K=3, D=2, use_sigmoid=True, require=BIG),
    "colors_precomp": dict(P=700, K=3, D=0, colors=True, require=BIG),
    "cov3D_precomp": dict(P=700, K=3, D=2, cov=True, require=BIG),
    "scale_modifier": dict(P=300, K=2, D=2, scale_modifier=0.7, require=frozenset({"blocks", "guard"})),
    "raw": dict(P=700, K=3, D=3, raw=dict(scale_lb=0.001), require=BIG),
    "raw_iso": dict(P=700, K=3, D=1, raw=dict(scale_lb=0.001, isotropic=True), require=BIG),
    "raw_hinge": dict(P=700, K=3, D=1, Dmax=2, raw=dict(scale_lb=0.001, hinge=0.37), require=BIG),
    "k1": dict(P=257, K=1, D=2, require=frozenset()),
    "k2": dict(P=257, K=2, D=2, require=frozenset()),
    "k4": dict(P=257, K=4, D=2, require=frozenset({"patterns"})),
    "tiny_1": dict(P=1, K=3, D=2, require=frozenset()),
    "tiny_63": dict(P=63, K=3, D=2, require=frozenset({"patterns"})),
    "kmax": dict(P=300, K=128, D=1, W=32, H=32, require=BIG),
}

_POSE = {"A": (np.eye(3), np.zeros(3)),
         "B": (np.diag([-1.0, 1.0, -1.0]), np.array([0.0, 0.0, 10.0])),
         "C": (np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), np.array([-5.0, 0.0, 5.0]))}


def order(K):
    return ORDER[K] if K in ORDER else ("ABACB" * (K // 5 + 1))[:K]


def _cameras(K, rng):
    """[K] (R, t): columns of R are the camera's axes in the base world, t its position; p_cam = (p - t) @ R."""
    cams = []
    for k, name in enumerate(order(K)):
        R, t = _POSE[name]
        d = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), 0.0])
        if K >= 4 and k == 0:
            d[0] = -3.0
        if K >= 4 and k == K - 1:
            d[1] = 3.0
        cams.append((R @ PS._rotmat(rng.normal(0.0, 0.02, 3)), t + R @ d))
    return cams


def _layout(P, rng):
    """The group of every Gaussian index.  Whole waves of one group in block 0 (a wave with no visible lane next to one
    that has some), a whole block of one group where there are two blocks, the rest mixed."""
    mixed = ["all", "A", "B", "C", "AC", "all", "never", "first", "last", "A", "B", "C"]
    lab = np.array([mixed[i % len(mixed)] for i in rng.permutation(P)], dtype=object)
    if P == 1:
        lab[:] = "all"
    if P > BLOCK:
        lab[0:64], lab[64:128], lab[128:160], lab[160:192] = "A", "B", "C", "AC"
    if P >= 2 * BLOCK:
        lab[192:224] = "all"
        lab[BLOCK:2 * BLOCK] = "A"
    elif P > BLOCK:
        lab[BLOCK:] = "B" if P > BLOCK + 1 else "all"
    # band and culled Gaussians among the mixed ones
    free = np.arange(224 if P >= 2 * BLOCK else 192, BLOCK) if P > BLOCK else np.arange(P)
    if P >= 2 * BLOCK:
        free = np.concatenate([free, np.arange(2 * BLOCK, P)])
    n_band = 0 if P < 63 else (len(free) * (3 if len(free) < 100 else 2)) // 5
    n_cull = 0 if P < 63 else max(len(free) // 8, 6)
    pick = rng.permutation(free)
    lab[pick[:n_band]] = "band"
    lab[pick[n_band:n_band + n_cull - n_cull // 3]] = "behind"
    lab[pick[n_band + n_cull - n_cull // 3:n_band + n_cull]] = "near"
    if P > BLOCK:
        must = ["all", "never", "first", "last", "AC", "C"]
        for i, g in enumerate(pick[n_band + n_cull:]):
            lab[g] = must[i % len(must)]
    return lab


def _base_scene(P, K, D, Dmax, Wc, Hc, seed):
    """The cloud in the base world (float64 placement, float32 arrays) and the K cameras."""
    rng = np.random.default_rng(seed)
    cam = synthetic.make_camera(Wc, Hc)
    tx, ty = cam["tanfovx"], cam["tanfovy"]
    focal = Wc / (2.0 * tx)
    cams = _cameras(K, rng)
    lab = _layout(P, rng)
    means = np.zeros((P, 3))
    home_z = np.full(P, 5.0)
    sig = np.exp(rng.normal(np.log(1.8), 0.35, (P, 3)))

    def to_world(c, u, v, z):
        R, t = c
        return np.stack([u * tx * z, v * ty * z, z], axis=1) @ R.T + t

    for g in ("all", "A", "B", "C", "AC", "never", "first", "last"):
        idx = np.nonzero(lab == g)[0]
        n = len(idx)
        if n == 0:
            continue
        U = lambda a, b: rng.uniform(a, b, n)
        if g == "all":
            z = U(4.2, 5.8)
            means[idx] = to_world(_POSE["A"], U(-0.4, 0.4), U(-0.4, 0.4), z)
        elif g in ("A", "B", "never"):
            z = U(10.5, 14.0)
            means[idx] = to_world(_POSE["B" if g == "B" else "A"], U(-0.85, 0.85), U(-0.85, 0.85), z)
            if g == "never":
                means[idx, 1] += 40.0
        elif g == "C":
            z = U(11.5, 14.0)
            means[idx] = to_world(_POSE["C"], U(-0.3, 0.3), U(-0.85, 0.85), z)
        elif g == "AC":
            z = U(10.3, 11.0)
            means[idx] = np.stack([U(4.9, 5.7), U(-2.5, 2.5), z], axis=1)
        else:      # the strip of the far field that only the first / the last subframe sees
            # (small splats, 2 pixels of radius: on the 32-pixel image of `kmax` the strip is 6 pixels wide)
            z = U(10.6, 11.5)
            if g == "first":
                means[idx] = to_world(cams[0], -U(0.80, 0.95), U(-0.7, 0.7), z)
            else:
                means[idx] = to_world(cams[K - 1], U(-0.7, 0.7), U(0.80, 0.95), z)
            sig[idx] = 0.3 * np.exp(rng.normal(0.0, 0.1, (n, 3)))
        home_z[idx] = z
    sc = dict(P=P, W=Wc, H=Hc, K=K, sh_degree=D, M=(Dmax + 1) ** 2, z_near=0.2, z_far=100.0, scale_modifier=1.0)
    sc.update(cam)
    sc["means3D"] = means.astype(np.float32)
    sc["scales"] = (home_z[:, None] * sig / focal).astype(np.float32)
    q = rng.normal(0.0, 1.0, (P, 4))
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc["opacities"] = rng.uniform(0.05, 1.0, (P, 1)).astype(np.float32)
    # band and culled splats: posed_scenes' own generators in A's frame (the identity pose of the base world)
    band, behind, near = (np.nonzero(lab == g)[0] for g in ("band", "behind", "near"))
    if len(band) + len(behind) + len(near) > 0:
        n = len(band) + len(behind) + len(near)
        tmp = dict(P=n, W=Wc, H=Hc, tanfovx=tx, tanfovy=ty, means3D=np.zeros((n, 3), np.float32),
                   scales=np.ones((n, 3), np.float32), opacities=np.full((n, 1), 0.5, np.float32))
        tmp = PS.culled(PS.border_band(tmp, len(band), rng, sigma_clip=(2.0, 14.0)), len(behind), len(near), rng)
        dst = np.concatenate([band, behind, near])
        for key in ("means3D", "scales"):
            sc[key][dst] = tmp[key]
        sc["opacities"][band] = tmp["opacities"][:len(band)]
    # colours: relu(x + 0.5) clamps about a quarter of the channel values; view-dependent part as posed_scenes.make
    M = sc["M"]
    sh = np.zeros((P, M, 3), np.float32)
    sh[:, 0] = (rng.normal(-0.25, 0.4, (P, 3)) / synthetic.SH_C0).astype(np.float32)
    sh[:, 1:] = rng.normal(0.0, 0.05 * PS.SH_REST_GAIN, (P, M - 1, 3))
    sc["sh"] = sh
    sc["bg"] = rng.random(3).astype(np.float32)
    view = np.zeros((K, 4, 4))
    for k, (R, t) in enumerate(cams):
        view[k] = np.eye(4)
        view[k, :3, :3] = R
        view[k, 3, :3] = -t @ R
    sc["viewmatrix"] = view.astype(np.float32)
    sc["projmatrix"] = np.stack([sc["viewmatrix"][k] @ cam["projection_matrix"] for k in range(K)]).astype(np.float32)
    sc["campos"] = np.stack([t for _, t in cams]).astype(np.float32)
    return sc, lab


# ------------------------------------------------------------------------------------------------ float64 forward
def _oracle_kw(kw):
    return {k: kw[k] for k in ("sh_degree", "use_sigmoid", "colors_precomp", "cov3D_precomp", "scale_modifier") if k in kw}


def oracle_radii(scene, kw):
    """[K,P] int32: the radii of the CPU oracle's preprocess (fp32, the reference's own arithmetic); visible = radii > 0."""
    return np.stack([oracle_forward(scene, k, render=False, **_oracle_kw(kw))["radii"] for k in range(scene["K"])])


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _leaves(case, dtype, grad):
    """The differentiable inputs (`leaf`) and the activated tensors preprocess takes (`act`), in dtype."""
    sc, kw, raw = case["scene"], case["kw"], case.get("raw")
    mk = lambda a: _t(a, dtype).requires_grad_(grad)
    leaf, act = {}, {}
    if raw is None:
        leaf["means3D"] = mk(sc["means3D"])
        leaf["opacity"] = mk(sc["opacities"].reshape(-1))
        act["opacity"] = leaf["opacity"]
        if kw.get("colors_precomp") is not None:
            leaf["colors"] = act["colors"] = mk(kw["colors_precomp"])
        else:
            leaf["sh"] = act["sh"] = mk(sc["sh"])
        if kw.get("cov3D_precomp") is not None:
            leaf["cov3D"] = act["cov3D"] = mk(kw["cov3D_precomp"])
        else:
            leaf["scales"], leaf["rotations"] = mk(sc["scales"]), mk(sc["rotations"])
            act["scales"], act["rotations"] = leaf["scales"], leaf["rotations"]
    else:      # the torch getters of deblurgs_amd/cloud.py on the raw tensors
        leaf["means3D"] = mk(raw["xyz"])
        leaf["opacity"] = mk(raw["opacity"].reshape(-1))
        act["opacity"] = leaf["opacity"].clamp(0.0, 1.0)
        leaf["f_dc"], leaf["f_rest"] = mk(raw["f_dc"]), mk(raw["f_rest"])
        act["sh"] = torch.cat((leaf["f_dc"], leaf["f_rest"]), dim=1)
        leaf["scales"], leaf["rotations"] = mk(raw["scaling"]), mk(raw["rotation"])
        s = leaf["scales"][:, :1].expand(-1, 3) if raw["isotropic"] else leaf["scales"]
        act["scales"] = torch.exp(s) + raw["scale_lb"]
        act["rotations"] = torch.nn.functional.normalize(leaf["rotations"])
        if raw["isotropic"] and grad:
            # the 3-D covariance formed here and handed over as cov3D_precomp (the same function of the leaves): its
            # gradient is the scale of the terms that cancel in dL_drotations, which is exactly zero for s^2 I (A_rot)
            RS = tn.quat_to_rotmat(act.pop("rotations")) * act.pop("scales")[:, None, :]
            Sg = RS @ RS.transpose(1, 2)
            act["cov3D"] = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], dim=1)
            act["cov3D"].retain_grad()
    act["means3D"] = leaf["means3D"]
    return leaf, act


def _preprocess(case, act, V, F, k, sel, dtype):
    sc, kw = case["scene"], case["kw"]
    pick = lambda name: None if name not in act else act[name][sel]
    return tn.preprocess(act["means3D"][sel], act["opacity"][sel], V, F, _t(sc["campos"][k], dtype), sc["W"], sc["H"],
                         sc["tanfovx"], sc["tanfovy"], sh=pick("sh"), colors_precomp=pick("colors"), scales=pick("scales"),
                         rotations=pick("rotations"), cov3D_precomp=pick("cov3D"), sh_degree=kw["sh_degree"],
                         scale_modifier=kw.get("scale_modifier", 1.0), use_sigmoid=kw.get("use_sigmoid", False),
                         reference_clamp=True)


def forward64(case):
    """Per subframe, the float64 forward of EVERY Gaussian (no visibility selection): preprocess's dict plus `rawcol`, the
    colour before its activation (None with precomputed colours)."""
    sc, kw = case["scene"], case["kw"]
    out = []
    with torch.no_grad():
        _, act = _leaves(case, torch.float64, False)
        allg = torch.arange(sc["P"])
        for k in range(sc["K"]):
            g = _preprocess(case, act, _t(sc["viewmatrix"][k], torch.float64), _t(sc["projmatrix"][k], torch.float64), k,
                            allg, torch.float64)
            g["rawcol"] = None
            if "sh" in act:
                d = act["means3D"] - _t(sc["campos"][k], torch.float64)[None]
                g["rawcol"] = tn.eval_sh_color(kw["sh_degree"], act["sh"], d / d.norm(dim=1, keepdim=True))
            out.append(g)
    return out


def decisions(case, fwd=None):
    """What conditions() and the repair loop look at, [K,P] each: depth, the guard-band ratios minus their limit, the
    condition number of the 2-D covariance, the smallest |raw colour + 0.5| of the three channels."""
    sc = case["scene"]
    fwd = forward64(case) if fwd is None else fwd
    z = np.stack([g["p_view"][:, 2].numpy() for g in fwd])
    with np.errstate(divide="ignore", invalid="ignore"):
        ux = np.stack([np.abs(g["p_view"][:, 0].numpy() / g["p_view"][:, 2].numpy()) for g in fwd]) - PS.GUARD * sc["tanfovx"]
        uy = np.stack([np.abs(g["p_view"][:, 1].numpy() / g["p_view"][:, 2].numpy()) for g in fwd]) - PS.GUARD * sc["tanfovy"]
        con = np.stack([g["conic"].numpy() for g in fwd])
        mid = 0.5 * (con[..., 0] + con[..., 2])
        disc = np.sqrt(np.maximum(mid * mid - (con[..., 0] * con[..., 2] - con[..., 1] ** 2), 0.0))
        cond = (mid + disc) / (mid - disc)
    col = None
    if fwd[0]["rawcol"] is not None:
        col = np.stack([np.abs(g["rawcol"].numpy() + 0.5).min(axis=1) for g in fwd])
    vis64 = np.stack([g["visible"].numpy() for g in fwd])
    return dict(z=z, ux=ux, uy=uy, cond=cond, col=col, vis64=vis64)


def _unstable(case, vis, margin=2.0):
    """Per Gaussian: (mean must move, colour must move, scale must round) for the repair loop of make()."""
    d = decisions(case)
    move = (np.abs(d["z"] - PS.Z_NEAR_CULL) < margin * Z_MARGIN) | (d["vis64"] != vis)
    front = d["z"] > PS.Z_NEAR_CULL
    move |= front & ((np.abs(d["ux"]) < margin * BAND_MARGIN) | (np.abs(d["uy"]) < margin * BAND_MARGIN))
    colour = np.zeros_like(move) if d["col"] is None or case["kw"].get("use_sigmoid") else vis & (d["col"] < margin * CLAMP_MARGIN)
    rounder = vis & ~(d["cond"] < 0.5 * COND_MAX)
    return move.any(axis=0), colour.any(axis=0), rounder.any(axis=0)


# ------------------------------------------------------------------------------------------------------- the cases
def _cov3D(sc, modifier=1.0):
    s, q = modifier * sc["scales"].astype(np.float64), sc["rotations"].astype(np.float64)
    R = tn.quat_to_rotmat(torch.from_numpy(q)).numpy()
    Mm = R * s[:, None, :]
    S = Mm @ Mm.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32)


def _activate_raw(raw):
    """float32 activations of the raw tensors, as the oracle is handed them (the kernels' own expf may differ by an ulp)."""
    s = raw["scaling"][:, :1].repeat(3, axis=1) if raw["isotropic"] else raw["scaling"]
    scales = (np.exp(s.astype(np.float32)) + np.float32(raw["scale_lb"])).astype(np.float32)
    q = raw["rotation"].astype(np.float32)
    rot = (q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    return scales, rot, np.clip(raw["opacity"], 0.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make(name, seed=0):
    """The case: dict(name, scene, kw, S [K,P,10] float32, visible [K,P], raw or None, groups, require)."""
    spec = dict(CASES[name])
    P, K, D = spec["P"], spec["K"], spec["D"]
    Dmax = spec.get("Dmax", D)
    sc, lab = _base_scene(P, K, D, Dmax, spec.get("W", W), spec.get("H", H), 100 + seed + sum(map(ord, name)))
    sc = PS.rigid_move(sc)
    rng = np.random.default_rng(7 + seed + sum(map(ord, name)))
    kw = dict(sh_degree=D, use_sigmoid=bool(spec.get("use_sigmoid")), scale_modifier=float(spec.get("scale_modifier", 1.0)))
    case = dict(name=name, scene=sc, kw=kw, raw=None, groups=lab, require=spec["require"])
    rawspec = spec.get("raw")
    if rawspec is not None:
        sc["scales"] = np.maximum(sc["scales"], np.float32(4 * rawspec["scale_lb"]))
        if rawspec.get("isotropic"):
            sc["scales"] = np.repeat(np.exp(np.log(sc["scales"]).mean(axis=1, keepdims=True)), 3, axis=1).astype(np.float32)
    # repair: move what sits on a decision threshold of the forward (see conditions)
    for it in range(12):
        if spec.get("colors"):
            kw["colors_precomp"] = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32) if it == 0 else kw["colors_precomp"]
        if spec.get("cov"):
            kw["cov3D_precomp"] = _cov3D(sc)
        radii = oracle_radii(sc, kw)
        vis = radii > 0
        move, colour, rounder = _unstable(case, vis)
        if not (move.any() or colour.any() or rounder.any()):
            break
        sc["means3D"][move] += rng.normal(0.0, 0.02, (int(move.sum()), 3)).astype(np.float32)
        sc["sh"][colour, 0] += np.float32(0.05)
        sc["scales"][rounder] = np.exp(np.log(sc["scales"][rounder]).mean(axis=1, keepdims=True) - 0.3).astype(np.float32)
    else:
        raise AssertionError(f"{name}: the repair loop did not settle")
    if rawspec is not None:
        lb = rawspec["scale_lb"]
        gain = rng.uniform(0.5, 2.0, (P, 1))
        scaling = np.log(sc["scales"].astype(np.float64) - lb).astype(np.float32)
        if rawspec.get("isotropic"):      # columns 1 and 2 of an isotropic cloud's _scaling are never read
            scaling[:, 1:] = rng.normal(0.0, 1.0, (P, 2)).astype(np.float32)
        op = sc["opacities"].reshape(-1).copy()
        special = rng.permutation(min(P, 224))[:48]
        op[special[0:12]], op[special[12:24]] = 0.0, 1.0
        op[special[24:36]] = rng.uniform(-0.5, -0.01, 12).astype(np.float32)
        op[special[36:48]] = rng.uniform(1.01, 1.5, 12).astype(np.float32)
        raw = dict(xyz=sc["means3D"], f_dc=np.ascontiguousarray(sc["sh"][:, :1]), f_rest=np.ascontiguousarray(sc["sh"][:, 1:]),
                   opacity=op.reshape(P, 1), scaling=scaling, rotation=(sc["rotations"] * gain).astype(np.float32),
                   scale_lb=lb, isotropic=bool(rawspec.get("isotropic")), hinge=float(rawspec.get("hinge", 0.0)))
        sc["scales"], sc["rotations"], opa = _activate_raw(raw)
        sc["opacities"] = opa.reshape(P, 1)
        case["raw"] = raw
        radii = oracle_radii(sc, kw)
        vis = radii > 0
    case["radii"], case["visible"] = radii, vis
    # the totals
    S = rng.normal(0.0, 1.0, (K, P, 10)) * 10.0 ** rng.uniform(-3.0, 0.0, (K, P, 1))
    S[rng.random((K, P)) < 0.03] = 0.0
    seen = np.nonzero(vis.any(axis=0))[0]
    alone = {}
    if len(seen) >= 20:
        pick = rng.permutation(seen)[:20].reshape(10, 2)
        for c in range(10):
            keep = S[:, pick[c], c].copy()
            S[:, pick[c], :] = 0.0
            S[:, pick[c], c] = np.where(keep == 0.0, 1e-2, keep)
            alone[c] = pick[c]
    z = decisions(case)["z"]
    S *= np.where((z > 0) & (z < NEAR_Z), (z / NEAR_Z) ** 2, 1.0)[..., None]
    case["S"] = S.astype(np.float32)
    case["alone"] = alone
    return case


# --------------------------------------------------------------------------------------------------- the reference
def reference(case, dtype=torch.float64, S=None, subframes=None, hinge=True):
    """Every output of dgs_backward_geometry + dgs_backward_pose for the totals S (default: the case's) of the subframes
    `subframes` (default: all), as float64 numpy: autograd through preprocess(reference_clamp=True) evaluated in `dtype`.

        loss = sum over k and the visible pairs of
               <pix, G_pix> + <conic, (-0.5 S2, -S3, -0.5 S4)> + opacity * S5 / opacity_row + <colour, S[6:9]> + depth * S9
        G_pix = -(cx S0 + cy S1, cz S1 + cy S0),    the row's conic (cx, cy, cz) and opacity detached

    (-0.5 S3 is the reference's sink dL_dconic.y, which holds HALF the derivative -- the off-diagonal element appears twice in
    the quadratic form -- and its cov2D backward doubles it again, backward.cu:214,633: the weight of conic.y is -S3.)
    Two more places where the reference's backward is not the derivative of its forward, and the kernel -- pinned to the
    reference's own kernels by tests/test_gpu_reference_kernels.py -- follows it; both were found by this test:
      * the conic backward multiplies by 1 / (det^2 + 1e-7) where the derivative of (c, -b, a) / det has 1 / det^2
        (backward.cu:208-214): the gradient that passes through the conic is scaled by det^2 / (det^2 + 1e-7) here, which
        is 1 - 1.2e-5 for the smallest splat the +0.3 low-pass allows (det = 0.09);
      * computeCov3D's dL_dscale is the derivative with respect to s = scale_modifier * scale, without the factor
        scale_modifier that d s / d scale is (backward.cu:316,343-346): autograd's dL_dscales is divided by it here.
    Plus opacity_hinge_scale * sum(x^2 [x <= 0] + (x - 1)^2 [x >= 1]) over the raw opacities.  dL_dmeans2D is G_pix scaled by
    (0.5 W, 0.5 H); dL_dprojmatrix is no analytic gradient in the reference (backward.cu:423-450) and is restated here in
    numpy float64; A_view / A_proj are the per-entry sums of the absolute values of the terms of the two matrices.
    Isotropic cloud: dL_drotations is exactly zero in exact arithmetic (the covariance s^2 I does not depend on the rotation),
    so what any evaluation returns is the rounding residue of terms that cancel; A_rot [P,1] = s^2 sum|dL/dSigma| / |q| is
    the scale of those terms, and the residue is measured against it."""
    sc, kw, raw = case["scene"], case["kw"], case.get("raw")
    P, Wc, Hc = sc["P"], sc["W"], sc["H"]
    S = case["S"] if S is None else S
    ks = list(range(sc["K"])) if subframes is None else list(subframes)
    leaf, act = _leaves(case, dtype, True)
    V = _t(sc["viewmatrix"], dtype).requires_grad_(True)
    F = _t(sc["projmatrix"], dtype)
    loss = torch.zeros((), dtype=dtype)
    m2d = np.zeros((len(ks), P, 3))
    gproj, aproj = np.zeros((len(ks), 4, 4)), np.zeros((len(ks), 4, 4))
    kept = []
    for i, k in enumerate(ks):
        sel = torch.from_numpy(np.nonzero(case["visible"][k])[0])
        if len(sel) == 0:
            kept.append(None)
            continue
        g = _preprocess(case, act, V[k], F[k], k, sel, dtype)
        g["p_view"].retain_grad()
        s = _t(S[k], dtype)[sel]
        con, opr = g["conic"].detach(), g["opacity"].detach()
        gpix = -torch.stack([con[:, 0] * s[:, 0] + con[:, 1] * s[:, 1], con[:, 2] * s[:, 1] + con[:, 1] * s[:, 0]], dim=1)
        wcon = torch.stack([-0.5 * s[:, 2], -s[:, 3], -0.5 * s[:, 4]], dim=1)
        dop = torch.where(opr > 0, s[:, 5] / torch.where(opr > 0, opr, torch.ones_like(opr)), torch.zeros_like(opr))
        # the reference's conic backward divides by (det^2 + 1e-7) where the derivative has det^2 (see above)
        det = 1.0 / (con[:, 0] * con[:, 2] - con[:, 1] * con[:, 1])
        conic = con + (g["conic"] - con) * (det * det / (det * det + 0.0000001))[:, None]
        loss = loss + ((g["pix"] * gpix).sum() + (conic * wcon).sum() + (g["opacity"] * dop).sum()
                       + (g["color"] * s[:, 6:9]).sum() + (g["depth"] * s[:, 9]).sum())
        kept.append((sel, g["p_view"]))
        g2 = gpix.double().numpy() * np.array([0.5 * Wc, 0.5 * Hc])
        m2d[i, sel.numpy(), :2] = g2
        # dL_dprojmatrix: mat[12..20] of geometry_bwd_kernel
        ph = np.concatenate([act["means3D"].detach().double().numpy()[sel.numpy()], np.ones((len(sel), 1))], axis=1)
        hom = ph @ sc["projmatrix"][k].astype(np.float64)
        m_w = 1.0 / (hom[:, 3] + 0.0000001)
        tx_ = 0.5 * g2[:, 0:1] * ph * Wc * m_w[:, None]
        ty_ = 0.5 * g2[:, 1:2] * ph * Hc * m_w[:, None]
        last = -0.5 * (hom[:, 0] * Wc * g2[:, 0] + hom[:, 1] * Hc * g2[:, 1]) * m_w * m_w
        gproj[i, :, 0], gproj[i, :, 1], gproj[i, :, 3] = tx_.sum(axis=0), ty_.sum(axis=0), last.sum()
        aproj[i, :, 0], aproj[i, :, 1], aproj[i, :, 3] = np.abs(tx_).sum(axis=0), np.abs(ty_).sum(axis=0), np.abs(last).sum()
    if raw is not None and hinge and raw["hinge"] != 0.0:
        x = leaf["opacity"]
        loss = loss + raw["hinge"] * (torch.where(x <= 0, x * x, torch.zeros_like(x))
                                      + torch.where(x >= 1, (x - 1) ** 2, torch.zeros_like(x))).sum()
    if loss.requires_grad:
        loss.backward()
    grad = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
    out = dict(dL_dmeans3D=grad(leaf["means3D"]), dL_dopacity=grad(leaf["opacity"]), dL_dmeans2D=m2d,
               dL_dprojmatrix=gproj, A_proj=aproj)
    if "colors" in leaf:
        out["dL_dcolors"] = grad(leaf["colors"])
    elif raw is None:
        out["dL_dsh"] = grad(leaf["sh"])
    else:
        out["dL_dsh"] = np.concatenate([grad(leaf["f_dc"]), grad(leaf["f_rest"])], axis=1)
    if "cov3D" in leaf:
        out["dL_dcov3D"] = grad(leaf["cov3D"])
    else:
        # dL_dscales as the reference returns it: the derivative with respect to scale_modifier * scale (see above)
        out["dL_dscales"] = grad(leaf["scales"]) / kw.get("scale_modifier", 1.0)
        out["dL_drotations"] = grad(leaf["rotations"])
    gv = grad(V)[ks]
    av = np.zeros((len(ks), 4, 4))
    means = act["means3D"].detach().double().numpy()
    for i, kp in enumerate(kept):
        if kp is not None and kp[1].grad is not None:
            ph = np.abs(np.concatenate([means[kp[0].numpy()], np.ones((len(kp[0]), 1))], axis=1))
            av[i, :, :3] = ph.T @ np.abs(kp[1].grad.double().numpy())
    out["dL_dviewmatrix"], out["A_view"] = gv, av
    if raw is not None and raw["isotropic"] and act["cov3D"].grad is not None:
        s2 = (np.exp(raw["scaling"][:, 0].astype(np.float64)) + raw["scale_lb"]) ** 2
        out["A_rot"] = (np.abs(act["cov3D"].grad.double().numpy()).sum(axis=1) * s2
                        / np.linalg.norm(raw["rotation"].astype(np.float64), axis=1))[:, None]
    return out


PER_GAUSSIAN = ("dL_dmeans3D", "dL_dsh", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dcov3D")


def output_keys(case):
    """The keys of reference() that are outputs of the kernel, per-Gaussian ones first."""
    kw = case["kw"]
    keys = ["dL_dmeans3D", "dL_dcolors" if kw.get("colors_precomp") is not None else "dL_dsh", "dL_dopacity"]
    keys += ["dL_dcov3D"] if kw.get("cov3D_precomp") is not None else ["dL_dscales", "dL_drotations"]
    return keys + ["dL_dmeans2D", "dL_dviewmatrix", "dL_dprojmatrix"]


# -------------------------------------------------------------------------------------------------- the conditions
def patterns(vis):
    """The set of per-Gaussian visibility patterns over the subframes, as strings of 0 / 1."""
    return {"".join("1" if v else "0" for v in vis[:, g]) for g in range(vis.shape[1])}


def conditions(case):
    """Asserts that the case populates what it was built for (by case["require"]) and that every decision of the forward is
    stable; returns the measured counts.

      patterns   always, never, visible - invisible - visible (1 0 1), invisible - visible - invisible (0 1 0), the first
                 subframe only, the last subframe only
      blocks     a block of 256 consecutive Gaussians with a wave that has no visible lane in a subframe in which another
                 wave of the block has one; a block that is entirely invisible in a subframe (and visible in another)
      guard      >= 8 visible pairs outside the guard band in x, >= 8 in y
      always     relu colours: 10 .. 50 % of the visible channel values clamped, none with |raw + 0.5| < 1e-4; no pair with
                 |p_view.z - 0.2| < 1e-3 or ||t / z| - 1.3 tanfov| < 1e-4 (in front of the near plane); the float64 forward
                 and the oracle agree on the visible pairs; the float64 2-D covariance of every visible pair has a
                 condition number below 1e3; raw cases: opacities exactly 0, exactly 1, below 0 and above 1"""
    sc, kw, vis, need = case["scene"], case["kw"], case["visible"], case["require"]
    K, P = vis.shape
    fwd = forward64(case)
    d = decisions(case, fwd)
    info = dict(visible_pairs=int(vis.sum()), order=order(K))
    assert (d["vis64"] == vis).all(), f"{int((d['vis64'] != vis).sum())} pairs are visible to one of oracle / float64 only"
    assert not (np.abs(d["z"] - PS.Z_NEAR_CULL) < Z_MARGIN).any(), "a pair sits on the near plane"
    front = d["z"] > PS.Z_NEAR_CULL
    assert not (front & ((np.abs(d["ux"]) < BAND_MARGIN) | (np.abs(d["uy"]) < BAND_MARGIN))).any(), "a pair sits on the guard band"
    info["cond_max"] = float(d["cond"][vis].max()) if vis.any() else 0.0
    assert info["cond_max"] < COND_MAX, f"condition number {info['cond_max']:.3g}"
    info["outside_x"], info["outside_y"] = int((vis & (d["ux"] > 0)).sum()), int((vis & (d["uy"] > 0)).sum())
    if d["col"] is not None and not kw.get("use_sigmoid"):
        raw3 = np.stack([g["rawcol"].numpy() for g in fwd])[vis]
        info["clamped_frac"] = float((raw3 + 0.5 < 0).mean()) if raw3.size else 0.0
        assert not (np.abs(raw3 + 0.5) < CLAMP_MARGIN).any(), "a colour channel sits on the clamp"
        if P >= 63:
            assert 0.10 <= info["clamped_frac"] <= 0.50, f"clamped share {info['clamped_frac']:.3f}"
    if case.get("raw") is not None:
        op = case["raw"]["opacity"].reshape(-1)
        info["raw_opacity"] = [int((op == 0.0).sum()), int((op == 1.0).sum()), int((op < 0).sum()), int((op > 1).sum())]
        assert min(info["raw_opacity"]) > 0, info["raw_opacity"]
    pats = patterns(vis)
    info["patterns"] = len(pats)
    if "patterns" in need:
        import re
        assert K >= 3
        want = {"always": "1" * K, "never": "0" * K, "first only": "1" + "0" * (K - 1), "last only": "0" * (K - 1) + "1"}
        for what, p in want.items():
            assert p in pats, f"no Gaussian is visible in the pattern '{what}' ({sorted(pats)[:12]} ...)"
        assert any(re.search("10+1", p) for p in pats), "no pattern 1 0 1"
        assert any(re.search("01+0", p) for p in pats), "no pattern 0 1 0"
    if "blocks" in need:
        mixed = dark = False
        for b0 in range(0, P, BLOCK):
            blk = vis[:, b0:b0 + BLOCK]
            waves = np.stack([blk[:, w0:w0 + 64].any(axis=1) for w0 in range(0, blk.shape[1], 64)], axis=1)    # [K, waves]
            mixed |= bool((waves.any(axis=1) & ~waves.all(axis=1)).any())
            dark |= bool((~waves.any(axis=1)).any() and waves.any())
        assert mixed, "no block has a wave without a visible lane next to a wave with one"
        assert dark, "no block is entirely invisible in a subframe"
    if "guard" in need:
        assert info["outside_x"] >= 8 and info["outside_y"] >= 8, (info["outside_x"], info["outside_y"])
    assert np.isfinite(case["S"]).all()
    zero_pairs = (case["S"] == 0).all(axis=2)
    info["zero_pairs"] = int((zero_pairs & vis).sum())
    if P >= 63:
        assert info["zero_pairs"] > 0 and len(case["alone"]) == 10
    return info


# ------------------------------------------------------------------------------------------ the measures and bars
def measures(a, b, key):
    """(column-relative, row-relative) error of a against b, as the GPU test measures them: helpers.grad_errors' column
    measure and helpers.row_errors' row measure with ROW_FLOOR; rows are Gaussians, or (subframe, Gaussian) pairs."""
    if key == "dL_dmeans2D":
        a, b = a.reshape(-1, 3)[:, :2], b.reshape(-1, 3)[:, :2]
    a, b = np.asarray(a, np.float64).reshape(b.shape[0], -1), np.asarray(b, np.float64).reshape(b.shape[0], -1)
    if not np.any(b):
        return float(np.abs(a).max()), float(np.abs(a).max())
    return grad_errors(a, b)["col"], float(row_errors(a, b, ROW_FLOOR)[0].max())


COL_FLOOR, ROW_FLOOR_BAR, MATRIX_BAR = 2.0 ** -20, 2.0 ** -18, 2.0 ** -19
# The last column of dL_dprojmatrix (entries 3, 7, 11, 15: -0.5 lastcol) is held to PROJ_LAST_MULT x the 2^-19 A_proj of the
# other entries.  The term responsible: lastcol = (mhx W g2x + mhy H g2y) m_w^2, where mhx and mhy are fp32 dot products
# of a general projection matrix with the mean (geometry_bwd.hip, backward.cu:423-450, fp32 in the reference as well).
# Their rounding error scales with their addends, |ph| . |F[:, c]|, which under a rigid move of the world are 5 ... 500 times
# the dot product itself for a mean near the optical axis: a per-Gaussian term of this column is NOT accurate to a few
# roundings of its own size, which is what the 2^-19 rests on.  Measured against 2^-19 A_proj on the device, the worst last
# column is 2.87 (the one-Gaussian case, where nothing averages) and <= 0.13 in every other case; the
# multiple is the next power of two above the worst.  proj_last_unraised() reports the figure under the unraised bar.
PROJ_LAST_MULT = 4.0


def proj_last_unraised(a, r64):
    """The worst error of the last column of dL_dprojmatrix over the UNRAISED 2^-19 A_proj (reported, not asserted)."""
    A = r64["A_proj"][..., 3]
    err = np.abs(np.asarray(a, np.float64).reshape(r64["dL_dprojmatrix"].shape) - r64["dL_dprojmatrix"])[..., 3]
    return float((err[A > 0] / (MATRIX_BAR * A[A > 0])).max()) if (A > 0).any() else 0.0


def over_bar(a, r64, r32, key):
    """The worst error of the array `a` against the float64 reference r64[key], over its bar; <= 1 passes.

    Per-Gaussian outputs and dL_dmeans2D: both measures, each against max(4 x m32, floor) with m32 the same measure of the
    float32 evaluation r32 of the reference and the floors 2^-20 (column) and 2^-18 (row).  The two matrices: per entry
    against 2^-19 x the sum of the absolute values of the entry's terms (A_view / A_proj; the last column of
    dL_dprojmatrix against PROJ_LAST_MULT times that, capped at GRAD_TOL of the matrix's largest entry).  dL_drotations of an isotropic
    cloud (exactly zero): per Gaussian against max(4 x m32, 2^-19) x A_rot, m32 measured against A_rot likewise."""
    a, b = np.asarray(a, np.float64).reshape(r64[key].shape), r64[key]
    if key in ("dL_dviewmatrix", "dL_dprojmatrix"):
        A = r64["A_view" if key == "dL_dviewmatrix" else "A_proj"]
        if (np.abs(a - b)[A == 0] != 0).any():
            return float("inf")
        bar = MATRIX_BAR * A
        if key == "dL_dprojmatrix":      # the last column's raised bar, never above the end-to-end one
            cap = GRAD_TOL * np.abs(b).max(axis=(1, 2))[:, None]
            bar[..., 3] = np.minimum(PROJ_LAST_MULT * bar[..., 3], np.maximum(cap, bar[..., 3]))
        return float((np.abs(a - b)[A > 0] / bar[A > 0]).max()) if (A > 0).any() else 0.0
    if key == "dL_drotations" and "A_rot" in r64:
        A = np.maximum(r64["A_rot"], 1e-300)
        m32 = float((np.abs(r32[key] - b) / A).max())
        return float((np.abs(a - b) / A).max()) / max(4.0 * m32, MATRIX_BAR)
    (col, row), (c32, w32) = measures(a, b, key), measures(r32[key], b, key)
    return max(col / max(4.0 * c32, COL_FLOOR), row / max(4.0 * w32, ROW_FLOOR_BAR))

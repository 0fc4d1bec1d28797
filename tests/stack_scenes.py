"""Constructed tile-list scenes shared by tests/test_stack_scenes_host.py and tests/test_gpu_stack_scenes.py (no test lives
here): clouds laid out so that the structural edges of the compositing kernels (csrc/composite.hip) are reached by design
instead of by the luck of a random cloud -- tile lists of exactly 63 / 64 / 65 / 127 / ... entries (the kernels walk a list
in batches of 64), pixels whose last contributor is the last entry of a batch or the first of the next, quadrants of a tile
that finish long before their neighbours (the alive[q] / maxq[q] masks), early termination taken and never taken, an empty
tile, ragged tiles with dead quadrants, K * T below and not a multiple of the waves of a block, and anisotropic splats that
graze 8 x 8 quadrant boxes at the alpha threshold (the quadrant cull and the tile cull).

preconditions(name, states) asserts, on the ORACLE's states alone, that a scene really has the properties it was built
for; both test files call it, so a change of the generator or of a seed cannot quietly turn a constructed scene back into
an ordinary one."""
import numpy as np

from helpers import oracle, synthetic

TILE = 16


def _pixel_to_camera(sc, px, py, z):
    """Camera-space position (identity pose) whose projection is the pixel (px, py): pix = ((ndc + 1) * W - 1) / 2."""
    ndcx, ndcy = (2.0 * px + 1.0) / sc["W"] - 1.0, (2.0 * py + 1.0) / sc["H"] - 1.0
    return np.stack([ndcx * sc["tanfovx"] * z, ndcy * sc["tanfovy"] * z, z], axis=1)


def stack_scene(W, H, stacks, K, seed, sigma_px=1.2):
    """Camera, trajectory, SH and background of synthetic.make_scene; the cloud is replaced by *stacks*.  A stack is
    (tile_x, tile_y, cx, cy, n, opacity[, z0 = 4.0]): n Gaussians at tile * 16 + (cx, cy) + U(-0.3, 0.3) pixels (centres
    are x.5 +- 0.3 or x.0 +- 0.3 on purpose: a mean within 0.02 px of a pixel centre has |power| < 1e-4 there and puts the
    pixel into the oracle's margin mask), at distinct depths z0 + permutation(n) * 0.01 + U(0, 0.004) so that the order is
    total, isotropic up to 10 % per axis with sigma_px pixels: every radius is 4 or 5 pixels, so a stack centred in
    [7, 9] stays inside its tile and one centred at 4.5 next to the clamped image border stays inside one quadrant."""
    P = sum(s[4] for s in stacks)
    sc = synthetic.make_scene(P, W, H, K=K, seed=seed, sigma_px=sigma_px)
    rng = np.random.default_rng(seed)
    focal = W / (2.0 * sc["tanfovx"])
    i = 0
    for s in stacks:
        tx, ty, cx, cy, n, op = s[:6]
        z0 = s[6] if len(s) > 6 else 4.0
        px = tx * TILE + cx + rng.uniform(-0.3, 0.3, n)
        py = ty * TILE + cy + rng.uniform(-0.3, 0.3, n)
        z = z0 + rng.permutation(n) * 0.01 + rng.uniform(0.0, 0.004, n)
        sc["means3D"][i:i + n] = _pixel_to_camera(sc, px, py, z)
        sc["scales"][i:i + n] = (z * sigma_px / focal)[:, None] * rng.uniform(0.9, 1.1, (n, 3))
        sc["opacities"][i:i + n, 0] = op
        i += n
    return sc


def grazer_scene(W, H, P, K, seed, opacity=(0.05, 0.4)):
    """Anisotropic splats rotated about the viewing axis (quaternion (cos t/2, 0, 0, sin t/2), t uniform), 2 ... 6 by
    0.4 ... 1 pixels wide and flat along the view, spread over the image plus 2 px; opacities low enough that nothing
    terminates, so every grazing (pixel, Gaussian) pair is reached."""
    sc = synthetic.make_scene(P, W, H, K=K, seed=seed, sigma_px=2.0)
    rng = np.random.default_rng(seed)
    focal = W / (2.0 * sc["tanfovx"])
    z = rng.uniform(3.0, 6.0, P)
    px, py = rng.uniform(-2, W + 2, P), rng.uniform(-2, H + 2, P)
    sc["means3D"][:] = _pixel_to_camera(sc, px, py, z)
    smaj, smin = rng.uniform(2.0, 6.0, P), rng.uniform(0.4, 1.0, P)
    sc["scales"][:] = np.stack([smaj * z / focal, smin * z / focal, np.full(P, 1e-3)], axis=1)
    th = rng.uniform(0.0, np.pi, P)
    q = np.zeros((P, 4), np.float32)
    q[:, 0], q[:, 3] = np.cos(th / 2), np.sin(th / 2)
    sc["rotations"][:] = q
    sc["opacities"][:, 0] = rng.uniform(opacity[0], opacity[1], P)
    return sc


# 57 x 41: 4 x 3 tiles, the last column 9 px wide and the last row 9 px high (quadrants 1 - 3 of those tiles are partly or
# wholly dead); K * T = 36 tile blocks = 9 thread blocks of 4 waves under the 16-block grid of the XCD map (empty waves)
BATCHES_STACKS = [
    (0, 0, 4.5, 4.5, 64, 0.04), (1, 0, 8.5, 8.5, 65, 0.04), (2, 0, 8.5, 8.5, 63, 0.04), (3, 0, 7.0, 8.5, 128, 0.02),
    (0, 1, 4.5, 8.5, 129, 0.02), (1, 1, 8.5, 8.5, 200, 0.3), (2, 1, 8.5, 8.5, 1, 0.9), (3, 1, 7.0, 8.5, 127, 0.5),
    (0, 2, 8.5, 7.0, 192, 0.02), (1, 2, 8.5, 7.0, 130, 0.25), (3, 2, 7.0, 7.0, 70, 0.6),
]
BATCHES_LISTS = [64, 65, 63, 128, 129, 200, 1, 127, 192, 130, 0, 70]      # per tile, row-major; tile (2, 2) is empty
# one tile: 65 entries at opacity 0.3 in front of 64 at 0.02.  K * T = 1: a single live wave in a grid of 8 blocks;
# K * T = 5: not a multiple of the 4 waves of a block
ONE_TILE_STACKS = [(0, 0, 8.5, 8.5, 65, 0.3, 4.0), (0, 0, 8.5, 8.5, 64, 0.02, 5.0)]

CATALOGUE = {
    # name: (builder, K, whether every Gaussian is held to the flat gradient bars)
    "batches": (lambda: stack_scene(57, 41, BATCHES_STACKS, K=3, seed=7), 3, True),
    "one_tile_k1": (lambda: stack_scene(16, 16, ONE_TILE_STACKS, K=1, seed=3), 1, True),
    "one_tile_k5": (lambda: stack_scene(16, 16, ONE_TILE_STACKS, K=5, seed=3), 5, True),
    "grazers": (lambda: grazer_scene(57, 41, 250, K=2, seed=1), 2, False),
}
NAMES = list(CATALOGUE)
MARGIN_FRAC = 0.01     # the oracle's own doubt (oracle.unstable) covers at most this fraction of a subframe


def make(name):
    """(scene, K) of a catalogue scene."""
    build, K, _ = CATALOGUE[name]
    return build(), K


def flat_bars(name):
    return CATALOGUE[name][2]


def list_lengths(st):
    r = st["ranges"].astype(np.int64)
    return (r[:, 1] - r[:, 0]).tolist()


def _tiles(st):
    W, H = st["W"], st["H"]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    for ty in range(gy):
        for tx in range(gx):
            yield ty * gx + tx, slice(ty * TILE, min(ty * TILE + TILE, H)), slice(tx * TILE, min(tx * TILE + TILE, W))


def quadrant_maxima(st):
    """Per tile, the largest n_contrib of each of its four 8 x 8 quadrants (None for a quadrant outside the image)."""
    nc = st["n_contrib"].reshape(st["H"], st["W"]).astype(np.int64)
    out = []
    for _, ys, xs in _tiles(st):
        t = nc[ys, xs]
        quads = [t[qy * 8:qy * 8 + 8, qx * 8:qx * 8 + 8] for qy in (0, 1) for qx in (0, 1)]
        out.append([int(q.max()) if q.size else None for q in quads])
    return out


def grazing_boxes(st):
    """(barely hit, barely missed): over every visible Gaussian and every 8 x 8 box of the tile grid (the quadrants the
    kernels cull by), m = the maximum over the box's in-image pixel centres of 255 * opacity * exp(power), in float64 from
    the oracle's conic_opacity and means2D.  Barely hit: m in [1.0, 1.5) AND the oracle really blends the pair at that
    pixel (the Gaussian is in the tile's list at or before the pixel's last contributor, and its fp32 alpha passes the
    reference's tests).  Barely missed: m in (0.6, 1.0)."""
    W, H = st["W"], st["H"]
    gx = (W + TILE - 1) // TILE
    co, m2 = st["conic_opacity"].astype(np.float64), st["means2D"].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    nc = st["n_contrib"].reshape(H, W)
    ranges, pl = st["ranges"].astype(np.int64), st["point_list"]
    hit = miss = 0
    for g in np.nonzero(st["radii"] > 0)[0]:
        dx, dy = m2[g, 0] - xs, m2[g, 1] - ys
        a = 255.0 * co[g, 3] * np.exp(-0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy)
        for by in range(0, H, 8):
            for bx in range(0, W, 8):
                box = a[by:by + 8, bx:bx + 8]
                m = box.max()
                if 0.6 < m < 1.0:
                    miss += 1
                elif 1.0 <= m < 1.5:
                    iy, ix = np.unravel_index(int(box.argmax()), box.shape)
                    y, x = by + iy, bx + ix
                    r0, r1 = ranges[(y // TILE) * gx + x // TILE]
                    pos = np.nonzero(pl[r0:r1] == g)[0]
                    if pos.size == 0 or pos[0] + 1 > nc[y, x]:
                        continue
                    c = st["conic_opacity"][g]
                    fx, fy = st["means2D"][g, 0] - np.float32(x), st["means2D"][g, 1] - np.float32(y)
                    power = np.float32(-0.5) * (c[0] * fx * fx + c[2] * fy * fy) - c[1] * fx * fy
                    alpha = min(np.float32(0.99), c[3] * np.exp(power))
                    hit += bool(power <= 0 and alpha >= np.float32(1.0 / 255.0))
    return hit, miss


def margin_counts(states):
    return [int(oracle.unstable(st).sum()) for st in states]


def preconditions(name, states):
    """Asserts on the oracle's states (one per subframe) that the scene `name` is what it was constructed to be.  Returns
    the measured figures."""
    info = {"margin": margin_counts(states), "lists": [list_lengths(st) for st in states]}
    for st, m in zip(states, info["margin"]):
        assert m <= MARGIN_FRAC * st["W"] * st["H"], f"{name}: {m} margin pixels of {st['W'] * st['H']}"
    if name == "batches":
        for k, st in enumerate(states):
            assert info["lists"][k] == BATCHES_LISTS, (k, info["lists"][k])
            assert {63, 64, 65, 127, 128, 129} <= set(np.unique(st["n_contrib"]).tolist()), f"k={k}: last contributors"
            qm = quadrant_maxima(st)
            early = [t for t, q in enumerate(qm) if max(v for v in q if v is not None) - min(v for v in q if v is not None) >= 64]
            assert len(early) >= 2, f"k={k}: tiles with a quadrant a whole batch behind another: {early} of {qm}"
            fT = st["final_T"].reshape(st["H"], st["W"])
            taken = [t for t, ys, xs in _tiles(st) if ((fT[ys, xs] >= 1e-4) & (fT[ys, xs] <= 1.1e-4)).any()]
            never = [t for t, ys, xs in _tiles(st) if (fT[ys, xs] > 0.02).all()]
            assert len(taken) >= 3 and len(never) >= 3, f"k={k}: termination taken in {taken}, never in {never}"
            info.setdefault("early_quadrant_tiles", []).append(early)
            info.setdefault("terminated_tiles", []).append(taken)
            info.setdefault("unterminated_tiles", []).append(never)
    elif name.startswith("one_tile"):
        for k, st in enumerate(states):
            assert info["lists"][k] == [129], (k, info["lists"][k])
            # some pixel stops inside the first batch, some pixel's last contributor is the first entry of the third
            nc = st["n_contrib"]
            assert nc.min() < 64 and nc.max() == 129, (int(nc.min()), int(nc.max()))
    elif name == "grazers":
        info["boxes"] = [grazing_boxes(st) for st in states]
        info["final_T_min"] = [float(st["final_T"].min()) for st in states]
        for k, (hit, miss) in enumerate(info["boxes"]):
            assert hit >= 40 and miss >= 40, f"k={k}: {hit} barely hit and {miss} barely missed 8 x 8 boxes"
        assert min(info["final_T_min"]) > 1e-3, "a pixel of the grazer scene terminates"
    return info


# ------------------------------------------------------------------- gradients: upstream values, the float64 reference
GRAD_KEYS = ["dL_dmeans3D", "dL_dopacities", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dmeans2D", "dL_dviewmatrix",
             "dL_dprojmatrix"]
CHECK_KEYS = GRAD_KEYS + ["dL_dconic", "dL_dcov3D"]
F64_KEYS = ["dL_dmeans3D", "dL_dopacities", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dviewmatrix", "dL_dproj_col0",
            "dL_dproj_col1"]


def upstream(sc, K, depth=True, seed=5):
    """The upstream gradients of the parity tests (tests/test_gpu_parity.py::_grads: same recipe, same seed)."""
    rng = np.random.default_rng(seed)
    gC = rng.normal(size=(K, 3, sc["H"], sc["W"])).astype(np.float32)
    gD = (rng.normal(size=(K, 1, sc["H"], sc["W"])) * 0.05).astype(np.float32) if depth else None
    return gC, gD


def checker_kw(name):
    """How helpers.assert_grads_close is called on a scene: on the stack scenes EVERY Gaussian is held to the flat 1e-4 / 1e-3
    bars (no ill-conditioned set, all rows well-conditioned: the host test proves the reference's own builds meet this)."""
    return dict(ill_frac=0, ill_min=0, well_frac=1.0) if flat_bars(name) else {}


def float64_reference(sc, k, gC, gD, **kw):
    """Subframe k through the dense torch rasteriser (oracle/torch_naive.py) in float64 and autograd: the image, the radii
    and the gradients F64_KEYS of <colour, gC> + <depth, gD>.  The two analytic columns of dL_dprojmatrix are given in the
    reference's units (backward.cu:430-450: times 0.5 W / 0.5 H).  kw: further keywords of torch_naive.rasterize."""
    import torch
    from oracle import torch_naive
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    inp = {n: T(sc[n]).requires_grad_(True) for n in ["means3D", "opacities", "sh", "scales", "rotations"]}
    V, F = T(sc["viewmatrix"][k]).requires_grad_(True), T(sc["projmatrix"][k]).requires_grad_(True)
    c, d, r = torch_naive.rasterize(inp["means3D"], inp["opacities"], V, F, T(sc["campos"][k]), T(sc["bg"]), sc["W"],
                                    sc["H"], sc["tanfovx"], sc["tanfovy"], sh=inp["sh"], scales=inp["scales"],
                                    rotations=inp["rotations"], sh_degree=sc["sh_degree"], **kw)
    loss = (c * T(gC)).sum()
    if gD is not None:
        loss = loss + (d * T(gD)).sum()
    loss.backward()
    g = lambda t: t.grad.numpy()
    Fg = g(F)
    return dict(color=c.detach().numpy(), radii=r.numpy(), dL_dmeans3D=g(inp["means3D"]), dL_dopacities=g(inp["opacities"]),
                dL_dsh=g(inp["sh"]), dL_dscales=g(inp["scales"]), dL_drotations=g(inp["rotations"]), dL_dviewmatrix=g(V),
                dL_dproj_col0=Fg[:, 0] * 0.5 * sc["W"], dL_dproj_col1=Fg[:, 1] * 0.5 * sc["H"])


def errors_to_float64(got, ref):
    """Per key of F64_KEYS: max |got - ref| / max |ref|.  got: the per-subframe gradients by the names of GRAD_KEYS
    (dL_dprojmatrix [4,4] whole: its columns 0 / 1 are compared, 2 must be zero and 3 constant as the reference leaves
    them)."""
    from helpers import relerr
    Pg = np.asarray(got["dL_dprojmatrix"]).reshape(4, 4)
    assert np.all(Pg[:, 2] == 0) and np.all(Pg[:, 3] == Pg[0, 3])
    got = dict(got, dL_dproj_col0=Pg[:, 0], dL_dproj_col1=Pg[:, 1])
    return {key: relerr(np.asarray(got[key]).reshape(ref[key].shape), ref[key]) for key in F64_KEYS}

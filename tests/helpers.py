"""Shared helpers of the parity tests: run the HIP path (through the C ABI, via the Python operator layer) and
the CPU oracle on the same seeded synthetic scene, and expose every intermediate of both for comparison."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deblurgs_amd import synthetic  # noqa: E402
from oracle import oracle  # noqa: E402


def oracle_forward(scene, k, sh_degree=None, use_sigmoid=False, colors_precomp=None, cov3D_precomp=None,
                   scale_modifier=1.0, render=True):
    kw = dict(sh_degree=scene["sh_degree"] if sh_degree is None else sh_degree, use_sigmoid=use_sigmoid,
              scale_modifier=scale_modifier, z_far=scene["z_far"], render=render)
    if colors_precomp is None:
        kw["sh"] = scene["sh"]
    else:
        kw["colors_precomp"] = colors_precomp
    if cov3D_precomp is None:
        kw["scales"] = scene["scales"]
        kw["rotations"] = scene["rotations"]
    else:
        kw["cov3D_precomp"] = cov3D_precomp
    return oracle.forward(scene["means3D"], scene["opacities"], scene["viewmatrix"][k], scene["projmatrix"][k],
                          scene["campos"][k], scene["bg"], scene["W"], scene["H"], scene["tanfovx"], scene["tanfovy"],
                          **kw)


def unstable_pixels(st, alpha_tol=5e-7, power_tol=1e-4, T_tol=1e-8):
    """Pixels where some (pixel, Gaussian) pair of the ORACLE's traversal sits within a small margin of one of the
    reference's three thresholds (power > 0, alpha < 1/255, T(1-alpha) < 1e-4).  exp() differs by an ulp or
    two between glibc, CUDA libdevice and the gfx950 hardware exp, so such a pair may legitimately fall on
    either side; everywhere else the images must agree to 1e-4."""
    W, H = st["W"], st["H"]
    gx = (W + 15) // 16
    means2D, co = st["means2D"], st["conic_opacity"]
    flag = np.zeros(W * H, bool)
    ranges, pl = st["ranges"], st["point_list"]
    for tile in range(ranges.shape[0]):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        if r1 <= r0:
            continue
        ty, tx = divmod(tile, gx)
        ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)),
                             indexing="ij")
        px, py = xs.reshape(-1).astype(np.float32), ys.reshape(-1).astype(np.float32)
        g = pl[r0:r1]
        dx = means2D[g, 0][None] - px[:, None]
        dy = means2D[g, 1][None] - py[:, None]
        c = co[g]
        power = (-0.5 * (c[:, 0][None] * dx * dx + c[:, 2][None] * dy * dy) - c[:, 1][None] * dx * dy).astype(
            np.float32)
        alpha = np.minimum(0.99, c[:, 3][None] * np.exp(power)).astype(np.float32)
        valid = (power <= 0) & (alpha >= 1.0 / 255.0)
        a = np.where(valid, alpha, 0.0)
        T_incl = np.cumprod(1.0 - a, axis=1)
        stop = valid & (T_incl < 1e-4)
        reached = (np.cumsum(stop, axis=1) - stop) == 0       # pairs the pixel actually evaluates
        # fp32 evaluation uncertainty of `power` (a few ulps of its largest term) and what it does to alpha and T
        perr = (5e-7 * (0.5 * np.abs(c[:, 0][None] * dx * dx) + 0.5 * np.abs(c[:, 2][None] * dy * dy)
                        + np.abs(c[:, 1][None] * dx * dy))).astype(np.float32)
        near = (np.abs(alpha - 1.0 / 255.0) < alpha_tol + alpha * perr) | (np.abs(power) < power_tol + perr)
        T_rel = np.cumsum(np.where(valid & (alpha < 0.99), a * perr / np.maximum(1.0 - a, 1e-6), 0.0), axis=1)
        near |= valid & (np.abs(T_incl - 1e-4) < T_tol + T_incl * (T_rel + 1e-6))
        near &= reached
        flag[(ys.reshape(-1) * W + xs.reshape(-1))[near.any(axis=1)]] = True
    return flag.reshape(H, W)


def oracle_pixel_walk(st, y, x):
    """The oracle's traversal of pixel (x, y), restated in fp32 numpy (dgs_oracle_render): one record
    (pos, Gaussian, power, alpha, T before the pair, contributes) per list entry the pixel evaluates; pos is 1-based."""
    gx = (st["W"] + 15) // 16
    r0, r1 = (int(v) for v in st["ranges"][(y // 16) * gx + x // 16])
    out, T = [], np.float32(1.0)
    for pos, g in enumerate(st["point_list"][r0:r1], start=1):
        c = st["conic_opacity"][g]
        dx, dy = st["means2D"][g, 0] - np.float32(x), st["means2D"][g, 1] - np.float32(y)
        power = np.float32(-0.5) * (c[0] * dx * dx + c[2] * dy * dy) - c[1] * dx * dy
        alpha = np.float32(min(np.float32(0.99), c[3] * np.exp(power)))
        ok = bool(power <= 0 and alpha >= np.float32(1.0 / 255.0))
        test_T = T * (np.float32(1.0) - alpha)
        if ok and test_T < np.float32(1e-4):
            out.append((pos, int(g), float(power), float(alpha), float(T), False))
            break
        out.append((pos, int(g), float(power), float(alpha), float(T), ok))
        if ok:
            T = test_T
    return out


_CHK_MUL_INV = pow(2654435761, -1, 1 << 32)


def describe_exempt(st, mask, hip_checksum, hip_n_contrib, limit=8):
    """For (at most `limit` of) the pixels of `mask`: the pixel, the two last contributors, and the ORACLE's numbers of the
    deciding pair -- the list position that a single flipped decision leaves in the checksum difference (pos * 2654435761
    mod 2^32) when there is one, else the evaluated pair that sits closest to the alpha threshold."""
    margin = oracle.unstable(st)
    lines = []
    hc, hn = np.asarray(hip_checksum).reshape(-1).view(np.uint32), np.asarray(hip_n_contrib).reshape(-1).view(np.uint32)
    for y, x in np.argwhere(mask)[:limit]:
        y, x = int(y), int(x)
        pix = y * st["W"] + x
        walk = oracle_pixel_walk(st, y, x)
        diff = (int(hc[pix]) - int(st["contrib_checksum"][pix])) % (1 << 32)
        extra, dropped = (diff * _CHK_MUL_INV) % (1 << 32), ((-diff) * _CHK_MUL_INV) % (1 << 32)
        by_pos = {w[0]: w for w in walk}
        if diff and extra in by_pos:
            why, w = "the HIP forward alone blends", by_pos[extra]
        elif diff and dropped in by_pos:
            why, w = "the HIP forward alone skips", by_pos[dropped]
        elif walk:
            why = "several decisions differ; closest to the alpha threshold:"
            w = min(walk, key=lambda r: abs(r[3] - 1.0 / 255.0))
        else:
            why, w = "empty list", (0, -1, 0.0, 0.0, 1.0, False)
        lines.append(f"pixel (x={x}, y={y}){'' if margin[y, x] else ' OUTSIDE the margin mask'}: last contributor HIP "
                     f"{int(hn[pix])} / oracle {int(st['n_contrib'][pix])}; {why} list position {w[0]} (Gaussian {w[1]}): "
                     f"alpha {w[3]:.9g} (1/255 = {1 / 255:.9g}), power {w[2]:.6g}, T {w[4]:.6g}")
    return "\n   ".join(lines)


def exempt_cap(st):
    """The most pixels of one subframe that may be exempt when the caller names no figure of its own."""
    return max(2e-4 * st["H"] * st["W"], 4)


def capped_exempt_masks(states, hip_checksum, hip_n_contrib, cap=None, what="exempt pixels"):
    """[len(states)] masks [H,W] of the pixels where the HIP forward (hip_*: [K', H*W] of a tile_cull = 0 forward) and the
    oracle's took a different per-pair decision -- and the ceiling on them, asserted HERE so that every caller inherits
    it.  A kernel regression in a per-pair decision (a cull that drops a contributing pair, a wrong quadrant mask, a
    termination off by one entry) IS such a difference: without a ceiling it would exempt itself.  Per subframe

        exempt <= max(2e-4 H W, 4)    (or the caller's `cap`: the scene's margin count, from the oracle alone)
        exempt <= margin + 2          (margin = oracle.unstable(state): the pixels where the ORACLE's own traversal sits
                                       within a rounding error of a threshold; computed only where exempt > 2)

    DGS_EXEMPT_LOG=<file>: one line per call with the exempt and margin counts (the margins are then always computed)."""
    masks, counts, margins = [], [], []
    log = os.environ.get("DGS_EXEMPT_LOG")
    for i, st in enumerate(states):
        hc = np.asarray(hip_checksum[i]).reshape(-1).view(np.uint32)
        hn = np.asarray(hip_n_contrib[i]).reshape(-1).view(np.uint32)
        d = ((hc != st["contrib_checksum"]) | (hn != st["n_contrib"])).reshape(st["H"], st["W"])
        n = int(d.sum())
        masks.append(d)
        counts.append(n)
        limit = exempt_cap(st) if cap is None else cap
        margin = int(oracle.unstable(st).sum()) if (n > 2 or log) else None
        margins.append(margin)
        if n > limit or (margin is not None and n > margin + 2):
            raise AssertionError(
                f"{what}, subframe {i}: {n} pixels of {st['H'] * st['W']} differ from the oracle in a per-pair decision "
                f"(allowed {limit:g}, and the oracle's margin mask + 2 = {margin if margin is not None else '?'} + 2):\n   "
                + describe_exempt(st, d, hc, hn))
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', what)} | {states[0]['W']}x{states[0]['H']} | exempt {counts} "
                    f"| margin {margins}\n")
    return masks


def exempt_pixels(scene, K, states, cap=None, **kw):
    """[K] masks [H,W]: the pixels where the HIP forward and the oracle's took a DIFFERENT per-pair decision -- their
    contributor checksums (DgsForwardOut.debug_contrib_checksum: a tile_cull = 0 forward through the C ABI; dgs_oracle_render)
    or their last contributors differ.  What the parity tests exempt from the 1e-4 bars since round 6 (the margin rule of
    unstable_pixels / oracle.unstable exempted every pixel NEAR a threshold: hundreds of times more).  Their number is
    bounded here (capped_exempt_masks).  kw: what hip_forward_state takes (sh_degree, use_sigmoid, colors_precomp,
    cov3D_precomp, scale_modifier)."""
    st = hip_forward_state(scene, K, checksum=True, **kw)
    return capped_exempt_masks(states[:K], st["contrib_checksum"], st["n_contrib"], cap=cap)


# --------------------------------------------------------------------------------------------- HIP side
def _t(a, device="cuda"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def hip_settings(scene, K, sh_degree=None, use_sigmoid=False, scale_modifier=1.0, debug=False, campos=None):
    from deblurgs_amd.diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = scene["campos"][:K] if campos is None else campos
    return GaussianRasterizationSettings(
        image_height=scene["H"], image_width=scene["W"], tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"],
        bg=_t(scene["bg"]), scale_modifier=scale_modifier, z_near=scene["z_near"], z_far=scene["z_far"],
        use_sigmoid=use_sigmoid, sh_degree=scene["sh_degree"] if sh_degree is None else sh_degree,
        campos=_t(cam if K > 1 else cam[0]), prefiltered=False, debug=debug)


import contextlib


@contextlib.contextmanager
def tile_cull(flag):
    """Selects the duplicate rule of the HIP path for the calls inside: False = the reference's rectangle lists."""
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    old = dgr.TILE_CULL
    dgr.TILE_CULL = bool(flag)
    try:
        yield
    finally:
        dgr.TILE_CULL = old


@contextlib.contextmanager
def wide_records(flag):
    """DgsProblem.wide_records for the calls inside: True keeps key + value arrays for the culled duplicates."""
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    old = dgr.WIDE_RECORDS
    dgr.WIDE_RECORDS = bool(flag)
    try:
        yield
    finally:
        dgr.WIDE_RECORDS = old


def hip_forward_state(scene, K, sh_degree=None, use_sigmoid=False, colors_precomp=None, cov3D_precomp=None,
                      scale_modifier=1.0, cull=False, capacity=None, checksum=False):
    """Runs the fused forward through the C ABI and returns outputs + every saved sub-array as numpy.  cull=False
    (default) keeps the reference's duplicate lists so that keys / point_list / ranges compare bit for bit; with
    cull=True the low key word is the duplicate's emission index instead of the depth bits."""
    with tile_cull(cull):
        return _hip_forward_state(scene, K, sh_degree, use_sigmoid, colors_precomp, cov3D_precomp, scale_modifier,
                                  capacity, checksum)


def _hip_forward_state(scene, K, sh_degree, use_sigmoid, colors_precomp, cov3D_precomp, scale_modifier, capacity=None,
                       checksum=False):
    import torch
    from deblurgs_amd import _lib
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    rs = hip_settings(scene, K, sh_degree, use_sigmoid, scale_modifier)
    rs = rs._replace(campos=_t(scene["campos"][:K]))
    sh = None if colors_precomp is not None else _t(scene["sh"])
    col = None if colors_precomp is None else _t(colors_precomp)
    sc = None if cov3D_precomp is not None else _t(scene["scales"])
    rot = None if cov3D_precomp is not None else _t(scene["rotations"])
    cov = None if cov3D_precomp is None else _t(cov3D_precomp)
    R, color, depth, radii, geom, binning, image = dgr._forward_impl(
        K, _t(scene["means3D"]), sh, col, _t(scene["opacities"]).reshape(-1), sc, rot, cov,
        _t(scene["viewmatrix"][:K]), _t(scene["projmatrix"][:K]), _t(scene["campos"][:K]), rs, capacity=capacity,
        debug_checksum=checksum)
    torch.cuda.synchronize()
    P, W, H = scene["P"], scene["W"], scene["H"]
    N = W * H
    T = ((W + 15) // 16) * ((H + 15) // 16)
    L = _lib.layout(P, W, H, K, R if capacity is None else capacity)   # the blob is laid out for the capacity
    R_obj = R
    R = int(R)

    def view(blob, off, nbytes, dtype, shape):
        return blob[off:off + nbytes].cpu().numpy().view(dtype).reshape(shape)

    rows = view(geom, L.geom_rows, K * P * 48, np.float32, (K, P, 12))
    st = dict(
        R=R, K=K, color=color.cpu().numpy(), depth=depth.cpu().numpy(), radii=radii.cpu().numpy(),
        rows=rows, rows_u32=rows.view(np.uint32),
        cov3D=view(geom, L.cov3D, P * 24, np.float32, (P, 6)),
        pre_sigmoid=view(geom, L.pre_sigmoid, K * P * 12, np.float32, (K, P, 3)),
        tiles_touched=view(geom, L.tiles_touched, K * P * 4, np.uint32, (K, P)),
        point_offsets=view(geom, L.point_offsets, K * P * 4, np.uint32, (K, P)),
        order=view(geom, L.gsort_vals, K * P * 4, np.uint32, (K * P,)),
        # tile_cull: 1 / 0 per position of the depth order = a visible pair sits there (the invisible pairs are dropped by
        # the first depth-order pass: the tail of every segment has flag 0 and an UNDEFINED index)
        order_visible=view(geom, L.tt_sorted, K * P * 4, np.uint32, (K * P,)) != 0,
        tt_tight=view(geom, L.tt_tight, K * P * 4, np.uint32, (K * P,)),
        offs_tight=view(geom, L.offs_tight, K * P * 4, np.uint32, (K * P,)),
        final_T=view(image, L.final_T, K * N * 4, np.float32, (K, N)),
        n_contrib=view(image, L.n_contrib, K * N * 4, np.uint32, (K, N)),
        ranges=view(image, L.ranges, K * T * 8, np.uint32, (K, T, 2)),
        keys=view(binning, L.keys_sorted, R * 8, np.uint64, (R,)),
        point_list=view(binning, L.point_list, R * 4, np.uint32, (R,)),
        sort_bits=L.sort_bits, T=T,
    )
    if not use_sigmoid:
        # relu colour activation (round 6): the clamp mask the backward multiplies by rides in the row's spare word (bits
        # 0..2 of word 10) instead of a [K,P,3] float array; the tests read it in the oracle's form
        bits = st["rows_u32"][:, :, 10]
        st["pre_sigmoid"] = np.stack([(bits >> c) & 1 for c in range(3)], axis=-1).astype(np.float32)
    if checksum:
        st["contrib_checksum"] = R_obj.contrib_checksum.cpu().numpy().view(np.uint32)
    st["compact_keys"] = False
    if R_obj.tile_cull and L.pack_tile_shift > 0:
        # compact keys (DgsLayout.pack_*): tile | Gaussian | emission index in one word and no value array; the tests
        # read the canonical form, key = tile << 32 | emission index and the Gaussian in point_list
        raw = st["keys"]
        gs, ts = np.uint64(L.pack_g_shift), np.uint64(L.pack_tile_shift)
        st["point_list"] = ((raw >> gs) & ((np.uint64(1) << (ts - gs)) - np.uint64(1))).astype(np.uint32)
        st["keys"] = ((raw >> ts) << np.uint64(32)) | (raw & ((np.uint64(1) << gs) - np.uint64(1)))
        st["compact_keys"] = True
    if capacity is not None:
        st.update(overflow=R_obj.overflow, counted=R_obj.counted)
    return st


def hip_forward_backward(scene, K, dL_dcolor, dL_ddepth=None, sh_degree=None, use_sigmoid=False, fused=True,
                         colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0):
    """Forward + backward through the public operator (autograd).  fused=False uses the K=1 reference API K
    times (and sums per-Gaussian grads like autograd does in the reference loop)."""
    import torch
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    from deblurgs_amd.diff_gaussian_rasterization import GaussianRasterizer
    dev = "cuda"
    names = ["means3D", "opacities", "sh", "scales", "rotations"]
    inp = {n: _t(scene[n]).requires_grad_(True) for n in names}
    col = None if colors_precomp is None else _t(colors_precomp).requires_grad_(True)
    cov = None if cov3D_precomp is None else _t(cov3D_precomp).requires_grad_(True)
    view = _t(scene["viewmatrix"][:K]).requires_grad_(True)
    proj = _t(scene["projmatrix"][:K]).requires_grad_(True)
    gC = _t(dL_dcolor)
    gD = None if dL_ddepth is None else _t(dL_ddepth)
    P = scene["P"]
    kw = dict(shs=inp["sh"] if col is None else None, colors_precomp=col,
              scales=inp["scales"] if cov is None else None, rotations=inp["rotations"] if cov is None else None,
              cov3D_precomp=cov)
    if fused:
        rs = hip_settings(scene, K, sh_degree, use_sigmoid, scale_modifier)._replace(campos=_t(scene["campos"][:K]))
        m2 = torch.zeros((K, P, 3), device=dev, requires_grad=True)
        color, depth, radii = GaussianRasterizer(rs).forward_subframes(
            inp["means3D"], m2, inp["opacities"], viewmatrices=view, projmatrices=proj, **kw)
        loss = (color * gC).sum()
        if gD is not None:
            loss = loss + (depth * gD).sum()
        dgr.BACKWARD_DEBUG = dbg = {}
        try:
            loss.backward()
        finally:
            dgr.BACKWARD_DEBUG = None
        m2g = m2.grad
    else:
        dbg = None
        colors, depths, radiis, m2s = [], [], [], []
        loss = 0
        for k in range(K):
            rs = hip_settings(scene, 1, sh_degree, use_sigmoid, scale_modifier, campos=scene["campos"][k:k + 1])
            m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
            c, d, r = GaussianRasterizer(rs)(inp["means3D"], m2, inp["opacities"], viewmatrix=view[k],
                                             projmatrix=proj[k], **kw)
            loss = loss + (c * gC[k]).sum()
            if gD is not None:
                loss = loss + (d * gD[k]).sum()
            colors.append(c)
            depths.append(d)
            radiis.append(r)
            m2s.append(m2)
        loss.backward()
        color, depth, radii = torch.stack(colors), torch.stack(depths), torch.stack(radiis)
        m2g = torch.stack([m.grad for m in m2s])
    torch.cuda.synchronize()
    out = dict(color=color.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), radii=radii.cpu().numpy(),
               dL_dmeans2D=m2g.cpu().numpy(), dL_dviewmatrix=view.grad.cpu().numpy(),
               dL_dprojmatrix=proj.grad.cpu().numpy())
    for n in names:
        out["dL_d" + n] = None if inp[n].grad is None else inp[n].grad.cpu().numpy()
    out["dL_dcolors_precomp"] = None if col is None or col.grad is None else col.grad.cpu().numpy()
    out["dL_dcov3D_precomp"] = None if cov is None or cov.grad is None else cov.grad.cpu().numpy()
    if dbg:
        out["internals"] = hip_backward_internals(dbg, out["radii"], means2D=out["dL_dmeans2D"])
        out["dL_dconic"], out["dL_dcov3D"] = out["internals"]["dL_dconic"], out["internals"]["dL_dcov3D"]
    return out


def oracle_forward_backward(scene, K, dL_dcolor, dL_ddepth=None, sh_degree=None, use_sigmoid=False,
                            colors_precomp=None, cov3D_precomp=None):
    """Reference semantics: K independent renders, per-Gaussian grads summed over k (autograd accumulation)."""
    outs = []
    for k in range(K):
        st = oracle_forward(scene, k, sh_degree, use_sigmoid, colors_precomp, cov3D_precomp)
        g = oracle.backward(st, dL_dcolor[k], None if dL_ddepth is None else dL_ddepth[k])
        outs.append((st, g))
    res = dict(
        color=np.stack([o[0]["color"] for o in outs]), depth=np.stack([o[0]["depth"] for o in outs]),
        radii=np.stack([o[0]["radii"] for o in outs]),
        dL_dmeans2D=np.stack([o[1]["dL_dmeans2D"] for o in outs]),
        dL_dviewmatrix=np.stack([o[1]["dL_dviewmatrix"] for o in outs]),
        dL_dprojmatrix=np.stack([o[1]["dL_dprojmatrix"] for o in outs]),
        dL_dmeans3D=sum(o[1]["dL_dmeans3D"] for o in outs), dL_dopacities=sum(o[1]["dL_dopacity"] for o in outs),
        dL_dsh=sum(o[1]["dL_dsh"] for o in outs), dL_dscales=sum(o[1]["dL_dscales"] for o in outs),
        dL_drotations=sum(o[1]["dL_drotations"] for o in outs),
        dL_dcolors_precomp=sum(o[1]["dL_dcolors"] for o in outs),
        dL_dcov3D_precomp=sum(o[1]["dL_dcov3D"] for o in outs),
        states=[o[0] for o in outs],
    )
    return res


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def grad_errors(a, b, rows=None, floor=0.05):
    """Sharper than relerr (which lets a component 1e4 x smaller than the tensor's largest one be 100 % wrong):

      col  max over the COLUMNS (the 3 / 27 / 1 / 3 / 4 components of a per-Gaussian gradient, each with its own
           scale) of  max_g |a - b| / max_g |b|   -- every component is held to the bar against its own magnitude;
      row  max over the ROWS (Gaussians) of  max_c |a - b| / max(max_c |b_row|, floor * column scale)  -- a relative
           error per Gaussian, with an absolute floor so that Gaussians whose gradient is below `floor` of the
           largest one are measured against that floor rather than against their own near-zero value.

    a, b: arrays whose leading `rows` dimension indexes Gaussians (default: first axis)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    n = a.shape[0] if rows is None else rows
    a, b = a.reshape(n, -1), b.reshape(n, -1)
    d = np.abs(a - b)
    colmax = np.abs(b).max(axis=0)
    nz = colmax > 0
    col = float((d[:, nz].max(axis=0) / colmax[nz]).max()) if nz.any() else float(d.max())
    # rows: each component normalised by its column scale first, so that components of different magnitude
    # (xyz vs the 27 SH coefficients) are commensurable inside one row
    scale = np.where(nz, colmax, 1.0)
    dn, bn = d / scale, np.abs(b) / scale
    row = float((dn.max(axis=1) / np.maximum(bn.max(axis=1), floor)).max())
    return {"col": col, "row": row}


# ------------------------------------------------------------------------------- conditioning-aware gradient checker
GRAD_TOL = 1e-4        # north_star bar, applied per gradient COMPONENT (column), each against its own scale
ROW_TOL = 1e-3         # per GAUSSIAN: relative to the Gaussian's own gradient magnitude, floored at ROW_FLOOR x column scale
ROW_FLOOR = 0.1


class OracleRun:
    """The checker side of a backward parity test, on the OpenMP oracle (deterministic, double accumulation):
    forward of the K subframes, the unstable-pixel masks, and the backward three times -- "double": accumulating in
    double (the value the HIP result is compared with); "f32": accumulating in emulated fp32 in the same order; "fma":
    the same source built with multiply-adds contracted into FMAs, which is what nvcc's default (--fmad=true) makes of
    the reference.  |f32 - double| and |fma - double| are the two ways in which correct fp32 builds of the reference
    algorithm differ from each other; they are large exactly where a gradient component is ill-conditioned (scale /
    rotation behind the covariance chain, the view matrix)."""

    def __init__(self, scene, K, margin_masks=True, exact=False, cap=None, **kw):
        """margin_masks=False: the caller will install the exact disagreement masks (use_exact_masks) and the oracle's
        threshold-margin masks are not computed.  exact=True: the masks are exempt_pixels() of this scene (a HIP forward
        with contributor checksums is run here: needs the GPU); their number is bounded there (cap: see
        capped_exempt_masks)."""
        self.scene, self.K, self.kw = scene, K, kw
        margin_masks = margin_masks and not exact
        oracle.use_openmp(True)
        try:
            self.states = oracle.map_subframes(lambda k: oracle_forward(scene, k, **kw), range(K))
            self.unstable = (oracle.map_subframes(oracle.unstable, self.states) if margin_masks else [None] * K)
        finally:
            oracle.use_openmp(False)
        for st in self.states:
            st.pop("keys_unsorted", None)
            st.pop("vals_unsorted", None)
        if exact:
            self.unstable = exempt_pixels(scene, K, self.states, cap=cap, **kw)

    def use_exact_masks(self, hip_checksum, hip_n_contrib, ks=None, cap=None):
        """Replaces the margin masks (every pixel whose ORACLE traversal sits within a margin of a threshold: 0.5 % of the
        pixels at the metric size) by the pixels where the HIP traversal and the oracle's really took a different per-pair
        decision: their contributor checksums (DgsForwardOut.debug_contrib_checksum / dgs_oracle_render) or their last
        contributors differ.  hip_* are [K', H*W] arrays of a tile_cull = 0 forward (positions in the reference's lists),
        for the subframes ks of this run (default: all).  Returns the exempt pixel count per subframe; it is bounded
        here (capped_exempt_masks), per subframe."""
        ks = list(range(self.K)) if ks is None else list(ks)
        oracle.use_openmp(True)
        try:
            masks = capped_exempt_masks([self.states[k] for k in ks], hip_checksum, hip_n_contrib, cap=cap)
        finally:
            oracle.use_openmp(False)
        for k, d in zip(ks, masks):
            self.unstable[k] = d
        return [int(d.sum()) for d in masks]

    def subset(self, idx):
        r = OracleRun.__new__(OracleRun)
        r.scene, r.K, r.kw = self.scene, len(idx), self.kw
        r.states, r.unstable = [self.states[i] for i in idx], [self.unstable[i] for i in idx]
        return r

    def mask(self, gC, gD=None):
        """Zero the upstream gradients on the unstable pixels: a pair sitting on one of the reference's thresholds may
        legitimately be blended by one implementation and skipped by the other; with no gradient flowing through those
        pixels every remaining gradient term is held to the bar."""
        gC = gC.copy()
        gD = None if gD is None else gD.copy()
        for k, un in enumerate(self.unstable):
            gC[k][:, un] = 0.0
            if gD is not None:
                gD[k][:, un] = 0.0
        return gC, gD

    def backward(self, gC, gD=None):
        out = {}
        oracle.use_openmp(True)
        try:
            for mode in ("double", "f32", "fma"):
                oracle.set_accum_f32(mode == "f32")
                oracle.use_fma(mode == "fma")
                gs = oracle.map_subframes(lambda k: oracle.backward(self.states[k], gC[k], None if gD is None else gD[k]),
                                          range(len(self.states)))
                r = {}
                for name, key in (("dL_dmeans3D", "dL_dmeans3D"), ("dL_dopacities", "dL_dopacity"), ("dL_dsh", "dL_dsh"),
                                  ("dL_dscales", "dL_dscales"), ("dL_drotations", "dL_drotations"),
                                  ("dL_dcolors_precomp", "dL_dcolors"), ("dL_dcov3D_precomp", "dL_dcov3D")):
                    r[name] = sum(g[key].astype(np.float64) for g in gs)
                for name in ("dL_dmeans2D", "dL_dviewmatrix", "dL_dprojmatrix"):
                    r[name] = np.stack([g[name] for g in gs]).astype(np.float64)
                # the compositing backward's per-(subframe, Gaussian) conic sink (backward.cu:620-637: .x, .y, .w of the
                # float4) and the per-Gaussian dL_dcov3D that leaves computeCov2DCUDA (backward.cu:145-295), i.e. the
                # values BEFORE the scale / rotation chain
                r["dL_dconic"] = np.stack([g["dL_dconic"][:, [0, 1, 3]] for g in gs]).astype(np.float64)
                r["dL_dcov3D"] = sum(g["dL_dcov3D"].astype(np.float64) for g in gs)
                out[mode] = r
        finally:
            oracle.use_fma(False)
            oracle.set_accum_f32(False)
            oracle.use_openmp(False)
        return out


CHAIN_KEYS = {"dL_dmeans3D", "xyz", "dL_dscales", "scaling", "dL_drotations", "rotation", "dL_dcov3D_precomp",
              "dL_dcov3D"}     # (xyz and dL_dcov3D turn out well-conditioned everywhere; they are kept here so that it shows)
# dL_dconic (the compositing backward's own sink) joined the conditioning-aware keys in round 6: with the exempt PIXELS cut from
# every pixel within a margin of a threshold (0.5 %) to the pixels whose decisions really differ (1e-5), rows on which two
# fp32 builds of the REFERENCE differ by several 1e-4 -- sums of signed w dx^2 terms that cancel -- are no longer hidden
# behind the mask (cfg5: the worst row is 1.5e-4 off here where the reference's own builds are 3.7e-4 apart).  The rows the
# reference agrees with itself on (noise <= WELL_ROW) keep the flat bars; the rows in between must stay within
# MID_NOISE_MULT x the reference's own noise.
NOISE_AWARE_DIRECT = {"dL_dconic"}
MID_NOISE_MULT = 10.0
ILL_ROW = 1e-3         # a Gaussian is ill-conditioned for a chain output when two correct fp32 builds of the reference ITSELF
                       # (fp32 vs double accumulation; FMA contraction on vs off) differ by more than this on its row
ILL_FRAC = 5e-4        # at most this fraction of the Gaussians that receive a gradient may be ill-conditioned (+ ILL_MIN)
ILL_MIN = 2
EXC_FRAC = 1e-6        # named exceptions among the well-conditioned rows (see assert_grads_close): none below 1e6 active rows
EXC_MULT = 3.0         # ... each within this multiple of the row bar
POSE_NOISE_MULT = 4.0  # dL_dviewmatrix sums the chain over ALL Gaussians, the ill-conditioned ones included


def row_errors(a, b, floor=ROW_FLOOR, _ref=None):
    """Per-row version of grad_errors: (err[rows], dn_rowmax[rows], colmax[cols]).  Each component is normalised by its
    column scale, a row's error is measured against the row's own largest normalised component, floored at `floor`.
    _ref: what depends on b alone (row_reference(b)), when several arrays are held against the same b."""
    b = np.asarray(b, np.float64)
    b = b.reshape(b.shape[0], -1)
    colmax, scale, bn_rowmax = _ref if _ref is not None else row_reference(b)
    d = np.subtract(np.asarray(a, np.float64).reshape(b.shape), b)
    np.abs(d, out=d)
    d /= scale
    dn_rowmax = d.max(axis=1)
    return dn_rowmax / np.maximum(bn_rowmax, floor), dn_rowmax, colmax


def row_reference(b):
    """(colmax, scale, largest normalised component per row) of the reference array of row_errors."""
    b = np.asarray(b, np.float64)
    b = b.reshape(b.shape[0], -1)
    ab = np.abs(b)
    colmax = ab.max(axis=0)
    scale = np.where(colmax > 0, colmax, 1.0)
    ab /= scale
    return colmax, scale, ab.max(axis=1)


WELL_ROW = 5e-5        # end to end, a chain output is held to the flat bars on the Gaussians whose row two correct fp32 builds
                       # of the reference (fp32 vs double accumulation, FMA contraction on vs off) move by less than this
WELL_FRAC = 0.99       # ... and those must be (at least) this fraction of the Gaussians that receive a gradient
REPORT_ONLY = os.environ.get("DGS_PARITY_REPORT", "0") == "1"


def _check(cond, msg, failures):
    if not cond:
        if REPORT_ONLY:
            failures.append(msg)
        else:
            raise AssertionError(msg)


def assert_grads_close(hip, ora, keys, tol=GRAD_TOL, floor=ROW_FLOOR, report=None, row_tol=ROW_TOL, ill_frac=ILL_FRAC,
                       ill_min=ILL_MIN, well_frac=WELL_FRAC, chain_tol=None):
    """hip[key] against ora["double"][key] with FLAT bars: every gradient component (column) within `tol` = 1e-4 of its
    own largest magnitude, every Gaussian (row) within `row_tol` = 1e-3 of its own gradient (floored at `floor` x the
    column scale); pose matrices per [4,4] matrix relative to its largest entry.

      * Direct outputs of the compositing backward and what is linear in them (dL_dmeans2D, dL_dconic, opacity, SH /
        colours, dL_dprojmatrix) and dL_dcov3D: the flat bars, nothing else.
      * Outputs behind the cov3D -> scale / rotation chain (CHAIN_KEYS), where r_i^T dSigma r_i cancels for splats whose
        gradient is dominated by another axis: the same flat bars on every WELL-CONDITIONED Gaussian -- one whose row two
        correct fp32 builds of the reference itself move by less than WELL_ROW (noise = max of |fp32 accumulation - double
        accumulation| and |FMA-contracted build - uncontracted build|, ora["f32"] / ora["fma"] vs ora["double"]).  The
        well-conditioned Gaussians must be >= WELL_FRAC of those that receive a gradient; the Gaussians above ILL_ROW
        are counted against ill_min + ill_frac x active and reported by index; in between nothing is asserted but
        finiteness (their error is reported next to their noise).
      * dL_dviewmatrix is a sum of ~P signed per-Gaussian terms that cancel to a small total, the ill-conditioned Gaussians
        included: max(tol, POSE_NOISE_MULT x the largest difference between two fp32 builds of the reference over the K
        matrices of the problem).  (The HIP path adds these terms in double beyond the 64-lane wave sums.)"""
    failures = []
    for key in keys:
        b, n, f = ora["double"][key], ora["f32"][key], ora["fma"][key]
        a = np.asarray(hip[key], np.float64).reshape(b.shape)
        _check(np.isfinite(a).all(), f"{key}: not finite", failures)
        if key in ("dL_dviewmatrix", "dL_dprojmatrix"):
            # one noise level for the K matrices of a problem: the largest difference between two fp32 builds of the
            # reference over the subframes (the per-subframe values are single samples of the same rounding process)
            en = max(max(relerr(n[k], b[k]), relerr(f[k], b[k])) for k in range(b.shape[0]))
            for k in range(b.shape[0]):
                e = relerr(a[k], b[k])
                if report is not None:
                    report.append((key, k, {"vs_oracle": e, "oracle_noise_max_k": en}))
                bar = tol if key == "dL_dprojmatrix" else max(tol, POSE_NOISE_MULT * en)
                _check(e <= bar, f"{key}[{k}]: {e:.2e} (bar {bar:.2e}, oracle noise {en:.2e})", failures)
            continue
        if key in ("dL_dmeans2D", "dL_dconic"):       # [K,P,c] -> rows = (k, Gaussian)
            a, b, n, f = (x.reshape(-1, x.shape[-1]) for x in (a, b, n, f))
            if key == "dL_dmeans2D":
                a, b, n, f = a[:, :2], b[:, :2], n[:, :2], f[:, :2]
        ref_b = row_reference(b)
        err_row, _, colmax = row_errors(a, b, floor, ref_b)
        if os.environ.get("DGS_PARITY_ROW") and REPORT_ONLY:      # one Gaussian across all outputs (debugging aid)
            rsel = int(os.environ["DGS_PARITY_ROW"])
            rows_ = [rsel] if a.shape[0] == b.shape[0] and key not in ("dL_dmeans2D", "dL_dconic") else \
                [kk * (a.shape[0] // max(ora["double"]["dL_dmeans2D"].shape[0], 1)) + rsel
                 for kk in range(ora["double"]["dL_dmeans2D"].shape[0])]
            for rr in rows_:
                if rr < a.shape[0]:
                    print(f"   [row {rsel}] {key}[{rr}]: hip {a.reshape(a.shape[0], -1)[rr].tolist()} double "
                          f"{b.reshape(b.shape[0], -1)[rr].tolist()} f32 {n.reshape(n.shape[0], -1)[rr].tolist()} "
                          f"colmax {colmax.tolist()}")
        d = np.abs(a - b).reshape(a.shape[0], -1)
        nz = colmax > 0

        def flat(sel):
            col = float((d[sel][:, nz].max(axis=0) / colmax[nz]).max()) if nz.any() and sel.any() else 0.0
            return col, (float(err_row[sel].max()) if sel.any() else 0.0)

        noise_row = np.maximum(row_errors(n, b, floor, ref_b)[0], row_errors(f, b, floor, ref_b)[0])
        if key not in CHAIN_KEYS and key not in NOISE_AWARE_DIRECT:
            col, row = flat(np.ones(a.shape[0], bool))
            if report is not None:
                rep = {"col": col, "row": row, "noise_row_max": float(noise_row.max())}
                if nz.any():      # where the column measure is reached, and how far two fp32 builds of the reference differ there
                    dcol = d[:, nz] / colmax[nz]
                    w = int(np.argmax(dcol.max(axis=1)))
                    ncol = np.maximum(np.abs(n - b).reshape(a.shape[0], -1), np.abs(f - b).reshape(a.shape[0], -1))[:, nz] / colmax[nz]
                    rep["col_worst_row"] = w
                    rep["col_noise_at_worst_row"] = float(ncol[w].max())
                    rep["col_noise_max"] = float(ncol.max())
                report.append((key, rep))
            _check(col <= tol, f"{key} col: {col:.2e} > {tol:.0e}", failures)
            _check(row <= row_tol, f"{key} row: {row:.2e} > {row_tol:.0e}", failures)
            continue
        active_rows = np.abs(b.reshape(b.shape[0], -1)).max(axis=1) > 0
        active = int(active_rows.sum())
        ill = noise_row > ILL_ROW
        well = noise_row <= WELL_ROW
        mid = ~ill & ~well
        col, row = flat(well)
        rep = {"active": active, "well_frac": float((well & active_rows).sum() / max(active, 1)), "col": col, "row": row,
               "mid": int(mid.sum()), "mid_row": float(err_row[mid].max()) if mid.any() else 0.0,
               "mid_row_over_noise": float((err_row[mid] / noise_row[mid]).max()) if mid.any() else 0.0,
               "ill": int(ill.sum()), "ill_rows": np.nonzero(ill)[0][:8].tolist(),
               "ill_row": float(err_row[ill].max()) if ill.any() else 0.0}
        if REPORT_ONLY:      # how the choice of WELL_ROW plays out
            rep["by_well_row"] = {thr: ((noise_row <= thr) & active_rows).sum() / max(active, 1) for thr in (1e-4, 5e-5, 2e-5)}
            rep["by_well_row"] = {thr: (round(float(fr), 5),) + tuple(f"{x:.2e}" for x in flat(noise_row <= thr))
                                  for thr, fr in rep["by_well_row"].items()}
        if REPORT_ONLY and well.any():      # the worst well-conditioned row, by name and value
            w = int(np.argmax(np.where(well, err_row, -1.0)))
            rep["worst_well"] = {"row": w, "err": float(err_row[w]), "noise": float(noise_row[w]),
                                 "hip": a.reshape(a.shape[0], -1)[w].tolist(), "double": b.reshape(b.shape[0], -1)[w].tolist(),
                                 "f32": n.reshape(n.shape[0], -1)[w].tolist(), "fma": f.reshape(f.shape[0], -1)[w].tolist(),
                                 "colmax": colmax.tolist()}
        if report is not None:
            report.append((key, rep))
        if key in NOISE_AWARE_DIRECT and mid.any():
            _check(rep["mid_row_over_noise"] <= MID_NOISE_MULT,
                   f"{key}: a row between the well- and ill-conditioned ones is {rep['mid_row_over_noise']:.1f} x the reference's "
                   f"own fp32 noise off (allowed {MID_NOISE_MULT})", failures)
        _check(ill.sum() <= ill_min + ill_frac * active,
               f"{key}: {int(ill.sum())} of {active} Gaussians are ill-conditioned (two fp32 builds of the reference differ "
               f"by more than {ILL_ROW} on their row)", failures)
        _check(rep["well_frac"] >= well_frac, f"{key}: only {rep['well_frac']:.4f} of the Gaussians are well-conditioned", failures)
        # NAMED exceptions: at most EXC_FRAC of the Gaussians that receive a gradient (none below a million of them; 3 of
        # cfg5's 3.8 M) may sit above the flat bars although the reference's own builds agree on them -- each is printed
        # with its index and must still be within EXC_MULT x the bars; everyone else is held to the flat bars.
        n_exc = int(EXC_FRAC * active)
        if n_exc > 0 and (col > tol or row > row_tol):
            over = np.nonzero(well & ((err_row > row_tol) | ((d[:, nz] / colmax[nz]).max(axis=1) > tol)))[0]
            _check(len(over) <= n_exc, f"{key}: {len(over)} well-conditioned Gaussians above the flat bars (allowed {n_exc})",
                   failures)
            if len(over) <= n_exc:
                worst = float(err_row[over].max())
                print(f"   [{key}] named exceptions (well-conditioned rows above the flat bars): "
                      + ", ".join(f"Gaussian {int(i)}: row {err_row[i]:.2e}, noise {noise_row[i]:.2e}" for i in over))
                _check(worst <= EXC_MULT * row_tol, f"{key}: named exception at {worst:.2e} > {EXC_MULT} x {row_tol:.0e}", failures)
                keep = well.copy()
                keep[over] = False
                col, row = flat(keep)
                rep["exceptions"] = over.tolist()
        ctol = tol if (chain_tol is None or key not in CHAIN_KEYS) else chain_tol
        _check(col <= ctol, f"{key} col on well-conditioned rows: {col:.2e} > {ctol:.0e}", failures)
        _check(row <= row_tol, f"{key} row on well-conditioned rows: {row:.2e} > {row_tol:.0e}", failures)
    if REPORT_ONLY and failures:
        print("PARITY REPORT (no assertion):")
        for f_ in failures:
            print("   FAIL", f_)


def hip_backward_internals(debug, radii, ks=None, means2D=None):
    """The compositing backward's per-(subframe, Gaussian) totals read back from the backward scratch
    (dgs_backward_scratch_layout; `debug` = the dict diff_gaussian_rasterization.BACKWARD_DEBUG received), for the
    subframes `ks` (default all): dL_dconic [k,P,3] = -0.5 (S_xx, S_xy, S_yy), dL_dcolors_k [k,P,3], dL_ddepths_k [k,P,1],
    and the K-summed dL_dcov3D [P,6].  Totals are defined for visible pairs only (zeros elsewhere here)."""
    import torch
    from deblurgs_amd import _lib
    K, P, R = debug["K"], debug["P"], debug["R"]
    so, _ = _lib.backward_scratch_layout(R, P, K)
    sums = debug["scratch"][so:so + K * P * 64].view(dtype=torch.float32).reshape(K, P, 16)[..., :12]
    radii = torch.as_tensor(np.asarray(radii)).reshape(K, P) if not torch.is_tensor(radii) else radii.reshape(K, P)
    sel = list(range(K)) if ks is None else list(ks)
    part = sums[sel].cpu().numpy()
    vis = (radii[sel].cpu().numpy() > 0)[..., None]
    out = {"ks": sel, "dL_dconic": np.where(vis, -0.5 * part[..., 2:5].astype(np.float64), 0.0),
           "dL_dcolors_k": np.where(vis, part[..., 6:9], 0.0).astype(np.float32),
           "dL_ddepths_k": np.where(vis, part[..., 9:10], 0.0).astype(np.float32),
           "dL_dcov3D": debug["dL_dcov3D"].cpu().numpy().astype(np.float64)}
    if means2D is not None:
        m = means2D[sel] if not torch.is_tensor(means2D) else means2D[sel].cpu().numpy()
        out["dL_dmeans2D"] = np.asarray(m, np.float32)
    return out


# ------------------------------------------------------------------------- the product path exactly as bench.py runs it
def cloud_grads_from_activated(scene, ora_res):
    """Chain rule from the oracle's gradients (w.r.t. the activated values the reference rasteriser takes) to the raw
    parameters of the cloud (scene/gaussian_activation.py:29-52, torch.nn.functional.normalize): log-scale, raw
    quaternion, clamped opacity, dc | rest SH split.  float64."""
    sc = scene["scales"].astype(np.float64)
    q = scene["rotations"].astype(np.float64)
    nq = np.linalg.norm(q, axis=1, keepdims=True)
    qn = q / nq
    op = scene["opacities"].astype(np.float64)
    out = {}
    for mode in ("double", "f32", "fma"):
        r = ora_res[mode]
        g_rot = r["dL_drotations"]
        out[mode] = dict(
            xyz=r["dL_dmeans3D"], f_dc=r["dL_dsh"][:, :1], f_rest=r["dL_dsh"][:, 1:],
            opacity=r["dL_dopacities"] * ((op >= 0.0) & (op <= 1.0)),
            scaling=r["dL_dscales"] * sc,
            rotation=(g_rot - qn * (qn * g_rot).sum(axis=1, keepdims=True)) / nq,
            dL_dmeans2D=r["dL_dmeans2D"], dL_dviewmatrix=r["dL_dviewmatrix"], dL_dprojmatrix=r["dL_dprojmatrix"],
            dL_dconic=r["dL_dconic"], dL_dcov3D=r["dL_dcov3D"])
    return out


def hip_cloud_forward_backward(scene, K, dL_dcolor, dL_ddepth=None, cull=True, keep_on_device=False, conic_ks=None):
    """The path bench.py times: GaussianCloud (raw parameters) -> gaussian_renderer.render_subframes ->
    rasterize_cloud_subframes (DgsProblem.raw_params = 1, activations inside the kernels) with tile culling as given,
    loss = <colour, dL_dcolor> (+ <depth, dL_ddepth>), autograd backward."""
    import torch
    from deblurgs_amd import gaussian_renderer
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import RefCamera
    dev = "cuda"
    cloud = GaussianCloud.from_scene(scene, dev)
    assert cloud.fused_activations
    ref = RefCamera(scene["W"], scene["H"], scene["FoVx"], scene["FoVy"], device=dev)
    view = _t(scene["viewmatrix"][:K]).requires_grad_(True)
    proj = _t(scene["projmatrix"][:K]).requires_grad_(True)
    with tile_cull(cull):
        pkg = gaussian_renderer.render_subframes(view, proj, _t(scene["campos"][:K]), ref, cloud, _t(scene["bg"]))
        loss = (pkg["render"] * _t(dL_dcolor)).sum()
        if dL_ddepth is not None:
            loss = loss + (pkg["depth"] * _t(dL_ddepth)).sum()
        from deblurgs_amd import diff_gaussian_rasterization as dgr
        dgr.BACKWARD_DEBUG = dbg = {}
        try:
            loss.backward()
        finally:
            dgr.BACKWARD_DEBUG = None
    torch.cuda.synchronize()
    get = (lambda t: t.detach()) if keep_on_device else (lambda t: t.detach().cpu().numpy())
    out = dict(color=get(pkg["render"]), depth=get(pkg["depth"]), radii=get(pkg["radii"]),
               dL_dmeans2D=get(pkg["viewspace_points"].grad), dL_dviewmatrix=get(view.grad), dL_dprojmatrix=get(proj.grad),
               xyz=get(cloud._xyz.grad), f_dc=get(cloud._features_dc.grad), f_rest=get(cloud._features_rest.grad),
               opacity=get(cloud._opacity.grad), scaling=get(cloud._scaling.grad), rotation=get(cloud._rotation.grad))
    if not keep_on_device:
        out["internals"] = hip_backward_internals(dbg, out["radii"], conic_ks, means2D=out["dL_dmeans2D"])
        out["dL_dconic"], out["dL_dcov3D"] = out["internals"]["dL_dconic"], out["internals"]["dL_dcov3D"]
    return out


CLOUD_KEYS = ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "dL_dmeans2D", "dL_dconic", "dL_dcov3D",
              "dL_dviewmatrix", "dL_dprojmatrix"]


def hip_state_on_device(scene, K, cull=True, raw=True, checksum=False):
    """Forward through the C ABI; returns the outputs and the carved state arrays as torch views ON THE DEVICE (for
    full-size property checks without multi-GB host copies).  raw=True: the cloud's raw parameters, as benchmarked."""
    import torch
    from deblurgs_amd import _lib
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    from deblurgs_amd.cloud import GaussianCloud
    rs = hip_settings(scene, K)._replace(campos=_t(scene["campos"][:K]))
    view, proj, cam = _t(scene["viewmatrix"][:K]), _t(scene["projmatrix"][:K]), _t(scene["campos"][:K])
    with tile_cull(cull), torch.no_grad():
        if raw:
            c = GaussianCloud.from_scene(scene, "cuda")
            R, color, depth, radii, geom, binning, image = dgr._forward_impl(
                K, c._xyz, c._features_dc, None, c._opacity.reshape(-1), c._scaling, c._rotation, None, view, proj, cam,
                rs, raw={"scale_lb": 0.0, "sh_rest": c._features_rest if c._features_rest.shape[1] > 0 else None},
                debug_checksum=checksum)
        else:
            R, color, depth, radii, geom, binning, image = dgr._forward_impl(
                K, _t(scene["means3D"]), _t(scene["sh"]), None, _t(scene["opacities"]).reshape(-1), _t(scene["scales"]),
                _t(scene["rotations"]), None, view, proj, cam, rs, debug_checksum=checksum)
    torch.cuda.synchronize()
    P, W, H = scene["P"], scene["W"], scene["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    L = _lib.layout(P, W, H, K, R)
    v = lambda blob, off, nbytes, dtype, shape: blob[off:off + nbytes].view(dtype).reshape(shape)
    keys = v(binning, L.keys_sorted, R * 8, torch.int64, (R,))
    point_list = v(binning, L.point_list, R * 4, torch.int32, (R,))
    if cull and L.pack_tile_shift > 0:   # compact keys -> the canonical (tile << 32 | emission index, Gaussian) form
        gs, ts = L.pack_g_shift, L.pack_tile_shift
        point_list = ((keys >> gs) & ((1 << (ts - gs)) - 1)).int()
        keys = ((keys >> ts) << 32) | (keys & ((1 << gs) - 1))
    return dict(R=int(R), K=K, T=T, compact_keys=bool(cull and L.pack_tile_shift > 0), sort_bits=L.sort_bits, sort_passes=L.sort_passes, color=color, depth=depth,
                radii=radii, _blobs=(geom, binning, image), contrib_checksum=getattr(R, "contrib_checksum", None),
                tiles_touched=v(geom, L.tiles_touched, K * P * 4, torch.int32, (K, P)),
                tt_tight=v(geom, L.tt_tight, K * P * 4, torch.int32, (K * P,)),
                rows=v(geom, L.geom_rows, K * P * 48, torch.float32, (K, P, 12)),
                final_T=v(image, L.final_T, K * W * H * 4, torch.float32, (K, H * W)),
                n_contrib=v(image, L.n_contrib, K * W * H * 4, torch.int32, (K, H * W)),
                ranges=v(image, L.ranges, K * T * 8, torch.int32, (K * T, 2)),
                keys=keys, point_list=point_list)

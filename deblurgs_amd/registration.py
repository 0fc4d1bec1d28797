"""Starting poses for unposed test images: the step of the reference's evaluation that `initialize_test_pose`
(test.py:188-398) does by shelling out to a `colmap` binary -- SIFT on renders of the training middle cameras, triangulation,
image registration.  No such binary exists here, so this module seeds the iNeRF-style fit (evaluation.optimize_test_pose) by
COARSE PHOTOMETRIC REGISTRATION against the trained cloud instead.  It is NOT the reference's method:

    candidate bank     poses taken from the learned training trajectories (candidate_cameras), rendered K at a time through
                       the forward-only rasteriser, finished to 8 bits (dgs_frames_finish) and box-reduced (dgs_box_reduce_u8)
    seed               the sum of absolute differences of every test image against every candidate (dgs_sad_matrix); the
                       best candidate per image, the lowest index on ties
    pattern search     refine_rounds times: the 12 poses c2w . exp(+-step . e) around every image's pose (seed_lattice) are
                       rendered and scored (the grouped dgs_sad_matrix); an image moves to its best lattice pose when that
                       scores STRICTLY lower, else its two steps are halved

Everything that is scored is integer arithmetic on the 8-bit images the fit's own L1 sees (clamped, tone-mapped), so every
score is exact and reproducible.  How well the seed lands on real captures is unmeasured (no dataset is available to this
project); the basin of the fit that follows is a few degrees and a few percent of the scene's depth.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, render_path
from .raster_call import _ptr, _stream

SAD_CHUNK = 16384        # DGS_SAD_CHUNK_DWORDS: dwords of an image one block of dgs_sad_matrix sums
SAD_TILE_A = 4           # DGS_SAD_TILE_A: images of `a` one block of the all-pairs kernel holds in registers
LATTICE = ("+tx", "-tx", "+ty", "-ty", "+tz", "-tz", "+rx", "-rx", "+ry", "-ry", "+rz", "-rz")

SeedResult = namedtuple("SeedResult", "cameras scores seed_index seed_score final_score moves poses trans_step rot_step_rad")
SeedResult.__doc__ = """What seed_test_poses returns.
    cameras       [evaluation.TestCamera] * n, original_image set: what optimize_test_pose / evaluate take
    scores        int64 [n,C] (device): the SAD of every test image against every candidate
    seed_index    int64 [n] (numpy): the candidate each image starts from (row of candidate_cameras' table)
    seed_score    int64 [n]: its score;  final_score: the score of the returned pose
    moves         [(round, image, lattice index, score before, score after)] of the pattern search
    poses         float64 [n,4,4]: the returned camera-to-world matrices
    trans_step, rot_step_rad   float64 [n]: every image's steps after the last round"""


# ------------------------------------------------------------------------------------------------- device wrappers
def box_reduce_u8(frames_u8, s, out=None):
    """uint8 [G,H,W,3] on the device -> int32 [G,pitch] (dgs_box_reduce_u8): the s x s box mean of every frame, one dword
    r | g << 8 | b << 16 per pixel of the [H // s, W // s] image, pitch = (h w + 3) & ~3, the pad zero.  out: where to write
    (a contiguous int32 [G,pitch], 16-byte aligned)."""
    render_path._need_device(frames_u8, "box_reduce_u8")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError("box_reduce_u8 takes a uint8 [G,H,W,3] tensor")
    frames_u8 = frames_u8.contiguous()
    G, H, W, _ = (int(v) for v in frames_u8.shape)
    s = int(s)
    pitch = ((max(H // max(s, 1), 0) * max(W // max(s, 1), 0)) + 3) & ~3
    if out is None:
        out = torch.empty((G, max(pitch, 4)), dtype=torch.int32, device=frames_u8.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (G, pitch) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 [{G},{pitch}] tensor")
    _lib.check(_lib.lib().dgs_box_reduce_u8(_ptr(frames_u8), G, H, W, s, _ptr(out), _stream(frames_u8.device)),
               "dgs_box_reduce_u8")
    return out


def sad_matrix(a, b, group=0, tmp=None):
    """a int32 [na,L], b int32 [nb,L] on the device (L a multiple of 4 dwords) -> int64 [na,nb]: the sum of |a_i - b_j| over
    the 4 L bytes (dgs_sad_matrix).  group = m > 0 (nb == na m): int64 [na,m], image a_i against b_{i m + j}.  tmp: a uint8
    work area of at least dgs_sad_matrix_tmp_bytes(na, nb, L) bytes (its contents do not matter)."""
    render_path._need_device(a, "sad_matrix")
    render_path._need_device(b, "sad_matrix")
    if a.dim() != 2 or b.dim() != 2 or a.dtype != torch.int32 or b.dtype != torch.int32 or a.shape[1] != b.shape[1]:
        raise ValueError("sad_matrix takes two int32 tensors [na,L] and [nb,L]")
    a, b = a.contiguous(), b.contiguous()
    na, L = (int(v) for v in a.shape)
    nb, group = int(b.shape[0]), int(group)
    lib = _lib.lib()
    out = torch.empty((na, group if group > 0 else nb), dtype=torch.int64, device=a.device)
    need = lib.dgs_sad_matrix_tmp_bytes(na, nb, L)
    if tmp is None:
        tmp = torch.empty(max(need, 16), dtype=torch.uint8, device=a.device)
    elif tmp.dtype != torch.uint8 or tmp.numel() < need or not tmp.is_contiguous() or tmp.device != a.device:
        raise ValueError(f"tmp must be a contiguous uint8 tensor of at least {need} bytes on the images' device")
    _lib.check(lib.dgs_sad_matrix(_ptr(a), na, _ptr(b), nb, group, L, _ptr(out), _ptr(tmp), _stream(a.device)),
               "dgs_sad_matrix")
    return out


# ------------------------------------------------------------------------------------------------- candidates
def _se3_between(c2w_a, c2w_b, fraction):
    """The pose a fraction of the way from a to b on SE(3): a . exp(fraction . log(a^-1 b)), float64 [4,4] (column-vector
    camera-to-world matrices; pose.se3_log_map / se3_exp_map take the transposed, row-vector form)."""
    from . import pose
    rel = torch.from_numpy(np.linalg.inv(c2w_a) @ c2w_b)
    log = pose.se3_log_map(rel.transpose(0, 1)[None].contiguous())
    step = pose.se3_exp_map(float(fraction) * log)[0].transpose(0, 1).numpy()
    return c2w_a @ step


@torch.no_grad()
def _middle_cam(motion, i):
    nu = motion._sample_nu_from_alignment(i)
    mid = nu.shape[0] // 2
    return motion.get_trajectory(i, nu[mid:mid + 1])[0]


@torch.no_grad()
def candidate_cameras(motion, subframes=3, between=1, exclude=()):
    """The candidate poses of the seed: (cams, table), a list of MiniCams and one (kind, view, index) row per camera.
        ("trajectory", i, k)   the camera of training view i at nu = linspace(0, 1, subframes)[k] of its learned trajectory,
                               for every view not in `exclude`, views in order, k in order
        ("between", i, j)      after those: pose j of `between` (j = 1 ..) interpolated on SE(3) from the middle camera of
                               kept view i to the middle camera of the next kept view, at the fraction j / (between + 1)
    The curves are evaluated with curve_random_sample off: two calls return the same matrices."""
    subframes, between = int(subframes), int(between)
    if subframes < 1 or between < 0:
        raise ValueError("subframes must be at least 1 and between at least 0")
    skip = {int(i) for i in exclude}
    views = [i for i in range(len(motion)) if i not in skip]
    if not views:
        raise ValueError("exclude leaves no training view")
    jitter, motion.curve_random_sample = motion.curve_random_sample, False
    try:
        nu = torch.linspace(0.0, 1.0, subframes)
        cams, table = [], []
        for i in views:
            for k, cam in enumerate(motion.get_trajectory(i, nu)):
                cam.world_view_transform = cam.world_view_transform.detach()
                cam.full_proj_transform = cam.full_proj_transform.detach()
                cam.camera_center = cam.camera_center.detach()
                cams.append(cam)
                table.append(("trajectory", i, k))
        if between > 0 and len(views) > 1:
            middle = [render_path.cam_to_c2w(_middle_cam(motion, i)) for i in views]
            for v in range(len(views) - 1):
                for j in range(1, between + 1):
                    cams.append(render_path.c2w_to_cam(cams[0], _se3_between(middle[v], middle[v + 1], j / (between + 1))))
                    table.append(("between", views[v], j))
    finally:
        motion.curve_random_sample = jitter
    return cams, table


def _so3_exp(w):
    """Rodrigues' formula in float64 with the series of its two factors at small angles."""
    theta = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if theta < 1e-6:
        a, b = 1.0 - theta * theta / 6.0, 0.5 - theta * theta / 24.0
    else:
        a, b = np.sin(theta) / theta, (1.0 - np.cos(theta)) / (theta * theta)
    return np.eye(3) + a * K + b * (K @ K)


def seed_lattice(c2w, trans_step, rot_step_rad):
    """The 12 poses c2w . exp(+-step . e) of a pattern-search round, float64 [12,4,4], in the camera's OWN frame: a
    translation by trans_step along, or a rotation by rot_step_rad about, each of its axes, in LATTICE's order
    (+tx, -tx, +ty, -ty, +tz, -tz, +rx, -rx, +ry, -ry, +rz, -rz).  Translations move the camera centre by exactly
    trans_step; rotations leave it where it is."""
    c2w = np.asarray(c2w, dtype=np.float64)
    out = np.empty((12, 4, 4), dtype=np.float64)
    for axis in range(3):
        e = np.zeros(3)
        e[axis] = 1.0
        for k, sign in enumerate((1.0, -1.0)):
            move = np.eye(4)
            move[:3, 3] = sign * float(trans_step) * e
            out[2 * axis + k] = c2w @ move
            turn = np.eye(4)
            turn[:3, :3] = _so3_exp(sign * float(rot_step_rad) * e)
            out[6 + 2 * axis + k] = c2w @ turn
    return out


def default_steps(middle_c2ws, fraction=0.25):
    """(trans_step, rot_step_rad) from the data: `fraction` of the median distance between the centres of consecutive
    training middle cameras, and of the median angle of their relative rotations."""
    m = np.asarray(middle_c2ws, dtype=np.float64)
    if m.shape[0] < 2:
        raise ValueError("with a single training view trans_step and rot_step_deg must be given")
    dist = np.linalg.norm(m[1:, :3, 3] - m[:-1, :3, 3], axis=1)
    rel = np.einsum("nji,njk->nik", m[:-1, :3, :3], m[1:, :3, :3])
    angle = np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) * 0.5, -1.0, 1.0))
    return fraction * float(np.median(dist)), fraction * float(np.median(angle))


# ------------------------------------------------------------------------------------------------- the seed
def _reduced_renders(cams, cloud, bg, tone_mapping, factor, frames_per_call):
    """int32 [len(cams),pitch]: every camera rendered (K per call), finished to 8 bits and box-reduced."""
    rows = []
    for b, e in render_path.frame_groups(cams, frames_per_call):
        color = render_path.render_group(cams[b:e], cloud, bg)["render"]
        rows.append(box_reduce_u8(render_path.frames_finish(color, tone_mapping), factor))
    return torch.cat(rows, dim=0) if len(rows) > 1 else rows[0]


def _test_camera(ref, c2w, image):
    """The evaluation.TestCamera of a camera-to-world pose: R is stored as the c2w rotation, T is the translation row of
    the world-to-view matrix (-centre . R), as c2w_to_cam forms it."""
    from .evaluation import TestCamera
    rot, centre = c2w[:3, :3], c2w[:3, 3]
    return TestCamera(rot.copy(), -centre @ rot, ref.FoVx, ref.FoVy, ref.image_width, ref.image_height,
                      original_image=image, znear=ref.znear, zfar=ref.zfar)


@torch.no_grad()
def seed_test_poses(motion, cloud, test_images, bg, tone_mapping=None, *, factor=8, subframes=3, between=1,
                    refine_rounds=3, trans_step=None, rot_step_deg=None, frames_per_call=None, exclude=()):
    """Starting poses of n unposed test images (module docstring): a SeedResult.
    test_images: [n,3,H,W] floats in display space (what the fit compares tone_map(render) with), of motion.ref_cam's size --
    the reference also reuses one training camera's intrinsics for its test views.  tone_mapping: the training's (identity
    or gamma: dgs_frames_finish's two).  factor: the box the 8-bit images are reduced by before they are compared.
    trans_step / rot_step_deg: the first round's lattice steps (default: default_steps of the training middle cameras)."""
    ref = motion.ref_cam
    H, W = int(ref.image_height), int(ref.image_width)
    images = torch.stack(list(test_images)) if not torch.is_tensor(test_images) else test_images
    if images.dim() != 4 or tuple(images.shape[1:]) != (3, H, W):
        raise ValueError(f"test_images must be [n,3,{H},{W}]: the size of motion.ref_cam, whose intrinsics the test views reuse")
    factor, rounds = int(factor), int(refine_rounds)
    per_call = render_path.FRAMES_PER_CALL if frames_per_call is None else int(frames_per_call)
    cams, table = candidate_cameras(motion, subframes=subframes, between=between, exclude=exclude)
    device = cams[0].world_view_transform.device
    if device.type != "cuda":
        raise RuntimeError("seed_test_poses needs a motion module and a cloud on a HIP device (no CPU fallback)")
    n = int(images.shape[0])
    if rounds > 0 and (trans_step is None or rot_step_deg is None):
        skip = {int(i) for i in exclude}
        jitter, motion.curve_random_sample = motion.curve_random_sample, False
        try:
            middle = [render_path.cam_to_c2w(_middle_cam(motion, i)) for i in range(len(motion)) if i not in skip]
        finally:
            motion.curve_random_sample = jitter
        auto = default_steps(middle)
        trans_step = auto[0] if trans_step is None else trans_step
        rot_step_deg = np.rad2deg(auto[1]) if rot_step_deg is None else rot_step_deg
    bg = bg.to(device=device, dtype=torch.float32)
    bank = _reduced_renders(cams, cloud, bg, tone_mapping, factor, per_call)
    tests = box_reduce_u8(render_path.frames_finish(images.to(device=device, dtype=torch.float32), None), factor)
    scores = sad_matrix(tests, bank)
    host = scores.cpu().numpy()
    seed_index = host.argmin(axis=1)                    # numpy: the first of equal minima
    seed_score = host[np.arange(n), seed_index]
    poses = np.stack([render_path.cam_to_c2w(cams[c]) for c in seed_index])
    current = seed_score.copy()
    t_step = np.full(n, 0.0 if trans_step is None else float(trans_step))
    r_step = np.full(n, 0.0 if rot_step_deg is None else float(np.deg2rad(rot_step_deg)))
    moves = []
    for rnd in range(rounds):
        lattice = np.concatenate([seed_lattice(poses[i], t_step[i], r_step[i]) for i in range(n)])
        lat_cams = [render_path.c2w_to_cam(cams[0], m) for m in lattice]
        lat = _reduced_renders(lat_cams, cloud, bg, tone_mapping, factor, per_call)
        grouped = sad_matrix(tests, lat, group=12).cpu().numpy()
        for i in range(n):
            k = int(grouped[i].argmin())
            if grouped[i, k] < current[i]:
                moves.append((rnd, i, k, int(current[i]), int(grouped[i, k])))
                poses[i], current[i] = lattice[12 * i + k], grouped[i, k]
            else:
                t_step[i] *= 0.5
                r_step[i] *= 0.5
    out_cams = [_test_camera(ref, poses[i], images[i]) for i in range(n)]
    return SeedResult(out_cams, scores, seed_index.astype(np.int64), seed_score.astype(np.int64), current.astype(np.int64),
                      moves, poses, t_step, r_step)

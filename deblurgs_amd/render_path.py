"""Camera-path rendering: the reference's render_spiral.py and render_trainview.py (the two programs train.py:230-233 runs
after every training) on the batched forward-only rasteriser, with the 8-bit frames made on the device.

    render_frames     K cameras per rasteriser call (gaussian_renderer.render_subframes under no_grad: forward_only), then
                      dgs_frames_finish -- tone map, clip, * 255, truncate, NCHW -> NHWC, centre crop in one pass -- and a
                      non_blocking copy of the packed uint8 frames into one of two pinned host buffers; the host drains
                      group g - 1 while group g is enqueued.  One stream, a linear chain, no graph.
    render_spiral     get_render_path (utils/export_utils.py:86-152) + render_spiral.py:27-33
    render_trainview  render_trainview.py:23-52: the middle camera of every training trajectory beside its ground truth
    write_frames      PNG files through PIL when it is importable, else one .npy.  render_spiral / render_trainview take a
                      writer(frames, path, fps) callable for the video: deblurgs_amd.video.make_video is one (a
                      Motion-JPEG AVI, the frames encoded on the device); imageio is no dependency of this package.
    write_frames_png  render_frames' loop with the PNG files made on the device (deblurgs_amd/png.py): the finished bytes
                      cross to the host, not the raw frames.  Opt-in; needs no PIL.
    write_frames_video  the same loop with JPEG files made on the device (deblurgs_amd/jpeg.py) appended to one
                      Motion-JPEG AVI (deblurgs_amd/video.py).  Opt-in.
                      All three start from one _path_plan (the cameras' groups, the shared image size, the crop window);
                      the two that make files are one _path_files pipeline -- render + encode group g, copy the bytes of
                      g - 1, write g - 2, over two device_files.Download slots -- with their own encode and sink.

Path geometry is the reference's, in float64 numpy: mean_camera_pose / c2w_from_eye (utils/mvg_utils.py:56-98),
cam_to_c2w / c2w_to_cam (scene/cameras.py:77-120), center_crop_window (center_crop_with_ratio's int() arithmetic), all
pinned by tests/golden/paths_golden.npz.  depth_colorize (utils/export_utils.py:44-65) runs on the device for its default
clip_percentage = 1 (dgs_depth_range + dgs_depth_colorize); its jet_r table is built here from the published segment
definition of "jet" (matplotlib need not be installed) and pinned by the same fixture.
"""
import collections
import math
import os

import numpy as np
import torch

from . import _lib, device_files, gaussian_renderer, losses
from .pose import MiniCam, get_projection_matrix
from .raster_call import _ptr, _stream

# Cameras per rasteriser call: the smallest of 1, 4, 8, 16 whose frames/s is within 1.5 % of the best (variants/NOTES.md's
# kill rule) in tools/path_timing.py's run at the metric scene -- 934 / 1155 / 1135 / 966 frames/s, 4 ahead of 1 in all five
# rounds (profiles/path_timing.json; one box, one run).  Device memory grows with it: 1.1 GB at 4,
# 4.5 GB at 16.
FRAMES_PER_CALL = 4


# ------------------------------------------------------------------------------------------------- path geometry
def mean_camera_pose(c2ws):
    """[n,4,4] camera-to-world matrices -> their mean pose [4,4]: the mean of the translations and the chordal L2 mean of
    the rotations -- the unit quaternion that maximises sum_i (q . q_i)^2, i.e. the eigenvector of sum_i q_i q_i^T with the
    largest eigenvalue (what scipy's Rotation.mean() computes; scipy is not imported)."""
    c2ws = np.asarray(c2ws, dtype=np.float64)
    A = np.zeros((4, 4))
    for R in c2ws[:, :3, :3]:
        q = _rotmat_to_quat(R)
        A += np.outer(q, q)
    _, vecs = np.linalg.eigh(A)
    out = np.eye(4)
    out[:3, :3] = _quat_to_rotmat(vecs[:, -1])
    out[:3, 3] = c2ws[:, :3, 3].mean(axis=0)
    return out


def _rotmat_to_quat(R):
    """(x, y, z, w) of a rotation matrix, pivoting on the largest of (m00, m11, m22, trace) (pose.rotmat_to_unitquat)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    c = int(np.argmax([R[0, 0], R[1, 1], R[2, 2], t]))
    q = np.empty(4)
    if c == 3:
        q[:] = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + t]
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1.0 - t + 2.0 * R[i, i]
        q[j] = R[j, i] + R[i, j]
        q[k] = R[k, i] + R[i, k]
        q[3] = R[k, j] - R[j, k]
    return q / np.linalg.norm(q)


def _quat_to_rotmat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]])


def c2w_from_eye(eye, lookat, up):
    """The camera-to-world matrix of a camera at `eye` whose +z axis points at `lookat`, x = up cross z, y = z cross x
    (utils/mvg_utils.py:83-98)."""
    eye, lookat, up = (np.asarray(v, dtype=np.float64) for v in (eye, lookat, up))
    z = lookat - eye
    x = np.cross(up, z)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([x / np.linalg.norm(x), y / np.linalg.norm(y), z / np.linalg.norm(z)], axis=1)
    c2w[:3, 3] = eye
    return c2w


def cam_to_c2w(cam):
    """scene/cameras.py:77-97: the rotation block of world_view_transform (row-vector convention: it IS the c2w rotation)
    and the camera centre, as a float64 [4,4]."""
    c2w = np.eye(4)
    c2w[:3, :3] = cam.world_view_transform[:3, :3].detach().cpu().numpy()
    c2w[:3, 3] = cam.camera_center.detach().cpu().numpy()
    return c2w


def c2w_to_cam(ref_cam, c2w):
    """scene/cameras.py:99-120: a MiniCam with ref_cam's image size, field of view and clip planes at the pose c2w (float64
    [4,4]); the matrices are float32 on ref_cam's device, rounded where the reference rounds (on assignment)."""
    device = ref_cam.world_view_transform.device
    c2w = torch.as_tensor(np.asarray(c2w, dtype=np.float64))
    rot, trans = c2w[:3, :3], c2w[:3, 3]
    wv = torch.eye(4)
    wv[:3, :3] = rot
    wv[3, :3] = -trans @ rot
    wv = wv.to(device)
    proj = get_projection_matrix(znear=ref_cam.znear, zfar=ref_cam.zfar, fovX=ref_cam.FoVx, fovY=ref_cam.FoVy) \
        .transpose(0, 1).to(device)
    cam = MiniCam(ref_cam.image_width, ref_cam.image_height, ref_cam.FoVy, ref_cam.FoVx, ref_cam.znear, ref_cam.zfar, wv,
                  wv @ proj)
    cam.projection_matrix = proj
    return cam


def center_crop_window(H, W, ratio):
    """(h1, h2, w1, w2) of center_crop_with_ratio (utils/export_utils.py:161-191): x[h1:h2, w1:w2], its int() arithmetic."""
    ch, cw = H / 2, W / 2
    lh, lw = H * ratio, W * ratio
    return int(ch - lh / 2), int(ch + lh / 2), int(cw - lw / 2), int(cw + lw / 2)


def center_depth(depth):
    """The mean of the centre half of a depth render [1,H,W] (utils/export_utils.py:123-124), a device scalar."""
    _, H, W = depth.shape
    return depth[:, H // 4:H * 3 // 4, W // 4:W * 3 // 4].mean()


@torch.no_grad()
def spiral_path(motion, cloud, spin_angle=5.0, n_frames=50, spin_for=2, lookat_depth=None):
    """get_render_path (utils/export_utils.py:86-152): n_frames * spin_for MiniCams on a widening circle around the mean of
    the trajectories' middle cameras, all looking at one point on the mean camera's axis, spin_angle degrees off it at the
    widest.  The distance of that point is the mean depth of the centre half of the mean camera's render -- ONE render()
    and one host read while the path is built; lookat_depth (a number) overrides it and needs no device."""
    angle = spin_angle * np.pi / 180.0
    cameras = motion.get_middle_cams()
    ref = cameras[0]
    pivot = mean_camera_pose(np.stack([cam_to_c2w(c) for c in cameras]))
    up, eye = pivot[:3, 1], pivot[:3, 3]
    if lookat_depth is None:
        pivot_cam = c2w_to_cam(ref, pivot)
        bg = torch.zeros(3, device=pivot_cam.world_view_transform.device)
        lookat_depth = center_depth(gaussian_renderer.render(pivot_cam, cloud, bg)["depth"]).cpu().numpy()
    lookat = eye + lookat_depth * pivot[:3, 2]
    n = n_frames * spin_for
    widest = math.tan(angle) * np.linalg.norm(eye - lookat)
    radius = np.linspace(widest / spin_for, widest, n)
    turn = np.linspace(0.0, 2.0 * np.pi, n_frames)
    local = np.stack([np.tile(np.cos(turn), spin_for) * radius, np.tile(np.sin(turn), spin_for) * radius, np.zeros(n),
                      np.ones(n)], axis=0)
    eyes = (pivot @ local).T[:, :3]
    return [c2w_to_cam(ref, c2w_from_eye(e, lookat, up)) for e in eyes]


# ------------------------------------------------------------------------------------------------- jet_r
# The published segment definition of the "jet" colour map: per channel the nodes (x, value below, value above).
_JET_SEGMENTS = {
    "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
_jet_r_cache = {}


def _segment_channel(nodes, N=256):
    """N samples of a piecewise-linear channel, evaluated the way a segmented colour map fills its table (node positions
    scaled to the table first, the two end entries taken from the end nodes), so that every entry rounds as matplotlib's."""
    a = np.array(nodes, dtype=np.float64)
    x, below, above = a[:, 0] * (N - 1), a[:, 1], a[:, 2]
    at = (N - 1) * np.linspace(0.0, 1.0, N)
    seg = np.searchsorted(x, at)[1:-1]
    frac = (at[1:-1] - x[seg - 1]) / (x[seg] - x[seg - 1])
    inner = frac * (below[seg] - above[seg - 1]) + above[seg - 1]
    return np.clip(np.concatenate([[above[0]], inner, [below[-1]]]), 0.0, 1.0)


def jet_r_table():
    """uint8 [256,4]: (jet_r(i) * 255).astype(uint8) for the 256 table entries -- the reversed map is built from the
    reversed NODES (x -> 1 - x, sides swapped), as a segmented map reverses itself; flipping jet's table differs in one
    entry.  Entry 0 is (127, 0, 0, 255), entry 255 (0, 0, 127, 255)."""
    lut = np.ones((256, 4))
    for c, name in enumerate(("red", "green", "blue")):
        lut[:, c] = _segment_channel([(1.0 - x, hi, lo) for x, lo, hi in reversed(_JET_SEGMENTS[name])])
    return (lut * 255).astype(np.uint8)


def _jet_r_device(device):
    key = str(device)
    if key not in _jet_r_cache:
        _jet_r_cache[key] = torch.from_numpy(jet_r_table()).to(device).contiguous()
    return _jet_r_cache[key]


# ------------------------------------------------------------------------------------------------- the three kernels
def _tone_args(tone_mapping):
    if tone_mapping is None or isinstance(tone_mapping, str):
        tone_mapping = losses.ToneMapping(tone_mapping or "identity")
    kind = tone_mapping.tone_mapping_type
    if kind in ("identity", "reverse_identity"):
        return _lib.TONE_IDENTITY, 0.0, 0.0
    if kind == "gamma":
        return _lib.TONE_GAMMA, float(tone_mapping.eps), float(tone_mapping.bound)
    raise NotImplementedError(f"frames are finished with the identity and gamma tone mappings (got {kind!r})")


def _need_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} needs a tensor on a HIP device (no CPU fallback)")


def frames_finish(color, tone_mapping=None, window=None, out=None):
    """color [K,3,H,W] fp32 on the device -> uint8 [K,h,w,3] on the device (dgs_frames_finish).  window: (h1, h2, w1, w2) as
    center_crop_window returns it (None: the whole image); out: where to write (uint8, K h w 3 bytes, any alignment)."""
    _need_device(color, "frames_finish")
    if color.dim() != 4 or color.shape[1] != 3 or color.dtype != torch.float32:
        raise ValueError("frames_finish takes a float32 [K,3,H,W] tensor")
    color = color.contiguous()
    K, _, H, W = (int(s) for s in color.shape)
    h1, h2, w1, w2 = (0, H, 0, W) if window is None else (int(v) for v in window)
    tone, eps, bound = _tone_args(tone_mapping)
    if out is None:
        out = torch.empty((K, max(h2 - h1, 0), max(w2 - w1, 0), 3), dtype=torch.uint8, device=color.device)
    elif out.dtype != torch.uint8 or out.numel() != K * (h2 - h1) * (w2 - w1) * 3 or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of K h w 3 bytes")
    _lib.check(_lib.lib().dgs_frames_finish(_ptr(color), K, H, W, tone, eps, bound, h1, w1, h2 - h1, w2 - w1, _ptr(out),
                                            _stream(color.device)), "dgs_frames_finish")
    return out


def depth_range(depth):
    """(min, max) of a float32 device tensor as a device tensor [2] (dgs_depth_range): no host read.  NaNs do not count."""
    _need_device(depth, "depth_range")
    depth = depth.contiguous()
    L = _lib.lib()
    n = depth.numel()
    lo_hi = torch.empty(2, dtype=torch.float32, device=depth.device)
    tmp = torch.empty(max(L.dgs_depth_range_tmp_bytes(n), 8), dtype=torch.uint8, device=depth.device)
    _lib.check(L.dgs_depth_range(_ptr(depth), n, _ptr(lo_hi), _ptr(tmp), _stream(depth.device)), "dgs_depth_range")
    return lo_hi


def depth_colorize(depths, z_near=0.01, z_far=100.0, clip_percentage=1.0, lo_hi=None, out=None):
    """utils/export_utils.py:44-65 on the device: depths [...] fp32 -> uint8 [...,4] RGBA (a device tensor; the reference
    returns the same bytes as a numpy array).  The range is taken over all of `depths` (lo_hi: a device [2] to use
    instead).  Only the reference's default clip_percentage = 1 is implemented (anything else needs a sort)."""
    if clip_percentage != 1.0:
        raise NotImplementedError("depth_colorize implements clip_percentage = 1.0, the reference's default")
    _need_device(depths, "depth_colorize")
    depths = depths.contiguous()
    if lo_hi is None:
        lo_hi = depth_range(depths)
    if out is None:
        out = torch.empty(tuple(depths.shape) + (4,), dtype=torch.uint8, device=depths.device)
    _lib.check(_lib.lib().dgs_depth_colorize(_ptr(depths), depths.numel(), _ptr(lo_hi), float(z_near), float(z_far),
                                             _ptr(_jet_r_device(depths.device)), _ptr(out), _stream(depths.device)),
               "dgs_depth_colorize")
    return out


# ------------------------------------------------------------------------------------------------- K cameras per call
def frame_groups(cams, frames_per_call):
    """[(begin, end)] over the camera list: consecutive runs of at most min(frames_per_call, DGS_MAX_K) cameras that share
    image size and field of view (one rasteriser call has one of each).  A pure function of the cameras' attributes."""
    per_call = int(frames_per_call)
    if per_call < 1:
        raise ValueError("frames_per_call must be at least 1")
    per_call = min(per_call, _lib.DGS_MAX_K)
    key = lambda c: (int(c.image_width), int(c.image_height), float(c.FoVx), float(c.FoVy))
    groups, begin = [], 0
    for i in range(1, len(cams) + 1):
        if i == len(cams) or i - begin == per_call or key(cams[i]) != key(cams[begin]):
            groups.append((begin, i))
            begin = i
    return groups


def render_group(cams, cloud, bg):
    """One forward-only rasteriser call for cameras of one image size and field of view: the render_subframes dict
    (render [K,3,H,W], depth [K,1,H,W], ...).  Slot i is what render(cams[i]) returns, bit for bit."""
    with torch.no_grad():
        wv = torch.stack([c.world_view_transform for c in cams]).float().contiguous()
        fp = torch.stack([c.full_proj_transform for c in cams]).float().contiguous()
        cc = torch.stack([c.camera_center for c in cams]).float().contiguous()
        return gaussian_renderer.render_subframes(wv, fp, cc, cams[0], cloud, bg)


_PathPlan = collections.namedtuple("_PathPlan", "cams groups H W window h w device G")


def _path_plan(cams, crop_ratio, frames_per_call, who):
    """What every loop over a camera path starts from: the cameras as a list, their frame_groups, the one image size H, W
    they share, the crop window and its size h, w, their device, and G, the cameras of the largest group.  who: the
    caller's name for the messages."""
    cams = list(cams)
    if not cams:
        raise ValueError("no cameras")
    groups = frame_groups(cams, FRAMES_PER_CALL if frames_per_call is None else frames_per_call)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cams):
        raise ValueError(f"{who} makes one array, one directory or one video: the cameras must share one image size")
    window = center_crop_window(H, W, crop_ratio)
    h, w = window[1] - window[0], window[3] - window[2]
    if h < 1 or w < 1:
        raise ValueError(f"crop_ratio {crop_ratio} leaves no pixel of a {W} x {H} image")
    device = cams[0].world_view_transform.device
    if device.type != "cuda":
        raise RuntimeError(f"{who} needs cameras and a cloud on a HIP device (no CPU fallback)")
    return _PathPlan(cams, groups, H, W, window, h, w, device, max(e - b for b, e in groups))


class _HostRing:
    """Two pinned host buffers and their events: group g's bytes are copied into buffer g % 2 on the rendering stream,
    and drained into the result while group g + 1 is enqueued."""

    def __init__(self, shape, result):
        self.buf = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.event = [torch.cuda.Event() for _ in range(2)]
        self.pending = None
        self.result = result
        self.g = 0

    def push(self, dev_frames, begin, end):
        i = self.g % 2
        self.buf[i][:end - begin].copy_(dev_frames, non_blocking=True)
        self.event[i].record()
        self.drain()
        self.pending = (i, begin, end)
        self.g += 1

    def drain(self):
        if self.pending is not None:
            i, begin, end = self.pending
            self.event[i].synchronize()
            self.result[begin:end] = self.buf[i][:end - begin].numpy()
            self.pending = None


@torch.no_grad()
def render_frames(cams, cloud, bg, tone_mapping=None, crop_ratio=1.0, frames_per_call=None, depth=False):
    """The frames of a camera path: uint8 [n,h,w,3] (numpy), the centre crop of ratio crop_ratio of
    (tone_map(render).clip(0, 1) * 255).astype(uint8) -- and with depth=True also uint8 [n,H,W,4], depth_colorize of the
    path's depth images (uncropped, the range taken over the WHOLE path, as the reference's one batched call takes it:
    the depth images stay on the device, 4 H W bytes per frame, until the last group is rendered, and are coloured in a
    second pass).  Cameras are rendered frames_per_call at a time (default FRAMES_PER_CALL); the result does not depend on
    it.  All cameras must share one image size (the result is one array); fields of view may differ."""
    cams, groups, H, W, window, h, w, device, G = _path_plan(cams, crop_ratio, frames_per_call, "render_frames")
    n = len(cams)
    frames = np.empty((n, h, w, 3), dtype=np.uint8)
    ring = _HostRing((G, h, w, 3), frames)
    depths = torch.empty((n, H, W), dtype=torch.float32, device=device) if depth else None
    for b, e in groups:
        pkg = render_group(cams[b:e], cloud, bg)
        ring.push(frames_finish(pkg["render"], tone_mapping, window), b, e)
        if depth:
            depths[b:e].copy_(pkg["depth"][:, 0])
    ring.drain()
    if not depth:
        return frames
    colours = np.empty((n, H, W, 4), dtype=np.uint8)
    ring = _HostRing((G, H, W, 4), colours)
    lo_hi = depth_range(depths)
    for b, e in groups:
        ring.push(depth_colorize(depths[b:e], cloud.z_near, cloud.z_far, lo_hi=lo_hi), b, e)
    ring.drain()
    return frames, colours


# ------------------------------------------------------------------------------------------------- the two programs
def render_spiral(motion, cloud, bg, tone_mapping=None, spin_angle=5.0, n_frames=50, spin_for=2, crop_ratio=1.0,
                  frames_per_call=None, depth=False, writer=None, path=None, fps=32):
    """render_spiral.py:23-35: the frames of spiral_path(motion, cloud, ...) -- what render_frames returns.  writer: a
    callable writer(frames, path, fps) that encodes them (the reference's make_video; deblurgs_amd.video.make_video
    writes a Motion-JPEG AVI).  writer=None writes nothing."""
    cams = spiral_path(motion, cloud, spin_angle=spin_angle, n_frames=n_frames, spin_for=spin_for)
    out = render_frames(cams, cloud, bg, tone_mapping, crop_ratio=crop_ratio, frames_per_call=frames_per_call, depth=depth)
    if writer is not None:
        writer(out[0] if depth else out, path, fps)
    return out


def render_trainview(motion, cloud, bg, tone_mapping=None, gt_images=None, start_index=0, length=200, crop_ratio=0.95,
                     frames_per_call=None, writer=None, directory=None, fps=10):
    """render_trainview.py:23-52: the middle cameras start_index .. start_index + length (inclusive, as the reference
    counts) rendered, beside their ground-truth images (default: motion.gt_images) -- returns (imgs, gts, side_by_side),
    uint8 [m,h,w,3] twice and [m,h,2w,3], all centre-cropped by crop_ratio.  writer(frames, path, fps) is called for the
    three of them under `directory` with the reference's file names."""
    cams = motion.get_middle_cams()
    idx = [i for i in range(len(cams)) if start_index <= i <= start_index + length]
    if not idx:
        raise ValueError("start_index selects no training view")
    gt_images = motion.gt_images if gt_images is None else gt_images
    imgs = render_frames([cams[i] for i in idx], cloud, bg, tone_mapping, crop_ratio=crop_ratio,
                         frames_per_call=frames_per_call)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    window = center_crop_window(H, W, crop_ratio)
    device = cams[0].world_view_transform.device
    with torch.no_grad():
        gt = torch.stack([gt_images[i] for i in idx]).to(device=device, dtype=torch.float32)
        gts = frames_finish(gt, None, window).cpu().numpy()
    both = np.concatenate([gts, imgs], axis=2)
    if writer is not None:
        for frames, name in ((imgs, "render_trainview_img.mp4"), (gts, "render_trainview_gt.mp4"),
                             (both, "render_trainview_all.mp4")):
            writer(frames, os.path.join(directory or ".", name), fps)
    return imgs, gts, both


def _path_files(plan, cloud, bg, tone_mapping, encode, sink, capacity):
    """A camera path made into files on the device, in three stages that overlap -- the three steps of a
    device_files.Download, group g in slot g % 2: while group g is rendered, encoded and its sizes copied, the files of
    group g - 2 go to the sink, then the bytes of group g - 1 are copied (that many bytes, not the slots).  plan: a
    _path_plan; encode(uint8 frames [K,h,w,3] on the device) -> (files, sizes) on the device; sink(begin, blobs) takes the
    finished files of the cameras begin, begin + 1, ...; capacity: the bytes a slot's host buffer starts with."""
    slots = [device_files.Download(capacity) for _ in range(2)]
    groups, last = plan.groups, len(plan.groups) - 1
    for g, (b, e) in enumerate(groups):
        color = render_group(plan.cams[b:e], cloud, bg)["render"]
        slots[g % 2].read_sizes(*encode(frames_finish(color, tone_mapping, plan.window)))
        if g >= 2:
            sink(groups[g - 2][0], slots[g % 2].blobs())
        if g >= 1:
            slots[(g - 1) % 2].copy_bytes()
    slots[last % 2].copy_bytes()
    for g in range(max(last - 1, 0), last + 1):
        sink(groups[g][0], slots[g % 2].blobs())


@torch.no_grad()
def write_frames_png(cams, cloud, bg, directory, tone_mapping=None, crop_ratio=1.0, frames_per_call=None):
    """render_frames' loop with the files made on the device: per group of cameras frames_finish -> png.encode, and what
    crosses to the host is sizes[i] bytes of finished file per frame (_path_files), written as directory/00000.png ... (the
    names write_frames gives).  The pixels are render_frames'; returns the paths."""
    from . import png
    plan = _path_plan(cams, crop_ratio, frames_per_call, "write_frames_png")
    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(directory, f"{i:05d}.png") for i in range(len(plan.cams))]

    def sink(begin, blobs):
        for path, data in zip(paths[begin:], blobs):
            with open(path, "wb") as f:
                f.write(data)

    # (a host buffer of the largest group's bound never grows)
    _path_files(plan, cloud, bg, tone_mapping, png.encode, sink, plan.G * png.bound(plan.w, plan.h, 3))
    return paths


@torch.no_grad()
def write_frames_video(cams, cloud, bg, path, fps, tone_mapping=None, crop_ratio=1.0, frames_per_call=None, quality=90,
                       subsampling="4:2:0"):
    """The same loop with the frames made into JPEG files on the device (deblurgs_amd/jpeg.py) and appended to ONE
    Motion-JPEG AVI (deblurgs_amd/video.py).  The frames are jpeg.to_bytes(render_frames(...)) byte for byte; returns the
    path."""
    from . import jpeg, video
    plan = _path_plan(cams, crop_ratio, frames_per_call, "write_frames_video")
    with video.MjpegAviWriter(path, fps, quality, subsampling) as out:
        def sink(begin, blobs):
            for data in blobs:
                out.add(data, (plan.w, plan.h))

        _path_files(plan, cloud, bg, tone_mapping, lambda frames: jpeg.encode(frames, quality, subsampling), sink,
                    video.HOST_BYTES)
    return path


def write_frames(frames, directory):
    """uint8 [n,h,w,3 or 4] -> directory/00000.png ... through PIL when it is importable, else directory/frames.npy.
    Returns the paths written."""
    os.makedirs(directory, exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        path = os.path.join(directory, "frames.npy")
        np.save(path, np.asarray(frames))
        return [path]
    paths = []
    for i, f in enumerate(frames):
        paths.append(os.path.join(directory, f"{i:05d}.png"))
        Image.fromarray(np.ascontiguousarray(f)).save(paths[-1])
    return paths

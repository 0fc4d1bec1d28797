"""The training-progress visualiser on the device: the reference's Visualizer.__init__ / run / save_video
(utils/visualization.py:24-135, 191-259, 296-309), which train.py:221-222 calls after every iteration and which fires
n_visualize_shots = 200 times per training.

    draw(img_u8, prims)        dgs_draw_prims: int32 [n,6] records (x0, y0, x1, y1, r, rgb) -- one-pixel lines, filled discs
                               -- painted into a uint8 [H,W,3] device image in painter's order (csrc/draw.hip).
    vis_iterations             _get_vis_iteration: the iterations a shot is taken at.
    view_colours               the per-view cone colours, (0,255,255) ... (255,255,0).
    overview_camera            _get_visualization_camera: the zoomed-out camera that sees every training camera; float64
                               numpy on the host, at init time only.
    camera_overlay             render_gaussian_and_cams: one forward-only render, render_path.frames_finish, then every
                               view's sampled subframe cameras as cones -- dgs_cone_segments makes the line records,
                               ONE draw() paints them.  No host read.
    alignment_prims / alignment_plot   visualize_alignment: the learned subframe alignment nu of up to nine views, as this
                               project's own plot (not matplotlib's pixels), built with torch operations on the device and
                               painted by the same draw().
    ProgressVisualizer         the driver: __init__, run(iteration), save_video().  Both images of a shot become .jpg
                               files on the device (jpeg.encode); the same bytes are the frames of two Motion-JPEG AVIs
                               (video.MjpegAviWriter), so nothing is read back from disk.  Finished files are the only
                               bytes that cross to the host.

Deviations from the reference (INTEGRATION.md has the list): lines are walked unclipped and their outside pixels dropped,
where cv2 clips the endpoints first; the alignment plot is not matplotlib's rendering; videos are AVI, vis_traj files
.jpg; overview_camera returns the camera of the smallest zoom that PASSED the test (the reference returns the last one
it tried, passed or not).  Needs no cv2, matplotlib, torchvision or imageio.
"""
import math
import os

import numpy as np
import torch

from . import _lib, device_files, gaussian_renderer, jpeg, render_path, report, video
from .pose import MiniCam
from .raster_call import _ptr, _stream
from .render_path import _need_device

PANELS = 9
BLUE, RED, BLACK = 31 | 119 << 8 | 180 << 16, 255, 0       # R | G << 8 | B << 16
BLUE_RADIUS, RED_RADIUS = 2, 3
_owner_cache = {}
_colour_cache = {}


# ------------------------------------------------------------------------------------------------- drawing
def draw(img_u8, prims):
    """Paints prims, int32 [n,6] = (x0, y0, x1, y1, r, rgb) on the device, into img_u8, uint8 [H,W,3] on the device, in
    place (dgs_draw_prims; include/dgs_hip.h has the rule of every record).  The owner scratch is allocated once per
    device and reused (it grows with the largest image seen).  Returns img_u8."""
    _need_device(img_u8, "draw")
    _need_device(prims, "draw")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3 or not img_u8.is_contiguous():
        raise ValueError("draw takes a contiguous uint8 [H,W,3] image")
    if prims.dtype != torch.int32 or prims.dim() != 2 or prims.shape[1] != 6:
        raise ValueError("draw takes int32 [n,6] records")
    if prims.shape[0] == 0:             # (an empty tensor has no address to hand over)
        return img_u8
    prims = prims.contiguous()
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    key = str(img_u8.device)
    owner = _owner_cache.get(key)
    if owner is None or owner.numel() < H * W:
        owner = _owner_cache[key] = torch.empty(H * W, dtype=torch.int32, device=img_u8.device)
    _lib.check(_lib.lib().dgs_draw_prims(_ptr(img_u8), W, H, _ptr(prims), int(prims.shape[0]), _ptr(owner),
                                         _stream(img_u8.device)), "dgs_draw_prims")
    return img_u8


def vis_iterations(n_iters, n_shots=200, alpha=1.7):
    """_get_vis_iteration (utils/visualization.py:76-81), the same numpy expression: shot k of n_shots is taken at
    int(n_iters (k / n_shots)^alpha)."""
    a = n_iters / n_shots ** (alpha)
    return (a * (np.arange(1, n_shots + 1).astype(float)) ** alpha).astype(int)


def view_colours(n):
    """uint8 [n,3], RGB: ((1 - t) (0,255,255) + t (255,255,0)).astype(uint8) over t = linspace(0, 1, n)
    (utils/visualization.py:199-202).  The reference flips them to BGR for an image cv2.imwrite flips back: on an RGB frame
    they are RGB."""
    t = np.linspace(0, 1, n)[:, None]
    return ((1 - t) * np.array([0, 255, 255]) + t * np.array([255, 255, 0])).astype(np.uint8)


def pack_rgb(colours):
    """uint8 [...,3] -> int32 [...]: R | G << 8 | B << 16, the colour word of a record."""
    c = np.asarray(colours).astype(np.int32)
    return c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16


# ------------------------------------------------------------------------------------------------- the overview camera
def _shell(ref, device):
    """A camera that only carries ref's image size, field of view and clip planes to render_path.c2w_to_cam."""
    return MiniCam(ref.image_width, ref.image_height, ref.FoVy, ref.FoVx, ref.znear, ref.zfar,
                   torch.eye(4, device=device), torch.eye(4, device=device), torch.zeros(3, device=device))


def zoomed_c2w(mean_c2w, lookat, zoom):
    """The pose at lookat + zoom (eye - lookat), looking at lookat, with the mean pose's up axis
    (utils/visualization.py:105-108)."""
    eye, up = mean_c2w[:3, 3], mean_c2w[:3, 1]
    return render_path.c2w_from_eye(lookat + zoom * (eye - lookat), lookat, up)


def centres_good(pts, cam, threshold=0.5):
    """bool [n]: which of the points [n,3] the camera has at depth >= 0.1 and inside the image widened by `threshold` of
    its size on every side (utils/visualization.py:112-125).  cam: host tensors."""
    W, H = cam.image_width, cam.image_height
    pts_hom = np.pad(np.asarray(pts, dtype=np.float64), ((0, 0), (0, 1)), "constant", constant_values=1.0)
    pts_cam_hom = pts_hom @ cam.world_view_transform.cpu().numpy()
    pts_cam = pts_cam_hom[:, :3] / pts_cam_hom[:, 3:]
    in_front = pts_cam[:, 2] >= 0.1
    pts_ndc_hom = pts_hom @ cam.full_proj_transform.cpu().numpy()
    pts_ndc = pts_ndc_hom[:, :3] / pts_ndc_hom[:, 3:]
    pix = ((pts_ndc[:, :2] + 1.0) * np.array([W, H]).astype(float) - 1.0) * 0.5
    inside = np.logical_and(np.logical_and(pix[:, 0] >= -threshold * W, pix[:, 0] <= (1.0 + threshold) * W),
                            np.logical_and(pix[:, 1] >= -threshold * H, pix[:, 1] <= (1.0 + threshold) * H))
    return np.logical_and(inside, in_front)


def overview_zoom(c2ws, lookat, ref, threshold=0.5):
    """(zoom, c2w): the reference's bisection over zoom in [1.5, 100] down to a bracket of 1e-3 for the lowest zoom at which
    a camera on the line from `lookat` through the mean pose's centre sees every camera centre (centres_good).  Host only:
    c2ws float64 [n,4,4], lookat [3], ref anything with image_width, image_height, FoVx, FoVy, znear, zfar.  Returns the
    upper end of the bracket -- the smallest zoom that passed, 100 if none did."""
    c2ws = np.asarray(c2ws, dtype=np.float64)
    lookat = np.asarray(lookat, dtype=np.float64)
    pts = c2ws[:, :3, 3]
    mean_c2w = render_path.mean_camera_pose(c2ws)
    host = _shell(ref, "cpu")
    lb, ub = 1.5, 100.0
    while ub - lb >= 1e-3:
        zoom = (lb + ub) / 2.0
        if centres_good(pts, render_path.c2w_to_cam(host, zoomed_c2w(mean_c2w, lookat, zoom)), threshold).all():
            ub = zoom
        else:
            lb = zoom
    return ub, zoomed_c2w(mean_c2w, lookat, ub)


@torch.no_grad()
def overview_camera(motion, cloud, threshold=0.5, vis_cam_idx=None):
    """_get_visualization_camera (utils/visualization.py:83-132): a MiniCam on the device.  The training cameras are the
    middle cameras of motion's trajectories, the look-at point the cloud's mean.  Init-time only: one host read of the
    cameras' rotations and centres, one of the cloud's mean; the search itself is overview_zoom's, on the host.
    vis_cam_idx: that view's first subframe camera instead (the caller then draws no cones)."""
    device = cloud._xyz.device
    if device.type != "cuda":
        raise RuntimeError("overview_camera needs a motion module and a cloud on a HIP device (no CPU fallback)")
    if vis_cam_idx is not None:
        nu = motion._sample_nu_from_alignment(vis_cam_idx)
        return motion.get_trajectory(vis_cam_idx, nu[torch.linspace(0, nu.shape[0] - 1, 1, device=nu.device).long()])[0]
    cams = motion.get_middle_cams()
    packed = torch.stack([torch.cat([c.world_view_transform[:3, :3].reshape(9), c.camera_center.reshape(3)])
                          for c in cams]).cpu().numpy()
    c2ws = np.tile(np.eye(4), (len(cams), 1, 1))
    c2ws[:, :3, :3] = packed[:, :9].reshape(-1, 3, 3)
    c2ws[:, :3, 3] = packed[:, 9:]
    lookat = cloud._xyz.detach().mean(dim=0).cpu().numpy()
    _, c2w = overview_zoom(c2ws, lookat, motion.ref_cam, threshold)
    return render_path.c2w_to_cam(_shell(motion.ref_cam, device), c2w)


# ------------------------------------------------------------------------------------------------- cones on a render
def cone_segments(view, campos, tanx, tany, scale, render_view, render_proj, W, H, rgb, out=None):
    """dgs_cone_segments: view float32 [C,4,4], campos float32 [C,3], render_view / render_proj float32 [4,4], rgb int32
    [C], all on the device -> int32 [8 C, 6] line records (r = -1 where the reference draws nothing)."""
    _need_device(view, "cone_segments")
    C = int(view.shape[0])
    f32 = lambda t: t.detach().to(dtype=torch.float32).contiguous()
    view, campos, render_view, render_proj = f32(view), f32(campos), f32(render_view), f32(render_proj)
    if view.numel() != 16 * C or campos.numel() != 3 * C or render_view.numel() != 16 or render_proj.numel() != 16:
        raise ValueError("cone_segments takes view [C,4,4], campos [C,3] and two [4,4] matrices")
    if rgb.dtype != torch.int32 or rgb.numel() != C:
        raise ValueError("cone_segments takes one int32 colour per camera")
    if out is None:
        out = torch.empty((8 * C, 6), dtype=torch.int32, device=view.device)
    elif out.dtype != torch.int32 or out.numel() != 48 * C or not out.is_contiguous():
        raise ValueError("out must be a contiguous int32 [8 C, 6] tensor")
    _lib.check(_lib.lib().dgs_cone_segments(C, _ptr(view), _ptr(campos), float(tanx), float(tany), float(scale),
                                            _ptr(render_view), _ptr(render_proj), int(W), int(H), _ptr(rgb.contiguous()),
                                            _ptr(out), _stream(view.device)), "dgs_cone_segments")
    return out


def _view_colour_words(n, per_view, device):
    key = (n, per_view, str(device))
    if key not in _colour_cache:
        _colour_cache[key] = torch.from_numpy(np.repeat(pack_rgb(view_colours(n)), per_view)).to(device)
    return _colour_cache[key]


@torch.no_grad()
def overlay_prims(motion, cam, scale=0.5, subframes_per_view=5):
    """The line records camera_overlay paints: for every view i, in list order, the cones of the subframe cameras at
    nu[linspace(0, f - 1, subframes_per_view).long()] (sample_subframe_cams), 8 records per camera, in view i's colour.
    One dgs_cone_segments call over all of them; int32 [8 n subframes_per_view, 6] on the device."""
    views, centres = [], []
    for i in range(len(motion)):
        nu = motion._sample_nu_from_alignment(i)
        pick = torch.linspace(0, nu.shape[0] - 1, subframes_per_view, device=nu.device).long()
        wv, _, cc = motion.get_trajectory_matrices(i, nu[pick])
        views.append(wv)
        centres.append(cc)
    ref = motion.ref_cam
    rgb = _view_colour_words(len(motion), subframes_per_view, views[0].device)
    return cone_segments(torch.cat(views), torch.cat(centres), math.tan(ref.FoVx / 2), math.tan(ref.FoVy / 2), scale,
                         cam.world_view_transform, cam.full_proj_transform, int(cam.image_width), int(cam.image_height), rgb)


@torch.no_grad()
def camera_overlay(motion, cloud, cam, bg, tone_mapping=None, scale=0.5, subframes_per_view=5, cones=True):
    """render_gaussian_and_cams (utils/visualization.py:191-208) without its file: uint8 [H,W,3] on the device, the cloud
    rendered from `cam` (one forward-only call; frames_finish truncates as the reference's astype(uint8) does) with every
    view's sampled subframe cameras drawn as cones, later views over earlier ones as the reference's loop leaves them.
    cones=False: the render alone (the reference's vis_cam_idx case).  No host read."""
    _need_device(cloud._xyz, "camera_overlay")
    color = gaussian_renderer.render(cam, cloud, bg)["render"]
    img = render_path.frames_finish(color[None], tone_mapping)[0]
    if cones and len(motion) > 0:
        draw(img, overlay_prims(motion, cam, scale, subframes_per_view))
    return img


# ------------------------------------------------------------------------------------------------- the alignment plot
# Seven-segment digits: a (top), b (upper right), c (lower right), d (bottom), e (lower left), f (upper left), g (middle)
_SEGMENTS = {"0": "abcdef", "1": "bc", "2": "abged", "3": "abgcd", "4": "fgbc", "5": "afgcd", "6": "afgedc", "7": "abc",
             "8": "abcdefg", "9": "abcdfg"}
DIGIT_W, DIGIT_H, DIGIT_PITCH = 8, 14, 13
MARGIN_LEFT, MARGIN_RIGHT, MARGIN_TOP, MARGIN_BOTTOM, TICK = 40, 16, 30, 21, 5
X_SPAN, Y_SPAN = (-0.05, 1.05), (-0.1, 1.1)
TICKS = (0.0, 0.5, 1.0)


def panel_frame(p, size):
    """(X0, Y0, X1, Y1): the pixel frame of panel p (row p // 3, column p % 3) of an image of size = (H, W)."""
    H, W = size
    cw, ch = W // 3, H // 3
    row, col = p // 3, p % 3
    return col * cw + MARGIN_LEFT, row * ch + MARGIN_TOP, (col + 1) * cw - MARGIN_RIGHT, (row + 1) * ch - MARGIN_BOTTOM


def panel_static_records(p, index, size):
    """The records of panel p that do not depend on nu, as a list of 6-tuples: 4 frame lines, 3 + 3 tick marks (x below the
    frame, y left of it, at 0, 0.5 and 1), and 7 per decimal digit of `index` above the frame's left end (a segment that
    is off has r = -1)."""
    X0, Y0, X1, Y1 = panel_frame(p, size)
    out = [(X0, Y0, X1, Y0, 0, BLACK), (X1, Y0, X1, Y1, 0, BLACK), (X1, Y1, X0, Y1, 0, BLACK), (X0, Y1, X0, Y0, 0, BLACK)]
    for t in TICKS:
        x = int(math.floor(X0 + (t - X_SPAN[0]) / (X_SPAN[1] - X_SPAN[0]) * (X1 - X0) + 0.5))
        out.append((x, Y1, x, Y1 + TICK, 0, BLACK))
    for t in TICKS:
        y = int(math.floor(Y1 - (t - Y_SPAN[0]) / (Y_SPAN[1] - Y_SPAN[0]) * (Y1 - Y0) + 0.5))
        out.append((X0 - TICK, y, X0, y, 0, BLACK))
    for k, digit in enumerate(str(int(index))):
        x, y = X0 + 4 + k * DIGIT_PITCH, Y0 - MARGIN_TOP + 8
        xr, ym, yb = x + DIGIT_W, y + DIGIT_H // 2, y + DIGIT_H
        lines = {"a": (x, y, xr, y), "b": (xr, y, xr, ym), "c": (xr, ym, xr, yb), "d": (x, yb, xr, yb),
                 "e": (x, ym, x, yb), "f": (x, y, x, ym), "g": (x, ym, xr, ym)}
        for name in "abcdefg":
            out.append(lines[name] + (0 if name in _SEGMENTS[digit] else -1, BLACK))
    return out


def alignment_prim_count(motion, indices):
    """The number of records alignment_prims returns: per panel 10 + 7 per digit of its view index + K + (K - 2), K the
    subframes of a view."""
    K = int(motion._nu.shape[1]) + 2
    return sum(10 + 7 * len(str(int(i))) + K + (K - 2) for i in list(indices)[:PANELS])


def _disc_records(nu, frame, radius, rgb):
    """nu [m] on the device -> int32 [m,6] disc records at (nu_j, j / (m - 1)) in the panel's frame."""
    X0, Y0, X1, Y1 = frame
    m = int(nu.shape[0])
    x = nu.double()
    y = torch.linspace(0.0, 1.0, m, dtype=torch.float64, device=nu.device)
    px = torch.floor(X0 + (x - X_SPAN[0]) / (X_SPAN[1] - X_SPAN[0]) * (X1 - X0) + 0.5).to(torch.int32)
    py = torch.floor(Y1 - (y - Y_SPAN[0]) / (Y_SPAN[1] - Y_SPAN[0]) * (Y1 - Y0) + 0.5).to(torch.int32)
    return torch.stack([px, py, px, py, torch.full_like(px, radius), torch.full_like(px, rgb)], dim=1)


@torch.no_grad()
def alignment_prims(motion, indices, size=(1000, 1200)):
    """The records of the alignment plot of the views `indices` (the first nine), int32 [n,6] on the device, n =
    alignment_prim_count: per panel its static records, then a blue disc of radius 2 at (nu_k, k / (K - 1)) for the view's K
    sorted subframe times (_sample_nu_from_alignment) and, over them, a red disc of radius 3 at (pivot_j, j / (m - 1)) for
    its m = K - 2 sorted sigmoid(_nu[idx]) pivots.  x spans [-0.05, 1.05] (fixed: nu is a sigmoid), y [-0.1, 1.1], y up.
    Built with torch operations: nu is never read by the host."""
    _need_device(motion._nu, "alignment_prims")
    device = motion._nu.device
    parts = []
    for p, idx in enumerate(list(indices)[:PANELS]):
        idx = int(idx)
        frame = panel_frame(p, size)
        parts.append(torch.tensor(panel_static_records(p, idx, size), dtype=torch.int32).to(device, non_blocking=True))
        parts.append(_disc_records(motion._sample_nu_from_alignment(idx), frame, BLUE_RADIUS, BLUE))
        parts.append(_disc_records(torch.sigmoid(motion._nu[idx].sort().values), frame, RED_RADIUS, RED))
    return torch.cat(parts).contiguous()


@torch.no_grad()
def alignment_plot(motion, indices, size=(1000, 1200)):
    """visualize_alignment (utils/visualization.py:218-253) as this project's own plot: uint8 [H,W,3] on the device, white,
    min(9, len(indices)) panels in a 3 x 3 grid, each with a black frame, tick marks at 0, 0.5 and 1 on both axes, the
    view's index in seven-segment digits, blue discs for its subframe times and red ones for its pivots."""
    _need_device(motion._nu, "alignment_plot")
    img = torch.full((int(size[0]), int(size[1]), 3), 255, dtype=torch.uint8, device=motion._nu.device)
    return draw(img, alignment_prims(motion, indices, size))


# ------------------------------------------------------------------------------------------------- the driver
class ProgressVisualizer:
    """Visualizer (utils/visualization.py:24-74, 255-259, 296-309).  The caller invokes run(iteration) after every step,
    as train.py:221 does, and save_video() at the end.  vis_traj/IIIII.jpg and vis_alignment/IIIII.jpg under model_path
    (both directories removed and recreated), vis_traj.avi and vis_alignment.avi beside them."""

    def __init__(self, motion, cloud, bg, model_path, iterations, tone_mapping=None, n_visualize_shots=200, exponential=1.7,
                 vis_cam_idx=None, rng=None, fps=20, quality=90):
        _need_device(cloud._xyz, "ProgressVisualizer")
        self.motion, self.cloud, self.bg, self.tone_mapping = motion, cloud, bg, tone_mapping
        self.vis_iters = vis_iterations(iterations, n_visualize_shots, exponential)
        self._shots = set(int(i) for i in self.vis_iters)
        n = len(motion)
        self.selected_indice = (np.random if rng is None else rng).choice(np.arange(n), size=min(PANELS, n), replace=False)
        self.selected_indice.sort()
        self.draw_camera = vis_cam_idx is None
        self.ref_camera = overview_camera(motion, cloud, vis_cam_idx=vis_cam_idx)
        self.cam_scale = 0.5            # _get_camera_scale
        self.alignment_path = report.fresh_directory(os.path.join(model_path, "vis_alignment"))
        self.traj_vis_path = report.fresh_directory(os.path.join(model_path, "vis_traj"))
        self.writers = [video.MjpegAviWriter(os.path.join(model_path, "vis_traj.avi"), fps, quality),
                        video.MjpegAviWriter(os.path.join(model_path, "vis_alignment.avi"), fps, quality)]
        self._downloads = [device_files.Download(video.HOST_BYTES) for _ in self.writers]

    @torch.no_grad()
    def run(self, current_iter):
        """Nothing off vis_iterations; else the two images, one jpeg.encode each, the files and the frames.  Returns the two
        paths written (None off a shot)."""
        if int(current_iter) not in self._shots:
            return None
        images = [camera_overlay(self.motion, self.cloud, self.ref_camera, self.bg, self.tone_mapping, self.cam_scale,
                                 cones=self.draw_camera),
                  alignment_plot(self.motion, self.selected_indice)]
        for image, writer, slot in zip(images, self.writers, self._downloads):
            slot.read_sizes(*jpeg.encode(image[None], writer.quality, writer.subsampling))
        for slot in self._downloads:
            slot.copy_bytes()
        paths = []
        for image, writer, slot, directory in zip(images, self.writers, self._downloads,
                                                  (self.traj_vis_path, self.alignment_path)):
            data, = slot.blobs()
            paths.append(os.path.join(directory, f"{int(current_iter):05d}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(data)
            writer.add(data, (int(image.shape[1]), int(image.shape[0])))
        return paths

    def save_video(self):
        """Closes the two AVIs (the reference re-reads its image files here; these frames were appended as they were made).
        Returns their paths, vis_traj.avi first."""
        return [w.close() for w in self.writers]

"""Visual reports on the device: what the reference's drivers write for a person to look at.

    evaluate(vis_dir=...)   test.py:122-126              NNN_gt.png, NNN_render.png, NNN_error.png per test view
    traj_render             utils/visualization.py:262-291   per training view the blurred synthesis, the ground truth,
                                                         evenly spaced sharp subframes and the L1 error map
    colorize                utils/colorize.py:63-122     a scalar map -> jet colours, scaled by its (1, 100) percentiles
    depth_colorize          utils/export_utils.py:44-65  with clip_percentage < 1 (render_path.depth_colorize has = 1)

The reference gets there through .cpu(), np.percentile (a full sort), matplotlib and torchvision, per view.  Here the
images never leave the device until they are bytes:

    order_stats / percentiles   dgs_order_stats / dgs_percentiles: exact radix select, four 8-bit passes, no sort, no
                                host read; numpy's linear percentile of a float32 array bit for bit (float64 results)
    report_images               dgs_report_images: tone mapping, save_image's ROUNDED 8-bit conversion (dgs_frames_finish
                                truncates, as render_spiral does), the 8-bit ground truth and the L1 error map in one pass;
                                with mean=True the sequential fp32 mean of K subframes first
    colorize                    dgs_percentiles -> vmax += 1e-6 on the device words -> dgs_scalar_colorize

The jet table is built from the published segment definition (render_path._JET_SEGMENTS; matplotlib need not be
installed) and pinned by tests/golden/report_golden.npz.  PNG files are written through PIL when it is importable, else
.npy; every writer argument is a callable writer(path, array) that takes the place of the file.  device_png=True
(write_view_report, traj_render, evaluation.evaluate) compresses the files on the device instead (deblurgs_amd/png.py).

Out of scope: colorize with a mask or a colour bar (cv2, a matplotlib canvas).  (The camera-cone drawings, the alignment
plots and the visualiser's videos are deblurgs_amd/progress.py; LPIPS, the third number of evaluate(), is
deblurgs_amd/lpips.py: evaluate(..., lpips=weights).)
"""
import ctypes
import os
import shutil

import numpy as np
import torch

from . import _lib, gaussian_renderer, render_path
from .raster_call import _ptr, _stream
from .render_path import _need_device, _tone_args

TINY_NUMBER = 1e-6          # utils/colorize.py:10
_jet_cache = {}


# ------------------------------------------------------------------------------------------------- order statistics
def _flat_f32(x, what):
    _need_device(x, what)
    if x.dtype != torch.float32:
        raise ValueError(f"{what} takes a float32 tensor")
    return x.contiguous().reshape(-1)


def _select_tmp(L, n, m, device):
    return torch.empty(max(L.dgs_order_stats_tmp_bytes(n, m), 8), dtype=torch.uint8, device=device)


def order_stats(x, ranks):
    """np.sort(x.reshape(-1))[ranks] as a float32 device tensor [m] (dgs_order_stats): 1 <= m <= 4 host ranks, one data
    pass per radix digit for all of them, no host read.  NaNs sort last."""
    x = _flat_f32(x, "order_stats")
    L = _lib.lib()
    ranks = [int(r) for r in ranks]
    n, m = x.numel(), len(ranks)
    if any(r < 0 for r in ranks):
        raise ValueError("ranks must not be negative")
    out = torch.empty(m, dtype=torch.float32, device=x.device)
    tmp = _select_tmp(L, n, m, x.device)
    _lib.check(L.dgs_order_stats(_ptr(x), n, (ctypes.c_uint64 * max(m, 1))(*ranks), m, _ptr(out), _ptr(tmp),
                                 _stream(x.device)), "dgs_order_stats")
    return out


def percentiles(x, q):
    """np.percentile(x.reshape(-1), tuple(q)) as a float64 device tensor [m] (dgs_percentiles), 1 <= m <= 4, bit for bit
    what numpy 2 returns for a float32 array and a TUPLE of percentages (a scalar q makes numpy return float32)."""
    x = _flat_f32(x, "percentiles")
    L = _lib.lib()
    q = [float(v) for v in q]
    n, m = x.numel(), len(q)
    out = torch.empty(m, dtype=torch.float64, device=x.device)
    tmp = _select_tmp(L, n, m, x.device)
    _lib.check(L.dgs_percentiles(_ptr(x), n, (ctypes.c_double * max(m, 1))(*q), m, _ptr(out), _ptr(tmp),
                                 _stream(x.device)), "dgs_percentiles")
    return out


# ------------------------------------------------------------------------------------------------- colours
def jet_table(rounded):
    """uint8 [256,4]: the 256 RGBA entries of "jet" (NOT jet_r) from render_path._JET_SEGMENTS.  rounded: floor(c * 255 +
    0.5), what torchvision's save_image makes of the map's float colours (the reference saves colorize's floats);
    else (c * 255).astype(uint8), the truncation depth_colorize applies."""
    lut = np.ones((256, 4))
    for c, name in enumerate(("red", "green", "blue")):
        lut[:, c] = render_path._segment_channel(render_path._JET_SEGMENTS[name])
    return np.floor(lut * 255 + 0.5).astype(np.uint8) if rounded else (lut * 255).astype(np.uint8)


def _jet_device(device, rounded):
    key = (str(device), bool(rounded))
    if key not in _jet_cache:
        _jet_cache[key] = torch.from_numpy(jet_table(rounded)).to(device).contiguous()
    return _jet_cache[key]


def scalar_colorize(x, lo_hi, rounded=True, out=None):
    """x [...] float32 and its range lo_hi (two float64 device words) -> uint8 [...,3] jet colours (dgs_scalar_colorize)."""
    _need_device(x, "scalar_colorize")
    if x.dtype != torch.float32 or lo_hi.dtype != torch.float64 or lo_hi.numel() != 2:
        raise ValueError("scalar_colorize takes a float32 tensor and a float64 [2] range")
    x = x.contiguous()
    if out is None:
        out = torch.empty(tuple(x.shape) + (3,), dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.numel() != 3 * x.numel() or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of 3 bytes per value")
    _lib.check(_lib.lib().dgs_scalar_colorize(_ptr(x), x.numel(), _ptr(lo_hi.contiguous()),
                                              _ptr(_jet_device(x.device, rounded)), _ptr(out), _stream(x.device)),
               "dgs_scalar_colorize")
    return out


def colorize(x, cmap_name="jet", mask=None, range=None, append_cbar=False, rounded=True):
    """utils/colorize.py:63-122 on its default path: x [H,W] float32 on the device -> uint8 [H,W,3] on the device.  The
    range is np.percentile(x, (1, 100)) with vmax += 1e-6 (formed on the device words: no host read), the chain
    clip -> (x - vmin) / (vmax - vmin) -> table runs in float64, numpy 2's promotion of a float32 array against the two
    float64 scalars.  The reference returns float colours and saves them with save_image: rounded=True gives those bytes.
    range=(lo, hi): that range instead, through the same float64 chain (numpy keeps float32 against two PYTHON floats:
    there a value on the edge of a table entry may land on its neighbour).  mask and append_cbar need cv2 and a matplotlib
    canvas: NotImplementedError."""
    if mask is not None or append_cbar:
        raise NotImplementedError("colorize implements the reference's default path: no mask, no colour bar")
    if cmap_name != "jet":
        raise NotImplementedError(f"colorize carries the jet table only (got {cmap_name!r})")
    _need_device(x, "colorize")
    if range is None:
        lo_hi = percentiles(x, (1.0, 100.0))
        lo_hi[1:] += TINY_NUMBER
    else:
        lo_hi = torch.tensor([float(range[0]), float(range[1])], dtype=torch.float64, device=x.device)
    return scalar_colorize(x, lo_hi, rounded)


def clip_rank(n, clip_percentage):
    """The index depth_colorize reads of the sorted depths (utils/export_utils.py:57)."""
    return int((n - 1) * clip_percentage)


def depth_colorize(depths, z_near=0.01, z_far=100.0, clip_percentage=1.0, out=None):
    """utils/export_utils.py:44-65 for any clip_percentage: the upper end of the range is additionally capped by the order
    statistic at rank int((n - 1) * clip_percentage), taken with dgs_order_stats and combined with dgs_depth_range's words
    on the device; the colours are render_path.depth_colorize's (uint8 [...,4], jet_r)."""
    _need_device(depths, "depth_colorize")
    if not 0.0 <= clip_percentage <= 1.0:
        raise ValueError("clip_percentage must be in [0, 1]")
    depths = depths.contiguous()
    lo_hi = render_path.depth_range(depths)
    if clip_percentage != 1.0:
        cap = order_stats(depths, [clip_rank(depths.numel(), clip_percentage)])
        lo_hi[1:] = torch.minimum(lo_hi[1:], cap)
    return render_path.depth_colorize(depths, z_near, z_far, lo_hi=lo_hi, out=out)


# ------------------------------------------------------------------------------------------------- report images
def report_images(x, tone_mapping=None, mean=False, gt=None, want_gt_u8=True, want_err=True):
    """x [K,3,H,W] linear renders -> (out_u8 [G,H,W,3], gt_u8 [G,H,W,3] or None, err [G,H,W] or None), one
    dgs_report_images call.  mean: G = 1, the image is tone_map of the sequential fp32 mean of the K renders and gt is
    [3,H,W]; else G = K and gt is [K,3,H,W].  Bytes are save_image's (uint8)clamp(y * 255 + 0.5, 0, 255); err is
    torch.abs(gt - y).permute(1, 2, 0).mean(-1) with y unclamped.  gt None: subframes, bytes only."""
    _need_device(x, "report_images")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError("report_images takes a float32 [K,3,H,W] tensor")
    x = x.contiguous()
    K, _, H, W = (int(s) for s in x.shape)
    G = 1 if mean else K
    tone, eps, bound = _tone_args(tone_mapping)
    u8 = dict(dtype=torch.uint8, device=x.device)
    out = torch.empty((G, H, W, 3), **u8)
    gt_u8 = err = None
    if gt is not None:
        gt = gt.to(device=x.device, dtype=torch.float32).contiguous()
        if gt.numel() != G * 3 * H * W:
            raise ValueError(f"gt must hold {G} x 3 x {H} x {W} values")
        gt_u8 = torch.empty((G, H, W, 3), **u8) if want_gt_u8 else None
        err = torch.empty((G, H, W), dtype=torch.float32, device=x.device) if want_err else None
    _lib.check(_lib.lib().dgs_report_images(_ptr(x), K, 1 if mean else 0, H, W, tone, eps, bound,
                                            _ptr(gt) if gt is not None else None, _ptr(out),
                                            _ptr(gt_u8) if gt_u8 is not None else None,
                                            _ptr(err) if err is not None else None, _stream(x.device)),
               "dgs_report_images")
    return out, gt_u8, err


def view_report(render, gt, tone_mapping=None):
    """(render_u8, gt_u8, error_rgb_u8), uint8 [G,H,W,3] each on the device, for G views: render [G,3,H,W] linear, gt
    [G,3,H,W].  One dgs_report_images call, then a percentile and a colorize per view (every error map has its own
    range, as the reference's per-view colorize call gives it)."""
    out, gt_u8, err = report_images(render, tone_mapping, mean=False, gt=gt)
    colours = torch.empty_like(out)
    for g in range(out.shape[0]):
        lo_hi = percentiles(err[g], (1.0, 100.0))
        lo_hi[1:] += TINY_NUMBER
        scalar_colorize(err[g], lo_hi, True, out=colours[g])
    return out, gt_u8, colours


# ------------------------------------------------------------------------------------------------- files
def write_image(path, array, writer=None):
    """One uint8 [H,W,3] image to `path` (a .png name): writer(path, array) when given; else a PNG through PIL when it is
    importable, else path with .npy in place of .png (as render_path.write_frames falls back).  Returns the path written."""
    array = np.ascontiguousarray(array)
    if writer is not None:
        writer(path, array)
        return path
    try:
        from PIL import Image
    except ImportError:
        path = os.path.splitext(path)[0] + ".npy"
        np.save(path, array)
        return path
    Image.fromarray(array).save(path)
    return path


def fresh_directory(path):
    """Removed and recreated, as the reference's drivers prepare their output directories -- they join a name to the
    model's directory; here the caller gives the directory itself, so what can only be a mistake is refused: an empty
    path, the root, the home directory, the working directory or a directory above it."""
    if not path or not str(path).strip():
        raise ValueError("an output directory that is removed and recreated needs a name")
    full = os.path.abspath(path)
    cwd = os.path.abspath(os.getcwd())
    if full == os.path.abspath(os.path.expanduser("~")) or cwd == full or cwd.startswith(full.rstrip(os.sep) + os.sep):
        raise ValueError(f"refusing to remove and recreate {full!r}: it is the root, the home directory or holds the working "
                         "directory")
    shutil.rmtree(path, ignore_errors=True)
    os.makedirs(path)
    return path


def evaluate_names(i):
    """test.py:124-126: the (gt, render, error) file names of test view i."""
    return f"{i:03d}_gt.png", f"{i:03d}_render.png", f"{i:03d}_error.png"


def no_writer_with_device_png(writer, device_png):
    if device_png and writer is not None:
        raise ValueError("device_png writes the files itself: it cannot be combined with a writer")


def write_device_png(directory, names, images_u8):
    """images_u8 uint8 [n,H,W,3] on the device -> the n files directory/names[k], compressed on the device in ONE
    png.encode call (the host reads the sizes and copies that many bytes).  Returns the paths."""
    from . import png
    return png.write_files(images_u8, [os.path.join(directory, name) for name in names])


def write_view_report(directory, i, image, gt, writer=None, device_png=False):
    """The three files of test view i (test.py:122-126) from ONE view_report call: image [3,H,W] is the tone-mapped,
    unclamped render the metrics were taken of (so the bytes and the error are those of the reference's torch
    expression, no second tone mapping), gt [3,H,W].  device_png=True: the three images become files on the device (one
    n = 3 png.encode call) instead of crossing to PIL; same names, same pixels."""
    no_writer_with_device_png(writer, device_png)
    render_u8, gt_u8, error_u8 = view_report(image[None], gt[None], "identity")
    if device_png:
        return write_device_png(directory, evaluate_names(i), torch.stack([gt_u8[0], render_u8[0], error_u8[0]]))
    host = torch.stack([gt_u8[0], render_u8[0], error_u8[0]]).cpu().numpy()
    return [write_image(os.path.join(directory, name), host[k], writer) for k, name in enumerate(evaluate_names(i))]


def traj_render_directory(model_path, iteration):
    return f"{model_path}/traj_render_{iteration:05d}"


def traj_render_names(i, num_visualize_subframes):
    """utils/visualization.py:283-291: the file names of training view i -- the subframes, then blur, gt, l1."""
    return [f"{i:03d}_{j:02d}.png" for j in range(num_visualize_subframes)] + \
        [f"{i:03d}_blur.png", f"{i:03d}_gt.png", f"{i:03d}_l1.png"]


@torch.no_grad()
def traj_render(motion, cloud, model_path, iteration, tone_mapping=None, num_visualize_subframes=3, background=None,
                writer=None, *, device_png=False, _two_calls=None):
    """Visualizer.traj_render (utils/visualization.py:262-291): for every training view of `motion` the files
    III_00.png ... (num_visualize_subframes evenly spaced sharp subframes), III_blur.png, III_gt.png and III_l1.png (the jet
    L1 error map of the blurred synthesis) under {model_path}/traj_render_{iteration:05d}, which is removed and recreated
    (not with a writer).  Returns the paths.

    Per view ONE K-fused forward-only call renders all f subframes; the blurred image, the ground truth and the error
    map come from dgs_report_images(mean=1) over them, the shown subframes are slots linspace(0, f - 1, n).long() of the
    same call, finished with mean=0.  That is what the reference's two query() calls render while
    motion.curve_random_sample is off (both see the same trajectory); with it on two calls are made
    as the reference makes them, each with its own draw.  One background is drawn per view (background None: torch.rand(3))
    and used for both; the reference draws one per query().  device_png=True: the n + 3 images of a view are compressed
    on the device in one png.encode call instead of by PIL on the host (same names, same pixels; not with a writer)."""
    no_writer_with_device_png(writer, device_png)
    device = cloud._xyz.device
    if device.type != "cuda":
        raise RuntimeError("traj_render needs a motion module and a cloud on a HIP device (no CPU fallback)")
    # (_two_calls: for tests, forces either path)
    fused = not (motion.curve_random_sample if _two_calls is None else _two_calls)
    directory = traj_render_directory(model_path, iteration)
    if writer is None:
        fresh_directory(directory)
    n_sub = int(num_visualize_subframes)
    paths = []
    for i in range(len(motion)):
        bg = torch.rand(3, device=device) if background is None else background
        nu = motion._sample_nu_from_alignment(i)
        pick = torch.linspace(0, nu.shape[0] - 1, n_sub, device=nu.device).long()
        all_frames = gaussian_renderer.render_subframes(*motion.get_trajectory_matrices(i, nu), motion.ref_cam, cloud,
                                                        bg)["render"]
        if fused:
            shown = all_frames[pick]
        else:
            nu2 = motion._sample_nu_from_alignment(i)[pick]
            shown = gaussian_renderer.render_subframes(*motion.get_trajectory_matrices(i, nu2), motion.ref_cam, cloud,
                                                       bg)["render"]
        blur_u8, gt_u8, err = report_images(all_frames, tone_mapping, mean=True, gt=motion.get_gt_image(i))
        sub_u8, _, _ = report_images(shown, tone_mapping, mean=False)
        l1_u8 = colorize(err[0])
        if device_png:
            paths += write_device_png(directory, traj_render_names(i, n_sub), torch.cat([sub_u8, blur_u8, gt_u8, l1_u8[None]]))
            continue
        host = torch.cat([sub_u8, blur_u8, gt_u8, l1_u8[None]]).cpu().numpy()
        for k, name in enumerate(traj_render_names(i, n_sub)):
            paths.append(write_image(os.path.join(directory, name), host[k], writer))
    return paths

"""Scene loading: from a dataset directory -- a COLMAP `sparse/0` model and an `images/` folder -- to what the package
trains on.  The counterpart of the reference's readColmapSceneInfo (scene/dataset_readers.py:211-308), loadCam
(utils/camera_utils.py:21-58), PILtoTorch (utils/general_utils.py:23-29) and random_pcd_init (scene/pcd_init.py):

    training_resolution    loadCam's resolution rule (round() for 1/2/4/8, int() for a target width, the 1600 cap of -1)
    resize_images          Pillow's antialiased BICUBIC `Image.resize` of 8-bit images on the device (dgs_resize_u8), byte for
                           byte, straight into a slice of the float ground-truth stack
    pil_to_torch           PILtoTorch for one image
    depth_bounds           get_bds: per camera the 0.1 / 99.9 percentiles of the depths of the points it "sees"
                           (dgs_depth_bound_keys + dgs_order_stats)
    nerfpp_radius          getNerfppNorm's radius
    random_frustum_points  random_pcd_init, drawing from numpy's global generator in the reference's order
    load_colmap_scene      the directory -> a SceneData
    rgba_over              readCamerasFromTransforms' float64 composite of RGBA over black / white (dgs_rgba_over_u8)
    resize_rgba_images     Pillow's RGBA `Image.resize`: premultiplied, resampled, un-premultiplied (dgs_resize_rgba_u8)
    read_blender_cameras   readCamerasFromTransforms' cameras of a transforms_*.json
    load_blender_scene     readNerfSyntheticInfo: a NeRF-synthetic ("Blender") directory -> a SceneData
    load_scene             the reader the reference's Scene picks for a directory

        scene = load_colmap_scene(path, resolution=2)
        motion, cloud = scene.motion_module(), scene.cloud()
        loop = TrainingLoop(cloud, motion, opt, scene.cameras_extent)

The reference's quirks are kept: get_bds multiplies the camera coordinates by inv(K) and uses the
first camera's intrinsics for every camera; the resolution rule rounds for 1/2/4/8 and truncates otherwise; the train/test
split takes int(image_name); the point cloud goes through the float32 / uint8 quantisation of the reference's points3D.ply
round trip.  Nothing is written into the dataset directory.  There is no CPU path: the images are resized by the HIP kernel.
"""
import math
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, colmap_io
from .raster_call import _ptr, _stream

C0 = 0.28209479177387814            # utils/sh_utils.py:24
RESOLUTION_CAP = 1600               # loadCam: resolution == -1 rescales wider images to this width
KEY_BUDGET_BYTES = 256 << 20        # depth_bounds: the float32 key array [cameras of a group, points] stays below this
UPLOAD_BUDGET_BYTES = 512 << 20     # load_colmap_scene: 8-bit source images uploaded and resized per group of this size
SUPPORTED_MODELS = ("SIMPLE_PINHOLE", "PINHOLE")

CameraInfo = namedtuple("CameraInfo", "uid R T FovY FovX image_path image_name width height")
CameraInfo.__doc__ = """A camera of the COLMAP model as the reference keeps it (scene/dataset_readers.py:36-47): R the
camera-to-world rotation (the transposed rotation of the quaternion), T the world-to-camera translation, width / height of the
COLMAP intrinsics."""


def _need_cuda(device, what):
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"{what} needs a tensor on a HIP device (no CPU fallback)")


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


# ------------------------------------------------------------------------------------------------- resolution
def training_resolution(orig_w, orig_h, resolution, resolution_scale=1.0):
    """(w, h) an image of orig_w x orig_h is trained at (loadCam, utils/camera_utils.py:24-41): round() for resolution in
    1/2/4/8; -1 caps the width at 1600; any other value is a target width, and both go through int()."""
    if resolution in [1, 2, 4, 8]:
        return (round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution)))
    if resolution == -1:
        global_down = orig_w / RESOLUTION_CAP if orig_w > RESOLUTION_CAP else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return (int(orig_w / scale), int(orig_h / scale))


# ------------------------------------------------------------------------------------------------- resize
_table_cache = {}


def resample_coeffs(in_size, out_size):
    """(kk int32 [out, ksize], bounds int32 [out, 2]) of dgs_resample_coeffs as numpy arrays: Pillow's 8-bit bicubic taps."""
    L = _lib.lib()
    in_size, out_size = int(in_size), int(out_size)
    ksize = L.dgs_resample_ksize(in_size, out_size)
    kk = np.zeros((max(out_size, 1), max(ksize, 1)), dtype=np.int32)
    bounds = np.zeros((max(out_size, 1), 2), dtype=np.int32)
    _lib.check(L.dgs_resample_coeffs(in_size, out_size, kk.ctypes.data, kk.size if ksize > 0 else 0, bounds.ctypes.data),
               "dgs_resample_coeffs")
    return kk, bounds


def _device_tables(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    if key not in _table_cache:
        kk, bounds = resample_coeffs(in_size, out_size)
        _table_cache[key] = (torch.from_numpy(kk).to(device).contiguous(), torch.from_numpy(bounds).to(device).contiguous())
    return _table_cache[key]


def resize_images(images_u8, size, out=None, out_u8=None):
    """Pillow's `Image.resize(size)` (antialiased BICUBIC) of uint8 images on the device, byte for byte (dgs_resize_u8).
    images_u8: uint8 [G,H,W,C] (or [H,W,C]) on the device, C = 1 or 3, as np.asarray(PIL image) lays a pixel out; size =
    (w, h), PIL's order.
        out      float32 [G,C,h,w] to write byte / 255 into -- torch.from_numpy(resized) / 255.0 bit for bit.  It may be a
                 slice of a larger stack: images may be any stride >= C h w apart, each image itself contiguous.
        out_u8   uint8 [G,h,w,C], contiguous, to write the resized bytes into.
    Neither given: a new float tensor is returned.  One given: it is written and returned.  Both: (out, out_u8)."""
    images_u8, single = _images_arg(images_u8, "resize_images")
    G, H, W, C = (int(v) for v in images_u8.shape)
    w, h = int(size[0]), int(size[1])
    dev = images_u8.device
    out, stride = _outputs_arg(single, G, C, h, w, dev, out, out_u8)
    L = _lib.lib()
    tables = _resize_tables(H, W, h, w, dev)
    _lib.check(L.dgs_resize_u8(_ptr(images_u8), G, H, W, C, h, w, *tables, _ptr(out_u8), _ptr(out), stride, _stream(dev)),
               "dgs_resize_u8")
    return _outputs_result(out, out_u8)


def _images_arg(images_u8, who, channels=None):
    """(contiguous uint8 [G,H,W,C] on a HIP device, whether a single [H,W,C] image was given)."""
    if not torch.is_tensor(images_u8):
        raise RuntimeError(f"{who} needs a tensor on a HIP device (no CPU fallback)")
    _need_cuda(images_u8.device, who)
    single = images_u8.dim() == 3
    if single:
        images_u8 = images_u8[None]
    if images_u8.dim() != 4 or images_u8.dtype != torch.uint8 or (channels is not None and images_u8.shape[3] != channels):
        raise ValueError(f"{who} takes a uint8 [G,H,W,{'C' if channels is None else channels}] tensor")
    return images_u8.contiguous(), single


def _outputs_arg(single, G, C, h, w, dev, out, out_u8):
    """The output rules the image kernels share: (out, image stride in floats); a new float tensor when neither is given."""
    if out is None and out_u8 is None:
        out = torch.empty((G, C, max(h, 0), max(w, 0)), dtype=torch.float32, device=dev)
    stride = 0
    if out is not None:
        o = out[None] if (single and out.dim() == 3) else out
        if o.dtype != torch.float32 or tuple(o.shape) != (G, C, h, w) or o.device != dev or \
                (o.numel() > 0 and (o[0].is_contiguous() is False or (G > 1 and o.stride(0) < C * h * w))):
            raise ValueError(f"out must be a float32 [{G},{C},{h},{w}] tensor on the images' device, each image contiguous")
        stride = o.stride(0) if G > 1 else C * h * w
    if out_u8 is not None:
        if out_u8.dtype != torch.uint8 or out_u8.numel() != G * h * w * C or not out_u8.is_contiguous() or out_u8.device != dev:
            raise ValueError(f"out_u8 must be a contiguous uint8 tensor of {G} x {h} x {w} x {C} bytes on the images' device")
    return out, stride


def _outputs_result(out, out_u8):
    if out is not None and out_u8 is not None:
        return out, out_u8
    return out if out is not None else out_u8


def _resize_tables(H, W, h, w, dev):
    """The four table pointers of a resize call (0 for an axis that keeps its size or that the call will refuse)."""
    L = _lib.lib()
    kk_h = b_h = kk_v = b_v = None
    if W != w and L.dgs_resample_ksize(W, w) > 0:
        kk_h, b_h = _device_tables(W, w, dev)
    if H != h and L.dgs_resample_ksize(H, h) > 0:
        kk_v, b_v = _device_tables(H, h, dev)
    return _ptr(kk_h), _ptr(b_h), _ptr(kk_v), _ptr(b_v)


def resize_rgba_images(images_u8, size, out=None, out_u8=None):
    """Pillow's `Image.resize(size)` of RGBA images on the device, byte for byte (dgs_resize_rgba_u8): premultiplied by
    alpha, resampled, un-premultiplied -- and a plain copy when the size does not change.  images_u8: uint8 [G,H,W,4] (or
    [H,W,4]); out float32 [G,4,h,w] / out_u8 uint8 [G,h,w,4] under resize_images' rules."""
    images_u8, single = _images_arg(images_u8, "resize_rgba_images", 4)
    G, H, W, _ = (int(v) for v in images_u8.shape)
    w, h = int(size[0]), int(size[1])
    dev = images_u8.device
    out, stride = _outputs_arg(single, G, 4, h, w, dev, out, out_u8)
    tables = _resize_tables(H, W, h, w, dev)
    _lib.check(_lib.lib().dgs_resize_rgba_u8(_ptr(images_u8), G, H, W, h, w, *tables, _ptr(out_u8), _ptr(out), stride,
                                             _stream(dev)), "dgs_resize_rgba_u8")
    return _outputs_result(out, out_u8)


def rgba_over(images_u8, white_background, out=None, out_u8=None):
    """The Blender reader's composite of RGBA images over a white or black background on the device (dgs_rgba_over_u8):
    per colour byte numpy's float64 `(c/255 * a/255 + bg * (1 - a/255)) * 255` cast to np.byte, bit for bit.  images_u8:
    uint8 [G,H,W,4] (or [H,W,4]); out float32 [G,3,H,W] (byte / 255) / out_u8 uint8 [G,H,W,3] under resize_images' rules."""
    images_u8, single = _images_arg(images_u8, "rgba_over", 4)
    G, H, W, _ = (int(v) for v in images_u8.shape)
    dev = images_u8.device
    out, stride = _outputs_arg(single, G, 3, H, W, dev, out, out_u8)
    _lib.check(_lib.lib().dgs_rgba_over_u8(_ptr(images_u8), G, H, W, 1 if white_background else 0, _ptr(out_u8), _ptr(out),
                                           stride, _stream(dev)), "dgs_rgba_over_u8")
    return _outputs_result(out, out_u8)


def pil_to_torch(image_u8, size, device="cuda"):
    """PILtoTorch (utils/general_utils.py:23-29) of one 8-bit image: float32 [C,h,w] on the device, resized to size = (w, h)
    and divided by 255.  image_u8: uint8 [H,W] (mode L) or [H,W,C] as np.asarray(PIL image) gives it.  L, RGB and RGBA are
    resized on the device (RGBA through premultiplied alpha, as Pillow does: resize_rgba_images); LA goes through
    premultiplied alpha too and takes PIL's own `resize` on the host when PIL is importable, and raises otherwise."""
    _need_cuda(device, "pil_to_torch")
    arr = image_u8.cpu().numpy() if torch.is_tensor(image_u8) else np.asarray(image_u8)
    if arr.dtype != np.uint8 or arr.ndim not in (2, 3):
        raise ValueError("pil_to_torch takes a uint8 [H,W] or [H,W,C] image")
    if arr.ndim == 2:
        arr = arr[:, :, None]
    C = arr.shape[2]
    if C in (1, 3, 4):
        src = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        return (resize_rgba_images if C == 4 else resize_images)(src, size)[0]
    if C != 2:
        raise ValueError(f"pil_to_torch: an 8-bit image has 1 to 4 channels, not {C}")
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("pil_to_torch: a 2-channel image (LA) is resized through premultiplied alpha by Pillow; that path "
                           "runs on the host and needs PIL, which is not importable") from None
    resized = np.array(Image.fromarray(np.ascontiguousarray(arr)).resize((int(size[0]), int(size[1]))))
    return (torch.from_numpy(resized) / 255.0).permute(2, 0, 1).contiguous().to(device)


# ------------------------------------------------------------------------------------------------- bounds
def _w2c_rows(cams):
    rows = np.empty((len(cams), 3, 4), dtype=np.float64)
    for i, cam in enumerate(cams):
        rows[i, :, :3] = np.asarray(cam.R, dtype=np.float64).T
        rows[i, :, 3] = np.asarray(cam.T, dtype=np.float64)
    return rows


def _lerp(a, b, t):
    """numpy's linear interpolation between two order statistics (numpy/lib/_function_base_impl.py, _lerp), float64."""
    diff = b - a
    return b - diff * (1 - t) if t >= 0.5 else a + diff * t


def depth_bound_keys(cams, points_dev, first=None, keys=None):
    """(keys float32 [m,n], counts int32 [m]) on the device for the cameras `cams` (dgs_depth_bound_keys): the depth of every
    point a camera "sees" by get_bds' test, a NaN elsewhere.  first: the camera whose width, height and focal lengths are
    used (get_bds takes the FIRST camera's for all of them; default cams[0])."""
    _need_cuda(points_dev.device, "depth_bound_keys")
    first = cams[0] if first is None else first
    w, h = first.width, first.height
    fx, fy = fov2focal(first.FovX, w), fov2focal(first.FovY, h)
    m, n = len(cams), int(points_dev.shape[0])
    dev = points_dev.device
    w2c = torch.from_numpy(_w2c_rows(cams)).to(dev)
    if keys is None:
        keys = torch.empty((m, n), dtype=torch.float32, device=dev)
    counts = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dgs_depth_bound_keys(_ptr(points_dev), n, _ptr(w2c), m, float(w), float(h), float(fx), float(fy),
                                               _ptr(keys), _ptr(counts), _stream(dev)), "dgs_depth_bound_keys")
    return keys[:m], counts[:m]


def depth_bounds(cams, points, device="cuda", key_budget_bytes=KEY_BUDGET_BYTES, return_counts=False):
    """get_bds (scene/dataset_readers.py:164-209): float64 [m,2], per camera np.percentile(depths, 0.1) and (.., 99.9) over
    the depths of the points that pass its test (module docstring: inv(K), the first camera's intrinsics).
    cams: CameraInfo-like objects (R, T, FovX, FovY, width, height); points: [n,3], a float64 array or device tensor.
    The test runs in double on the device; the depths are selected as float32 keys (dgs_order_stats: two order statistics per
    percentile) and interpolated in float64 as numpy does, so a bound is within half a float32 ulp of the reference's.  The
    cameras are processed in groups whose key array stays below key_budget_bytes; the counts of a group are read once.
    A camera that sees no point raises ValueError."""
    from . import report
    _need_cuda(device, "depth_bounds")
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64))
    pts = pts.to(device=device, dtype=torch.float64).contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("depth_bounds takes points [n,3], n >= 1")
    cams = list(cams)
    m, n = len(cams), int(pts.shape[0])
    if m < 1:
        raise ValueError("depth_bounds takes at least one camera")
    group = max(1, min(m, int(key_budget_bytes) // (4 * n)))
    keys = torch.empty((group, n), dtype=torch.float32, device=pts.device)
    stats, plan, all_counts = [], [], []
    for b in range(0, m, group):
        e = min(b + group, m)
        k, counts = depth_bound_keys(cams[b:e], pts, first=cams[0], keys=keys)
        counts = counts.cpu().numpy().astype(np.int64)              # the one small read of this group
        all_counts.append(counts)
        for j, cnt in enumerate(counts):
            if cnt < 1:
                name = getattr(cams[b + j], "image_name", None)
                raise ValueError(f"depth_bounds: camera {b + j}" + (f" ({name})" if name is not None else "") +
                                 " sees none of the points")
            ranks, gammas = [], []
            for q in (0.1, 99.9):
                v = (int(cnt) - 1) * (q / 100.0)
                lo = int(math.floor(v))
                ranks += [lo, min(lo + 1, int(cnt) - 1)]
                gammas.append(v - lo)
            stats.append(report.order_stats(k[j], ranks))
            plan.append(gammas)
    host = torch.stack(stats).cpu().numpy().astype(np.float64)      # [m,4]
    out = np.empty((m, 2), dtype=np.float64)
    for i, (g_near, g_far) in enumerate(plan):
        out[i, 0] = _lerp(host[i, 0], host[i, 1], g_near)
        out[i, 1] = _lerp(host[i, 2], host[i, 3], g_far)
    return (out, np.concatenate(all_counts)) if return_counts else out


# ------------------------------------------------------------------------------------------------- scene radius
def camera_centers(cams):
    """The camera centres as getNerfppNorm forms them: the translation of inv(getWorld2View2(R, T)), a float32 matrix."""
    out = []
    for cam in cams:
        Rt = np.zeros((4, 4))
        Rt[:3, :3] = np.asarray(cam.R).transpose()
        Rt[:3, 3] = cam.T
        Rt[3, 3] = 1.0
        Rt = np.float32(np.linalg.inv(np.linalg.inv(Rt)))          # getWorld2View2 with translate 0, scale 1
        out.append(np.linalg.inv(Rt)[:3, 3])
    return np.stack(out)


def nerfpp_radius(cam_centers, points=None):
    """getNerfppNorm's radius (scene/dataset_readers.py:56-90): the smaller of 1.1 x the largest distance of a camera centre
    from their mean and -- with points -- the 10th percentile of the centres' distances from the points' mean, or -- without
    -- the 90th percentile of the centres' pairwise distances.  The arrays are used in the dtype they come in."""
    cam_centers = np.stack(list(cam_centers))
    if points is not None:
        center = np.asarray(points).mean(axis=0)
        radius1 = np.percentile(np.linalg.norm(cam_centers - center, axis=1), 10.0)
    else:
        radius1 = np.percentile(np.linalg.norm(cam_centers - cam_centers[:, None, :], axis=-1), 90)
    avg = np.mean(cam_centers, axis=0, keepdims=True)
    radius2 = np.max(np.linalg.norm(cam_centers - avg, axis=1)) * 1.1
    return min(radius1, radius2)


# ------------------------------------------------------------------------------------------------- random initialisation
def random_frustum_points(cams, near=0.0, far=8.0, num_pcd=100_000, bds=None):
    """random_pcd_init (scene/pcd_init.py): points along the rays of a strided pixel grid of every camera (its frustum
    widened to 1 / 0.8 of the field of view), at depths drawn uniformly from [max(near, bds[i,0]), min(far, bds[i,1])], the
    first num_pcd // max(len(cams) - 5, 1) + 2 of every camera, num_pcd in all.  float64 [<= num_pcd, 3].  The depths come
    from numpy's GLOBAL generator (np.random.random), one draw of 100 x grid values per camera in camera order: after
    np.random.seed(s) the result is the reference's, bit for bit."""
    cams = list(cams)
    d = 50
    per_cam = num_pcd // (max(len(cams) - 5, 1)) + 2
    all_xyz = []
    for i, cam in enumerate(cams):
        w2c = np.eye(4)
        w2c[:3, :3] = np.asarray(cam.R).T
        w2c[:3, 3] = cam.T
        c2w = np.linalg.inv(w2c)
        w, h = cam.width, cam.height
        fx, fy = fov2focal(cam.FovX, w), fov2focal(cam.FovY, h)
        K = np.array([[fx * 0.8, 0., w / 2], [0., fy * 0.8, h / 2], [0., 0., 1.]]).astype(np.float64)
        stride_coeff = per_cam ** (-1 / 3)
        stride_h, stride_w = int(h * stride_coeff), int(w * stride_coeff)
        if stride_h < 1 or stride_w < 1:
            raise ValueError(f"random_frustum_points: {per_cam} points per camera need a pixel grid finer than the "
                             f"{w} x {h} image (the reference fails here with a zero slice step)")
        pixels = np.stack(np.meshgrid(np.linspace(0, w - 1, w), np.linspace(0, h - 1, h), indexing="xy"), axis=-1)
        pixels = pixels[::stride_h, ::stride_w].reshape((-1, 2))
        homog = np.pad(pixels, ((0, 0), (0, 1)), "constant", constant_values=1.0)
        norm = ((np.linalg.inv(K) @ homog.T).T)[..., :2]
        norm = np.tile(norm, (d * 2, 1))
        cam_near = max(near, bds[i, 0] if bds is not None else 0.0)
        cam_far = min(far, bds[i, 1] if bds is not None else 999999999.9)
        depth = np.random.random((norm.shape[0])) * (cam_far - cam_near) + cam_near
        norm_homog = np.pad(norm, ((0, 0), (0, 1)), "constant", constant_values=1.0)
        cam_coords = (norm_homog * depth.reshape(-1, 1))[:per_cam]
        cam_homog = np.pad(cam_coords, ((0, 0), (0, 1)), "constant", constant_values=1.0)
        all_xyz.append(((c2w @ cam_homog.T).T)[..., :3])
    return np.concatenate(all_xyz, axis=0)[:num_pcd]


# ------------------------------------------------------------------------------------------------- the loader
def default_image_reader(path):
    """uint8 [H,W] or [H,W,C] of an image file: PIL when importable (any format it opens), else `.npy` arrays only."""
    if str(path).endswith(".npy"):
        return np.load(path)
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"cannot read {path}: PIL is not importable, so the default image_reader reads .npy arrays only "
                           "(pass image_reader=)") from None
    with Image.open(path) as im:
        return np.asarray(im)


def read_cameras(source_path, images="images"):
    """The CameraInfo list of <source_path>/sparse/0, in the order of the images file (readColmapCameras).  Binary files
    first; if either does not read, both are taken from the text files."""
    sparse = os.path.join(source_path, "sparse/0")
    try:
        extr = colmap_io.read_images_binary(os.path.join(sparse, "images.bin"))
        intr = colmap_io.read_cameras_binary(os.path.join(sparse, "cameras.bin"))
    except Exception:
        extr = colmap_io.read_images_text(os.path.join(sparse, "images.txt"))
        intr = colmap_io.read_cameras_text(os.path.join(sparse, "cameras.txt"))
    folder = os.path.join(source_path, "images" if images is None else images)
    out = []
    for key in extr:
        e = extr[key]
        c = intr[e.camera_id]
        R = np.transpose(colmap_io.qvec2rotmat(e.qvec))
        T = np.array(e.tvec)
        if c.model == "SIMPLE_PINHOLE":
            fov_y, fov_x = focal2fov(c.params[0], c.height), focal2fov(c.params[0], c.width)
        elif c.model == "PINHOLE":
            fov_y, fov_x = focal2fov(c.params[1], c.height), focal2fov(c.params[0], c.width)
        else:
            raise ValueError(f"camera {c.id} has the COLMAP model {c.model}: only undistorted datasets "
                             f"({' or '.join(SUPPORTED_MODELS)} cameras) are supported")
        path = os.path.join(folder, os.path.basename(e.name))
        name = os.path.basename(path).split(".")[0]
        out.append(CameraInfo(c.id, R, T, fov_y, fov_x, path, name, c.width, c.height))
    return out


def split_cameras(cams, source_path, eval=False, llffhold=0):
    """(train, test) of the cameras sorted by image name (readColmapSceneInfo:229-252).  llffhold 0: a file or directory
    named `hold=n` in source_path sets it.  With eval and llffhold > 0 the images whose int(image_name) is a multiple of
    llffhold are the test views; one of the two without the other is an error, as in the reference."""
    cams = sorted(list(cams), key=lambda c: c.image_name)
    if llffhold == 0:
        marks = [e for e in os.listdir(source_path) if "hold=" in e]
        if len(marks) > 1:
            raise ValueError(f"more than one llffhold indicator in {source_path}: {marks}")
        if marks:
            llffhold = int(marks[0].strip().split("=")[-1])
    if eval and llffhold > 0:
        def number(c):
            try:
                return int(c.image_name)
            except ValueError:
                raise ValueError(f"the train/test split takes int(image_name): {c.image_name!r} is not a number") from None
        return [c for c in cams if number(c) % llffhold != 0], [c for c in cams if number(c) % llffhold == 0]
    if llffhold > 0 or eval:
        raise ValueError(f"one of eval ({eval}) and llffhold ({llffhold}) is set while the other is off")
    return cams, []


def read_points(source_path, num_initial_pcd=0):
    """(xyz float64 [n,3], rgb float64 [n,3] in 0..255) of sparse/0/points3D (.bin, else .txt).  num_initial_pcd > 0 keeps the
    points whose reprojection error is BELOW the percentile min(num_initial_pcd / n x 100, 100) of all errors
    (readColmapSceneInfo:266-275; numpy, float64, once)."""
    pts = colmap_io._either(os.path.join(source_path, "sparse/0"), "points3D", colmap_io.read_points3D_binary,
                            colmap_io.read_points3D_text)
    xyz, rgb, error = pts.xyz, pts.rgb, pts.error
    if num_initial_pcd > 0:
        error = error.reshape((-1,))
        percent = min(num_initial_pcd / xyz.shape[0] * 100, 100.0)
        keep = error < np.percentile(error, percent)
        xyz, rgb = xyz[keep], rgb[keep]
    return xyz, rgb


def _ply_round_trip(xyz, rgb255):
    """What the reference trains on after storePly / fetchPly: float32 positions, uint8 colours / 255."""
    # (C order: random_pcd_init's points come out of np.concatenate column-major, and a cloud's parameters are contiguous)
    return np.ascontiguousarray(xyz, dtype=np.float32), np.ascontiguousarray(rgb255).astype(np.uint8) / 255.0


@dataclass
class SceneData:
    """What load_colmap_scene and load_blender_scene return.
        ref_cam         motion.RefCamera of the training size and the training cameras' field of view
        gt_images       float32 [n,3,h,w] on the device
        init_c2w        (rotations float64 [n,3,3], positions float64 [n,3]): CameraMotionModule(init_c2w=...)'s form
        image_names     the n training image names, sorted
        test_images     float32 [t,3,h,w] on the device, or None;  test_c2w / test_names: the same for the test views
        points, colors  float32 [P,3], float64 [P,3] in 0..1 (numpy): the initial cloud
        cameras_extent  the scene radius (TrainingLoop's cameras_extent)
        train_cameras, test_cameras   the CameraInfo lists"""
    ref_cam: Any
    gt_images: torch.Tensor
    init_c2w: Tuple[torch.Tensor, torch.Tensor]
    image_names: List[str]
    test_images: Optional[torch.Tensor]
    test_c2w: Optional[Tuple[torch.Tensor, torch.Tensor]]
    points: np.ndarray
    colors: np.ndarray
    cameras_extent: float
    test_names: List[str] = None
    train_cameras: List[Any] = None
    test_cameras: List[Any] = None
    activation: str = "relu"
    z_near: float = 0.2
    z_far: float = 100.0
    device: Any = "cuda"
    white_background: bool = False      # the background the images were composited over (TrainingLoop's white_background)

    def motion_module(self, **kw):
        """CameraMotionModule on this scene's images and initial poses (kw: curve_order, num_subframes, ...)."""
        from .motion import CameraMotionModule
        kw.setdefault("device", self.device)
        return CameraMotionModule(self.ref_cam, self.gt_images, init_c2w=self.init_c2w, **kw)

    def cloud(self, **kw):
        """The initial GaussianCloud of this scene's points (simple_knn.create_from_points; kw: sh_degree, scale_lb, ...)."""
        from .simple_knn import create_from_points
        kw.setdefault("device", self.device)
        kw.setdefault("use_sigmoid", self.activation == "sigmoid")
        kw.setdefault("z_near", self.z_near)
        kw.setdefault("z_far", self.z_far)
        return create_from_points(self.points, self.colors, **kw)


def _c2w_of(cams):
    rot = torch.from_numpy(np.stack([np.asarray(c.R, dtype=np.float64) for c in cams]))
    pos = torch.from_numpy(np.stack([-np.asarray(c.T) @ np.asarray(c.R).T for c in cams]))     # scene/motion.py:44-45
    return rot, pos


def _find_image(path):
    if os.path.exists(path):
        return path
    for alt in (path[:-4] + ".jpg", os.path.splitext(path)[0] + ".npy"):    # (readColmapCameras:127-129 retries as .jpg)
        if os.path.exists(alt):
            return alt
    raise FileNotFoundError(path)


def _device_jpeg(path):
    """(file bytes, decode plan) of a .jpg / .jpeg file that jpeg.decode takes as RGB, else None: progressive, CMYK, gray and
    malformed files -- everything jpeg.plan refuses -- stay with the image reader, as every other format does."""
    if os.path.splitext(path)[1].lower() not in (".jpg", ".jpeg"):
        return None
    from . import jpeg
    with open(path, "rb") as f:
        data = f.read()
    try:
        plan = jpeg.plan(data)
    except ValueError:
        return None
    head = jpeg._head(plan)
    return (data, plan, (head.h, head.w, 3)) if head.channels == 3 else None


def _load_images(cams, resolution, reader, device, what, device_jpeg=False):
    """float32 [n,3,h,w] on the device: every image read, uploaded and resized in groups of at most UPLOAD_BUDGET_BYTES.
    A group holds images of one channel count; RGBA images are resized through premultiplied alpha (resize_rgba_images)
    and their first three planes are the ground truth, as in loadCam.  device_jpeg: the .jpg / .jpeg files the device
    decoder takes (_device_jpeg) go up as FILES and are decoded there (jpeg.decode), inside the same groups, into the
    8-bit source the resize reads; every other file is read by `reader` as without it."""
    if not cams:
        return None
    stack, size, src_shape, pending, shapes = None, None, None, [], []

    def flush(first):
        if pending:
            files = [k for k, e in enumerate(pending) if not isinstance(e, np.ndarray)]
            if not files:
                src = torch.from_numpy(np.stack(pending)).to(device)
            else:
                from . import jpeg
                host = [k for k in range(len(pending)) if k not in set(files)]
                src = torch.empty((len(pending),) + tuple(shapes[0]), dtype=torch.uint8, device=device)
                decoded = jpeg.decode([pending[k][0] for k in files], device, plans=[pending[k][1] for k in files],
                                      out=None if host else src)
                if host:
                    src[files] = decoded
                    src[host] = torch.from_numpy(np.stack([pending[k] for k in host])).to(device)
            if src.shape[3] == 4:
                stack[first:first + len(pending)] = resize_rgba_images(src, size)[:, :3]
            else:
                resize_images(src, size, out=stack[first:first + len(pending)])
            pending.clear()
            shapes.clear()

    first = 0
    for i, cam in enumerate(cams):
        path = _find_image(cam.image_path)
        item = _device_jpeg(path) if device_jpeg else None
        if item is None:
            img = np.asarray(reader(path))
            if img.dtype != np.uint8 or img.ndim not in (2, 3):
                raise ValueError(f"{cam.image_path}: the image reader must return uint8 [H,W,C], got {img.dtype} {img.shape}")
            if img.ndim == 2:
                img = img[:, :, None]
            if img.shape[2] not in (3, 4):
                raise ValueError(f"{cam.image_path}: {what} images must be RGB (or RGBA), got {img.shape[2]} channel(s)")
            shape, entry = img.shape, np.ascontiguousarray(img)
        else:
            shape, entry = item[2], item[:2]
        if src_shape is None:
            src_shape = shape[:2]
            size = training_resolution(shape[1], shape[0], resolution)
            stack = torch.empty((len(cams), 3, size[1], size[0]), dtype=torch.float32, device=device)
        elif shape[:2] != src_shape:
            raise ValueError(f"{what} images must share one size: {cam.image_path} is {shape[:2]}, the first is {src_shape}")
        if pending and shapes[0][2] != shape[2]:
            flush(first)
            first = i
        pending.append(entry)
        shapes.append(shape)
        if len(pending) * shape[0] * shape[1] * shape[2] >= UPLOAD_BUDGET_BYTES:
            flush(first)
            first = i + 1
    flush(first)
    return stack


def load_colmap_scene(source_path, images="images", resolution=-1, eval=False, llffhold=0, random_init=False,
                      num_initial_pcd=0, z_near=0.2, z_far=100.0, activation="relu", device="cuda", image_reader=None,
                      num_random_points=100_000, device_jpeg=False):
    """readColmapSceneInfo + cameraList_from_camInfos for a COLMAP dataset directory: a SceneData.
    source_path/sparse/0 holds cameras, images and points3D (.bin, else .txt); source_path/<images> the pictures.
        resolution       loadCam's rule (training_resolution); the images are resized on the device
        eval, llffhold   the train/test split (split_cameras)
        num_initial_pcd  > 0: prune the points with the largest reprojection errors (read_points)
        random_init      replace the points by num_random_points (the reference: 100 000) drawn in the training cameras'
                         frusta between the depth bounds of the COLMAP points (depth_bounds, random_frustum_points with
                         near = z_near + 1 % and far = z_far - 30 % of z_far - z_near), colour 0.01; the scene radius then
                         comes from the cameras alone.  Draws from numpy's global generator.
        activation       "relu" or "sigmoid": the colour activation the cloud is made for
        image_reader     path -> uint8 [H,W,C] (default: PIL, or .npy arrays where PIL is not importable)
        device_jpeg      True: baseline .jpg / .jpeg files (jpeg.probe says which) are uploaded as files and decoded on the
                         device (jpeg.decode: Pillow's pixels, bit for bit) on their way into the resize; every other file
                         goes through image_reader as before.  Off by default.
    The training images must share one size and one set of intrinsics (CameraMotionModule has one RefCamera)."""
    from .motion import RefCamera
    _need_cuda(device, "load_colmap_scene")
    reader = default_image_reader if image_reader is None else image_reader
    train, test = split_cameras(read_cameras(source_path, images), source_path, eval=eval, llffhold=llffhold)
    if not train:
        raise ValueError(f"{source_path}: no training camera")
    first = train[0]
    for c in train[1:]:
        if (c.width, c.height, c.FovX, c.FovY) != (first.width, first.height, first.FovX, first.FovY):
            raise ValueError(f"the training cameras must share one set of intrinsics: {c.image_name} has "
                             f"{(c.width, c.height, c.FovX, c.FovY)}, {first.image_name} has "
                             f"{(first.width, first.height, first.FovX, first.FovY)}")
    xyz, rgb = read_points(source_path, num_initial_pcd)
    sigmoid = activation == "sigmoid"
    if random_init:
        span = z_far - z_near
        bds = depth_bounds(train, xyz, device=device)
        xyz = random_frustum_points(train, near=z_near + span * 0.01, far=z_far - span * 0.30, num_pcd=num_random_points,
                                    bds=bds)
        shs = np.ones((num_random_points, 3)) * 0.01
        shs = shs / C0 if sigmoid else (shs - 0.5) / C0                      # RGB2SH
        rgb = (shs * C0 if sigmoid else shs * C0 + 0.5)[:xyz.shape[0]] * 255   # SH2RGB, as storePly receives it
    points, colors = _ply_round_trip(xyz, rgb)
    radius = nerfpp_radius(camera_centers(train), None if random_init else points)
    gt = _load_images(train, resolution, reader, device, "training", device_jpeg)
    tests = _load_images(test, resolution, reader, device, "test", device_jpeg)
    h, w = int(gt.shape[2]), int(gt.shape[3])
    ref = RefCamera(w, h, first.FovX, first.FovY, device=device)
    return SceneData(ref_cam=ref, gt_images=gt, init_c2w=_c2w_of(train), image_names=[c.image_name for c in train],
                     test_images=tests, test_c2w=_c2w_of(test) if test else None, points=points, colors=colors,
                     cameras_extent=float(radius), test_names=[c.image_name for c in test], train_cameras=train,
                     test_cameras=test, activation=activation, z_near=z_near, z_far=z_far, device=device)


# ------------------------------------------------------------------------------------------------- Blender scenes
def _rgba_of(img, path):
    """uint8 [H,W,3] or [H,W,4] of what a reader returned: PIL's lossless `convert("RGBA")` of L and LA on the host (the
    grey replicated), RGB and RGBA as they are (RGB has alpha 255, over which the composite is the identity)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError(f"{path}: the image reader must return uint8 [H,W,C], got {img.dtype} {img.shape}")
    if img.ndim == 2:
        img = img[:, :, None]
    C = img.shape[2]
    if C == 1:
        return np.repeat(img, 3, axis=2)
    if C == 2:
        return np.concatenate([np.repeat(img[:, :, :1], 3, axis=2), img[:, :, 1:]], axis=2)
    if C not in (3, 4):
        raise ValueError(f"{path}: an 8-bit image has 1 to 4 channels, not {C}")
    return np.ascontiguousarray(img)


def _read_blender(path, transformsfile, extension, reader):
    """(CameraInfo list, the images as uint8 [H,W,3|4] arrays) of a transforms file, in the file's order."""
    import json
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    fovx = contents["camera_angle_x"]
    cams, images = [], []
    for idx, frame in enumerate(contents["frames"]):
        cam_name = frame["file_path"] + extension
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1                                  # OpenGL / Blender axes (y up, z back) -> COLMAP's (y down, z forward)
        w2c = np.linalg.inv(c2w)
        R = np.transpose(w2c[:3, :3])
        T = w2c[:3, 3]
        image_path = os.path.join(path, cam_name)
        img = _rgba_of(reader(_find_image(image_path)), image_path)
        height, width = int(img.shape[0]), int(img.shape[1])
        fovy = focal2fov(fov2focal(fovx, width), height)
        name = os.path.splitext(os.path.basename(cam_name))[0]
        cams.append(CameraInfo(idx, R, T, fovy, fovx, image_path, name, width, height))
        images.append(img)
    return cams, images


def read_blender_cameras(path, transformsfile, extension=".png", image_reader=None):
    """The CameraInfo list of a NeRF-synthetic transforms file (readCamerasFromTransforms, scene/dataset_readers.py:310-350):
    the frame's camera-to-world matrix with its y and z columns negated, inverted; R the transposed rotation of that, T its
    translation; FovX the file's camera_angle_x, FovY from the focal length of FovX and the image's size (each image is
    read for it); image_name the stem of file_path + extension; uid the frame's index."""
    return _read_blender(path, transformsfile, extension, default_image_reader if image_reader is None else image_reader)[0]


def split_blender(train, test, eval=False):
    """(train, test) as readNerfSyntheticInfo splits them: without eval the test views are appended to the training views."""
    return (list(train), list(test)) if eval else (list(train) + list(test), [])


def blender_random_cloud(train_cams, num_points=100_000):
    """(xyz float64 [n,3], rgb float64 [n,3] in 0..255) of readNerfSyntheticInfo's random initialisation: random_pcd_init
    between the depths 2 and 8, THEN np.random.random((num_points, 3)) / 255 through SH2RGB, times 255 as storePly receives
    it -- both from numpy's global generator, in this order."""
    xyz = random_frustum_points(train_cams, near=2.0, far=8.0, num_pcd=num_points)
    shs = np.random.random((num_points, 3)) / 255.0
    return xyz, ((shs * C0 + 0.5) * 255)[:xyz.shape[0]]


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply_points(path):
    """(xyz [n,3], rgb [n,3] in 0..255) of the vertex element of a PLY file in storePly's layout (x y z nx ny nz red green
    blue; any scalar properties are accepted, lists are not): binary little- or big-endian, or ascii."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, in_vertex, first_element = None, None, [], False, None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: the PLY header does not end")
            words = line.decode("ascii").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                first_element = words[1] if first_element is None else first_element
                in_vertex = words[1] == "vertex"
                if in_vertex:
                    count = int(words[2])
            elif words[0] == "property" and in_vertex:
                if words[1] == "list" or words[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unsupported vertex property {' '.join(words[1:])}")
                props.append((words[2], _PLY_TYPES[words[1]]))
            elif words[0] == "end_header":
                break
        if count is None or first_element != "vertex":
            raise ValueError(f"{path}: the first element of the PLY file must be its vertices")
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=count, ndmin=2) if count else np.zeros((0, len(props)))
            data = {name: rows[:, k].astype(t) for k, (name, t) in enumerate(props)}
        elif fmt in ("binary_little_endian", "binary_big_endian"):
            order = "<" if fmt == "binary_little_endian" else ">"
            data = np.frombuffer(f.read(), dtype=np.dtype([(name, order + t) for name, t in props]), count=count)
        else:
            raise ValueError(f"{path}: unknown PLY format {fmt}")
    missing = [k for k in ("x", "y", "z", "red", "green", "blue") if k not in dict(props)]
    if missing:
        raise ValueError(f"{path}: the vertices have no {', '.join(missing)}")
    return (np.vstack([data["x"], data["y"], data["z"]]).T, np.vstack([data["red"], data["green"], data["blue"]]).T)


def _load_blender_images(images, white_background, resolution, device, what):
    """float32 [n,3,h,w] on the device of the uint8 [H,W,3|4] arrays: uploaded in groups of one channel count and at most
    UPLOAD_BUDGET_BYTES, RGBA composited over the background (rgba_over), then resized to training_resolution's size
    (resize_images) -- one launch where the size does not change, two with a 3 byte / pixel intermediate where it does."""
    if not images:
        return None
    H, W = images[0].shape[:2]
    for k, img in enumerate(images):
        if img.shape[:2] != (H, W):
            raise ValueError(f"{what} images must share one size: image {k} is {img.shape[:2]}, the first is {(H, W)}")
    size = training_resolution(W, H, resolution)
    stack = torch.empty((len(images), 3, size[1], size[0]), dtype=torch.float32, device=device)
    first = 0
    while first < len(images):
        C = images[first].shape[2]
        last = first
        while last < len(images) and images[last].shape[2] == C and (last - first) * H * W * C < UPLOAD_BUDGET_BYTES:
            last += 1
        src = torch.from_numpy(np.stack(images[first:last])).to(device)
        out = stack[first:last]
        if C == 3:
            resize_images(src, size, out=out)
        elif size == (W, H):
            rgba_over(src, white_background, out=out)
        else:
            resize_images(rgba_over(src, white_background, out_u8=torch.empty((last - first, H, W, 3), dtype=torch.uint8,
                                                                               device=device)), size, out=out)
        first = last
    return stack


def load_blender_scene(source_path, white_background=False, eval=False, resolution=-1, extension=".png", activation="relu",
                       z_near=0.2, z_far=100.0, device="cuda", image_reader=None, num_random_points=100_000):
    """readNerfSyntheticInfo + cameraList_from_camInfos for a NeRF-synthetic ("Blender") directory: a SceneData.
    source_path holds transforms_train.json and transforms_test.json; a frame's picture is file_path + extension.
        white_background  composite the RGBA pictures over white instead of black (on the device, rgba_over: numpy's float64
                          expression and its truncating cast, bit for bit); RGB pictures are taken as they are
        eval              keep the test views apart; otherwise they are appended to the training views
        resolution        loadCam's rule (training_resolution), applied to the composited bytes
        points            source_path/points3d.ply when it exists (storePly's vertex layout); otherwise num_random_points
                          (the reference: 100 000) from blender_random_cloud, drawn from numpy's global generator.  Both
                          go through the float32 / uint8 quantisation of the reference's ply round trip; nothing is written.
    The scene radius comes from the cameras alone.  The pictures must share one size."""
    from .motion import RefCamera
    _need_cuda(device, "load_blender_scene")
    reader = default_image_reader if image_reader is None else image_reader
    train, train_images = _read_blender(source_path, "transforms_train.json", extension, reader)
    test, test_images = _read_blender(source_path, "transforms_test.json", extension, reader)
    if not eval:
        train_images, test_images = train_images + test_images, []
    train, test = split_blender(train, test, eval)
    if not train:
        raise ValueError(f"{source_path}: no training camera")
    first = train[0]
    for c in train[1:]:
        if (c.width, c.height, c.FovX, c.FovY) != (first.width, first.height, first.FovX, first.FovY):
            raise ValueError(f"the training cameras must share one set of intrinsics: {c.image_name} has "
                             f"{(c.width, c.height, c.FovX, c.FovY)}, {first.image_name} has "
                             f"{(first.width, first.height, first.FovX, first.FovY)}")
    ply = os.path.join(source_path, "points3d.ply")
    xyz, rgb = read_ply_points(ply) if os.path.exists(ply) else blender_random_cloud(train, num_random_points)
    points, colors = _ply_round_trip(xyz, rgb)
    radius = nerfpp_radius(camera_centers(train))
    white_background = bool(white_background)
    gt = _load_blender_images(train_images, white_background, resolution, device, "training")
    tests = _load_blender_images(test_images, white_background, resolution, device, "test")
    h, w = int(gt.shape[2]), int(gt.shape[3])
    ref = RefCamera(w, h, first.FovX, first.FovY, device=device)
    return SceneData(ref_cam=ref, gt_images=gt, init_c2w=_c2w_of(train), image_names=[c.image_name for c in train],
                     test_images=tests, test_c2w=_c2w_of(test) if test else None, points=points, colors=colors,
                     cameras_extent=float(radius), test_names=[c.image_name for c in test], train_cameras=train,
                     test_cameras=test, activation=activation, z_near=z_near, z_far=z_far, device=device,
                     white_background=white_background)


def load_scene(source_path, **kw):
    """The loader the reference's Scene picks (scene/__init__.py:50-56): a `sparse` directory or `poses_bounds.npy` means a
    COLMAP dataset (load_colmap_scene), `transforms_train.json` a Blender one (load_blender_scene); kw goes to that loader."""
    if os.path.exists(os.path.join(source_path, "sparse")) or os.path.exists(os.path.join(source_path, "poses_bounds.npy")):
        return load_colmap_scene(source_path, **kw)
    if os.path.exists(os.path.join(source_path, "transforms_train.json")):
        return load_blender_scene(source_path, **kw)
    raise ValueError(f"{source_path}: neither a COLMAP dataset (sparse/, poses_bounds.npy) nor a Blender one "
                     "(transforms_train.json): could not recognise the scene type")

"""Cases shared by tests/test_scene_host.py, tests/test_gpu_scene.py and tests/golden/make_golden_scene.py: the resize cases
and their seeded inputs, a numpy restatement of Pillow's 8-bit bicubic resize, the depth-bounds cases with their
preconditions, a COLMAP model WRITER (struct packing from COLMAP's published format, binary and text) and the small models
the reader tests parse."""
import math
import os
import struct
from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------------------------------------- resize cases
ResizeCase = namedtuple("ResizeCase", "name H W h w C G covers")
RESIZE_CASES = [
    ResizeCase("odd", 37, 53, 18, 26, 3, 1, "odd sizes, non-integer ratio"),
    ResizeCase("odd_ksize", 37, 53, 19, 27, 3, 1, "a different ksize alignment"),
    ResizeCase("ratio7", 64, 48, 9, 7, 3, 1, "ratio ~ 7, 31 taps"),
    ResizeCase("h_only", 31, 45, 31, 20, 3, 1, "vertical pass skipped"),
    ResizeCase("v_only_L", 50, 70, 13, 70, 1, 1, "horizontal pass skipped, one channel"),
    ResizeCase("upscale", 20, 30, 45, 61, 3, 1, "upscale, heavy clipping"),
    ResizeCase("one_pixel", 16, 16, 1, 1, 3, 1, "single output pixel"),
    ResizeCase("tiles", 135, 240, 68, 120, 3, 3, "crosses tile borders on both axes, misaligned input pointer"),
    ResizeCase("ratio33", 330, 24, 10, 12, 3, 1, "vertical ratio 33: the LDS budget's fallback (a shrunk tile)"),
]
EXTRA_COEFF_SIZES = [(1080, 540), (2160, 900), (7, 448)]


def resize_input(case):
    """uint8 [G,H,W,C], seeded by the case's position: uniform noise, and a third of the rows -- every third band of rows --
    drawn from {0, 255} in blocks as large as the positive lobe of the filter (two output pixels each way, at most a
    third of the image), so that the
    bicubic lobes overshoot on both sides in both passes and both clamps fire (CLAMPS_FIRE)."""
    rng = np.random.default_rng(1000 + [c.name for c in RESIZE_CASES].index(case.name))
    img = rng.integers(0, 256, (case.G, case.H, case.W, case.C), dtype=np.uint8)
    run_w = min(2 * max(1, int(round(case.W / case.w))), max(1, case.W // 3))
    band = min(2 * max(1, int(round(case.H / case.h))), max(1, case.H // 3))
    for g in range(case.G):
        for y in range(case.H):
            if (y // band) % 3 != g % 3:
                continue
            if y % band == 0:
                bits = rng.integers(0, 2, (case.W // run_w + 1, case.C), dtype=np.uint8).repeat(run_w, axis=0)[:case.W]
            img[g, y] = bits * 255
    return img


# every tap of 16 -> 1 lies in the filter's positive lobe: its samples are convex combinations and cannot leave 0..255
CLAMPS_FIRE = {c.name: c.name != "one_pixel" for c in RESIZE_CASES}


# ------------------------------------------------------------------------------------------------- Pillow, restated
PRECISION_BITS = 32 - 8 - 2


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_ksize(in_size, out_size):
    return int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


def resample_coeffs(in_size, out_size):
    """(kk int32 [out, ksize], bounds int32 [out, 2]): precompute_coeffs + normalize_coeffs_8bpc of Pillow's Resample.c for
    the bicubic filter, in Python floats (IEEE doubles, one rounding per operation)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(img, out_size, axis, clamps):
    """One pass of ImagingResample along `axis` of an int64 array; clamps[0] / clamps[1] count the samples clipped at 0 / 255."""
    img = np.moveaxis(img, axis, 0)
    kk, bounds = resample_coeffs(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], dtype=np.int64)
    for xx in range(out_size):
        xmin, xmax = (int(v) for v in bounds[xx])
        k = kk[xx, :xmax].astype(np.int64).reshape((-1,) + (1,) * (img.ndim - 1))
        ss = (1 << (PRECISION_BITS - 1)) + (img[xmin:xmin + xmax] * k).sum(axis=0)
        assert np.abs(ss).max() < 2 ** 31
        v = ss >> PRECISION_BITS
        clamps[0] += int((v < 0).sum())
        clamps[1] += int((v > 255).sum())
        out[xx] = np.clip(v, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_restated(images_u8, size, clamps=None):
    """Pillow's Image.resize(size) (BICUBIC) of uint8 [G,H,W,C] -> uint8 [G,h,w,C]: horizontal pass first, rounded to bytes,
    then the vertical pass; a pass whose size does not change is skipped."""
    clamps = [0, 0] if clamps is None else clamps
    w, h = size
    x = np.asarray(images_u8).astype(np.int64)
    if x.shape[2] != w:
        x = _pass(x, w, 2, clamps)
    if x.shape[1] != h:
        x = _pass(x, h, 1, clamps)
    return x.astype(np.uint8)


# ------------------------------------------------------------------------------------------------- resolution table
RESOLUTION_TABLE = [(w, h, r) for (w, h) in ((1601, 1067), (1600, 1066), (1599, 901), (3840, 2160), (4001, 2251), (97, 65),
                                             (1234, 821), (50, 30), (101, 67))
                    for r in (1, 2, 4, 8, -1, 800, 1600, 3, 960.5)]

# ------------------------------------------------------------------------------------------------- cameras and bounds
Cam = namedtuple("Cam", "uid R T FovY FovX image_path image_name width height")   # the fields of scene.CameraInfo


def _rotvec(v):
    v = np.asarray(v, dtype=np.float64)
    t = np.linalg.norm(v)
    if t == 0.0:
        return np.eye(3)
    k = v / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def make_cameras(n, seed, width=96, height=64, fov_x=1.1, fov_y=0.8):
    """n cameras around the origin looking roughly down +z of the world: CameraInfo-like tuples."""
    rng = np.random.default_rng(seed)
    cams = []
    for i in range(n):
        Rc2w = _rotvec(rng.normal(0.0, 0.25, 3))
        centre = rng.normal(0.0, 0.6, 3)
        T = -Rc2w.T @ centre
        cams.append(Cam(1, Rc2w, T, fov_y, fov_x, "", f"{i:03d}", width, height))
    return cams


BoundsCase = namedtuple("BoundsCase", "name cams points")
BOUNDS_SHAPES = [("m3_n500", 3, 500), ("m17_n4099", 17, 4099)]


def bounds_quantities(cams, points):
    """get_bds' per-pair quantities in float64: (depth, px, py, d, mag) [m,n], mag the magnitude of d's terms."""
    first = cams[0]
    w, h = first.width, first.height
    fx = w / (2 * math.tan(first.FovX / 2))
    fy = h / (2 * math.tan(first.FovY / 2))
    out = []
    for c in cams:
        cam = points @ c.R + c.T            # rows: R^T p + T with R the c2w rotation
        x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
        d = z - x * (w / 2) / fx - y * (h / 2) / fy
        mag = np.abs(z) + np.abs(x * (w / 2) / fx) + np.abs(y * (h / 2) / fy)
        out.append((z, (x / fx) / d, (y / fy) / d, d, mag))
    return [np.stack(v) for v in zip(*out)], (w, h)


def bounds_valid(cams, points):
    (z, px, py, d, mag), (w, h) = bounds_quantities(cams, points)
    return (z > 0.01) & (px >= 0) & (px < w) & (py >= 0) & (py < h)


def bounds_cases():
    """The depth-bounds cases, with their preconditions asserted on the float64 restatement alone: no (camera, point) pair
    within 1e-9 (relative) of a decision boundary -- depth = 0.01, px = 0, px = w, py = 0, py = h, and the sign change of the
    divisor d -- and at least 20 visible points per camera."""
    cases = []
    for k, (name, m, n) in enumerate(BOUNDS_SHAPES):
        cams = make_cameras(m, 50 + k)
        rng = np.random.default_rng(70 + k)
        pts = np.stack([rng.normal(0.0, 2.0, n), rng.normal(0.0, 2.0, n), rng.uniform(-1.0, 9.0, n)], axis=1)
        (z, px, py, d, mag), (w, h) = bounds_quantities(cams, pts)
        eps = 1e-9
        assert (np.abs(z - 0.01) > eps * np.maximum(np.abs(z), 0.01)).all()
        assert (np.abs(d) > eps * mag).all()
        for p, size in ((px, w), (py, h)):
            assert (np.abs(p) > eps * size).all() and (np.abs(p - size) > eps * size).all()
        assert (bounds_valid(cams, pts).sum(axis=1) >= 20).all(), bounds_valid(cams, pts).sum(axis=1)
        cases.append(BoundsCase(name, cams, pts))
    return cases


# ------------------------------------------------------------------------------------------------- COLMAP model writer
MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
             "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}


def write_model(directory, cameras, images, points, binary=True):
    """cameras: [(id, model, width, height, params)], images: [(id, qvec, tvec, camera_id, name, [(x, y, point3D_id)])],
    points: [(id, xyz, rgb, error, [(image_id, point2D_idx)])] -> cameras / images / points3D (.bin or .txt) in directory."""
    os.makedirs(directory, exist_ok=True)
    if binary:
        with open(os.path.join(directory, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(cameras)))
            for cid, model, width, height, params in cameras:
                f.write(struct.pack("<iiQQ", cid, MODEL_IDS[model], width, height))
                f.write(struct.pack("<%dd" % len(params), *params))
        with open(os.path.join(directory, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(images)))
            for iid, q, t, cid, name, pts in images:
                f.write(struct.pack("<i7di", iid, *q, *t, cid))
                f.write(name.encode("utf-8") + b"\0")
                f.write(struct.pack("<Q", len(pts)))
                for x, y, pid in pts:
                    f.write(struct.pack("<ddq", x, y, pid))
        with open(os.path.join(directory, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(points)))
            for pid, xyz, rgb, err, track in points:
                f.write(struct.pack("<Q3d3BdQ", pid, *xyz, *rgb, err, len(track)))
                for iid, idx in track:
                    f.write(struct.pack("<ii", iid, idx))
        return
    with open(os.path.join(directory, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, model, width, height, params in cameras:
            f.write(" ".join([str(cid), model, str(width), str(height)] + [repr(float(p)) for p in params]) + "\n")
    with open(os.path.join(directory, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for iid, q, t, cid, name, pts in images:
            f.write(" ".join([str(iid)] + [repr(float(v)) for v in list(q) + list(t)] + [str(cid), name]) + "\n")
            f.write(" ".join(f"{float(x)!r} {float(y)!r} {pid}" for x, y, pid in pts) + "\n")
    with open(os.path.join(directory, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, xyz, rgb, err, track in points:
            f.write(" ".join([str(pid)] + [repr(float(v)) for v in xyz] + [str(int(v)) for v in rgb] + [repr(float(err))] +
                             [f"{iid} {idx}" for iid, idx in track]) + "\n")


def quat_of(R):
    """(w, x, y, z) of a rotation matrix (the branch for a positive trace; the cases keep their rotations small)."""
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def reader_model(seed=11):
    """A small model for the reader tests: three cameras of different models (one with 12 parameters), five images (one
    without 2-D points, one whose name has a directory), 40 points with tracks of different lengths."""
    rng = np.random.default_rng(seed)
    cameras = [(1, "PINHOLE", 96, 64, [88.5, 90.25, 48.0, 32.0]), (2, "SIMPLE_PINHOLE", 640, 480, [512.125, 320.0, 240.0]),
               (7, "FULL_OPENCV", 800, 600, [float(v) for v in rng.normal(0, 1, 12)])]
    images = []
    for i in range(5):
        q = rng.normal(0, 1, 4)
        q /= np.linalg.norm(q)
        pts = [] if i == 2 else [(float(rng.uniform(0, 96)), float(rng.uniform(0, 64)), int(rng.integers(-1, 40)))
                                 for _ in range(int(rng.integers(1, 6)))]
        name = ("sub/" if i == 3 else "") + f"{(i * 7) % 5:03d}.png"
        images.append((10 + i, [float(v) for v in q], [float(v) for v in rng.normal(0, 2, 3)], (1, 2, 1, 7, 1)[i], name, pts))
    points = []
    for p in range(40):
        track = [(int(rng.integers(10, 15)), int(rng.integers(0, 5))) for _ in range(int(rng.integers(0, 5)))]
        points.append((100 + 3 * p, [float(v) for v in rng.normal(0, 3, 3)], [int(v) for v in rng.integers(0, 256, 3)],
                       float(rng.uniform(0.1, 3.0)), track))
    return cameras, images, points


def scene_model(n_images=4, n_points=300, width=96, height=64, seed=5, names=None, camera_model="PINHOLE"):
    """A dataset-shaped model: n_images PINHOLE views of one camera around n_points points in front of them.  Returns
    (cameras, images, points, Cam list in file order)."""
    rng = np.random.default_rng(seed)
    fx, fy = 95.0, 93.0
    params = [fx, fy, width / 2, height / 2] if camera_model == "PINHOLE" else [fx, width / 2, height / 2]
    cameras = [(1, camera_model, width, height, params)]
    names = [f"{i:03d}" for i in range(n_images)] if names is None else names
    images, cams = [], []
    order = list(rng.permutation(n_images))            # the images file is NOT sorted by name
    for j in order:
        Rc2w = _rotvec(rng.normal(0.0, 0.05, 3))
        centre = rng.normal(0.0, 0.3, 3)
        Rw2c = Rc2w.T
        t = -Rw2c @ centre
        images.append((j + 1, [float(v) for v in quat_of(Rw2c)], [float(v) for v in t], 1, names[j] + ".png", []))
    pts = np.stack([rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.8, 1.8, n_points), rng.uniform(2.0, 8.0, n_points)], 1)
    points = [(p + 1, [float(v) for v in pts[p]], [int(v) for v in rng.integers(0, 256, 3)], float(rng.uniform(0.05, 2.0)), [])
              for p in range(n_points)]
    return cameras, images, points

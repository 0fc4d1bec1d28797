"""Readers for a COLMAP sparse model (`cameras`, `images`, `points3D`, as `.bin` or `.txt`), written from COLMAP's published
model format (https://colmap.github.io/format.html and src/colmap/scene/reconstruction_io), numpy only.

    binary, little endian
      cameras.bin    uint64 count | per camera: int32 id, int32 model id, uint64 width, uint64 height, float64 params[n(model)]
      images.bin     uint64 count | per image: int32 id, float64 qvec[4] (w x y z), float64 tvec[3], int32 camera id,
                     the name as a NUL-terminated string, uint64 count2D, per 2-D point float64 x, float64 y, int64 point3D id
      points3D.bin   uint64 count | per point: uint64 id, float64 xyz[3], uint8 rgb[3], float64 error, uint64 track length,
                     per track element int32 image id, int32 point2D index
    text ('#' starts a comment line)
      cameras.txt    CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]
      images.txt     two lines per image: IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME / POINTS2D[] as (X, Y, POINT3D_ID)
                     (the second line may be empty)
      points3D.txt   POINT3D_ID X Y Z R G B ERROR TRACK[] as (IMAGE_ID, POINT2D_IDX)

(qvec, tvec) is the world-to-camera transform: x_cam = R(qvec) x_world + tvec.  Every camera model's parameter count is
parsed; which models a scene may use is the scene loader's decision (deblurgs_amd/scene.py)."""
import os
import struct
from collections import namedtuple

import numpy as np

# model id -> (name, number of parameters): COLMAP's src/colmap/sensor/models.h
CAMERA_MODELS = {
    0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
    5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
    9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12),
}
MODEL_PARAMS = {name: n for name, n in CAMERA_MODELS.values()}
MODEL_IDS = {name: i for i, (name, _) in CAMERA_MODELS.items()}

Camera = namedtuple("Camera", "id model width height params")
Image = namedtuple("Image", "id qvec tvec camera_id name xys point3D_ids")
Points3D = namedtuple("Points3D", "ids xyz rgb error")
Points3D.__doc__ = "ids int64 [n], xyz float64 [n,3], rgb float64 [n,3] (0..255), error float64 [n,1]; the tracks are skipped"


def qvec2rotmat(qvec):
    """The rotation matrix of a unit quaternion (w, x, y, z), float64 [3,3]."""
    w, x, y, z = (float(v) for v in qvec)
    return np.array([
        [1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
        [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
        [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


class _Bytes:
    def __init__(self, path):
        with open(path, "rb") as f:
            self.data = f.read()
        self.pos = 0
        self.path = path

    def take(self, fmt):
        size = struct.calcsize("<" + fmt)
        if self.pos + size > len(self.data):
            raise ValueError(f"{self.path}: truncated (wanted {size} bytes at offset {self.pos} of {len(self.data)})")
        out = struct.unpack_from("<" + fmt, self.data, self.pos)
        self.pos += size
        return out

    def array(self, dtype, count):
        dtype = np.dtype(dtype)
        size = dtype.itemsize * count
        if self.pos + size > len(self.data):
            raise ValueError(f"{self.path}: truncated (wanted {size} bytes at offset {self.pos} of {len(self.data)})")
        out = np.frombuffer(self.data, dtype=dtype, count=count, offset=self.pos)
        self.pos += size
        return out

    def cstring(self):
        end = self.data.find(b"\0", self.pos)
        if end < 0:
            raise ValueError(f"{self.path}: unterminated name at offset {self.pos}")
        out = self.data[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return out


def _lines(path):
    with open(path, "r") as f:
        for line in f:
            yield line.strip()


# ------------------------------------------------------------------------------------------------- cameras
def read_cameras_binary(path):
    b = _Bytes(path)
    cameras = {}
    for _ in range(b.take("Q")[0]):
        cam_id, model_id, width, height = b.take("iiQQ")
        if model_id not in CAMERA_MODELS:
            raise ValueError(f"{path}: unknown camera model id {model_id}")
        name, n = CAMERA_MODELS[model_id]
        cameras[cam_id] = Camera(cam_id, name, int(width), int(height), np.array(b.take("d" * n)))
    return cameras


def read_cameras_text(path):
    cameras = {}
    for line in _lines(path):
        if not line or line.startswith("#"):
            continue
        e = line.split()
        if e[1] not in MODEL_PARAMS:
            raise ValueError(f"{path}: unknown camera model {e[1]!r}")
        params = np.array([float(v) for v in e[4:]])
        if len(params) != MODEL_PARAMS[e[1]]:
            raise ValueError(f"{path}: {e[1]} takes {MODEL_PARAMS[e[1]]} parameters, the line has {len(params)}")
        cameras[int(e[0])] = Camera(int(e[0]), e[1], int(e[2]), int(e[3]), params)
    return cameras


# ------------------------------------------------------------------------------------------------- images
def read_images_binary(path):
    b = _Bytes(path)
    images = {}
    pt = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
    for _ in range(b.take("Q")[0]):
        p = b.take("idddddddi")
        name = b.cstring()
        pts = b.array(pt, b.take("Q")[0])
        images[p[0]] = Image(p[0], np.array(p[1:5]), np.array(p[5:8]), p[8], name,
                             np.stack([pts["x"], pts["y"]], axis=1), pts["id"].astype(np.int64))
    return images


def read_images_text(path):
    images = {}
    lines = [ln for ln in _lines(path) if not ln.startswith("#")]
    while lines and not lines[-1]:
        lines.pop()
    i = 0
    while i < len(lines):
        if not lines[i]:             # blank separators between records
            i += 1
            continue
        e = lines[i].split()
        pts = lines[i + 1].split() if i + 1 < len(lines) else []
        i += 2
        xys = np.array([[float(x), float(y)] for x, y in zip(pts[0::3], pts[1::3])]).reshape(-1, 2)
        ids = np.array([int(v) for v in pts[2::3]], dtype=np.int64)
        images[int(e[0])] = Image(int(e[0]), np.array([float(v) for v in e[1:5]]), np.array([float(v) for v in e[5:8]]),
                                  int(e[8]), " ".join(e[9:]), xys, ids)
    return images


# ------------------------------------------------------------------------------------------------- points
def read_points3D_binary(path):
    b = _Bytes(path)
    n = b.take("Q")[0]
    ids, xyz = np.empty(n, np.int64), np.empty((n, 3))
    rgb, error = np.empty((n, 3)), np.empty((n, 1))
    for i in range(n):
        p = b.take("QdddBBBdQ")
        ids[i], xyz[i], rgb[i], error[i, 0] = p[0], p[1:4], p[4:7], p[7]
        b.array("<i4", 2 * p[8])                                  # the track
    return Points3D(ids, xyz, rgb, error)


def read_points3D_text(path):
    rows = [ln.split() for ln in _lines(path) if ln and not ln.startswith("#")]
    n = len(rows)
    ids, xyz = np.empty(n, np.int64), np.empty((n, 3))
    rgb, error = np.empty((n, 3)), np.empty((n, 1))
    for i, e in enumerate(rows):
        ids[i] = int(e[0])
        xyz[i] = [float(v) for v in e[1:4]]
        rgb[i] = [int(v) for v in e[4:7]]
        error[i, 0] = float(e[7])
    return Points3D(ids, xyz, rgb, error)


# ------------------------------------------------------------------------------------------------- a model directory
def _either(directory, stem, binary, text):
    """`.bin` first, `.txt` when the binary file is missing or does not parse (readColmapSceneInfo:217-226, 261-264)."""
    try:
        return binary(os.path.join(directory, stem + ".bin"))
    except (OSError, ValueError, struct.error):
        path = os.path.join(directory, stem + ".txt")
        if not os.path.exists(path):
            raise FileNotFoundError(f"neither {stem}.bin nor {stem}.txt can be read in {directory}")
        return text(path)


def read_model(directory):
    """(cameras {id: Camera}, images {id: Image}, Points3D) of a sparse model directory (`<scene>/sparse/0`)."""
    return (_either(directory, "cameras", read_cameras_binary, read_cameras_text),
            _either(directory, "images", read_images_binary, read_images_text),
            _either(directory, "points3D", read_points3D_binary, read_points3D_text))

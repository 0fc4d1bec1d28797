"""Regenerates tests/golden/scene_golden.npz by RUNNING the reference's scene-loading helpers and Pillow on the CPU:

    scene/colmap_loader.py      read_*_binary / read_*_text on the small model tests/scene_cases.py writes
    scene/dataset_readers.py    get_bds (float64) on the bounds cases, getNerfppNorm with and without points
    scene/pcd_init.py           random_pcd_init after np.random.seed(3)
    utils/camera_utils.py       loadCam's resolution for scene_cases.RESOLUTION_TABLE
    PIL                         Image.resize of the seeded resize inputs (only the outputs are stored)

Needs the reference checkout (DGS_REFERENCE, default /root/reference) and PIL.  The reference's modules are imported by path:
`scene` is registered as a bare package (its __init__ pulls in the CUDA extensions), and the modules this image lacks and
that are not on these paths (plyfile, open3d, cv2) get empty import shims, scene.gaussian_model a minimal BasicPointCloud.
The fixture is data only.
    python tests/golden/make_golden_scene.py
"""
import os
import sys
import tempfile
import types
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DGS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import scene_cases as sc  # noqa: E402


def _shims():
    for name in ("plyfile", "open3d", "cv2"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(REF, "scene")]
    sys.modules["scene"] = pkg
    gm = types.ModuleType("scene.gaussian_model")
    gm.BasicPointCloud = namedtuple("BasicPointCloud", "points colors normals")
    sys.modules["scene.gaussian_model"] = gm
    sys.path.insert(0, REF)


class _Stop(Exception):
    pass


def _resolutions(camera_utils):
    """loadCam up to its PILtoTorch call, whose `resolution` argument is what is recorded."""
    seen = []

    def record(image, resolution):
        seen.append(resolution)
        raise _Stop()
    camera_utils.PILtoTorch = record
    Info = namedtuple("Info", "image depth")
    Img = namedtuple("Img", "size")
    for w, h, r in sc.RESOLUTION_TABLE:
        try:
            camera_utils.loadCam(types.SimpleNamespace(resolution=r), 0, Info(Img((w, h)), None), 1.0)
        except _Stop:
            pass
    return np.array(seen, dtype=np.int64)


def _parse(out, prefix, cameras=None, images=None, points=None):
    if cameras is not None:
        ids = list(cameras)
        out[prefix + "cam_ids"] = np.array(ids, dtype=np.int64)
        out[prefix + "cam_models"] = np.array([cameras[i].model for i in ids])
        out[prefix + "cam_sizes"] = np.array([[cameras[i].width, cameras[i].height] for i in ids], dtype=np.int64)
        out[prefix + "cam_params"] = np.concatenate([np.asarray(cameras[i].params, dtype=np.float64) for i in ids])
    if images is not None:
        ids = list(images)
        out[prefix + "img_ids"] = np.array(ids, dtype=np.int64)
        out[prefix + "img_qvec"] = np.stack([images[i].qvec for i in ids])
        out[prefix + "img_tvec"] = np.stack([images[i].tvec for i in ids])
        out[prefix + "img_cam"] = np.array([images[i].camera_id for i in ids], dtype=np.int64)
        out[prefix + "img_names"] = np.array([images[i].name for i in ids])
        out[prefix + "img_npts"] = np.array([len(images[i].point3D_ids) for i in ids], dtype=np.int64)
        out[prefix + "img_xys"] = np.concatenate([np.asarray(images[i].xys, dtype=np.float64).reshape(-1, 2) for i in ids])
        out[prefix + "img_pids"] = np.concatenate([np.asarray(images[i].point3D_ids, dtype=np.int64).reshape(-1) for i in ids])
    if points is not None:
        out[prefix + "pts_xyz"], out[prefix + "pts_rgb"], out[prefix + "pts_err"] = points


def main():
    import PIL
    from PIL import Image
    _shims()
    import scene.colmap_loader as cl
    import scene.dataset_readers as dr
    import scene.pcd_init as pi
    import utils.camera_utils as cu
    out = {"pillow_version": np.array(PIL.__version__), "numpy_version": np.array(np.__version__)}

    # ---- the readers
    cameras, images, points = sc.reader_model()
    with tempfile.TemporaryDirectory() as d:
        sc.write_model(d, cameras, images, points, binary=True)
        _parse(out, "bin_", cl.read_intrinsics_binary(os.path.join(d, "cameras.bin")),
               cl.read_extrinsics_binary(os.path.join(d, "images.bin")), cl.read_points3D_binary(os.path.join(d, "points3D.bin")))
        sc.write_model(d, cameras, images, points, binary=False)
        _parse(out, "txt_", None, cl.read_extrinsics_text(os.path.join(d, "images.txt")),
               cl.read_points3D_text(os.path.join(d, "points3D.txt")))
        # (the reference's text reader of the cameras accepts PINHOLE alone)
        sc.write_model(d, [c for c in cameras if c[1] == "PINHOLE"], images, points, binary=False)
        _parse(out, "txt_", cl.read_intrinsics_text(os.path.join(d, "cameras.txt")))
    out["qvec_rotmat"] = np.stack([cl.qvec2rotmat(np.asarray(im[1])) for im in images])

    # ---- depth bounds, scene radius, random initialisation
    for case in sc.bounds_cases():
        out["bds_" + case.name] = dr.get_bds(case.cams, case.points)
    cams = sc.make_cameras(7, 90)
    pts32 = np.random.default_rng(91).normal(0.0, 2.0, (400, 3)).astype(np.float32)
    pcd = dr.BasicPointCloud(points=pts32, colors=None, normals=None)
    out["radius_centers"] = np.stack([np.linalg.inv(dr.getWorld2View2(c.R, c.T))[:3, 3] for c in cams])
    out["radius_points"] = np.asarray(dr.getNerfppNorm(cams, pcd)["radius"])
    out["radius_cameras"] = np.asarray(dr.getNerfppNorm(cams, None)["radius"])
    bds = np.stack([np.linspace(0.5, 1.5, 7), np.linspace(4.0, 9.0, 7)], axis=1)
    np.random.seed(3)
    out["random_pcd_bds"] = pi.random_pcd_init(cams, near=1.2, far=6.0, num_pcd=900, bds=bds)
    np.random.seed(3)
    out["random_pcd_plain"] = pi.random_pcd_init(cams[:3], near=2.0, far=8.0, num_pcd=300)

    # ---- resolution rule and Pillow's resize
    out["resolutions"] = _resolutions(cu)
    for case in sc.RESIZE_CASES:
        x = sc.resize_input(case)
        res = [np.asarray(Image.fromarray(x[g] if case.C == 3 else x[g, :, :, 0]).resize((case.w, case.h)))
               for g in range(case.G)]
        out["resize_" + case.name] = np.stack(res).reshape(case.G, case.h, case.w, case.C)
    path = os.path.join(HERE, "scene_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

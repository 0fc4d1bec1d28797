"""Regenerates tests/golden/blender_golden.npz on the CPU:

    over_black / over_white   the Blender reader's composite (scene/dataset_readers.py:335-341) over all 256 x 256 (alpha,
                              colour) pairs, evaluated by numpy in float64 as tests/blender_cases.py restates it
    rgba_<case>               PIL's own Image.resize of the seeded RGBA inputs (only the outputs are stored)
    cam_R, cam_T, cam_fov     what a small transforms file means (the restatement of readCamerasFromTransforms)
    cloud_xyz, cloud_rgb      readNerfSyntheticInfo's random initialisation after np.random.seed(7): the reference's own
                              random_pcd_init (scene/pcd_init.py), then the colour draw, in that order

The composite cannot be taken from the reference by running it: Pillow 12.2 refuses `Image.fromarray(int8 array, "RGB")`
with a TypeError, where the reference's environment accepts it and takes the raw bytes -- hence `.view(np.uint8)`.
Needs PIL and, for the random points, the reference checkout (DGS_REFERENCE, default /root/reference), imported by path as
make_golden_scene.py does.  The fixture is data only.
    python tests/golden/make_golden_blender.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DGS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import blender_cases as bc  # noqa: E402
import scene_cases as sc  # noqa: E402

C0 = 0.28209479177387814
CLOUD_SEED, CLOUD_POINTS = 7, 3000


def golden_cameras():
    """The Cam tuples of blender_frames(4, 40) for 40 x 32 pictures (not square: FovY differs from FovX)."""
    frames = bc.blender_frames(4, 40)
    R, T, fov_x, fov_y = bc.cameras_restated(frames, bc.CAMERA_ANGLE_X, 40, 32)
    return [sc.Cam(i, R[i], T[i], fov_y, fov_x, "", f"r_{i}", 40, 32) for i in range(4)], (R, T, fov_x, fov_y)


def main():
    import PIL
    from PIL import Image
    out = {"pillow_version": np.array(PIL.__version__), "numpy_version": np.array(np.__version__)}
    out["over_black"], out["over_white"] = bc.over_table(False), bc.over_table(True)
    try:
        Image.fromarray(np.zeros((2, 2, 3), np.int8), "RGB")
        print("note: this Pillow accepts int8 RGB arrays")
    except TypeError:
        pass
    for case in bc.RGBA_CASES:
        x = bc.rgba_input(case)
        out["rgba_" + case.name] = np.stack([np.asarray(Image.fromarray(x[g], "RGBA").resize((case.w, case.h)))
                                             for g in range(case.G)])
    cams, (R, T, fov_x, fov_y) = golden_cameras()
    out["cam_R"], out["cam_T"], out["cam_fov"] = R, T, np.array([fov_x, fov_y])

    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(REF, "scene")]
    sys.modules["scene"] = pkg
    sys.path.insert(0, REF)
    import scene.pcd_init as pi
    np.random.seed(CLOUD_SEED)
    out["cloud_xyz"] = pi.random_pcd_init(cams, near=2.0, far=8.0, num_pcd=CLOUD_POINTS)
    shs = np.random.random((CLOUD_POINTS, 3)) / 255.0
    out["cloud_rgb"] = (shs * C0 + 0.5) * 255
    path = os.path.join(HERE, "blender_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Regenerates tests/golden/paths_golden.npz by IMPORTING the reference's own path helpers from /root/reference:
utils/mvg_utils.py (mean_camera_pose, get_c2w_from_eye), utils/export_utils.py (center_crop_with_ratio) and matplotlib's
jet_r table as depth_colorize reads it.

Run in the build container only (the reference never travels to the GPU box); needs scipy and matplotlib (made with 3.10):
    python tests/golden/make_golden_paths.py
utils/export_utils.py imports, at module import time, packages that are not on the path of the one function used here
(imageio, and through `scene` the dataset readers' plyfile, ...): every module the import chain misses gets an empty
stand-in, and the rasteriser import is satisfied by this package's drop-in shim.
The fixture is data (seeded inputs and the reference's outputs); no reference source text is stored.
"""
import importlib
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

CROP_TABLE = [(5, 7, 1.0), (5, 7, 0.95), (5, 7, 0.5), (37, 53, 1.0), (37, 53, 0.95), (37, 53, 0.5), (64, 128, 1.0),
              (64, 128, 0.95), (64, 128, 0.5), (96, 144, 0.95), (1080, 1920, 0.95), (1080, 1920, 0.5), (1, 1, 0.95),
              (3, 2, 0.5), (401, 599, 0.95), (400, 600, 0.3)]


def import_with_stand_ins(name, tries=40):
    """import `name`, giving every module its import chain cannot find an empty stand-in."""
    for _ in range(tries):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as ex:
            missing = ex.name
            if missing is None or missing == name:
                raise
            print("stand-in for", missing)
            parts = missing.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
        except ImportError as ex:       # `from stand_in import X`
            mod = sys.modules.get(ex.name) if ex.name else None
            if mod is None or getattr(mod, "__file__", None) is not None:
                raise
            mod.__getattr__ = lambda attr: None
    raise RuntimeError(f"could not import {name}")


def random_c2ws(rng, n, spread):
    from scipy.spatial.transform import Rotation
    base = Rotation.from_rotvec(rng.normal(size=3))
    out = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        out[i, :3, :3] = (Rotation.from_rotvec(rng.normal(size=3) * spread) * base).as_matrix()
        out[i, :3, 3] = rng.normal(size=3)
    return out


def main():
    import matplotlib
    sys.path.insert(0, os.path.join(ROOT, "deblurgs_amd", "dropin"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    os.chdir(REF)                       # (export_utils appends os.getcwd() to sys.path)
    mvg = import_with_stand_ins("utils.mvg_utils")
    exp = import_with_stand_ins("utils.export_utils")
    rng = np.random.default_rng(31)
    data = {}
    # ---- mean_camera_pose: tight and wide clusters, one camera, two cameras
    for name, (n, spread) in {"tight": (7, 0.05), "wide": (12, 0.6), "one": (1, 0.3), "two": (2, 0.4)}.items():
        c2ws = random_c2ws(rng, n, spread)
        data[f"mean_{name}_in"] = c2ws
        data[f"mean_{name}_out"] = mvg.mean_camera_pose(c2ws)
    # ---- get_c2w_from_eye
    eyes, lookats, ups = rng.normal(size=(6, 3)), rng.normal(size=(6, 3)) * 3.0, rng.normal(size=(6, 3))
    data["eye_in"] = np.stack([eyes, lookats, ups])
    data["eye_out"] = np.stack([mvg.get_c2w_from_eye(e, l, u) for e, l, u in zip(eyes, lookats, ups)])
    # ---- center_crop_with_ratio: the shape and the first pixel of the crop of an index image -> (h1, h2, w1, w2)
    rows = []
    for H, W, ratio in CROP_TABLE:
        yy, xx = np.mgrid[0:H, 0:W]
        out = exp.center_crop_with_ratio(np.stack([yy, xx], axis=-1), ratio)
        h, w = out.shape[:2]
        h1, w1 = (int(out[0, 0, 0]), int(out[0, 0, 1])) if h and w else (-1, -1)
        rows.append([H, W, h, w, h1, w1])
    data["crop_table"] = np.array(rows, dtype=np.int64)
    data["crop_ratio"] = np.array([r for _, _, r in CROP_TABLE], dtype=np.float64)
    # ---- jet_r as depth_colorize uses it: (cmapper(d) * 255).astype(uint8) at the 256 table entries
    cm = matplotlib.colormaps["jet_r"]
    data["jet_r"] = (cm(np.arange(256)) * 255).astype(np.uint8)
    data["jet_r_bad"] = (np.asarray(cm(np.float32("nan"))) * 255).astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "paths_golden.npz"), **data)
    for k, v in data.items():
        print(k, getattr(v, "shape", None))


if __name__ == "__main__":
    main()

"""Cases shared by tests/test_blender_host.py, tests/test_gpu_blender.py and tests/golden/make_golden_blender.py: the
Blender reader's composite restated in numpy (and its integer and float32 look-alikes), the RGBA resize cases with their
seeded inputs and a numpy restatement of Pillow's RGBA `Image.resize`, and a writer of small NeRF-synthetic directories."""
import json
import math
import os
from collections import namedtuple

import numpy as np

import scene_cases as sc

# ------------------------------------------------------------------------------------------------- the composite
# what differs from the float64 expression in this many of the 65 536 (colour, alpha) pairs (black, white)
FLOOR_DIFFERS = (154, 152)
FLOAT32_DIFFERS = (154, 391)


def over_restated(rgba_u8, white, dtype=np.float64):
    """uint8 [...,3] of uint8 [...,4]: the pixels scaled to 0..1, colour times alpha plus background times (1 - alpha), times
    255, cast to SIGNED bytes (numpy truncates toward zero and keeps the low byte) and read as unsigned ones.  In `dtype`."""
    unit = rgba_u8.astype(dtype) / dtype(255.0)
    bg = np.array([1, 1, 1] if white else [0, 0, 0])
    mixed = unit[..., :3] * unit[..., 3:4] + (bg * (1 - unit[..., 3:4])).astype(dtype)
    with np.errstate(invalid="ignore"):
        return np.array(mixed * dtype(255.0), dtype=np.byte).view(np.uint8)


def over_pairs():
    """uint8 [256,256,4]: alpha along the rows, colour along the columns; the channels carry c, (c + 85) % 256,
    (c + 170) % 256 -- every (colour, alpha) pair three times."""
    a, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([c, (c + 85) % 256, (c + 170) % 256, a], axis=-1).astype(np.uint8)


def over_table(white, dtype=np.float64):
    """uint8 [256 alpha, 256 colour]."""
    return over_restated(over_pairs(), white, dtype)[:, :, 0]


def over_floor_table(white):
    """The exact integer floor (c a + bg 255 (255 - a)) // 255."""
    a, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return ((c * a + (255 if white else 0) * (255 - a)) // 255).astype(np.uint8)


def over_from_table(table, rgba_u8):
    """uint8 [...,3]: the composite of rgba_u8 looked up in a [alpha, colour] table."""
    return table[rgba_u8[..., 3:4], rgba_u8[..., :3]]


# ------------------------------------------------------------------------------------------------- RGBA resize
RgbaCase = namedtuple("RgbaCase", "name H W h w G covers")
RGBA_CASES = [
    RgbaCase("odd", 37, 53, 18, 26, 1, "odd sizes, non-integer ratio"),
    RgbaCase("h_only", 31, 45, 31, 20, 1, "vertical pass skipped: premultiplied at the horizontal load"),
    RgbaCase("v_only", 50, 70, 13, 70, 1, "horizontal pass skipped: premultiplied at the row copy"),
    RgbaCase("upscale", 20, 30, 45, 61, 1, "upscale"),
    RgbaCase("tiles", 135, 240, 68, 120, 2, "crosses tile borders on both axes, misaligned input pointer"),
    RgbaCase("ratio33", 330, 24, 10, 12, 1, "vertical ratio 33: the shrunk tile, with four channels"),
    RgbaCase("same", 8, 8, 8, 8, 1, "same size: a copy, no premultiply round trip"),
]


def rgba_input(case):
    """uint8 [G,H,W,4], seeded by the case's position.  Upper half: a block of alpha 0 (the colour stays noise), a block of
    alpha 255 and a block of noise, each a third of the width.  Lower half: a checkerboard of opaque black blocks and
    blocks of saturated colour under a low alpha (4..40), as large as the positive lobe of the filter -- the negative
    lobes over the opaque blocks pull the resampled alpha below the resampled colour, so `255 c // a` exceeds 255."""
    rng = np.random.default_rng(2000 + [c.name for c in RGBA_CASES].index(case.name))
    img = rng.integers(0, 256, (case.G, case.H, case.W, 4), dtype=np.uint8)
    H, W = case.H, case.W
    img[:, :H // 2, :W // 3, 3] = 0
    img[:, :H // 2, W // 3:2 * W // 3, 3] = 255
    run_w = min(2 * max(1, int(round(W / case.w))), max(1, W // 3))
    run_h = min(2 * max(1, int(round(H / case.h))), max(1, H // 3))
    y, x = np.meshgrid(np.arange(H // 2, H), np.arange(W), indexing="ij")
    faint = ((y // run_h + x // run_w) % 2 == 1)
    low = rng.integers(4, 41, (case.G,) + faint.shape, dtype=np.uint8)
    lower = img[:, H // 2:]
    lower[:, ~faint] = (0, 0, 0, 255)
    lower[:, faint, :3] = 255
    lower[:, :, :, 3] = np.where(faint[None], low, lower[:, :, :, 3])
    if case.name == "same":
        img[0, 0, 0] = (9, 8, 7, 0)                     # a colour under alpha 0: a premultiply round trip would zero it
    return img


def premultiply(rgba_u8):
    x = rgba_u8.astype(np.int64)
    t = x[..., :3] * x[..., 3:4] + 128
    x[..., :3] = ((t >> 8) + t) >> 8
    return x


def unpremultiply(x, clipped=None):
    """int64 [...,4] -> uint8: the colour copied where alpha is 0 or 255, else min(255, 255 c // a); clipped[0] counts the
    colour bytes the min changes."""
    x = np.asarray(x).astype(np.int64)
    a = x[..., 3:4]
    q = 255 * x[..., :3] // np.maximum(a, 1)
    plain = (a == 0) | (a == 255)
    if clipped is not None:
        clipped[0] += int(((q > 255) & ~plain).sum())
    out = x.copy()
    out[..., :3] = np.where(plain, x[..., :3], np.minimum(q, 255))
    return out.astype(np.uint8)


def resize_rgba_restated(rgba_u8, size, clipped=None):
    """Pillow's Image.resize(size) of uint8 [G,H,W,4] RGBA images: a copy when the size does not change; otherwise
    premultiplied, the four bytes resampled by the 8-bit bicubic (scene_cases.resize_restated), un-premultiplied."""
    w, h = size
    if (rgba_u8.shape[2], rgba_u8.shape[1]) == (w, h):
        return rgba_u8.copy()
    return unpremultiply(sc.resize_restated(premultiply(rgba_u8), size), clipped)


def rgba_counts(out_u8):
    """(pixels of alpha 0, of alpha 255, of an alpha in between) of a result."""
    a = out_u8[..., 3]
    return int((a == 0).sum()), int((a == 255).sum()), int(((a > 0) & (a < 255)).sum())


# ------------------------------------------------------------------------------------------------- Blender directories
CAMERA_ANGLE_X = 0.6911112070083618


def blender_frames(n, seed, split="train"):
    """n frames of a transforms file: cameras on a sphere of radius 4 around the origin looking at it, in Blender's axes
    (x right, y up, z BACK), as nested lists."""
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n):
        d = np.array([rng.normal(0.0, 0.25), rng.normal(0.0, 0.25), 1.0])
        z = d / np.linalg.norm(d)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, 4.0 * z
        frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.012566370614359171,
                       "transform_matrix": [[float(v) for v in row] for row in c2w]})
    return frames


def cameras_restated(frames, angle_x, width, height):
    """(R [n,3,3], T [n,3], FovX, FovY) a transforms file means: the y and z columns of the camera-to-world matrix negated,
    the matrix inverted; R the transposed rotation of the inverse, T its translation; FovY from FovX's focal length."""
    R, T = [], []
    for f in frames:
        c2w = np.array(f["transform_matrix"])
        c2w[:3, 1:3] *= -1
        w2c = np.linalg.inv(c2w)
        R.append(np.transpose(w2c[:3, :3]))
        T.append(w2c[:3, 3])
    focal = width / (2 * math.tan(angle_x / 2))
    return np.stack(R), np.stack(T), angle_x, 2 * math.atan(height / (2 * focal))


def blender_image(seed, H=32, W=40):
    """uint8 [H,W,4]: noise, a block of alpha 0 and a block of alpha 255."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    img[:H // 3, :W // 2, 3] = 0
    img[H // 3:2 * H // 3, W // 2:, 3] = 255
    return img


def write_blender_dir(root, n_train=4, n_test=2, H=32, W=40, seed=40, rgb_views=()):
    """A NeRF-synthetic directory with .npy pictures; returns {image name: uint8 [H,W,4]} per split.  The views named in
    rgb_views are stored as RGB (their alpha dropped)."""
    root = str(root)
    out = {}
    for split, n, s in (("train", n_train, seed), ("test", n_test, seed + 1)):
        frames = blender_frames(n, s, split)
        os.makedirs(os.path.join(root, split), exist_ok=True)
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": CAMERA_ANGLE_X, "frames": frames}, f)
        out[split] = {}
        for i in range(n):
            img = blender_image(1000 * s + i, H, W)
            name = f"r_{i}"
            np.save(os.path.join(root, split, name + ".npy"), img[:, :, :3] if (split, name) in rgb_views else img)
            out[split][name] = img
    return out

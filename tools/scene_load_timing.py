"""Times the two device parts of scene loading (deblurgs_amd/scene.py) beside the host code they replace:

    resize   scene.resize_images of 30 images, 3840 x 2160 -> 1600 x 900 and 1920 x 1080 -> 960 x 540, written as floats into
             a ground-truth stack -- (a) the kernel alone (device events around the launch, images already on the device) and
             (b) the upload of the 8-bit sources + the kernel -- against the reference's route per image: PIL Image.resize,
             torch.from_numpy(..) / 255.0, permute, upload of the floats (host clock, ending in a synchronise).  The kernel's
             bytes are compared with PIL's on the first image.
    bounds   scene.depth_bounds at 100 cameras x 200 000 points (host clock around the whole call, its uploads, one read of
             the counts and one of the order statistics included) against a numpy restatement of get_bds in float64.

The median of `--reps` after one warm-up.  Without PIL the host arm of `resize` is reported as not measured.  Each leg is
measured by a child process of its own under `timeout`; if one fails, faults or runs out of time nothing more is started on the
device and the JSON says so.

    python tools/scene_load_timing.py [--out profiles/scene_load_timing.json]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

RESIZE_LEGS = {"resize_4k": (2160, 3840, 900, 1600), "resize_1080p": (1080, 1920, 540, 960)}
LEGS = tuple(RESIZE_LEGS) + ("bounds",)


def _median_ms(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def measure_resize(leg, images, reps):
    import numpy as np
    import torch
    from deblurgs_amd import scene
    H, W, h, w = RESIZE_LEGS[leg]
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3), dtype=np.uint8).repeat(8, axis=0).repeat(8, axis=1)[:H, :W]
    src = np.stack([np.roll(base, 7 * i, axis=1) ^ np.uint8(i) for i in range(images)])      # [n,H,W,3], distinct images
    stack = torch.empty((images, 3, h, w), dtype=torch.float32, device="cuda")
    dev = torch.from_numpy(src).cuda()
    sync = torch.cuda.synchronize
    res = {"images": images, "in": [H, W], "out": [h, w], "reps": reps, "device": torch.cuda.get_device_name(0), "ms": {}}

    scene.resize_images(dev, (w, h), out=stack)
    sync()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        scene.resize_images(dev, (w, h), out=stack)
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    res["ms"]["kernel"] = statistics.median(ev)
    res["ms"]["upload_u8_and_kernel"] = _median_ms(lambda: scene.resize_images(torch.from_numpy(src).cuda(), (w, h), out=stack),
                                                   reps, sync)
    # bytes the kernel has to move at least: the 8-bit sources in, the floats out
    res["min_bytes"] = int(src.size + stack.numel() * 4)
    res["kernel_GBps_of_min_bytes"] = res["min_bytes"] / (res["ms"]["kernel"] * 1e-3) / 1e9
    try:
        from PIL import Image
    except ImportError:
        res["ms"]["pil_route"] = None
        res["note"] = "PIL is not importable: the host arm is not measured"
        return res
    pil = [Image.fromarray(s) for s in src]

    def host_route():
        for i, im in enumerate(pil):
            t = torch.from_numpy(np.array(im.resize((w, h)))) / 255.0
            stack[i] = t.permute(2, 0, 1).cuda()
    res["ms"]["pil_route"] = _median_ms(host_route, max(1, reps // 2), sync)
    first = torch.from_numpy(np.array(pil[0].resize((w, h))))
    got = scene.resize_images(dev[:1], (w, h), out_u8=torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda"))
    res["equals_pil"] = bool(torch.equal(got[0].cpu(), first))
    return res


def _numpy_get_bds(cams, pcd):
    """get_bds (scene/dataset_readers.py:164-209) restated with its numpy expressions, float64."""
    import numpy as np
    h, w = cams[0].height, cams[0].width
    fx = w / (2 * math.tan(cams[0].FovX / 2))
    fy = h / (2 * math.tan(cams[0].FovY / 2))
    K = np.array([[fx, 0.0, w / 2], [0.0, fy, h / 2], [0.0, 0.0, 1.0]])
    bds = []
    for c in cams:
        w2c = np.eye(4)
        w2c[:3, :3] = c.R.T
        w2c[:3, 3] = c.T
        homog = np.pad(pcd, ((0, 0), (0, 1)), mode="constant", constant_values=1.0)
        cam = (homog @ w2c.T)[:, :3]
        depths = cam[:, 2]
        valid = depths > 0.01
        pix = cam @ np.linalg.inv(K)
        pix = pix[:, :2] / pix[:, 2:]
        valid = valid & (pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h)
        d = depths[valid]
        bds.append([np.percentile(d, 0.1), np.percentile(d, 99.9)])
    return np.array(bds)


def measure_bounds(cameras, points, reps):
    import numpy as np
    import torch
    from deblurgs_amd import scene
    rng = np.random.default_rng(1)
    cams = []
    for i in range(cameras):
        v = rng.normal(0.0, 0.2, 3)
        t = np.linalg.norm(v)
        k = v / t
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + math.sin(t) * Kx + (1 - math.cos(t)) * (Kx @ Kx)
        cams.append(scene.CameraInfo(1, R, -R.T @ rng.normal(0.0, 0.5, 3), 0.8, 1.1, "", f"{i:04d}", 1600, 900))
    pcd = np.stack([rng.normal(0, 3, points), rng.normal(0, 3, points), rng.uniform(-2, 20, points)], axis=1)
    res = {"cameras": cameras, "points": points, "reps": reps, "device": torch.cuda.get_device_name(0), "ms": {}}
    res["ms"]["depth_bounds"] = _median_ms(lambda: scene.depth_bounds(cams, pcd), reps, torch.cuda.synchronize)
    res["ms"]["numpy_get_bds"] = _median_ms(lambda: _numpy_get_bds(cams, pcd), max(1, reps // 2), lambda: None)
    got, want = scene.depth_bounds(cams, pcd), _numpy_get_bds(cams, pcd)
    res["max_abs_diff_over_far"] = float((np.abs(got - want) / want[:, 1:2]).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=30)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_load_timing.json"))
    ap.add_argument("--leg", default="", help="internal: measure this leg in this process and print the JSON")
    a = ap.parse_args()
    if a.leg:
        res = measure_bounds(a.cameras, a.points, a.reps) if a.leg == "bounds" else measure_resize(a.leg, a.images, a.reps)
        print("SCENE_LOAD_TIMING_JSON " + json.dumps(res), flush=True)
        return 0
    result = {"note": "one box, one run", "legs": {}}
    ok = True
    for leg in LEGS:                 # (this process never opens the device)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--images",
               str(a.images), "--cameras", str(a.cameras), "--points", str(a.points), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SCENE_LOAD_TIMING_JSON ")]
        ok = r.returncode == 0 and bool(lines)
        if not ok:                   # nothing more is started on the device
            result["legs"][leg] = {"failed": r.returncode, "stderr": r.stderr[-2000:]}
            break
        result["legs"][leg] = json.loads(lines[-1][len("SCENE_LOAD_TIMING_JSON "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

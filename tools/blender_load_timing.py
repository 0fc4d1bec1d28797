"""Times the device route of Blender scene loading and of the RGBA resize (deblurgs_amd/scene.py) beside the host code they
replace, ms per stage with the upload apart:

    blender_r1, blender_r2   100 RGBA pictures of 800 x 800 at resolution 1 and 2.  Device: the upload of the 8-bit RGBA
                 sources (host clock, ending in a synchronise), scene.rgba_over (device events) and -- at resolution 2 --
                 scene.resize_images of the composited bytes (device events): two launches with a 3 byte / pixel
                 intermediate.  Host, per picture as the reference does it: the float64 numpy composite and its cast to
                 bytes, PIL Image.resize, torch.from_numpy(..) / 255.0, permute, upload of the floats.
    rgba_resize  30 RGBA pictures of 1920 x 1080 -> 960 x 540: scene.resize_rgba_images (device events; the upload apart)
                 against PIL Image.resize, / 255.0, permute, upload per picture.

The first picture's device bytes are compared with the host route's.  The median of `--reps` after one warm-up; no
threshold.  Without PIL the host arms are reported as not measured.  Each leg is measured by a child process of its own under
`timeout`; if one fails, faults or runs out of time nothing more is started on the device and the JSON says so.

    python tools/blender_load_timing.py [--out profiles/blender_load_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

LEGS = ("blender_r1", "blender_r2", "rgba_resize")
TAG = "BLENDER_LOAD_TIMING_JSON "


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


def _event_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    return statistics.median(ev)


def _pictures(n, H, W):
    """uint8 [n,H,W,4]: distinct pictures of blocky noise, with blocks of alpha 0 and of alpha 255."""
    import numpy as np
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 4), dtype=np.uint8).repeat(8, axis=0).repeat(8, axis=1)[:H, :W]
    base[:H // 4, :, 3] = 0
    base[H // 4:H // 2, :, 3] = 255
    return np.stack([np.roll(base, 7 * i, axis=1) ^ np.uint8(i) for i in range(n)])


def _host_composite(img, white):
    import numpy as np
    unit = img / 255.0
    bg = np.array([1, 1, 1]) if white else np.array([0, 0, 0])
    mixed = unit[:, :, :3] * unit[:, :, 3:4] + bg * (1 - unit[:, :, 3:4])
    return np.array(mixed * 255.0, dtype=np.byte).view(np.uint8)


def measure_blender(resolution, images, reps, white=True):
    import numpy as np
    import torch
    from deblurgs_amd import scene
    H = W = 800
    w, h = scene.training_resolution(W, H, resolution)
    src = _pictures(images, H, W)
    stack = torch.empty((images, 3, h, w), dtype=torch.float32, device="cuda")
    sync = torch.cuda.synchronize
    res = {"images": images, "in": [H, W], "out": [h, w], "reps": reps, "device": torch.cuda.get_device_name(0), "ms": {}}
    res["ms"]["upload_rgba_u8"] = _median_ms(lambda: torch.from_numpy(src).cuda(), reps, sync)
    dev = torch.from_numpy(src).cuda()
    if (w, h) == (W, H):
        res["ms"]["composite_kernel"] = _event_ms(lambda: scene.rgba_over(dev, white, out=stack), reps)

        def device_route():
            scene.rgba_over(torch.from_numpy(src).cuda(), white, out=stack)
    else:
        mid = torch.empty((images, H, W, 3), dtype=torch.uint8, device="cuda")
        res["ms"]["composite_kernel"] = _event_ms(lambda: scene.rgba_over(dev, white, out_u8=mid), reps)
        res["ms"]["resize_kernel"] = _event_ms(lambda: scene.resize_images(mid, (w, h), out=stack), reps)

        def device_route():
            scene.resize_images(scene.rgba_over(torch.from_numpy(src).cuda(), white, out_u8=mid), (w, h), out=stack)
    res["ms"]["device_route"] = _median_ms(device_route, reps, sync)
    res["composite_min_bytes"] = int(src.size + (stack.numel() * 4 if (w, h) == (W, H) else src.size // 4 * 3))
    res["composite_GBps_of_min_bytes"] = res["composite_min_bytes"] / (res["ms"]["composite_kernel"] * 1e-3) / 1e9
    device_first = stack[0].cpu()
    try:
        from PIL import Image
    except ImportError:
        res["ms"]["host_route"] = None
        res["note"] = "PIL is not importable: the host arm is not measured"
        return res

    def host_route():
        for i in range(images):
            im = Image.fromarray(_host_composite(src[i], white), "RGB").resize((w, h))
            stack[i] = (torch.from_numpy(np.array(im)) / 255.0).permute(2, 0, 1).cuda()
    res["ms"]["host_route"] = _median_ms(host_route, max(1, reps // 2), sync)
    res["equals_host_route"] = bool(torch.equal(stack[0].cpu(), device_first))
    return res


def measure_rgba_resize(images, reps):
    import numpy as np
    import torch
    from deblurgs_amd import scene
    H, W, h, w = 1080, 1920, 540, 960
    src = _pictures(images, H, W)
    stack = torch.empty((images, 4, h, w), dtype=torch.float32, device="cuda")
    sync = torch.cuda.synchronize
    res = {"images": images, "in": [H, W], "out": [h, w], "reps": reps, "device": torch.cuda.get_device_name(0), "ms": {}}
    res["ms"]["upload_rgba_u8"] = _median_ms(lambda: torch.from_numpy(src).cuda(), reps, sync)
    dev = torch.from_numpy(src).cuda()
    res["ms"]["kernel"] = _event_ms(lambda: scene.resize_rgba_images(dev, (w, h), out=stack), reps)
    res["ms"]["device_route"] = _median_ms(lambda: scene.resize_rgba_images(torch.from_numpy(src).cuda(), (w, h), out=stack),
                                           reps, sync)
    res["min_bytes"] = int(src.size + stack.numel() * 4)
    res["kernel_GBps_of_min_bytes"] = res["min_bytes"] / (res["ms"]["kernel"] * 1e-3) / 1e9
    device_first = stack[0].cpu()
    try:
        from PIL import Image
    except ImportError:
        res["ms"]["pil_route"] = None
        res["note"] = "PIL is not importable: the host arm is not measured"
        return res
    pil = [Image.fromarray(s, "RGBA") for s in src]

    def host_route():
        for i, im in enumerate(pil):
            stack[i] = (torch.from_numpy(np.array(im.resize((w, h)))) / 255.0).permute(2, 0, 1).cuda()
    res["ms"]["pil_route"] = _median_ms(host_route, max(1, reps // 2), sync)
    res["equals_pil"] = bool(torch.equal(stack[0].cpu(), device_first))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blender-images", type=int, default=100)
    ap.add_argument("--resize-images", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blender_load_timing.json"))
    ap.add_argument("--leg", default="", help="internal: measure this leg in this process and print the JSON")
    a = ap.parse_args()
    if a.leg:
        res = measure_rgba_resize(a.resize_images, a.reps) if a.leg == "rgba_resize" else \
            measure_blender(1 if a.leg == "blender_r1" else 2, a.blender_images, a.reps)
        print(TAG + json.dumps(res), flush=True)
        return 0
    result = {"note": "one box, one run", "legs": {}}
    ok = True
    for leg in LEGS:                 # (this process never opens the device)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--blender-images",
               str(a.blender_images), "--resize-images", str(a.resize_images), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        ok = r.returncode == 0 and bool(lines)
        if not ok:                   # nothing more is started on the device
            result["legs"][leg] = {"failed": r.returncode, "stderr": r.stderr[-2000:]}
            break
        result["legs"][leg] = json.loads(lines[-1][len(TAG):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

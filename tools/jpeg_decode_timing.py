"""Times the device JPEG decoder (deblurgs_amd/jpeg.py decode, scene.load_colmap_scene(device_jpeg=True)) on an MI355X
against the host route on the same box: PIL's decoder and the upload of the raw pixels.

Pictures: 30 different 1920 x 1080 RGB images (smooth structure plus mild noise, seeded), as three kinds of file at quality
90, 4:2:0:

    device_encoder   what jpeg.encode writes: one restart interval per MCU row (68 intervals: 68 lanes decode a file)
    pillow_rows      Pillow with restart_marker_rows=1 (the same interval structure, optimised-off standard tables)
    pillow_plain     Pillow's default: no DRI -- the whole scan of a file is decoded by ONE lane

For batches of 1, 6 and 30 files, per image:

    decode           jpeg.decode: the plans on the host, one upload of files and plans, the kernels, one read of the status
    pil_upload       np.asarray(Image.open(...)) of every file, stacked, uploaded
    load_device      scene._load_images(..., device_jpeg=True) at resolution 2 from files on disk: decode + resize
    load_pil         the same call with device_jpeg=False: PIL, upload, resize

medians over the rounds with min and max, and ms per kernel from one profiled decode per kind and batch.  The comparison is
against PIL, never against the code under test.  Nothing rests on these numbers -- the feature is opt-in -- and where the
device route loses the table says so ("decode_below_pil": false).  The measurement runs in a child process under `timeout`;
if it fails nothing more is started on the device.

    python tools/jpeg_decode_timing.py [--out profiles/jpeg_decode_timing.json]
"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from collections import namedtuple

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
QUALITY = 90
W, H = 1920, 1080
BATCHES = (1, 6, 30)
Cam = namedtuple("Cam", "image_path")


def _span(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "rounds": values}


def pictures(n):
    """uint8 [n,H,W,3] on the device: low-frequency structure, edges and mild noise, different per image."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    x = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        p = torch.rand(3, 6, generator=g, device="cuda")
        for c in range(3):
            a, b, u, v, s, t = (float(k) for k in p[c])
            img = 127.5 + 70 * torch.sin((0.004 + 0.02 * a) * x + 6 * u) * torch.cos((0.004 + 0.02 * b) * y + 6 * v)
            img = img + 40 * ((x * (0.5 + s) + y * (0.5 + t)) % 97 < 40)
            img = img + 4 * torch.randn((H, W), generator=g, device="cuda")
            out[i, :, :, c] = img.clamp(0, 255).to(torch.uint8)
    return out


def measure(rounds):
    import numpy as np
    import torch
    from PIL import Image
    from deblurgs_amd import jpeg, scene
    n = max(BATCHES)
    images = pictures(n)
    host = images.cpu().numpy()

    def pillow(i, **kw):
        f = io.BytesIO()
        Image.fromarray(host[i]).save(f, "JPEG", quality=QUALITY, subsampling=2, **kw)
        return f.getvalue()

    kinds = {"device_encoder": [b for k in range(0, n, 6) for b in jpeg.to_bytes(images[k:k + 6], QUALITY, "4:2:0")],
             "pillow_rows": [pillow(i, restart_marker_rows=1) for i in range(n)],
             "pillow_plain": [pillow(i) for i in range(n)]}
    del images
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "width": W, "height": H, "quality": QUALITY,
           "subsampling": "4:2:0", "raw_bytes_per_image": W * H * 3, "kinds": {}}
    tmp = tempfile.mkdtemp(prefix="jpeg_decode_timing_")

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def pil_upload(files):
        return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])).cuda()

    for kind, files in kinds.items():
        probe = jpeg.probe(files[0])
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(tmp, f"{kind}_{i:02d}.jpg"))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        assert torch.equal(jpeg.decode(files[:2]), pil_upload(files[:2]))           # the same pixels, or no timing
        entry = {"intervals": probe["intervals"], "restart_interval": probe["restart_interval"],
                 "file_bytes_per_image": sum(map(len, files)) / n, "batches": {}}
        for b in BATCHES:
            cams = [Cam(p) for p in paths[:b]]
            arms = {"decode": lambda: jpeg.decode(files[:b]), "pil_upload": lambda: pil_upload(files[:b]),
                    "load_device": lambda: scene._load_images(cams, 2, scene.default_image_reader, "cuda", "timing", True),
                    "load_pil": lambda: scene._load_images(cams, 2, scene.default_image_reader, "cuda", "timing", False)}
            for fn in arms.values():
                fn()                                # warm-up of every shape
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():          # (alternating: the arms share whatever else the box is doing)
                    times[k].append(window(fn) / b)
            kernels = {}
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    jpeg.decode(files[:b])
                    torch.cuda.synchronize()
                kernels = {e.key: e.device_time_total / 1e3 / b for e in prof.key_averages()
                           if "jd_" in e.key or "Memset" in e.key or "fill" in e.key.lower() or "Memcpy" in e.key}
            except Exception as e:       # (the profiler is a convenience: the timings above do not depend on it)
                kernels = {"unavailable": repr(e)[:200]}
            entry["batches"][str(b)] = {"ms_per_image": {k: _span(v) for k, v in times.items()}, "kernel_ms_per_image": kernels,
                                        "decode_below_pil": max(times["decode"]) < min(times["pil_upload"]),
                                        "load_below_pil": max(times["load_device"]) < min(times["load_pil"])}
        res["kinds"][kind] = entry
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("JPEG_DECODE_TIMING_JSON " + json.dumps(measure(a.rounds)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("JPEG_DECODE_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("JPEG_DECODE_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

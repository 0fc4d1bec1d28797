"""Times the device JPEG encoder and the Motion-JPEG AVI writer (deblurgs_amd/jpeg.py, deblurgs_amd/video.py) on an MI355X
against the host route on the same box, Image.save(..., "JPEG").

Frames: four 1920 x 1080 RGB frames of the metric scene (render_path.frames_finish bytes of a spiral path).  At quality 90,
for 4:2:0 and 4:4:4, for one frame and for the batch of four, per frame:

    encode_1 / encode_4      jpeg.encode alone (device time between two synchronisations)
    append_1 / append_4      MjpegAviWriter.append: encode + the read of the sizes + the copy of sizes[i] bytes + the append
                             to the open file
    pil / pil_save_only      the host route: .cpu() of the raw frame + Image.save into memory at the same quality and
                             subsampling (save alone is reported too)

medians over the rounds with min and max; bytes per frame of both routes; ms per kernel from one profiled call per shape;
and frames/s of render_path.write_frames_video against render_path.render_frames alone on a spiral path of the scene.  The
comparison is against Image.save, never against the code under test.  The measurement runs in a child process under
`timeout`; if it fails nothing more is started on the device.

    python tools/video_timing.py [--out profiles/video_timing.json]
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
QUALITY = 90


def _span(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "rounds": values}


def measure(P, rounds, n, path_frames):
    import numpy as np
    import torch
    from PIL import Image
    from deblurgs_amd import jpeg, losses, render_path as rp, synthetic, video
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    sc = synthetic.make_config("metric", seed=0, P=P, K=1)
    W, H = sc["W"], sc["H"]
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    torch.manual_seed(0)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    motion = CameraMotionModule(ref, torch.zeros(4, 3, 8, 8, device="cuda"), curve_order=3, num_subframes=5,
                                init_se3=torch.randn(4, 6) * 0.01, device="cuda")
    cams = rp.spiral_path(motion, cloud, n_frames=path_frames, spin_for=1)
    with torch.no_grad():
        images = rp.frames_finish(rp.render_group(cams[:n], cloud, bg)["render"], tm).contiguous()
    one = images[:1]
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "batch": n, "P": P, "width": W, "height": H,
           "quality": QUALITY, "modes": {}}
    tmp = tempfile.mkdtemp(prefix="video_timing_")

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for mode in ("4:2:0", "4:4:4"):
        writer = video.MjpegAviWriter(os.path.join(tmp, "timing.avi"), 32, QUALITY, mode)
        arms = {"encode_1": (lambda: jpeg.encode(one, QUALITY, mode), 1), "encode_4": (lambda: jpeg.encode(images, QUALITY, mode), n),
                "append_1": (lambda: writer.append(one), 1), "append_4": (lambda: writer.append(images), n)}
        for fn, _ in arms.values():
            fn()                                    # warm-up of every shape
        times = {k: [] for k in list(arms) + ["pil", "pil_save_only"]}
        for _ in range(rounds):
            for k, (fn, per) in arms.items():
                times[k].append(window(fn) / per)
            total = save = 0.0
            for i in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = images[i].cpu().numpy()
                t1 = time.perf_counter()
                Image.fromarray(host).save(io.BytesIO(), "JPEG", quality=QUALITY, subsampling=mode)
                t2 = time.perf_counter()
                total += (t2 - t0) * 1e3 / 2
                save += (t2 - t1) * 1e3 / 2
            times["pil"].append(total)
            times["pil_save_only"].append(save)
        writer.close()
        blobs = jpeg.to_bytes(images, QUALITY, mode)
        host = images.cpu().numpy()
        pil_bytes, psnr = [], {"device": [], "pil": []}
        for i in range(n):
            f = io.BytesIO()
            Image.fromarray(host[i]).save(f, "JPEG", quality=QUALITY, subsampling=mode)
            pil_bytes.append(len(f.getvalue()))
            for key, data in (("device", blobs[i]), ("pil", f.getvalue())):
                err = np.asarray(Image.open(io.BytesIO(data)), np.float64) - host[i]
                psnr[key].append(10.0 * np.log10(255.0 ** 2 / max(np.mean(err ** 2), 1e-12)))
        kernels = {}
        try:
            from torch.profiler import ProfilerActivity, profile
            for key, batch in (("batch_of_1", one), (f"batch_of_{n}", images)):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    jpeg.encode(batch, QUALITY, mode)
                    torch.cuda.synchronize()
                kernels[key] = {e.key: e.device_time_total / 1e3 for e in prof.key_averages() if "jpeg_" in e.key}
        except Exception as e:       # (the profiler is a convenience: the timings above do not depend on it)
            kernels = {"unavailable": repr(e)[:200]}
        res["modes"][mode] = {"ms_per_frame": {k: _span(v) for k, v in times.items()},
                              "bytes_per_frame": {"device": sum(map(len, blobs)) / n, "pil": sum(pil_bytes) / n,
                                                  "raw": host[0].size, "bound": jpeg.bound(W, H, 3, mode)},
                              "psnr_db": {k: sum(v) / n for k, v in psnr.items()}, "kernel_ms": kernels,
                              "append_1_below_pil": max(times["append_1"]) < min(times["pil"]),
                              "append_4_below_pil": max(times["append_4"]) < min(times["pil"])}
    # the camera path: frames/s with and without the video
    path = os.path.join(tmp, "path.avi")
    arms = {"render_frames": lambda: rp.render_frames(cams, cloud, bg, tm),
            "write_frames_video": lambda: rp.write_frames_video(cams, cloud, bg, path, 32, tm, quality=QUALITY)}
    for fn in arms.values():
        fn()
    fps = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            fps[k].append(len(cams) / (window(fn) / 1e3))
    res["path"] = {"frames": len(cams), "frames_per_call": rp.FRAMES_PER_CALL, "frames_per_s": {k: _span(v) for k, v in fps.items()},
                   "avi_bytes": os.path.getsize(path)}
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--path-frames", type=int, default=24)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("VIDEO_TIMING_JSON " + json.dumps(measure(a.P, a.rounds, a.batch, a.path_frames)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--P", str(a.P),
           "--rounds", str(a.rounds), "--batch", str(a.batch), "--path-frames", str(a.path_frames)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("VIDEO_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("VIDEO_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

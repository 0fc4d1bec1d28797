"""Times the device PNG encoder (deblurgs_amd/png.py) on an MI355X against the route it replaces, Image.save on the host.

Images: six 1920 x 1080 RGB frames each of (a) the metric scene and (b) the `surfaces` scene, both render_path.frames_finish
bytes of a spiral path, and (c) report.view_report's colorize'd error maps of the metric frames against a noisy ground truth.
Per set, per image:

    encode_1 / encode_6      png.encode of one image / of the batch of six (device time between two synchronisations)
    file_1 / file_6          png.write_files: encode + the read of the sizes + the copy of sizes[i] bytes + the file write
    pil_default / pil_fast   the parent commit's route on the same bytes on the same host: the copy of the raw image to the
                             host + Image.fromarray(...).save(path) at PIL's default level and at compress_level=1
                             (save alone is reported too); two images a round

three rounds, min - max; file sizes beside PIL's; the IDAT length against zlib's Z_RLE over the file's own filtered stream in
one piece; and ms per kernel from one profiled batch call.  The comparison is against Image.save, never against the code
under test.  The measurement runs in a child process under `timeout`; if it fails nothing more is started on the device.

    python tools/png_timing.py [--out profiles/png_timing.json]
"""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def _frames(layout, P, n):
    import torch
    from deblurgs_amd import losses, render_path as rp, synthetic
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    over = {"layout": "surfaces"} if layout == "surfaces" else {}
    sc = synthetic.make_config("metric", seed=0, P=P, K=1, **over)
    W, H = sc["W"], sc["H"]
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    torch.manual_seed(0)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    motion = CameraMotionModule(ref, torch.zeros(4, 3, 8, 8, device="cuda"), curve_order=3, num_subframes=5,
                                init_se3=torch.randn(4, 6) * 0.01, device="cuda")
    cams = rp.spiral_path(motion, cloud, n_frames=n, spin_for=1)[:n]
    with torch.no_grad():
        render = rp.render_group(cams, cloud, bg)["render"]
        return rp.frames_finish(render, tm), tm(render).contiguous()


def _span(values):
    return {"min": min(values), "max": max(values), "rounds": values}


def measure(P, rounds, n):
    import numpy as np
    import torch
    from PIL import Image
    from deblurgs_amd import png, report
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "batch": n, "P": P, "segment": png._lib.PNG_SEGMENT,
           "sets": {}}
    metric_u8, metric_f = _frames("uniform", P, n)
    surfaces_u8, _ = _frames("surfaces", P, n)
    g = torch.Generator(device="cuda").manual_seed(7)
    gts = (metric_f + 0.03 * torch.randn(metric_f.shape, device="cuda", generator=g)).clamp_(0.0, 1.0)
    error_u8 = report.view_report(metric_f, gts, "identity")[2]
    del metric_f, gts
    sets = {"metric": metric_u8, "surfaces": surfaces_u8, "error_map": error_u8}
    tmp = tempfile.mkdtemp(prefix="png_timing_")
    paths = [os.path.join(tmp, f"{i}.png") for i in range(n)]

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, images in sets.items():
        images = images.contiguous()
        one = images[:1]
        arms = {"encode_1": (lambda: png.encode(one), 1), "encode_6": (lambda: png.encode(images), n),
                "file_1": (lambda: png.write_files(one, paths[:1]), 1), "file_6": (lambda: png.write_files(images, paths), n)}
        for fn, _ in arms.values():
            fn()                                    # warm-up of every shape
        times = {k: [] for k in list(arms) + ["pil_default", "pil_default_save_only", "pil_fast", "pil_fast_save_only"]}
        for _ in range(rounds):
            for k, (fn, per) in arms.items():
                times[k].append(window(fn) / per)
            for key, kw in (("pil_default", {}), ("pil_fast", {"compress_level": 1})):
                total = save = 0.0
                for i in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    host = images[i].cpu().numpy()
                    t1 = time.perf_counter()
                    Image.fromarray(host).save(paths[i], **kw)
                    t2 = time.perf_counter()
                    total += (t2 - t0) * 1e3 / 2
                    save += (t2 - t1) * 1e3 / 2
                times[key].append(total)
                times[key + "_save_only"].append(save)
        # sizes and correctness of image 0
        blob = png.to_bytes(one)[0]
        host = images[0].cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob))), host), name
        parsed = list(png.chunks(blob))
        assert all(ok for _, _, ok in parsed)
        idat = parsed[1][1]
        filtered = zlib.decompress(idat)
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
        rle = len(co.compress(filtered) + co.flush())
        sizes = {"device": len(blob)}
        for key, kw in (("pil_default", {}), ("pil_fast", {"compress_level": 1})):
            Image.fromarray(host).save(paths[0], **kw)
            sizes[key] = os.path.getsize(paths[0])
        raw = host.size
        res["sets"][name] = {"ms_per_image": {k: _span(v) for k, v in times.items()}, "file_bytes": sizes,
                             "of_raw": {k: v / raw for k, v in sizes.items()}, "idat_bytes": len(idat),
                             "z_rle_one_piece_bytes": rle, "idat_over_z_rle": len(idat) / rle,
                             "file_1_below_pil_fast": max(times["file_1"]) < min(times["pil_fast"])}
    # ms per kernel: one profiled batch call on the metric frames
    try:
        from torch.profiler import ProfilerActivity, profile
        images = sets["metric"].contiguous()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            png.encode(images)
            torch.cuda.synchronize()
        res["kernel_ms_batch_of_6"] = {e.key: e.device_time_total / 1e3 for e in prof.key_averages() if "png_" in e.key}
    except Exception as e:       # (the profiler is a convenience: the timings above do not depend on it)
        res["kernel_ms_batch_of_6"] = {"unavailable": repr(e)[:200]}
    for p in paths:
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(tmp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("PNG_TIMING_JSON " + json.dumps(measure(a.P, a.rounds, a.batch)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--P", str(a.P),
           "--rounds", str(a.rounds), "--batch", str(a.batch)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PNG_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("PNG_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

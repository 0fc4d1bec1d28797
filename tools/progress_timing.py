"""Times one shot of the training-progress visualiser (deblurgs_amd/progress.py) on an MI355X at 1920 x 1080 for 30 and 100
training views, the device route against a host route on the same box.

Both routes start from the same finished 8-bit render of the overview camera (its cost is reported apart: it is the same in
both) and draw the same cones, 5 subframe cameras per view:

    device_cones     progress.overlay_prims (the trajectory kernels of every view, ONE dgs_cone_segments) + progress.draw
    host_cones       the reference's route as far as this box has its parts: .cpu() of the frame, per view the sampled
                     subframe cameras brought to the host one by one, the five cone vertices projected in numpy, and
                     PIL.ImageDraw.line per segment where PIL is importable (cv2 is not required by this project; without
                     PIL the arm stops after the projections and says so)
    device_shot      everything run(iteration) does at a shot: camera_overlay, alignment_plot, two jpeg.encode calls and
                     the download of the two files
    render           gaussian_renderer.render + frames_finish alone

medians over the rounds with min and max, and the share of device time per kernel of one profiled device_shot.  The
comparison is against the host route, never against the code under test.  The measurement runs in a child process under
`timeout`; if it fails nothing more is started on the device.

    python tools/progress_timing.py [--out profiles/progress_timing.json]
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
CONNECTIVITY = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1)]


def _span(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "rounds": values}


def host_cones(frame, motion, cam, scale, colours, draw_lines):
    """The reference's loop (utils/visualization.py:156-185, 204-206) on the host.  Returns the segments drawn."""
    import numpy as np
    import torch
    img = frame.cpu().numpy()
    H, W, _ = img.shape
    canvas = pen = None
    if draw_lines:
        from PIL import Image, ImageDraw
        canvas = Image.fromarray(img)
        pen = ImageDraw.Draw(canvas)
    render_view = cam.world_view_transform.cpu().numpy()
    render_proj = cam.full_proj_transform.cpu().numpy()
    cone_x, cone_y = math.tan(motion.ref_cam.FoVx / 2), math.tan(motion.ref_cam.FoVy / 2)
    drawn = 0
    for i in range(len(motion)):
        nu = motion._sample_nu_from_alignment(i)
        pick = torch.linspace(0, nu.shape[0] - 1, 5, device=nu.device).long()
        for c in motion.get_trajectory(i, nu[pick]):
            c2w = np.eye(4)
            c2w[:3, :3] = c.world_view_transform[:3, :3].cpu().numpy()
            c2w[:3, 3] = c.camera_center.cpu().numpy()
            cone = np.pad(np.array([[0.0, 0.0, 0.0], [cone_x, cone_y, 1.0], [cone_x, -cone_y, 1.0], [-cone_x, -cone_y, 1.0],
                                    [-cone_x, cone_y, 1.0]]) * scale, ((0, 0), (0, 1)), "constant", constant_values=1.0)
            world = cone @ c2w.T
            cam_hom = cone @ render_view
            if (cam_hom[:, 2] / cam_hom[:, 3] < 0.1).any():
                continue
            ndc_hom = world @ render_proj
            ndc = ndc_hom[:, :3] / ndc_hom[:, 3:]
            pix = ((ndc[:, :2] + 1.0) * np.array([W, H]).astype(float) - 1.0) * 0.5
            for a, b in CONNECTIVITY:
                drawn += 1
                if pen is not None:
                    pen.line([tuple(pix[a].astype(int).tolist()), tuple(pix[b].astype(int).tolist())],
                             fill=tuple(int(v) for v in colours[i]), width=1)
    return drawn


def measure(P, rounds, view_counts):
    import numpy as np
    import torch
    from deblurgs_amd import device_files, gaussian_renderer, jpeg, losses, progress, render_path as rp, synthetic, video
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    torch.set_grad_enabled(False)       # (the reference's visualiser runs under no_grad; nothing here differentiates)
    sc = synthetic.make_config("metric", seed=0, P=P, K=1)
    W, H = sc["W"], sc["H"]
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "P": P, "width": W, "height": H,
           "host_route_draws_lines": have_pil, "views": {}}

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for n in view_counts:
        torch.manual_seed(n)
        motion = CameraMotionModule(ref, torch.zeros(n, 3, 8, 8, device="cuda"), curve_order=9, num_subframes=21,
                                    init_se3=torch.randn(n, 6) * torch.tensor([0.3] * 3 + [0.05] * 3), device="cuda")
        cam = progress.overview_camera(motion, cloud)
        colours = progress.view_colours(n)
        indices = np.arange(min(9, n))
        slots = [device_files.Download(video.HOST_BYTES) for _ in range(2)]
        with torch.no_grad():
            frame = rp.frames_finish(gaussian_renderer.render(cam, cloud, bg)["render"][None], tm)[0]
        segments = int((progress.overlay_prims(motion, cam)[:, 4] == 0).sum())

        def render():
            with torch.no_grad():
                rp.frames_finish(gaussian_renderer.render(cam, cloud, bg)["render"][None], tm)

        def device_cones():
            progress.draw(frame.clone(), progress.overlay_prims(motion, cam))

        def device_shot():
            images = [progress.camera_overlay(motion, cloud, cam, bg, tm), progress.alignment_plot(motion, indices)]
            for image, slot in zip(images, slots):
                slot.read_sizes(*jpeg.encode(image[None], 90))
            for slot in slots:
                slot.copy_bytes()
            return [slot.blobs() for slot in slots]

        arms = {"render": render, "device_cones": device_cones, "device_shot": device_shot,
                "host_cones": lambda: host_cones(frame, motion, cam, 0.5, colours, have_pil)}
        for fn in arms.values():
            fn()                                        # warm-up of every shape
        times = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                times[k].append(window(fn))
        kernels = {}
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                device_shot()
                torch.cuda.synchronize()
            per = {e.key: e.device_time_total / 1e3 for e in prof.key_averages() if e.device_time_total > 0}
            total = sum(per.values())
            top = sorted(per.items(), key=lambda kv: -kv[1])[:12]
            kernels = {"device_ms_total": total, "share": {k[:80]: v / total for k, v in top},
                       "draw_and_cone_ms": {k[:80]: v for k, v in per.items() if "draw_" in k or "cone_" in k}}
        except Exception as e:       # (the profiler is a convenience: the timings above do not depend on it)
            kernels = {"unavailable": repr(e)[:200]}
        res["views"][str(n)] = {"ms_per_shot": {k: _span(v) for k, v in times.items()}, "segments_drawn": segments,
                                "host_segments": host_cones(frame, motion, cam, 0.5, colours, False), "kernels": kernels,
                                "device_cones_below_host_cones": max(times["device_cones"]) < min(times["host_cones"])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--views", type=int, nargs="+", default=[30, 100])
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progress_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("PROGRESS_TIMING_JSON " + json.dumps(measure(a.P, a.rounds, a.views)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--P", str(a.P),
           "--rounds", str(a.rounds), "--views"] + [str(v) for v in a.views]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PROGRESS_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("PROGRESS_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

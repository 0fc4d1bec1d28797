"""Times camera-path rendering at the metric scene (1 M Gaussians, 1920 x 1080) over a 60-frame spiral:

  arm A    the reference's shape (render_spiral.py:27-33) built from what the package offered before render_path: per
           camera one render() and the tone mapping; then stack, permute, .cpu() of the float frames, and numpy's
           clip * 255 -> astype(uint8) on the host
  arm B    render_path.render_frames at frames_per_call 1, 4, 8 and 16: K cameras per rasteriser call, 8-bit frames made
           on the device, packed frames copied through two pinned buffers

Both arms run in ONE process on one device, interleaved over `--rounds` rounds after a warm-up of every shape; a window
is `--reps` passes over the path between two host timestamps, the second after a device synchronise -- the copy to the
host and the host-side work are part of what is measured.  Per arm: frames/s of every round, bytes moved to the host per
pass, and the peak of device memory above what was allocated before the pass.

    python tools/path_timing.py [--P 1000000] [--out profiles/path_timing.json]

The measurement runs in a child process under `timeout`; if it fails, faults or runs out of time nothing more is started
on the device and the JSON says so.  The default frames_per_call follows variants/NOTES.md's kill rule: the smallest value
whose median is within 1.5 % of the best; and 1 unless some K > 1 beats K = 1 by more than 1.5 % in every round.
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

PER_CALL = (1, 4, 8, 16)
KILL = 0.015


def choose_default(rounds_by_k):
    """rounds_by_k: {frames_per_call: [frames/s per round]} -> (default, why)."""
    med = {k: statistics.median(v) for k, v in rounds_by_k.items()}
    best = max(med.values())
    beats_one = [k for k in sorted(rounds_by_k) if k > 1 and
                 all(a > b * (1.0 + KILL) for a, b in zip(rounds_by_k[k], rounds_by_k[1]))]
    if not beats_one:
        return 1, "no frames_per_call > 1 beat 1 by more than 1.5 % in every round"
    k = min(k for k in sorted(med) if med[k] >= best * (1.0 - KILL))
    return k, f"the smallest value whose median is within 1.5 % of the best ({best:.1f} frames/s)"


def measure(P, rounds, reps, n_frames):
    import numpy as np
    import torch
    from deblurgs_amd import gaussian_renderer, losses, render_path as rp, synthetic
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
    cams = rp.spiral_path(motion, cloud, n_frames=n_frames // 2, spin_for=2)
    n = len(cams)

    def arm_a():
        with torch.no_grad():
            imgs = torch.stack([tm(gaussian_renderer.render(c, cloud, bg)["render"]) for c in cams])
            return (imgs.permute(0, 2, 3, 1).cpu().numpy().clip(0.0, 1.0) * 255.0).astype(np.uint8)

    arms = {"A": arm_a}
    for k in PER_CALL:
        arms[f"B{k}"] = (lambda k=k: rp.render_frames(cams, cloud, bg, tm, frames_per_call=k))
    out = {}
    first = {}
    for name, fn in arms.items():           # warm-up: every shape once, and what each arm returns
        first[name] = fn()
    torch.cuda.synchronize()
    base = first["B1"]
    res = {"P": P, "W": W, "H": H, "frames": n, "rounds": rounds, "passes_per_window": reps, "tone_mapping": "gamma",
           "device": torch.cuda.get_device_name(0), "arms": {}}
    for name in arms:
        differ = int((first[name] != base).sum())
        res["arms"][name] = {"frames_per_s": [], "bytes_differing_from_B1": differ,
                             "bytes_to_host_per_pass": n * H * W * 3 * (4 if name == "A" else 1)}
    del first
    for _ in range(rounds):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            a = res["arms"][name]
            a["frames_per_s"].append(n * reps / dt)
            a["peak_device_bytes_above_start"] = max(a.get("peak_device_bytes_above_start", 0),
                                                     int(torch.cuda.max_memory_allocated() - before))
    for a in res["arms"].values():
        a["median_frames_per_s"] = statistics.median(a["frames_per_s"])
    k, why = choose_default({k: res["arms"][f"B{k}"]["frames_per_s"] for k in PER_CALL})
    res["default_frames_per_call"], res["default_reason"] = k, why
    res["speedup_default_over_A"] = res["arms"][f"B{k}"]["median_frames_per_s"] / res["arms"]["A"]["median_frames_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("PATH_TIMING_JSON " + json.dumps(measure(a.P, a.rounds, a.reps, a.frames)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--P", str(a.P),
           "--rounds", str(a.rounds), "--reps", str(a.reps), "--frames", str(a.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PATH_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("PATH_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Times the test-pose seeding (deblurgs_amd/registration.py) at the metric scene (1 M Gaussians, 1920 x 1080) for the box
factors 1, 4 and 8: milliseconds per stage of registration.seed_test_poses --

    render     the candidate bank through the K-fused forward-only rasteriser (render_path.render_group)
    finish     dgs_frames_finish of those renders (gamma tone map)
    box        dgs_box_reduce_u8 of the 8-bit frames
    sad        dgs_sad_matrix of the test images against the bank
    round      one whole refinement round: n * 12 lattice renders, finish, box, grouped SAD, the host's decision

-- and dgs_sad_matrix beside the torch expression (a[:, None].int() - b[None].int()).abs().sum(-1) on the same device
tensors (bytes), whose result must be equal.  Device stages are timed with events on the rendering stream, the median of
`--reps` after one warm-up; `round` is host time between two synchronisations.

    python tools/registration_timing.py [--P 1000000] [--out profiles/registration_timing.json]

Every factor is measured by a child process of its own under `timeout`; if one fails, faults or runs out of time nothing
more is started on the device and the JSON says so.
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

FACTORS = (1, 4, 8)


def measure(P, factor, reps, n_tests, views):
    import numpy as np
    import torch
    from deblurgs_amd import losses, registration as reg, render_path as rp, synthetic
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    sc = synthetic.make_config("metric", seed=0, P=P, K=1)
    W, H = sc["W"], sc["H"]
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    torch.manual_seed(0)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    motion = CameraMotionModule(ref, torch.zeros(views, 3, 8, 8, device="cuda"), curve_order=3, num_subframes=5,
                                init_se3=torch.randn(views, 6) * 0.01, device="cuda")
    cams, table = reg.candidate_cameras(motion, subframes=3, between=1)
    C = len(cams)
    groups = rp.frame_groups(cams, rp.FRAMES_PER_CALL)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), out

    res = {"P": P, "W": W, "H": H, "factor": factor, "candidates": C, "tests": n_tests, "reps": reps,
           "frames_per_call": rp.FRAMES_PER_CALL, "device": torch.cuda.get_device_name(0), "ms": {}}
    with torch.no_grad():
        res["ms"]["render"], colors = timed(lambda: [rp.render_group(cams[b:e], cloud, bg)["render"] for b, e in groups])
        res["ms"]["finish"], frames = timed(lambda: [rp.frames_finish(c, tm) for c in colors])
        res["ms"]["box"], rows = timed(lambda: [reg.box_reduce_u8(f, factor) for f in frames])
        bank = torch.cat(rows, dim=0)
        picks = [(3 * i + 1) % C for i in range(n_tests)]
        tests = bank[picks].contiguous()
        res["ms"]["sad"], scores = timed(lambda: reg.sad_matrix(tests, bank))
        res["L_dwords"] = int(bank.shape[1])
        assert scores[torch.arange(n_tests), torch.tensor(picks)].abs().max().item() == 0
        a8, b8 = tests.view(torch.uint8), bank.view(torch.uint8)
        res["ms"]["sad_torch"], ref_scores = timed(lambda: (a8[:, None].int() - b8[None].int()).abs().sum(-1))
        res["sad_equals_torch"] = bool(torch.equal(ref_scores.to(torch.int64), scores))
        images = torch.stack([tm(colors[p // rp.FRAMES_PER_CALL][p % rp.FRAMES_PER_CALL]).clamp(0.0, 1.0) for p in picks])
        del colors, frames, rows, ref_scores
        kw = dict(factor=factor, subframes=3, between=1, trans_step=0.01, rot_step_deg=0.2)
        wall = {}
        for rounds in (0, 1):
            reg.seed_test_poses(motion, cloud, images, bg, tm, refine_rounds=rounds, **kw)
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                reg.seed_test_poses(motion, cloud, images, bg, tm, refine_rounds=rounds, **kw)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            wall[rounds] = statistics.median(ts)
        res["ms"]["seed_wall"] = wall[0]
        res["ms"]["round"] = wall[1] - wall[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tests", type=int, default=4)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds one factor's measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_timing.json"))
    ap.add_argument("--leg", type=int, default=0, help="internal: measure this factor in this process and print the JSON")
    a = ap.parse_args()
    if a.leg:
        print("REGISTRATION_TIMING_JSON " + json.dumps(measure(a.P, a.leg, a.reps, a.tests, a.views)), flush=True)
        return 0
    result = {"note": "one box, one run", "factors": {}}
    ok = True
    for factor in FACTORS:           # (this process never opens the device)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", str(factor), "--P",
               str(a.P), "--reps", str(a.reps), "--tests", str(a.tests), "--views", str(a.views)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("REGISTRATION_TIMING_JSON ")]
        ok = r.returncode == 0 and bool(lines)
        if not ok:           # nothing more is started on the device
            result["factors"][str(factor)] = {"failed": r.returncode, "stderr": r.stderr[-2000:]}
            break
        result["factors"][str(factor)] = json.loads(lines[-1][len("REGISTRATION_TIMING_JSON "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

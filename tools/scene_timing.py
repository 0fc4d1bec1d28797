"""Times the K = 15 training step at the metric size (1 M Gaussians, 1920 x 1080, SH degree 2) on TWO workloads, the
uniform scene every other figure of the project is quoted on and the scene-shaped `surfaces` layout
(synthetic.make_scene(layout="surfaces")), and records what their tile lists look like (deblurgs_amd/workload.py).

The step is built the way bench.py builds its headline step: TrainingLoop.step over a GaussianCloud and one
CameraMotionModule view whose ground truth is torch.rand noise (generator seed 1234), the same optimisation parameters,
learning rates scaled by 1e-6 so that the workload does not drift.  Protocol: ONE process; every shape warmed up; the two
scenes alternate for `--rounds` rounds; a window is at least `--window` seconds of steps between two host timestamps, the
second after a device synchronise; the median window per scene.  Then, outside the timed windows: the per-stage times of
dgs_profile_read over an eager region, R, the visible pairs, and the list profile of subframe 0 with tile culling and on
the reference's rectangle lists.

    python tools/scene_timing.py [--out profiles/scene_workload.json]

The ratio surfaces / uniform of subframe-renders per second is the number the decision rule of DESIGN.md section 9 reads.
The measurement runs in a child process under `timeout`; if it fails, faults or runs out of time nothing more is started
on the device and the JSON says so.
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

LAYOUTS = ("uniform", "surfaces")


def measure(config, rounds, window, seed, overrides):
    import torch
    from deblurgs_amd import _lib, synthetic, workload
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    from deblurgs_amd.training import TrainingLoop, default_optimization_params
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    C = synthetic.CONFIGS[config]["C"]
    far = 10 ** 9
    LR_SCALE = 1e-6

    def build(layout):
        scene = synthetic.make_config(config, seed=seed, sh_degree=2, layout=layout, **overrides)
        W, H, K = scene["W"], scene["H"], scene["K"]
        cloud = GaussianCloud.from_scene(scene, dev)
        ref_cam = RefCamera(W, H, scene["FoVx"], scene["FoVy"], device=dev)
        gen = torch.Generator(device="cpu").manual_seed(1234)
        gt = torch.rand((1, 3, H, W), generator=gen).to(dev)
        motion = CameraMotionModule(ref_cam, gt, curve_order=C, num_subframes=K, device=dev)
        traj = synthetic.make_trajectory(K, C, scene["projection_matrix"], seed=0)
        with torch.no_grad():
            motion._trans._control_points.copy_(torch.from_numpy(traj["ctrl_trans"])[None].to(dev))
            motion._rot._control_points.copy_(torch.from_numpy(traj["ctrl_rot"])[None].to(dev))
        motion.link_gaussian(cloud)
        opt = default_optimization_params(iterations=far, lambda_t_smooth_init=1e-3, lambda_t_smooth_final=1e-3,
                                          lambda_hinge=0.1, curve_start_iter=1, curve_end_iter=far, densify_from_iter=far,
                                          densify_until_iter=far, opacity_reset_interval=far, curve_rotation_lr=1e-3,
                                          curve_controlpoints_lr=1e-2, curve_alignment_lr=0.0)
        loop = TrainingLoop(cloud, motion, opt, cameras_extent=1.0, spatial_lr_scale=1.0, distributed=False,
                            fused_step="auto", log_losses=False, graph="auto")
        for group in cloud.optimizer.param_groups:
            group["lr"] *= LR_SCALE
        cloud.xyz_scheduler_args = lambda it: 0.00016 * LR_SCALE
        return dict(scene=scene, cloud=cloud, motion=motion, loop=loop, it=0, K=K)

    def step(a):
        a["it"] += 1
        a["last"] = a["loop"].step(a["it"], 0)

    def run_window(a):
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(4):
                step(a)
            n += 4
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= window:
                return dt, n

    arms = {name: build(name) for name in LAYOUTS}
    for a in arms.values():            # warm-up of every shape (the fused step learns its duplicate capacity here)
        for _ in range(6):
            step(a)
    torch.cuda.synchronize()
    res = {"config": config, "overrides": overrides, "seed": seed, "rounds": rounds, "window_s": window,
           "device": torch.cuda.get_device_name(0), "scenes": {}}
    for name in LAYOUTS:
        res["scenes"][name] = {"ms_per_step": [], "steps_per_window": []}
    for _ in range(rounds):
        for name in LAYOUTS:
            dt, n = run_window(arms[name])
            res["scenes"][name]["ms_per_step"].append(dt / n * 1e3)
            res["scenes"][name]["steps_per_window"].append(n)
    for name, a in arms.items():
        s = res["scenes"][name]
        s["median_ms_per_step"] = statistics.median(s["ms_per_step"])
        s["subframe_renders_per_s"] = a["K"] / s["median_ms_per_step"] * 1e3
        fused = a["loop"]._fused
        s["fused_step"] = fused is not None
        if fused is not None:
            s["replayed_steps"], s["dropped"], s["retried"] = int(fused.replayed), int(fused.dropped), int(a["loop"].retried)
    # ---- outside the timed windows: stage times (an eager region: events cannot be recorded inside a replayed graph)
    for name, a in arms.items():
        s = res["scenes"][name]
        keep = a["loop"].graph
        a["loop"].graph = False
        for _ in range(2):
            step(a)
        torch.cuda.synchronize()
        _lib.profile_reset()
        _lib.profile_enable(True)
        n_prof = 10
        t0 = time.perf_counter()
        for _ in range(n_prof):
            step(a)
        torch.cuda.synchronize()
        s["profiled_ms_per_step"] = (time.perf_counter() - t0) / n_prof * 1e3
        _lib.profile_enable(False)
        s["stage_ms_per_step"] = {k: v[0] / n_prof for k, v in _lib.profile_read().items()}
        a["loop"].graph = keep
    # ---- the workload itself: visible pairs, R, list profiles
    for name, a in arms.items():
        s, scene, K = res["scenes"][name], a["scene"], a["K"]
        with torch.no_grad():
            probe = a["motion"].query(0, "all", compute_blurred=False)
            s["visible_pairs"] = int((probe["radii_all"] > 0).sum().item())
            del probe
        a["loop"] = a["motion"] = a["cloud"] = None
        torch.cuda.empty_cache()
        full = workload.profile_scene(scene, K, tile_cull=True, per_tile=True)
        s["R"] = full.total
        d = full.as_dict()
        d.pop("subframes")
        d["skew"] = full.skew()
        s["all_subframes_tile_cull"] = d
        # what a 64-entry batch some pixel still needed cost: were the time set by the work alone and not by how it is
        # spread over the tiles, the two scenes would pay the same
        s["ns_per_walked_batch"] = {k: s["stage_ms_per_step"][k] * 1e6 / max(full.walked_batches, 1)
                                    for k in ("composite_fwd", "composite_bwd")}
        del full
        for key, cull in (("subframe0_tile_cull", True), ("subframe0_reference_lists", False)):
            p = workload.profile_scene(scene, 1, tile_cull=cull, per_tile=True)
            d = p.as_dict()
            d.pop("subframes")
            d["skew"] = p.skew()
            d["length_p50_p90_p99"] = p.percentiles((50.0, 90.0, 99.0))
            s[key] = d
            del p
        s["R_subframe0_reference_lists"] = s["subframe0_reference_lists"]["total"]
    u, v = res["scenes"]["uniform"], res["scenes"]["surfaces"]
    res["ratio_surfaces_over_uniform_renders_per_s"] = v["subframe_renders_per_s"] / u["subframe_renders_per_s"]
    res["ratio_R_surfaces_over_uniform"] = v["R"] / u["R"]
    res["ratio_at_equal_R"] = res["ratio_surfaces_over_uniform_renders_per_s"] * res["ratio_R_surfaces_over_uniform"]
    res["ratio_at_equal_R_note"] = ("renders/s ratio x R ratio: the ratio of duplicates composited per second; the whole step "
                                    "is in it, also the parts whose cost does not scale with R")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="metric")
    ap.add_argument("--P", type=int, default=None)
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window")
    ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_workload.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.window < 1.0 and a.config == "metric" and a.P is None:
        ap.error("windows of at least one second")
    over = {k: v for k, v in (("P", a.P), ("K", a.K)) if v is not None}
    if a.leg:
        print("SCENE_TIMING_JSON " + json.dumps(measure(a.config, a.rounds, a.window, a.seed, over)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--config", a.config,
           "--seed", str(a.seed), "--rounds", str(a.rounds), "--window", str(a.window)]
    for k, v in over.items():
        cmd += [f"--{k}", str(v)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SCENE_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("SCENE_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-3000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Times the evaluation protocol at the metric scene (1 M Gaussians, 1920 x 1080):

  fit      ms per step of the fused test-view pose fit (evaluation.FusedPoseFit: one hipGraph replay per step) against
           ms per step of the same fit driven through render(), autograd and torch.optim.Adam
           (tests/autograd_pose_fit.py: the only way to run it before ABI 15)
  epoch_fit  ms per EPOCH of that fit at n = 3, 8 and 16 test views: the sequential FusedPoseFit (n graph replays per
           epoch) against the epoch-fused EpochPoseFit (one K = n launch chain per epoch), same scene, same schedule,
           same repetition scheme (20 epochs of warm-up, 50 epochs between two device events)
  stages   the context's stage timers of dgs_backward_pose_only against dgs_backward on the same forward state, at
           K = 1 and at K = 15
  metrics  ms per dgs_image_metrics call (PSNR + SSIM of two 1080p images)

    python tools/eval_timing.py [--P 1000000] [--out profiles/eval_fit.json]

Every leg runs in a child process of its own under `timeout`, one after the other; the first leg that fails, faults or
times out ends the run (nothing more is started on the device) and the JSON holds what was measured until then.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = [("fit", 420), ("epoch_fit", 600), ("stages_k1", 240), ("stages_k15", 300), ("metrics", 120)]


def _scene(P, K):
    from deblurgs_amd import synthetic
    return synthetic.make_config("metric", seed=0, P=P, K=K)


def _fit_setup(P, n=3):
    import numpy as np
    import torch
    from scipy.spatial.transform import Rotation
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses
    from deblurgs_amd.cloud import GaussianCloud
    sc = _scene(P, n)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    W, H = sc["W"], sc["H"]
    cam = lambda R, T: ev.TestCamera(R, T, sc["FoVx"], sc["FoVy"], W, H)
    truth = ev.TestPoseModel([cam(V[i][:3, :3], V[i][3, :3]) for i in range(n)], device="cuda")
    with torch.no_grad():
        gts = torch.stack([tm(gaussian_renderer.render(truth(i), cloud, bg)["render"]).clamp(0.0, 1.0) for i in range(n)])
    dR = Rotation.from_rotvec(np.deg2rad(0.3) * np.array([0.6, -0.64, 0.48])).as_matrix()
    start = [cam(V[i][:3, :3] @ dR, V[i][3, :3] + np.array([0.02, -0.01, 0.02])) for i in range(n)]
    return cloud, start, gts, bg, tm


def leg_fit(P):
    import torch
    from deblurgs_amd import evaluation as ev
    cloud, start, gts, bg, tm = _fit_setup(P)
    n_fused, n_auto = 150, 30
    fit = ev.FusedPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=2000)
    fit.schedule(ev.epoch_orders(3, 20 + n_fused // 3, order=[0, 1, 2]))
    fit.run(60)                                   # warm-up: code objects, the graph's first replays
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fit.run(n_fused)
    e1.record()
    t_enqueue = time.perf_counter() - t0
    torch.cuda.synchronize()
    fused_ms = e0.elapsed_time(e1) / n_fused
    l1_fused = float(fit.work[0])
    from autograd_pose_fit import AutogradPoseFit      # tests/: the yardstick, not part of the package
    auto = AutogradPoseFit(cloud, start, list(gts), bg, tm, num_iter_per_view=2000)
    for i in range(6):
        auto.step(i % 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_auto):
        auto.step(i % 3)
    torch.cuda.synchronize()
    auto_ms = (time.perf_counter() - t0) * 1e3 / n_auto
    return {"P": P, "W": int(gts.shape[3]), "H": int(gts.shape[2]), "fused_ms_per_step": fused_ms,
            "fused_host_enqueue_ms_per_step": t_enqueue * 1e3 / n_fused, "autograd_ms_per_step": auto_ms,
            "speedup": auto_ms / fused_ms, "fused_steps_timed": n_fused, "autograd_steps_timed": n_auto,
            "capacity": fit.capacity, "dropped": fit.dropped(), "l1_after_fused_steps": l1_fused}


def leg_epoch_fit(P, views=(3, 8, 16), warm=20, reps=50):
    """ms per epoch, sequential against epoch-fused, at each number of views; both fits run the same schedule from the same
    start, so their parameters after the timed epochs are compared as well."""
    import torch
    from deblurgs_amd import evaluation as ev
    out = {"P": P, "warmup_epochs": warm, "timed_epochs": reps, "by_views": {}}
    for n in views:
        cloud, start, gts, bg, tm = _fit_setup(P, n)
        orders = ev.epoch_orders(n, warm + reps, order=list(range(n)))
        res = {}
        fits = {}
        for name, cls, unit in (("sequential", ev.FusedPoseFit, n), ("epoch", ev.EpochPoseFit, 1)):
            fit = cls(cloud, start, gts, bg, tm, num_iter_per_view=2000)
            fit.schedule(orders)
            fit.run(warm * unit)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fit.run(reps * unit)
            e1.record()
            t_enqueue = time.perf_counter() - t0
            torch.cuda.synchronize()
            res[name + "_ms_per_epoch"] = e0.elapsed_time(e1) / reps
            res[name + "_host_enqueue_ms_per_epoch"] = t_enqueue * 1e3 / reps
            res[name + "_dropped"] = fit.dropped()
            res[name + "_capacity"] = fit.capacity
            fits[name] = fit
        a, b = fits["sequential"], fits["epoch"]
        res["speedup"] = res["sequential_ms_per_epoch"] / res["epoch_ms_per_epoch"]
        res["parameters_bit_identical"] = bool(torch.equal(a.model._rot, b.model._rot) and torch.equal(a.model._trans, b.model._trans))
        res["max_abs_diff_rot"] = float((a.model._rot.detach() - b.model._rot.detach()).abs().max())
        res["max_abs_diff_trans"] = float((a.model._trans.detach() - b.model._trans.detach()).abs().max())
        out["by_views"][str(n)] = res
        print("epoch_fit", n, json.dumps(res), file=sys.stderr, flush=True)
        del fits, a, b, fit, cloud, gts
        torch.cuda.empty_cache()
    return out


def leg_stages(P, K):
    """dgs_backward and dgs_backward_pose_only on one forward state of the cloud's raw parameters (tile culling on), each
    timed with the context's stage timers over `reps` calls."""
    import numpy as np
    import torch
    from helpers import _t, hip_settings
    from deblurgs_amd import _lib, raster_call
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    from deblurgs_amd.cloud import GaussianCloud
    L = _lib.lib()
    sc = _scene(P, K)
    dev = torch.device("cuda")
    c = GaussianCloud.from_scene(sc, "cuda")
    rs = hip_settings(sc, K)._replace(campos=_t(sc["campos"][:K]))
    cams = [_t(sc["viewmatrix"][:K]), _t(sc["projmatrix"][:K]), _t(sc["campos"][:K])]
    rest = c._features_rest if c._features_rest.shape[1] > 0 else None
    raw = {"scale_lb": 0.0, "sh_rest": rest}
    args = [c._xyz.detach(), c._features_dc.detach(), None, c._opacity.detach().reshape(-1), c._scaling.detach(),
            c._rotation.detach(), None]
    with torch.no_grad():
        R, color, depth, radii, geom, binning, image = dgr._forward_impl(K, *args, *cams, rs, raw=raw)
        prob = raster_call.problem(K, *args, *cams, rs, dgr._bg(rs, dev), dgr.TILE_CULL, dgr.WIDE_RECORDS, raw=raw,
                                   geom=geom, image=image, binning=binning)
    R = int(R)
    g = torch.Generator(device="cuda").manual_seed(1)
    gC = torch.randn((K, 3, sc["H"], sc["W"]), device="cuda", generator=g)
    f = dict(dtype=torch.float32, device=dev)
    Pn = sc["P"]
    io, own = raster_call.backward_io(R, radii, gC, None, torch.empty((Pn, 3), **f), torch.empty((K, Pn, 3), **f),
                                      torch.empty((Pn, 1, 3), **f), torch.empty(Pn, **f), torch.empty((Pn, 3), **f),
                                      torch.empty((Pn, 4), **f), sh_rest=None if rest is None else torch.empty_like(rest))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, reps = {"P": Pn, "K": K, "num_rendered": R}, 10
    for name, fn in (("dgs_backward", L.dgs_backward), ("dgs_backward_pose_only", L.dgs_backward_pose_only)):
        for _ in range(3):
            _lib.check(fn(ctypes.byref(prob), ctypes.byref(io), st), name)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_reset()
        for _ in range(reps):
            _lib.check(fn(ctypes.byref(prob), ctypes.byref(io), st), name)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        stages = {k: v[0] / reps for k, v in prof.items() if v[1] > 0}
        stages["total"] = sum(stages.values())
        out[name] = stages
        out[name + "_pose_grads"] = [own["viewmatrix"].cpu().numpy().tolist(), own["projmatrix"].cpu().numpy().tolist()]
    a, b = out.pop("dgs_backward_pose_grads"), out.pop("dgs_backward_pose_only_pose_grads")
    out["pose_grads_bit_identical"] = bool(np.array_equal(np.array(a, np.float32), np.array(b, np.float32)))
    return out


def leg_metrics(P):
    import torch
    from deblurgs_amd import metrics
    g = torch.Generator(device="cuda").manual_seed(2)
    a = torch.rand((3, 1080, 1920), device="cuda", generator=g)
    b = (a + 0.05 * torch.randn((3, 1080, 1920), device="cuda", generator=g)).clamp(0, 1)
    for _ in range(5):
        metrics.psnr_ssim(a, b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        o = metrics.psnr_ssim(a, b)
    e1.record()
    torch.cuda.synchronize()
    return {"W": 1920, "H": 1080, "ms_per_call": e0.elapsed_time(e1) / 50, "psnr": float(o[0]), "ssim": float(o[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_fit.json"))
    ap.add_argument("--leg", default=None, help="internal: run one leg in this process and print its JSON")
    a = ap.parse_args()
    if a.leg is not None:
        res = {"fit": lambda: leg_fit(a.P), "epoch_fit": lambda: leg_epoch_fit(a.P), "stages_k1": lambda: leg_stages(a.P, 1),
               "stages_k15": lambda: leg_stages(a.P, 15), "metrics": lambda: leg_metrics(a.P)}[a.leg]()
        print("EVAL_TIMING_JSON " + json.dumps(res), flush=True)
        return 0
    result = {"P": a.P, "legs": {}}       # (this process never opens the device: the legs do, one at a time)
    rc = 0
    for leg, limit in LEGS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--P", str(a.P)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("EVAL_TIMING_JSON ")]
        if r.returncode != 0 or not lines:
            result["legs"][leg] = {"failed": r.returncode, "stderr": r.stderr[-2000:]}
            rc = 1
            break                          # a leg that failed, faulted or ran out of time: nothing more runs on the device
        result["legs"][leg] = json.loads(lines[-1][len("EVAL_TIMING_JSON "):])
        print(leg, json.dumps(result["legs"][leg]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", a.out)
    return rc


if __name__ == "__main__":
    sys.exit(main())

"""Times the visual reports (deblurgs_amd/report.py) on an MI355X against the torch / host formulation they replace:

  (i)  one order statistic (rank int((n - 1) * 0.99)), the (1, 100) percentiles and four percentiles (8 ranks) of n floats -- report.order_stats /
       report.percentiles (radix select, results stay on the device) against torch.sort(x).values[rank] -- at
       n = 1920 x 1080 (one error map) and n = 50 x 1920 x 1080 (the depth images of a 50-frame path);
  (ii) the three images of evaluate(vis_dir=...) for 8 views at 1920 x 1080, from the tone-mapped render and the ground
       truth on the device to uint8 arrays on the host: report.view_report + one copy of the bytes, against the
       reference's formulation (test.py:122-126, utils/colorize.py): the error map in torch, .cpu(), np.percentile, the
       clip / scale / table lookup on the host, and save_image's byte conversion of the two float images.  Rendering, the
       metrics and the PNG encoder are the same on both sides and are left out.

The parent commit has neither capability: the baseline is the torch / host formulation.  Arms are interleaved over
`--rounds` rounds in ONE process after a warm-up of every shape; a window is `--reps` calls (ten times as many at the
smaller select size; one pass over the views in (ii)) between two host timestamps, the second after a device synchronise.  The measurement runs in a child process under `timeout`; if it fails, faults or
runs out of time nothing more is started on the device and the JSON says so.

    python tools/report_timing.py [--out profiles/report_timing.json]
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

SIZES = {"1920x1080": 1920 * 1080, "50x1920x1080": 50 * 1920 * 1080}


def _window(fn, reps, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(rounds, reps, views):
    import numpy as np
    import torch
    from deblurgs_amd import report
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "calls_per_window": reps, "select": {}, "views": {}}
    # ---- (i) the select against a sort
    for name, n in SIZES.items():
        g = torch.Generator(device="cuda").manual_seed(n % 1000)
        x = (torch.randn(n, device="cuda", generator=g) * 0.05).abs_()
        rank = report.clip_rank(n, 0.99)
        arms = {"order_stats": lambda: report.order_stats(x, [rank]),
                "percentiles_1_100": lambda: report.percentiles(x, (1.0, 100.0)),
                "percentiles_4": lambda: report.percentiles(x, (0.0, 37.5, 50.0, 99.0)),     # 8 ranks in one select
                "torch_sort": lambda: torch.sort(x).values[rank]}
        first = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        same = bool(first["order_stats"][0] == first["torch_sort"])
        want = np.percentile(x.cpu().numpy(), (1, 100))
        times = {k: [] for k in arms}
        r = reps * 10 if n < 10**7 else reps       # (tens of milliseconds per window at either size)
        for _ in range(rounds):
            for k, fn in arms.items():
                times[k].append(_window(fn, r, torch) * 1e6)
        med = {k: statistics.median(v) for k, v in times.items()}
        res["select"][name] = {"n": n, "us_per_call": times, "median_us": med, "order_stat_equals_sort": same,
                               "percentiles_equal_numpy": bool((first["percentiles_1_100"].cpu().numpy() == want).all()),
                               "tmp_bytes": int(report._lib.lib().dgs_order_stats_tmp_bytes(n, 1)),
                               "sort_over_order_stats": med["torch_sort"] / med["order_stats"],
                               "sort_over_percentiles": med["torch_sort"] / med["percentiles_1_100"],
                               "sort_over_percentiles_4": med["torch_sort"] / med["percentiles_4"]}
        del x, first
    # ---- (ii) the images of a test view
    H, W = 1080, 1920
    g = torch.Generator(device="cuda").manual_seed(7)
    gts = torch.rand(views, 3, H, W, device="cuda", generator=g)
    images = (gts + 0.03 * torch.randn(views, 3, H, W, device="cuda", generator=g)).contiguous()
    lut = report.jet_table(True)

    def device_arm():
        out = []
        for i in range(views):
            render_u8, gt_u8, error_u8 = report.view_report(images[i:i + 1], gts[i:i + 1], "identity")
            out.append(torch.stack([gt_u8[0], render_u8[0], error_u8[0]]).cpu().numpy())
        return out

    def host_arm():
        out = []
        for i in range(views):
            image, gt = images[i], gts[i]
            x = torch.abs(gt - image).permute(1, 2, 0).mean(dim=-1).cpu().numpy()
            vmin, vmax = np.percentile(x, (1, 100))
            vmax += 1e-6
            d = (np.clip(x, vmin, vmax) - vmin) / (vmax - vmin)
            err = lut[np.minimum((d * 256).astype(np.int64), 255)][..., :3]
            b = [t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy() for t in (gt, image)]
            out.append(np.stack([b[0], b[1], err]))
        return out

    arms = {"device": device_arm, "host": host_arm}
    first = {k: fn() for k, fn in arms.items()}
    differ = int(sum((a != b).sum() for a, b in zip(first["device"], first["host"])))
    del first
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(_window(fn, 1, torch) * 1e3 / views)
    med = {k: statistics.median(v) for k, v in times.items()}
    res["views"] = {"views": views, "H": H, "W": W, "ms_per_view": times, "median_ms_per_view": med,
                    "bytes_differing": differ, "host_over_device": med["host"] / med["device"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("REPORT_TIMING_JSON " + json.dumps(measure(a.rounds, a.reps, a.views)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--rounds", str(a.rounds),
           "--reps", str(a.reps), "--views", str(a.views)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("REPORT_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("REPORT_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

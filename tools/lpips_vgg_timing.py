"""Times LPIPS-vgg (deblurgs_amd/lpips.py) on an MI355X for one 1920 x 1080 pair:

  * each of the thirteen layer shapes (both images of the pair) on three arms: dgs_conv3x3_bias_relu (conv3x3_kernel: the
    halo-tile kernel), dgs_conv2d_bias_relu (conv_kernel: the generic gather kernel, the baseline -- the code the library
    had before the halo kernel, in the same process) and F.conv2d + relu (whatever MIOpen picks); ms and TFLOP/s
    (2 Cout 9 Cin N flops over the time) per layer and arm;
  * the whole dgs_lpips_vgg against the package's torch expressions (lpips._layers_torch), ms per pair.

The rules are tools/lpips_timing.py's: the arms are interleaved over `--rounds` rounds in ONE process after a warm-up; a
window is `--reps` calls between two host timestamps, the second after a device synchronise; the median over the rounds
is reported.  `decision`: per layer, conv3x3_kernel wins when it is more than 1.5 % below the generic kernel in EVERY
round (the project's rule, applied once; a layer that is not on the same side in every round stays on the generic
kernel).  The weights are seeded random numbers of the layers' shapes (He-scaled): no weight file is needed and no
timing depends on their values.  The measurement runs in a
child process under `timeout`; if it fails, faults or runs out of time nothing more is started on the device and the JSON
says so.

    python tools/lpips_vgg_timing.py [--out profiles/lpips_vgg_timing.json]
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

RULE = 0.015


def _window(fn, reps, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(rounds, reps, W, H, skip_torch_pair):
    import torch
    import torch.nn.functional as F
    from deblurgs_amd import lpips as lp
    g = torch.Generator().manual_seed(12)
    conv_w = [torch.randn((co, ci, 3, 3), generator=g) * (2.0 / (ci * 9)) ** 0.5 for co, ci in zip(lp.VGG_COUT, lp.VGG_CIN)]
    conv_b = [torch.randn((co,), generator=g) * 0.05 for co in lp.VGG_COUT]
    lin = [torch.rand((1, c, 1, 1), generator=g) / c for c in lp.VGG_CHANNELS]
    w = lp.LPIPSVggWeights(conv_w, conv_b, lin).to("cuda")
    x = torch.rand((1, 3, H, W), generator=g).cuda()
    y = (0.7 * x + 0.3 * torch.rand((1, 3, H, W), generator=g).cuda()).contiguous()
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "calls_per_window": reps, "W": W, "H": H,
           "tmp_bytes": int(lp._lib.lib().dgs_lpips_vgg_tmp_bytes(W, H, 1)), "rule": RULE}
    with torch.no_grad():
        # ---- the thirteen layers one by one, at the shapes the pair's two images give them
        layers = []
        z = torch.cat([x, y])
        for i, tap in enumerate(lp.VGG_TAP):
            co, ci = lp.VGG_COUT[i], lp.VGG_CIN[i]
            zs = i == 0
            arms = {"conv3x3": lambda: lp.conv3x3_bias_relu(z, w.conv_w[i], w.conv_b[i], zscore=zs),
                    "generic": lambda: lp.conv2d_bias_relu(z, w.conv_w[i], w.conv_b[i], stride=1, padding=1, zscore=zs)}
            zt = z
            if zs:
                t = lambda a: torch.tensor(a, device="cuda")[None, :, None, None]
                zt = (z - t(lp.MEAN)) / t(lp.STD)
            arms["torch"] = lambda: F.relu(F.conv2d(zt, w.conv_w[i], w.conv_b[i], stride=1, padding=1))
            first = {k: fn() for k, fn in arms.items()}          # warm-up, and the arms agree
            torch.cuda.synchronize()
            out = first["conv3x3"]
            scale = float(first["torch"].abs().max())
            agree = {k: float((first[k] - first["torch"]).abs().max()) / scale for k in ("conv3x3", "generic")}
            n = out.shape[0] * out.shape[2] * out.shape[3]
            flop = 2.0 * co * ci * 9 * n
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():
                    times[k].append(_window(fn, reps, torch) * 1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            layers.append({"layer": i + 1, "Cin": ci, "Cout": co, "H": int(out.shape[2]), "W": int(out.shape[3]), "N": n,
                           "gflop": flop / 1e9, "ms": times, "median_ms": med,
                           "tflops": {k: flop / (v * 1e-3) / 1e12 for k, v in med.items()},
                           "max_difference_to_torch_over_max": agree,
                           "conv3x3_over_generic": med["conv3x3"] / med["generic"],
                           "conv3x3_over_generic_per_round": [a / b for a, b in zip(times["conv3x3"], times["generic"])],
                           "decision": "conv3x3" if all(a < (1.0 - RULE) * b for a, b in zip(times["conv3x3"], times["generic"]))
                           else "generic"})
            del first
            z = lp.maxpool2x2(out) if tap is not None and tap < 4 else out
            del out
        res["conv_layers"] = layers
        res["conv_gflop_per_pair"] = sum(l["gflop"] for l in layers)
        for k in ("conv3x3", "generic", "torch"):
            res[f"conv_ms_per_pair_{k}"] = sum(l["median_ms"][k] for l in layers)
        del z
        torch.cuda.empty_cache()
        # ---- the whole network
        arms = {"dgs_lpips_vgg": lambda: lp.lpips_layers(x, y, w)}
        if not skip_torch_pair:
            arms["torch_expressions"] = lambda: lp._layers_torch(x, y, w)
        first = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        res["values"] = {k: [float(v) for v in first[k][0]] for k in first}
        if not skip_torch_pair:
            a, b = first["dgs_lpips_vgg"][0].double(), first["torch_expressions"][0].double()
            res["max_rel_difference_between_the_paths"] = float(((a - b).abs() / b.abs()).max())
        times = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                times[k].append(_window(fn, reps, torch) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        res["pair"] = {"ms_per_pair": times, "median_ms_per_pair": med}
        if not skip_torch_pair:
            res["pair"]["torch_over_kernel"] = med["torch_expressions"] / med["dgs_lpips_vgg"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--skip-torch-pair", action="store_true", help="do not time the torch expressions of the whole network")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_vgg_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("LPIPS_VGG_TIMING_JSON " + json.dumps(measure(a.rounds, a.reps, a.width, a.height, a.skip_torch_pair)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--rounds", str(a.rounds),
           "--reps", str(a.reps), "--width", str(a.width), "--height", str(a.height)] + \
          (["--skip-torch-pair"] if a.skip_torch_pair else [])
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LPIPS_VGG_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("LPIPS_VGG_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

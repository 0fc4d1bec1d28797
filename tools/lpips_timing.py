"""Times LPIPS-alex (deblurgs_amd/lpips.py) on an MI355X, ms per 1920 x 1080 pair:

  (a) dgs_lpips_alex: the library's own kernels through the C ABI (lpips.lpips_layers on fp32 device tensors);
  (b) the package's torch-expression path (lpips._layers_torch: F.conv2d and friends, whatever algorithm MIOpen picks) on
      the same device with the same weights -- what a user could do before the operator existed.

and the achieved TFLOP/s of each of the five convolution layers on its own (dgs_conv2d_bias_relu at the layer's 1080p
shape with both images of a pair, 2 Cout K N flops over its time).

Arms are interleaved over `--rounds` rounds in ONE process after a warm-up; a window is `--reps` calls between two host
timestamps, the second after a device synchronise; the median over the rounds is reported.  The weights are seeded random
numbers of the layers' shapes (He-scaled): no weight file is needed, and no timing depends on their values.  The measurement
runs in a child process under `timeout`; if it fails, faults or runs out of time nothing more is started on the device and
the JSON says so.

    python tools/lpips_timing.py [--out profiles/lpips_timing.json]
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


def _window(fn, reps, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(rounds, reps, W, H):
    import torch
    from deblurgs_amd import lpips as lp
    g = torch.Generator().manual_seed(11)
    conv_w = [torch.randn((co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5 for co, ci, k, _, _, _ in lp.CONVS]
    conv_b = [torch.randn((co,), generator=g) * 0.05 for co in lp.CHANNELS]
    lin = [torch.rand((1, co, 1, 1), generator=g) / co for co in lp.CHANNELS]
    w = lp.LPIPSWeights(conv_w, conv_b, lin).to("cuda")
    x = torch.rand((1, 3, H, W), generator=g).cuda()
    y = (0.7 * x + 0.3 * torch.rand((1, 3, H, W), generator=g).cuda()).contiguous()
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "calls_per_window": reps, "W": W, "H": H,
           "tmp_bytes": int(lp._lib.lib().dgs_lpips_alex_tmp_bytes(W, H, 1))}
    with torch.no_grad():
        arms = {"dgs_lpips_alex": lambda: lp.lpips_layers(x, y, w), "torch_expressions": lambda: lp._layers_torch(x, y, w)}
        first = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        a, b = first["dgs_lpips_alex"][0].double(), first["torch_expressions"][0].double()
        res["values"] = {k: [float(v) for v in first[k][0]] for k in first}
        res["max_rel_difference_between_the_paths"] = float(((a - b).abs() / b.abs()).max())
        times = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                times[k].append(_window(fn, reps, torch) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        res["pair"] = {"ms_per_pair": times, "median_ms_per_pair": med,
                       "torch_over_kernel": med["torch_expressions"] / med["dgs_lpips_alex"]}
        # ---- the convolution layers one by one, at the shapes the pair's two images give them
        layers = []
        z = torch.cat([x, y])
        total_flop = 0.0
        for i, (co, ci, k, stride, pad, pool) in enumerate(lp.CONVS):
            run = lambda: lp.conv2d_bias_relu(z, w.conv_w[i], w.conv_b[i], stride=stride, padding=pad, zscore=(i == 0))
            out = run()
            flop = 2.0 * co * (ci * k * k) * (out.shape[0] * out.shape[2] * out.shape[3])
            total_flop += flop
            t = [_window(run, reps, torch) for _ in range(rounds)]
            m = statistics.median(t)
            layers.append({"layer": i + 1, "Cout": co, "K": ci * k * k, "N": out.shape[0] * out.shape[2] * out.shape[3],
                           "gflop": flop / 1e9, "median_ms": m * 1e3, "ms": [v * 1e3 for v in t], "tflops": flop / m / 1e12})
            z = torch.nn.functional.max_pool2d(out, 3, 2) if pool else out
        res["conv_layers"] = layers
        res["conv_gflop_per_pair"] = total_flop / 1e9
        res["conv_ms_per_pair"] = sum(l["median_ms"] for l in layers)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_timing.json"))
    ap.add_argument("--leg", action="store_true", help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        print("LPIPS_TIMING_JSON " + json.dumps(measure(a.rounds, a.reps, a.width, a.height)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", "--rounds", str(a.rounds),
           "--reps", str(a.reps), "--width", str(a.width), "--height", str(a.height)]
    r = subprocess.run(cmd, capture_output=True, text=True)       # (this process never opens the device)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LPIPS_TIMING_JSON ")]
    ok = r.returncode == 0 and bool(lines)
    result = json.loads(lines[-1][len("LPIPS_TIMING_JSON "):]) if ok else {"failed": r.returncode, "stderr": r.stderr[-2000:]}
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Times LPIPS-squeeze (deblurgs_amd/lpips.py) on an MI355X for one 1920 x 1080 pair:

  * each of the eight Fire modules at its shape (both images of the pair) on three arms: dgs_fire_bias_relu (fire_kernel:
    the whole module in one launch), the composition of the operators the library had before it -- conv2d_bias_relu
    1 x 1 for the squeeze and for the 1 x 1 expand, conv3x3_bias_relu for the 3 x 3 expand, torch.cat -- and F.conv2d +
    relu + cat (whatever MIOpen picks); ms and TFLOP/s (2 N (Cin S + S E1 + 9 S E3) flops over the time) per module and arm;
  * the first convolution (the generic kernel against F.conv2d) and the three ceil-mode pools (against F.max_pool2d);
  * the whole dgs_lpips_squeeze against the package's torch expressions (lpips._layers_torch), ms per pair.

The rules are tools/lpips_timing.py's: the arms are interleaved over `--rounds` rounds in ONE process after a warm-up; a
window is `--reps` calls between two host timestamps, the second after a device synchronise; the median over the rounds
is reported.  `verdict`: per module, "fused" when fire_kernel is more than 1.5 % below the composition in EVERY round,
"composition" when it is more than 1.5 % above it in every round, else "undecided" (the project's rule; the library keeps
the one fused path either way, the verdict is what DESIGN.md reports).  The weights are seeded random numbers of the
layers' shapes (He-scaled): no weight file is needed and no timing depends on their values.  The two measurements (the
layers; the whole network) run one after the other in child processes, each under its own `timeout`; if one fails,
faults or runs out of time nothing more is started on the device and the JSON says so.

    python tools/lpips_squeeze_timing.py [--out profiles/lpips_squeeze_timing.json]
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
TAG = "LPIPS_SQUEEZE_TIMING_JSON "


def _window(fn, reps, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def _interleaved(arms, rounds, reps, torch):
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(_window(fn, reps, torch) * 1e3)
    return times, {k: statistics.median(v) for k, v in times.items()}


def _weights(lp, torch, g):
    conv = lambda co, ci, k: torch.randn((co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
    bias = lambda co: torch.randn((co,), generator=g) * 0.05
    fire = [(conv(s, ci, 1), 0.1 + bias(s).abs(), conv(e, s, 1), bias(e), conv(e, s, 3), bias(e)) for ci, s, e in lp.SQUEEZE_FIRES]
    lin = [torch.rand((1, c, 1, 1), generator=g) / c for c in lp.SQUEEZE_CHANNELS]
    return lp.LPIPSSqueezeWeights(conv(64, 3, 3), bias(64), fire, lin).to("cuda")


def _inputs(torch, g, W, H):
    x = torch.rand((1, 3, H, W), generator=g).cuda()
    y = (0.7 * x + 0.3 * torch.rand((1, 3, H, W), generator=g).cuda()).contiguous()
    return x, y


def flops_per_pair(lp, W, H):
    """Multiply-adds x 2 of the 25 convolutions for the two images of a pair, from the layer shapes."""
    h, w = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    total = 2.0 * 2 * h * w * 64 * 27
    h, w = h // 2, w // 2
    for (ci, s, e), pool in zip(lp.SQUEEZE_FIRES, lp.SQUEEZE_POOL):
        total += 2.0 * 2 * h * w * (ci * s + s * e + 9 * s * e)
        if pool:
            h, w = h // 2, w // 2
    return total


def measure_layers(rounds, reps, W, H):
    import torch
    import torch.nn.functional as F
    from deblurgs_amd import lpips as lp
    g = torch.Generator().manual_seed(12)
    w = _weights(lp, torch, g)
    x, y = _inputs(torch, g, W, H)
    res = {}
    with torch.no_grad():
        z = torch.cat([x, y])
        t = lambda a: torch.tensor(a, device="cuda")[None, :, None, None]
        zt = (z - t(lp.MEAN)) / t(lp.STD)
        arms = {"generic": lambda: lp.conv2d_bias_relu(z, w.conv_w, w.conv_b, stride=2, padding=0, zscore=True),
                "torch": lambda: F.relu(F.conv2d(zt, w.conv_w, w.conv_b, stride=2))}
        first = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        out = first["generic"]
        n = out.shape[0] * out.shape[2] * out.shape[3]
        times, med = _interleaved(arms, rounds, reps, torch)
        res["first_conv"] = {"H": int(out.shape[2]), "W": int(out.shape[3]), "gflop": 2.0 * n * 64 * 27 / 1e9, "ms": times,
                             "median_ms": med,
                             "max_difference_to_torch_over_max": float((out - first["torch"]).abs().max() / first["torch"].abs().max())}
        del first
        pools, fires = [], []

        def pool(v):
            arms = {"kernel": lambda: lp.maxpool3x3s2_ceil(v), "torch": lambda: F.max_pool2d(v, 3, 2, ceil_mode=True)}
            first = {k: fn() for k, fn in arms.items()}
            torch.cuda.synchronize()
            times, med = _interleaved(arms, rounds, reps, torch)
            pools.append({"C": int(v.shape[1]), "H": int(v.shape[2]), "W": int(v.shape[3]), "ms": times, "median_ms": med,
                          "equal_to_torch": bool(torch.equal(first["kernel"], first["torch"]))})
            return first["kernel"]

        z = pool(out)
        del out
        for i, (six, (ci, s, e), pooled) in enumerate(zip(w.fire, lp.SQUEEZE_FIRES, lp.SQUEEZE_POOL)):
            zi = z

            def composed():
                sq = lp.conv2d_bias_relu(zi, six[0], six[1])
                return torch.cat([lp.conv2d_bias_relu(sq, six[2], six[3]), lp.conv3x3_bias_relu(sq, six[4], six[5])], dim=1)

            arms = {"fused": lambda: lp.fire_bias_relu(zi, six), "composition": composed, "torch": lambda: lp._fire_torch(zi, six)}
            first = {k: fn() for k, fn in arms.items()}
            torch.cuda.synchronize()
            out = first["fused"]
            scale = float(first["torch"].abs().max())
            agree = {k: float((first[k] - first["torch"]).abs().max()) / scale for k in ("fused", "composition")}
            n = out.shape[0] * out.shape[2] * out.shape[3]
            flop = 2.0 * n * (ci * s + s * e + 9 * s * e)
            times, med = _interleaved(arms, rounds, reps, torch)
            ratios = [a / b for a, b in zip(times["fused"], times["composition"])]
            verdict = "fused" if all(r < 1.0 - RULE for r in ratios) else ("composition" if all(r > 1.0 + RULE for r in ratios)
                                                                           else "undecided")
            fires.append({"fire": i + 1, "Cin": ci, "S": s, "E": e, "H": int(out.shape[2]), "W": int(out.shape[3]), "N": n,
                          "gflop": flop / 1e9, "ms": times, "median_ms": med,
                          "tflops": {k: flop / (v * 1e-3) / 1e12 for k, v in med.items()},
                          "max_difference_to_torch_over_max": agree, "fused_over_composition": med["fused"] / med["composition"],
                          "fused_over_composition_per_round": ratios, "fused_over_torch": med["fused"] / med["torch"],
                          "verdict": verdict})
            del first
            z = pool(out) if pooled else out
            del out
        res["fires"], res["pools"] = fires, pools
        for k in ("fused", "composition", "torch"):
            res[f"fire_ms_per_pair_{k}"] = sum(f["median_ms"][k] for f in fires)
        res["pool_ms_per_pair"] = {k: sum(p["median_ms"][k] for p in pools) for k in ("kernel", "torch")}
    return res


def measure_pair(rounds, reps, W, H):
    import torch
    from deblurgs_amd import lpips as lp
    g = torch.Generator().manual_seed(12)
    w = _weights(lp, torch, g)
    x, y = _inputs(torch, g, W, H)
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "calls_per_window": reps, "W": W, "H": H,
           "tmp_bytes": int(lp._lib.lib().dgs_lpips_squeeze_tmp_bytes(W, H, 1)), "rule": RULE,
           "gflop_per_pair": flops_per_pair(lp, W, H) / 1e9}
    with torch.no_grad():
        arms = {"dgs_lpips_squeeze": lambda: lp.lpips_layers(x, y, w), "torch_expressions": lambda: lp._layers_torch(x, y, w)}
        first = {k: fn() for k, fn in arms.items()}
        torch.cuda.synchronize()
        res["values"] = {k: [float(v) for v in first[k][0]] for k in first}
        a, b = first["dgs_lpips_squeeze"][0].double(), first["torch_expressions"][0].double()
        res["max_rel_difference_between_the_paths"] = float(((a - b).abs() / b.abs()).max())
        times, med = _interleaved(arms, rounds, reps, torch)
        res["pair"] = {"ms_per_pair": times, "median_ms_per_pair": med,
                       "torch_over_kernel": med["torch_expressions"] / med["dgs_lpips_squeeze"],
                       "kernel_tflops": res["gflop_per_pair"] / med["dgs_lpips_squeeze"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--limit", type=int, default=240, help="seconds each of the two measurements may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_squeeze_timing.json"))
    ap.add_argument("--leg", choices=("layers", "pair"), help="internal: measure in this process and print the JSON")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.leg:
        fn = measure_layers if a.leg == "layers" else measure_pair
        print(TAG + json.dumps(fn(a.rounds, a.reps, a.width, a.height)), flush=True)
        return 0
    result, ok = {}, True
    for leg in ("pair", "layers"):                                    # (this process never opens the device)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds",
               str(a.rounds), "--reps", str(a.reps), "--width", str(a.width), "--height", str(a.height)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not lines:
            result["failed"] = {"leg": leg, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            ok = False
            break                                                     # nothing more is started on the device
        result.update(json.loads(lines[-1][len(TAG):]))
    result["note"] = "one box, one run"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

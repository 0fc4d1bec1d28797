"""Regenerates tests/golden/metrics_golden.npz by IMPORTING the reference's own metrics from /root/reference:
utils/loss_utils.py ssim and utils/image_utils.py psnr, each evaluated in fp32 and in fp64 on seeded image pairs.

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_metrics.py
The fixture is data (the seeded inputs and the reference's outputs); no reference source text is stored.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    a = rng.random((3, 32, 40))
    out["noise"] = (a, rng.random((3, 32, 40)))
    out["noise_close"] = (a, np.clip(a + rng.normal(0, 0.03, a.shape), 0, 1))
    y, x = np.mgrid[0:48, 0:64]
    g = np.stack([x / 63.0, y / 47.0, (x + y) / 110.0])
    out["gradient"] = (g, 0.9 * g + 0.05 + rng.normal(0, 0.01, g.shape))
    f = np.zeros((3, 96, 128))
    f[:, :, 48:] = 0.8
    f[1, 30:, :] = 0.35
    f2 = np.roll(f, 2, axis=2) * 0.95
    out["flat_edge"] = (f, f2)
    out["out_of_range"] = (rng.normal(0.5, 0.6, (3, 24, 28)), rng.normal(0.5, 0.6, (3, 24, 28)) * 1.2 - 0.3)
    o = rng.random((3, 37, 53))
    out["odd_size"] = (o, np.clip(o + rng.normal(0, 0.1, o.shape), 0, 1))
    out["tiny"] = (rng.random((3, 7, 9)), rng.random((3, 7, 9)))
    i = rng.random((3, 20, 25))
    out["identical"] = (i, i.copy())
    # values representable in fp16: the fixture stores them as fp16 (half the bytes), the tests widen them exactly
    return {k: (a.astype(np.float16).astype(np.float32), b.astype(np.float16).astype(np.float32)) for k, (a, b) in out.items()}


def main():
    from utils.image_utils import psnr
    from utils.loss_utils import ssim
    data = {"names": np.array(list(cases().keys()))}
    with torch.no_grad():
        for name, (a, b) in cases().items():
            ta, tb = torch.from_numpy(a), torch.from_numpy(b)
            data[name + "_a"], data[name + "_b"] = a.astype(np.float16), b.astype(np.float16)
            data[name + "_psnr32"] = np.float64(psnr(ta, tb).mean().item())
            data[name + "_psnr64"] = np.float64(psnr(ta.double(), tb.double()).mean().item())
            data[name + "_ssim32"] = np.float64(ssim(ta, tb).mean().item())
            data[name + "_ssim64"] = np.float64(ssim(ta.double(), tb.double()).mean().item())
            print(name, a.shape, data[name + "_psnr32"], data[name + "_psnr64"], data[name + "_ssim32"], data[name + "_ssim64"])
    np.savez_compressed(os.path.join(HERE, "metrics_golden.npz"), **data)


if __name__ == "__main__":
    main()

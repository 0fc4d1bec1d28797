"""Regenerates tests/golden/lpips_golden.npz by IMPORTING the reference's own lpipsPyTorch.modules.lpips.LPIPS from
/root/reference (tap indices, normalisation, z-score constants and key renaming are the real code's) and evaluating it
in fp32 and in fp64 on the seeded image pairs of tests/lpips_cases.py with the seeded stand-in weights of the same file.

torchvision is not installed in the build container and nothing may be downloaded, so two names the reference resolves
at import / construction time are stood in for:
    torchvision.models.alexnet()           an object whose `.features` is an nn.Sequential of AlexNet's architecture,
                                           loaded with the recipe's weights
    torch.hub.load_state_dict_from_url     returns the recipe's lin weights under the published `lin{i}.model.1.weight`
                                           names (the reference renames them itself)

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_lpips.py
The fixture is data (the reference's outputs); no reference source text, no weights and no images are stored.
Per pair NAME:  NAME_total32   the reference's fp32 result (the [1,1,1,1] tensor's value)
                NAME_layers64  the five per-layer values of the same module in fp64 (`.double()`)
                NAME_layers32  the same in fp32
                NAME_rel32     |layers32 - layers64| / layers64
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_cases as lc  # noqa: E402


def _alexnet_features():
    return nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))


def _stand_ins():
    feats_sd, lin_sd = lc.state_dicts()

    def alexnet(*args, **kwargs):
        net = types.SimpleNamespace(features=_alexnet_features())
        net.features.load_state_dict({k[len("features."):]: v for k, v in feats_sd.items()})
        return net

    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.alexnet = alexnet
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    torch.hub.load_state_dict_from_url = lambda url, **kw: {k: v.clone() for k, v in lin_sd.items()}


def _layers(model, x, y):
    """The five per-layer values of LPIPS.forward (lpips.py:28-34) before its final sum."""
    fx, fy = model.net(x), model.net(y)
    return np.array([float(l((a - b) ** 2).mean((2, 3), True).item()) for a, b, l in zip(fx, fy, model.lin)])


def main():
    _stand_ins()
    sys.path.insert(0, REF)
    from lpipsPyTorch.modules.lpips import LPIPS
    m32 = LPIPS("alex", "0.1").eval()
    m64 = LPIPS("alex", "0.1").eval().double()
    data = {"names": np.array(lc.NAMES)}
    with torch.no_grad():
        for name, (x, y) in lc.image_pairs().items():
            tx, ty = torch.from_numpy(x)[None], torch.from_numpy(y)[None]
            total32 = m32(tx, ty)
            assert tuple(total32.shape) == (1, 1, 1, 1)
            l32, l64 = _layers(m32, tx, ty), _layers(m64, tx.double(), ty.double())
            assert abs(float(m64(tx.double(), ty.double()).item()) - l64.sum()) <= 1e-12 * l64.sum()
            data[name + "_total32"] = np.float64(total32.item())
            data[name + "_layers32"], data[name + "_layers64"] = l32, l64
            data[name + "_rel32"] = np.abs(l32 - l64) / np.abs(l64)
            print(name, x.shape, data[name + "_total32"], l64, data[name + "_rel32"])
        # the batch quirk: N = 2 pairs in one call give ONE value, the sum over the batch
        p = lc.image_pairs()
        a, b = p["noise_37x53"], p["blend_37x53"]
        tx, ty = torch.from_numpy(np.stack([a[0], b[0]])), torch.from_numpy(np.stack([a[1], b[1]]))
        both = m64(tx.double(), ty.double())
        assert tuple(both.shape) == (1, 1, 1, 1)
        data["batch2_total64"] = np.float64(both.item())
        # the smallest accepted image: 30 x 30 raises in the reference
        try:
            m32(torch.zeros(1, 3, 30, 30), torch.zeros(1, 3, 30, 30))
            raise AssertionError("the reference accepted 30 x 30")
        except RuntimeError:
            pass
    np.savez_compressed(os.path.join(HERE, "lpips_golden.npz"), **data)


if __name__ == "__main__":
    main()

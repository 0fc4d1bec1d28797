"""Regenerates tests/golden/lpips_vgg_golden.npz by IMPORTING the reference's own lpipsPyTorch.modules.lpips.LPIPS from
/root/reference (tap indices, normalisation, z-score constants and key renaming are the real code's) and evaluating
LPIPS('vgg', '0.1') in fp32 and in fp64 on the seeded image pairs of tests/lpips_vgg_cases.py with the seeded stand-in
weights of the same file.

torchvision is not installed in the build container and nothing may be downloaded, so the names the reference resolves
at import / construction time are stood in for:
    torchvision.models.vgg16(weights=...)  an object whose `.features` is an nn.Sequential of VGG16's architecture,
                                           loaded with the recipe's weights
    torchvision.models.VGG16_Weights       a namespace with IMAGENET1K_V1
    torch.hub.load_state_dict_from_url     returns the recipe's lin weights under the published `lin{i}.model.1.weight`
                                           names (the reference renames them itself)

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_lpips_vgg.py
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
import lpips_vgg_cases as lc  # noqa: E402

VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def _vgg16_features():
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def _stand_ins():
    feats_sd, lin_sd = lc.state_dicts()

    def vgg16(*args, **kwargs):
        net = types.SimpleNamespace(features=_vgg16_features())
        net.features.load_state_dict({k[len("features."):]: v for k, v in feats_sd.items()})
        return net

    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = vgg16
    tv.models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
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
    m32 = LPIPS("vgg", "0.1").eval()
    m64 = LPIPS("vgg", "0.1").eval().double()
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
            # no bar is an accident of cancellation
            assert data[name + "_rel32"].max() >= 1e-7, (name, data[name + "_rel32"])
            print(name, x.shape, data[name + "_total32"], l64, data[name + "_rel32"])
        # the batch quirk: N = 2 pairs in one call give ONE value, the sum over the batch
        p = lc.image_pairs()
        a, b = p["noise_37x53"], p["blend_37x53"]
        tx, ty = torch.from_numpy(np.stack([a[0], b[0]])), torch.from_numpy(np.stack([a[1], b[1]]))
        both = m64(tx.double(), ty.double())
        assert tuple(both.shape) == (1, 1, 1, 1)
        data["batch2_total64"] = np.float64(both.item())
        # the smallest accepted image is 16 x 16: 15 rows or 15 columns raise in the reference
        for shape in ((1, 3, 15, 16), (1, 3, 16, 15)):
            try:
                m32(torch.zeros(shape), torch.zeros(shape))
                raise AssertionError(f"the reference accepted {shape}")
            except RuntimeError:
                pass
    np.savez_compressed(os.path.join(HERE, "lpips_vgg_golden.npz"), **data)


if __name__ == "__main__":
    main()

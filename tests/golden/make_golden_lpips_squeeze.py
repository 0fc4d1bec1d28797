"""Regenerates tests/golden/lpips_squeeze_golden.npz by IMPORTING the reference's own lpipsPyTorch.modules.lpips.LPIPS from
/root/reference (tap indices, normalisation, z-score constants and key renaming are the real code's) and evaluating
LPIPS('squeeze', '0.1') in fp32 and in fp64 on the seeded image pairs of tests/lpips_squeeze_cases.py with the seeded
stand-in weights of the same file.

torchvision is not installed in the build container and nothing may be downloaded, so the names the reference resolves
at import / construction time are stood in for:
    torchvision.models.squeezenet1_1(True)  an object whose `.features` is an nn.Sequential of SqueezeNet 1.1's published
                                            architecture (conv 3x3 /2, ReLU, MaxPool2d(3, 2, ceil_mode=True), Fire modules
                                            with the submodules `squeeze`, `expand1x1`, `expand3x3`), loaded with the
                                            recipe's weights
    torch.hub.load_state_dict_from_url      returns the recipe's lin weights under the published `lin{i}.model.1.weight`
                                            names (the reference renames them itself)

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_lpips_squeeze.py
The fixture is data (the reference's outputs); no reference source text, no weights and no images are stored.
Per pair NAME:  NAME_total32   the reference's fp32 result (the [1,1,1,1] tensor's value)
                NAME_layers64  the seven per-layer values of the same module in fp64 (`.double()`)
                NAME_layers32  the same in fp32
                NAME_rel32     |layers32 - layers64| / layers64
and batch2_total64, the reference's one value for the two 37 x 53 pairs in one call.
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
import lpips_squeeze_cases as lc  # noqa: E402


class Fire(nn.Module):
    def __init__(self, cin, s, e1, e3):
        super().__init__()
        self.squeeze = nn.Conv2d(cin, s, kernel_size=1)
        self.squeeze_activation = nn.ReLU(inplace=True)
        self.expand1x1 = nn.Conv2d(s, e1, kernel_size=1)
        self.expand1x1_activation = nn.ReLU(inplace=True)
        self.expand3x3 = nn.Conv2d(s, e3, kernel_size=3, padding=1)
        self.expand3x3_activation = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.squeeze_activation(self.squeeze(x))
        return torch.cat([self.expand1x1_activation(self.expand1x1(x)), self.expand3x3_activation(self.expand3x3(x))], 1)


def _squeezenet1_1_features():
    pool = lambda: nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True)
    f = [Fire(ci, s, e, e) for ci, s, e in lc.FIRES]
    return nn.Sequential(nn.Conv2d(3, 64, kernel_size=3, stride=2), nn.ReLU(inplace=True), pool(), f[0], f[1], pool(), f[2],
                         f[3], pool(), f[4], f[5], f[6], f[7])


def _stand_ins():
    feats_sd, lin_sd = lc.state_dicts()

    def squeezenet1_1(*args, **kwargs):
        net = types.SimpleNamespace(features=_squeezenet1_1_features())
        net.features.load_state_dict({k[len("features."):]: v for k, v in feats_sd.items()})
        return net

    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.squeezenet1_1 = squeezenet1_1
    # the reference's module builds all three class bodies at import; only SqueezeNet is constructed here
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    torch.hub.load_state_dict_from_url = lambda url, **kw: {k: v.clone() for k, v in lin_sd.items()}


def _layers(model, x, y):
    """The seven per-layer values of LPIPS.forward (lpips.py:28-34) before its final sum."""
    fx, fy = model.net(x), model.net(y)
    assert len(fx) == 7
    return np.array([float(l((a - b) ** 2).mean((2, 3), True).item()) for a, b, l in zip(fx, fy, model.lin)])


def main():
    _stand_ins()
    sys.path.insert(0, REF)
    from lpipsPyTorch.modules.lpips import LPIPS
    m32 = LPIPS("squeeze", "0.1").eval()
    m64 = LPIPS("squeeze", "0.1").eval().double()
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
        # the smallest accepted image is 17 x 17: 16 rows or 16 columns raise in the reference (in the third pool)
        for shape in ((1, 3, 16, 17), (1, 3, 17, 16)):
            try:
                m32(torch.zeros(shape), torch.zeros(shape))
                raise AssertionError(f"the reference accepted {shape}")
            except RuntimeError:
                pass
        assert [tuple(f.shape[2:]) for f in m32.net(torch.zeros(1, 3, 17, 17))] == [(8, 8), (4, 4), (2, 2)] + [(1, 1)] * 4
    np.savez_compressed(os.path.join(HERE, "lpips_squeeze_golden.npz"), **data)


if __name__ == "__main__":
    main()

"""What the LPIPS-vgg tests and tests/golden/make_golden_lpips_vgg.py share: the seeded recipe of the stand-in network
weights and of the image pairs (np.random.RandomState: its stream is frozen), the fixture, and the bar of a pair.

The weights are not stored (59 MB).  Draw order from RandomState(WEIGHT_SEED), everything drawn in float64 and then
rounded to float32:
    per convolution (in network order)   weight = standard_normal([Cout,Cin,3,3]) * sqrt(2 / (9 Cin)),
                                         then bias = standard_normal([Cout]) * 0.05
    then per tap (in network order)      lin = random_sample([1,C,1,1]) / C
The images come from RandomState(IMAGE_SEED): per size of SIZES, x = random_sample([3,H,W]) then y = random_sample([3,H,W]);
then the blended pair at BLEND_SIZE: x = random_sample, noise = random_sample, y = 0.7 x + 0.3 noise.
What a size pins: 16 x 16 a 1 x 1 last tap whose 3 x 3 windows have eight of nine weights on padding; 17 x 23 floor pools
that drop a row and a column; 37 x 53 a second, ragged 32-column tile; 70 x 33 many row tiles, a 1-column tile and H > W;
64 x 200 several full tiles.

The bar of a pair is lpips_cases' rule: BAR_FACTOR x the largest of its five recorded fp32-vs-fp64 differences of the
reference's own module.
"""
import os

import numpy as np

from lpips_cases import BAR_FACTOR

WEIGHT_SEED, IMAGE_SEED = 20262, 20263
COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CIN = (3,) + COUT[:-1]
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
LIN_CHANNELS = (64, 128, 256, 512, 512)
SIZES = ((16, 16), (17, 23), (37, 53), (70, 33), (64, 200))                           # H, W
BLEND_SIZE = (37, 53)
NAMES = tuple(f"noise_{h}x{w}" for h, w in SIZES) + ("blend_37x53",)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_vgg_golden.npz")


def weight_arrays():
    """(features state dict under torchvision's `features.N.*` names, lin state dict under the published names) as float32
    numpy arrays."""
    rng = np.random.RandomState(WEIGHT_SEED)
    feats, lin = {}, {}
    for idx, co, ci in zip(FEATURE_INDEX, COUT, CIN):
        feats[f"features.{idx}.weight"] = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        feats[f"features.{idx}.bias"] = (rng.standard_normal((co,)) * 0.05).astype(np.float32)
    for i, c in enumerate(LIN_CHANNELS):
        lin[f"lin{i}.model.1.weight"] = (rng.random_sample((1, c, 1, 1)) / c).astype(np.float32)
    return feats, lin


def state_dicts():
    import torch
    feats, lin = weight_arrays()
    return {k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in lin.items()}


def image_pairs():
    """{name: (x, y)} float32 [3,H,W] arrays, in NAMES order."""
    rng = np.random.RandomState(IMAGE_SEED)
    out = {}
    for name, (h, w) in zip(NAMES, SIZES):
        x = rng.random_sample((3, h, w))
        y = rng.random_sample((3, h, w))
        out[name] = (x.astype(np.float32), y.astype(np.float32))
    h, w = BLEND_SIZE
    x = rng.random_sample((3, h, w))
    noise = rng.random_sample((3, h, w))
    out[NAMES[-1]] = (x.astype(np.float32), (0.7 * x + 0.3 * noise).astype(np.float32))
    return out


_cache = {}


def weights():
    """The LPIPSVggWeights of the recipe (CPU), built once."""
    if "w" not in _cache:
        from deblurgs_amd.lpips import LPIPSVggWeights
        _cache["w"] = LPIPSVggWeights.from_state_dicts(*state_dicts())
    return _cache["w"]


def pairs():
    if "p" not in _cache:
        _cache["p"] = image_pairs()
    return _cache["p"]


def fixture():
    if "f" not in _cache:
        _cache["f"] = dict(np.load(FIXTURE))
    return _cache["f"]


def bar(name):
    """The relative bar of a pair: BAR_FACTOR x the largest of its five recorded fp32-vs-fp64 differences."""
    return BAR_FACTOR * float(np.max(fixture()[name + "_rel32"]))


def check_against_fixture(name, got, what):
    """got: six numbers (total, layer 1..5) against the fixture's fp64 values; prints every figure before it asserts."""
    f = fixture()
    want = np.concatenate([[f[name + "_layers64"].sum()], f[name + "_layers64"]])
    got = np.asarray(got, dtype=np.float64)
    rel = np.abs(got - want) / np.abs(want)
    b = bar(name)
    print(f"{what} {name}: rel err total {rel[0]:.3e} layers {np.array2string(rel[1:], precision=3)} bar {b:.3e}")
    assert np.all(np.isfinite(got)) and np.all(rel <= b), (what, name, rel, b)
    return rel

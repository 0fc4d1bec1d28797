"""What the LPIPS tests and tests/golden/make_golden_lpips.py share: the seeded recipe of the stand-in network weights
and of the image pairs (np.random.RandomState: its stream is frozen), the fixture, and the bar of a pair.

The weights are not stored (9.9 MB).  Draw order from RandomState(WEIGHT_SEED), everything drawn in float64 and then
rounded to float32:
    per convolution (in network order)   weight = standard_normal([Cout,Cin,k,k]) * sqrt(2 / (Cin k k)),
                                         then bias = standard_normal([Cout]) * 0.05
    then per tap (in network order)      lin = random_sample([1,C,1,1]) / C
The images come from RandomState(IMAGE_SEED): per size of SIZES, x = random_sample([3,H,W]) then y = random_sample([3,H,W]);
then the blended pair at BLEND_SIZE: x = random_sample, noise = random_sample, y = 0.7 x + 0.3 noise.
"""
import os

import numpy as np

WEIGHT_SEED, IMAGE_SEED = 20260, 20261
CONVS = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))      # Cout, Cin, k
FEATURE_INDEX = (0, 3, 6, 8, 10)
SIZES = ((31, 31), (37, 53), (64, 200), (135, 240))                                  # H, W
BLEND_SIZE = (37, 53)
NAMES = tuple(f"noise_{h}x{w}" for h, w in SIZES) + ("blend_37x53",)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_golden.npz")
BAR_FACTOR = 8.0        # x the largest of a pair's five recorded fp32-vs-fp64 differences of the reference itself


def weight_arrays():
    """(features state dict under torchvision's `features.N.*` names, lin state dict under the published names) as float32
    numpy arrays."""
    rng = np.random.RandomState(WEIGHT_SEED)
    feats, lin = {}, {}
    for idx, (co, ci, k) in zip(FEATURE_INDEX, CONVS):
        feats[f"features.{idx}.weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        feats[f"features.{idx}.bias"] = (rng.standard_normal((co,)) * 0.05).astype(np.float32)
    for i, (co, _, _) in enumerate(CONVS):
        lin[f"lin{i}.model.1.weight"] = (rng.random_sample((1, co, 1, 1)) / co).astype(np.float32)
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
    """The LPIPSWeights of the recipe (CPU), built once."""
    if "w" not in _cache:
        from deblurgs_amd.lpips import LPIPSWeights
        _cache["w"] = LPIPSWeights.from_state_dicts(*state_dicts())
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

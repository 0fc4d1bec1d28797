"""What the LPIPS-squeeze tests and tests/golden/make_golden_lpips_squeeze.py share: the seeded recipe of the stand-in
network weights and of the image pairs (np.random.RandomState: its stream is frozen), the fixture, and the bar of a pair.

The weights are not stored (2.9 MB).  Draw order from RandomState(WEIGHT_SEED), everything drawn in float64 and then
rounded to float32:
    the first convolution                weight = standard_normal([64,3,3,3]) * sqrt(2 / 27), bias = standard_normal([64]) * 0.05
    per Fire module (in network order)   for squeeze, expand1x1, expand3x3 in this order:
                                         weight = standard_normal([Cout,Cin,k,k]) * sqrt(2 / (Cin k k)), then
                                         bias = standard_normal([Cout]) * 0.05 -- but the SQUEEZE bias is
                                         0.1 + 0.05 |standard_normal([S])|: strictly positive, so that a squeeze map whose
                                         padding held relu(bias) instead of 0 would change every edge pixel of the 3 x 3 expand
    then per tap (in network order)      lin = random_sample([1,C,1,1]) / C
The images come from RandomState(IMAGE_SEED): per size of SIZES, x = random_sample([3,H,W]) then y = random_sample([3,H,W]);
then the blended pair at BLEND_SIZE: x = random_sample, noise = random_sample, y = 0.7 x + 0.3 noise.
What a size pins (the first map is ((H-3)/2+1) x ((W-3)/2+1), every ceil-mode pool halves it): 17 x 17 the minimum -- the
last four taps are 1 x 1, so eight of nine 3 x 3 weights sit on padding, and every pool has a ragged window; 18 x 20 an
8 x 9 first map: even and odd pool inputs side by side; 37 x 53 maps of 18 x 26, 9 x 13, 4 x 6 and 2 x 3; 40 x 135 a
67-wide first map and 33-wide Fire maps: a 1-column second tile; 70 x 33 H > W and many row tiles; 64 x 200 99- and
49-wide maps: several full tiles and a ragged one.

The bar of a pair is lpips_cases' rule: BAR_FACTOR x the largest of its seven recorded fp32-vs-fp64 differences of the
reference's own module.
"""
import os

import numpy as np

from lpips_cases import BAR_FACTOR

WEIGHT_SEED, IMAGE_SEED = 20264, 20265
FIRES = ((64, 16, 64), (128, 16, 64), (128, 32, 128), (256, 32, 128), (256, 48, 192), (384, 48, 192), (384, 64, 256),
         (512, 64, 256))                                                               # Cin, S, E
FIRE_INDEX = (3, 4, 6, 7, 9, 10, 11, 12)
LIN_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
SIZES = ((17, 17), (18, 20), (37, 53), (40, 135), (70, 33), (64, 200))                  # H, W
BLEND_SIZE = (37, 53)
NAMES = tuple(f"noise_{h}x{w}" for h, w in SIZES) + ("blend_37x53",)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_squeeze_golden.npz")


def weight_arrays():
    """(features state dict under torchvision's `features.N.*` names, lin state dict under the published names) as float32
    numpy arrays."""
    rng = np.random.RandomState(WEIGHT_SEED)
    feats, lin = {}, {}

    def conv(key, co, ci, k, positive_bias=False):
        feats[key + ".weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        b = rng.standard_normal((co,))
        feats[key + ".bias"] = ((0.1 + 0.05 * np.abs(b)) if positive_bias else b * 0.05).astype(np.float32)

    conv("features.0", 64, 3, 3)
    for idx, (ci, s, e) in zip(FIRE_INDEX, FIRES):
        conv(f"features.{idx}.squeeze", s, ci, 1, positive_bias=True)
        conv(f"features.{idx}.expand1x1", e, s, 1)
        conv(f"features.{idx}.expand3x3", e, s, 3)
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
    """The LPIPSSqueezeWeights of the recipe (CPU), built once."""
    if "w" not in _cache:
        from deblurgs_amd.lpips import LPIPSSqueezeWeights
        _cache["w"] = LPIPSSqueezeWeights.from_state_dicts(*state_dicts())
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
    """The relative bar of a pair: BAR_FACTOR x the largest of its seven recorded fp32-vs-fp64 differences."""
    return BAR_FACTOR * float(np.max(fixture()[name + "_rel32"]))


def check_against_fixture(name, got, what):
    """got: eight numbers (total, layer 1..7) against the fixture's fp64 values; prints every figure before it asserts."""
    f = fixture()
    want = np.concatenate([[f[name + "_layers64"].sum()], f[name + "_layers64"]])
    got = np.asarray(got, dtype=np.float64)
    rel = np.abs(got - want) / np.abs(want)
    b = bar(name)
    print(f"{what} {name}: rel err total {rel[0]:.3e} layers {np.array2string(rel[1:], precision=3)} bar {b:.3e}")
    assert np.all(np.isfinite(got)) and np.all(rel <= b), (what, name, rel, b)
    return rel

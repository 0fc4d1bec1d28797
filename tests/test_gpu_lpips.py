"""GPU tests of LPIPS-alex on the device (csrc/lpips.hip through deblurgs_amd/lpips.py): dgs_lpips_alex against the
reference's own module (tests/golden/lpips_golden.npz, the bar of tests/lpips_cases.py), its bitwise properties, the
convolution kernel on its own against torch in fp64, and evaluate(..., lpips=).  Every case is a few ms of device work."""
import numpy as np
import pytest

import lpips_cases as lc
from helpers import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    """The recipe's weights and the five pairs on the device (moved once, never written to)."""
    import torch
    w = lc.weights().to(gpu)
    pairs = {n: (torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)) for n, (x, y) in lc.pairs().items()}
    return w, pairs


@pytest.mark.parametrize("name", lc.NAMES)
def test_kernel_matches_the_reference(dev, name):
    """Per layer and in total against the fixture's fp64 values.  31 x 31: N = 2 pixels in the last three layers and
    windows that are mostly padding; 37 x 53: rows and columns that stride 4 and the floor pools must ignore; 64 x 200 and
    135 x 240: several blocks of pixels with a ragged last one."""
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs[name]
    got = lp.lpips_layers(x, y, w)
    assert tuple(got.shape) == (1, 6) and got.dtype.is_floating_point and got.is_cuda
    lc.check_against_fixture(name, got[0].cpu().numpy(), "dgs_lpips_alex")
    # the reference's signature: one [1,1,1,1] tensor
    one = lp.lpips(x, y, w)
    assert tuple(one.shape) == (1, 1, 1, 1) and float(one) == float(got[0, 0])


def test_three_pairs_in_one_call_equal_three_single_calls_bitwise(dev):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    names = ["noise_37x53", "blend_37x53", "noise_37x53"]
    x = torch.stack([pairs[n][0] for n in names])
    y = torch.stack([pairs[n][1] for n in names])
    y[2] = pairs["blend_37x53"][1]              # a third, different pair of the same size
    both = lp.lpips_layers(x, y, w)
    assert tuple(both.shape) == (3, 6)
    for i in range(3):
        single = lp.lpips_layers(x[i], y[i], w)
        assert torch.equal(both[i], single[0]), (i, both[i], single)
    # the batch quirk of the reference's function: one value, the sum over the batch
    assert float(lp.lpips(x, y, w)) == float(both[:, 0].sum())
    assert len({float(v) for v in both[:, 0]}) == 3


@pytest.mark.parametrize("name", ["noise_31x31", "noise_64x200"])
def test_identity_symmetry_and_reproducibility_are_exact(dev, name):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs[name]
    same = lp.lpips_layers(x, x.clone(), w)
    assert torch.equal(same, torch.zeros_like(same)), same            # exactly 0.0 in all six
    xy, yx = lp.lpips_layers(x, y, w), lp.lpips_layers(y, x, w)
    assert torch.equal(xy, yx) and float(xy[0, 0]) > 0.0
    assert torch.equal(lp.lpips_layers(x, y, w), xy)                  # two runs


# (n_img, Cin, IH, IW, Cout, k, stride, pad, zscore): the five layer shapes at small images -- K = 363 (a K tail) with
# stride 4, Cout = 192 (an M tail of the 128-row tile), N = 2 (one pixel per image), N = 2 * 81 + a ragged last block
CONV_CASES = [(2, 3, 37, 53, 64, 11, 4, 2, True), (3, 64, 9, 13, 192, 5, 1, 2, False), (2, 192, 1, 1, 384, 3, 1, 1, False),
              (2, 384, 9, 9, 256, 3, 1, 1, False), (5, 256, 6, 7, 256, 3, 1, 1, False), (1, 3, 31, 31, 64, 11, 4, 2, False)]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c[:8]))
def test_convolution_kernel_against_torch_in_float64(gpu, case):
    """dgs_conv2d_bias_relu against relu(conv2d) in fp64.  The bound is the kernel's own arithmetic (include/dgs_hip.h):
    a chain of 32 fmaf from 0 errs by at most 32 u sum|w x| over its terms, the compensated sum of the chains by 2 u sum|w x|
    (+ O(u^2)), the bias addition by u (sum|w x| + |b|), the fused z-score by 2 u per input: below 40 u (sum|w x| + |b|) per
    output element, u = 2^-24; relu does not enlarge a difference."""
    import torch
    import torch.nn.functional as F
    from deblurgs_amd import lpips as lp
    n_img, Cin, IH, IW, Cout, k, stride, pad, zscore = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.rand((n_img, Cin, IH, IW), generator=g) * (1.0 if zscore else 2.0) - (0.0 if zscore else 0.5)
    wgt = torch.randn((Cout, Cin, k, k), generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    bias = torch.randn((Cout,), generator=g) * 0.05
    got = lp.conv2d_bias_relu(x.to(gpu), wgt.to(gpu), bias.to(gpu), stride=stride, padding=pad, zscore=zscore).cpu().double()
    xd = x.double()
    if zscore:
        xd = (xd - torch.tensor(lp.MEAN, dtype=torch.float32).double()[None, :, None, None]) / \
            torch.tensor(lp.STD, dtype=torch.float32).double()[None, :, None, None]
    pre = F.conv2d(xd, wgt.double(), bias.double(), stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wgt.double().abs(), bias.double().abs(), stride=stride, padding=pad)
    assert got.shape == pre.shape
    err = (got - F.relu(pre)).abs()
    ratio = float((err / (mag * 2.0 ** -24)).max())
    print(f"conv {case}: max error {float(err.max()):.3e} = {ratio:.2f} u (sum|w x| + |b|)")
    assert torch.isfinite(got).all() and ratio <= 40.0, ratio
    assert float((got > 0).double().mean()) > 0.2       # (not all clipped by the ReLU)


def test_lpips_refuses_weights_on_another_device_and_small_images(dev):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs["noise_31x31"]
    with pytest.raises(RuntimeError, match="weights"):
        lp.lpips(x, y, lc.weights())                    # CPU weights, device images
    with pytest.raises(ValueError, match="31"):
        lp.lpips(x[:, :30], y[:, :30], w)
    # fp64 device inputs take the torch expressions, on the device
    got = lp.lpips_layers(x.double(), y.double(), w)
    assert got.dtype == torch.float64 and got.is_cuda
    assert np.allclose(got[0, 1:].cpu().numpy(), lc.fixture()["noise_31x31_layers64"], rtol=1e-9, atol=0.0)


def test_evaluate_with_lpips_on_a_synthetic_scene(gpu, dev):
    """A few hundred Gaussians at 48 x 64, three cameras: evaluate(..., lpips=w) returns a triple whose first two floats
    are bitwise those of the call without it and whose third is the mean of metrics.lpips over the tone-mapped renders;
    views_per_call = 2 gives the same three floats."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses, metrics
    from deblurgs_amd.cloud import GaussianCloud
    w, _ = dev
    P, W, H, n = 400, 64, 48, 3
    sc = synthetic.make_scene(P, W, H, K=n, seed=4, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    tm = losses.ToneMapping("gamma")
    V = sc["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    with torch.no_grad():
        cams = [model(i) for i in range(n)]
        renders = [tm(gaussian_renderer.render(c, cloud, bg)["render"]) for c in cams]
    torch.manual_seed(0)
    gts = torch.stack([(r.clamp(0.0, 1.0) + 0.05 * torch.randn_like(r)).clamp(0.0, 1.0) for r in renders])
    pair = ev.evaluate(cams, cloud, bg, gts, tm)
    triple = ev.evaluate(cams, cloud, bg, gts, tm, lpips=w)
    assert len(pair) == 2 and len(triple) == 3 and triple[:2] == pair
    want = sum(float(metrics.lpips(r, g, w)) for r, g in zip(renders, gts)) / n
    assert triple[2] == want and 0.0 < want < 1.0
    assert ev.evaluate(cams, cloud, bg, gts, tm, views_per_call=2, lpips=w) == triple
    assert ev.evaluate(cams, cloud, bg, gts, tm, views_per_call=2) == pair

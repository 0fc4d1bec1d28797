"""GPU tests of LPIPS-vgg on the device (csrc/lpips.hip through deblurgs_amd/lpips.py): dgs_lpips_vgg against the
reference's own module (tests/golden/lpips_vgg_golden.npz, the bar of tests/lpips_vgg_cases.py), its bitwise properties,
the halo-tile convolution and the 2 x 2 pool on their own, and evaluate(..., lpips=).  Every case is a few ms of device
work."""
import numpy as np
import pytest

import lpips_vgg_cases as vc
from helpers import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    """The recipe's weights and the six pairs on the device (moved once, never written to)."""
    import torch
    w = vc.weights().to(gpu)
    pairs = {n: (torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)) for n, (x, y) in vc.pairs().items()}
    return w, pairs


@pytest.mark.parametrize("name", vc.NAMES)
def test_kernel_matches_the_reference(dev, name):
    """Per layer and in total against the fixture's fp64 values (what each size pins: tests/lpips_vgg_cases.py)."""
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs[name]
    got = lp.lpips_layers(x, y, w)
    assert tuple(got.shape) == (1, 6) and got.dtype.is_floating_point and got.is_cuda
    vc.check_against_fixture(name, got[0].cpu().numpy(), "dgs_lpips_vgg")
    one = lp.lpips(x, y, w)
    assert tuple(one.shape) == (1, 1, 1, 1) and float(one) == float(got[0, 0])


def _three(pairs):
    import torch
    names = ["noise_37x53", "blend_37x53", "noise_37x53"]
    x = torch.stack([pairs[n][0] for n in names])
    y = torch.stack([pairs[n][1] for n in names])
    y[2] = pairs["blend_37x53"][1]              # a third, different pair of the same size
    return x, y


def test_three_pairs_in_one_call_equal_three_single_calls_bitwise(dev):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = _three(pairs)
    both = lp.lpips_layers(x, y, w)
    assert tuple(both.shape) == (3, 6)
    for i in range(3):
        single = lp.lpips_layers(x[i], y[i], w)
        assert torch.equal(both[i], single[0]), (i, both[i], single)
    assert float(lp.lpips(x, y, w)) == float(both[:, 0].sum())
    assert len({float(v) for v in both[:, 0]}) == 3


def test_a_batch_cut_by_max_tmp_bytes_equals_the_uncut_call_bitwise(dev):
    import torch
    from deblurgs_amd import _lib, lpips as lp
    w, pairs = dev
    x, y = _three(pairs)
    q = _lib.lib().dgs_lpips_vgg_tmp_bytes
    whole = lp.lpips_layers(x, y, w)
    assert q(53, 37, 3) > q(53, 37, 2) > q(53, 37, 1)
    for cap in (q(53, 37, 2), q(53, 37, 1), 1):          # calls of 2 + 1 pairs; one pair each; one pair each (never below)
        assert torch.equal(lp.lpips_layers(x, y, w, max_tmp_bytes=cap), whole), cap


@pytest.mark.parametrize("name", ["noise_16x16", "noise_64x200"])
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


# (n_img, Cin, H, W, Cout, zscore): Cin = 3 (one ragged chunk) with and without the z-score; Cin and Cout that are no
# multiple of the chunk or of either channel tile, a 2-column second tile; 37 channels, 130 = a 2-channel second tile;
# two column tiles and ten row tiles, the last ragged; a 1 x 1 image (eight of nine weights on padding); a 1-column tile
CONV3_CASES = [(2, 3, 16, 16, 64, True), (2, 3, 16, 16, 64, False), (1, 5, 7, 35, 33, False), (3, 37, 9, 13, 130, False),
               (2, 64, 37, 53, 128, False), (2, 512, 1, 1, 512, False), (1, 128, 4, 33, 256, False)]


def chain(case):
    """L of dgs_conv3x3_bias_relu (include/dgs_hip.h): 9 x the input channels of a chunk, 4 where Cout <= 64, else 8."""
    return 36 if case[4] <= 64 else 72


def _conv3_inputs(case):
    import torch
    n_img, Cin, H, W, Cout, zscore = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = torch.rand((n_img, Cin, H, W), generator=g) * (1.0 if zscore else 2.0) - (0.0 if zscore else 0.5)
    wgt = torch.randn((Cout, Cin, 3, 3), generator=g) * (2.0 / (Cin * 9)) ** 0.5
    bias = torch.randn((Cout,), generator=g) * 0.05
    return x, wgt, bias


@pytest.fixture(scope="module")
def conv3_results(gpu):
    """Every case's device result, computed once and shared by the two tests below."""
    from deblurgs_amd import lpips as lp
    out = {}
    for case in CONV3_CASES:
        x, wgt, bias = _conv3_inputs(case)
        out[case] = lp.conv3x3_bias_relu(x.to(gpu), wgt.to(gpu), bias.to(gpu), zscore=case[5])
    return out


@pytest.mark.parametrize("case", CONV3_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_conv3x3_kernel_against_torch_in_float64(conv3_results, case):
    """dgs_conv3x3_bias_relu against relu(conv2d) in fp64.  The bound is the kernel's own arithmetic (include/dgs_hip.h),
    derived as for dgs_conv2d_bias_relu: a chain of L (36 or 72) fmaf from 0 errs by at most L u sum|w x| over its terms, the
    compensated sum of the chains by 2 u sum|w x| (+ O(u^2)), the bias addition by u (sum|w x| + |b|), the fused z-score
    by 2 u per input: below (L + 8) u (sum|w x| + |b|) per output element, u = 2^-24; relu does not enlarge a
    difference."""
    import torch
    import torch.nn.functional as F
    from deblurgs_amd import lpips as lp
    x, wgt, bias = _conv3_inputs(case)
    got = conv3_results[case].cpu().double()
    xd = x.double()
    if case[5]:
        xd = (xd - torch.tensor(lp.MEAN, dtype=torch.float32).double()[None, :, None, None]) / \
            torch.tensor(lp.STD, dtype=torch.float32).double()[None, :, None, None]
    pre = F.conv2d(xd, wgt.double(), bias.double(), stride=1, padding=1)
    mag = F.conv2d(xd.abs(), wgt.double().abs(), bias.double().abs(), stride=1, padding=1)
    assert got.shape == pre.shape
    err = (got - F.relu(pre)).abs()
    ratio = float((err / (mag * 2.0 ** -24)).max())
    print(f"conv3x3 {case}: max error {float(err.max()):.3e} = {ratio:.2f} u (sum|w x| + |b|), bound {chain(case) + 8} u")
    assert torch.isfinite(got).all() and ratio <= chain(case) + 8.0, ratio
    assert float((got > 0).double().mean()) > 0.2       # (not all clipped by the ReLU)


@pytest.mark.parametrize("case", CONV3_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_conv3x3_result_does_not_depend_on_the_place_in_the_call(gpu, conv3_results, case):
    """The case's first image as image 1 of a 3-image call: bitwise the same map."""
    import torch
    from deblurgs_amd import lpips as lp
    x, wgt, bias = _conv3_inputs(case)
    g = torch.Generator().manual_seed(99)
    three = torch.stack([torch.rand(x.shape[1:], generator=g), x[0], torch.rand(x.shape[1:], generator=g)])
    got = lp.conv3x3_bias_relu(three.to(gpu), wgt.to(gpu), bias.to(gpu), zscore=case[5])
    assert torch.equal(got[1], conv3_results[case][0])
    assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize("shape", [(6, 2, 2), (3, 5, 7), (2, 2, 17, 23), (2, 64, 200), (1, 3, 8, 12)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_maxpool2x2_equals_torch_bitwise(gpu, shape):
    """2 x 2 planes (1 x 1 out), odd sizes (floor), the 16-byte path (W a multiple of 4) and the scalar one; then with
    NaNs at every place of a window."""
    import torch
    import torch.nn.functional as F
    from deblurgs_amd import lpips as lp
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g)).to(gpu)
    want = F.max_pool2d(x.reshape((-1, 1) + shape[-2:]), 2, 2).reshape(shape[:-2] + (shape[-2] // 2, shape[-1] // 2))
    got = lp.maxpool2x2(x)
    assert got.shape == want.shape and torch.equal(got, want)
    xn = x.clone()
    flat = xn.view(-1)
    flat[::5] = float("nan")
    want = F.max_pool2d(xn.reshape((-1, 1) + shape[-2:]), 2, 2).reshape(got.shape)
    got = lp.maxpool2x2(xn)
    assert torch.isnan(want).any() and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))


def test_lpips_vgg_refuses_weights_on_another_device_and_small_images(dev):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs["noise_16x16"]
    with pytest.raises(RuntimeError, match="weights"):
        lp.lpips(x, y, vc.weights())                    # CPU weights, device images
    with pytest.raises(ValueError, match="16"):
        lp.lpips(x[:, :15], y[:, :15], w)
    # fp64 device inputs take the torch expressions, on the device
    got = lp.lpips_layers(x.double(), y.double(), w)
    assert got.dtype == torch.float64 and got.is_cuda
    assert np.allclose(got[0, 1:].cpu().numpy(), vc.fixture()["noise_16x16_layers64"], rtol=1e-9, atol=0.0)


def test_evaluate_with_vgg_weights_on_a_synthetic_scene(gpu, dev):
    """The 400-Gaussian 48 x 64 scene of the alex test: evaluate(..., lpips=vgg weights) returns a triple whose first two
    floats are bitwise those of the call without it; views_per_call = 2 gives the same three floats."""
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

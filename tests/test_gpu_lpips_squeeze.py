"""GPU tests of LPIPS-squeeze on the device (csrc/lpips.hip through deblurgs_amd/lpips.py): dgs_lpips_squeeze against the
reference's own module (tests/golden/lpips_squeeze_golden.npz, the bar of tests/lpips_squeeze_cases.py), its bitwise
properties, the one-launch Fire kernel and the ceil-mode pool on their own, and evaluate(..., lpips=).  Every case is a
few ms of device work."""
import numpy as np
import pytest

import lpips_squeeze_cases as sc
from helpers import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    """The recipe's weights and the seven pairs on the device (moved once, never written to)."""
    import torch
    w = sc.weights().to(gpu)
    pairs = {n: (torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)) for n, (x, y) in sc.pairs().items()}
    return w, pairs


@pytest.mark.parametrize("name", sc.NAMES)
def test_kernel_matches_the_reference(dev, name):
    """Per layer and in total against the fixture's fp64 values (what each size pins: tests/lpips_squeeze_cases.py)."""
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs[name]
    got = lp.lpips_layers(x, y, w)
    assert tuple(got.shape) == (1, 8) and got.dtype.is_floating_point and got.is_cuda
    sc.check_against_fixture(name, got[0].cpu().numpy(), "dgs_lpips_squeeze")
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
    assert tuple(both.shape) == (3, 8)
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
    q = _lib.lib().dgs_lpips_squeeze_tmp_bytes
    whole = lp.lpips_layers(x, y, w)
    assert q(53, 37, 3) > q(53, 37, 2) > q(53, 37, 1)
    for cap in (q(53, 37, 2), q(53, 37, 1), 1):          # calls of 2 + 1 pairs; one pair each; one pair each (never below)
        assert torch.equal(lp.lpips_layers(x, y, w, max_tmp_bytes=cap), whole), cap


@pytest.mark.parametrize("name", ["noise_17x17", "noise_64x200"])
def test_identity_symmetry_and_reproducibility_are_exact(dev, name):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs[name]
    same = lp.lpips_layers(x, x.clone(), w)
    assert torch.equal(same, torch.zeros_like(same)), same            # exactly 0.0 in all eight
    xy, yx = lp.lpips_layers(x, y, w), lp.lpips_layers(y, x, w)
    assert torch.equal(xy, yx) and float(xy[0, 0]) > 0.0
    assert torch.equal(lp.lpips_layers(x, y, w), xy)                  # two runs


# (n_img, Cin, H, W, S, E1, E3): Fire 1's shape on one tile; everything ragged (Cin below a chunk, odd S, E1 and E3 no
# multiple of 32, a 3-column second tile); Fire 3's shape with a 1-column second tile and three row tiles; a 1 x 1 map whose
# whole halo is padding, at the deepest squeeze (the 32-channel chunks, two MFMA row tiles, four expand slabs); a 2 x 3
# map at S = 48; one row, two column tiles, S = 64 from a single ragged chunk, E1 far below E3 (slabs with no 1 x 1 part)
FIRE_CASES = [(2, 64, 8, 8, 16, 64, 64), (1, 7, 5, 35, 5, 33, 37), (2, 128, 9, 33, 32, 128, 128), (1, 512, 1, 1, 64, 256, 256),
              (1, 384, 2, 3, 48, 192, 192), (3, 16, 1, 40, 64, 8, 130)]
_ids = lambda c: "x".join(str(int(v)) for v in c)


def chains(case):
    """(L1, L2a, L2b) of dgs_fire_bias_relu (include/dgs_hip.h): the squeeze's chain is a chunk of 16 input channels where
    S <= 32, else of 32; the 1 x 1 expand is one chain of S terms (S + 1 for odd S); the 3 x 3 expand's chain is 9 weights x
    8 squeeze channels = 72."""
    S = case[4]
    return (16 if S <= 32 else 32), S + (S & 1), 72


def _fire_inputs(case):
    """x and the six weights: He-scaled weights, biases 0.05 N(0,1), the squeeze bias strictly positive."""
    import torch
    n_img, Cin, H, W, S, E1, E3 = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.rand((n_img, Cin, H, W), generator=g) * 2.0 - 0.5
    conv = lambda co, ci, k: torch.randn((co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
    sw, sb = conv(S, Cin, 1), 0.1 + 0.05 * torch.randn((S,), generator=g).abs()
    w1, b1 = conv(E1, S, 1), torch.randn((E1,), generator=g) * 0.05
    w3, b3 = conv(E3, S, 3), torch.randn((E3,), generator=g) * 0.05
    return x, (sw, sb, w1, b1, w3, b3)


@pytest.fixture(scope="module")
def fire_results(gpu):
    """Every case's device result (out, squeeze_out), computed once and shared by the tests below."""
    from deblurgs_amd import lpips as lp
    out = {}
    for case in FIRE_CASES:
        x, ws = _fire_inputs(case)
        out[case] = lp.fire_bias_relu(x.to(gpu), [w.to(gpu) for w in ws], return_squeeze=True)
    return out


def _ratio(got, pre, mag):
    import torch
    import torch.nn.functional as F
    assert got.shape == pre.shape
    err = (got - F.relu(pre)).abs()
    return float(err.max()), float((err / (mag * 2.0 ** -24)).max())


@pytest.mark.parametrize("case", FIRE_CASES, ids=_ids)
def test_fire_squeeze_map_against_torch_in_float64(fire_results, case):
    """squeeze_out against relu(conv2d) in fp64.  The bound is the kernel's own arithmetic (include/dgs_hip.h), derived as
    for dgs_conv3x3_bias_relu: a chain of L1 fmaf from 0 errs by at most L1 u sum|w x| over its terms, the compensated sum of
    the chains by 2 u sum|w x| (+ O(u^2)), the bias addition by u (sum|w x| + |b|): below (L1 + 8) u (sum|w x| + |b|) per
    element, u = 2^-24; relu does not enlarge a difference."""
    import torch
    import torch.nn.functional as F
    x, (sw, sb, *_) = _fire_inputs(case)
    got = fire_results[case][1].cpu().double()
    pre = F.conv2d(x.double(), sw.double(), sb.double())
    mag = F.conv2d(x.double().abs(), sw.double().abs(), sb.double().abs())
    err, ratio = _ratio(got, pre, mag)
    L1 = chains(case)[0]
    print(f"fire squeeze {case}: max error {err:.3e} = {ratio:.2f} u (sum|w x| + |b|), bound {L1 + 8} u")
    assert torch.isfinite(got).all() and ratio <= L1 + 8.0, ratio
    assert float((got > 0).double().mean()) > 0.2


@pytest.mark.parametrize("case", FIRE_CASES, ids=_ids)
def test_fire_expands_against_torch_in_float64_of_the_device_squeeze_map(fire_results, case):
    """`out` against cat(relu(conv1x1), relu(conv3x3 pad 1)) in fp64 OF THE DEVICE'S OWN squeeze_out, so the stages' errors
    do not compound and a halo that held relu(bias) > 0 instead of 0 outside the image shows at full size on every edge
    pixel.  Bounds as above with the stage-2 chains: (L2a + 8) u for the 1 x 1 channels, (L2b + 8) u for the 3 x 3 ones."""
    import torch
    import torch.nn.functional as F
    E1 = case[5]
    _, (_, _, w1, b1, w3, b3) = _fire_inputs(case)
    out, sq = (t.cpu().double() for t in fire_results[case])
    assert tuple(out.shape) == (case[0], case[5] + case[6], case[2], case[3])
    _, L2a, L2b = chains(case)
    for what, got, w, b, pad, L in (("1x1", out[:, :E1], w1, b1, 0, L2a), ("3x3", out[:, E1:], w3, b3, 1, L2b)):
        pre = F.conv2d(sq, w.double(), b.double(), padding=pad)
        mag = F.conv2d(sq.abs(), w.double().abs(), b.double().abs(), padding=pad)
        err, ratio = _ratio(got, pre, mag)
        print(f"fire expand {what} {case}: max error {err:.3e} = {ratio:.2f} u (sum|w s| + |b|), bound {L + 8} u")
        assert torch.isfinite(got).all() and ratio <= L + 8.0, (what, ratio)
    assert float((out > 0).double().mean()) > 0.2       # (not all clipped by the ReLU)


@pytest.mark.parametrize("case", FIRE_CASES, ids=_ids)
def test_fire_output_is_the_same_without_squeeze_out_and_anywhere_in_the_call(gpu, fire_results, case):
    """squeeze_out = NULL: bitwise the same `out`.  The case's first image as image 1 of a 3-image call: bitwise the same
    maps."""
    import torch
    from deblurgs_amd import lpips as lp
    x, ws = _fire_inputs(case)
    ws = [w.to(gpu) for w in ws]
    want_out, want_sq = fire_results[case]
    assert torch.equal(lp.fire_bias_relu(x.to(gpu), ws), want_out)
    g = torch.Generator().manual_seed(99)
    three = torch.stack([torch.rand(x.shape[1:], generator=g), x[0], torch.rand(x.shape[1:], generator=g)])
    out, sq = lp.fire_bias_relu(three.to(gpu), ws, return_squeeze=True)
    assert torch.equal(out[1], want_out[0]) and torch.equal(sq[1], want_sq[0])
    assert not torch.equal(out[0], out[1])


def test_fire_refuses_a_squeeze_depth_above_64(gpu):
    import torch
    from deblurgs_amd import lpips as lp
    z = lambda *s: torch.zeros(s, device=gpu)
    with pytest.raises(RuntimeError, match="1..64"):
        lp.fire_bias_relu(z(1, 8, 4, 4), (z(65, 8, 1, 1), z(65), z(8, 65, 1, 1), z(8), z(8, 65, 3, 3), z(8)))
    with pytest.raises(ValueError, match="expand3x3"):
        lp.fire_bias_relu(z(1, 8, 4, 4), (z(16, 8, 1, 1), z(16), z(8, 16, 1, 1), z(8), z(8, 16, 1, 1), z(8)))


POOL_SHAPES = [(3, 2, 2), (2, 3, 3), (3, 4, 4), (2, 5, 4), (2, 2, 8, 9), (3, 17, 23), (2, 64, 200)]


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_maxpool3x3s2_ceil_equals_torch_bitwise(gpu, shape):
    """Planes of 2 x 2 (one window of two by two), 3 x 3, even sizes (a last window of two), odd ones; then with a NaN at
    every place of a full window (rows and columns 0..2) and of the ragged last windows (the last two rows and columns)."""
    import torch
    import torch.nn.functional as F
    from deblurgs_amd import lpips as lp
    H, W = shape[-2:]
    ref = lambda t: F.max_pool2d(t.reshape((-1, 1, H, W)), 3, 2, ceil_mode=True).reshape(shape[:-2] + (H // 2, W // 2))
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(gpu)
    got = lp.maxpool3x3s2_ceil(x)
    assert tuple(got.shape) == shape[:-2] + (H // 2, W // 2) and torch.equal(got, ref(x))
    places = {(r, c) for r in range(min(3, H)) for c in range(min(3, W))} | {(r, c) for r in (H - 2, H - 1) for c in (W - 2, W - 1)}
    xs = torch.stack([x] * len(places))
    for i, (r, c) in enumerate(sorted(places)):
        xs[i, ..., r, c] = float("nan")
    want = torch.stack([ref(v) for v in xs])
    got = torch.stack([lp.maxpool3x3s2_ceil(v) for v in xs])
    assert torch.isnan(want).flatten(1).any(dim=1).all()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))


def test_lpips_squeeze_refuses_weights_on_another_device_and_small_images(dev):
    import torch
    from deblurgs_amd import lpips as lp
    w, pairs = dev
    x, y = pairs["noise_17x17"]
    with pytest.raises(RuntimeError, match="weights"):
        lp.lpips(x, y, sc.weights())                    # CPU weights, device images
    with pytest.raises(ValueError, match="17"):
        lp.lpips(x[:, :16], y[:, :16], w)
    with pytest.raises(ValueError, match="17"):
        lp.lpips(x[:, :, :16], y[:, :, :16], w)
    sc.check_against_fixture("noise_17x17", lp.lpips_layers(x, y, w)[0].cpu().numpy(), "dgs_lpips_squeeze 17 x 17")
    # fp64 device inputs take the torch expressions, on the device
    got = lp.lpips_layers(x.double(), y.double(), w)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (1, 8)
    assert np.allclose(got[0, 1:].cpu().numpy(), sc.fixture()["noise_17x17_layers64"], rtol=1e-9, atol=0.0)


def test_evaluate_with_squeeze_weights_on_a_synthetic_scene(gpu, dev):
    """The 400-Gaussian 48 x 64 scene of the vgg test: evaluate(..., lpips=squeeze weights) returns a triple whose first
    two floats are bitwise those of the call without it and whose third is the mean of the per-view lpips_layers[:, 0]."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses, lpips as lp
    from deblurgs_amd.cloud import GaussianCloud
    w, _ = dev
    P, W, H, n = 400, 64, 48, 3
    scn = synthetic.make_scene(P, W, H, K=n, seed=4, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(scn, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    tm = losses.ToneMapping("gamma")
    V = scn["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], scn["FoVx"], scn["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    with torch.no_grad():
        cams = [model(i) for i in range(n)]
        renders = [tm(gaussian_renderer.render(c, cloud, bg)["render"]) for c in cams]
    torch.manual_seed(0)
    gts = torch.stack([(r.clamp(0.0, 1.0) + 0.05 * torch.randn_like(r)).clamp(0.0, 1.0) for r in renders])
    pair = ev.evaluate(cams, cloud, bg, gts, tm)
    triple = ev.evaluate(cams, cloud, bg, gts, tm, lpips=w)
    assert len(pair) == 2 and len(triple) == 3 and triple[:2] == pair
    want = sum(float(lp.lpips_layers(r, g, w)[0, 0]) for r, g in zip(renders, gts)) / n
    assert triple[2] == want and 0.0 < want < 1.0

"""CPU tests of LPIPS-alex (deblurgs_amd/lpips.py, dgs_lpips_alex): the torch-expression path against the reference's own
module (tests/golden/lpips_golden.npz, made by tests/golden/make_golden_lpips.py), the weight loader, the C ABI's argument
checks (refused before any HIP call, so they need no GPU), evaluate(..., lpips=) and the lpipsPyTorch shim.

The bar of a pair (tests/lpips_cases.bar): 8 x the largest of the five fp32-vs-fp64 differences the reference's own module
showed on that pair -- the implementations under test commit fp32 rounding of the same class in another summation order.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import lpips_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_covers_the_five_pairs():
    f = lc.fixture()
    assert list(f["names"]) == list(lc.NAMES) and len(lc.NAMES) == 5
    for name, (x, y) in lc.pairs().items():
        assert x.dtype == np.float32 and x.shape == y.shape and x.shape[0] == 3
        assert f[name + "_layers64"].shape == (5,) and f[name + "_rel32"].shape == (5,)
        assert 0.0 < lc.bar(name) < 1e-5            # the bar never reaches 1e-5
        # the reference's own fp32 total sits inside its bar too
        assert abs(float(f[name + "_total32"]) - f[name + "_layers64"].sum()) <= lc.bar(name) * f[name + "_layers64"].sum()
    assert [tuple(p[0].shape[1:]) for p in lc.pairs().values()] == [(31, 31), (37, 53), (64, 200), (135, 240), (37, 53)]


@pytest.mark.parametrize("name", lc.NAMES)
def test_torch_path_matches_the_reference(name):
    from deblurgs_amd import lpips as lp
    x, y = (torch.from_numpy(a) for a in lc.pairs()[name])
    got = lp.lpips_layers(x, y, lc.weights())
    assert tuple(got.shape) == (1, 6) and got.dtype == torch.float32
    lc.check_against_fixture(name, got[0].numpy(), "torch fp32")
    # fp64 inputs run the same expressions in fp64: the fixture's values to fp64 rounding
    got64 = lp.lpips_layers(x.double(), y.double(), lc.weights())[0].numpy()
    assert got64.dtype == np.float64
    assert np.allclose(got64[1:], lc.fixture()[name + "_layers64"], rtol=1e-12, atol=0.0)


def test_batch_quirk_one_value_summed_over_the_batch():
    from deblurgs_amd import lpips as lp, metrics
    assert metrics.lpips is lp.lpips
    p = lc.pairs()
    a, b = p["noise_37x53"], p["blend_37x53"]
    x, y = torch.from_numpy(np.stack([a[0], b[0]])), torch.from_numpy(np.stack([a[1], b[1]]))
    both = lp.lpips(x, y, lc.weights())
    assert tuple(both.shape) == (1, 1, 1, 1)
    one = lp.lpips(x[0], y[0], lc.weights())            # [3,H,W] in, [1,1,1,1] out
    two = lp.lpips(x[1:], y[1:], lc.weights())
    assert tuple(one.shape) == tuple(two.shape) == (1, 1, 1, 1)
    assert float(both) == pytest.approx(float(one) + float(two), rel=1e-6)
    want = float(lc.fixture()["batch2_total64"])         # the reference's own N = 2 call, in fp64
    assert abs(float(lp.lpips(x.double(), y.double(), lc.weights())) - want) <= 1e-12 * want
    assert abs(float(both) - want) <= max(lc.bar("noise_37x53"), lc.bar("blend_37x53")) * want


def test_images_below_31_are_refused_like_the_reference():
    from deblurgs_amd import lpips as lp
    w = lc.weights()
    for shape in ((3, 30, 31), (3, 31, 30), (2, 3, 30, 40)):
        with pytest.raises(ValueError, match="31"):
            lp.lpips(torch.zeros(shape), torch.zeros(shape), w)
    with pytest.raises(ValueError, match="shape"):
        lp.lpips(torch.zeros(3, 40, 40), torch.zeros(3, 40, 41), w)
    with pytest.raises(ValueError):
        lp.lpips(torch.zeros(1, 40, 40), torch.zeros(1, 40, 40), w)
    assert tuple(lp.lpips(torch.zeros(3, 31, 31), torch.zeros(3, 31, 31), w).shape) == (1, 1, 1, 1)


def test_both_key_spellings_load_identical_weights():
    from deblurgs_amd.lpips import LPIPSWeights
    feats, lin = lc.state_dicts()
    w0 = LPIPSWeights.from_state_dicts(feats, lin)
    bare = {k[len("features."):]: v for k, v in feats.items()}                          # a `.features` state dict
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}     # utils.py:22-28
    assert sorted(renamed) == [f"{i}.1.weight" for i in range(5)]
    w1 = LPIPSWeights.from_state_dicts(bare, renamed)
    assert len(w0.tensors()) == 15
    for a, b in zip(w0.tensors(), w1.tensors()):
        assert a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, b)
    assert [tuple(t.shape) for t in w0.conv_w] == [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3),
                                                   (256, 256, 3, 3)]
    assert [tuple(t.shape) for t in w0.lin] == [(1, c, 1, 1) for c in (64, 192, 384, 256, 256)]
    assert w0.to("cpu").device == torch.device("cpu")


def test_load_reads_the_two_local_files(tmp_path):
    from deblurgs_amd.lpips import LPIPSWeights
    feats, lin = lc.state_dicts()
    torch.save(feats, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    w = LPIPSWeights.load(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"))
    for a, b in zip(w.tensors(), lc.weights().tensors()):
        assert torch.equal(a, b)


def test_missing_key_and_wrong_shape_are_refused_by_name():
    from deblurgs_amd.lpips import LPIPSWeights
    feats, lin = lc.state_dicts()
    broken = dict(feats)
    del broken["features.6.bias"]
    with pytest.raises(KeyError, match=r"features\.6\.bias"):
        LPIPSWeights.from_state_dicts(broken, lin)
    broken = dict(lin)
    del broken["lin3.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        LPIPSWeights.from_state_dicts(feats, broken)
    broken = dict(feats)
    broken["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight.*\(192, 64, 3, 3\)"):
        LPIPSWeights.from_state_dicts(broken, lin)
    broken = dict(lin)
    broken["lin0.model.1.weight"] = torch.zeros(1, 65, 1, 1)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        LPIPSWeights.from_state_dicts(feats, broken)


def _weights_struct(addr):
    from deblurgs_amd import _lib
    w = _lib.DgsLpipsAlexWeights()
    for i in range(5):
        w.conv_w[i] = w.conv_b[i] = w.lin[i] = addr
    return w


def test_lpips_alex_argument_checks_need_no_gpu():
    """NULL pointers, n_pairs < 1 and images below 31 x 31 come back as DGS_E_ARG with a text, before any HIP call; a
    31 x 31 call passes every check (what it returns then is the HIP runtime's business: 0 on a GPU, DGS_E_HIP without)."""
    from deblurgs_amd import _lib
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(256)
    a = ctypes.cast(dummy, ctypes.c_void_p)
    w = _weights_struct(a.value)
    ok = lambda *args: L.dgs_lpips_alex(*args)
    assert ok(None, a, 1, 31, 31, ctypes.byref(w), a, a, None) == -1 and b"null" in L.dgs_last_error()
    assert ok(a, None, 1, 31, 31, ctypes.byref(w), a, a, None) == -1
    assert ok(a, a, 1, 31, 31, None, a, a, None) == -1
    assert ok(a, a, 1, 31, 31, ctypes.byref(w), None, a, None) == -1
    assert ok(a, a, 1, 31, 31, ctypes.byref(w), a, None, None) == -1
    hole = _weights_struct(a.value)
    hole.lin[4] = None
    assert ok(a, a, 1, 31, 31, ctypes.byref(hole), a, a, None) == -1 and b"weight" in L.dgs_last_error()
    assert ok(a, a, 0, 31, 31, ctypes.byref(w), a, a, None) == -1 and b"n_pairs" in L.dgs_last_error()
    assert ok(a, a, -3, 31, 31, ctypes.byref(w), a, a, None) == -1
    assert ok(a, a, 1, 30, 31, ctypes.byref(w), a, a, None) == -1 and b"31 x 31" in L.dgs_last_error()     # W = 30
    assert ok(a, a, 1, 31, 30, ctypes.byref(w), a, a, None) == -1 and b"31 x 31" in L.dgs_last_error()     # H = 30
    if not torch.cuda.is_available():     # (with a device the dummy pointers would be dereferenced)
        assert ok(a, a, 1, 31, 31, ctypes.byref(w), a, a, None) in (0, -3)
        assert L.dgs_conv2d_bias_relu(a, 1, 3, 31, 31, a, a, 64, 11, 11, 4, 2, 1, a, None) in (0, -3)
    c = lambda *args: L.dgs_conv2d_bias_relu(*args)
    assert c(None, 1, 3, 31, 31, a, a, 64, 11, 11, 4, 2, 1, a, None) == -1
    assert c(a, 0, 3, 31, 31, a, a, 64, 11, 11, 4, 2, 1, a, None) == -1
    assert c(a, 1, 3, 31, 31, a, a, 64, 16, 11, 4, 2, 0, a, None) == -1                      # kernel sizes are 1..15
    assert c(a, 1, 3, 31, 31, a, a, 64, 11, 11, 0, 2, 0, a, None) == -1                      # stride 0
    assert c(a, 1, 4, 31, 31, a, a, 64, 11, 11, 4, 2, 1, a, None) == -1 and b"zscore" in L.dgs_last_error()
    assert c(a, 1, 3, 5, 31, a, a, 64, 11, 11, 4, 2, 0, a, None) == -1 and b"smaller" in L.dgs_last_error()


def test_tmp_bytes_is_positive_and_monotone():
    from deblurgs_amd import _lib
    q = _lib.lib().dgs_lpips_alex_tmp_bytes
    assert q(30, 31, 1) == 0 and q(31, 30, 1) == 0 and q(31, 31, 0) == 0
    base = q(31, 31, 1)
    # two feature buffers: tap 1 [2,64,7,7] floats and the first pooled map [2,64,3,3] at the least
    assert base >= 2 * 64 * 49 * 4 + 2 * 64 * 9 * 4
    prev = base
    for W in range(32, 400, 7):
        cur = q(W, 31, 1)
        assert cur >= prev > 0
        prev = cur
    prev = base
    for H in range(32, 400, 7):
        cur = q(31, H, 1)
        assert cur >= prev > 0
        prev = cur
    prev = base
    for n in range(2, 40):
        cur = q(31, 31, n)
        assert cur > prev
        prev = cur
    # 1080p: tap 1 is [2,64,269,479] floats
    assert q(1920, 1080, 1) >= 2 * 64 * 269 * 479 * 4
    assert q(1920, 1080, 2) > q(1920, 1080, 1) > q(1280, 720, 1)


def test_symbols_struct_header_and_abi():
    from deblurgs_amd import _lib, build
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in ("dgs_lpips_alex", "dgs_lpips_alex_tmp_bytes", "dgs_conv2d_bias_relu"):
        assert hasattr(L, s) and s in _lib.EXPORTS and re.search(r"\b%s\s*\(" % s, code), s
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", text).group(1)) == 15 == _lib.ABI_VERSION == L.dgs_abi_version()
    # fifteen device pointers, nothing else
    assert ctypes.sizeof(_lib.DgsLpipsAlexWeights) == 15 * ctypes.sizeof(ctypes.c_void_p)
    body = re.search(r"typedef struct DgsLpipsAlexWeights \{(.*?)\} DgsLpipsAlexWeights;", code, flags=re.S).group(1)
    assert re.findall(r"const float\* (\w+)\[5\];", body) == ["conv_w", "conv_b", "lin"]
    assert [n for n, _ in _lib.DgsLpipsAlexWeights._fields_] == ["conv_w", "conv_b", "lin"]
    assert "lpips.hip" in build.SOURCES and any(f.startswith("-ffp-contract=") for f in build.SOURCES["lpips.hip"])
    src = open(os.path.join(ROOT, "deblurgs_amd", "csrc", "lpips.hip")).read()
    for banned in ("rocprim", "hipcub", "miopen", "getenv", "atomicAdd"):
        assert banned not in src.lower().replace("no float atomics", ""), banned


def test_header_with_the_lpips_struct_is_plain_c(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "h.c"
    src.write_text('#include "%s"\nint main(void) { DgsLpipsAlexWeights w; w.lin[4] = 0; (void)w;\n'
                   '  return (int)sizeof(w) == 15 * (int)sizeof(void*) ? 0 : 1; }\n' % os.path.join(ROOT, "include", "dgs_hip.h"))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", str(src), "-o", str(tmp_path / "h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "h")]).returncode == 0


def test_evaluate_with_lpips_returns_a_triple_and_leaves_the_pair_alone(monkeypatch):
    """evaluate() on CPU tensors (the render stubbed out: the rasteriser has no CPU path): with lpips= a triple whose first
    two entries are the pair returned without it, the third the mean of metrics.lpips over the tone-mapped images."""
    from deblurgs_amd import evaluation as ev, losses, metrics
    p = lc.pairs()
    renders = [torch.from_numpy(p["noise_37x53"][0]), torch.from_numpy(p["blend_37x53"][0])]
    gts = [torch.from_numpy(p["noise_37x53"][1]), torch.from_numpy(p["blend_37x53"][1])]
    monkeypatch.setattr(ev.gaussian_renderer, "render", lambda cam, cloud, bg: {"render": renders[cam]})
    tm = losses.ToneMapping("gamma")
    pair = ev.evaluate([0, 1], None, None, gts, tm)
    triple = ev.evaluate([0, 1], None, None, gts, tm, lpips=lc.weights())
    assert len(pair) == 2 and len(triple) == 3 and all(isinstance(v, float) for v in triple)
    assert triple[:2] == pair
    want = sum(float(metrics.lpips(tm(r), g, lc.weights())) for r, g in zip(renders, gts)) / 2
    assert triple[2] == pytest.approx(want, rel=1e-6) and 0.0 < triple[2] < 1.0


@pytest.fixture
def shim(monkeypatch, tmp_path):
    import importlib
    from deblurgs_amd import lpips as lp
    monkeypatch.syspath_prepend(os.path.join(ROOT, "deblurgs_amd", "dropin"))
    old_dir = torch.hub.get_dir()
    torch.hub.set_dir(str(tmp_path))                 # an empty hub directory: no checkpoint to be found
    lp.set_default_weights(None)
    sys.modules.pop("lpipsPyTorch", None)
    yield importlib.import_module("lpipsPyTorch")
    lp.set_default_weights(None)
    torch.hub.set_dir(old_dir)
    sys.modules.pop("lpipsPyTorch", None)


def test_shim_has_the_reference_signature_and_needs_weights(shim, tmp_path):
    import inspect
    from deblurgs_amd import lpips as lp
    sig = inspect.signature(shim.lpips)
    assert list(sig.parameters) == ["x", "y", "net_type", "version"]
    assert sig.parameters["net_type"].default == "alex" and sig.parameters["version"].default == "0.1"
    x, y = (torch.from_numpy(a) for a in lc.pairs()["noise_31x31"])
    with pytest.raises(FileNotFoundError, match=r"alexnet-owt-\*\.pth.*alex\.pth"):
        shim.lpips(x, y, net_type="alex")
    with pytest.raises(NotImplementedError, match="alex"):
        shim.lpips(x, y, net_type="vgg")
    lp.set_default_weights(lc.weights())
    got = shim.lpips(x, y, net_type="alex")
    assert tuple(got.shape) == (1, 1, 1, 1) and torch.equal(got, lp.lpips(x, y, lc.weights()))
    # the files of a hub directory are found by name, and only there
    lp.set_default_weights(None)
    os.makedirs(tmp_path / "checkpoints")
    feats, lin = lc.state_dicts()
    torch.save(feats, tmp_path / "checkpoints" / "alexnet-owt-7be5be79.pth")
    with pytest.raises(FileNotFoundError):
        shim.lpips(x, y)                              # the lin file is still missing
    torch.save(lin, tmp_path / "checkpoints" / "alex.pth")
    assert torch.equal(shim.lpips(x, y), got)


def test_shim_never_calls_a_hub_loader():
    for path in (os.path.join(ROOT, "deblurgs_amd", "dropin", "lpipsPyTorch", "__init__.py"),
                 os.path.join(ROOT, "deblurgs_amd", "lpips.py")):
        code = open(path).read()
        for banned in ("load_state_dict_from_url", "hub.load(", "download", "urllib", "requests"):
            assert banned not in code, (path, banned)

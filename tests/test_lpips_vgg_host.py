"""CPU tests of LPIPS-vgg (deblurgs_amd/lpips.py, dgs_lpips_vgg): the torch-expression path against the reference's own
module (tests/golden/lpips_vgg_golden.npz, made by tests/golden/make_golden_lpips_vgg.py), the weight loader, the C ABI's
argument checks (refused before any HIP call, so they need no GPU), evaluate(..., lpips=), the lpipsPyTorch shim and
metrics_dirs.evaluate_directories.

The bar of a pair (tests/lpips_vgg_cases.bar) is lpips_cases' rule: 8 x the largest of the five fp32-vs-fp64 differences
the reference's own module showed on that pair.
"""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import lpips_vgg_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_covers_the_six_pairs():
    f = vc.fixture()
    assert list(f["names"]) == list(vc.NAMES) and len(vc.NAMES) == 6
    for name, (x, y) in vc.pairs().items():
        assert x.dtype == np.float32 and x.shape == y.shape and x.shape[0] == 3
        assert f[name + "_layers64"].shape == (5,) and f[name + "_rel32"].shape == (5,)
        assert float(f[name + "_rel32"].max()) >= 1e-7      # no bar is an accident of cancellation
        assert 8e-7 <= vc.bar(name) < 1e-4
        assert abs(float(f[name + "_total32"]) - f[name + "_layers64"].sum()) <= vc.bar(name) * f[name + "_layers64"].sum()
    assert [tuple(p[0].shape[1:]) for p in vc.pairs().values()] == [(16, 16), (17, 23), (37, 53), (70, 33), (64, 200), (37, 53)]


@pytest.mark.parametrize("name", vc.NAMES)
def test_torch_path_matches_the_reference(name):
    from deblurgs_amd import lpips as lp
    x, y = (torch.from_numpy(a) for a in vc.pairs()[name])
    got = lp.lpips_layers(x, y, vc.weights())
    assert tuple(got.shape) == (1, 6) and got.dtype == torch.float32
    vc.check_against_fixture(name, got[0].numpy(), "torch fp32")
    got64 = lp.lpips_layers(x.double(), y.double(), vc.weights())[0].numpy()
    assert got64.dtype == np.float64
    assert np.allclose(got64[1:], vc.fixture()[name + "_layers64"], rtol=1e-9, atol=0.0)


def test_batch_quirk_one_value_summed_over_the_batch():
    from deblurgs_amd import lpips as lp
    p = vc.pairs()
    a, b = p["noise_37x53"], p["blend_37x53"]
    x, y = torch.from_numpy(np.stack([a[0], b[0]])), torch.from_numpy(np.stack([a[1], b[1]]))
    both = lp.lpips(x, y, vc.weights())
    assert tuple(both.shape) == (1, 1, 1, 1)
    one, two = lp.lpips(x[0], y[0], vc.weights()), lp.lpips(x[1:], y[1:], vc.weights())
    assert tuple(one.shape) == tuple(two.shape) == (1, 1, 1, 1)
    assert float(both) == pytest.approx(float(one) + float(two), rel=1e-6)
    want = float(vc.fixture()["batch2_total64"])         # the reference's own N = 2 call, in fp64
    assert abs(float(lp.lpips(x.double(), y.double(), vc.weights())) - want) <= 1e-9 * want
    assert abs(float(both) - want) <= max(vc.bar("noise_37x53"), vc.bar("blend_37x53")) * want


def test_images_below_16_are_refused_like_the_reference():
    from deblurgs_amd import lpips as lp
    w = vc.weights()
    assert w.net_type == "vgg" and lp.LPIPSWeights.net_type == "alex"
    for shape in ((3, 15, 16), (3, 16, 15), (2, 3, 15, 40)):
        with pytest.raises(ValueError, match="16"):
            lp.lpips(torch.zeros(shape), torch.zeros(shape), w)
    with pytest.raises(ValueError, match="shape"):
        lp.lpips(torch.zeros(3, 40, 40), torch.zeros(3, 40, 41), w)
    with pytest.raises(ValueError):
        lp.lpips(torch.zeros(1, 40, 40), torch.zeros(1, 40, 40), w)
    assert tuple(lp.lpips(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16), w).shape) == (1, 1, 1, 1)


def test_both_key_spellings_load_identical_weights(tmp_path):
    from deblurgs_amd.lpips import LPIPSVggWeights
    feats, lin = vc.state_dicts()
    w0 = LPIPSVggWeights.from_state_dicts(feats, lin)
    bare = {k[len("features."):]: v for k, v in feats.items()}
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}
    assert sorted(renamed) == [f"{i}.1.weight" for i in range(5)]
    w1 = LPIPSVggWeights.from_state_dicts(bare, renamed)
    assert len(w0.tensors()) == 31
    for a, b in zip(w0.tensors(), w1.tensors()):
        assert a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, b)
    assert [tuple(t.shape) for t in w0.conv_w] == [(co, ci, 3, 3) for co, ci in zip(vc.COUT, vc.CIN)]
    assert [tuple(t.shape) for t in w0.lin] == [(1, c, 1, 1) for c in (64, 128, 256, 512, 512)]
    assert w0.to("cpu").device == torch.device("cpu") and w0.to("cpu").net_type == "vgg"
    torch.save(feats, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    w2 = LPIPSVggWeights.load(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))
    for a, b in zip(w2.tensors(), w0.tensors()):
        assert torch.equal(a, b)


def test_missing_key_and_wrong_shape_are_refused_by_name():
    from deblurgs_amd.lpips import LPIPSVggWeights
    feats, lin = vc.state_dicts()
    broken = dict(feats)
    del broken["features.17.bias"]
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        LPIPSVggWeights.from_state_dicts(broken, lin)
    broken = dict(lin)
    del broken["lin3.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        LPIPSVggWeights.from_state_dicts(feats, broken)
    broken = dict(feats)
    broken["features.5.weight"] = torch.zeros(128, 64, 5, 5)
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 5, 5\)"):
        LPIPSVggWeights.from_state_dicts(broken, lin)
    broken = dict(lin)
    broken["lin1.model.1.weight"] = torch.zeros(1, 192, 1, 1)     # the alex file's shape
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        LPIPSVggWeights.from_state_dicts(feats, broken)


def _weights_struct(addr):
    from deblurgs_amd import _lib
    w = _lib.DgsLpipsVggWeights()
    for i in range(13):
        w.conv_w[i] = w.conv_b[i] = addr
    for i in range(5):
        w.lin[i] = addr
    return w


def test_lpips_vgg_argument_checks_need_no_gpu():
    """NULL pointers, n_pairs < 1 and images below 16 x 16 come back as DGS_E_ARG with a text, before any HIP call."""
    from deblurgs_amd import _lib
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(256)
    a = ctypes.cast(dummy, ctypes.c_void_p)
    w = _weights_struct(a.value)
    ok = lambda *args: L.dgs_lpips_vgg(*args)
    assert ok(None, a, 1, 16, 16, ctypes.byref(w), a, a, None) == -1 and b"null" in L.dgs_last_error()
    assert ok(a, None, 1, 16, 16, ctypes.byref(w), a, a, None) == -1
    assert ok(a, a, 1, 16, 16, None, a, a, None) == -1
    assert ok(a, a, 1, 16, 16, ctypes.byref(w), None, a, None) == -1
    assert ok(a, a, 1, 16, 16, ctypes.byref(w), a, None, None) == -1
    for field, i in (("conv_w", 0), ("conv_w", 12), ("conv_b", 7), ("lin", 4)):
        hole = _weights_struct(a.value)
        getattr(hole, field)[i] = None
        assert ok(a, a, 1, 16, 16, ctypes.byref(hole), a, a, None) == -1 and b"weight" in L.dgs_last_error(), (field, i)
    assert ok(a, a, 0, 16, 16, ctypes.byref(w), a, a, None) == -1 and b"n_pairs" in L.dgs_last_error()
    assert ok(a, a, -3, 16, 16, ctypes.byref(w), a, a, None) == -1
    assert ok(a, a, 65536, 16, 16, ctypes.byref(w), a, a, None) == -1 and b"65535" in L.dgs_last_error()
    assert ok(a, a, 1, 15, 16, ctypes.byref(w), a, a, None) == -1 and b"16 x 16" in L.dgs_last_error()     # W = 15
    assert ok(a, a, 1, 16, 15, ctypes.byref(w), a, a, None) == -1 and b"16 x 16" in L.dgs_last_error()     # H = 15
    assert ok(a, a, 1, 8192, 8192, ctypes.byref(w), a, a, None) == -1                                       # 64 H W = 2^32
    if not torch.cuda.is_available():     # (with a device the dummy pointers would be dereferenced)
        assert ok(a, a, 1, 16, 16, ctypes.byref(w), a, a, None) in (0, -3)
        assert L.dgs_conv3x3_bias_relu(a, 1, 3, 16, 16, a, a, 64, 1, a, None) in (0, -3)
        assert L.dgs_maxpool2x2(a, 1, 2, 2, a, None) in (0, -3)
    c = lambda *args: L.dgs_conv3x3_bias_relu(*args)
    assert c(None, 1, 3, 16, 16, a, a, 64, 1, a, None) == -1 and b"null" in L.dgs_last_error()
    assert c(a, 1, 3, 16, 16, a, a, 64, 1, None, None) == -1
    assert c(a, 0, 3, 16, 16, a, a, 64, 1, a, None) == -1 and b"empty" in L.dgs_last_error()
    assert c(a, 1, 3, 16, 0, a, a, 64, 0, a, None) == -1
    assert c(a, 1, 4, 16, 16, a, a, 64, 1, a, None) == -1 and b"zscore" in L.dgs_last_error()
    assert c(a, 1, 3, 16, 16, a, a, 64, 2, a, None) == -1 and b"zscore" in L.dgs_last_error()
    assert c(a, 1, 64, 8192, 8192, a, a, 64, 0, a, None) == -1 and b"32-bit" in L.dgs_last_error()
    p = lambda *args: L.dgs_maxpool2x2(*args)
    assert p(None, 1, 4, 4, a, None) == -1 and p(a, 1, 4, 4, None, None) == -1
    assert p(a, 0, 4, 4, a, None) == -1 and p(a, 1, 1, 4, a, None) == -1 and p(a, 1, 4, 1, a, None) == -1


def test_tmp_bytes_is_positive_and_monotone():
    from deblurgs_amd import _lib
    q = _lib.lib().dgs_lpips_vgg_tmp_bytes
    assert q(15, 16, 1) == 0 and q(16, 15, 1) == 0 and q(16, 16, 0) == 0 and q(16, 16, 65536) == 0
    base = q(16, 16, 1)
    assert base >= 2 * (2 * 64 * 16 * 16 * 4)           # two [2,64,H,W] maps
    prev = base
    for W in range(17, 400, 7):
        cur = q(W, 16, 1)
        assert cur >= prev > 0 and cur >= 2 * (2 * 64 * 16 * W * 4)
        prev = cur
    prev = base
    for H in range(17, 400, 7):
        cur = q(16, H, 1)
        assert cur >= prev > 0
        prev = cur
    prev = base
    for n in range(2, 40):
        cur = q(16, 16, n)
        assert cur > prev
        prev = cur
    one = q(1920, 1080, 1)
    assert 2 * (2 * 64 * 1080 * 1920 * 4) <= one < 2.2e9           # "about 2.1 GB" per 1080p pair
    assert q(1920, 1080, 2) > one > q(1280, 720, 1)


def test_symbols_struct_header_and_abi():
    from deblurgs_amd import _lib, build
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in ("dgs_lpips_vgg", "dgs_lpips_vgg_tmp_bytes", "dgs_conv3x3_bias_relu", "dgs_maxpool2x2"):
        assert hasattr(L, s) and s in _lib.EXPORTS and re.search(r"\b%s\s*\(" % s, code), s
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", text).group(1)) == 15 == _lib.ABI_VERSION == L.dgs_abi_version()
    assert ctypes.sizeof(_lib.DgsLpipsVggWeights) == 31 * ctypes.sizeof(ctypes.c_void_p)
    body = re.search(r"typedef struct DgsLpipsVggWeights \{(.*?)\} DgsLpipsVggWeights;", code, flags=re.S).group(1)
    assert re.findall(r"const float\* (\w+)\[(\d+)\];", body) == [("conv_w", "13"), ("conv_b", "13"), ("lin", "5")]
    assert [n for n, _ in _lib.DgsLpipsVggWeights._fields_] == ["conv_w", "conv_b", "lin"]
    # the file that holds the new kernels is built without FMA contraction and with nothing borrowed
    src_name = "lpips_vgg.hip" if "lpips_vgg.hip" in build.SOURCES else "lpips.hip"
    assert "-ffp-contract=off" in build.SOURCES[src_name]
    src = open(os.path.join(ROOT, "deblurgs_amd", "csrc", src_name)).read()
    assert "conv3x3_kernel" in src and "maxpool2x2_kernel" in src
    for banned in ("rocprim", "hipcub", "miopen", "getenv", "atomicAdd"):
        assert banned not in src.lower().replace("no float atomics", ""), banned


def test_header_with_the_vgg_struct_is_plain_c(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "h.c"
    src.write_text('#include "%s"\nint main(void) { DgsLpipsVggWeights w; w.conv_b[12] = 0; w.lin[4] = 0; (void)w;\n'
                   '  return (int)sizeof(w) == 31 * (int)sizeof(void*) ? 0 : 1; }\n' % os.path.join(ROOT, "include", "dgs_hip.h"))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", str(src), "-o", str(tmp_path / "h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "h")]).returncode == 0


def test_evaluate_with_vgg_weights_returns_a_triple(monkeypatch):
    """evaluate() on CPU tensors with the render stubbed out: lpips= takes either weights class."""
    from deblurgs_amd import evaluation as ev, losses, metrics
    p = vc.pairs()
    renders = [torch.from_numpy(p["noise_37x53"][0]), torch.from_numpy(p["blend_37x53"][0])]
    gts = [torch.from_numpy(p["noise_37x53"][1]), torch.from_numpy(p["blend_37x53"][1])]
    monkeypatch.setattr(ev.gaussian_renderer, "render", lambda cam, cloud, bg: {"render": renders[cam]})
    tm = losses.ToneMapping("gamma")
    pair = ev.evaluate([0, 1], None, None, gts, tm)
    triple = ev.evaluate([0, 1], None, None, gts, tm, lpips=vc.weights())
    assert len(pair) == 2 and len(triple) == 3 and all(isinstance(v, float) for v in triple)
    assert triple[:2] == pair
    want = sum(float(metrics.lpips(tm(r), g, vc.weights())) for r, g in zip(renders, gts)) / 2
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


def test_shim_evaluates_vgg_once_weights_are_there(shim, tmp_path):
    import lpips_cases as lc
    from deblurgs_amd import lpips as lp
    x, y = (torch.from_numpy(a) for a in vc.pairs()["noise_37x53"])
    with pytest.raises(NotImplementedError, match=r"vgg16-\*\.pth.*vgg\.pth.*set_default_weights.*only\s+'alex'"):
        shim.lpips(x, y, net_type="vgg")
    with pytest.raises(NotImplementedError):
        shim.lpips(x, y, net_type="squeeze")
    # registered weights are filed by backbone: alex weights do not make 'vgg' work, and the other way round
    lp.set_default_weights(lc.weights())
    with pytest.raises(NotImplementedError):
        shim.lpips(x, y, net_type="vgg")
    lp.set_default_weights(vc.weights())
    got = shim.lpips(x, y, net_type="vgg")
    want = lp.lpips(x, y, vc.weights())
    assert tuple(got.shape) == (1, 1, 1, 1) and torch.equal(got, want)
    assert torch.equal(shim.lpips(x, y, net_type="alex"), lp.lpips(x, y, lc.weights()))      # both stay registered
    assert lp.default_weights("cpu") is lc.weights() and lp.default_weights("cpu", "vgg") is vc.weights()
    lp.set_default_weights(None)                                                             # None clears both
    with pytest.raises(FileNotFoundError):
        lp.default_weights("cpu")
    with pytest.raises(FileNotFoundError, match=r"vgg16-\*\.pth.*vgg\.pth"):
        lp.default_weights("cpu", "vgg")
    # the files of a hub directory are found by name, and only there
    os.makedirs(tmp_path / "checkpoints")
    feats, lin = vc.state_dicts()
    torch.save(feats, tmp_path / "checkpoints" / "vgg16-397923af.pth")
    with pytest.raises(NotImplementedError):
        shim.lpips(x, y, net_type="vgg")             # the lin file is still missing
    torch.save(lin, tmp_path / "checkpoints" / "vgg.pth")
    assert torch.equal(shim.lpips(x, y, net_type="vgg"), want)


def test_nothing_is_fetched():
    for rel in (("deblurgs_amd", "dropin", "lpipsPyTorch", "__init__.py"), ("deblurgs_amd", "lpips.py"),
                ("deblurgs_amd", "metrics_dirs.py")):
        code = open(os.path.join(ROOT, *rel)).read()
        for banned in ("load_state_dict_from_url", "hub.load(", "download", "urllib", "requests"):
            assert banned not in code, (rel, banned)


def test_evaluate_directories_writes_the_reference_files(tmp_path):
    """PNGs in <scene>/test/<method>/{renders,gt}: results.json and per_view.json with metrics.py's keys and nesting, the
    values those of direct calls; names sorted; a missing partner raises."""
    Image = pytest.importorskip("PIL.Image")
    from deblurgs_amd import lpips as lp, metrics, metrics_dirs
    scene = tmp_path / "scene"
    rng = np.random.RandomState(5)
    imgs = {}
    for sub in ("renders", "gt"):
        os.makedirs(scene / "test" / "ours_100" / sub)
    for name in ("00002.png", "00000.png", "00001.png"):       # written out of order: the result is sorted
        base = rng.randint(0, 256, (24, 40, 3)).astype(np.uint8)
        other = np.clip(base.astype(np.int32) + rng.randint(-30, 31, base.shape), 0, 255).astype(np.uint8)
        rgba = np.concatenate([base, np.full((24, 40, 1), 255, np.uint8)], axis=2)    # four channels: the first three count
        Image.fromarray(rgba, "RGBA").save(scene / "test" / "ours_100" / "renders" / name)
        Image.fromarray(other, "RGB").save(scene / "test" / "ours_100" / "gt" / name)
        imgs[name] = (base, other)
    w = vc.weights()
    full, per_view = metrics_dirs.evaluate_directories([str(scene)], w, device="cpu")
    res = json.load(open(scene / "results.json"))
    pv = json.load(open(scene / "per_view.json"))
    assert res == full[str(scene)] and pv == per_view[str(scene)]
    assert list(res) == ["ours_100"] and list(res["ours_100"]) == ["SSIM", "PSNR", "LPIPS"]
    assert list(pv["ours_100"]) == ["SSIM", "PSNR", "LPIPS"]
    for key in ("SSIM", "PSNR", "LPIPS"):
        assert list(pv["ours_100"][key]) == ["00000.png", "00001.png", "00002.png"]
    want = {"SSIM": [], "PSNR": [], "LPIPS": []}
    for name in sorted(imgs):
        r, g = (torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1)[None].contiguous() for a in imgs[name])
        want["SSIM"].append(float(metrics.ssim(r, g)))
        want["PSNR"].append(float(metrics.psnr(r, g).mean()))
        want["LPIPS"].append(float(lp.lpips(r, g, w)))
        for key in want:
            assert pv["ours_100"][key][name] == pytest.approx(want[key][-1], rel=1e-6), (key, name)
    for key in want:
        assert res["ours_100"][key] == pytest.approx(float(torch.tensor(want[key]).mean()), rel=1e-6)
    # a render without ground truth raises instead of being skipped, and the scene is not swallowed
    os.remove(scene / "test" / "ours_100" / "gt" / "00001.png")
    with pytest.raises(FileNotFoundError, match="00001.png"):
        metrics_dirs.evaluate_directories([str(scene)], w, device="cpu")
    with pytest.raises(Exception):
        metrics_dirs.evaluate_directories([str(tmp_path / "no_such_scene")], w, device="cpu")

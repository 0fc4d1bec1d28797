"""CPU tests of LPIPS-squeeze (deblurgs_amd/lpips.py, dgs_lpips_squeeze): the torch-expression path against the
reference's own module (tests/golden/lpips_squeeze_golden.npz, made by tests/golden/make_golden_lpips_squeeze.py), the
weight loader, the C ABI's argument checks (refused before any HIP call, so they need no GPU), evaluate(..., lpips=) and
the lpipsPyTorch shim.

The bar of a pair (tests/lpips_squeeze_cases.bar) is lpips_cases' rule: 8 x the largest of the seven fp32-vs-fp64
differences the reference's own module showed on that pair.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import lpips_squeeze_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dgs_lpips_squeeze", "dgs_lpips_squeeze_tmp_bytes", "dgs_fire_bias_relu", "dgs_maxpool3x3s2_ceil")


def test_fixture_covers_the_seven_pairs():
    f = sc.fixture()
    assert list(f["names"]) == list(sc.NAMES) and len(sc.NAMES) == 7
    for name, (x, y) in sc.pairs().items():
        assert x.dtype == np.float32 and x.shape == y.shape and x.shape[0] == 3
        assert f[name + "_layers64"].shape == (7,) and f[name + "_rel32"].shape == (7,)
        assert float(f[name + "_rel32"].max()) >= 1e-7      # no bar is an accident of cancellation
        assert 8e-7 <= sc.bar(name) < 2e-4
        assert abs(float(f[name + "_total32"]) - f[name + "_layers64"].sum()) <= sc.bar(name) * f[name + "_layers64"].sum()
    assert [tuple(p[0].shape[1:]) for p in sc.pairs().values()] == \
        [(17, 17), (18, 20), (37, 53), (40, 135), (70, 33), (64, 200), (37, 53)]
    feats, _ = sc.weight_arrays()
    for idx in sc.FIRE_INDEX:                               # a padded squeeze map must be told from relu(bias)
        assert float(feats[f"features.{idx}.squeeze.bias"].min()) >= 0.1


def test_symbols_structs_header_and_abi():
    from deblurgs_amd import _lib, build
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib.EXPORTS and re.search(r"\b%s\s*\(" % s, code), s
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", text).group(1)) == 15 == _lib.ABI_VERSION == L.dgs_abi_version()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.DgsFireWeights) == 6 * ptr and ctypes.sizeof(_lib.DgsLpipsSqueezeWeights) == 57 * ptr
    body = re.search(r"typedef struct DgsFireWeights \{(.*?)\} DgsFireWeights;", code, flags=re.S).group(1)
    names = re.findall(r"const float\* (\w+);", body)
    assert names == ["squeeze_w", "squeeze_b", "expand1_w", "expand1_b", "expand3_w", "expand3_b"]
    assert [n for n, _ in _lib.DgsFireWeights._fields_] == names
    body = re.search(r"typedef struct DgsLpipsSqueezeWeights \{(.*?)\} DgsLpipsSqueezeWeights;", code, flags=re.S).group(1)
    fields = re.findall(r"(const float\*|DgsFireWeights) (\w+)(?:\[(\d+)\])?;", body)
    assert fields == [("const float*", "conv_w", ""), ("const float*", "conv_b", ""), ("DgsFireWeights", "fire", "8"),
                      ("const float*", "lin", "7")]
    assert [n for n, _ in _lib.DgsLpipsSqueezeWeights._fields_] == ["conv_w", "conv_b", "fire", "lin"]
    assert _lib.DgsLpipsSqueezeWeights.fire.offset == 2 * ptr and _lib.DgsLpipsSqueezeWeights.lin.offset == 50 * ptr
    # the kernels live in the file that is built without FMA contraction, with nothing borrowed
    assert "-ffp-contract=off" in build.SOURCES["lpips.hip"]
    src = open(os.path.join(ROOT, "deblurgs_amd", "csrc", "lpips.hip")).read()
    assert "fire_kernel" in src and "maxpool3x3s2_ceil_kernel" in src
    for banned in ("rocprim", "hipcub", "miopen", "getenv", "atomicAdd"):
        assert banned not in src.lower().replace("no float atomics", ""), banned


def test_header_with_the_squeeze_structs_is_plain_c(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "h.c"
    src.write_text('#include "%s"\nint main(void) { DgsLpipsSqueezeWeights w; w.fire[7].expand3_b = 0; w.lin[6] = 0; (void)w;\n'
                   '  return (int)sizeof(w) == 57 * (int)sizeof(void*) ? 0 : 1; }\n' % os.path.join(ROOT, "include", "dgs_hip.h"))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", str(src), "-o", str(tmp_path / "h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "h")]).returncode == 0


@pytest.mark.parametrize("name", sc.NAMES)
def test_torch_path_matches_the_reference(name):
    """fp64 on the CPU against the reference's own fp64 values: tap indices, ceil-mode pools, concatenation order, z-score
    and lin weights; fp32 within the pair's bar."""
    from deblurgs_amd import lpips as lp
    x, y = (torch.from_numpy(a) for a in sc.pairs()[name])
    got64 = lp.lpips_layers(x.double(), y.double(), sc.weights())
    assert tuple(got64.shape) == (1, 8) and got64.dtype == torch.float64
    assert np.allclose(got64[0, 1:].numpy(), sc.fixture()[name + "_layers64"], rtol=1e-9, atol=0.0)
    assert float(got64[0, 0]) == pytest.approx(float(got64[0, 1:].sum()), rel=1e-12)
    got = lp.lpips_layers(x, y, sc.weights())
    assert tuple(got.shape) == (1, 8) and got.dtype == torch.float32
    sc.check_against_fixture(name, got[0].numpy(), "torch fp32")


def test_the_taps_have_the_sizes_the_sizes_are_chosen_for():
    from deblurgs_amd import lpips as lp
    sizes = lambda h, w: [tuple(f.shape[1:]) for f in lp._features_torch(torch.zeros(1, 3, h, w), sc.weights())]
    assert sizes(17, 17) == [(64, 8, 8), (128, 4, 4), (256, 2, 2), (384, 1, 1), (384, 1, 1), (512, 1, 1), (512, 1, 1)]
    assert sizes(18, 20)[:2] == [(64, 8, 9), (128, 4, 4)]
    assert [s[1:] for s in sizes(37, 53)[:4]] == [(18, 26), (9, 13), (4, 6), (2, 3)]
    assert [s[1:] for s in sizes(40, 135)[:2]] == [(19, 67), (9, 33)]
    assert [s[1:] for s in sizes(64, 200)[:3]] == [(31, 99), (15, 49), (7, 24)]


def test_images_below_17_are_refused_like_the_reference():
    from deblurgs_amd import lpips as lp
    w = sc.weights()
    assert w.net_type == "squeeze" and w.min_size == 17
    for shape in ((3, 16, 17), (3, 17, 16), (2, 3, 16, 40)):
        with pytest.raises(ValueError, match="17"):
            lp.lpips(torch.zeros(shape), torch.zeros(shape), w)
    assert tuple(lp.lpips(torch.zeros(3, 17, 17), torch.zeros(3, 17, 17), w).shape) == (1, 1, 1, 1)


def test_both_key_spellings_load_identical_weights(tmp_path):
    from deblurgs_amd.lpips import LPIPSSqueezeWeights
    feats, lin = sc.state_dicts()
    w0 = LPIPSSqueezeWeights.from_state_dicts(feats, lin)
    bare = {k[len("features."):]: v for k, v in feats.items()}
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}
    assert sorted(renamed) == [f"{i}.1.weight" for i in range(7)]
    w1 = LPIPSSqueezeWeights.from_state_dicts(bare, renamed)
    assert len(w0.tensors()) == 57 == len(feats) + len(lin)
    for a, b in zip(w0.tensors(), w1.tensors()):
        assert a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, b)
    assert tuple(w0.conv_w.shape) == (64, 3, 3, 3) and torch.equal(w0.conv_b, feats["features.0.bias"])
    for six, idx, (ci, s, e) in zip(w0.fire, sc.FIRE_INDEX, sc.FIRES):
        assert [tuple(t.shape) for t in six] == [(s, ci, 1, 1), (s,), (e, s, 1, 1), (e,), (e, s, 3, 3), (e,)]
        assert torch.equal(six[0], feats[f"features.{idx}.squeeze.weight"])
        assert torch.equal(six[3], feats[f"features.{idx}.expand1x1.bias"])
        assert torch.equal(six[4], feats[f"features.{idx}.expand3x3.weight"])
    assert [tuple(t.shape) for t in w0.lin] == [(1, c, 1, 1) for c in (64, 128, 256, 384, 384, 512, 512)]
    assert w0.to("cpu").device == torch.device("cpu") and w0.to("cpu").net_type == "squeeze"
    torch.save(feats, tmp_path / "squeezenet1_1.pth")
    torch.save(lin, tmp_path / "squeeze.pth")
    w2 = LPIPSSqueezeWeights.load(str(tmp_path / "squeezenet1_1.pth"), str(tmp_path / "squeeze.pth"))
    for a, b in zip(w2.tensors(), w0.tensors()):
        assert torch.equal(a, b)
    s = w0.struct()
    assert s.conv_w == w0.conv_w.data_ptr() and s.fire[7].expand3_b == w0.fire[7][5].data_ptr()
    assert s.fire[2].expand1_w == w0.fire[2][2].data_ptr() and s.lin[6] == w0.lin[6].data_ptr()


def test_missing_key_and_wrong_shape_are_refused_by_name():
    from deblurgs_amd.lpips import LPIPSSqueezeWeights
    feats, lin = sc.state_dicts()
    broken = dict(feats)
    del broken["features.9.expand3x3.bias"]
    with pytest.raises(KeyError, match=r"features\.9\.expand3x3\.bias"):
        LPIPSSqueezeWeights.from_state_dicts(broken, lin)
    broken = dict(lin)
    del broken["lin5.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin5\.model\.1\.weight"):
        LPIPSSqueezeWeights.from_state_dicts(feats, broken)
    broken = dict(feats)
    broken["features.4.squeeze.weight"] = torch.zeros(16, 64, 1, 1)      # Fire 1's shape in Fire 2's place
    with pytest.raises(ValueError, match=r"features\.4\.squeeze\.weight.*\(16, 64, 1, 1\)"):
        LPIPSSqueezeWeights.from_state_dicts(broken, lin)
    broken = dict(feats)
    broken["features.0.weight"] = torch.zeros(96, 3, 7, 7)               # SqueezeNet 1.0's first convolution
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        LPIPSSqueezeWeights.from_state_dicts(broken, lin)
    broken = dict(lin)
    broken["lin3.model.1.weight"] = torch.zeros(1, 512, 1, 1)            # the vgg file's shape
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        LPIPSSqueezeWeights.from_state_dicts(feats, broken)


def _weights_struct(addr):
    from deblurgs_amd import _lib
    w = _lib.DgsLpipsSqueezeWeights()
    w.conv_w = w.conv_b = addr
    for i in range(8):
        for field, _ in _lib.DgsFireWeights._fields_:
            setattr(w.fire[i], field, addr)
    for i in range(7):
        w.lin[i] = addr
    return w


def test_argument_checks_need_no_gpu():
    """NULL pointers, n_pairs < 1, images below 17 x 17 and a squeeze depth above 64 come back as DGS_E_ARG with a text,
    before any HIP call."""
    from deblurgs_amd import _lib
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(256)
    a = ctypes.cast(dummy, ctypes.c_void_p)
    w = _weights_struct(a.value)
    ok = lambda *args: L.dgs_lpips_squeeze(*args)
    assert ok(None, a, 1, 17, 17, ctypes.byref(w), a, a, None) == -1 and b"null" in L.dgs_last_error()
    assert ok(a, None, 1, 17, 17, ctypes.byref(w), a, a, None) == -1
    assert ok(a, a, 1, 17, 17, None, a, a, None) == -1
    assert ok(a, a, 1, 17, 17, ctypes.byref(w), None, a, None) == -1
    assert ok(a, a, 1, 17, 17, ctypes.byref(w), a, None, None) == -1
    for hole in ("conv_w", "conv_b", ("fire", 0, "squeeze_w"), ("fire", 7, "expand3_b"), ("fire", 4, "expand1_w"), ("lin", 6)):
        h = _weights_struct(a.value)
        if isinstance(hole, str):
            setattr(h, hole, None)
        elif hole[0] == "lin":
            h.lin[hole[1]] = None
        else:
            setattr(h.fire[hole[1]], hole[2], None)
        assert ok(a, a, 1, 17, 17, ctypes.byref(h), a, a, None) == -1 and b"weight" in L.dgs_last_error(), hole
    assert ok(a, a, 0, 17, 17, ctypes.byref(w), a, a, None) == -1 and b"n_pairs" in L.dgs_last_error()
    assert ok(a, a, -3, 17, 17, ctypes.byref(w), a, a, None) == -1
    assert ok(a, a, 65536, 17, 17, ctypes.byref(w), a, a, None) == -1 and b"65535" in L.dgs_last_error()
    assert ok(a, a, 1, 16, 17, ctypes.byref(w), a, a, None) == -1 and b"17 x 17" in L.dgs_last_error()     # W = 16
    assert ok(a, a, 1, 17, 16, ctypes.byref(w), a, a, None) == -1 and b"17 x 17" in L.dgs_last_error()     # H = 16
    assert ok(a, a, 1, 32768, 32768, ctypes.byref(w), a, a, None) == -1                                    # 3 H W = 3 * 2^30
    fw = _lib.DgsFireWeights(*([a.value] * 6))
    f = lambda *args: L.dgs_fire_bias_relu(*args)
    assert f(None, 1, 8, 4, 4, 16, 8, 8, ctypes.byref(fw), None, a, None) == -1 and b"null" in L.dgs_last_error()
    assert f(a, 1, 8, 4, 4, 16, 8, 8, None, None, a, None) == -1
    assert f(a, 1, 8, 4, 4, 16, 8, 8, ctypes.byref(fw), None, None, None) == -1
    for i in range(6):
        ptrs = [a.value] * 6
        ptrs[i] = None
        assert f(a, 1, 8, 4, 4, 16, 8, 8, ctypes.byref(_lib.DgsFireWeights(*ptrs)), None, a, None) == -1, i
        assert b"null" in L.dgs_last_error()
    assert f(a, 0, 8, 4, 4, 16, 8, 8, ctypes.byref(fw), None, a, None) == -1 and b"empty" in L.dgs_last_error()
    assert f(a, 1, 0, 4, 4, 16, 8, 8, ctypes.byref(fw), None, a, None) == -1
    assert f(a, 1, 8, 4, 4, 16, 0, 8, ctypes.byref(fw), None, a, None) == -1
    assert f(a, 1, 8, 4, 4, 16, 8, 0, ctypes.byref(fw), None, a, None) == -1
    assert f(a, 1, 8, 4, 4, 0, 8, 8, ctypes.byref(fw), None, a, None) == -1 and b"1..64" in L.dgs_last_error()
    assert f(a, 1, 8, 4, 4, 65, 8, 8, ctypes.byref(fw), None, a, None) == -1 and b"1..64" in L.dgs_last_error()
    assert f(a, 1, 64, 8192, 8192, 16, 8, 8, ctypes.byref(fw), None, a, None) == -1 and b"32-bit" in L.dgs_last_error()
    p = lambda *args: L.dgs_maxpool3x3s2_ceil(*args)
    assert p(None, 1, 4, 4, a, None) == -1 and p(a, 1, 4, 4, None, None) == -1
    assert p(a, 0, 4, 4, a, None) == -1 and p(a, 1, 1, 4, a, None) == -1 and p(a, 1, 4, 1, a, None) == -1
    if not torch.cuda.is_available():     # (with a device the dummy pointers would be dereferenced)
        assert ok(a, a, 1, 17, 17, ctypes.byref(w), a, a, None) in (0, -3)
        assert f(a, 1, 8, 4, 4, 16, 8, 8, ctypes.byref(fw), None, a, None) in (0, -3)
        assert p(a, 1, 2, 2, a, None) in (0, -3)


def test_tmp_bytes_is_positive_and_monotone():
    from deblurgs_amd import _lib
    q = _lib.lib().dgs_lpips_squeeze_tmp_bytes
    assert q(16, 17, 1) == 0 and q(17, 16, 1) == 0 and q(17, 17, 0) == 0 and q(17, 17, 65536) == 0
    base = q(17, 17, 1)
    assert base >= 2 * (2 * 64 * 8 * 8 * 4)             # two [2,64,8,8] maps
    prev = base
    for W in range(18, 400, 7):
        cur = q(W, 17, 1)
        assert cur >= prev > 0 and cur >= 2 * (2 * 64 * 8 * ((W - 3) // 2 + 1) * 4)
        prev = cur
    prev = base
    for H in range(18, 400, 7):
        cur = q(17, H, 1)
        assert cur >= prev > 0
        prev = cur
    prev = base
    for n in range(2, 40):
        cur = q(17, 17, n)
        assert cur > prev
        prev = cur
    one = q(1920, 1080, 1)
    assert one == 529328896 and one >= 2 * (2 * 64 * 539 * 959 * 4)       # the figure include/dgs_hip.h states
    assert "529,328,896" in open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    assert q(1920, 1080, 2) > one > q(1280, 720, 1)


def test_evaluate_with_squeeze_weights_returns_a_triple(monkeypatch):
    """evaluate() on CPU tensors with the render stubbed out: lpips= takes the squeeze weights through the same dispatch."""
    from deblurgs_amd import evaluation as ev, losses, lpips as lp
    p = sc.pairs()
    renders = [torch.from_numpy(p["noise_37x53"][0]), torch.from_numpy(p["blend_37x53"][0])]
    gts = [torch.from_numpy(p["noise_37x53"][1]), torch.from_numpy(p["blend_37x53"][1])]
    monkeypatch.setattr(ev.gaussian_renderer, "render", lambda cam, cloud, bg: {"render": renders[cam]})
    tm = losses.ToneMapping("gamma")
    pair = ev.evaluate([0, 1], None, None, gts, tm)
    triple = ev.evaluate([0, 1], None, None, gts, tm, lpips=sc.weights())
    assert len(pair) == 2 and len(triple) == 3 and all(isinstance(v, float) for v in triple)
    assert triple[:2] == pair
    want = sum(float(lp.lpips_layers(tm(r), g, sc.weights())[0, 0]) for r, g in zip(renders, gts)) / 2
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


def test_shim_evaluates_squeeze_once_weights_are_there(shim, tmp_path):
    import lpips_vgg_cases as vc
    from deblurgs_amd import lpips as lp
    p = sc.pairs()
    a, b = p["noise_37x53"], p["blend_37x53"]
    x, y = torch.from_numpy(np.stack([a[0], b[0]])), torch.from_numpy(np.stack([a[1], b[1]]))
    with pytest.raises(NotImplementedError, match=r"squeezenet1_1-\*\.pth.*squeeze\.pth.*set_default_weights"):
        shim.lpips(x, y, net_type="squeeze")
    with pytest.raises(NotImplementedError):
        shim.lpips(x, y, net_type="resnet")
    lp.set_default_weights(vc.weights())             # filed by backbone: vgg weights do not make 'squeeze' work
    with pytest.raises(NotImplementedError):
        shim.lpips(x, y, net_type="squeeze")
    lp.set_default_weights(sc.weights())
    got = shim.lpips(x.double(), y.double(), net_type="squeeze")
    want = float(sc.fixture()["batch2_total64"])     # the reference's own N = 2 call, in fp64: ONE value, summed over the batch
    assert tuple(got.shape) == (1, 1, 1, 1) and abs(float(got) - want) <= 1e-9 * want
    got32 = shim.lpips(x, y, net_type="squeeze")
    assert tuple(got32.shape) == (1, 1, 1, 1) and torch.equal(got32, lp.lpips(x, y, sc.weights()))
    assert abs(float(got32) - want) <= max(sc.bar("noise_37x53"), sc.bar("blend_37x53")) * want
    assert lp.default_weights("cpu", "squeeze") is sc.weights() and lp.default_weights("cpu", "vgg") is vc.weights()
    lp.set_default_weights(None)
    with pytest.raises(FileNotFoundError, match=r"squeezenet1_1-\*\.pth.*squeeze\.pth"):
        lp.default_weights("cpu", "squeeze")
    # the files of a hub directory are found by name, and only there
    os.makedirs(tmp_path / "checkpoints")
    feats, lin = sc.state_dicts()
    torch.save(feats, tmp_path / "checkpoints" / "squeezenet1_1-b8a52dc0.pth")
    with pytest.raises(NotImplementedError):
        shim.lpips(x, y, net_type="squeeze")         # the lin file is still missing
    torch.save(lin, tmp_path / "checkpoints" / "squeeze.pth")
    assert torch.equal(shim.lpips(x, y, net_type="squeeze"), got32)


def test_nothing_is_fetched():
    for rel in (("deblurgs_amd", "dropin", "lpipsPyTorch", "__init__.py"), ("deblurgs_amd", "lpips.py")):
        code = open(os.path.join(ROOT, *rel)).read()
        for banned in ("load_state_dict_from_url", "hub.load(", "download", "urllib", "requests"):
            assert banned not in code, (rel, banned)

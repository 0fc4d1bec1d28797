"""CPU tests of the visual reports (deblurgs_amd/report.py, csrc/report.hip): the new entry points are declared, exported and
bound and reject bad arguments before any HIP call; the restated percentile formula equals the installed numpy's
np.percentile bit for bit; the jet tables equal tests/golden/report_golden.npz (matplotlib's own map,
tests/golden/make_golden_report.py); the wrappers refuse CPU tensors; the file names are the reference's."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import report_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "report_golden.npz")
NEW_SYMBOLS = ("dgs_order_stats_tmp_bytes", "dgs_order_stats", "dgs_percentiles", "dgs_report_images", "dgs_scalar_colorize")


def test_new_symbols_are_declared_exported_and_bound():
    from deblurgs_amd import _lib, build
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(L, s) and (s + "(") in header, s
        assert getattr(L, s).argtypes == _lib.EXPORTS[s][1]
    assert L.dgs_abi_version() == 15 == _lib.ABI_VERSION           # additions to ABI 15
    assert build.SOURCES["report.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(ROOT, "deblurgs_amd", "csrc", "report.hip"))


def test_order_stats_tmp_bytes_is_a_function_of_n_and_m():
    from deblurgs_amd import _lib
    L = _lib.lib()
    assert L.dgs_order_stats_tmp_bytes(0, 1) == 0 and L.dgs_order_stats_tmp_bytes(10, 0) == 0
    assert L.dgs_order_stats_tmp_bytes(10, 5) == 0 and L.dgs_order_stats_tmp_bytes(2**32, 1) == 0
    one = L.dgs_order_stats_tmp_bytes(1, 1)
    assert one == L.dgs_order_stats_tmp_bytes(8192, 1) == 256 + 2 * 1024          # one block, the two neighbours of a percentile
    assert L.dgs_order_stats_tmp_bytes(8193, 1) == 256 + 2 * 2 * 1024
    assert L.dgs_order_stats_tmp_bytes(1920 * 1080, 4) == 256 + 254 * 8 * 1024
    assert L.dgs_order_stats_tmp_bytes(2**32 - 1, 4) == L.dgs_order_stats_tmp_bytes(10**9, 4) == 256 + 2048 * 8 * 1024


def test_select_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096                                      # non-null dummies: only the argument logic runs
    ranks = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    qs = (ctypes.c_double * 4)(0.0, 1.0, 50.0, 100.0)

    def stats(x=a, n=10, r=ranks, m=4, out=a, tmp=a):
        return L.dgs_order_stats(x, n, r, m, out, tmp, None)

    def perc(x=a, n=10, q=qs, m=4, out=a, tmp=a):
        return L.dgs_percentiles(x, n, q, m, out, tmp, None)

    for fn, name in ((stats, b"order_stats"), (perc, b"percentiles")):
        for kw, text in (({"x": None}, b"null"), ({"out": None}, b"null"), ({"tmp": None}, b"null"), ({"n": 0}, b"at least 1"),
                         ({"n": 2**32}, b"2^32 - 1"), ({"m": 0}, b"1..4"), ({"m": 5}, b"1..4"), ({"m": -1}, b"1..4"),
                         ({"x": a + 2}, b"aligned"), ({"tmp": a + 1}, b"aligned")):
            assert fn(**kw) == -1, (name, kw)
            assert text in L.dgs_last_error() and name in L.dgs_last_error(), (kw, L.dgs_last_error())
    assert stats(r=None) == -1 and b"null" in L.dgs_last_error()
    assert perc(q=None) == -1 and b"null" in L.dgs_last_error()
    assert stats(n=3) == -1 and b"rank" in L.dgs_last_error()                      # rank 3 of 3 values
    assert stats(r=(ctypes.c_uint64 * 1)(2**40), m=1) == -1 and b"rank" in L.dgs_last_error()
    for bad in (-0.5, 100.5, float("nan"), float("inf")):
        assert perc(q=(ctypes.c_double * 1)(bad), m=1) == -1 and b"[0, 100]" in L.dgs_last_error(), bad
    assert perc(out=a + 4) == -1 and b"8-byte" in L.dgs_last_error()
    with pytest.raises(RuntimeError, match="dgs_order_stats failed"):
        _lib.check(stats(n=0), "dgs_order_stats")


def test_report_images_and_colorize_argument_errors_need_no_gpu():
    from deblurgs_amd import _lib
    L = _lib.lib()
    a = 4096
    ok = dict(x=a, K=3, mean=0, H=10, W=12, tone=_lib.TONE_IDENTITY, eps=0.0, bound=0.0, gt=a, out=a, gt_u8=a, err=a)

    def images(**kw):
        v = dict(ok, **kw)
        return L.dgs_report_images(v["x"], v["K"], v["mean"], v["H"], v["W"], v["tone"], v["eps"], v["bound"], v["gt"],
                                   v["out"], v["gt_u8"], v["err"], None)

    for kw, text in (({"x": None}, b"null"), ({"out": None}, b"null"), ({"gt": None}, b"null"),
                     ({"gt": None, "gt_u8": None}, b"null"), ({"gt": None, "err": None}, b"null"),
                     ({"K": 0}, b"K must be"), ({"K": -2}, b"K must be"), ({"K": 65536}, b"K must be"),
                     ({"mean": 2}, b"mean"), ({"H": 0}, b"empty image"), ({"W": -1}, b"empty image"),
                     ({"tone": 2}, b"tone_mapping"), ({"tone": -1}, b"tone_mapping"),
                     ({"tone": _lib.TONE_GAMMA, "bound": 0.5}, b"bound"),
                     ({"tone": _lib.TONE_GAMMA, "bound": float("nan")}, b"bound"),
                     ({"x": a + 1}, b"aligned"), ({"err": a + 2}, b"aligned")):
        assert images(**kw) == -1, kw
        assert text in L.dgs_last_error() and b"report_images" in L.dgs_last_error(), (kw, L.dgs_last_error())
    for args, text in (((None, 5, a, a, a), b"null"), ((a, 5, None, a, a), b"null"), ((a, 5, a, None, a), b"null"),
                       ((a, 5, a, a, None), b"null"), ((a, 0, a, a, a), b"n must be"), ((a, 5, a, a + 1, a), b"lut must be"),
                       ((a, 5, a, a + 2, a), b"lut must be"), ((a, 5, a + 4, a, a), b"8-byte")):
        assert L.dgs_scalar_colorize(*args, None) == -1 and text in L.dgs_last_error(), args


def test_percentile_restatement_equals_numpy_bit_for_bit():
    """What dgs_percentiles evaluates (tests/report_cases.percentile_restated over rc.percentile_plan) against the
    installed numpy's np.percentile(float32 array, (q, 100)): 8 sizes x 5 percentages x 3 scales, with ties."""
    cases = 0
    for n in rc.PERCENTILE_NS:
        for scale in rc.SCALES:
            x = rc.normal_with_ties(n, scale)
            s = np.sort(x)
            for q in rc.PERCENTILE_QS:
                want = np.percentile(x, (q, 100))
                assert want.dtype == np.float64
                got = np.array([rc.percentile_restated(s, q), rc.percentile_restated(s, 100)])
                assert rc.same_bits(got, want), (n, scale, q, got, want)
                cases += 1
    assert cases == 120
    # a scalar q is another code path of numpy's (float32 out): the reference passes a tuple, and so does colorize
    assert np.percentile(rc.normal_with_ties(63, 1.0), 37.5).dtype == np.float32


def test_percentile_plan_and_clip_rank():
    from deblurgs_amd import report
    assert rc.percentile_plan(1, 50.0) == (0, 0, 1.0)                # at the top numpy's weight is v - (-1)
    assert rc.percentile_plan(11, 100.0) == (10, 10, 11.0)
    assert rc.percentile_plan(11, 0.0) == (0, 1, 0.0)
    i, above, g = rc.percentile_plan(1000, 37.5)
    assert (i, above) == (374, 375) and g == 999 * 0.375 - 374
    for n in (1, 2, 63, 257, 70_001, 1920 * 1080, 50 * 1920 * 1080):
        for p in (0.0, 0.5, 0.9, 0.99, 0.999, 1.0):
            assert report.clip_rank(n, p) == int((n - 1) * p)
            assert 0 <= report.clip_rank(n, p) <= n - 1


def test_jet_tables_equal_the_fixture():
    from deblurgs_amd import render_path as rp, report
    g = np.load(GOLDEN)
    for rounded, key in ((False, "jet"), (True, "jet_rounded")):
        lut = report.jet_table(rounded)
        assert lut.dtype == np.uint8 and lut.shape == (256, 4)
        assert np.array_equal(lut, g[key]), key
    assert tuple(report.jet_table(False)[0]) == (0, 0, 127, 255) and tuple(report.jet_table(True)[0]) == (0, 0, 128, 255)
    assert tuple(report.jet_table(True)[255]) == (128, 0, 0, 255)
    assert not np.array_equal(report.jet_table(False)[::-1], rp.jet_r_table())     # jet, not a flipped jet_r
    src = open(os.path.join(ROOT, "deblurgs_amd", "report.py")).read()
    assert "import matplotlib" not in src and "import cv2" not in src and "import torchvision" not in src


def test_wrappers_refuse_cpu_tensors_and_the_paths_that_need_cv2():
    import torch
    from deblurgs_amd import report
    x = torch.zeros(4, 4)
    for call in (lambda: report.order_stats(x, [0]), lambda: report.percentiles(x, (1.0, 100.0)), lambda: report.colorize(x),
                 lambda: report.depth_colorize(x[None], clip_percentage=0.99),
                 lambda: report.report_images(torch.zeros(1, 3, 4, 4)),
                 lambda: report.view_report(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4)),
                 lambda: report.scalar_colorize(x, torch.zeros(2, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(NotImplementedError, match="mask"):
        report.colorize(x, mask=torch.ones(4, 4))
    with pytest.raises(NotImplementedError, match="colour bar"):
        report.colorize(x, append_cbar=True)
    with pytest.raises(NotImplementedError, match="jet"):
        report.colorize(x, cmap_name="viridis")


def test_file_names_are_the_reference_s_and_the_writer_takes_the_place_of_the_files(tmp_path):
    from deblurgs_amd import evaluation as ev, report
    assert report.evaluate_names(7) == ("007_gt.png", "007_render.png", "007_error.png")
    assert report.traj_render_names(12, 3) == ["012_00.png", "012_01.png", "012_02.png", "012_blur.png", "012_gt.png",
                                               "012_l1.png"]
    assert report.traj_render_names(0, 1) == ["000_00.png", "000_blur.png", "000_gt.png", "000_l1.png"]
    assert report.traj_render_directory("out/run", 30) == "out/run/traj_render_00030"
    seen = []
    img = (np.arange(5 * 7 * 3) % 256).astype(np.uint8).reshape(5, 7, 3)
    path = str(tmp_path / "nowhere" / "000_gt.png")
    assert report.write_image(path, img, writer=lambda p, a: seen.append((p, a))) == path
    assert seen[0][0] == path and np.array_equal(seen[0][1], img) and not (tmp_path / "nowhere").exists()
    d = report.fresh_directory(str(tmp_path / "vis"))
    (tmp_path / "vis" / "stale.png").write_bytes(b"x")
    assert os.listdir(report.fresh_directory(d)) == []                               # removed and recreated
    written = report.write_image(os.path.join(d, "000_render.png"), img)
    try:
        from PIL import Image
    except ImportError:
        assert written.endswith("000_render.npy") and np.array_equal(np.load(written), img)
    else:
        assert written.endswith("000_render.png") and np.array_equal(np.asarray(Image.open(written)), img)
    sig = inspect.signature(ev.evaluate).parameters
    assert sig["vis_dir"].default is None and sig["writer"].default is None and sig["views_per_call"].default is None
    sig = inspect.signature(report.traj_render).parameters
    assert sig["num_visualize_subframes"].default == 3 and sig["background"].default is None and sig["writer"].default is None


def test_traj_render_and_evaluate_refuse_what_cannot_work():
    """No device: traj_render raises before it touches a directory; a writer without vis_dir, and a vis_dir that can only be
    a mistake, are refused before anything is rendered or removed."""
    import torch
    from deblurgs_amd import evaluation as ev, report

    class Cloud:
        _xyz = torch.zeros(4, 3)

    seen = []
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        report.traj_render(None, Cloud(), "model", 30, writer=lambda p, a: seen.append(p))
    assert not seen and not os.path.exists("model")
    with pytest.raises(ValueError, match="vis_dir"):
        ev.evaluate([], None, None, [], "identity", writer=lambda p, a: seen.append(p))
    for bad in ("", "  ", os.sep, os.path.expanduser("~"), ".", os.getcwd(), os.path.dirname(os.getcwd())):
        with pytest.raises(ValueError):
            ev.evaluate([], None, None, [], "identity", vis_dir=bad)
        with pytest.raises(ValueError):
            report.fresh_directory(bad)
    assert os.path.isdir(os.getcwd()) and not seen

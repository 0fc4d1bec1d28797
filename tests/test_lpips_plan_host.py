"""The one plan function and the one argument prologue of csrc/lpips.hip against the three of each they replaced:
tests/golden/lpips_tmp_bytes.json holds dgs_lpips_{alex,vgg,squeeze}_tmp_bytes over a grid of sizes and the
dgs_last_error() texts of a list of refused calls, recorded by tests/golden/make_lpips_tmp_bytes.py from a library built
before the change.  Equality, numbers and texts; no device is touched.
"""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_lpips_tmp_bytes", os.path.join(GOLDEN, "make_lpips_tmp_bytes.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "lpips_tmp_bytes.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("net", list(make.NETS))
def test_tmp_bytes_are_those_of_the_three_plan_functions(net, golden):
    from deblurgs_amd import _lib
    q = getattr(_lib.lib(), f"dgs_lpips_{net}_tmp_bytes")
    want = golden[net]["tmp_bytes"]
    assert [tuple(row[:3]) for row in want] == make.size_cases(net) and len(want) > 350
    got = [[W, H, n, q(W, H, n)] for W, H, n, _ in want]
    assert got == want
    m = make.NETS[net]
    sizes = {(W, H, n): b for W, H, n, b in want}
    assert sizes[m, m, 1] > 0 and sizes[1920, 1080, 40] > 0 and sizes[65536, m, 1] > 0       # accepted corners ...
    assert sizes[m - 1, m, 1] == sizes[m, m - 1, 1] == sizes[m, m, 0] == sizes[m, m, 65536] == 0   # ... and refused ones
    assert sizes[65537, m, 1] == sizes[32768, 32768, 1] == 0


@pytest.mark.parametrize("net", list(make.NETS))
def test_refused_calls_say_what_they_said(net, golden):
    from deblurgs_amd import _lib
    L = _lib.lib()
    f = getattr(L, f"dgs_lpips_{net}")
    want = golden[net]["refused"]
    calls = make.refused_calls(net)
    assert [w["call"] for w in want] == [label for label, _, _ in calls] and len(calls) == 8
    for w, (label, args, _keep) in zip(want, calls):
        assert w["rc"] == -1 and w["error"].startswith(f"lpips_{net}: "), label
        assert (f(*args), L.dgs_last_error().decode()) == (w["rc"], w["error"]), label

"""Host-side rules of the reference-kernel recipe (oracle/ref_rasterizer.py): no GPU and no reference tree needed."""
import json
import os

import numpy as np
import pytest

from oracle import ref_rasterizer as rr


@pytest.fixture
def fake_ref_dir(tmp_path, monkeypatch):
    """oracle/_ref/ redirected to an empty directory."""
    monkeypatch.setattr(rr, "REF_DIR", str(tmp_path))
    monkeypatch.setattr(rr, "BUILD_INFO", str(tmp_path / "BUILD_INFO.json"))
    return tmp_path


def _fill(d, **over):
    for v in rr.VARIANTS:
        (d / os.path.basename(rr.lib_path(v))).write_bytes(b"not a library")
    info = dict(reference_sources={}, recipe=rr.recipe_hash(), wrapper=rr.wrapper_hash(), compiler="x")
    info.update(over)
    (d / "BUILD_INFO.json").write_text(json.dumps(info))


def test_build_is_a_no_op_without_the_reference_tree(fake_ref_dir, monkeypatch):
    monkeypatch.setenv("DGS_REFERENCE_ROOT", str(fake_ref_dir / "no_such_tree"))
    assert not rr.reference_present() and not rr.available()
    assert rr.build_ref() is None and rr.build_ref(force=True) is None
    assert os.listdir(fake_ref_dir) == []
    _fill(fake_ref_dir)                       # ... and what is there stays as it is
    before = {n: (fake_ref_dir / n).read_bytes() for n in os.listdir(fake_ref_dir)}
    assert rr.build_ref(force=True) is None and rr.available()
    assert {n: (fake_ref_dir / n).read_bytes() for n in os.listdir(fake_ref_dir)} == before


def test_loader_refuses_libraries_of_another_recipe_or_wrapper(fake_ref_dir):
    with pytest.raises(RuntimeError, match="no reference-kernel libraries"):
        rr.check_build_info()
    _fill(fake_ref_dir)
    assert rr.check_build_info()["recipe"] == rr.recipe_hash()
    for field in ("recipe", "wrapper"):
        _fill(fake_ref_dir, **{field: "0" * 64})
        with pytest.raises(RuntimeError, match="another recipe or wrapper"):
            rr.check_build_info()
    _fill(fake_ref_dir)
    (fake_ref_dir / "BUILD_INFO.json").unlink()
    with pytest.raises(RuntimeError, match="BUILD_INFO.json"):
        rr.check_build_info()


def test_recipe_hash_covers_flags_edits_and_shims(monkeypatch, tmp_path):
    base = rr.recipe_hash()
    assert base == rr.recipe_hash()
    monkeypatch.setattr(rr, "FLAGS", rr.FLAGS + ("-DX",))
    assert rr.recipe_hash() != base
    monkeypatch.undo()
    monkeypatch.setattr(rr, "EDITS", rr.EDITS[:1])
    assert rr.recipe_hash() != base
    monkeypatch.undo()
    shim = tmp_path / "refshim"
    shim.mkdir()
    (shim / "cuda.h").write_text("#pragma once\n")
    monkeypatch.setattr(rr, "SHIM_DIR", str(shim))
    assert rr.recipe_hash() != base


def test_recipe_keeps_to_its_build_rules():
    flags = " ".join(rr.FLAGS + sum(rr.VARIANTS.values(), ()))
    assert "--offload-arch=gfx950" in flags and "xnack+" not in flags and "sanitize" not in flags
    assert "fast-math" not in flags and "unsafe-fp-atomics" not in flags
    assert rr.VARIANTS["f32"] == ("-ffp-contract=off",) and rr.VARIANTS["fma"] == ("-ffp-contract=fast",)
    assert rr.MAX_JOBS <= 16
    assert rr.EDITS == ((r"<< <", "<<<"), (r">> >", ">>>"))


def test_empty_cloud_guard_needs_no_library(fake_ref_dir):
    """P == 0 returns zero images before any library is loaded, as the reference's binding returns before any launch."""
    sc = dict(W=40, H=24, sh_degree=2, means3D=np.zeros((0, 3), np.float32), sh=np.zeros((0, 9, 3), np.float32))
    r = rr.forward(sc, 0)
    assert r["num_rendered"] == 0 and r["color"].shape == (3, 24, 40) and not r["color"].any() and not r["depth"].any()
    assert r["ranges"].shape == (6, 2) and r["n_contrib"].shape == (960,) and r["radii"].size == 0

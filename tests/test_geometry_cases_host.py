"""Host side of the isolated per-Gaussian backward test (tests/geometry_cases.py), on the CPU oracle and torch alone: every
case populates the branches it was built for, the float64 reference is the linear functional of the totals it claims to
be, and its float32 evaluation -- the yardstick of the GPU test's bars -- is finite for every output."""
import numpy as np
import pytest
import torch

import geometry_cases as GC
from geometry_cases import measures

NAMES = list(GC.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_meets_its_conditions(name):
    info = GC.conditions(GC.make(name))
    print(f"\n[geometry case {name}] " + ", ".join(f"{k}: {v}" for k, v in info.items()))


@pytest.mark.parametrize("name", ["deg3", "raw_hinge", "cov3D_precomp", "colors_precomp"])
def test_reference_is_linear_in_the_totals(name):
    """ref(S1 + S2) = ref(S1) + ref(S2) within float64 rounding (1e-12 of the largest entry of a key; the hinge term, which
    does not depend on S, is left out).  S1 + S2 is formed in float64 and handed over as such."""
    case = GC.make(name)
    rng = np.random.default_rng(3)
    S1 = case["S"].astype(np.float64)
    S2 = rng.normal(0.0, 1.0, S1.shape) * 10.0 ** rng.uniform(-3.0, 0.0, S1.shape[:2] + (1,))
    r1, r2, r12 = (GC.reference(case, torch.float64, S=s, hinge=False) for s in (S1, S2, S1 + S2))
    for key in GC.output_keys(case) + ["A_view", "A_proj"]:
        scale = max(np.abs(r1[key]).max(), np.abs(r2[key]).max())
        assert scale > 0, key
        if key.startswith("A_"):      # sums of absolute values: sub-additive, not additive
            assert (r12[key] <= (r1[key] + r2[key]) * (1 + 1e-12)).all(), key
            continue
        err = np.abs(r12[key] - (r1[key] + r2[key])).max() / scale
        assert err < 1e-12, f"{key}: {err:.2e}"


@pytest.mark.parametrize("name", NAMES)
def test_float32_gap_of_the_reference_is_finite(name):
    """The float32-vs-float64 gap of every key, in both measures (printed): 4 x this gap, floored, is the bar the kernel is
    held to on the device."""
    case = GC.make(name)
    r64, r32 = GC.reference(case, torch.float64), GC.reference(case, torch.float32)
    line = []
    for key in GC.output_keys(case):
        assert np.isfinite(r64[key]).all() and np.isfinite(r32[key]).all(), key
        if key in ("dL_dviewmatrix", "dL_dprojmatrix"):
            A = r64["A_view" if key == "dL_dviewmatrix" else "A_proj"]
            nz = A > 0
            gap = float((np.abs(r32[key] - r64[key])[nz] / A[nz]).max()) if nz.any() else 0.0
            assert np.isfinite(gap)
            line.append(f"{key} {gap:.1e} of A")
            continue
        if key == "dL_drotations" and "A_rot" in r64:
            gap = float((np.abs(r32[key] - r64[key]) / np.maximum(r64["A_rot"], 1e-300)).max())
            assert np.isfinite(gap) and float((np.abs(r64[key]) / np.maximum(r64["A_rot"], 1e-300)).max()) < 1e-12
            line.append(f"{key} {gap:.1e} of A_rot")
            continue
        col, row = measures(r32[key], r64[key], key)
        assert np.isfinite(col) and np.isfinite(row), key
        line.append(f"{key} col {col:.1e} row {row:.1e}")
    print(f"\n[geometry case {name}: fp32 vs fp64] " + "; ".join(line))

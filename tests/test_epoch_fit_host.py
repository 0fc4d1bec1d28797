"""CPU tests of the epoch-fused test-view pose fit (deblurgs_amd.evaluation.EpochPoseFit): its entry points are declared,
bound and check their arguments before any HIP call, and the pure-host schedule (epoch_rows) carries the positions and,
bit for bit, the Adam scalars of the sequential fit's schedule (step_rows)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPOCH_SYMBOLS = ["dgs_adam_epoch_peek", "dgs_adam_epoch_step", "dgs_testpose_forward_rows", "dgs_testpose_backward_rows",
                 "dgs_view_loss_grad_rows", "dgs_l2_ema_epoch"]


def test_epoch_entry_points_are_declared_and_bound_and_the_abi_stays_15():
    from deblurgs_amd import _lib
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", text).group(1)) == 15 == _lib.ABI_VERSION
    L = _lib.lib()
    assert L.dgs_abi_version() == 15
    for s in EPOCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s + " is not declared in include/dgs_hip.h"
        assert s in _lib.EXPORTS and hasattr(L, s), s


def _adam_groups(a, n=5):
    from deblurgs_amd import _lib
    return (_lib.DgsAdamGroup * 2)(_lib.DgsAdamGroup(a, a, a, a, 4 * n, 1e-3, 1), _lib.DgsAdamGroup(a, a, a, a, 3 * n, 1e-3, 1))


def test_epoch_entry_points_check_their_arguments_without_a_gpu():
    """Dummy host addresses and a NULL stream: every call below must return DGS_E_ARG before touching HIP."""
    from deblurgs_amd import _lib
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(256)
    a = ctypes.cast(dummy, ctypes.c_void_p)
    n = 5
    g = _adam_groups(a.value, n)
    outs = (ctypes.c_void_p * 2)(a.value, a.value)
    B = (0.9, 0.999, 1e-15)
    K = _lib.DGS_MAX_K

    def peek(groups=g, n_groups=2, out=outs, n=n, b=0, e=n, pos=a, sc=a, steps=n):
        return L.dgs_adam_epoch_peek(groups, n_groups, out, n, b, e, pos, sc, steps, *B, None)

    def step(groups=g, n_groups=2, n=n, b=0, e=n, pos=a, sc=a, steps=n):
        return L.dgs_adam_epoch_step(groups, n_groups, n, b, e, pos, sc, steps, *B, None, None)

    for fn in (peek, step):
        assert fn(groups=None) == -1
        assert fn(pos=None) == -1 and fn(sc=None) == -1
        assert fn(n=0, e=0) == -1
        assert fn(b=2, e=2) == -1 and fn(b=3, e=2) == -1 and fn(b=-1) == -1      # empty / reversed / negative range
        assert fn(e=n + 1) == -1
        assert fn(steps=K + 1) == -1 and fn(steps=0) == -1
        assert b"n_steps" in L.dgs_last_error()
        assert fn(n_groups=0) == -1 and fn(n_groups=5) == -1
    assert peek(out=None) == -1
    assert peek(out=(ctypes.c_void_p * 2)(a.value, None)) == -1
    bad = _adam_groups(a.value, n)
    bad[1].exp_avg_sq = None
    assert peek(groups=bad) == -1 and step(groups=bad) == -1
    bad = _adam_groups(a.value, n)
    bad[0].grad = None
    assert step(groups=bad) == -1                       # (the peek reads no gradient)
    bad = _adam_groups(a.value, n)
    bad[0].numel = 4 * n + 1                            # not n rows of equal width
    assert peek(groups=bad) == -1 and step(groups=bad) == -1
    assert b"adam_epoch_step" in L.dgs_last_error()

    fwd = lambda rot=a, trans=a, n=n, b=0, e=n, proj=a, view=a, full=a, cam=a: \
        L.dgs_testpose_forward_rows(rot, trans, n, b, e, proj, view, full, cam, None)
    bwd = lambda rot=a, trans=a, n=n, b=0, e=n, proj=a, gv=a, gf=a, gr=a, gt=a: \
        L.dgs_testpose_backward_rows(rot, trans, n, b, e, proj, gv, gf, gr, gt, None)
    for fn in (fwd, bwd):
        assert fn(rot=None) == -1 and fn(trans=None) == -1 and fn(proj=None) == -1
        assert fn(n=0, e=0) == -1 and fn(b=2, e=2) == -1 and fn(e=n + 1) == -1 and fn(b=-1) == -1
        assert fn(n=K + 10, e=K + 1) == -1                                       # more than DGS_MAX_K rows in one call
        assert b"DGS_MAX_K" in L.dgs_last_error()
    assert fwd(view=None) == -1 and fwd(full=None) == -1 and fwd(cam=None) == -1
    assert bwd(gv=None) == -1 and bwd(gf=None) == -1 and bwd(gr=None) == -1 and bwd(gt=None) == -1

    def loss(x=a, gt=a, n_gt=3, b=0, e=3, C=3, HW=16, tone=0, eps=1e-8, bound=0.0, dx=a, work=a):
        return L.dgs_view_loss_grad_rows(x, gt, n_gt, b, e, C, HW, tone, eps, bound, None, dx, work, None)

    assert loss(x=None) == -1 and loss(gt=None) == -1 and loss(work=None) == -1
    assert loss(n_gt=0, e=0) == -1 and loss(b=1, e=1) == -1 and loss(e=4) == -1 and loss(b=-1) == -1
    assert loss(C=0) == -1 and loss(HW=0) == -1
    assert loss(n_gt=K + 10, e=K + 1) == -1
    assert loss(tone=7) == -1
    assert b"tone_mapping" in L.dgs_last_error()
    assert loss(tone=1, bound=0.5) == -1

    skips = (ctypes.c_void_p * 2)(a.value, a.value)
    begins = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def ema(work=a, pos=a, n=n, sk=skips, gb=begins(0, 2, n), n_groups=2, out=a):
        return L.dgs_l2_ema_epoch(work, pos, n, sk, gb, n_groups, out, None)

    assert ema(work=None) == -1 and ema(pos=None) == -1 and ema(out=None) == -1
    assert ema(n=0) == -1 and ema(n=K + 1) == -1
    assert ema(sk=None) == -1 and ema(gb=None) == -1
    assert ema(gb=begins(1, 2, n)) == -1 and ema(gb=begins(0, 2, n - 1)) == -1 and ema(gb=begins(0, 0, n)) == -1
    assert ema(gb=begins(0, n + 1, n)) == -1
    assert b"group_begin" in L.dgs_last_error()
    assert ema(n_groups=n + 1) == -1 and ema(n_groups=-1) == -1


def test_epoch_schedule_rows_against_the_sequential_schedule():
    """epoch_rows on the orders of epoch_orders(5, 4, seed=11), with num_iter_per_view = 40 (StepLR every 2 epochs), 7 steps
    already taken and the first epoch being StepLR epoch 1: pos is the inverse of the order; the scalars of epoch e, step
    j are words [1:5] of row e n + j of the sequential fit's schedule, bit for bit, and equal dgs_adam_scalars called
    directly with that step's count and the rates step_lrs gives its epoch -- which change exactly where step_lrs says."""
    from deblurgs_amd import _lib
    from deblurgs_amd import evaluation as ev
    n, E, t0, num_iter, first = 5, 4, 7, 40, 1
    orders = ev.epoch_orders(n, E, seed=11)
    assert any(o != orders[0] for o in orders)
    rows = ev.epoch_rows(t0, orders, first, num_iter)
    assert rows.shape == (E, 5 * n) and rows.dtype == np.float32
    pos = rows[:, :n].view(np.int32)
    scal = rows[:, n:].reshape(E, n, 4)
    seq = ev.step_rows(t0, orders, first, num_iter)
    assert seq.shape == (E * n, ev.FusedPoseFit.HYPER_WORDS)
    lrs = ev.step_lrs(first + E, num_iter)[first:]
    assert lrs[0] != lrs[1] and lrs[1] == lrs[2] and lrs[2] != lrs[3]      # epochs 1 | 2, 3 | 4: StepLR fires at 2 and 4
    L = _lib.lib()
    groups, tmp = (_lib.DgsAdamGroup * 2)(), (ctypes.c_float * 4)()
    for e in range(E):
        assert sorted(pos[e].tolist()) == list(range(n))
        for j in range(n):
            assert pos[e, orders[e][j]] == j
            assert seq[e * n + j, :1].view(np.int32)[0] == orders[e][j]
            assert scal[e, j].tobytes() == seq[e * n + j, 1:5].tobytes()
            groups[0].lr, groups[1].lr = lrs[e]
            groups[0].step = groups[1].step = t0 + e * n + j + 1
            assert L.dgs_adam_scalars(groups, 2, 0.9, 0.999, tmp) == 0
            assert scal[e, j].tobytes() == np.frombuffer(tmp, dtype=np.float32).tobytes()
        # the rate enters only through -(lr / (1 - beta1^t)): its ratio between the groups is the rates' ratio
        assert scal[e, 0, 2] / scal[e, 0, 0] == pytest.approx(lrs[e][1] / lrs[e][0], rel=1e-6)
    # -lr_rot as every step of the run carries it: constant inside an epoch, changing exactly where step_lrs changes
    stage = np.array([[scal[e, j, 0] * (1.0 - 0.9 ** (t0 + e * n + j + 1)) for j in range(n)] for e in range(E)])
    for e in range(E):
        assert stage[e] == pytest.approx(-lrs[e][0], rel=1e-6)
    assert stage[1, 0] == pytest.approx(stage[0, 0] * 0.9, rel=1e-6) and stage[3, 0] == pytest.approx(stage[2, 0] * 0.9, rel=1e-6)
    with pytest.raises(ValueError):
        ev.epoch_rows(0, [[0, 1, 1]], 0, 40)


def test_optimize_test_pose_refuses_an_unknown_mode():
    from deblurgs_amd import evaluation as ev
    with pytest.raises(ValueError, match="mode"):
        ev.optimize_test_pose(None, [], [], None, "identity", mode="bogus")


def test_epoch_fit_refuses_a_cpu_cloud():
    from deblurgs_amd import evaluation as ev

    class Cloud:
        fused_activations = True
        _xyz = torch.zeros(4, 3)

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.EpochPoseFit(Cloud(), [], [], torch.zeros(3), "identity")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.FusedPoseFit(Cloud(), [], [], torch.zeros(3), "identity")


class _StandInCloud:
    """The attributes of a GaussianCloud that raster_call.cloud_problem reads, as CPU tensors (P = 4)."""

    def __init__(self, n_rest, isotropic):
        g = torch.Generator().manual_seed(3)
        P = 4
        self._xyz = torch.randn(P, 3, generator=g)
        self._features_dc = torch.randn(P, 1, 3, generator=g)
        self._features_rest = torch.randn(P, n_rest, 3, generator=g)
        self._opacity = torch.randn(P, 1, generator=g)
        self._scaling = torch.randn(P, 3, generator=g)
        self._rotation = torch.randn(P, 4, generator=g)
        self.active_sh_degree, self.scale_lower_bound, self.use_isotrophic = 2, 0.003, isotropic
        self.z_near, self.z_far, self.use_sigmoid = 0.2, 100.0, True


@pytest.mark.parametrize("n_rest, isotropic", [(8, True), (0, False)])
def test_cloud_problem_equals_the_spelled_out_problem(n_rest, isotropic):
    """raster_call.cloud_problem against raster_call.problem called with the settings, the raw dict and the fixed
    arguments written out (dgs_context_create allocates nothing on a device, so CPU tensors fill a DgsProblem): the two
    structs byte for byte; a cloud without rest coefficients sends a null shs_rest and M = 1."""
    import math
    from deblurgs_amd import raster_call
    from deblurgs_amd import diff_gaussian_rasterization as dgr
    K, H, W, FoVx, FoVy, cull = 2, 24, 40, 0.9, 0.6, True
    cloud = _StandInCloud(n_rest, isotropic)
    view, full, campos = torch.rand(K, 4, 4), torch.rand(K, 4, 4), torch.rand(K, 3)
    bg = torch.tensor([0.2, 0.3, 0.1])
    geom, image, binning = (torch.zeros(64, dtype=torch.uint8), torch.zeros(96, dtype=torch.uint8),
                            torch.zeros(128, dtype=torch.uint8))
    rs = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(FoVx * 0.5), tanfovy=math.tan(FoVy * 0.5),
        bg=bg, scale_modifier=1.0, z_near=cloud.z_near, z_far=cloud.z_far, use_sigmoid=cloud.use_sigmoid,
        sh_degree=cloud.active_sh_degree, campos=campos, prefiltered=False, debug=False)
    rest = cloud._features_rest if cloud._features_rest.shape[1] > 0 else None
    raw = {"scale_lb": cloud.scale_lower_bound, "sh_rest": rest, "isotropic": getattr(cloud, "use_isotrophic", False)}
    for blob in (None, binning):
        want = raster_call.problem(K, cloud._xyz, cloud._features_dc, None, cloud._opacity, cloud._scaling, cloud._rotation,
                                   None, view, full, campos, rs, bg, cull, 0, raw=raw, geom=geom, image=image, binning=blob)
        got = raster_call.cloud_problem(cloud, K, view, full, campos, H, W, FoVx, FoVy, bg, cull, geom, image, blob)
        assert bytes(got) == bytes(want)
        assert got.P == 4 and got.K == K and got.D == 2 and got.wide_records == 0 and got.geom_state == geom.data_ptr()
        assert got.raw_params == (3 if isotropic else 1) and got.scale_lb == pytest.approx(0.003, rel=1e-6)
        assert got.binning_state == (None if blob is None else binning.data_ptr())
    if n_rest == 0:
        assert not got.shs_rest and got.M == 1
    else:
        assert got.shs_rest == cloud._features_rest.data_ptr() and got.M == 9


def test_round_capacity_on_pinned_values():
    """1/32 of the leading power of two, at least 1024 (by hand: 166384 has 18 bits, q = 8192, 21 q = 172032; 1000000 has
    20 bits, q = 32768, 31 q = 1015808); the fits' capacity for a need of 100000 is round(100000 + 50000 + 16384)."""
    from deblurgs_amd import evaluation as ev, raster_call
    for cap, want in ((1, 1024), (16384, 16384), (166384, 172032), (1000000, 1015808)):
        assert raster_call.round_capacity(cap) == want, cap
    assert ev._capacity_for(100000) == 172032

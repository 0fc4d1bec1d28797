"""GPU tests of the epoch-fused test-view pose fit (evaluation.EpochPoseFit): every new kernel against the single-view /
single-step kernel it batches, bit for bit, and the fit against the sequential FusedPoseFit -- whose distance from the
autograd fit is the only bar a non-zero difference is ever held to."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import GRAD_TOL, _t, relerr, synthetic
from test_evaluation_host import EPS32
from test_gpu_evaluation import _NoHostSync, _fit_fixture, _pose_error

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
BETAS_EPS = (0.9, 0.999, 1e-15)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def fixture3():
    """test_gpu_evaluation._fit_fixture(): 3000 Gaussians, 144 x 96, 3 views; built once, never modified."""
    return _fit_fixture()


@functools.lru_cache(maxsize=None)
def fixture5(P=3000, W=144, H=96, seed=3, n=5):
    """The same construction with five views (make_scene(..., K=5))."""
    import torch
    from scipy.spatial.transform import Rotation
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses
    from deblurgs_amd.cloud import GaussianCloud
    torch.manual_seed(seed)
    sc = synthetic.make_scene(P, W, H, K=n, seed=seed, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    tm = losses.ToneMapping("gamma")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    cam = lambda R, T: ev.TestCamera(R, T, sc["FoVx"], sc["FoVy"], W, H)
    truth = ev.TestPoseModel([cam(V[i][:3, :3], V[i][3, :3]) for i in range(n)], device="cuda")
    with torch.no_grad():
        gts = torch.stack([tm(gaussian_renderer.render(truth(i), cloud, bg)["render"]).clamp(0.0, 1.0) for i in range(n)])
    dR = Rotation.from_rotvec(np.deg2rad(0.4) * np.array([0.6, -0.64, 0.48])).as_matrix()
    dT = np.array([0.03, -0.02, 0.04])
    start = [cam(V[i][:3, :3] @ dR, V[i][3, :3] + dT) for i in range(n)]
    return cloud, start, gts, bg, tm, truth


# ------------------------------------------------------------------------------------------------ epoch Adam
def _decades(rng, shape, lo, hi, zero_every=0):
    a = rng.normal(size=shape) * 10.0 ** rng.uniform(lo, hi, size=shape)
    if zero_every:
        a.reshape(-1)[::zero_every] = 0.0
    return a.astype(np.float32)


class _AdamCase:
    """Random [n,4] / [n,3] parameters, moments and gradients over many decades (second moments down to 1e-32, so that
    sqrt(v) / bc2 sits below, at and above eps = 1e-15; some moments and gradients exactly zero), a random permutation
    pos, t0 = 37 steps already taken and the rates of the 3rd StepLR stage."""

    def __init__(self, n, seed):
        import torch
        from deblurgs_amd import _lib
        from deblurgs_amd import evaluation as ev
        self.n, self.t0 = n, 37
        rng = np.random.default_rng(seed)
        self.widths = (4, 3)
        self.p0 = [_decades(rng, (n, w), -3, 1) for w in self.widths]
        self.m0 = [_decades(rng, (n, w), -12, -2, zero_every=7) for w in self.widths]
        self.v0 = [np.square(_decades(rng, (n, w), -16, -2, zero_every=5)) for w in self.widths]
        self.g = [_decades(rng, (n, w), -9, 0, zero_every=11) for w in self.widths]
        self.order = rng.permutation(n)
        self.pos = np.empty(n, dtype=np.int32)
        self.pos[self.order] = np.arange(n, dtype=np.int32)
        lrs = (ev.ROT_LR * ev.LR_GAMMA * ev.LR_GAMMA, ev.TRANS_LR * ev.LR_GAMMA * ev.LR_GAMMA)
        L = _lib.lib()
        groups, tmp = (_lib.DgsAdamGroup * 2)(), (ctypes.c_float * 4)()
        self.scalars = np.zeros((n, 4), dtype=np.float32)
        for j in range(n):
            for i in range(2):
                groups[i].lr, groups[i].step = lrs[i], self.t0 + j + 1
            _lib.check(L.dgs_adam_scalars(groups, 2, 0.9, 0.999, tmp), "dgs_adam_scalars")
            self.scalars[j] = np.frombuffer(tmp, dtype=np.float32)
        self.pos_dev = torch.from_numpy(self.pos).cuda()
        self.scal_dev = torch.from_numpy(self.scalars).cuda()
        self.g_dev = [_t(a) for a in self.g]

    def state(self):
        return [_t(a.copy()) for a in self.p0], [_t(a.copy()) for a in self.m0], [_t(a.copy()) for a in self.v0]

    @staticmethod
    def groups(p, g, m, v):
        from deblurgs_amd import _lib
        return (_lib.DgsAdamGroup * 2)(*[_lib.DgsAdamGroup(p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(),
                                                           p[i].numel(), 1.0, 1) for i in range(2)])

    def reference(self):
        """n launches of dgs_adam_step_dev on a dense gradient that is zero except for row order[j] at step j.  Returns
        the final (p, m, v) and, per row, the parameter just before the row's own step."""
        import torch
        from deblurgs_amd import _lib
        L = _lib.lib()
        p, m, v = self.state()
        dense = [torch.zeros_like(x) for x in p]
        before = [torch.zeros_like(x) for x in p]
        groups = self.groups(p, dense, m, v)
        for j in range(self.n):
            r = int(self.order[j])
            for i in range(2):
                dense[i].zero_()
                dense[i][r] = self.g_dev[i][r]
                before[i][r] = p[i][r]
            _lib.check(L.dgs_adam_step_dev(groups, 2, *BETAS_EPS, 0.0, None, self.scal_dev[j].data_ptr(), _stream()),
                       "dgs_adam_step_dev")
        torch.cuda.synchronize()
        return p, m, v, before

    def step(self, p, m, v, ranges, skip=None, pos=None):
        from deblurgs_amd import _lib
        groups = self.groups(p, self.g_dev, m, v)
        for b, e in ranges:
            _lib.check(_lib.lib().dgs_adam_epoch_step(groups, 2, self.n, b, e, (self.pos_dev if pos is None else pos).data_ptr(),
                                                      self.scal_dev.data_ptr(), self.n, *BETAS_EPS,
                                                      None if skip is None else skip.data_ptr(), _stream()), "dgs_adam_epoch_step")

    def peek(self, p, m, v, ranges):
        import torch
        from deblurgs_amd import _lib
        out = [torch.full_like(x, SENTINEL) for x in p]
        outs = (ctypes.c_void_p * 2)(out[0].data_ptr(), out[1].data_ptr())
        groups = self.groups(p, self.g_dev, m, v)
        for b, e in ranges:
            _lib.check(_lib.lib().dgs_adam_epoch_peek(groups, 2, outs, self.n, b, e, self.pos_dev.data_ptr(),
                                                      self.scal_dev.data_ptr(), self.n, *BETAS_EPS, _stream()), "dgs_adam_epoch_peek")
        return out


def _same(a, b):
    return all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [1, 5, 128])
def test_epoch_adam_equals_n_launches_of_the_sequential_kernel(gpu, n):
    import torch
    case = _AdamCase(n, seed=100 + n)
    p_ref, m_ref, v_ref, before = case.reference()
    # the denominators really straddle eps: sqrt(v) / bc2 below 1e-15 somewhere, above elsewhere
    root = np.sqrt(np.concatenate([a.reshape(-1) for a in case.v0]).astype(np.float64))
    if n == 128:
        assert (root < 1e-15).any() and (root > 1e-13).any() and (root == 0).any()
    p, m, v = case.state()
    peeked = case.peek(p, m, v, [(0, n)])
    torch.cuda.synchronize()
    assert _same(p, [_t(a) for a in case.p0]) and _same(m, [_t(a) for a in case.m0]) and _same(v, [_t(a) for a in case.v0]), \
        "the peek changed the state"
    assert _same(peeked, before), "peek != the sequential parameter just before the row's step"
    case.step(p, m, v, [(0, n)])
    torch.cuda.synchronize()
    assert _same(p, p_ref), "parameters"
    assert _same(m, m_ref), "exp_avg"
    assert _same(v, v_ref), "exp_avg_sq"
    if n > 1:       # rows that waited moved by their momentum: the peek is not the start value everywhere
        assert not _same(peeked, [_t(a) for a in case.p0])
    # skip_flag = 1: nothing is written
    p2, m2, v2 = case.state()
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    case.step(p2, m2, v2, [(0, n)], skip=skip)
    torch.cuda.synchronize()
    assert _same(p2, [_t(a) for a in case.p0]) and _same(m2, [_t(a) for a in case.m0]) and _same(v2, [_t(a) for a in case.v0])
    skip.zero_()
    case.step(p2, m2, v2, [(0, n)], skip=skip)
    torch.cuda.synchronize()
    assert _same(p2, p_ref) and _same(m2, m_ref) and _same(v2, v_ref)


def test_epoch_adam_row_ranges_and_corrupt_positions(gpu):
    """[0,2) + [2,5) = [0,5) for the step and the peek; a range leaves the other rows alone; a pos outside [0, n_steps)
    counts as 0."""
    import torch
    n = 5
    case = _AdamCase(n, seed=105)
    p_ref, m_ref, v_ref, before = case.reference()
    p, m, v = case.state()
    peeked = case.peek(p, m, v, [(0, 2), (2, 5)])
    part = case.peek(p, m, v, [(1, 4)])
    case.step(p, m, v, [(0, 2)])
    torch.cuda.synchronize()
    for x, x0 in zip(p + m + v, case.p0 + case.m0 + case.v0):
        assert np.array_equal(x[2:].cpu().numpy(), x0[2:]), "rows outside the range were written"
    case.step(p, m, v, [(2, 5)])
    torch.cuda.synchronize()
    assert _same(peeked, before) and _same(p, p_ref) and _same(m, m_ref) and _same(v, v_ref)
    for x, y in zip(part, before):
        assert np.array_equal(x[1:4].cpu().numpy(), y[1:4].cpu().numpy())
        assert bool((x[0] == SENTINEL).all()) and bool((x[4] == SENTINEL).all())
    # corrupt positions: row 1 -> 99, row 3 -> -4 behave as position 0 (and nothing faults)
    bad = case.pos.copy()
    bad[1], bad[3] = 99, -4
    zero = case.pos.copy()
    zero[1], zero[3] = 0, 0
    res = []
    for pos in (bad, zero):
        q, qm, qv = case.state()
        case.step(q, qm, qv, [(0, n)], pos=torch.from_numpy(pos).cuda())
        torch.cuda.synchronize()
        res.append(q + qm + qv)
    assert _same(res[0], res[1])


# ------------------------------------------------------------------------------------------------ pose chain
def test_batched_pose_chain_equals_the_single_view_kernels(gpu):
    import torch
    from deblurgs_amd import _lib, pose
    L = _lib.lib()
    n = 5
    rng = np.random.default_rng(8)
    q = (rng.normal(size=(n, 4)) * np.array([[0.3], [1.0], [2.5], [1.0], [0.05]])).astype(np.float32)   # NOT normalised
    q[3] = -1.3 * q[1] + np.array([1e-6, -2e-6, 0.0, 1e-6], dtype=np.float32)                          # nearly antipodal to row 1
    t = rng.normal(0.0, 2.0, (n, 3)).astype(np.float32)
    rot, trans = _t(q), _t(t)
    proj = pose.get_projection_matrix(znear=0.01, zfar=100.0, fovX=0.9, fovY=0.7).transpose(0, 1).contiguous().float().cuda()
    dv, df = _t(rng.normal(size=(n, 4, 4)).astype(np.float32)), _t(rng.normal(size=(n, 4, 4)).astype(np.float32))
    f = dict(dtype=torch.float32, device="cuda")
    single = []
    for r in range(n):
        view, full, cam = torch.empty((4, 4), **f), torch.empty((4, 4), **f), torch.empty(3, **f)
        g_rot, g_trans = torch.empty((n, 4), **f), torch.empty((n, 3), **f)
        _lib.check(L.dgs_testpose_forward(rot.data_ptr(), trans.data_ptr(), None, r, n, proj.data_ptr(), view.data_ptr(),
                                          full.data_ptr(), cam.data_ptr(), _stream()), "dgs_testpose_forward")
        _lib.check(L.dgs_testpose_backward(rot.data_ptr(), trans.data_ptr(), None, r, n, proj.data_ptr(), dv[r].data_ptr(),
                                           df[r].data_ptr(), g_rot.data_ptr(), g_trans.data_ptr(), _stream()),
                   "dgs_testpose_backward")
        torch.cuda.synchronize()
        single.append([x.cpu().numpy() for x in (view, full, cam, g_rot[r], g_trans[r])])
        assert np.abs(single[-1][3]).max() > 0 and np.abs(single[-1][4]).max() > 0
    for b, e in ((0, n), (1, 4)):
        G = e - b
        view, full, cam = torch.full((G, 4, 4), SENTINEL, **f), torch.full((G, 4, 4), SENTINEL, **f), torch.full((G, 3), SENTINEL, **f)
        g_rot, g_trans = torch.full((n, 4), SENTINEL, **f), torch.full((n, 3), SENTINEL, **f)
        _lib.check(L.dgs_testpose_forward_rows(rot.data_ptr(), trans.data_ptr(), n, b, e, proj.data_ptr(), view.data_ptr(),
                                               full.data_ptr(), cam.data_ptr(), _stream()), "dgs_testpose_forward_rows")
        dvr, dfr = dv[b:e].contiguous(), df[b:e].contiguous()
        _lib.check(L.dgs_testpose_backward_rows(rot.data_ptr(), trans.data_ptr(), n, b, e, proj.data_ptr(), dvr.data_ptr(),
                                                dfr.data_ptr(), g_rot.data_ptr(), g_trans.data_ptr(), _stream()),
                   "dgs_testpose_backward_rows")
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in (view, full, cam)]
        gr, gt = g_rot.cpu().numpy(), g_trans.cpu().numpy()
        for r in range(n):
            if b <= r < e:
                for name, a, w in zip(("view", "full", "campos"), got, single[r][:3]):
                    assert np.array_equal(a[r - b], w), (name, r, (b, e))
                assert np.array_equal(gr[r], single[r][3]), ("dL_drot", r, (b, e))
                assert np.array_equal(gt[r], single[r][4]), ("dL_dtrans", r, (b, e))
            else:
                assert (gr[r] == SENTINEL).all() and (gt[r] == SENTINEL).all(), "rows outside the range were written"


# ------------------------------------------------------------------------------------------------ view loss
@pytest.mark.parametrize("kind,bound", [("identity", 0.0), ("gamma", 0.125)])
@pytest.mark.parametrize("H,W", [(7, 9), (20, 24), (300, 300)])
def test_batched_view_loss_equals_the_single_image_kernel(gpu, H, W, kind, bound):
    """Three images in one launch against three dgs_view_loss_grad calls: the one-block, many-block and capped-grid sizes
    of the existing totals test; the images are compared against rows [1, 4) of a stack of four."""
    import torch
    from deblurgs_amd import _lib
    L = _lib.lib()
    G, E = 3, 3 * H * W
    rng = np.random.default_rng(H * 1000 + W)
    x = rng.uniform(-0.2, 1.3, (G, 3, H, W)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (G + 1, 3, H, W)).astype(np.float32)
    span = 1.0 - 2.0 * bound
    for k in range(G):          # on and around 0, 1, eps and the bound (in x, and where the tone-mapped operand is eps)
        edge = [0.0, 1.0, EPS32, EPS32 / 2, -EPS32, bound, bound + EPS32 * span, bound + 2 * EPS32 * span, bound - 1e-3,
                1.0 - bound, 1.0 - bound + 1e-3, -0.5, 2.0, np.nextafter(np.float32(1.0), np.float32(0.0))]
        x[k].reshape(-1)[k:k + len(edge)] = edge
        gt[k + 1].reshape(-1)[40:60] = np.clip(x[k].reshape(-1)[40:60], 0.0, 1.0)
    tone = _lib.TONE_GAMMA if kind == "gamma" else _lib.TONE_IDENTITY
    gts = _t(gt)

    def single(xs, k):
        idx = torch.tensor([k + 1], dtype=torch.int32, device="cuda")
        dx, work = torch.full((3, H, W), SENTINEL, device="cuda"), torch.full((12,), 7.0, device="cuda")
        _lib.check(L.dgs_view_loss_grad(xs[k].data_ptr(), gts.data_ptr(), idx.data_ptr(), G + 1, 3, H * W, tone, EPS32, bound,
                                        None, dx.data_ptr(), work.data_ptr(), None, None, _stream()), "dgs_view_loss_grad")
        torch.cuda.synchronize()
        return work.cpu().numpy(), dx.cpu().numpy()

    def batched(xs):
        dx, work = torch.full((G, 3, H, W), SENTINEL, device="cuda"), torch.full((G, 12), 7.0, device="cuda")
        _lib.check(L.dgs_view_loss_grad_rows(xs.data_ptr(), gts.data_ptr(), G + 1, 1, G + 1, 3, H * W, tone, EPS32, bound, None,
                                             dx.data_ptr(), work.data_ptr(), _stream()), "dgs_view_loss_grad_rows")
        torch.cuda.synchronize()
        return work.cpu().numpy(), dx.cpu().numpy()

    xs = _t(x)
    work, dx = batched(xs)
    first = []
    for k in range(G):
        w1, d1 = single(xs, k)
        first.append(w1)
        assert np.isfinite(w1[:2]).all() and w1[0] > 0 and np.count_nonzero(d1) > 0.3 * E
        assert np.array_equal(work[k, 0:2], w1[0:2]), (k, work[k, 0:2], w1[0:2])
        assert work[k, 8:12].tobytes() == w1[8:12].tobytes(), k
        assert np.array_equal(dx[k], d1), k
    assert not np.array_equal(work[0, 0:2], work[1, 0:2])
    # a NaN in image 1 reaches image 1's values only
    xs[1].view(-1)[E // 2] = float("nan")
    work_n, dx_n = batched(xs)
    assert np.isnan(work_n[1, 0:2]).all() and np.isnan(work_n[1, 8:12].view(np.float64)).all()
    w1, _ = single(xs, 1)
    assert np.isnan(w1[0:2]).all()
    for k in (0, 2):
        assert np.array_equal(work_n[k, 0:2], first[k][0:2]) and work_n[k, 8:12].tobytes() == first[k][8:12].tobytes()
        assert np.array_equal(dx_n[k], dx[k])


def test_l2_ema_over_an_epoch_follows_the_order_and_the_skip_words(gpu):
    """ema = ema * 0.6f + (float) mse_j * 0.4f in the order of the turns; the rows of a group whose skip word is set, and
    rows with a corrupt position, do not count."""
    import torch
    from deblurgs_amd import _lib
    L = _lib.lib()
    n = 5
    rng = np.random.default_rng(4)
    work = np.full((n, 12), 7.0, dtype=np.float32)
    work[:, 1] = rng.uniform(0.001, 0.2, n).astype(np.float32)
    order = [3, 0, 4, 1, 2]
    pos = np.empty(n, dtype=np.int32)
    pos[order] = np.arange(n)
    skips = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * 3)(*[skips.data_ptr() + 4 * i for i in range(3)])
    begins = (ctypes.c_int32 * 4)(0, 2, 4, 5)

    work_dev = _t(work)

    def run(pos, n_groups):
        ema, pos_dev = torch.tensor([0.5], device="cuda"), torch.from_numpy(pos).cuda()
        _lib.check(L.dgs_l2_ema_epoch(work_dev.data_ptr(), pos_dev.data_ptr(), n, ptrs, begins, n_groups, ema.data_ptr(),
                                      _stream()), "dgs_l2_ema_epoch")
        torch.cuda.synchronize()
        return np.float32(ema.item())

    def want(rows):
        e = np.float32(0.5)
        for r in rows:
            e = np.float32(np.float32(e * np.float32(0.6)) + np.float32(work[r, 1] * np.float32(0.4)))
        return e

    assert run(pos, 0) == want(order)
    assert want(order) != want(sorted(order))                       # (the order matters on these values)
    assert run(pos, 3) == want([r for r in order if r not in (2, 3)])   # group 1 = rows [2, 4) is skipped
    bad = pos.copy()
    bad[4] = 77
    assert run(bad, 0) == want([r for r in order if r != 4])


# ------------------------------------------------------------------------------------------------ the fit
def test_epoch_fit_first_epoch_gradients_equal_the_sequential_fit_and_match_autograd(gpu):
    """At epoch 0 the moments are zero, so every view's turn-time pose is its start pose: the K = 3 call's rendered
    colours, losses and pose gradients against three K = 1 steps of FusedPoseFit (bit for bit), and against autograd."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer
    cloud, start, gts, bg, tm, _ = fixture3()
    epoch = ev.EpochPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=60)
    assert len(epoch.groups) == 1 and epoch.groups[0].G == 3
    g_rot, g_trans, vals = epoch.gradients()
    colors = epoch.groups[0].color.clone()
    torch.cuda.synchronize()
    seq = ev.FusedPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=60)
    ref = ev.TestPoseModel(start, device="cuda")
    for idx in range(3):
        s_rot, s_trans, s_vals = seq.gradients(idx)
        torch.cuda.synchronize()
        assert torch.equal(seq.color[0], colors[idx]), f"slot {idx} of the K = 3 render differs from the K = 1 render"
        assert np.array_equal(vals[idx].cpu().numpy(), s_vals.cpu().numpy()), (idx, vals[idx], s_vals)
        for name, a, b in (("dL/dq", g_rot[idx], s_rot[idx]), ("dL/dt", g_trans[idx], s_trans[idx])):
            print(f"view {idx} {name}: epoch {a.cpu().numpy()} sequential {b.cpu().numpy()}")
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (idx, name)
        for p in ref.parameters():
            p.grad = None
        image = gaussian_renderer.render(ref(idx), cloud, bg)["render"]
        l1, mse = ev.view_loss(image, gts[idx], tm)
        l1.backward()
        torch.cuda.synchronize()
        for name, a, b in (("dL/dq", g_rot[idx], ref._rot.grad[idx]), ("dL/dt", g_trans[idx], ref._trans.grad[idx])):
            e = relerr(a.cpu().numpy(), b.cpu().numpy())
            print(f"view {idx} {name}: rel err vs autograd {e:.3e}")
            assert e <= GRAD_TOL, (idx, name, e)
        assert abs(float(vals[idx, 0]) - float(l1.detach())) <= 1e-6 and abs(float(vals[idx, 1]) - float(mse.detach())) <= 1e-6
    for p in cloud.parameters():
        p.grad = None


def _distances(model_a, l1_a, model_b, l1_b, err_a, err_b):
    return {"final mean L1": abs(l1_a - l1_b), "pose error": abs(err_a - err_b),
            "max |rot|": float((model_a._rot.detach() - model_b._rot.detach()).abs().max()),
            "max |trans|": float((model_a._trans.detach() - model_b._trans.detach()).abs().max())}


def test_epoch_fit_equals_the_sequential_fit_over_a_whole_run(gpu):
    """S = 60 epochs, fixed order, num_iter_per_view = S: the epoch fit's distance from the sequential fit in the
    final-epoch mean L1, the pose error and the parameters must not exceed the sequential fit's distance from the
    autograd fit (zero when the gradients are bit-equal); no drops, S n steps, the same PSNR EMA, no host sync."""
    import torch
    from autograd_pose_fit import AutogradPoseFit
    from deblurgs_amd import evaluation as ev
    S, n = 60, 3
    cloud, start, gts, bg, tm, truth = fixture3()
    orders = ev.epoch_orders(n, S, order=[2, 0, 1])
    auto = AutogradPoseFit(cloud, start, list(gts), bg, tm, num_iter_per_view=S)
    l1_auto = 0.0
    for order in orders:
        l1_auto = float(np.mean([float(auto.step(i)) for i in order]))
        auto.scheduler.step()
    for p in cloud.parameters():
        p.grad = None
    seq = ev.FusedPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=S)
    seq.schedule(orders)
    seq.run(S * n - n)
    last = torch.zeros(n, device="cuda")
    for i in range(n):
        seq.run(1)
        last[i:i + 1].copy_(seq.work[:1], non_blocking=True)
    torch.cuda.synchronize()
    l1_seq = float(last.cpu().numpy().astype(np.float64).mean())
    epoch = ev.EpochPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=S)
    assert epoch.schedule(orders) == S
    torch.cuda.synchronize()
    with _NoHostSync():
        assert epoch.run() == S
    torch.cuda.synchronize()
    assert epoch.dropped() == 0 and seq.dropped() == 0 and epoch.steps == S * n == seq.steps
    l1_epoch = float(epoch.work[:, 0].cpu().numpy().astype(np.float64).mean())
    errs = {k: _pose_error(m, truth, cloud) for k, m in (("auto", auto.model), ("seq", seq.model), ("epoch", epoch.model))}
    bar = _distances(seq.model, l1_seq, auto.model, l1_auto, errs["seq"], errs["auto"])
    got = _distances(epoch.model, l1_epoch, seq.model, l1_seq, errs["epoch"], errs["seq"])
    for k in bar:
        print(f"{k}: |epoch - sequential| {got[k]:.3e}   bar |sequential - autograd| {bar[k]:.3e}")
    print(f"final mean L1: autograd {l1_auto:.6e} sequential {l1_seq:.6e} epoch {l1_epoch:.6e}; pose errors {errs}")
    for k in bar:
        assert got[k] <= bar[k], (k, got[k], bar[k])
    assert epoch.psnr_ema() == pytest.approx(seq.psnr_ema(), rel=1e-6)
    assert 0.0 < epoch.psnr_ema() < 100.0
    assert float(epoch.exp_avg_sq[0].abs().min()) > 0.0


def test_epoch_fit_in_groups_equals_one_call(gpu):
    """Five views, S = 12 epochs of shuffled orders (the positions differ per epoch): views_per_call = 2 (groups of 2, 2
    and 1 rows, three chains per epoch) against one K = 5 call -- parameters, moments and l2_ema bit for bit; both end
    closer to the true poses than they started."""
    import torch
    from deblurgs_amd import evaluation as ev
    S, n = 12, 5
    cloud, start, gts, bg, tm, truth = fixture5()
    orders = ev.epoch_orders(n, S, seed=7)
    assert len({tuple(o) for o in orders}) > 1
    fits = []
    for per_call in (None, 2):
        fit = ev.EpochPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=S, views_per_call=per_call)
        err0 = _pose_error(fit.model, truth, cloud)
        fit.schedule(orders)
        fit.run()
        torch.cuda.synchronize()
        assert fit.dropped() == 0 and fit.steps == S * n
        err = _pose_error(fit.model, truth, cloud)
        print(f"views_per_call {per_call}: groups {[(g.begin, g.end) for g in fit.groups]} pose error {err0} -> {err}")
        assert err < err0
        fits.append(fit)
    one, grouped = fits
    assert [(g.begin, g.end) for g in one.groups] == [(0, 5)]
    assert [(g.begin, g.end) for g in grouped.groups] == [(0, 2), (2, 4), (4, 5)]
    for name, a, b in [("rot", one.model._rot, grouped.model._rot), ("trans", one.model._trans, grouped.model._trans),
                       ("exp_avg rot", one.exp_avg[0], grouped.exp_avg[0]), ("exp_avg trans", one.exp_avg[1], grouped.exp_avg[1]),
                       ("exp_avg_sq rot", one.exp_avg_sq[0], grouped.exp_avg_sq[0]),
                       ("exp_avg_sq trans", one.exp_avg_sq[1], grouped.exp_avg_sq[1]), ("l2_ema", one.l2_ema, grouped.l2_ema)]:
        d = float((a.detach() - b.detach()).abs().max())
        print(f"{name}: max |one call - groups| {d:.3e}")
        assert torch.equal(a.detach(), b.detach()), name
    assert float(one.l2_ema) > 0.0


def test_epoch_fit_drops_the_whole_epoch_of_a_group_that_overflows(gpu):
    """A capacity below what the start poses need: the forward sets its overflow word, the epoch's step and EMA are
    skipped on the device -- parameters, moments and l2_ema unchanged, dropped() == n -- and optimize_test_pose raises."""
    import torch
    from deblurgs_amd import evaluation as ev
    cloud, start, gts, bg, tm, _ = fixture3()
    need = ev.EpochPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=60).capacity
    small = max((need - 16384) // 4, 256)           # a good third of the count the start poses need
    fit = ev.EpochPoseFit(cloud, start, gts, bg, tm, num_iter_per_view=60, capacity=small)
    rot0, trans0 = fit.model._rot.detach().clone(), fit.model._trans.detach().clone()
    fit.schedule([[2, 0, 1]])
    fit.run()
    torch.cuda.synchronize()
    assert fit.dropped() == 3 and fit.steps == 3
    assert torch.equal(fit.model._rot.detach(), rot0) and torch.equal(fit.model._trans.detach(), trans0)
    for t in fit.exp_avg + fit.exp_avg_sq + [fit.l2_ema]:
        assert float(t.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="exceeded the duplicate capacity"):
        ev.optimize_test_pose(cloud, start, gts, bg, tm, num_iter_per_view=2, order=[0, 1, 2], mode="epoch", capacity=small)


def test_optimize_test_pose_in_epoch_mode_improves_the_evaluation(gpu):
    import torch
    from deblurgs_amd import evaluation as ev
    cloud, start, gts, bg, tm, _ = fixture3()
    cams = ev.optimize_test_pose(cloud, start, gts, bg, tm, num_iter_per_view=20, order=[0, 1, 2], mode="epoch")
    assert len(cams) == 3 and not cams[0].world_view_transform.requires_grad
    psnr, ssim = ev.evaluate(cams, cloud, bg, gts, tm)
    with torch.no_grad():
        m0 = ev.TestPoseModel(start, device="cuda")
        p0, s0 = ev.evaluate([m0(i) for i in range(3)], cloud, bg, gts, tm)
    print(f"evaluate: epoch-mode fit {psnr:.3f} dB / {ssim:.5f}, start poses {p0:.3f} dB / {s0:.5f}")
    assert psnr > p0

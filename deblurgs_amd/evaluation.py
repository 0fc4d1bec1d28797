"""The reference's evaluation protocol (test.py): the learned trajectories make a dataset's test poses invalid, so every
number the reference reports comes from

    optimize_test_pose   test.py:131-186   an iNeRF-style fit of the test cameras to the trained cloud: per step one
                                           render, a tone-mapped and clamped L1 against the test image, a backward into the
                                           CAMERA only, one Adam step on a quaternion and a translation
    evaluate             test.py:93-129    PSNR / SSIM (/ LPIPS) of the renders at the fitted cameras

`TestPoseModel` is OptimPoseModel (test.py:39-91).  Both fits share `_PoseFit` (checks, ground truth, Adam's state, capture
and replay) and hold the state of a rasteriser call in a `_RasterCall`.  `FusedPoseFit` is one step of the fit enqueued
straight through the C ABI and replayed as ONE captured hipGraph -- no autograd, no host read:

    quaternion + translation of the drawn view -> camera     dgs_testpose_forward   (view index from device memory)
    K = 1 rasterisation of the cloud's raw parameters        dgs_forward            (capacity sized ahead)
    clamp(tone_map(render), 0, 1), L1, MSE, dL/drender       dgs_view_loss_grad
    dL/d{world_view, full_proj}, nothing else                dgs_backward_pose_only
    -> dL/dquaternion, dL/dtranslation (dense [n,4], [n,3])  dgs_testpose_backward
    Adam on the two tensors                                  dgs_adam_step_dev      (step sizes from device memory)

The graph is a linear chain (the pose-only backward never forks).  What changes between steps -- the view index and Adam's
bias-corrected step sizes, which carry the StepLR stage -- is read from an 8-word device block that a one-launch copy
refreshes from the run's schedule before every replay, so one capture serves every view and every learning-rate stage.

Semantics are the reference's: Adam (rates 5e-5 / 5e-4, eps 1e-15) runs over the WHOLE [n,4] and [n,3] tensors every step
(rows with zero gradient still move by their momentum, as torch's dense Adam moves them), StepLR(num_iter // 20, 0.9)
advances once per epoch, an epoch visits every view once in shuffled order.

`EpochPoseFit` (opt-in: optimize_test_pose(mode="epoch")) runs the same fit with ONE launch chain per epoch and group of
`views_per_call` rows (default: all n views in one K = n call).  No update changes: Adam is elementwise, and row i of
`_rot` / `_trans` gets a non-zero gradient only at view i's turn, from row i alone; so a row at position p of the epoch's
order sees p zero-gradient steps (it still moves by its momentum), one real step at the parameters it has THEN, and
n - 1 - p more zero-gradient steps, each with that global step's bias corrections.  The chain of a group of rows is

    parameters of every row at ITS turn (p_i zero-gradient steps)   dgs_adam_epoch_peek
    -> the G cameras                                                dgs_testpose_forward_rows
    K = G rasterisation                                             dgs_forward            (capacity sized ahead)
    the G losses and dL/drender                                     dgs_view_loss_grad_rows
    dL/d{world_view, full_proj} [G,4,4]                             dgs_backward_pose_only
    -> rows of dL/dquaternion, dL/dtranslation                      dgs_testpose_backward_rows
    the epoch's n Adam steps of those rows                          dgs_adam_epoch_step
    (after the last group) l2_error_ema in the order of the turns   dgs_l2_ema_epoch

One difference from the sequential fit: there a forward that overflows its capacity skips ONE step; here it skips the whole
epoch of its group's rows (all n steps of those rows, zero-gradient ones included) -- dropped() counts the view-steps.

LPIPS, the third number, needs network weights that are not part of this package: `evaluate(..., lpips=weights)` with a
caller's lpips.LPIPSWeights (or LPIPSVggWeights, LPIPSSqueezeWeights) returns (psnr, ssim, lpips) (dgs_lpips_alex / _vgg / _squeeze on the device); without it, (psnr, ssim).
`initialize_test_pose` (test.py:188-398) gives unposed test images their starting poses.  The reference registers them with a
COLMAP binary; here it is coarse photometric registration against the trained cloud (registration.py) -- a different method.
The dataset readers are out of scope.
"""
import ctypes
import math
import random

import numpy as np
import torch
import torch.nn as nn

from . import _lib, gaussian_renderer, losses, metrics, pose, raster_call
from . import diff_gaussian_rasterization as dgr
from .raster_call import _ptr, _stream

ROT_LR, TRANS_LR, ADAM_EPS = 5e-5, 5e-4, 1e-15      # test.py:146-149
LR_STAGES, LR_GAMMA = 20, 0.9                        # test.py:151


class TestCamera:
    """The attributes of the reference's Camera that the evaluation reads (scene/cameras.py): R [3,3] (stored as the
    camera-to-world rotation, as the reference's loaders store it) and T [3] of the world-to-view transform, the
    intrinsics, and the test image."""
    __test__ = False      # (not a pytest class)

    def __init__(self, R, T, FoVx, FoVy, image_width, image_height, original_image=None, znear=0.01, zfar=100.0):
        self.R, self.T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)
        self.FoVx, self.FoVy = float(FoVx), float(FoVy)
        self.image_width, self.image_height = int(image_width), int(image_height)
        self.znear, self.zfar = float(znear), float(zfar)
        self.original_image = original_image


def _as_tensor(a):
    return a.detach().double().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float64))


class TestPoseModel(nn.Module):
    """OptimPoseModel (test.py:39-91): `_rot` [n,4] unit quaternions in (x, y, z, w) order from the cameras' rotations
    (pose.rotmat_to_unitquat: the algorithm roma documents for rotmat_to_unitquat, pinned against scipy -- unpinned
    against roma itself, which is not available here), `_trans` [n,3] their translations.  forward(idx) is the torch
    expression of the pose chain (differentiable; what the autograd path of the fit runs); FusedPoseFit evaluates the
    same chain with dgs_testpose_forward / _backward."""
    __test__ = False

    def __init__(self, cams, device=None):
        super().__init__()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.cams = list(cams)
        rots = torch.stack([_as_tensor(c.R) for c in self.cams])
        transes = torch.stack([_as_tensor(c.T) for c in self.cams])
        self._rot = nn.Parameter(pose.rotmat_to_unitquat(rots).float().to(device).contiguous())
        self._trans = nn.Parameter(transes.float().to(device).contiguous())
        self._proj = {}

    def __len__(self):
        return len(self.cams)

    def projection_matrix(self, idx):
        """The transposed projection matrix of view idx on the model's device (test.py:87), cached per intrinsics."""
        c = self.cams[idx]
        key = (c.znear, c.zfar, c.FoVx, c.FoVy)
        if key not in self._proj:
            self._proj[key] = pose.get_projection_matrix(znear=c.znear, zfar=c.zfar, fovX=c.FoVx, fovY=c.FoVy) \
                .transpose(0, 1).contiguous().to(self._rot.device)
        return self._proj[key]

    def forward(self, idx):
        """A camera carrying the four tensors render() reads (world_view_transform, full_proj_transform, camera_center,
        and projection_matrix) plus the intrinsics and the test image of view idx."""
        c = self.cams[idx]
        quat = self._rot[idx] + 1e-8
        unit = quat / quat.norm()
        R = pose.unitquat_to_rotmat(unit[None])[0]
        trans = self._trans[idx]
        # world_view[:3,:3] = (R^T)^T, world_view[3,:3] = trans: test.py:82-85 after its final transpose
        top = torch.cat([R, R.new_zeros(3, 1)], dim=1)
        bottom = torch.cat([trans, trans.new_ones(1)])[None]
        wv = torch.cat([top, bottom], dim=0)
        proj = self.projection_matrix(idx).to(wv.dtype)
        cam = pose.MiniCam(c.image_width, c.image_height, c.FoVy, c.FoVx, c.znear, c.zfar, wv, wv @ proj,
                           camera_center=-(trans @ R.transpose(0, 1)))       # = inverse(world_view)[3,:3]
        cam.projection_matrix = proj
        cam.original_image = getattr(c, "original_image", None)
        return cam


def view_loss(image, gt, tone_mapping):
    """The fit's loss in torch (test.py:171-172): L1 of clamp(tone_map(image), 0, 1) against gt.  Returns (l1, mse)."""
    y = tone_mapping(image).clamp(0.0, 1.0)
    return losses.l1_loss(y, gt), ((gt - y) ** 2).mean()


def _tone_args(tone_mapping):
    if tone_mapping is None or isinstance(tone_mapping, str):
        tone_mapping = losses.ToneMapping(tone_mapping or "identity")
    kind = tone_mapping.tone_mapping_type
    if kind in ("identity", "reverse_identity"):
        return tone_mapping, _lib.TONE_IDENTITY, 0.0, 0.0
    if kind == "gamma":
        return tone_mapping, _lib.TONE_GAMMA, float(tone_mapping.eps), float(tone_mapping.bound)
    raise NotImplementedError(f"FusedPoseFit implements the identity and gamma tone mappings (got {kind!r})")


def epoch_orders(n, epochs, seed=None, order=None):
    """The view order of every epoch.  order None: a shuffle per epoch, drawn and consumed as test.py:159-165 does
    (random.shuffle, then pop() from the END) from a generator seeded with `seed` (None: the global `random` state);
    a list of n indices: that order every epoch; a list of lists: one per epoch."""
    if order is not None:
        order = [list(o) for o in order] if (len(order) and isinstance(order[0], (list, tuple))) else [list(order)] * epochs
        if len(order) != epochs or any(sorted(o) != list(range(n)) for o in order):
            raise ValueError("order must be a permutation of the views, or one permutation per epoch")
        return order
    rng = random if seed is None else random.Random(seed)
    out = []
    for _ in range(epochs):
        idx = list(range(n))
        rng.shuffle(idx)
        out.append(idx[::-1])
    return out


def step_lrs(epochs, num_iter_per_view):
    """(rot lr, trans lr) of every epoch under StepLR(step_size = num_iter_per_view // 20, gamma = 0.9), advanced once per
    epoch; the products are formed one stage at a time, as the scheduler forms them."""
    step_size = max(int(num_iter_per_view) // LR_STAGES, 1)
    lr = [ROT_LR, TRANS_LR]
    out = []
    for e in range(epochs):
        if e > 0 and e % step_size == 0:
            lr = [x * LR_GAMMA for x in lr]
        out.append(tuple(lr))
    return out


def _capacity_for(need):
    """The capacity for poses that need `need` duplicates at the start: half as much again + 16384, rounded up as every
    learnt capacity is (raster_call.round_capacity)."""
    return raster_call.round_capacity(need + need // 2 + 16384)


def step_rows(steps_done, orders, first_epoch, num_iter_per_view):
    """The sequential fit's schedule on the host (no device is touched): one HYPER_WORDS row per step -- [0] the view
    index (int32), [1:5] dgs_adam_scalars' (-(lr / (1 - beta1^t)), sqrt(1 - beta2^t)) for rot and trans at the step's count
    t = steps_done + 1, ... and its epoch's learning rates.  orders: one view order per epoch; first_epoch: the StepLR
    epoch the first of them is."""
    L = _lib.lib()
    lrs = step_lrs(first_epoch + len(orders), num_iter_per_view)[first_epoch:]
    rows = np.zeros((sum(len(o) for o in orders), FusedPoseFit.HYPER_WORDS), dtype=np.float32)
    groups = (_lib.DgsAdamGroup * 2)()
    tmp = (ctypes.c_float * 4)()
    t, i = int(steps_done), 0
    for order, (lr_rot, lr_trans) in zip(orders, lrs):
        for idx in order:
            t += 1
            groups[0].lr, groups[0].step = lr_rot, t
            groups[1].lr, groups[1].step = lr_trans, t
            _lib.check(L.dgs_adam_scalars(groups, 2, 0.9, 0.999, tmp), "dgs_adam_scalars")
            rows[i, :1].view(np.int32)[0] = int(idx)
            rows[i, 1:5] = np.frombuffer(tmp, dtype=np.float32)
            i += 1
    return rows


def epoch_rows(steps_done, orders, first_epoch, num_iter_per_view):
    """The epoch-fused fit's schedule on the host: one row of 5 n words per epoch -- [0:n] pos (int32), pos[order[j]] = j,
    the turn of every view; [n:5n] the [n,4] scalars of the epoch's n steps, words [1:5] of step_rows' rows e n + j."""
    n = len(orders[0]) if len(orders) else 0
    if any(sorted(o) != list(range(n)) for o in orders):
        raise ValueError("every epoch's order must be a permutation of the views")
    per_step = step_rows(steps_done, orders, first_epoch, num_iter_per_view).reshape(len(orders), n, FusedPoseFit.HYPER_WORDS)
    rows = np.zeros((len(orders), 5 * n), dtype=np.float32)
    pos = rows[:, :n].view(np.int32)
    for e, order in enumerate(orders):
        pos[e, np.asarray(order, dtype=np.int64)] = np.arange(n, dtype=np.int32)
    rows[:, n:] = per_step[:, :, 1:5].reshape(len(orders), 4 * n)
    return rows


class _RasterCall:
    """The buffers, blobs, structs, capacity and captured graph of one K = G rasteriser call of a fit, over rows
    [begin, end) of its views.  Everything is allocated once: the captured graph bakes the addresses in."""

    def __init__(self, fit, begin, end, capacity):
        self.begin, self.end, self.G = begin, end, end - begin
        self.graph = None
        G, H, W, P = self.G, fit.H, fit.W, fit.cloud._xyz.shape[0]
        dev = fit.cloud._xyz.device
        f32 = dict(dtype=torch.float32, device=dev)
        L = _lib.lib()
        self.view, self.full = torch.empty((G, 4, 4), **f32), torch.empty((G, 4, 4), **f32)
        self.campos = torch.empty((G, 3), **f32)
        self.color, self.dcolor = torch.empty((G, 3, H, W), **f32), torch.empty((G, 3, H, W), **f32)
        self.radii = torch.empty((G, P), dtype=torch.int32, device=dev)
        self.drops = torch.zeros(1, dtype=torch.int32, device=dev)
        self.g_view, self.g_proj = torch.empty((G, 4, 4), **f32), torch.empty((G, 4, 4), **f32)
        self.host = torch.zeros(8, dtype=torch.int32).pin_memory()
        self.geom = torch.empty(L.dgs_geom_state_bytes(P, G), dtype=torch.uint8, device=dev)
        self.image = torch.empty(L.dgs_image_state_bytes(W, H, G), dtype=torch.uint8, device=dev)
        self.out_probe = raster_call.forward_out(self.color, None, self.radii, self.host)     # skips nothing, counts nothing
        self.capacity = int(capacity) if capacity is not None else _capacity_for(fit._duplicates(self))
        self.binning = torch.empty(L.dgs_binning_state_bytes(self.capacity, W, H, G), dtype=torch.uint8, device=dev)
        self.scratch = torch.empty(L.dgs_backward_scratch_bytes(self.capacity, P, G), dtype=torch.uint8, device=dev)
        self.skip_ptr = self.geom.data_ptr() + raster_call.skip_word_offset(P, W, H, G)
        self.prob = self.problem(fit, self.binning)
        self.out = raster_call.forward_out(self.color, None, self.radii, self.host, drop_counter=self.drops)
        self.io = _lib.DgsBackwardIO()
        self.io.num_rendered = self.capacity
        self.io.radii, self.io.dL_dout_color = _ptr(self.radii), _ptr(self.dcolor)
        self.io.scratch, self.io.scratch_bytes = _ptr(self.scratch), self.scratch.numel()
        self.io.dL_dviewmatrix, self.io.dL_dprojmatrix = _ptr(self.g_view), _ptr(self.g_proj)

    def problem(self, fit, binning=None):
        c0 = fit.model.cams[0]
        return raster_call.cloud_problem(fit.cloud, self.G, self.view, self.full, self.campos, fit.H, fit.W, c0.FoVx, c0.FoVy,
                                         fit.bg, fit.cull, self.geom, self.image, binning)

    def exact_count(self, fit):
        """The duplicate count of one exact (two-phase) forward at the cameras the call's buffers hold; a host read."""
        R, _ = raster_call.forward(fit.cloud._xyz.device, self.problem(fit), self.out_probe, self.host, None)
        return int(R)


class _PoseFit:
    """What the two fits share: the checks, the pose model, the ground truth, Adam's state, one _RasterCall per group of
    rows (`groups`), the capture of every group's launch chain, and the replay of an uploaded schedule.  A subclass
    gives the row ranges of its groups (_ranges), the duplicate count a group's lists are sized from (_duplicates), its
    device block and work area, its schedule rows, its chain (_enqueue), gradients() and dropped()."""

    def __init__(self, cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view, model, tile_cull, capacity):
        name = type(self).__name__
        if not getattr(cloud, "fused_activations", False):
            raise NotImplementedError(f"{name} needs a cloud with fused_activations")
        self.cloud = cloud
        dev = cloud._xyz.device
        if dev.type != "cuda":
            raise RuntimeError(f"{name} needs a cloud on a HIP device (no CPU fallback)")
        self.model = m = model if model is not None else TestPoseModel(cams, device=dev)
        self.n = n = len(m)
        ranges = self._ranges()
        c0 = m.cams[0]
        for c in m.cams:
            if (c.image_width, c.image_height, c.FoVx, c.FoVy, c.znear, c.zfar) != \
                    (c0.image_width, c0.image_height, c0.FoVx, c0.FoVy, c0.znear, c0.zfar):
                raise NotImplementedError(f"{name} captures one launch chain for all views: they must share image size and "
                                          f"intrinsics (fit views of different sizes with one {name} each)")
        self.H, self.W = H, W = int(c0.image_height), int(c0.image_width)
        self.num_iter_per_view = int(num_iter_per_view)
        self.tone_mapping, self._tone, self._eps, self._bound = _tone_args(tone_mapping)
        f32 = dict(dtype=torch.float32, device=dev)
        gt = torch.stack(list(gt_images)) if not torch.is_tensor(gt_images) else gt_images
        self.gt = gt.to(**f32).contiguous()
        if tuple(self.gt.shape) != (n, 3, H, W):
            raise ValueError(f"gt_images must be [{n},3,{H},{W}]")
        self.bg = bg.to(**f32).contiguous()
        self.proj = m.projection_matrix(0).to(**f32).contiguous()
        self.cull = dgr.TILE_CULL if tile_cull is None else bool(tile_cull)
        self.steps = 0                # Adam steps enqueued so far (the bias-correction exponent)
        self._sched = None
        # ---- what all groups share: the dense gradients (zero-filled: a rows kernel writes only its own rows), the
        # reference's l2_error_ema on the device, Adam's moments
        self.g_rot, self.g_trans = torch.zeros((n, 4), **f32), torch.zeros((n, 3), **f32)
        self.l2_ema = torch.zeros(1, **f32)
        self.exp_avg = [torch.zeros((n, 4), **f32), torch.zeros((n, 3), **f32)]
        self.exp_avg_sq = [torch.zeros((n, 4), **f32), torch.zeros((n, 3), **f32)]
        self._adam = (_lib.DgsAdamGroup * 2)(
            _lib.DgsAdamGroup(m._rot.data_ptr(), self.g_rot.data_ptr(), self.exp_avg[0].data_ptr(),
                              self.exp_avg_sq[0].data_ptr(), m._rot.numel(), ROT_LR, 1),
            _lib.DgsAdamGroup(m._trans.data_ptr(), self.g_trans.data_ptr(), self.exp_avg[1].data_ptr(),
                              self.exp_avg_sq[1].data_ptr(), m._trans.numel(), TRANS_LR, 1))
        # ---- per group: the cameras, images, lists and gradient matrices of its K = G call
        self.groups = [_RasterCall(self, b, e, capacity) for b, e in ranges]
        self.capacity = max(g.capacity for g in self.groups)

    def _capture(self):
        self.block.zero_()                    # view 0 / every view's turn the first
        for g in self.groups:                 # every kernel of the chain has run once: nothing is loaded inside the capture
            self._enqueue(g, apply=False)
        torch.cuda.synchronize(self.block.device)
        for g in self.groups:
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    self._enqueue(g)
            except RuntimeError as ex:
                raise RuntimeError(f"the pose-fit launch chain could not be captured into a hipGraph: {ex}") from ex
            g.graph = graph

    def _upload(self, rows):
        """The device schedule of a run, one row of the device block per replay; returns the number of rows."""
        self._sched = torch.from_numpy(rows).to(self.block.device)
        self._sched_pos = 0
        if self.groups[0].graph is None:
            self._capture()
        return rows.shape[0]

    def _replay(self, n_rows=None):
        """Enqueues the next n_rows (default: all remaining) rows of the uploaded schedule: per row one small copy launch
        (the row into the device block) and one graph launch per group.  No host synchronisation."""
        L = _lib.lib()
        stream = _stream(self.block.device)
        left = self._sched.shape[0] - self._sched_pos
        n_rows = left if n_rows is None else min(int(n_rows), left)
        block = ctypes.c_void_p(self.block.data_ptr())
        base, words = self._sched.data_ptr(), self.block.numel()
        for i in range(self._sched_pos, self._sched_pos + n_rows):
            _lib.check(L.dgs_copy_words(block, ctypes.c_void_p(base + 4 * words * i), words, stream), "dgs_copy_words")
            for g in self.groups:
                g.graph.replay()
        self._sched_pos += n_rows
        return n_rows

    def psnr_ema(self):
        """20 log10(1 / sqrt(l2_error_ema)) as the reference logs it (test.py:183); a host read."""
        v = float(self.l2_ema.item())
        return 20.0 * math.log10(1.0 / math.sqrt(v)) if v > 0.0 else float("inf")

    def cameras(self):
        with torch.no_grad():
            return [self.model(i) for i in range(self.n)]


class FusedPoseFit(_PoseFit):
    """The sequential fit (module docstring): one K = 1 launch chain per view step, its view drawn from the device block."""
    HYPER_WORDS = 8      # [0] view index (int32), [1:5] Adam's (-(lr / (1 - beta1^t)), sqrt(1 - beta2^t)) for rot, trans

    def __init__(self, cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view=2000, model=None, tile_cull=None,
                 capacity=None):
        """cloud: a GaussianCloud (fused_activations); cams: the test cameras (all of one image size and field of view);
        gt_images: [n,3,H,W] or a list of [3,H,W]; bg: [3]; tone_mapping: losses.ToneMapping("identity" | "gamma") or its
        name.  capacity: duplicates the lists are sized for (None: 1.5 x the largest count over the views at their
        start poses + 16384, learnt with one exact forward per view here, outside the loop)."""
        super().__init__(cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view, model, tile_cull, capacity)
        f32 = dict(dtype=torch.float32, device=cloud._xyz.device)
        self.block = torch.zeros(self.HYPER_WORDS, **f32)
        self.work = torch.zeros(12, **f32)           # dgs_view_loss_grad's work area: [0] l1, [1] mse

    color = property(lambda self: self.groups[0].color)      # the [1,3,H,W] render of the last step

    def _ranges(self):
        return [(0, 1)]

    def _pose_forward(self, g, idx_dev, idx, stream):
        m = self.model
        _lib.check(_lib.lib().dgs_testpose_forward(_ptr(m._rot), _ptr(m._trans), idx_dev, int(idx), self.n, _ptr(self.proj),
                                                   _ptr(g.view), _ptr(g.full), _ptr(g.campos), stream),
                   "dgs_testpose_forward")

    @torch.no_grad()
    def _duplicates(self, g):
        """One exact forward per view at its start pose: the largest duplicate count."""
        need = 0
        for i in range(self.n):
            self._pose_forward(g, None, i, _stream(self.cloud._xyz.device))
            need = max(need, g.exact_count(self))
        return need

    @torch.no_grad()
    def _enqueue(self, g, apply=True):
        """The six launches of one step on the current stream, everything read from the device block."""
        L = _lib.lib()
        m = self.model
        stream = _stream(self.cloud._xyz.device)
        idx_dev = ctypes.c_void_p(self.block.data_ptr())
        skip = ctypes.c_void_p(g.skip_ptr)
        self._pose_forward(g, idx_dev, 0, stream)
        _lib.check(L.dgs_forward(ctypes.byref(g.prob), ctypes.byref(g.out), g.capacity, stream), "dgs_forward")
        _lib.check(L.dgs_view_loss_grad(_ptr(g.color), _ptr(self.gt), idx_dev, self.n, 3, self.H * self.W, self._tone,
                                        self._eps, self._bound, None, _ptr(g.dcolor), _ptr(self.work),
                                        _ptr(self.l2_ema) if apply else None, skip, stream), "dgs_view_loss_grad")
        _lib.check(L.dgs_backward_pose_only(ctypes.byref(g.prob), ctypes.byref(g.io), stream), "dgs_backward_pose_only")
        _lib.check(L.dgs_testpose_backward(_ptr(m._rot), _ptr(m._trans), idx_dev, 0, self.n, _ptr(self.proj),
                                           _ptr(g.g_view), _ptr(g.g_proj), _ptr(self.g_rot), _ptr(self.g_trans),
                                           stream), "dgs_testpose_backward")
        if apply:
            _lib.check(L.dgs_adam_step_dev(self._adam, 2, 0.9, 0.999, ADAM_EPS, 0.0, skip,
                                           ctypes.c_void_p(self.block.data_ptr() + 4), stream), "dgs_adam_step_dev")

    @torch.no_grad()
    def gradients(self, idx):
        """One step WITHOUT its update, enqueued eagerly: the dense (dL/drot [n,4], dL/dtrans [n,3]) of view idx and the
        loss values (l1, mse) as device tensors."""
        self.block[:1].copy_(torch.tensor([int(idx)], dtype=torch.int32).view(torch.float32))
        self._enqueue(self.groups[0], apply=False)
        return self.g_rot.clone(), self.g_trans.clone(), self.work[:2].clone()

    def schedule(self, orders, first_epoch=0):
        """Uploads the device schedule of a run -- one 8-word row per step: the view index and Adam's scalars for the
        step's count and its epoch's learning rates -- and returns the number of steps.  orders: one view order per
        epoch (epoch_orders); first_epoch: the StepLR epoch the first of them is."""
        return self._upload(step_rows(self.steps, orders, first_epoch, self.num_iter_per_view))

    def run(self, n_steps=None):
        """Enqueues the next n_steps (default: all remaining) steps of the uploaded schedule (_replay)."""
        n_steps = self._replay(n_steps)
        self.steps += n_steps
        return n_steps

    def dropped(self):
        """Steps whose duplicate count exceeded the capacity (a host read): their update was skipped on the device."""
        return int(self.groups[0].drops.item())


class EpochPoseFit(_PoseFit):
    """The fit of FusedPoseFit with one launch chain per epoch and group of rows (module docstring): the same updates,
    n times fewer chains.  views_per_call: None = all n views in one K = n call; a number caps the views per call (memory:
    every call holds its own K = G images and lists) -- consecutive row groups of that size, each its own chain, buffers
    and captured graph, replayed one after the other.  n <= DGS_MAX_K views (an epoch's schedule is one device block)."""
    ROW_WORDS = 5         # per view and epoch: pos, then Adam's four scalars of one step

    def __init__(self, cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view=2000, model=None, tile_cull=None,
                 capacity=None, views_per_call=None):
        """As FusedPoseFit.  capacity: duplicates EVERY group's lists are sized for (None: per group, 1.5 x the count of one
        exact K = G forward at the start poses + 16384, rounded up as FusedPoseFit rounds)."""
        self._per_call = views_per_call
        super().__init__(cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view, model, tile_cull, capacity)
        n = self.n
        f32 = dict(dtype=torch.float32, device=cloud._xyz.device)
        # (each group writes its own rows of the turn-time parameters and of the work areas)
        self.block = torch.zeros(self.ROW_WORDS * n, **f32)      # [0:n] pos (int32), [n:5n] the [n,4] scalars
        self.peek = [torch.zeros((n, 4), **f32), torch.zeros((n, 3), **f32)]
        self.work = torch.zeros((n, 12), **f32)      # dgs_view_loss_grad_rows' work areas by row: [r,0] l1, [r,1] mse
        self._peek_out = (ctypes.c_void_p * 2)(self.peek[0].data_ptr(), self.peek[1].data_ptr())
        self._skips = (ctypes.c_void_p * len(self.groups))(*[g.skip_ptr for g in self.groups])
        self._begins = (ctypes.c_int32 * (len(self.groups) + 1))(*([g.begin for g in self.groups] + [n]))

    def _ranges(self):
        n = self.n
        if n > _lib.DGS_MAX_K:
            raise NotImplementedError(f"EpochPoseFit fits at most DGS_MAX_K = {_lib.DGS_MAX_K} views (got {n}): an epoch's "
                                      "schedule is one device block; use the sequential fit")
        per_call = n if self._per_call is None else int(self._per_call)
        if per_call < 1:
            raise ValueError("views_per_call must be at least 1")
        per_call = min(per_call, n)
        return [(b, min(b + per_call, n)) for b in range(0, n, per_call)]

    def _pose_forward(self, g, rot, trans, stream):
        _lib.check(_lib.lib().dgs_testpose_forward_rows(_ptr(rot), _ptr(trans), self.n, g.begin, g.end, _ptr(self.proj),
                                                        _ptr(g.view), _ptr(g.full), _ptr(g.campos), stream),
                   "dgs_testpose_forward_rows")

    @torch.no_grad()
    def _duplicates(self, g):
        """One exact K = G forward of the group at its start poses."""
        self._pose_forward(g, self.model._rot, self.model._trans, _stream(self.cloud._xyz.device))
        return g.exact_count(self)

    @torch.no_grad()
    def _enqueue(self, g, apply=True):
        """The launches of one group's epoch on the current stream, the schedule read from the device block."""
        L = _lib.lib()
        n = self.n
        stream = _stream(self.cloud._xyz.device)
        pos = ctypes.c_void_p(self.block.data_ptr())
        scalars = ctypes.c_void_p(self.block.data_ptr() + 4 * n)
        skip = ctypes.c_void_p(g.skip_ptr)
        _lib.check(L.dgs_adam_epoch_peek(self._adam, 2, self._peek_out, n, g.begin, g.end, pos, scalars, n, 0.9, 0.999,
                                         ADAM_EPS, stream), "dgs_adam_epoch_peek")
        self._pose_forward(g, self.peek[0], self.peek[1], stream)
        _lib.check(L.dgs_forward(ctypes.byref(g.prob), ctypes.byref(g.out if apply else g.out_probe), g.capacity, stream),
                   "dgs_forward")
        _lib.check(L.dgs_view_loss_grad_rows(_ptr(g.color), _ptr(self.gt), n, g.begin, g.end, 3, self.H * self.W, self._tone,
                                             self._eps, self._bound, None, _ptr(g.dcolor), _ptr(self.work, 12 * g.begin),
                                             stream), "dgs_view_loss_grad_rows")
        _lib.check(L.dgs_backward_pose_only(ctypes.byref(g.prob), ctypes.byref(g.io), stream), "dgs_backward_pose_only")
        _lib.check(L.dgs_testpose_backward_rows(_ptr(self.peek[0]), _ptr(self.peek[1]), n, g.begin, g.end, _ptr(self.proj),
                                                _ptr(g.g_view), _ptr(g.g_proj), _ptr(self.g_rot), _ptr(self.g_trans),
                                                stream), "dgs_testpose_backward_rows")
        if apply:
            _lib.check(L.dgs_adam_epoch_step(self._adam, 2, n, g.begin, g.end, pos, scalars, n, 0.9, 0.999, ADAM_EPS, skip,
                                             stream), "dgs_adam_epoch_step")
            if g is self.groups[-1]:
                _lib.check(L.dgs_l2_ema_epoch(_ptr(self.work), pos, n, self._skips, self._begins, len(self.groups),
                                              _ptr(self.l2_ema), stream), "dgs_l2_ema_epoch")

    @torch.no_grad()
    def gradients(self):
        """An epoch WITHOUT its update, enqueued eagerly, at the current parameters (every view's turn taken as the first:
        no zero-gradient step precedes it): all rows of (dL/drot [n,4], dL/dtrans [n,3]) and the views' (l1, mse) [n,2],
        as device tensors."""
        self.block.zero_()
        for g in self.groups:
            self._enqueue(g, apply=False)
        return self.g_rot.clone(), self.g_trans.clone(), self.work[:, :2].clone()

    def schedule(self, orders, first_epoch=0):
        """Uploads the device schedule of a run -- one row of 5 n words per epoch (epoch_rows) -- and returns the number of
        epochs.  orders: one view order per epoch (epoch_orders); first_epoch: the StepLR epoch the first of them is."""
        if any(len(o) != self.n for o in orders):
            raise ValueError("every epoch's order must be a permutation of the views")
        return self._upload(epoch_rows(self.steps, orders, first_epoch, self.num_iter_per_view))

    def run(self, n_epochs=None):
        """Enqueues the next n_epochs (default: all remaining) epochs of the uploaded schedule (_replay)."""
        n_epochs = self._replay(n_epochs)
        self.steps += n_epochs * self.n
        return n_epochs

    def dropped(self):
        """View-steps skipped (a host read): a group whose K = G forward exceeded its capacity skips its rows' whole epoch,
        G view-steps -- where the sequential fit skips the one step of the view that overflowed."""
        return sum(int(g.drops.item()) * g.G for g in self.groups)


def optimize_test_pose(cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view=2000, order=None, seed=None,
                       log_every=0, mode="sequential", views_per_call=None, capacity=None):
    """test.py:131-186 on the fused step: fits the test cameras to the cloud and returns the fitted cameras
    ([TestPoseModel(i) for i in range(n)]).  order: see epoch_orders (None: a seeded or global shuffle per epoch).
    log_every > 0 prints the reference's progress line every that many epochs (one host read each).
    mode: "sequential" (FusedPoseFit: one launch chain per view step) or "epoch" (EpochPoseFit: one per epoch, the same
    updates; views_per_call caps the views rendered by one call).  capacity: see the two classes (None: learnt)."""
    if mode not in ("sequential", "epoch"):
        raise ValueError(f"mode must be 'sequential' or 'epoch' (got {mode!r})")
    if mode == "epoch":
        fit = EpochPoseFit(cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view=num_iter_per_view, capacity=capacity,
                           views_per_call=views_per_call)
    else:
        fit = FusedPoseFit(cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view=num_iter_per_view, capacity=capacity)
    epochs = int(num_iter_per_view)
    orders = epoch_orders(fit.n, epochs, seed=seed, order=order)
    chunk = int(log_every) if log_every and log_every > 0 else epochs
    for e0 in range(0, epochs, max(chunk, 1)):
        fit.schedule(orders[e0:e0 + chunk], first_epoch=e0)
        fit.run()
        if log_every and log_every > 0:
            print(f"Optimizing...PSNR ={fit.psnr_ema():6.2f} epoch {min(e0 + chunk, epochs)}/{epochs}", flush=True)
    torch.cuda.synchronize(cloud._xyz.device)
    drops = fit.dropped()
    if drops:
        raise RuntimeError(f"{drops} of {fit.steps} pose-fit steps exceeded the duplicate capacity ({fit.capacity}) and "
                           f"were skipped; fit again with {type(fit).__name__}(capacity=...) sized for the poses it moves through")
    return fit.cameras()


def initialize_test_pose(motion, cloud, test_images, bg, tone_mapping=None, **kw):
    """Starting poses for unposed test images, the place of test.py:188-398: [TestCamera] * n (original_image set) for
    optimize_test_pose.  This is coarse photometric registration and NOT the reference's COLMAP registration: renders of
    poses along the learned training trajectories are scored against every test image on the device and the best one is
    polished by a short pattern search (registration.seed_test_poses, which takes **kw and returns the scores too)."""
    from . import registration
    return registration.seed_test_poses(motion, cloud, test_images, bg, tone_mapping, **kw).cameras


def _write_view(vis_dir, i, image, gt, writer, device_png=False):
    """The three files of view i (test.py:122-126) from the image the metrics were taken of."""
    if vis_dir is not None:
        from . import report
        report.write_view_report(vis_dir, i, image, gt.contiguous(), writer, device_png=device_png)


@torch.no_grad()
def _lpips_values(images, gts, weights):
    """The LPIPS of every (image, gt) pair as host floats: one call with n_pairs = len(images) (a pair's value does not
    depend on the others of its call), the reference's `.mean().item()` per view."""
    from . import lpips as _lpips
    x = torch.stack(list(images))
    y = torch.stack([g.to(x) for g in gts])
    return [float(v) for v in _lpips.lpips_layers(x, y, weights)[:, 0].tolist()]


@torch.no_grad()
def _evaluate_grouped(cams, cloud, bg, gt_images, tone_mapping, views_per_call, vis_dir=None, writer=None, lpips=None,
                      device_png=False):
    """evaluate() with the cameras rendered views_per_call at a time: one K-fused forward-only call per group
    (render_path.render_group), then the per-view metrics of evaluate() on slot k, summed in the same order (LPIPS: the G
    views of a call as n_pairs = G)."""
    from . import render_path
    cams = list(cams)
    psnr_test, ssim_test, lpips_test = 0.0, 0.0, 0.0
    for b, e in render_path.frame_groups(cams, views_per_call):
        images = render_path.render_group(cams[b:e], cloud, bg)["render"]
        if lpips is not None:
            for v in _lpips_values([tone_mapping(images[k]) for k in range(e - b)], gt_images[b:e], lpips):
                lpips_test += v
        for k in range(e - b):
            image = tone_mapping(images[k]).contiguous()
            gt = gt_images[b + k].to(image)
            _write_view(vis_dir, b + k, image, gt, writer, device_png)
            if image.device.type == "cuda":
                both = metrics.psnr_ssim(image, gt.contiguous())
                psnr_test += both[2:5].reshape(3, 1).mean().item()
                ssim_test += both[1].mean().item()
            else:
                psnr_test += metrics.psnr(image, gt).mean().item()
                ssim_test += metrics.ssim(image, gt).mean().item()
    if lpips is not None:
        return psnr_test / len(cams), ssim_test / len(cams), lpips_test / len(cams)
    return psnr_test / len(cams), ssim_test / len(cams)


@torch.no_grad()
def evaluate(cams, cloud, bg, gt_images, tone_mapping, views_per_call=None, vis_dir=None, writer=None, lpips=None,
             device_png=False):
    """test.py:93-129: (mean PSNR, mean SSIM) over the cameras -- and, with lpips = an lpips.LPIPSWeights (on the images'
    device), (mean PSNR, mean SSIM, mean LPIPS-alex): test.py:120 on the same tone-mapped, unclamped image, one
    dgs_lpips_alex call per view (per group of views under views_per_call), its value independent of views_per_call.
    Without `lpips` the two floats are what they were, bit for bit.  The render of every camera goes through the
    forward_only inference path (gaussian_renderer.render under no_grad), is tone-mapped and NOT clamped, and both metrics
    come from one fused kernel per view (metrics.psnr / metrics.ssim).
    views_per_call: None renders one camera per call; a number renders the cameras that many at a time through the
    K-fused forward-only call -- slot i of such a call is the K = 1 render bit for bit, so the two floats are the same.
    vis_dir: a directory (removed and recreated, as test.py:104-107 prepares model_path/vis_dir) that receives
    III_gt.png, III_render.png and III_error.png -- the jet-coloured L1 map -- per view (report.write_view_report: the
    images are made on the device, needs a HIP device); writer(path, array) takes the place of the files (then no
    directory is touched).  The two floats, and the files, do not depend on views_per_call; the floats not on vis_dir.
    device_png=True: the three files of a view are compressed on the device in one png.encode call instead of by PIL on
    the host (same names, same pixels; not together with a writer)."""
    if tone_mapping is None or isinstance(tone_mapping, str):
        tone_mapping = losses.ToneMapping(tone_mapping or "identity")
    if writer is not None and vis_dir is None:
        raise ValueError("writer takes the place of the files under vis_dir: give vis_dir too (it names the paths)")
    from . import report
    report.no_writer_with_device_png(writer, device_png)
    if vis_dir is not None and writer is None:
        report.fresh_directory(vis_dir)
    if views_per_call is not None:
        return _evaluate_grouped(cams, cloud, bg, gt_images, tone_mapping, views_per_call, vis_dir, writer, lpips,
                                 device_png)
    psnr_test, ssim_test, lpips_test = 0.0, 0.0, 0.0
    n = len(cams)
    for i, (cam, gt) in enumerate(zip(cams, gt_images)):
        image = tone_mapping(gaussian_renderer.render(cam, cloud, bg)["render"]).contiguous()
        gt = gt.to(image)
        _write_view(vis_dir, i, image, gt, writer, device_png)
        if image.device.type == "cuda":       # one launch for both: the values metrics.psnr / metrics.ssim return
            both = metrics.psnr_ssim(image, gt.contiguous())
            psnr_test += both[2:5].reshape(3, 1).mean().item()
            ssim_test += both[1].mean().item()
        else:
            psnr_test += metrics.psnr(image, gt).mean().item()
            ssim_test += metrics.ssim(image, gt).mean().item()
        if lpips is not None:
            lpips_test += _lpips_values([image], [gt], lpips)[0]
    if lpips is not None:
        return psnr_test / n, ssim_test / n, lpips_test / n
    return psnr_test / n, ssim_test / n

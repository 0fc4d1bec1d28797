"""The device work of one training iteration enqueued straight through the C ABI -- no torch autograd graph, no
elementwise torch glue, no host synchronisation:

    alignment (nu = sort(clamp(cat(0, sigmoid(_nu[view]), 1)))            dgs_alignment_forward
    -> Bezier / se3_exp_map / K cameras                                   dgs_pose_forward
    -> fused K-subframe rasterisation of the cloud's raw parameters       dgs_forward (capacity sized ahead) or the
                                                                          two-phase dgs_forward_geometry / _render
    -> blur image, L1 + temporal-smoothness values and dL/dsubframes      dgs_blur_loss_grad (one pass)
    -> rasteriser backward (+ the opacity-hinge gradient)                 dgs_backward
    -> camera gradients back to the control points and alignment          dgs_pose_backward, dgs_alignment_backward

i.e. scene/motion.py:78-160 + train.py:143-165 of the reference for one blurry view.  The gradients are left in `.grad`
of the cloud's and the motion module's parameters exactly where `loss.backward()` of the autograd path
(CameraMotionModule.query + losses.blur_l1_smooth + losses.hinge_l2) leaves them -- the six per-Gaussian ones as views
of one flat bucket -- so the optimiser step, the sharded all-reduce and the densification statistics that follow are
unchanged.  tests/test_gpu_train.py checks the two paths against each other.

Why: at DeblurGS's real scene sizes (1e4..1e5 Gaussians) the autograd path is host-bound -- ~45 small torch launches,
autograd bookkeeping and one blocking read of num_rendered per step cost more than the kernels.  Here a step is ~12
ctypes calls.

Sizing ahead (`speculative=True`): the duplicate arrays of a step are sized from the duplicate counts observed in earlier
steps OF THE SAME (view, subframe count) (+25 %), which are read from pinned memory only once their copy has completed --
never blocking.  A (view, subframe count) that has no count yet -- a view drawn for the first time, the switch from one
subframe to all of them at curve_start_iter, any view after a densification -- takes the exact two-phase forward (one
host read), so those changes never overflow.  If a step's count still exceeds its capacity the kernels set a device flag
instead of writing out of bounds; the flag makes the optimiser step and the densification statistics of THAT step
no-ops (FusedAdam.skip_flag_ptr), so a truncated gradient is never applied.  Such a step is counted (`dropped`) and
queued (`retry`): TrainingLoop re-runs the view through the exact path as soon as the flag has been read, so every view
still gets its update (the reference applies every step).
"""
import collections
import ctypes

import torch

from . import _lib
from . import diff_gaussian_rasterization as dgr
from . import raster_call
from .raster_call import _ptr, _stream


class CaptureRefused(RuntimeError):
    """The runtime refused to capture a step into a hipGraph.  Raised only from inside the capture block: nothing of the
    step has been enqueued, so the caller may run the step eagerly instead.  Errors of a cached graph's replay or of the
    eager part behind it are NOT of this kind and propagate as they are."""


class _Pending:
    __slots__ = ("host", "event", "capacity", "speculative", "key", "generation", "request")


# What a step that is being RECORDED into a hipGraph is handed from outside the graph's memory pool (_capture_setup): the
# capacity of the duplicate arrays, the pinned count words, the status words, the address of the scalar block (lambda_t is
# read from it on the device; words [4:6] hold the address of the step's pinned status slot), the loss kernel's work block
# and the gradient bucket -- and, for a sharded front, the radii, the screen gradients and the skip word that all fronts of
# a cloud generation share.  No host bookkeeping happens for such a step.  How far a capture records is the capture's own
# business: it calls the stages it wants.
_Capture = collections.namedtuple("_Capture", "capacity host status lambda_ptr work bucket radii means2D skipw",
                                  defaults=(None, None, None))


class _Step:
    """Everything one iteration owns, by name.  The stages of FusedStep (_cameras -> _forward -> _loss_backward ->
    _finish) fill it in; nothing else keeps a step's tensors alive.

    LARGE fields -- a capture gives them back to the graph pool (release_large), so the pool holds ONE step's buffers, not
    one set per captured view.  The launches reach them through raw addresses that outlive the Python references:

        field      raw address in                        last read by
        geom       prob.geom_state, skip_ptr (one word)  the backward; the optimiser / statistics launch (skip word)
        image      prob.image_state                      the backward's compositing half
        binning    prob.binning_state                    the backward's compositing half
        scratch    io.scratch                            dgs_backward_pose, the last launch of _finish
        color      out.out_color                         the loss kernel (or the result's 'subframes')
        depth      out.out_depth                         the depth-smoothness term (or the result's 'depths')
        dsub       io.dL_dout_color                      the backward's compositing half
        blur       --                                    the result's 'blur'
        g_colors   io.dL_dcolors                         the backward's per-Gaussian half
        g_cov3D    io.dL_dcov3D                          the backward's per-Gaussian half

    The three kinds of raw address and what keeps their memory valid until the last reader has run:
      * skip_ptr points into the geometry blob and is read by the optimiser launch AFTER the step.  An eager step is
        FusedStep._keep until the next step begins, so the blob is not handed to a later allocation in between.  A whole
        captured step (replay) runs that launch inside the graph.  A captured front copies the word into one outside the
        pool (_Capture.skipw) before it lets go of the blob -- `skip_flag` as a VIEW of the blob would pin all of it.
      * prob / io hold the addresses of every large field but blur.  After a capture those are blocks of the graph pool
        that this step no longer owns: they stay valid until the next replay of ANY graph of the pool, and that replay is
        enqueued behind this step's eager part on the same stream (stream order inside the shared pool).  An eager
        step's are allocations of the current stream, kept by FusedStep._keep until the next step.
      * out.status_host_indirect is the address of words [4:6] of the scalar block: no field of the step, it belongs to
        the graph entry ('hyper') and lives as long as the graph.

    SMALL fields live as long as the step -- until the next one replaces FusedStep._keep -- or, for a recorded step, as
    long as its graph entry.  A front recorded up to the forward keeps `color` and `depth` too (release_large(keep=)):
    its loss runs eagerly and reads them as tensors."""
    LARGE = ("geom", "image", "binning", "scratch", "color", "depth", "dsub", "blur", "g_colors", "g_cov3D")
    SMALL = (
        # the request
        "cap", "request", "gt", "need_blur", "lambda_depth_tv", "shard", "ar", "stats",
        # alignment and cameras
        "nu_all", "src", "sel", "uniform", "raw_ptr", "proj", "view", "full", "campos", "nu", "nu_loc",
        "cam", "K", "K_total", "k0", "P", "H", "W", "Mr", "C", "row", "rrow", "quat", "nrow",
        # forward
        "bg", "radii", "prob", "out", "R", "skip_ptr", "skip_flag",
        # loss and backward
        "gtc", "work", "losses", "flat", "g_xyz", "g_dc", "g_rest", "g_op", "g_sc", "g_rot", "g_means2D", "g_depth",
        "depth_tv", "g_view", "g_proj", "io", "chunked")
    __slots__ = LARGE + SMALL

    def __init__(self, **fields):
        # (what an eager step's stages read but need not set; every other unset field reads as None too, more slowly)
        self.cap = self.sel = self.depth = self.skip_ptr = self.skip_flag = self.g_depth = self.depth_tv = None
        self.g_means2D = None
        for name, value in fields.items():
            setattr(self, name, value)

    def __getattr__(self, name):        # only reached for a field that nothing has set yet
        if name in _Step.__slots__:
            return None
        raise AttributeError(name)

    def release_large(self, keep=()):
        for name in self.LARGE:
            if name not in keep:
                setattr(self, name, None)

    def copy(self):
        new = _Step.__new__(_Step)
        for name in self.__slots__:
            setattr(new, name, getattr(self, name))
        return new


class FusedStep:
    def __init__(self, cloud, motion, lambda_hinge=0.0, speculative=True, tile_cull=None):
        if not getattr(cloud, "fused_activations", False):
            raise NotImplementedError("FusedStep needs a cloud with fused_activations")
        self.cloud, self.motion = cloud, motion
        self.lambda_hinge = float(lambda_hinge)
        self.speculative = bool(speculative)
        self.tile_cull = tile_cull
        self.dropped = 0            # steps whose duplicate count exceeded the capacity (their update was skipped)
        self.retry = []             # their (cam_idx, subframe_indice): to be re-run by the caller (pop from here)
        self._seen = {}             # (cam_idx, subframe count) -> recent duplicate counts of that view
        self._generation = 0        # bumped when the cloud changes size: counts of older forwards are not learnt
        self._pending = []          # forwards whose counts have not been read back yet
        self._free_hosts = []
        self._keep = None           # the last step (_Step: its skip word lives in its geometry blob)
        self._proj_cache = None     # (the matrix, its version, its contiguous fp32 copy on the device)
        self.last_capacity = None
        # replay() / replay_front() decline (None: the caller enqueues the step eagerly) when the library would run this
        # view's compositing backward in parts if it were enqueued eagerly (dgs_backward_parts > 1: large views).  Inside a
        # capture the backward is one launch -- a forked executable graph does not return its memory on this runtime --
        # and beside its row totals the eagerly enqueued step is the faster one at these sizes (metric configuration:
        # 10.54-10.62 against 10.76-10.87 ms replayed).  True (TrainingLoop(graph="always")) captures anyway.
        self.capture_large = False
        # the reference composites the depth image with every render (forward.cu:373,390) and query() returns it; the default
        # loss never reads it (train.py:150-153, lambda_depth_tv = 0), so the fused step leaves it out unless asked
        # (run(need_depth=True), lambda_depth_tv > 0) -- or unless this is set (bench.py's value_with_depth region)
        self.always_depth = False
        # "mesh" sharding: the process group of this rank's ROW (the ranks that split one view's subframes); None = the
        # default group ("subframes" mode: all ranks share the view)
        self.loss_group = None
        self.eager_preferred = 0    # steps declined for that reason
        self._sel_cache = {}
        self._side = None           # side stream of the chunked gradient all-reduce
        self.time_allreduce = False
        self.ar_events = []
        self._drops_dev = None      # device word: captured forwards that overflowed so far (DgsForwardOut.drop_counter)
        self._bucket = None         # (generation, numel, tensor): the gradient bucket all captured steps write to
        self._front_shared = None   # (key, radii, screen gradients, skip word) of the captured sharded fronts
        self._graphs = {}           # captured steps by what they bake in (replay)
        self._pool = None           # one memory pool for all of them: replays never overlap
        self._release_pool = False  # a dropped pool's blocks go back to the driver before the next capture
        self._ring, self._ring_pos = [], 0
        self.max_graphs = 256
        self.captured = 0
        self.replayed = 0

    # ------------------------------------------------------------------------------------------ capacity policy
    def _poll(self, block=False):
        still = []
        for pnd in self._pending:
            if block:
                pnd.event.synchronize()
            if pnd.event.query():
                # Every entry owns its pinned words.  An eager step's are written by dgs_forward's own copies; a REPLAYED
                # step's by a copy of the graph's DgsForwardOut.status_dev enqueued right behind that replay (_track)
                # -- the pinned block baked into a graph is rewritten by every later replay of the same view while the host
                # runs several replays ahead, so it can never say which replay overflowed (with two views in
                # flight a running drop counter read from those blocks went backwards and queued 2^32 - 1 retries).
                R, overflow, _ = raster_call.counts(pnd.host)
                if pnd.speculative and overflow:
                    self.dropped += 1
                    self.retry.append(pnd.request)
                if pnd.generation == self._generation:
                    self._seen[pnd.key] = (self._seen.get(pnd.key, []) + [R])[-4:]
                self._free_hosts.append(pnd.host)
            else:
                still.append(pnd)
        self._pending = still

    def _track(self, host, speculative, ckey, request, cap, dev):
        """Behind a forward: the step joins the pending list with the pinned words its count / overflow words go to.  An
        eager step's are written by dgs_forward's own copies.  A replayed step's are the slot that its forward's finalize
        kernel writes into (DgsForwardOut.status_host_indirect: the slot's address travelled to the graph through the
        scalar block, no copy behind the replay)."""
        pnd = _Pending()
        pnd.host = host
        pnd.speculative, pnd.key, pnd.generation = speculative, ckey, self._generation
        pnd.request, pnd.capacity = request, cap
        pnd.event = torch.cuda.Event()
        pnd.event.record(torch.cuda.current_stream(dev))
        self._pending.append(pnd)

    def _push_scalars(self, ent, hbuf, dev):
        """This step's scalar block -- and the address of the pinned slot its count words go to (words [4:6]) -- from the
        pinned ring buffer to the graph's device block by a KERNEL (dgs_copy_words): an asynchronous copy in front of every
        graph launch costs a hand-over between the copy engine and the compute queue, tens of microseconds per step."""
        slot = self._host_words()
        hbuf.numpy().view("uint64")[2] = slot.data_ptr()
        _lib.check(_lib.lib().dgs_copy_words(_ptr(ent["hyper"]), _ptr(hbuf), int(hbuf.numel()), _stream(dev)),
                   "dgs_copy_words")
        return slot

    def _eager_is_faster(self, K, cap, cull):
        dev = self.cloud._xyz.device.index     # (the context the step's backward runs with)
        if self.capture_large or _lib.context_overlap_mode(dev) == 3:   # (3: the library forks inside a capture too)
            return False
        if _lib.lib().dgs_backward_parts(_lib.context(dev), int(K), int(cap), int(bool(cull))) <= 1:
            return False
        self.eager_preferred += 1
        return True

    def _capacity(self, key):
        seen = self._seen.get(key)
        if not seen:
            return None
        need = max(seen)
        return need + need // 4 + 16384

    def invalidate(self):
        """The cloud changed (densification, pruning, a restored checkpoint): forget the learnt counts -- also those still
        on their way back -- so that every view takes the exact path once."""
        self._generation += 1
        self._seen = {}
        if self._graphs or self._pool is not None:
            # the captured steps die with the cloud they were captured for, and their memory pool with them: a pool only
            # ever grows (a block freed by one capture is re-used by the next only if it is large enough), so a cloud that
            # grows a little at every densification would otherwise leave one full set of step buffers behind per
            # generation (soak run, 100 k -> 3.4 M Gaussians: 159 GiB instead of 25)
            self._graphs = {}
            self._pool = None
            self._bucket = None
            self._front_shared = None
            self._release_pool = True

    def _host_words(self):
        if self._free_hosts:
            h = self._free_hosts.pop()
            h.zero_()
            return h
        return torch.zeros(8, dtype=torch.int32).pin_memory()

    def _empty_slice(self, st, lambda_t):
        """"subframes" sharding with more ranks than subframes: this rank rasterises nothing but takes part in the loss
        block's exchanges; all its gradients are zero."""
        from . import sharding
        cloud, m = self.cloud, self.motion
        dev = cloud._xyz.device
        gt, K_total, P, H, W, lambda_depth_tv, ar = st.gt, st.K_total, st.P, st.H, st.W, st.lambda_depth_tv, st.ar
        ct_all, cr_all, nu_raw = m._trans._control_points, m._rot._control_points, m._nu
        f32 = dict(dtype=torch.float32, device=dev)
        color = torch.zeros((0, 3, H, W), **f32)
        _, l1, sm = sharding.subframe_sharded_loss_grad(color, gt.to(dev, torch.float32).contiguous(), K_total,
                                                        float(lambda_t), self.loss_group)
        # The collectives below are issued in EXACTLY the order _loss_backward and _finish issue them on a rank that holds subframes -- loss
        # block, depth-smoothness value, gradient bucket (whole or in chunks) -- because RCCL pairs collectives by issue
        # order on the communicator: a different order here would pair a one-element all-reduce with a bucket slice.
        depth_tv = None
        if lambda_depth_tv > 0.0:      # this rank's share of the depth-smoothness value is zero
            import torch.distributed as dist
            depth_tv = torch.zeros((), **f32)
            dist.all_reduce(depth_tv, group=self.loss_group)
        if ar is None:
            for p in cloud.hot_parameters():
                p.grad = torch.zeros_like(p)
        else:      # take part in the other ranks' (chunked) reduction of the gradient bucket with a bucket of zeros
            hot = list(cloud.hot_parameters())
            bucket = raster_call.Bucket([p.numel() for p in hot])
            flat = torch.zeros(bucket.size, **f32)
            for p, g in zip(hot, bucket.views(flat, [p.shape for p in hot])):
                p.grad = g
            if int(ar.get("chunks", 1)) <= 1 or P < 512:
                if P > 0:
                    sharding._allreduce(flat, ar.get("average", False), ar.get("group"))
            else:
                for b0, b1 in sharding.chunk_bounds(P, int(ar["chunks"])):
                    sharding.allreduce_slices(bucket.chunk(flat, P, b0, b1), ar.get("average", False), ar.get("group"))
        if m.is_optimizing():
            m._trans._control_points.grad, m._rot._control_points.grad = torch.zeros_like(ct_all), torch.zeros_like(cr_all)
            if nu_raw.numel() > 0:
                m._nu.grad = torch.zeros_like(nu_raw)
        return {"losses": torch.stack([l1.reshape(()), sm.reshape(())]).float(), "blur": None,
                "radii": torch.zeros((0, P), dtype=torch.int32, device=dev), "viewspace_grad": torch.zeros((0, P, 3), **f32),
                "K": K_total, "subframes": color, "depths": torch.zeros((0, 1, H, W), **f32), "skip_flag_ptr": None,
                "skip_flag": None, "depth_tv": depth_tv}

    def _linspace_sel(self, f, n, dev):
        key = (f, n, str(dev))
        if key not in self._sel_cache:
            self._sel_cache[key] = torch.linspace(0, f - 1, n, device=dev).long()
        return self._sel_cache[key]

    def _drop_counter(self, dev):
        if self._drops_dev is None:
            self._drops_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._drops_dev

    # ------------------------------------------------------------------------------------------ captured replay
    HYPER_FLOATS = 64        # [0] lambda_t, [1:4] background, [4:6] address of the step's pinned status slot (one uint64),
                             # [8:8 + 2 * 16] Adam scalars, [48:] alignment jitter (f <= 16)

    def _hyper_words(self, f):
        return (max(self.HYPER_FLOATS, 48 + f) + 1) // 2 * 2        # (even: words [4:6] are written as one uint64)

    def replay(self, cam_idx, lambda_t, gt, subframe_indice, optimizer, tail, signature=(), background=None,
               uniform=None, stats=None):
        """One training iteration as ONE hipGraph launch (SURVEY 8f / DESIGN 2b): alignment -> cameras -> dgs_forward
        (capacity sized ahead) -> loss -> dgs_backward -> camera gradients -> `tail` (densification statistics + the
        optimiser launch).  At DeblurGS's real scene sizes a step is ~60 kernels of a few microseconds each; replayed
        from a graph they cost one launch instead of ~20 ctypes calls and their driver round trips.

        What changes from step to step travels through one small device block written before the launch: lambda_t, the
        random background, the alignment jitter and Adam's step-size scalars (optimizer.step_scalars).  Everything else
        -- the view, the subframe selection, the active SH degree, which parameters are optimised, the capacity of the
        duplicate arrays, every buffer address -- is baked into the graph: one graph per distinct combination, captured
        the first time it is needed (and re-captured when the cloud is rebuilt or a capacity grows).

        Returns the result dict of run(), or None when this step cannot be replayed yet (no duplicate count learnt for
        the view: the caller runs the eager step, which learns it)."""
        plan = self._replay_plan(cam_idx, subframe_indice)
        if plan is None:
            return None
        K_total, ckey, cap, cull = plan
        gkey = self._graph_key(cam_idx, subframe_indice, cap, gt, cull) + (
            tuple(signature), tuple(t.data_ptr() for t in stats) if stats is not None else ())
        ent = self._graphs.get(gkey)
        if ent is None:
            ent = self._capture(gkey, cam_idx, gt, subframe_indice, cap, optimizer, tail, stats)
        hbuf, hev = self._scalar_slot(ent, lambda_t, background, uniform)
        for p, g in ent["grads"]:              # the step's gradients live in the graph's buffers
            p.grad = g
        optimizer.skip_flag_ptr = ent["result"]["skip_flag_ptr"]
        optimizer.step_scalars(hbuf.numpy()[8:8 + 2 * _lib.ADAM_MAX_GROUPS])
        self._launch(ent, hbuf, hev, ckey, (cam_idx, subframe_indice), cap)
        return ent["result"]

    def replay_front(self, cam_idx, lambda_t, gt, subframe_indice, ar, background=None, uniform=None, shard=None,
                     background_dev=None, uniform_dev=None):
        """A SHARDED step ("views" mode) with everything up to its first collective replayed as one hipGraph: alignment ->
        cameras -> dgs_forward (capacity sized ahead) -> loss -> the compositing half of the backward
        (dgs_backward_composite; the whole dgs_backward when the bucket is reduced in one piece) -- then, eagerly, what
        run() does after that point: the per-Gaussian half in Gaussian-index chunks with each chunk's all-reduce behind it
        on the side stream, the camera gradients.  The caller's reductions of the skip flag and the trajectory gradients and
        its optimiser step follow as after run().  Bit-identical to the eager step (the same launches in the same order on
        the same stream); what it saves is the ~20 ctypes calls and driver round trips of the front, 0.2-0.3 ms per step.

        shard = (rank, world): "subframes" sharding.  Its first collective is the loss block, so the captured front ends
        with the forward of this rank's slice of the cameras; the background and the alignment jitter are rank 0's draws and
        arrive as DEVICE tensors (background_dev, uniform_dev: TrainingLoop._shared_draws), copied into the graph's scalar
        block on the stream.  A rank whose slice is empty is not captured (None).

        Returns run()'s result dict ('subframes', 'blur' and 'depths' are None in "views" mode: the images live in the
        graph's pool), or None when the step cannot be replayed yet (no duplicate count learnt for the view)."""
        plan = self._replay_plan(cam_idx, subframe_indice, shard)
        if plan is None:
            return None
        K_total, ckey, cap, cull = plan
        chunks = 1 if ar is None else int(ar.get("chunks", 1))
        gkey = ("front",) + self._graph_key(cam_idx, subframe_indice, cap, gt, cull) + (
            chunks, float(self.lambda_hinge), None if shard is None else (int(shard[0]), int(shard[1])))
        ent = self._graphs.get(gkey)
        if ent is None:
            ent = self._capture_front(gkey, cam_idx, gt, subframe_indice, cap, ar, K_total, shard)
        hbuf, hev = self._scalar_slot(ent, lambda_t, background, uniform)
        self._launch(ent, hbuf, hev, ckey, (cam_idx, subframe_indice), cap, background_dev, uniform_dev)
        return ent["finish"](ent["step"], float(lambda_t))

    def _graph_key(self, cam_idx, subframe_indice, cap, gt, cull):
        """What every captured step bakes in; replay() and replay_front() add their own."""
        cloud, m = self.cloud, self.motion
        return (int(cam_idx), subframe_indice, int(cloud.active_sh_degree), bool(m.is_optimizing()),
                bool(m.curve_random_sample), cap, self._generation, gt.data_ptr(), bool(cull), bool(dgr.WIDE_RECORDS),
                tuple(p.data_ptr() for p in cloud.hot_parameters()), bool(self.always_depth))

    def _resume(self, front, lambda_now):
        """The eager part behind a replayed front (the hook of its graph entry, 'finish').  A front recorded up to the
        forward goes on in a copy of the recorded step: what its loss and backward allocate lives until the next step,
        like an eager step's, not as long as the graph entry."""
        if front.shard is None:
            return self._finish(front)
        st = front.copy()
        self._loss_backward(st, lambda_now)
        return self._finish(st)

    def _replay_plan(self, cam_idx, subframe_indice, shard=None):
        """What replay() and replay_front() settle before they look up a graph: (K_total, the capacity key, the capacity
        quantised to ~3-6 % -- small count drifts do not force a re-capture --, tile culling); None when the step is not
        replayed (no duplicate count learnt for the view, an explicit subframe list, an empty "subframes" slice, or a view
        whose backward is faster enqueued eagerly)."""
        f = self.motion.n_subframes
        self._poll()
        K_total = f if (isinstance(subframe_indice, str) and subframe_indice == "all") else (
            int(subframe_indice) if isinstance(subframe_indice, int) else len(subframe_indice))
        k0 = 0
        if shard is not None:
            from .sharding import shard_range
            k0, k1 = shard_range(K_total, int(shard[0]), int(shard[1]))
            if k1 <= k0:
                return None
        ckey = (int(cam_idx), K_total, k0)
        cap = self._capacity(ckey) if self.speculative else None
        if cap is None or isinstance(subframe_indice, (list, tuple)) or torch.is_tensor(subframe_indice):
            return None
        cap = raster_call.round_capacity(cap)
        cull = dgr.TILE_CULL if self.tile_cull is None else bool(self.tile_cull)
        # ("subframes" sharding: the captured front ends before the backward)
        if shard is None and self._eager_is_faster(K_total, cap, cull):
            return None
        return K_total, ckey, cap, cull

    def _scalar_slot(self, ent, lambda_t, background, uniform):
        """This step's scalar block, filled in the next pinned slot of the ring (which keeps a block alive until its copy
        has run): lambda_t, the background and the alignment jitter.  Returns (block, its event)."""
        m = self.motion
        f = m.n_subframes
        slot = self._ring[self._ring_pos % len(self._ring)] if self._ring else None
        if slot is None or slot[0].numel() != ent["hyper"].numel():
            self._ring = [(torch.zeros(ent["hyper"].numel(), dtype=torch.float32).pin_memory(), torch.cuda.Event())
                          for _ in range(8)]
            self._ring_pos = 0
            slot = self._ring[0]
        self._ring_pos += 1
        hbuf, hev = slot
        hev.synchronize()                      # (recorded 8 replays ago: never waits in practice)
        hv = hbuf.numpy()
        hv[0] = float(lambda_t)
        hv[1:4] = (torch.rand(3) if background is None else background.detach().float().cpu()).numpy()   # motion.py:112-113
        if m.curve_random_sample and f > 2:                               # scene/motion.py:213-214
            hv[48:48 + f - 2] = (torch.rand(f - 2) if uniform is None else uniform.detach().float().cpu()).numpy()
        return hbuf, hev

    def _launch(self, ent, hbuf, hev, ckey, request, cap, background_dev=None, uniform_dev=None):
        """The scalar block to the graph, the replay, and the step on the pending list."""
        dev = self.cloud._xyz.device
        f = self.motion.n_subframes
        slot = self._push_scalars(ent, hbuf, dev)
        hev.record(torch.cuda.current_stream(dev))
        if background_dev is not None:               # (shared draws of a "subframes" step: device to device, stream-ordered)
            ent["hyper"][1:4].copy_(background_dev.reshape(3))
        if uniform_dev is not None and self.motion.curve_random_sample and f > 2:
            ent["hyper"][48:48 + f - 2].copy_(uniform_dev.reshape(f - 2))
        ent["graph"].replay()
        self._track(slot, True, ckey, request, cap, dev)
        self.last_capacity = cap
        self.replayed += 1

    def _capture_setup(self, cap, optimizer=None):
        """What both captures allocate OUTSIDE the capture pool before they record: the scalar block, the pinned count
        words, the status words, the drop counter, the loss kernel's work block and the gradient bucket.  Returns (ent,
        the _Capture record of these, the background and the alignment jitter as views of the scalar block)."""
        cloud, m = self.cloud, self.motion
        dev = cloud._xyz.device
        f = m.n_subframes
        if len(self._graphs) >= self.max_graphs:      # (views x subframe selections of one run; bounded all the same)
            self._graphs.pop(next(iter(self._graphs)))
        hyper = torch.zeros(self._hyper_words(f), dtype=torch.float32, device=dev)
        host = torch.zeros(8, dtype=torch.int32).pin_memory()
        self._drop_counter(dev)
        if self._release_pool:
            self._release_pool = False
            self._keep = None
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        ent = {"hyper": hyper, "host": host, "status": torch.zeros(4, dtype=torch.int32, device=dev)}
        # The gradient bucket is ONE per cloud generation for all graphs (replays never overlap and what reads the
        # gradients -- the optimiser launch at the end of a replay, a front's eager part -- has consumed them before the next
        # replay; a bucket per graph would be 236 MB per view at P = 1M, SH 3).  The loss kernel's work block is one per
        # graph: `losses` handed to the caller is a view of it and holds a replay's two values until the SAME graph is
        # replayed again (in the pool it could be another graph's scratch: all graphs share the pool).
        n_bucket = raster_call.cloud_bucket(cloud._xyz.shape[0], cloud._features_rest.shape[1]).size
        if self._bucket is None or self._bucket[0] != self._generation or self._bucket[1] != n_bucket:
            self._bucket = (self._generation, n_bucket, torch.empty(n_bucket, dtype=torch.float32, device=dev))
        ent["work"] = torch.zeros(8, dtype=torch.float32, device=dev)
        cap_args = _Capture(int(cap), host, ent["status"], hyper.data_ptr(), ent["work"], self._bucket[2])
        params = list(cloud.hot_parameters()) + (list(m.parameters()) if m.is_optimizing() else [])
        if optimizer is not None:
            optimizer.ensure_state(params)
        for p in params:
            p.grad = None
        uniform = hyper[48:48 + f - 2] if (m.curve_random_sample and f > 2) else None
        return ent, cap_args, hyper[1:4], uniform, params

    def _register(self, gkey, ent, graph):
        ent["graph"] = graph
        self._keep = None
        self._graphs[gkey] = ent
        self.captured += 1
        return ent

    def _capture_front(self, gkey, cam_idx, gt, subframe_indice, cap, ar, K_total, shard=None):
        dev = self.cloud._xyz.device
        ent, cap_args, bg, uniform, _ = self._capture_setup(cap)
        # sharded runs update the densification statistics in a launch of their own: the radii, the screen-space gradients
        # and the skip word live outside the pool too, shared by all graphs of a cloud generation
        P = self.cloud._xyz.shape[0]
        skey = (self._generation, K_total, P)
        if self._front_shared is None or self._front_shared[0] != skey:
            self._front_shared = (skey, torch.empty((K_total, P), dtype=torch.int32, device=dev),
                                  torch.empty((K_total, P, 3), dtype=torch.float32, device=dev),
                                  torch.zeros(1, dtype=torch.int32, device=dev))
        cap_args = cap_args._replace(radii=self._front_shared[1], means2D=self._front_shared[2], skipw=self._front_shared[3])
        st = _Step(cap=cap_args, request=(cam_idx, subframe_indice), gt=gt, need_blur=False, lambda_depth_tv=0.0,
                   shard=shard, ar=ar)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, pool=self._pool, capture_error_mode="thread_local"), torch.no_grad():
                # "views" sharding: up to the first collective, the reduction of the gradient bucket.  "subframes" sharding
                # (shard): that is the loss block, so the front ends with the forward.
                self._cameras(st, uniform)
                self._forward(st, bg)
                if shard is None:
                    self._loss_backward(st, 0.0)
                # the skip word to one of its own, outside the pool (as a view it would pin the whole geometry blob)
                cap_args.skipw.copy_(st.skip_flag)
                st.skip_flag = cap_args.skipw
        except RuntimeError as ex:
            raise CaptureRefused(str(ex)) from ex
        # the step's large buffers go back to the pool (the other views' captures re-use the blocks): _Step has the rules
        st.release_large(keep=() if shard is None else ("color", "depth"))
        ent["step"], ent["finish"] = st, self._resume
        return self._register(gkey, ent, graph)

    def _capture(self, gkey, cam_idx, gt, subframe_indice, cap, optimizer, tail, stats=None):
        dev = self.cloud._xyz.device
        ent, cap_args, bg, uniform, params = self._capture_setup(cap, optimizer)
        st = _Step(cap=cap_args, request=(cam_idx, subframe_indice), gt=gt, need_blur=False, lambda_depth_tv=0.0,
                   stats=stats)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=self._pool, capture_error_mode="thread_local"), torch.no_grad():
            self._cameras(st, uniform)
            self._forward(st, bg)
            self._loss_backward(st, 0.0)
            fr = self._finish(st)
            if tail is not None:
                tail(fr, ent["hyper"].data_ptr() + 4 * 8)
        # What a replay leaves behind for the host is the two loss values, the count words (pinned) and the gradients of
        # the parameters (the first and the last allocated outside the pool, by _capture_setup).  Every replay is a complete
        # step, so everything else goes back to the pool with `st` (here and in _register).
        ent["result"] = {"losses": fr["losses"], "K": fr["K"], "skip_flag_ptr": fr["skip_flag_ptr"], "blur": None,
                         "radii": None, "viewspace_grad": None, "subframes": None, "depths": None, "depth_tv": None}
        ent["grads"] = [(p, p.grad) for p in params if p.grad is not None]
        return self._register(gkey, ent, graph)

    # ------------------------------------------------------------------------------------------------- the step
    @torch.no_grad()
    def run(self, cam_idx, lambda_t, gt, background, subframe_indice="all", need_blur=False, uniform=None,
            lambda_depth_tv=0.0, shard=None, exact=False, need_depth=False, ar=None, stats=None):
        """gt: [3,H,W] ground truth of view cam_idx (already tone-mapped / noised by the caller); background: [3].
        lambda_depth_tv > 0 adds the reference's optional depth-smoothness term (train.py:150-153,
        utils/loss_utils.py:66-78): its gradient on the K depth images is formed with a few torch ops and handed to the
        rasteriser's backward as dL/ddepth; 'depth_tv' is its value.
        shard=(rank, world): "subframes" sharding (deblurgs_amd.sharding): this rank rasterises subframes
        [floor(rank K / world), floor((rank+1) K / world)) of the view; the loss block runs across the ranks
        (sharding.subframe_sharded_loss_grad: one all-reduce of the partial blur sum, one boundary frame each way), the
        gradients are this rank's PARTIAL sums (the caller adds them over the ranks; the opacity hinge is added on rank 0
        only); 'radii' / 'viewspace_grad' / 'subframes' hold the local slice, 'K' the view's subframe count.
        exact=True forces the two-phase forward (one host read) whatever has been learnt.
        need_depth=True renders the K depth images too ('depths'; implied by lambda_depth_tv > 0), else 'depths' is None.
        ar = {"chunks": G, "average": bool, "group": ...}: a sharded run's all-reduce of the per-Gaussian gradient bucket,
        overlapped with the backward's tail: the per-Gaussian half of the backward runs in G Gaussian-index
        chunks (dgs_backward_geometry) and chunk i is reduced on a side stream while chunk i + 1 computes; the caller must
        then NOT reduce the bucket again (the trajectory gradients remain its job).
        stats = (max_radii2D, xyz_gradient_accum, denom): the cloud's densification accumulators ([P] float32); the
        backward then updates them itself (DgsBackwardIO.stats_*, exactly densify_stats.add_densification_stats_subframes
        on this step's screen gradients) and 'viewspace_grad' comes back None -- the [K,P,3] gradient is never stored.
        The step is four stages on one _Step (which states what lives how long); a capture (replay, replay_front) records a
        prefix of the same stages and the eager part behind a replayed front runs the rest (_resume).
        Returns a dict: 'losses' (device float32 [2]: L1(blur, gt), smoothness -- no host read), 'blur' ([3,H,W] if
        need_blur), 'radii' [K,P] int32, 'viewspace_grad' [K,P,3], 'K', 'skip_flag_ptr' (int or None)."""
        st = _Step(request=(cam_idx, subframe_indice), gt=gt, need_blur=need_blur, lambda_depth_tv=lambda_depth_tv,
                   shard=shard, ar=ar, stats=stats)
        self._cameras(st, uniform)
        if st.K == 0:
            return self._empty_slice(st, lambda_t)
        self._forward(st, background, exact, need_depth)
        self._loss_backward(st, lambda_t)
        return self._finish(st)

    def _cameras(self, st, uniform):
        """Stage 1: alignment -> nu (all f candidates, then the requested subset) -> the K cameras -> this rank's slice of
        them ("subframes" sharding; K == 0: the caller goes to _empty_slice)."""
        L = _lib.lib()
        cloud, m = self.cloud, self.motion
        dev = cloud._xyz.device
        stream = _stream(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        f = m.n_subframes
        cam_idx, subframe_indice = st.request
        cam = st.cam = int(cam_idx)
        nu_raw = m._nu
        nu_all = st.nu_all = torch.empty(f, **f32)
        st.src = torch.empty(f, dtype=torch.int32, device=dev)
        nrow = st.nrow = nu_raw.shape[1] if nu_raw.ndim == 2 else 0
        st.raw_ptr = _ptr(nu_raw, cam * nrow) if nrow > 0 else None
        if uniform is None and m.curve_random_sample and nrow > 0:
            uniform = torch.rand(nrow, **f32)
        if not m.curve_random_sample:
            uniform = None
        st.uniform = uniform
        _lib.check(L.dgs_alignment_forward(st.raw_ptr, _ptr(uniform), f, f, _ptr(nu_all), _ptr(st.src), stream),
                   "dgs_alignment_forward")
        if isinstance(subframe_indice, str) and subframe_indice == "all":
            nu = nu_all
        else:
            if isinstance(subframe_indice, int):     # scene/motion.py:129-131 (1 selects index 0)
                st.sel = self._linspace_sel(f, subframe_indice, dev)
            else:
                st.sel = torch.as_tensor(subframe_indice, device=dev).long()
            nu = nu_all[st.sel].contiguous()
        K = nu.shape[0]

        ct_all, cr_all = m._trans._control_points, m._rot._control_points
        C = st.C = ct_all.shape[1] - 1
        row = st.row = cam * (C + 1) * 3              # this view's curve in the translation control points ...
        quat = st.quat = int(cr_all.shape[-1] == 4)   # ... and in the rotation ones ([C+1,4]: quaternion curve)
        rrow = st.rrow = cam * (C + 1) * cr_all.shape[-1]
        # (stored as a transposed view: made contiguous ONCE -- a 16-float copy kernel per step is a launch and a gap on the
        # device's timeline, 2 % of a cfg2 step)
        pm = m.ref_cam.projection_matrix
        pc = self._proj_cache
        if pc is None or pc[0] is not pm or pc[1] != pm._version or pc[2].device != dev:
            pc = self._proj_cache = (pm, pm._version, pm.to(dev, torch.float32).contiguous().clone())
        proj = st.proj = pc[2]
        view = torch.empty((K, 4, 4), **f32)
        full = torch.empty((K, 4, 4), **f32)
        campos = torch.empty((K, 3), **f32)
        _lib.check(L.dgs_pose_forward(_ptr(ct_all, row), _ptr(cr_all, rrow), _ptr(nu), _ptr(proj), C, K, quat, _ptr(view),
                                      _ptr(full), _ptr(campos), stream), "dgs_pose_forward")

        st.K_total, st.k0 = K, 0
        nu_loc = nu
        if st.shard is not None:
            from .sharding import shard_range
            st.k0, k1 = shard_range(K, int(st.shard[0]), int(st.shard[1]))
            k0 = st.k0
            view, full, campos, nu_loc = view[k0:k1], full[k0:k1], campos[k0:k1], nu[k0:k1]   # (contiguous row slices)
            K = k1 - k0
        st.view, st.full, st.campos, st.nu, st.nu_loc, st.K = view, full, campos, nu, nu_loc, K
        st.P, st.Mr = cloud._xyz.shape[0], cloud._features_rest.shape[1]
        st.H, st.W = int(m.ref_cam.image_height), int(m.ref_cam.image_width)

    def _forward(self, st, background, exact=False, need_depth=False):
        """Stage 2: the state blobs, the problem, the forward (capacity None: the exact two-phase one, one blocking read of
        the count -- also how the first capacity is learnt) and the skip word."""
        L = _lib.lib()
        cloud, m = self.cloud, self.motion
        dev = cloud._xyz.device
        f32 = dict(dtype=torch.float32, device=dev)
        cap, K, P, H, W = st.cap, st.K, st.P, st.H, st.W
        st.color = torch.empty((K, 3, H, W), **f32)
        # the depth images are rendered only if somebody reads them (the reference always renders them, and its default
        # loss, lambda_depth_tv = 0, never looks at them: train.py:150-153)
        if need_depth or self.always_depth or st.lambda_depth_tv > 0.0:
            st.depth = torch.empty((K, 1, H, W), **f32)
        st.radii = (torch.empty((K, P), dtype=torch.int32, device=dev) if (cap is None or cap.radii is None)
                    else cap.radii[:K])
        geom = st.geom = torch.empty(L.dgs_geom_state_bytes(P, K), dtype=torch.uint8, device=dev)
        st.image = torch.empty(L.dgs_image_state_bytes(W, H, K), dtype=torch.uint8, device=dev)
        st.bg = background.to(dev, torch.float32).contiguous()
        cull = dgr.TILE_CULL if self.tile_cull is None else bool(self.tile_cull)
        st.prob = raster_call.cloud_problem(cloud, K, st.view, st.full, st.campos, H, W, m.ref_cam.FoVx, m.ref_cam.FoVy,
                                            st.bg, cull, geom, st.image)
        key = (st.cam, st.K_total, st.k0)
        if cap is None:
            host = self._host_words()
            self._poll()
            capacity = self._capacity(key) if (self.speculative and not exact) else None
            st.out = raster_call.forward_out(st.color, st.depth, st.radii, host)
        else:
            host, capacity = cap.host, cap.capacity
            st.out = raster_call.forward_out(st.color, st.depth, st.radii, host, drop_counter=self._drop_counter(dev),
                                             status_dev=cap.status,
                                             status_host_indirect=cap.lambda_ptr + 16)   # words [4:6] of the scalar block
        st.R, st.binning = raster_call.forward(dev, st.prob, st.out, host, capacity)
        if cap is None:
            self._track(host, capacity is not None, key, st.request, st.R, dev)
        self.last_capacity = st.R
        if capacity is not None:
            off = raster_call.skip_word_offset(P, W, H, K)
            st.skip_ptr = geom.data_ptr() + off
            st.skip_flag = geom[off:off + 4].view(torch.int32)

    def _loss_backward(self, st, lambda_t):
        """Stage 3: the loss and the launches up to the first collective of the gradient reduction.  lambda_t is the
        scheduled weight of THIS call (a recorded step reads it from the scalar block on the device instead)."""
        L = _lib.lib()
        cloud = self.cloud
        dev = cloud._xyz.device
        stream = _stream(dev)       # (the stream of THIS call: behind a replayed front that is the caller's, not the capture's)
        f32 = dict(dtype=torch.float32, device=dev)
        cap, shard, K, K_total, P, H, W = st.cap, st.shard, st.K, st.K_total, st.P, st.H, st.W
        # ---- loss: blur, both values and dL/dsubframes in one pass (train.py:143-165 image terms)
        gtc = st.gtc = st.gt.to(dev, torch.float32).contiguous()
        blur = torch.empty((3, H, W), **f32)
        dsub = torch.empty((K, 3, H, W), **f32)
        # dgs_blur_loss_grad's work area: [l1, smooth | accumulators, counter]
        work = st.work = torch.empty(8, **f32) if cap is None else cap.work
        st.losses = work[:2]
        if cap is not None and shard is None:      # the scheduled weight is read from device memory when the replayed kernel runs
            _lib.check(L.dgs_blur_loss_grad_dev(_ptr(st.color), _ptr(gtc), K, 3, H * W, ctypes.c_void_p(cap.lambda_ptr),
                                                None, _ptr(blur), _ptr(dsub), _ptr(work), stream),
                       "dgs_blur_loss_grad_dev")
        elif shard is None:
            _lib.check(L.dgs_blur_loss_grad(_ptr(st.color), _ptr(gtc), K, 3, H * W, float(lambda_t), None, _ptr(blur),
                                            _ptr(dsub), _ptr(work), stream), "dgs_blur_loss_grad")
        else:   # the loss block across the ranks holding the view's other subframes
            from . import sharding
            dsub, l1, sm = sharding.subframe_sharded_loss_grad(st.color, gtc, K_total, float(lambda_t), self.loss_group)
            dsub = dsub.contiguous()
            st.losses = torch.stack([l1.reshape(()), sm.reshape(())]).float()
            blur = None
        st.blur, st.dsub = blur, dsub

        # ---- backward: one flat gradient bucket in optimiser-group order (as _RasterizeCloudK.backward)
        bucket = raster_call.cloud_bucket(P, st.Mr)
        flat = st.flat = torch.empty(bucket.size, **f32) if cap is None else cap.bucket
        assert flat.numel() == bucket.size
        st.g_xyz, st.g_dc, st.g_rest, st.g_op, st.g_sc, st.g_rot = bucket.views(flat, [
            (P, 3), cloud._features_dc.shape, cloud._features_rest.shape, cloud._opacity.shape, (P, 3), (P, 4)])
        if st.stats is None:
            st.g_means2D = (torch.empty((K, P, 3), **f32) if (cap is None or cap.means2D is None) else cap.means2D[:K])
        if st.lambda_depth_tv > 0.0:
            from . import losses as _losses
            # tv_loss is a mean over the view's K depth images of per-image terms (utils/loss_utils.py:66-78): a rank
            # holding K of the K_total subframes contributes K / K_total of it and needs no other rank's depths
            share = K / float(K_total)
            with torch.enable_grad():
                dleaf = st.depth.detach().requires_grad_(True)
                depth_tv = _losses.tv_loss(dleaf) * share
                g_depth, = torch.autograd.grad(float(st.lambda_depth_tv) * depth_tv, dleaf)
            st.g_depth, st.depth_tv = g_depth.contiguous(), depth_tv.detach()
            if shard is not None:
                import torch.distributed as dist
                dist.all_reduce(st.depth_tv, group=self.loss_group)   # the value only (logging); the gradient is local
        st.io, own = raster_call.backward_io(
            st.R, st.radii, dsub, st.g_depth, means3D=st.g_xyz, means2D=st.g_means2D, sh=st.g_dc,
            sh_rest=st.g_rest if st.Mr > 0 else None, opacity=st.g_op, scales=st.g_sc, rotations=st.g_rot,
            # sharded: the ranks' gradients are summed, so the hinge term is added by one of them only
            opacity_hinge_scale=self.lambda_hinge / max(P, 1) if (shard is None or int(shard[0]) == 0) else 0.0,
            stats=st.stats, stats_K_total=K_total)
        st.scratch, st.g_colors, st.g_cov3D = own["scratch"], own["colors"], own["cov3D"]
        st.g_view, st.g_proj = own["viewmatrix"], own["projmatrix"]
        # a sharded run reduces the bucket in Gaussian-index chunks, each behind its part of the per-Gaussian half (_finish)
        st.chunked = not (st.ar is None or int(st.ar.get("chunks", 1)) <= 1 or P < 512)
        if st.chunked:
            _lib.check(L.dgs_backward_composite(ctypes.byref(st.prob), ctypes.byref(st.io), stream), "dgs_backward_composite")
        else:
            _lib.check(L.dgs_backward(ctypes.byref(st.prob), ctypes.byref(st.io), stream), "dgs_backward")

    def _finish(self, st):
        """Stage 4, everything from the first collective on: a sharded run's reduction of the bucket (overlapped with the
        per-Gaussian half of the backward when `chunked`), the gradients into `.grad`, the camera gradients back to the
        control points and the alignment, the result.  `st` becomes the step that is kept until the next one."""
        L = _lib.lib()
        cloud, m = self.cloud, self.motion
        dev = cloud._xyz.device
        # (the stream of THIS call: a captured front was recorded on torch's capture stream, its eager part runs on the
        # caller's stream, behind the replay)
        stream_obj = torch.cuda.current_stream(dev)
        stream = ctypes.c_void_p(stream_obj.cuda_stream)
        f32 = dict(dtype=torch.float32, device=dev)
        ar, shard, K, P, flat, prob, io = st.ar, st.shard, st.K, st.P, st.flat, st.prob, st.io
        if st.chunked:
            from . import sharding
            if self._side is None:
                self._side = torch.cuda.Stream(device=dev)
            side = self._side
            flat.record_stream(side)
            bucket = raster_call.cloud_bucket(P, st.Mr)
            t_ar = None
            if self.time_allreduce:  # (bench.py: span of the side stream's reductions, first chunk ready -> last done)
                t_ar = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            for ci, (b0, b1) in enumerate(sharding.chunk_bounds(P, int(ar["chunks"]))):
                _lib.check(L.dgs_backward_geometry(ctypes.byref(prob), ctypes.byref(io), b0, b1, stream),
                           "dgs_backward_geometry")
                ev = torch.cuda.Event()
                ev.record(stream_obj)
                with torch.cuda.stream(side):
                    side.wait_event(ev)
                    if t_ar is not None and ci == 0:
                        t_ar[0].record(side)
                    sharding.allreduce_slices(bucket.chunk(flat, P, b0, b1), ar.get("average", False),
                                              ar.get("group"))
            _lib.check(L.dgs_backward_pose(ctypes.byref(prob), ctypes.byref(io), stream), "dgs_backward_pose")
            done = torch.cuda.Event()
            done.record(side)
            if t_ar is not None:
                t_ar[1].record(side)
                self.ar_events = (self.ar_events + [t_ar])[-256:]
            stream_obj.wait_event(done)
        elif ar is not None and P > 0:
            from . import sharding
            sharding._allreduce(flat, ar.get("average", False), ar.get("group"))
        if P == 0:
            flat.zero_()
            if st.g_means2D is not None:
                st.g_means2D.zero_()
        cloud._xyz.grad, cloud._features_dc.grad, cloud._features_rest.grad = st.g_xyz, st.g_dc, st.g_rest
        cloud._opacity.grad, cloud._scaling.grad, cloud._rotation.grad = st.g_op, st.g_sc, st.g_rot

        # ---- cameras -> control points and alignment (only while the trajectory is being optimised)
        if m.is_optimizing():
            ct_all, cr_all, nu_raw = m._trans._control_points, m._rot._control_points, m._nu
            row, rrow, f = st.row, st.rrow, m.n_subframes
            d_ct_all, d_cr_all = torch.zeros_like(ct_all), torch.zeros_like(cr_all)
            d_nu = torch.empty(K, **f32)
            pscratch = torch.empty(L.dgs_pose_scratch_bytes(K), dtype=torch.uint8, device=dev)
            _lib.check(L.dgs_pose_backward(_ptr(ct_all, row), _ptr(cr_all, rrow), _ptr(st.nu_loc), _ptr(st.proj), st.C, K,
                                           st.quat, _ptr(st.g_view), _ptr(st.g_proj), _ptr(pscratch), _ptr(d_ct_all, row),
                                           _ptr(d_cr_all, rrow), _ptr(d_nu), stream), "dgs_pose_backward")
            m._trans._control_points.grad, m._rot._control_points.grad = d_ct_all, d_cr_all
            if st.nrow > 0:
                d_raw_all = torch.zeros_like(nu_raw)
                if shard is not None:                    # this rank's slice of the view's subframe times
                    d_all = torch.zeros(st.K_total, **f32)
                    d_all[st.k0:st.k0 + K] = d_nu
                    d_nu = d_all
                if st.sel is not None:                   # gradients of the selected subframes back to all f slots
                    d_full = torch.zeros(f, **f32)
                    d_full.index_add_(0, st.sel, d_nu)
                    d_nu = d_full
                _lib.check(L.dgs_alignment_backward(st.raw_ptr, _ptr(st.uniform), f, f, _ptr(st.src), _ptr(d_nu),
                                                    _ptr(d_raw_all, st.cam * st.nrow), stream), "dgs_alignment_backward")
                m._nu.grad = d_raw_all
        self._keep = st
        return {"losses": st.losses, "blur": st.blur if st.need_blur else None, "radii": st.radii,
                "viewspace_grad": st.g_means2D, "K": st.K_total, "subframes": st.color, "depths": st.depth,
                "skip_flag_ptr": st.skip_ptr, "skip_flag": st.skip_flag, "depth_tv": st.depth_tv}

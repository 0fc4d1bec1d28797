"""What a scene does to the tile lists: the device tile-list profile (dgs_list_profile, csrc/listprof.hip).

Every speed figure of the project used to come from synthetic.make_scene's uniform layout, where each tile carries the same
list -- the one case in which "one wave64 per tile" cannot tail.  synthetic.make_scene(layout="surfaces") is a scene-shaped
load; this module is the instrument to look at either:

    list_profile(image_state, W, H, K)   per subframe and over all of them: tiles, non-empty tiles, the sum and maximum of the
                                         list lengths, 64-entry batches (the compositing kernels' unit of work), the same of
                                         `walked` (how far the forward really went down each list: the largest n_contrib of
                                         the tile's pixels) and two power-of-two histograms -- one call, two launches, no
                                         host read before the caller asks for the numbers
    ListProfile.percentiles(q)           exact percentiles of the list length over the non-empty tiles (report.order_stats:
                                         the device radix select)
    ListProfile.skew()                   max / mean, the share of the entries in tiles longer than 4 x the mean, the share
                                         of short tiles, walked / total
    profile_scene(scene, K)              a forward of a synthetic scene through the operator layer, then list_profile

The summary words are integers summed in integers: two calls give the same bytes.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .raster_call import _ptr, _stream

SCALARS = ("tiles", "nonempty", "total", "max_length", "batches", "walked_total", "walked_max", "walked_batches")
BUCKETS = 33                       # bucket 0: the value 0; bucket b >= 1: values in [2^(b-1), 2^b)
WORDS = len(SCALARS) + 2 * BUCKETS   # DGS_LIST_PROFILE_WORDS
EXACT_F32 = 1 << 24                # integers below this are exact in fp32 (percentiles go through a float copy)


def tiles_of(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def bucket_of(v):
    """The histogram bucket of a value: 0 for 0, else its bit length."""
    return int(v).bit_length()


class ProfileRow:
    """One summary row: the eight scalars as Python ints, hist_length / hist_walked as lists of 33 ints."""

    def __init__(self, words):
        words = [int(w) for w in words]
        if len(words) != WORDS:
            raise ValueError(f"a summary row has {WORDS} words")
        for name, w in zip(SCALARS, words):
            setattr(self, name, w)
        self.hist_length = words[len(SCALARS):len(SCALARS) + BUCKETS]
        self.hist_walked = words[len(SCALARS) + BUCKETS:]

    def words(self):
        return [getattr(self, n) for n in SCALARS] + self.hist_length + self.hist_walked

    def skew(self, share_long=None, share_short=None):
        """Derived figures.  share_long (the share of `total` in tiles longer than 4 x the mean over all tiles) and
        share_short (the share of the non-empty tiles with at most 64 entries) need the per-tile lengths, which a row
        does not hold: ListProfile.skew supplies them."""
        mean = self.total / self.tiles if self.tiles else 0.0
        walked_mean = self.walked_total / self.tiles if self.tiles else 0.0
        return {"mean_length": mean, "max_over_mean": self.max_length / mean if mean else 0.0,
                "share_long": share_long, "share_short": share_short,
                "walked_max_over_mean": self.walked_max / walked_mean if walked_mean else 0.0,
                "walked_over_total": self.walked_total / self.total if self.total else 0.0,
                "walked_batches_over_batches": self.walked_batches / self.batches if self.batches else 0.0}

    def as_dict(self):
        d = {n: getattr(self, n) for n in SCALARS}
        d["hist_length"], d["hist_walked"] = list(self.hist_length), list(self.hist_walked)
        return d


class ListProfile(ProfileRow):
    """The result of list_profile: the row over all subframes (this object's own fields), `rows` (one ProfileRow per
    subframe), `summary` (the u64 [K+1, WORDS] words as a host int64 array) and, when asked for, `per_tile`: the int32
    [K, T, 2] device tensor of (length, walked) -- the u32 words of the library, values below 2^31."""

    def __init__(self, summary, K, T, per_tile=None):
        summary = np.asarray(summary).reshape(K + 1, WORDS)
        super().__init__(summary[K])
        self.K, self.T = K, T
        self.summary = summary
        self.rows = [ProfileRow(summary[k]) for k in range(K)]
        self.per_tile = per_tile

    def _lengths(self):
        if self.per_tile is None:
            raise ValueError("this figure needs the per-tile lengths: call list_profile(..., per_tile=True)")
        return self.per_tile[..., 0].reshape(-1)

    def percentiles(self, q):
        """Exact percentiles (numpy's "lower" method: an element of the data, rank floor((n - 1) q / 100)) of the list
        length over the NON-EMPTY tiles of all subframes, as Python ints, for up to 4 percentages.  The device radix
        select (report.order_stats) on a float copy of all lengths: the empty tiles sort first, so the rank among all
        tiles is the number of empty tiles + the rank among the non-empty ones.  Lengths of 2^24 and more are not exact in
        fp32 and are refused."""
        from . import report
        q = [float(v) for v in q]
        if not q or len(q) > 4 or any(not 0.0 <= v <= 100.0 for v in q):
            raise ValueError("percentiles takes 1..4 percentages in [0, 100]")
        if self.max_length >= EXACT_F32:
            raise ValueError(f"a list of {self.max_length} entries is not exact in fp32 (limit 2^24): no percentiles")
        if self.nonempty == 0:
            raise ValueError("every tile is empty: no percentiles")
        empty = self.tiles - self.nonempty
        ranks = [empty + int(math.floor((self.nonempty - 1) * v / 100.0)) for v in q]
        x = self._lengths().to(torch.float32)
        return [int(v) for v in report.order_stats(x, ranks).cpu().tolist()]

    def skew(self):
        """max_length / mean, the share of `total` in tiles longer than 4 x the mean over all tiles, the share of the
        non-empty tiles with at most 64 entries, walked_total / total (and the same in batches).  The two shares need the
        per-tile lengths (per_tile=True); without them they are None."""
        share_long = share_short = None
        if self.per_tile is not None and self.total:
            length = self._lengths().to(torch.int64)
            share_long = length[length * self.tiles > 4 * self.total].sum().item() / self.total
            share_short = ((length > 0) & (length <= 64)).sum().item() / self.nonempty
        return ProfileRow.skew(self, share_long, share_short)

    def as_dict(self):
        d = ProfileRow.as_dict(self)
        d["subframes"] = [r.as_dict() for r in self.rows]
        return d


def list_profile(image_state, W, H, K, forward_only=False, per_tile=False, stream=None):
    """Runs dgs_list_profile on the image blob of a forward of K subframes of W x H pixels (the uint8 device tensor the
    forward filled).  forward_only: the blob is a forward-only one -- the ranges sit at offset 0 and there is no n_contrib,
    so the walked figures are 0.  per_tile: also return the [K, T, 2] (length, walked) device tensor.  stream: a raw
    stream handle (default: the current stream of the blob's device).  One blocking read of the summary at the end."""
    if not torch.is_tensor(image_state) or image_state.device.type != "cuda" or image_state.dtype != torch.uint8:
        raise RuntimeError("list_profile takes the image blob of a forward: a uint8 tensor on a HIP device (no CPU fallback)")
    L = _lib.lib()
    W, H, K = int(W), int(H), int(K)
    T = tiles_of(W, H)
    device = image_state.device
    if forward_only:
        need, off_ranges, off_contrib = L.dgs_image_state_bytes_forward_only(W, H, K), 0, None
    else:
        lay = _lib.layout(1, W, H, K, 0)          # (the image blob's layout depends on W, H, K alone)
        need, off_ranges, off_contrib = lay.image_total, lay.ranges, lay.n_contrib
    if image_state.numel() < need:
        raise ValueError(f"the image blob holds {image_state.numel()} bytes, a {'forward-only ' if forward_only else ''}"
                         f"forward of K={K}, {W}x{H} fills {need}")
    base = image_state.data_ptr()
    tiles = torch.empty((K, T, 2), dtype=torch.int32, device=device) if per_tile else None
    summary = torch.empty((K + 1, WORDS), dtype=torch.int64, device=device)
    tmp = torch.empty(max(L.dgs_list_profile_tmp_bytes(W, H, K), 8), dtype=torch.uint8, device=device)
    _lib.check(L.dgs_list_profile(ctypes.c_void_p(base + off_ranges),
                                  None if off_contrib is None else ctypes.c_void_p(base + off_contrib), W, H, K,
                                  _ptr(tiles), _ptr(summary), _ptr(tmp), _stream(device) if stream is None else stream),
               "dgs_list_profile")
    return ListProfile(summary.cpu().numpy(), K, T, tiles)


def profile_scene(scene, K, tile_cull=True, per_tile=True, forward_only=False):
    """A forward of the first K subframes of a synthetic scene (synthetic.make_scene) through the operator layer, with or
    without tile culling, then list_profile.  The returned ListProfile carries `.state`: R (the duplicates the lists hold),
    the radii [K,P] and the geometry / binning / image blobs of the forward."""
    from . import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = dgr.GaussianRasterizationSettings(
        image_height=scene["H"], image_width=scene["W"], tanfovx=scene["tanfovx"], tanfovy=scene["tanfovy"],
        bg=t(scene["bg"]), scale_modifier=scene["scale_modifier"], z_near=scene["z_near"], z_far=scene["z_far"],
        use_sigmoid=False, sh_degree=scene["sh_degree"], campos=t(scene["campos"][:K]), prefiltered=False, debug=False)
    old = dgr.TILE_CULL
    dgr.TILE_CULL = bool(tile_cull)
    try:
        with torch.no_grad():
            R, color, depth, radii, geom, binning, image = dgr._forward_impl(
                K, t(scene["means3D"]), t(scene["sh"]), None, t(scene["opacities"]).reshape(-1), t(scene["scales"]),
                t(scene["rotations"]), None, t(scene["viewmatrix"][:K]), t(scene["projmatrix"][:K]),
                t(scene["campos"][:K]), rs, forward_only=forward_only)
    finally:
        dgr.TILE_CULL = old
    prof = list_profile(image, scene["W"], scene["H"], K, forward_only=forward_only, per_tile=per_tile)
    prof.state = dict(R=int(R), tile_cull=bool(tile_cull), radii=radii, geom=geom, binning=binning, image=image)
    return prof

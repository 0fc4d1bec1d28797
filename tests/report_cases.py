"""Inputs and numpy restatements shared by tests/test_report_host.py and tests/test_gpu_report.py (no test lives here)."""
import numpy as np

BAND = 1e-3
PERCENTILE_NS = (1, 2, 3, 63, 257, 1000, 70_001, 600_001)
PERCENTILE_QS = (0.0, 1.0, 37.5, 50.0, 99.0)
SCALES = (1.0, 1e-3, 100.0)


def normal_with_ties(n, scale, seed=0):
    rng = np.random.default_rng(seed + n)
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    if n > 3:
        x[::7] = x[3]
    return x


def percentile_plan(n, q):
    """What dgs_percentiles' host side computes (csrc/report.hip), restated: (i, i_above, g) of numpy's linear method for
    n values -- the virtual index v = (n - 1) * (q / 100) in float64, its floor, the neighbour above and the fraction
    v - i.  From v = n - 1 on numpy takes the last element for both neighbours and forms the weight from the index -1 it
    has put in the floor's place: g = v + 1 (the interpolation then returns the last element itself)."""
    v = float(n - 1) * (float(q) / 100.0)
    if v >= n - 1:
        return n - 1, n - 1, v + 1.0
    i = int(np.floor(v))
    return i, i + 1, v - float(i)


def percentile_restated(sorted_x, q):
    """numpy's linear percentile of a SORTED float32 array, restated: the virtual index in float64, the two neighbours, a
    float32 difference, the float64 interpolation in the form numpy chooses by the weight."""
    i, above, g = percentile_plan(sorted_x.size, q)
    a, b = np.float32(sorted_x[i]), np.float32(sorted_x[above])
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(b - a)
        r = np.float64(a) + np.float64(d) * np.float64(g)
        if g >= 0.5:
            r = np.float64(b) - np.float64(d) * (np.float64(1.0) - np.float64(g))
    return np.float64(r)


def sort_like_device(x):
    """np.sort(x) with -0.0 in front of +0.0 (numpy holds the two equal and keeps them as they came) and every NaN last:
    the order of dgs_order_stats' keys."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    key = np.where(np.isnan(x), np.uint32(0xFFFFFFFF), key)
    return np.asarray(x, dtype=np.float32)[np.argsort(key, kind="stable")]


def same_bits_or_zeros(a, b):
    """same_bits, but a -0.0 may stand for 0.0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)) | ((a == 0.0) & (b == 0.0))).all())


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def order_inputs(n, seed=0):
    """name -> float32 [n]: what a radix select over float keys can get wrong."""
    rng = np.random.default_rng(1000 + seed + n)
    out = {f"normal x {s:g}": normal_with_ties(n, s, seed) for s in SCALES}
    out["all equal"] = np.full(n, 0.375, dtype=np.float32)
    out["all negative"] = -np.abs(normal_with_ties(n, 1.0, seed + 1)) - np.float32(1e-3)
    x = normal_with_ties(n, 1.0, seed + 2)
    x[rng.integers(0, n, max(n // 9, 1))] = np.inf
    x[rng.integers(0, n, max(n // 11, 1))] = -np.inf
    out["with infinities"] = x
    x = normal_with_ties(n, 1.0, seed + 3)
    x[rng.integers(0, n, max(n // 3, 1))] = 0.0
    x[rng.integers(0, n, max(n // 3, 1))] = -0.0
    out["with both zeros"] = x
    x = normal_with_ties(n, 1e-3, seed + 4)
    idx = rng.integers(0, n, max(n // 2, 1))
    x[idx] = (rng.integers(-(1 << 22), 1 << 22, idx.size).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    out["with denormals"] = x
    x = normal_with_ties(n, 1.0, seed + 5)
    x[rng.integers(0, n, max(n // 5, 1))] = np.nan
    if n > 2:
        x[1] = -np.nan
    out["with NaNs"] = x
    return out


def ranks_of(n):
    return [0, n - 1, (n - 1) // 2, int((n - 1) * 0.99)]


def frames_input(K, H, W, seed):
    """uniform in [-0.15, 1.15] with sprinkled exact 0, 1, k/255, +-inf and NaN (as tests/test_gpu_render_path.py draws it)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.15, 1.15, (K, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    m = max(n // 12, 6)
    pos = rng.permutation(n)[:6 * m].reshape(6, -1) if n >= 6 * m else rng.integers(0, n, (6, m))
    flat[pos[0]] = 0.0
    flat[pos[1]] = 1.0
    flat[pos[2]] = (rng.integers(0, 256, pos[2].size) / 255.0).astype(np.float32)
    flat[pos[3][: max(m // 4, 1)]] = np.inf
    flat[pos[4][: max(m // 4, 1)]] = -np.inf
    flat[pos[5][: max(m // 4, 1)]] = np.nan
    return x


def gt_input(G, H, W, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, 1.0, (G, 3, H, W)).astype(np.float32)
    flat = g.reshape(-1)
    flat[rng.integers(0, flat.size, max(flat.size // 10, 2))] = (rng.integers(0, 256, max(flat.size // 10, 2)) / 255.0) \
        .astype(np.float32)
    flat[0], flat[-1] = 0.0, 1.0
    return g


def sequential_mean(x):
    """(((x_0 + x_1) + ...) + x_{K-1}) / (float)K in float32, [3,H,W]."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = x[0].copy()
        for k in range(1, x.shape[0]):
            s = s + x[k]
        return (s / np.float32(x.shape[0])).astype(np.float32)


def rounded_bytes(y):
    """save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8) in float32, NCHW -> NHWC; a NaN gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = y.astype(np.float32) * np.float32(255.0)
        t = t + np.float32(0.5)
        t = np.where(np.isnan(t), np.float32(0.0), t)
        return np.ascontiguousarray(np.clip(t, 0.0, 255.0).astype(np.uint8).transpose(0, 2, 3, 1))


def l1_error(gt, y):
    """((|gt_r - y_r| + |gt_g - y_g|) + |gt_b - y_b|) / 3.0f in float32: [G,3,H,W] twice -> [G,H,W]."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(gt.astype(np.float32) - y.astype(np.float32))
        return ((a[:, 0] + a[:, 1]) + a[:, 2]) / np.float32(3.0)


def gamma64(x32, eps, bound):
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x32.astype(np.float64) - bound) / (1.0 - 2.0 * bound)
        return np.maximum(u, eps) ** (1.0 / 2.2)


def band_compare(got, v64, inside, what):
    """tests/test_gpu_render_path.py's band rule (copied): got are integer levels, v64 the float64 value whose floor is
    expected (already clipped to its range), inside where the unclipped quantity lies strictly inside its range.  A value
    within BAND of an integer may come out one level off, every other value must be equal; returns the in-band share,
    which must not exceed 1 %."""
    want = np.floor(v64).astype(np.int64)
    band = inside & (np.abs(v64 - np.rint(v64)) < BAND)
    diff = got.astype(np.int64) - want
    outside_bad = (diff != 0) & ~band
    share = float(band.mean())
    print(f"{what}: {band.sum()} of {band.size} values in the band ({100 * share:.3f} %), {int((diff != 0).sum())} differ, "
          f"{int(outside_bad.sum())} of them outside the band")
    assert not outside_bad.any(), (what, v64[outside_bad][:5], got[outside_bad][:5])
    assert (np.abs(diff[band]) <= 1).all(), what
    assert share <= 0.01, (what, share)
    return share


def colorize_restated(x, lo, hi, lut):
    """colorize_np after its range, in float64 (numpy 2's promotion): uint8 [...,3]; hi == lo or a NaN gives zeros."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    if not hi != lo:
        return np.zeros(x64.shape + (3,), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        d = (np.clip(x64, lo, hi) - lo) / (hi - lo)
        bad = np.isnan(d)
        idx = np.minimum((np.where(bad, 0.0, d) * 256.0).astype(np.int64), 255)
    out = np.asarray(lut)[idx][..., :3].copy()
    out[bad] = 0
    return out


def colorize_reference(x, lut):
    """utils/colorize.py's default path with numpy itself: np.percentile(x, (1, 100)), vmax += 1e-6, then the chain."""
    vmin, vmax = np.percentile(np.asarray(x, dtype=np.float32), (1, 100))
    vmax += 1e-6
    return colorize_restated(x, vmin, vmax, lut)

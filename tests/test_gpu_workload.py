"""GPU tests of the scene-shaped workload: the device tile-list profile (dgs_list_profile, deblurgs_amd/workload.py)
against numpy on constructed arrays and against the real forward's state, parity of the rasteriser on a `surfaces` scene
(synthetic.make_scene(layout="surfaces")) with the existing helpers and bars, and long lists / big rectangles end to end."""
import ctypes

import numpy as np
import pytest

from helpers import hip_forward_state, synthetic, tile_cull
from test_gpu_parity import (DEPTH_TOL, GRAD_KEYS, IMG_TOL, _check_binning_bits, _check_preprocess_bits, _grads,
                             sharp_backward_check)

pytestmark = pytest.mark.gpu

SPECIAL_LENGTHS = (0, 1, 63, 64, 65, 4096, 1 << 20)
SENTINEL = 0xFFFFFFF0          # a value that is wrong wherever it is read: above every length


# ------------------------------------------------------------------------------------- numpy statement of the profile
def _bucket(v):
    return int(v).bit_length()


def numpy_profile(ranges, n_contrib, W, H, K):
    """(per_tile [K,T,2], summary [K+1, WORDS]) as the header words them.  ranges [K,T,2]; n_contrib [K,H,W] or None."""
    from deblurgs_amd import workload
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    per_tile = np.zeros((K, T, 2), np.int64)
    per_tile[..., 0] = ranges[..., 1].astype(np.int64) - ranges[..., 0].astype(np.int64)
    if n_contrib is not None:
        for k in range(K):
            for t in range(T):
                ty, tx = divmod(t, gx)
                per_tile[k, t, 1] = n_contrib[k, ty * 16:min(ty * 16 + 16, H), tx * 16:min(tx * 16 + 16, W)].max()
    summary = np.zeros((K + 1, workload.WORDS), np.int64)
    for row, sel in [(k, per_tile[k]) for k in range(K)] + [(K, per_tile.reshape(-1, 2))]:
        length, walked = sel[:, 0], sel[:, 1]
        summary[row, :8] = [length.size, (length > 0).sum(), length.sum(), length.max(), ((length + 63) // 64).sum(),
                            walked.sum(), walked.max(), ((walked + 63) // 64).sum()]
        for v in length:
            summary[row, 8 + _bucket(v)] += 1
        for v in walked:
            summary[row, 8 + 33 + _bucket(v)] += 1
    return per_tile, summary


def _constructed(W, H, K, seed):
    """An image-blob-shaped device buffer [sentinel | n_contrib | sentinel | ranges | sentinel] with list lengths that
    include SPECIAL_LENGTHS and a random n_contrib <= the tile's length on every pixel inside the image."""
    import torch
    rng = np.random.default_rng(seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    length = rng.integers(0, 300, size=K * T).astype(np.int64)
    spots = rng.permutation(K * T)[:len(SPECIAL_LENGTHS)] if K * T >= len(SPECIAL_LENGTHS) else np.arange(K * T)
    length[spots] = np.asarray(SPECIAL_LENGTHS)[-len(spots):]
    start = np.concatenate([[0], np.cumsum(length)[:-1]]) + 17
    assert start[-1] + length[-1] < 2 ** 32
    ranges = np.stack([start, start + length], axis=1).astype(np.uint32).reshape(K, T, 2)
    n_contrib = np.zeros((K, H, W), np.uint32)
    for k in range(K):
        for t in range(T):
            ty, tx = divmod(t, gx)
            h, w = min(ty * 16 + 16, H) - ty * 16, min(tx * 16 + 16, W) - tx * 16
            n_contrib[k, ty * 16:ty * 16 + h, tx * 16:tx * 16 + w] = rng.integers(0, length[k * T + t] + 1, size=(h, w))
    pad = 64       # u32 words of sentinel around each array (a read past a ragged edge lands in one of them or in the
    #                next image row, whose values belong to ANOTHER tile: numpy_profile would then disagree)
    off_c, off_r = pad, 2 * pad + n_contrib.size + (n_contrib.size & 1)     # (ranges are read as 8-byte pairs)
    words = np.full(off_r + ranges.size + pad, SENTINEL, np.uint32)
    words[off_c:off_c + n_contrib.size] = n_contrib.reshape(-1)
    words[off_r:off_r + ranges.size] = ranges.reshape(-1)
    buf = torch.from_numpy(words.view(np.int32)).cuda()
    return dict(buf=buf, off_c=off_c, off_r=off_r, ranges=ranges, n_contrib=n_contrib, T=T, length=length)


def _run(c, W, H, K, with_contrib=True, want_tiles=True):
    import torch
    from deblurgs_amd import _lib, workload
    L = _lib.lib()
    base = c["buf"].data_ptr()
    tiles = torch.full((K, c["T"], 2), -3, dtype=torch.int32, device="cuda") if want_tiles else None
    summary = torch.full((K + 1, workload.WORDS), -5, dtype=torch.int64, device="cuda")
    nbytes = L.dgs_list_profile_tmp_bytes(W, H, K)
    assert nbytes > 0
    tmp = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")      # dirty, with a guard behind it
    rc = L.dgs_list_profile(ctypes.c_void_p(base + 4 * c["off_r"]),
                            ctypes.c_void_p(base + 4 * c["off_c"]) if with_contrib else None, W, H, K,
                            None if tiles is None else ctypes.c_void_p(tiles.data_ptr()),
                            ctypes.c_void_p(summary.data_ptr()), ctypes.c_void_p(tmp.data_ptr()),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.dgs_last_error()
    torch.cuda.synchronize()
    assert (tmp[nbytes:] == 0x5A).all(), "wrote past dgs_list_profile_tmp_bytes"
    return None if tiles is None else tiles.cpu().numpy().view(np.uint32).astype(np.int64), summary.cpu().numpy()


@pytest.mark.parametrize("W,H,K", [(70, 50, 2), (9, 7, 1), (530, 20, 3)])
def test_profile_equals_numpy_on_constructed_lists(gpu, W, H, K):
    """70 x 50: 5 x 4 tiles, ragged on both edges, K = 2, lengths 0, 1, 63, 64, 65, 4096 and 2^20 among them.  9 x 7: one
    tile, K = 1.  530 x 20: 34 x 2 = 68 tiles, more than one block per subframe and a last block that is not full."""
    c = _constructed(W, H, K, seed=W)
    if K * c["T"] >= len(SPECIAL_LENGTHS):
        assert set(SPECIAL_LENGTHS) <= set(c["length"].tolist())
    want_tiles, want_summary = numpy_profile(c["ranges"], c["n_contrib"], W, H, K)
    tiles, summary = _run(c, W, H, K)
    assert np.array_equal(tiles, want_tiles)
    assert np.array_equal(summary, want_summary)
    assert summary[K, 0] == K * c["T"] and summary[K, 8:41].sum() == K * c["T"] and summary[K, 41:].sum() == K * c["T"]
    # per_tile NULL: the same summary; a second call: the same bytes
    _, again = _run(c, W, H, K, want_tiles=False)
    assert np.array_equal(again, summary)
    # n_contrib NULL: the walked columns are zero, the rest is unchanged
    tiles0, summary0 = _run(c, W, H, K, with_contrib=False)
    want_tiles0, want_summary0 = numpy_profile(c["ranges"], None, W, H, K)
    assert np.array_equal(tiles0, want_tiles0) and np.array_equal(summary0, want_summary0)
    assert not tiles0[..., 1].any() and np.array_equal(tiles0[..., 0], tiles[..., 0])
    assert np.array_equal(summary0[:, :5], summary[:, :5]) and np.array_equal(summary0[:, 8:41], summary[:, 8:41])
    assert not summary0[:, 5:8].any() and (summary0[:, 41] == summary0[:, 0]).all() and not summary0[:, 42:].any()


def test_profile_call_can_be_captured_and_replayed(gpu):
    """No host synchronisation, no allocation: the two launches go into a captured graph; a replay profiles what the
    buffers hold THEN."""
    import torch
    from deblurgs_amd import _lib, workload
    L = _lib.lib()
    W, H, K = 70, 50, 2
    c = _constructed(W, H, K, seed=11)
    base = c["buf"].data_ptr()
    tiles = torch.zeros((K, c["T"], 2), dtype=torch.int32, device="cuda")
    summary = torch.zeros((K + 1, workload.WORDS), dtype=torch.int64, device="cuda")
    tmp = torch.zeros(L.dgs_list_profile_tmp_bytes(W, H, K), dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rc = L.dgs_list_profile(ctypes.c_void_p(base + 4 * c["off_r"]), ctypes.c_void_p(base + 4 * c["off_c"]), W, H, K,
                                ctypes.c_void_p(tiles.data_ptr()), ctypes.c_void_p(summary.data_ptr()),
                                ctypes.c_void_p(tmp.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.dgs_last_error()
    graph.replay()
    torch.cuda.synchronize()
    want_tiles, want_summary = numpy_profile(c["ranges"], c["n_contrib"], W, H, K)
    assert np.array_equal(tiles.cpu().numpy(), want_tiles) and np.array_equal(summary.cpu().numpy(), want_summary)
    # other contents in the same buffers: every list one entry longer, nothing walked
    ranges2 = c["ranges"].copy()
    ranges2[..., 1] += 1
    words = c["buf"].cpu().numpy().view(np.uint32).copy()
    words[c["off_r"]:c["off_r"] + ranges2.size] = ranges2.reshape(-1)
    words[c["off_c"]:c["off_c"] + c["n_contrib"].size] = 0
    c["buf"].copy_(torch.from_numpy(words.view(np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    want_tiles, want_summary = numpy_profile(ranges2, np.zeros_like(c["n_contrib"]), W, H, K)
    assert np.array_equal(tiles.cpu().numpy(), want_tiles) and np.array_equal(summary.cpu().numpy(), want_summary)


def test_profile_refuses_bad_arguments(gpu):
    import torch
    from deblurgs_amd import _lib, workload
    L = _lib.lib()
    c = _constructed(70, 50, 2, seed=3)
    summary = torch.full((3, workload.WORDS), -5, dtype=torch.int64, device="cuda")
    tmp = torch.zeros(L.dgs_list_profile_tmp_bytes(70, 50, 2), dtype=torch.uint8, device="cuda")
    r = ctypes.c_void_p(c["buf"].data_ptr() + 4 * c["off_r"])
    s, t, st = ctypes.c_void_p(summary.data_ptr()), ctypes.c_void_p(tmp.data_ptr()), ctypes.c_void_p(0)
    for args, word in (((r, None, 70, 50, 0, None, s, t, st), "K"), ((None, None, 70, 50, 2, None, s, t, st), "null"),
                       ((r, None, 70, 50, 2, None, None, t, st), "null"), ((r, None, 70, 50, 2, None, s, None, st), "null"),
                       ((r, None, 0, 50, 2, None, s, t, st), "empty"), ((r, None, 70, 50, 129, None, s, t, st), "K"),
                       ((ctypes.c_void_p(r.value + 4), None, 70, 50, 2, None, s, t, st), "aligned")):
        assert L.dgs_list_profile(*args) != 0
        msg = L.dgs_last_error().decode()
        assert "list_profile" in msg and word in msg, msg
    assert L.dgs_list_profile_tmp_bytes(70, 50, 0) == 0 and L.dgs_list_profile_tmp_bytes(0, 50, 1) == 0
    torch.cuda.synchronize()
    assert (summary == -5).all(), "a refused call must not enqueue anything"
    with pytest.raises(RuntimeError):
        workload.list_profile(torch.zeros(64, dtype=torch.uint8), 70, 50, 2)
    with pytest.raises(ValueError):
        workload.list_profile(torch.zeros(64, dtype=torch.uint8, device="cuda"), 70, 50, 2)


# ------------------------------------------------------------------------------------------- against the real forward
def surfaces_scene(P=4000, W=170, H=106, K=2, seed=0):
    return synthetic.make_scene(P, W, H, K=K, seed=seed, layout="surfaces", layout_args=dict(n_surfaces=6))


@pytest.mark.parametrize("cull", [False, True])
def test_profile_of_a_real_forward(gpu, cull):
    """Surfaces scene, 170 x 106 (11 x 7 tiles, ragged on both edges), K = 2: the profile of the forward's own image blob
    against the state hip_forward_state reads back, and against the forward-only blob."""
    from deblurgs_amd import workload
    sc = surfaces_scene()
    K, W, H = 2, sc["W"], sc["H"]
    st = hip_forward_state(sc, K, cull=cull)
    prof = workload.profile_scene(sc, K, tile_cull=cull)
    assert prof.state["R"] == st["R"]
    tiles = prof.per_tile.cpu().numpy().astype(np.int64)
    assert np.array_equal(tiles[..., 0], st["ranges"][..., 1].astype(np.int64) - st["ranges"][..., 0].astype(np.int64))
    want_tiles, want_summary = numpy_profile(st["ranges"], st["n_contrib"].reshape(K, H, W), W, H, K)
    assert np.array_equal(tiles, want_tiles)
    assert np.array_equal(prof.summary, want_summary)
    assert prof.total == st["R"] and prof.tiles == K * st["T"] and sum(r.total for r in prof.rows) == st["R"]
    assert prof.walked_max <= prof.max_length and 0 < prof.walked_total <= prof.total
    assert prof.words() == [int(v) for v in want_summary[K]]
    # two calls on the same blob: identical bytes
    again = workload.list_profile(prof.state["image"], W, H, K, per_tile=True)
    assert again.summary.tobytes() == prof.summary.tobytes()
    assert again.per_tile.cpu().numpy().tobytes() == prof.per_tile.cpu().numpy().tobytes()
    # the forward-only blob (ranges at offset 0, no n_contrib): the same lengths
    fo = workload.profile_scene(sc, K, tile_cull=cull, forward_only=True)
    assert np.array_equal(fo.per_tile.cpu().numpy()[..., 0], tiles[..., 0]) and not fo.per_tile[..., 1].any().item()
    assert fo.words()[:5] == prof.words()[:5] and fo.hist_length == prof.hist_length and fo.walked_total == 0
    # percentiles and skew against numpy on the per-tile lengths
    length = tiles[..., 0].reshape(-1)
    nonempty = np.sort(length[length > 0])
    q = (0.0, 50.0, 90.0, 100.0)
    assert prof.percentiles(q) == [int(nonempty[int(np.floor((nonempty.size - 1) * v / 100.0))]) for v in q]
    sk = prof.skew()
    mean = length.sum() / length.size
    assert sk["max_over_mean"] == pytest.approx(length.max() / mean)
    assert sk["share_long"] == pytest.approx(length[length > 4 * mean].sum() / length.sum())
    assert sk["share_short"] == pytest.approx((nonempty <= 64).sum() / nonempty.size)
    assert sk["walked_over_total"] == pytest.approx(tiles[..., 1].sum() / length.sum())


# ------------------------------------------------------------------------------------------- parity on the new scene
@pytest.fixture(scope="module")
def surfaces_states(gpu):
    from helpers import OracleRun
    sc = surfaces_scene()
    K = sc["K"]
    run = OracleRun(sc, K, exact=True)        # the exempt set, capped at max(2e-4 H W, 4) per subframe (helpers)
    return sc, hip_forward_state(sc, K), run


def test_surfaces_scene_forward_parity(surfaces_states):
    """Integers bit-exact on the reference lists; images within 1e-4 off the (capped) exempt set; the tile-culled forward
    gives the same bits."""
    sc, hip, run = surfaces_states
    _check_preprocess_bits(sc, hip, run.states)
    _check_binning_bits(sc, hip, run.states)
    for k, o in enumerate(run.states):
        ex = run.unstable[k]
        print(f"[surfaces k={k}] exempt {int(ex.sum())} of {ex.size} pixels")
        keep = ~ex
        s = keep.reshape(-1)
        assert np.array_equal(hip["n_contrib"][k][s], o["n_contrib"][s]), f"n_contrib k={k}"
        assert np.abs(hip["final_T"][k][s] - o["final_T"][s]).max() <= 1e-5, f"final_T k={k}"
        dc = np.abs(hip["color"][k] - o["color"]).max(axis=0)
        dd = np.abs(hip["depth"][k][0] - o["depth"][0]) / sc["z_far"]
        assert dc[keep].max() <= IMG_TOL, f"colour k={k}: {dc[keep].max()}"
        assert dd[keep].max() <= DEPTH_TOL, f"depth k={k}: {dd[keep].max()}"
    cul = hip_forward_state(sc, sc["K"], cull=True)
    for key in ("radii", "color", "depth", "final_T"):
        assert np.array_equal(cul[key], hip[key]), key
    assert cul["R"] < hip["R"]


@pytest.mark.parametrize("depth", [True, False])
def test_surfaces_scene_backward_parity(gpu, depth):
    """assert_grads_close at its defaults (through test_gpu_parity.sharp_backward_check: OracleRun(exact=True) at its
    default cap), then the same gradients bit for bit with and without tile culling."""
    from helpers import hip_forward_backward
    sc = surfaces_scene()
    K = sc["K"]
    sharp_backward_check(sc, K, depth=depth)
    gC, gD = _grads(sc, K, depth=depth)
    with tile_cull(False):
        a = hip_forward_backward(sc, K, gC, gD)
    with tile_cull(True):
        b = hip_forward_backward(sc, K, gC, gD)
    for key in GRAD_KEYS + ["color", "depth"]:
        assert np.array_equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ long lists end to end
def test_long_lists_and_big_rectangles_end_to_end(gpu):
    """Surfaces scene P = 62,500 at 480 x 270, K = 3, tile culling on: a list above 1000 entries, Gaussians whose rectangle
    covers more than 64 tiles -- the `big` record of the tile cull (cull_rec word 0, bit 31) -- and a second run with
    identical bytes."""
    from deblurgs_amd import _lib, workload
    sc = synthetic.make_scene(62_500, 480, 270, K=3, seed=0, layout="surfaces")
    K, P = 3, sc["P"]
    prof = workload.profile_scene(sc, K)
    print("[long lists]", {n: getattr(prof, n) for n in workload.SCALARS}, prof.skew())
    assert prof.max_length > 1000
    assert prof.total == prof.state["R"] and prof.tiles == K * workload.tiles_of(480, 270)
    lay = _lib.layout(P, 480, 270, K, prof.state["R"])
    geom = prof.state["geom"]
    touched = geom[lay.tiles_touched:lay.tiles_touched + 4 * K * P].cpu().numpy().view(np.uint32)
    rec = geom[lay.cull_rec:lay.cull_rec + 16 * K * P].cpu().numpy().view(np.uint32).reshape(K * P, 4)
    big = touched > 64
    assert big.sum() >= 1, "no Gaussian covers more than 64 tiles"
    assert ((rec[:, 0] >> 31) == big).all(), "cull_rec bit 31 must mark exactly the rectangles of more than 64 tiles"
    again = workload.profile_scene(sc, K)
    assert again.summary.tobytes() == prof.summary.tobytes()
    assert again.per_tile.cpu().numpy().tobytes() == prof.per_tile.cpu().numpy().tobytes()
    assert again.state["R"] == prof.state["R"]

"""GPU tests of the test-pose seeding (deblurgs_amd/registration.py, csrc/register.hip).  The two kernels are integer
arithmetic: every comparison with the dozen lines of numpy below is exact equality.  The seeds are planted: a test image
that IS the render at a candidate (or at a lattice pose around one) scores 0 there, because render_group is bit-identical
per slot and both images go through the same 8-bit finish."""
import numpy as np
import pytest

from deblurgs_amd import synthetic

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ numpy references
def box_ref(x, s):
    """uint8 [G,H,W,3] -> uint32 [G,pitch]: the packed s x s box means, pad dwords zero."""
    G, H, W, _ = x.shape
    h, w = H // s, W // s
    sums = x[:, :h * s, :w * s].reshape(G, h, s, w, s, 3).astype(np.uint32).sum(axis=(2, 4))
    c = (sums + (s * s) // 2) // (s * s)
    out = np.zeros((G, (h * w + 3) & ~3), dtype=np.uint32)
    out[:, :h * w] = (c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)).reshape(G, h * w)
    return out


def sad_ref(a, b):
    """uint32 [na,L], [nb,L] -> int64 [na,nb]: the sum of absolute differences over all four bytes of every dword."""
    a8, b8 = a.view(np.uint8).astype(np.int16), b.view(np.uint8).astype(np.int16)
    return np.array([[np.abs(x - y).sum(dtype=np.int64) for y in b8] for x in a8], dtype=np.int64)


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def _random_words(rng, n, L):
    return rng.integers(0, 2 ** 32, size=(n, L), dtype=np.uint64).astype(np.uint32)      # all four bytes live


# ------------------------------------------------------------------------------------------------ box_reduce_u8
BOX_CASES = [(1, 1, 1, 1), (2, 5, 7, 1), (1, 9, 10, 2), (3, 17, 23, 3), (1, 64, 64, 64), (2, 96, 128, 8)]


@pytest.mark.parametrize("G,H,W,s", BOX_CASES)
def test_box_reduce_equals_numpy(gpu, G, H, W, s):
    import torch
    from deblurgs_amd import registration as reg
    rng = np.random.default_rng(G * 1000 + H * 10 + s)
    full = np.full((G, H, W, 3), 255, np.uint8)             # (1, 64, 64, 64): the largest per-pixel sum
    fills = [rng.integers(0, 256, size=(G, H, W, 3), dtype=np.uint8), np.zeros((G, H, W, 3), np.uint8), full]
    h, w = H // s, W // s
    pitch = (h * w + 3) & ~3
    for x in fills:
        want = box_ref(x, s)
        out = torch.full((G, pitch), -1, dtype=torch.int32, device="cuda")        # poisoned: the pad must be WRITTEN
        got = reg.box_reduce_u8(torch.from_numpy(x).cuda(), s, out=out)
        assert got.shape == (G, pitch) and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (G, H, W, s)
        if h * w < pitch:
            assert int(got[:, h * w:].abs().max()) == 0
    assert int(box_ref(full, s)[0, 0]) == 0x00FFFFFF                         # all 255 stays 255, top byte 0


def test_box_reduce_takes_a_misaligned_input_and_allocates_its_output(gpu):
    import torch
    from deblurgs_amd import registration as reg
    rng = np.random.default_rng(5)
    G, H, W, s = 3, 17, 23, 3
    x = rng.integers(0, 256, size=(G, H, W, 3), dtype=np.uint8)
    for off in (1, 2, 3, 7):
        buf = torch.zeros(off + x.size, dtype=torch.uint8, device="cuda")
        buf[off:] = torch.from_numpy(x).cuda().reshape(-1)
        view = buf[off:].view(G, H, W, 3)
        assert view.data_ptr() % 4 == off % 4 and view.is_contiguous()
        assert np.array_equal(reg.box_reduce_u8(view, s).cpu().numpy().view(np.uint32), box_ref(x, s)), off
    with pytest.raises(RuntimeError, match="s must be"):
        reg.box_reduce_u8(torch.from_numpy(x).cuda(), 0)
    with pytest.raises(RuntimeError, match="empty output"):
        reg.box_reduce_u8(torch.from_numpy(x).cuda(), 18)


# ------------------------------------------------------------------------------------------------ sad_matrix
def _sad_cases():
    from deblurgs_amd import registration as reg
    c, ta = reg.SAD_CHUNK, reg.SAD_TILE_A
    return [(1, 1, 4), (1, 1, 8), (3, 5, 12), (17, 1, 1024), (1, 33, 1028), (5, 7, c - 4), (5, 7, c), (5, 7, c + 4),
            (4, 6, 3 * c + 4), (ta + 1, 9, 260), (ta + 1, 1, c + 8)]


@pytest.mark.parametrize("case", range(11))
def test_sad_matrix_equals_numpy(gpu, case):
    import torch
    from deblurgs_amd import _lib, registration as reg
    na, nb, L = _sad_cases()[case]
    rng = np.random.default_rng(100 + case)
    a, b = _random_words(rng, na, L), _random_words(rng, nb, L)
    want = sad_ref(a, b)
    da, db = _dev(a), _dev(b)
    need = _lib.lib().dgs_sad_matrix_tmp_bytes(na, nb, L)
    tmp = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")        # poisoned: nothing may depend on it
    got = reg.sad_matrix(da, db, tmp=tmp)
    assert got.dtype == torch.int64 and tuple(got.shape) == (na, nb)
    assert np.array_equal(got.cpu().numpy(), want), (na, nb, L)
    assert int(tmp[need:].min()) == 0xFF                                         # and nothing is written past its size
    again = reg.sad_matrix(da, db)                                               # a fresh work area: bit-identical
    assert torch.equal(got, again)
    assert torch.equal(reg.sad_matrix(db, da), got.t())                          # |a - b| = |b - a|
    assert int(reg.sad_matrix(da, da).diagonal().abs().max()) == 0


def test_sad_matrix_totals_are_64_bit(gpu):
    import torch
    from deblurgs_amd import registration as reg
    L = 4_300_000
    a = torch.zeros((1, L), dtype=torch.int32, device="cuda")
    b = torch.full((1, L), -1, dtype=torch.int32, device="cuda")                  # 0xFFFFFFFF
    got = reg.sad_matrix(a, b)
    assert 1020 * L > 2 ** 32
    assert got.cpu().numpy().tolist() == [[1020 * L]]
    assert reg.sad_matrix(a, b, group=1).cpu().numpy().tolist() == [[1020 * L]]


def _group_cases():
    from deblurgs_amd import registration as reg
    return [(1, 12, 256), (3, 12, 1028), (5, 13, reg.SAD_CHUNK + 8)]


@pytest.mark.parametrize("case", range(3))
def test_grouped_sad_equals_the_block_diagonal_of_all_pairs(gpu, case):
    import torch
    from deblurgs_amd import _lib, registration as reg
    na, m, L = _group_cases()[case]
    rng = np.random.default_rng(200 + case)
    a, b = _random_words(rng, na, L), _random_words(rng, na * m, L)
    da, db = _dev(a), _dev(b)
    need = _lib.lib().dgs_sad_matrix_tmp_bytes(na, na * m, L)
    tmp = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    got = reg.sad_matrix(da, db, group=m, tmp=tmp)
    assert tuple(got.shape) == (na, m)
    full = reg.sad_matrix(da, db).cpu().numpy()
    want = np.stack([full[i, i * m:(i + 1) * m] for i in range(na)])
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want, np.stack([sad_ref(a[i:i + 1], b[i * m:(i + 1) * m])[0] for i in range(na)]))
    assert torch.equal(got, reg.sad_matrix(da, db, group=m))
    with pytest.raises(RuntimeError, match="na \\* m"):
        reg.sad_matrix(da, db, group=m + 1)


# ------------------------------------------------------------------------------------------------ planted seeds
W, H = 160, 120


@pytest.fixture(scope="module")
def seed_scene(gpu):
    """A product cloud (as test_gpu_evaluation._fit_fixture makes its own) and a 4-view motion module whose views sit a
    few pixels apart and whose trajectories bend by about a pixel."""
    import torch
    from deblurgs_amd.cloud import GaussianCloud
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    torch.manual_seed(3)
    sc = synthetic.make_scene(2500, W, H, K=3, seed=3, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    init = torch.arange(4.0)[:, None] * torch.tensor([0.08, -0.03, 0.02, 0.01, 0.03, -0.01]) + torch.randn(4, 6) * 0.003
    m = CameraMotionModule(ref, torch.rand(4, 3, H, W, device="cuda"), curve_order=3, num_subframes=5, init_se3=init,
                           device="cuda")
    with torch.no_grad():
        m._rot._control_points.add_(torch.randn_like(m._rot._control_points) * 0.004)
        m._trans._control_points.add_(torch.randn_like(m._trans._control_points) * 0.01)
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    return dict(sc=sc, cloud=cloud, motion=m, bg=bg)


def _renders(cams, s, tone=None):
    """[n,3,H,W]: the display-space images of the cameras (one K-fused call, as the bank renders them)."""
    import torch
    from deblurgs_amd import losses, render_path as rp
    color = rp.render_group(cams, s["cloud"], s["bg"])["render"]
    if tone is None:
        return color
    return losses.ToneMapping(tone)(color).clamp(0.0, 1.0)


@pytest.mark.parametrize("factor", [1, 4])
def test_planted_seeds_are_found_exactly(seed_scene, factor):
    import torch
    from deblurgs_amd import evaluation as ev, registration as reg
    s = seed_scene
    cams, table = reg.candidate_cameras(s["motion"], subframes=3, between=1)
    assert len(cams) == 4 * 3 + 3
    planted = [table.index(("trajectory", 1, 0)), table.index(("trajectory", 2, 1)), table.index(("between", 1, 1)),
               table.index(("trajectory", 3, 2))]
    # (four cameras in one call: slot i is the K = 1 render bit for bit, whatever the call's other slots are)
    images = _renders([cams[c] for c in planted], s)
    res = reg.seed_test_poses(s["motion"], s["cloud"], images, s["bg"], None, factor=factor, refine_rounds=0)
    assert res.seed_index.tolist() == planted
    assert res.seed_score.tolist() == [0, 0, 0, 0] and res.final_score.tolist() == [0, 0, 0, 0] and res.moves == []
    scores = res.scores.cpu().numpy()
    assert scores.shape == (4, 15) and scores.dtype == np.int64
    assert (np.delete(scores[0], planted[0]) > 0).all()                  # the other candidates are other images
    model = ev.TestPoseModel(res.cameras, device="cuda")
    for j, c in enumerate(planted):
        assert res.cameras[j].original_image is not None and torch.equal(res.cameras[j].original_image, images[j])
        assert (res.cameras[j].image_width, res.cameras[j].image_height) == (W, H)
        with torch.no_grad():
            err = float((model(j).world_view_transform - cams[c].world_view_transform).abs().max())
        assert err <= 1e-6, (j, err)
    # frames_per_call changes how the bank is rendered, not one score
    other = reg.seed_test_poses(s["motion"], s["cloud"], images, s["bg"], None, factor=factor, refine_rounds=0,
                                frames_per_call=7)
    assert torch.equal(other.scores, res.scores)


def test_planted_seeds_under_the_gamma_tone_map(seed_scene):
    from deblurgs_amd import registration as reg
    s = seed_scene
    cams, table = reg.candidate_cameras(s["motion"], subframes=3, between=1)
    planted = [table.index(("trajectory", 0, 2)), table.index(("between", 2, 1)), table.index(("trajectory", 2, 0))]
    images = _renders([cams[c] for c in planted], s, "gamma")
    res = reg.seed_test_poses(s["motion"], s["cloud"], images, s["bg"], "gamma", factor=4, refine_rounds=0)
    assert res.seed_index.tolist() == planted


def test_planted_lattice_move_is_taken_then_the_steps_halve(seed_scene):
    import torch
    from deblurgs_amd import registration as reg, render_path as rp
    s = seed_scene
    cams, table = reg.candidate_cameras(s["motion"], subframes=3, between=1)
    c = table.index(("trajectory", 1, 1))
    ts, rs_deg = 0.004, 0.1
    lattice = reg.seed_lattice(rp.cam_to_c2w(cams[c]), ts, np.deg2rad(rs_deg))
    ks = [0, 7]
    images = _renders([rp.c2w_to_cam(cams[c], lattice[k]) for k in ks], s)
    res = reg.seed_test_poses(s["motion"], s["cloud"], images, s["bg"], None, factor=1, refine_rounds=2, trans_step=ts,
                              rot_step_deg=rs_deg)
    assert res.seed_index.tolist() == [c, c]
    assert (res.seed_score > 0).all()
    assert res.final_score.tolist() == [0, 0]
    assert [(r, i, k) for r, i, k, _, _ in res.moves] == [(0, 0, ks[0]), (0, 1, ks[1])]      # round 1 moves, round 2 does not
    for j, k in enumerate(ks):
        assert np.array_equal(res.poses[j], lattice[k])
    assert np.array_equal(res.trans_step, [ts / 2, ts / 2]) and np.allclose(res.rot_step_rad, np.deg2rad(rs_deg) / 2, rtol=1e-15)
    assert (res.final_score <= res.seed_score).all()
    assert all(after < before for _, _, _, before, after in res.moves)


def test_pattern_search_never_raises_the_score(seed_scene):
    """An unplanted pose (between candidates, off the lattice) with the default, data-driven steps."""
    from deblurgs_amd import registration as reg, render_path as rp
    s = seed_scene
    cams, table = reg.candidate_cameras(s["motion"], subframes=3, between=1)
    a, b = rp.cam_to_c2w(cams[table.index(("trajectory", 1, 2))]), rp.cam_to_c2w(cams[table.index(("trajectory", 2, 0))])
    pose = reg._se3_between(a, b, 0.3)
    images = _renders([rp.c2w_to_cam(cams[0], pose)], s, "gamma")
    res = reg.seed_test_poses(s["motion"], s["cloud"], images, s["bg"], "gamma", factor=4, refine_rounds=3)
    assert (res.final_score <= res.seed_score).all()
    last = int(res.seed_score[0])
    for _, i, _, before, after in res.moves:
        assert i == 0 and before == last and after < before
        last = after
    assert last == int(res.final_score[0])
    assert (res.trans_step > 0).all() and (res.rot_step_rad > 0).all()


def test_initialize_fit_evaluate_end_to_end(seed_scene):
    import torch
    from deblurgs_amd import evaluation as ev, losses, registration as reg, render_path as rp
    s = seed_scene
    tm = losses.ToneMapping("gamma")
    cams, table = reg.candidate_cameras(s["motion"], subframes=3, between=1)
    truth = []
    for name, f in ((("trajectory", 0, 1), 0.2), (("trajectory", 2, 1), 0.35)):
        i = table.index(name)
        truth.append(reg._se3_between(rp.cam_to_c2w(cams[i]), rp.cam_to_c2w(cams[i + 1]), f))
    images = _renders([rp.c2w_to_cam(cams[0], p) for p in truth], s, "gamma")
    start = ev.initialize_test_pose(s["motion"], s["cloud"], images, s["bg"], tm, factor=4, refine_rounds=2)
    assert len(start) == 2 and all(isinstance(c, ev.TestCamera) for c in start)
    fitted = ev.optimize_test_pose(s["cloud"], start, images, s["bg"], tm, num_iter_per_view=20, seed=0)
    torch.cuda.synchronize()
    psnr, ssim = ev.evaluate(fitted, s["cloud"], s["bg"], images, tm)
    assert np.isfinite(psnr) and np.isfinite(ssim) and psnr > 0.0 and -1.0 <= ssim <= 1.0

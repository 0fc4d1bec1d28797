"""PNG files made on the device (dgs_png_encode, deblurgs_amd/png.py) against the format's own decoders: zlib.decompress,
PIL and zlib.crc32 (tests/png_cases.py).  Decoded pixels equal the input exactly; there is no tolerance anywhere."""
import os

import numpy as np
import pytest

import png_cases as pc
from deblurgs_amd import _lib
from helpers import synthetic

pytestmark = pytest.mark.gpu

GUARD = 0xA5
S = _lib.PNG_SEGMENT            # DGS_PNG_SEGMENT (tests/test_png_host.py keeps it in step with the header)


def _encode(images, image_stride=None, src_offset=0):
    """dgs_png_encode through ctypes with guard bytes around files, sizes and tmp and an odd file stride.  images uint8
    [n,h,w,c] (numpy).  Returns the list of file bytes; asserts the guards, sizes <= bound and the untouched slot tails."""
    import torch
    from deblurgs_amd import _lib
    from deblurgs_amd.raster_call import _stream
    L = _lib.lib()
    images = np.ascontiguousarray(images)
    n, h, w, c = images.shape
    per = h * w * c
    stride_i = per if image_stride is None else image_stride
    dev = torch.device("cuda:0")
    src = torch.full((src_offset + n * stride_i + 16,), 0x33, dtype=torch.uint8, device=dev)
    for i in range(n):
        at = src_offset + i * stride_i
        src[at:at + per] = torch.from_numpy(images[i].reshape(-1)).to(dev)
    bound = L.dgs_png_bound(w, h, c)
    assert bound == 63 + h * (1 + w * c) + 5 * -(-(h * (1 + w * c)) // S)
    stride_f = bound + 7                                  # file i starts at any alignment
    g = 67
    files = torch.full((g + n * stride_f + g,), GUARD, dtype=torch.uint8, device=dev)
    sizes = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    tmp_bytes = L.dgs_png_tmp_bytes(n, w, h, c)
    assert tmp_bytes > 0
    tmp = torch.full((g + tmp_bytes + g,), GUARD, dtype=torch.uint8, device=dev)
    _lib.check(L.dgs_png_encode(src.data_ptr() + src_offset, n, w, h, c, stride_i, files.data_ptr() + g, stride_f,
                                sizes.data_ptr() + 8, tmp.data_ptr() + g, _stream(dev)), "dgs_png_encode")
    torch.cuda.synchronize()
    files, sizes, tmp = files.cpu().numpy(), sizes.cpu().numpy(), tmp.cpu().numpy()
    assert sizes[0] == -7 and sizes[-1] == -7
    assert (files[:g] == GUARD).all() and (files[g + n * stride_f:] == GUARD).all()
    assert (tmp[:g] == GUARD).all() and (tmp[g + tmp_bytes:] == GUARD).all()
    out = []
    for i in range(n):
        size = int(sizes[1 + i])
        assert 63 < size <= bound, (size, bound)
        slot = files[g + i * stride_f:g + (i + 1) * stride_f]
        assert (slot[size:] == GUARD).all(), "bytes of the slot past sizes[i] were written"
        out.append(slot[:size].tobytes())
    return out


def _check(data, image, size=False):
    from deblurgs_amd import png
    filtered, idat_len = pc.check_file(data, image, png.chunks)
    if size:
        assert filtered.size >= 4 * S - S + 1            # four or more segments
        pc.check_size(idat_len, filtered)
    return filtered


# ------------------------------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (3, 5), (64, 64)])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_round_trip_of_random_bytes(gpu, c, w, h):
    image = pc.random_image(h, w, c, seed=100 * c + w + h)
    data, = _encode(image[None])
    _check(data, image)


# ------------------------------------------------------------------------------------------------- 2. segment edges
@pytest.mark.parametrize("w", [S - 2, S - 1, S, 2 * S - 1])
def test_segment_edges_of_one_gray_row(gpu, w):
    image = pc.smooth_noise(1, w, 1, seed=w)
    data, = _encode(image[None])
    filtered = _check(data, image)
    assert filtered.size == w + 1


@pytest.fixture(scope="module")
def straddling():
    """1000 x 17 RGB, smooth plus noise: rows of 3001 filtered bytes straddle the segments (four of them)."""
    image = pc.smooth_noise(17, 1000, 3, seed=3)
    return image, pc.filter_rows(image)


def test_rows_straddling_segments(gpu, straddling):
    image, (_, want) = straddling
    data, = _encode(image[None])
    filtered = _check(data, image, size=True)
    assert np.array_equal(filtered, want)                                # 6. the filter bytes and the residuals


# ------------------------------------------------------------------------------------------------- 3. run arithmetic
@pytest.mark.parametrize("w", [2, 3, 258, 259, 260, 261, 516, 517])
def test_one_run_of_zeros(gpu, w):
    image = np.zeros((1, w, 1), np.uint8)
    data, = _encode(image[None])
    filtered = _check(data, image)
    assert not filtered.any()                    # the filter byte 0 ties to None: one run of 1 + w zeros


def test_one_run_across_all_segments(gpu):
    image = np.zeros((301, 300, 1), np.uint8)
    data, = _encode(image[None])
    filtered = _check(data, image, size=True)
    assert not filtered.any()
    assert len(data) < 400


# ------------------------------------------------------------------------------------------------- 4. fallback and gain
def test_incompressible_bytes_fall_back_to_stored_blocks(gpu):
    image = pc.random_image(128, 128, 3, seed=4)
    data, = _encode(image[None])                 # (_encode asserts size <= bound)
    _check(data, image, size=True)


def test_a_constant_image_is_a_few_hundred_bytes(gpu):
    image = np.full((64, 64, 3), 255, np.uint8)
    data, = _encode(image[None])
    filtered = _check(data, image)
    assert (filtered[1:, 0] == 2).all() and not filtered[1:, 1:].any()
    assert len(data) * 20 < image.size, len(data)


# ------------------------------------------------------------------------------------------------- 5. code-length limit
def test_a_histogram_whose_unlimited_code_is_16_deep(gpu):
    image = pc.skewed_row()
    data, = _encode(image[None])
    filtered = _check(data, image)               # zlib.decompress refuses an over-subscribed or incomplete code
    assert filtered[0, 0] == 0


# ------------------------------------------------------------------------------------------------- 6. filter bytes
def test_filter_choice_equals_the_numpy_restatement_rgba(gpu):
    image = pc.smooth_noise(29, 37, 4, seed=6)
    image[5:9] = pc.random_image(4, 37, 4, seed=7)
    image[20:] = image[19]                                              # rows that repeat: Up
    types, want = pc.filter_rows(image)
    data, = _encode(image[None])
    filtered = _check(data, image)
    assert np.array_equal(filtered[:, 0], types)
    assert np.array_equal(filtered, want)
    assert len(set(types.tolist())) >= 3


# ------------------------------------------------------------------------------------------------- 7. batch, determinism
def test_batch_strides_alignment_and_determinism(gpu):
    images = np.stack([pc.smooth_noise(33, 211, 3, seed=8), pc.random_image(33, 211, 3, seed=9),
                       np.full((33, 211, 3), 7, np.uint8)])
    per = images[0].size
    batch = _encode(images, image_stride=per + 13)
    for i in range(3):
        _check(batch[i], images[i])
        assert _encode(images[i:i + 1]) == [batch[i]], i                 # file i of the batch = a call of its own
    assert _encode(images, image_stride=per + 13) == batch               # a second call
    assert _encode(images, image_stride=per + 13, src_offset=1) == batch   # a source one byte off alignment


def test_python_front_end(gpu, tmp_path):
    import torch
    from deblurgs_amd import png
    images = np.stack([pc.smooth_noise(20, 31, 1, seed=10), pc.random_image(20, 31, 1, seed=11)])[..., 0]
    dev = torch.from_numpy(images).cuda()
    files, sizes = png.encode(dev)
    assert files.dtype == torch.uint8 and sizes.dtype == torch.uint64 and files.shape[1] >= png.bound(31, 20, 1)
    blobs = png.to_bytes(dev)
    for i in range(2):
        _check(blobs[i], images[i])
    paths = png.write_files(dev, [str(tmp_path / "a.png"), str(tmp_path / "b.png")])
    assert [open(p, "rb").read() for p in paths] == blobs
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        png.encode(torch.from_numpy(images))
    assert png.encode(dev[:0])[1].numel() == 0


def test_download_of_a_strided_files_view(gpu):
    """device_files.download alone: files= is a view into a wider tensor (row stride > width, 5 bytes in)."""
    import torch
    from deblurgs_amd import device_files, png
    images = np.stack([pc.smooth_noise(33, 211, 3, seed=8), pc.random_image(33, 211, 3, seed=9),
                       np.full((33, 211, 3), 7, np.uint8)])
    need = png.bound(211, 33, 3)
    wide = torch.full((3, need + 40), GUARD, dtype=torch.uint8, device="cuda")
    files, sizes = png.encode(torch.from_numpy(images).cuda(), files=wide[:, 5:5 + need + 3])
    assert files.stride(0) > files.shape[1]
    blobs = device_files.download(files, sizes)
    host, host_sizes = wide.cpu().numpy(), sizes.view(torch.int64).cpu().tolist()
    assert blobs == [host[i, 5:5 + host_sizes[i]].tobytes() for i in range(3)]
    assert blobs == png.to_bytes(torch.from_numpy(images).cuda())
    for i in range(3):
        _check(blobs[i], images[i])
        assert (host[i, :5] == GUARD).all() and (host[i, 5 + host_sizes[i]:] == GUARD).all()


# ------------------------------------------------------------------------------------------------- 8. end to end
@pytest.fixture(scope="module")
def small_scene(gpu):
    """The report tests' scene: 500 Gaussians at 64 x 48, three test cameras, noisy ground truth."""
    import torch
    from deblurgs_amd import evaluation as ev, gaussian_renderer, losses
    from deblurgs_amd.cloud import GaussianCloud
    P, W, H, n = 500, 64, 48, 3
    sc = synthetic.make_scene(P, W, H, K=n, seed=5, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    tm = losses.ToneMapping("gamma")
    with torch.no_grad():
        cams = [model(i) for i in range(n)]
        renders = torch.stack([gaussian_renderer.render(c, cloud, bg)["render"] for c in cams]).contiguous()
        torch.manual_seed(0)
        gts = (tm(renders).clamp(0.0, 1.0) + 0.03 * torch.randn_like(renders)).clamp(0.0, 1.0)
    return dict(cloud=cloud, bg=bg, cams=cams, gts=gts, tm=tm, H=H, W=W, n=n, sc=sc)


def _same_files(a, b):
    from PIL import Image
    from deblurgs_amd import png
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(a)
    for name in os.listdir(a):
        want = np.asarray(Image.open(os.path.join(a, name)))
        data = open(os.path.join(b, name), "rb").read()
        assert want.shape == (48, 64, 3)
        pc.check_file(data, want, png.chunks)


def test_evaluate_with_device_png_writes_the_same_files(small_scene, tmp_path):
    from deblurgs_amd import evaluation as ev
    s = small_scene
    args = (s["cams"], s["cloud"], s["bg"], s["gts"], s["tm"])
    plain = ev.evaluate(*args, vis_dir=str(tmp_path / "host"))
    assert ev.evaluate(*args, vis_dir=str(tmp_path / "device"), device_png=True) == plain
    _same_files(str(tmp_path / "host"), str(tmp_path / "device"))
    with pytest.raises(ValueError, match="writer"):
        ev.evaluate(*args, vis_dir=str(tmp_path / "x"), writer=lambda p, a: None, device_png=True)


def test_traj_render_with_device_png_writes_the_same_files(small_scene, tmp_path):
    import torch
    from deblurgs_amd import report
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    s = small_scene
    sc, H, W = s["sc"], s["H"], s["W"]
    torch.manual_seed(11)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    gt = torch.rand(2, 3, H, W, device="cuda")
    m = CameraMotionModule(ref, gt, curve_order=3, num_subframes=5, init_se3=torch.randn(2, 6) * 0.01, device="cuda")
    m.link_gaussian(s["cloud"])
    host = report.traj_render(m, s["cloud"], str(tmp_path / "host"), 30, "gamma", background=s["bg"])
    device = report.traj_render(m, s["cloud"], str(tmp_path / "device"), 30, "gamma", background=s["bg"], device_png=True)
    assert [os.path.basename(p) for p in device] == [os.path.basename(p) for p in host]
    assert len(device) == 2 * 6
    _same_files(os.path.dirname(host[0]), os.path.dirname(device[0]))
    with pytest.raises(ValueError, match="writer"):
        report.traj_render(m, s["cloud"], str(tmp_path / "x"), 30, writer=lambda p, a: None, device_png=True)


def test_write_frames_png_equals_render_frames(small_scene, tmp_path):
    from PIL import Image
    from deblurgs_amd import png, render_path
    s = small_scene
    cams = s["cams"] + s["cams"][:2]                     # five frames, groups of 2, 2 and 1: all three pipeline stages
    want = render_path.render_frames(cams, s["cloud"], s["bg"], s["tm"], crop_ratio=0.9, frames_per_call=2)
    paths = render_path.write_frames_png(cams, s["cloud"], s["bg"], str(tmp_path / "frames"), s["tm"], crop_ratio=0.9,
                                         frames_per_call=2)
    assert [os.path.basename(p) for p in paths] == [f"{i:05d}.png" for i in range(5)]
    for i, p in enumerate(paths):
        pc.check_file(open(p, "rb").read(), want[i], png.chunks)
        assert np.array_equal(np.asarray(Image.open(p)), want[i])


@pytest.fixture(scope="module")
def seven_frames(small_scene):
    """Seven cameras (the fixture's three, repeated) and the PNG files of their render_frames, made in one encode call."""
    import torch
    from deblurgs_amd import png, render_path
    s = small_scene
    cams = (s["cams"] * 3)[:7]
    frames = render_path.render_frames(cams, s["cloud"], s["bg"], s["tm"], crop_ratio=0.9, frames_per_call=2)
    want = png.to_bytes(torch.from_numpy(frames).cuda())
    assert len(set(want)) == 3                           # (neighbours differ: a file in the wrong place shows)
    return cams, want


# groups 2, 2, 2, 1: every download slot is used again after its files were written; one camera and one group of seven:
# nothing but the drain; groups 4, 3: no steady state
@pytest.mark.parametrize("n,per_call", [(7, 2), (1, 2), (7, 7), (7, 4)])
def test_write_frames_png_schedules(small_scene, seven_frames, tmp_path, n, per_call):
    from deblurgs_amd import render_path
    s = small_scene
    cams, want = seven_frames
    paths = render_path.write_frames_png(cams[:n], s["cloud"], s["bg"], str(tmp_path / "frames"), s["tm"], crop_ratio=0.9,
                                         frames_per_call=per_call)
    assert paths == [str(tmp_path / "frames" / f"{i:05d}.png") for i in range(n)]
    assert sorted(os.listdir(tmp_path / "frames")) == [f"{i:05d}.png" for i in range(n)]
    for i, p in enumerate(paths):
        assert open(p, "rb").read() == want[i], i

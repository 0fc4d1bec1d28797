"""Motion-JPEG AVI files of rendered camera paths (deblurgs_amd/video.py, render_path.write_frames_video): the frames inside
the container are the device's JPEG files byte for byte, the container parses, Pillow decodes every frame."""
import numpy as np
import pytest

import jpeg_cases as jc
from helpers import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small_scene(gpu):
    """500 Gaussians at 64 x 48, three cameras along the scene's trajectory."""
    import torch
    from deblurgs_amd import evaluation as ev, losses
    from deblurgs_amd.cloud import GaussianCloud
    P, W, H, n = 500, 64, 48, 3
    sc = synthetic.make_scene(P, W, H, K=n, seed=5, sigma_px=2.5)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    with torch.no_grad():
        cams = [model(i) for i in range(n)]
    return dict(cloud=cloud, bg=bg, cams=cams, tm=losses.ToneMapping("gamma"), H=H, W=W, n=n, sc=sc)


def test_write_frames_video_holds_the_device_jpegs_of_render_frames(small_scene, tmp_path):
    import torch
    from deblurgs_amd import jpeg, render_path, video
    s = small_scene
    cams = s["cams"] + s["cams"][:2]                     # five frames, groups of 2, 2 and 1: all three pipeline stages
    frames = render_path.render_frames(cams, s["cloud"], s["bg"], s["tm"], crop_ratio=0.9, frames_per_call=2)
    assert len(np.unique(frames)) > 50                   # (a picture, not a constant)
    path = render_path.write_frames_video(cams, s["cloud"], s["bg"], str(tmp_path / "path.avi"), 32, s["tm"], crop_ratio=0.9,
                                          frames_per_call=2, quality=85, subsampling="4:2:0")
    header, inside = video.parse_avi(open(path, "rb").read())
    assert inside == jpeg.to_bytes(torch.from_numpy(frames).cuda(), 85, "4:2:0")
    h, w = frames.shape[1:3]
    assert (header["avih"]["total_frames"], header["avih"]["width"], header["avih"]["height"]) == (5, w, h)
    assert (header["strh"]["rate"], header["strh"]["scale"], header["strh"]["length"]) == (32, 1, 5)
    for i, data in enumerate(inside):
        assert data == jc.encode(frames[i], 85, "4:2:0")                  # and the specification's bytes
        assert np.asarray(jc.decode(data)).shape == frames[i].shape       # Pillow decodes it
    # the defaults, and 4:4:4
    path = render_path.write_frames_video(cams[:3], s["cloud"], s["bg"], str(tmp_path / "b.avi"), 10, s["tm"], subsampling="4:4:4")
    _, inside = video.parse_avi(open(path, "rb").read())
    full = render_path.render_frames(cams[:3], s["cloud"], s["bg"], s["tm"])
    assert inside == jpeg.to_bytes(torch.from_numpy(full).cuda(), 90, "4:4:4")


def test_render_spiral_with_make_video_as_its_writer(small_scene, tmp_path):
    import torch
    from deblurgs_amd import render_path, video
    from deblurgs_amd.motion import CameraMotionModule, RefCamera
    s = small_scene
    sc, H, W = s["sc"], s["H"], s["W"]
    torch.manual_seed(7)
    ref = RefCamera(W, H, sc["FoVx"], sc["FoVy"], device="cuda")
    m = CameraMotionModule(ref, torch.rand(3, 3, H, W, device="cuda"), curve_order=3, num_subframes=5,
                           init_se3=torch.randn(3, 6) * 0.01, device="cuda")
    path = str(tmp_path / "render_img.avi")
    frames = render_path.render_spiral(m, s["cloud"], s["bg"], "gamma", n_frames=5, spin_for=2, frames_per_call=4,
                                       writer=video.make_video, path=path)
    header, inside = video.parse_avi(open(path, "rb").read())
    assert len(inside) == 10 == header["avih"]["total_frames"] and header["strh"]["rate"] == 32
    assert (header["avih"]["width"], header["avih"]["height"]) == (W, H)
    for data, frame in zip(inside, frames):
        assert data == jc.encode(frame, 90, "4:2:0")
    assert video.make_video(frames[:2], str(tmp_path / "named.mp4")).endswith("named.avi")       # the reference's names


def test_make_video_of_a_numpy_array_equals_write_video_on_the_device(small_scene, tmp_path):
    import torch
    from deblurgs_amd import video
    frames = np.stack([jc.smooth_patch(40, 56, 3, seed=s) for s in range(video.UPLOAD_GROUP + 3)])      # two uploads
    a = video.make_video(frames, str(tmp_path / "host.avi"), fps=20)
    b = video.write_video(torch.from_numpy(frames).cuda(), str(tmp_path / "device.avi"), 20)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read()
    header, inside = video.parse_avi(data)
    assert len(inside) == len(frames) and header["strh"]["rate"] == 20
    assert video.make_video(list(frames), str(tmp_path / "list.avi"), 20) and open(tmp_path / "list.avi", "rb").read() == data
    with video.MjpegAviWriter(str(tmp_path / "mixed.avi"), 20) as w:
        w.append(torch.from_numpy(frames[:4]).cuda())
        with pytest.raises(ValueError, match="one size"):
            w.append(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            w.append(torch.from_numpy(frames[:1]))
    assert video.parse_avi(open(tmp_path / "mixed.avi", "rb").read())[1] == inside[:4]


def _inside(path, n):
    """The frames of the .avi at path, after checking that its index and its counts name n frames in file order."""
    from deblurgs_amd import video
    header, inside = video.parse_avi(open(path, "rb").read())
    assert header["avih"]["total_frames"] == header["strh"]["length"] == len(inside) == n
    at = 4                                               # index offsets count from the 'movi' fourcc
    for (fourcc, _, offset, size), data in zip(header["index"], inside):
        assert (fourcc, offset, size) == (b"00dc", at, len(data))
        at += 8 + len(data) + (len(data) & 1)
    return inside


@pytest.fixture(scope="module")
def seven_frames(small_scene):
    """Seven cameras (the fixture's three, repeated) and the JPEG files of their render_frames, made in one encode call."""
    import torch
    from deblurgs_amd import jpeg, render_path
    s = small_scene
    cams = (s["cams"] * 3)[:7]
    frames = render_path.render_frames(cams, s["cloud"], s["bg"], s["tm"], crop_ratio=0.9, frames_per_call=2)
    want = jpeg.to_bytes(torch.from_numpy(frames).cuda(), 85, "4:2:0")
    assert len(set(want)) == 3                           # (neighbours differ: a frame in the wrong place shows)
    return cams, want


# groups 2, 2, 2, 1: every download slot is used again after its frames were appended; one camera and one group of seven:
# nothing but the drain; groups 4, 3: no steady state
@pytest.mark.parametrize("n,per_call", [(7, 2), (1, 2), (7, 7), (7, 4)])
def test_write_frames_video_schedules(small_scene, seven_frames, tmp_path, n, per_call):
    from deblurgs_amd import render_path
    s = small_scene
    cams, want = seven_frames
    path = render_path.write_frames_video(cams[:n], s["cloud"], s["bg"], str(tmp_path / "path.avi"), 32, s["tm"],
                                          crop_ratio=0.9, frames_per_call=per_call, quality=85, subsampling="4:2:0")
    assert _inside(path, n) == want[:n]


def test_write_frames_video_grows_its_host_buffers(gpu, tmp_path):
    """A cloud of 5000 splats of about a pixel at 128 x 96, quality 100, 4:4:4: the files of a group of four take more
    than the HOST_BYTES a download slot starts with, so both slots grow, and the third group uses a grown one."""
    import torch
    from deblurgs_amd import evaluation as ev, jpeg, losses, render_path, video
    from deblurgs_amd.cloud import GaussianCloud
    P, W, H, n = 5000, 128, 96, 3
    sc = synthetic.make_scene(P, W, H, K=n, seed=6, sigma_px=0.6, sigma_log=0.3)
    cloud = GaussianCloud.from_scene(sc, "cuda")
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    V = sc["viewmatrix"][:n].astype(np.float64)
    model = ev.TestPoseModel([ev.TestCamera(V[i][:3, :3], V[i][3, :3], sc["FoVx"], sc["FoVy"], W, H) for i in range(n)],
                             device="cuda")
    with torch.no_grad():
        cams = [model(i) for i in range(n)] * 3          # nine frames, groups of 4, 4 and 1
    tm = losses.ToneMapping("gamma")
    frames = render_path.render_frames(cams, cloud, bg, tm, frames_per_call=4)
    want = jpeg.to_bytes(torch.from_numpy(frames).cuda(), 100, "4:4:4")
    sizes = [len(data) for data in want]
    print("bytes per frame:", sizes, "a slot starts with", video.HOST_BYTES)
    assert sum(sizes[0:4]) > video.HOST_BYTES and sum(sizes[4:8]) > video.HOST_BYTES
    path = render_path.write_frames_video(cams, cloud, bg, str(tmp_path / "noisy.avi"), 32, tm, frames_per_call=4,
                                          quality=100, subsampling="4:4:4")
    assert _inside(path, 9) == want


def test_download_of_a_strided_files_view(gpu):
    """device_files.download alone: files= is a view into a wider tensor (row stride > width, 5 bytes in)."""
    import torch
    from deblurgs_amd import device_files, jpeg
    images = np.stack([jc.smooth_patch(33, 211, 3, seed=8), jc.random_image(33, 211, 3, seed=9),
                       np.full((33, 211, 3), 7, np.uint8)])
    need = jpeg.bound(211, 33, 3, "4:2:0")
    wide = torch.full((3, need + 40), 0xA5, dtype=torch.uint8, device="cuda")
    files, sizes = jpeg.encode(torch.from_numpy(images).cuda(), 90, "4:2:0", files=wide[:, 5:5 + need + 3])
    assert files.stride(0) > files.shape[1]
    blobs = device_files.download(files, sizes)
    host, host_sizes = wide.cpu().numpy(), sizes.view(torch.int64).cpu().tolist()
    assert blobs == [host[i, 5:5 + host_sizes[i]].tobytes() for i in range(3)]
    assert blobs == jpeg.to_bytes(torch.from_numpy(images).cuda(), 90, "4:2:0")


def test_add_takes_finished_files_of_one_size(gpu, tmp_path):
    import torch
    from deblurgs_amd import jpeg, video
    big = jpeg.to_bytes(torch.from_numpy(np.stack([jc.smooth_patch(40, 56, 3, seed=s) for s in range(3)])).cuda())
    small, = jpeg.to_bytes(torch.from_numpy(jc.smooth_patch(8, 8, 3, seed=0)[None]).cuda())
    with video.MjpegAviWriter(str(tmp_path / "added.avi"), 20) as w:
        w.add(big[0], (56, 40))                          # the size as the caller knows it
        w.add(big[1])                                    # and read from the file
        with pytest.raises(ValueError, match="one size"):
            w.add(small, (8, 8))
        with pytest.raises(ValueError, match="one size"):
            w.add(small)
        w.append(big[2])                                 # append(bytes) still works
        assert w.n_frames == 3 and w.size == (56, 40)
    assert _inside(str(tmp_path / "added.avi"), 3) == big

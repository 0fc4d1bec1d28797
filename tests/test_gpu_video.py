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

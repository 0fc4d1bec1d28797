"""JPEG files decoded on the device (dgs_jpeg_decode, deblurgs_amd/jpeg.py decode) against the numpy restatement of the pixel
specification (tests/jpeg_decode_cases.py, itself held against Pillow in tests/test_jpeg_decode_host.py): device pixels ==
restatement pixels, exactly.  There is no tolerance anywhere."""
import os

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_decode_cases as dc
import scene_cases as sc
from deblurgs_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _decode(files, expect_status=None):
    """dgs_jpeg_decode through ctypes: guard bytes around images, tmp and status, an image stride that is no multiple of 16.
    files: JPEG byte strings of one size.  Returns (uint8 [n,h,w,c] numpy, status list); asserts the guards, the untouched
    bytes between the images and -- unless expect_status is given -- that every status is 0."""
    import torch
    from deblurgs_amd import jpeg
    from deblurgs_amd.raster_call import _stream
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = len(files)
    plans = [jpeg.plan(f) for f in files]
    heads = [jpeg._head(p) for p in plans]
    w, h, c = heads[0].w, heads[0].h, heads[0].channels
    at, index = 16 * n, np.zeros((n, 2), np.uint64)
    for i in range(n):
        index[i, 1] = at
        at += (plans[i].size + 7) // 8 * 8
    for i in range(n):
        index[i, 0] = at
        at += (len(files[i]) + 3) // 4 * 4
    blob = np.full(at, 0xEE, np.uint8)          # (the gaps hold no zeros: nothing may lean on them)
    blob[:16 * n] = index.reshape(-1).view(np.uint8)
    for i in range(n):
        blob[int(index[i, 1]):int(index[i, 1]) + plans[i].size] = plans[i]
        blob[int(index[i, 0]):int(index[i, 0]) + len(files[i])] = np.frombuffer(files[i], np.uint8)
    blob_dev = torch.from_numpy(blob).to(dev)
    per = h * w * c
    stride = (per + 3) // 4 * 4 + 4
    stride += 4 if stride % 16 == 0 else 0
    assert stride % 16 != 0 and stride % 4 == 0
    g = 64
    images = torch.full((g + n * stride + g,), GUARD, dtype=torch.uint8, device=dev)
    status = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    tmp_bytes = L.dgs_jpeg_decode_tmp_bytes(n, w, h, c)
    assert tmp_bytes > 0
    tmp = torch.full((g + 1 + tmp_bytes + g,), GUARD, dtype=torch.uint8, device=dev)      # (tmp starts at an odd address)
    _lib.check(L.dgs_jpeg_decode(blob_dev.data_ptr(), at, blob_dev.data_ptr(), n, w, h, c, max(p.n_intervals for p in heads),
                                 images.data_ptr() + g, stride, status.data_ptr() + 4, tmp.data_ptr() + g + 1, _stream(dev)),
               "dgs_jpeg_decode")
    torch.cuda.synchronize()
    images, status, tmp = images.cpu().numpy(), status.cpu().numpy(), tmp.cpu().numpy()
    assert status[0] == -7 and status[-1] == -7
    assert (images[:g] == GUARD).all() and (images[g + n * stride:] == GUARD).all()
    assert (tmp[:g + 1] == GUARD).all() and (tmp[g + 1 + tmp_bytes:] == GUARD).all()
    out = np.zeros((n, h, w, c), np.uint8)
    for i in range(n):
        slot = images[g + i * stride:g + (i + 1) * stride]
        assert (slot[per:] == GUARD).all(), "bytes between the images were written"
        out[i] = slot[:per].reshape(h, w, c)
    got = status[1:-1].tolist()
    assert got == (expect_status if expect_status is not None else [0] * n), got
    return out, got


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} bytes differ, the first at (y, x, c) = {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


# ------------------------------------------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_pixels_equal_the_restatement(gpu, name):
    data, _ = dc.golden()[name]
    dc.check_needs(name, data)
    out, _ = _decode([data])
    _same(out[0], dc.expected(name), name)


# ------------------------------------------------------------------------------------------------- 2. the encoder's files
@pytest.mark.parametrize("mode", jc.MODES)
def test_the_encoders_own_files(gpu, mode):
    import torch
    from deblurgs_amd import jpeg
    images = np.stack([jc.image_for(45, 131, mode, seed=s) for s in (3, 4)])
    images = images[..., None] if mode == "gray" else images
    files = jpeg.to_bytes(torch.from_numpy(images).cuda(), 90, "4:2:0" if mode == "gray" else mode)
    assert jpeg.probe(files[0])["restart_interval"] == -(-131 // (16 if mode == "4:2:0" else 8))      # one interval per MCU row
    got = jpeg.decode(files)
    assert got.shape == images.shape and got.dtype == torch.uint8 and got.device.type == "cuda"
    for i in range(2):
        want = dc.decode(files[i])
        _same(got[i].cpu().numpy(), want[..., None] if want.ndim == 2 else want, f"{mode} {i}")


# ------------------------------------------------------------------------------------------------- 3. a mixed batch
RGB_17x33 = ["smooth_17x33_4:4:4", "smooth_17x33_4:2:2", "smooth_17x33_4:2:0"]


def _restart_variant():
    """smooth_17x33_4:2:0's picture once more, as the device encoder writes it: other tables, DRI = MCUs per row."""
    import torch
    from deblurgs_amd import jpeg
    return jpeg.to_bytes(torch.from_numpy(dc.expected("smooth_17x33_4:2:0")[None]).cuda(), 60, "4:2:0")[0]


def test_a_batch_whose_images_differ_in_tables_sampling_and_dri(gpu):
    from deblurgs_amd import jpeg
    files = [dc.golden()[n][0] for n in RGB_17x33] + [_restart_variant()]
    probes = [jpeg.probe(f) for f in files]
    assert len({p["subsampling"] for p in probes}) == 3 and {p["restart_interval"] for p in probes} == {0, 3}
    want = [dc.expected(n) for n in RGB_17x33] + [dc.decode(files[3])]
    out, _ = _decode(files)
    for i in range(4):
        _same(out[i], want[i], f"image {i} of the batch")
    again, _ = _decode(files)
    assert np.array_equal(out, again)                                   # two identical runs
    alone, _ = _decode(files[2:3])
    assert np.array_equal(alone[0], out[2])                             # image 2 of the batch = a call of its own


# ------------------------------------------------------------------------------------------------- 4. malformed scans
def test_malformed_scans_cost_their_image_only(gpu):
    from deblurgs_amd import jpeg
    bad = dc.malformed_scans()
    gray = [dc.golden()["smooth_8x8_gray"][0], bad["invalid_code"][0], bad["over_long_block"][0], dc.golden()["smooth_8x8_gray"][0]]
    out, status = _decode(gray, expect_status=[0, bad["invalid_code"][1], bad["over_long_block"][1], 0])
    assert not out[1].any() and not out[2].any()
    _same(out[0], dc.expected("smooth_8x8_gray"), "the neighbour before")
    _same(out[3], dc.expected("smooth_8x8_gray"), "the neighbour after")
    good, _ = dc.golden()["noise_q100_4:4:4"]
    rgb = [good, bad["truncated_scan"][0], good]
    out, status = _decode(rgb, expect_status=[0, bad["truncated_scan"][1], 0])
    assert not out[1].any()
    _same(out[0], dc.expected("noise_q100_4:4:4"), "the neighbour before")
    _same(out[2], dc.expected("noise_q100_4:4:4"), "the neighbour after")
    with pytest.raises(ValueError, match=r"corrupt JPEG scan: file 1 \(restart interval ran out of bytes\)$"):
        jpeg.decode(rgb)


def test_a_plan_that_is_not_the_files_costs_a_status(gpu):
    """The kernels check the plan against the call: the plan of a 17 x 33 file handed in as a 9 x 9 call decodes nothing."""
    import torch
    from deblurgs_amd import jpeg
    from deblurgs_amd.raster_call import _stream
    L = _lib.lib()
    data = dc.golden()["smooth_17x33_4:4:4"][0]
    plan = jpeg.plan(data)
    blob = np.zeros(16 + plan.size + (len(data) + 15) // 16 * 16, np.uint8)
    blob[:16] = np.array([16 + plan.size, 16], np.uint64).view(np.uint8)
    blob[16:16 + plan.size] = plan
    blob[16 + plan.size:16 + plan.size + len(data)] = np.frombuffer(data, np.uint8)
    dev = torch.from_numpy(blob).cuda()
    out = torch.full((9 * 9 * 3 + 1,), GUARD, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    tmp = torch.empty(L.dgs_jpeg_decode_tmp_bytes(1, 9, 9, 3), dtype=torch.uint8, device="cuda")
    _lib.check(L.dgs_jpeg_decode(dev.data_ptr(), blob.size, dev.data_ptr(), 1, 9, 9, 3, 1, out.data_ptr(), 9 * 9 * 3 + 1,
                                 status.data_ptr(), tmp.data_ptr(), _stream(torch.device("cuda:0"))), "dgs_jpeg_decode")
    assert status.item() == 1 and not out[:-1].any().item() and out[-1].item() == GUARD


# ------------------------------------------------------------------------------------------------- 5. the front end
def test_python_front_end(gpu, tmp_path):
    import torch
    from deblurgs_amd import jpeg
    files = [dc.golden()[n][0] for n in RGB_17x33]
    got = jpeg.decode(files)                                            # 17 * 33 * 3 is odd: the padded-row route
    for i, n in enumerate(RGB_17x33):
        _same(got[i].cpu().numpy(), dc.expected(n), n)
    out = torch.empty((3, 17, 33, 3), dtype=torch.uint8, device="cuda")
    assert jpeg.decode(files, out=out) is out and torch.equal(out, got)
    paths = [str(tmp_path / f"{i}.jpg") for i in range(3)]
    for p, f in zip(paths, files):
        with open(p, "wb") as fh:
            fh.write(f)
    assert torch.equal(jpeg.read_files(paths), got)
    gray = jpeg.decode([dc.golden()["smooth_9x9_gray"][0]])
    assert gray.shape == (1, 9, 9, 1)
    _same(gray[0].cpu().numpy(), dc.expected("smooth_9x9_gray"), "gray")
    with pytest.raises(ValueError, match="share one size: file 1"):
        jpeg.decode([files[0], dc.golden()["smooth_9x9_4:4:4"][0]])
    with pytest.raises(ValueError, match="file 1: corrupt JPEG"):
        jpeg.decode([files[0], files[1][:-2]])
    with pytest.raises(jpeg.Unsupported, match="file 0"):
        sof = files[0].index(b"\xff\xc0")
        jpeg.decode([files[0][:sof + 1] + b"\xc2" + files[0][sof + 2:]])
    with pytest.raises(ValueError, match="out must be"):
        jpeg.decode(files, out=out[:2])


# ------------------------------------------------------------------------------------------------- 6. scene loading
def test_load_colmap_scene_decodes_jpeg_on_the_device(gpu, tmp_path):
    """device_jpeg=True gives the ground truth that the same call gives with image_reader = the restatement; a picture
    that is no JPEG rides in the same upload group through the reader."""
    import torch
    from deblurgs_amd import jpeg, scene
    cameras, images, points = sc.scene_model()
    sc.write_model(os.path.join(str(tmp_path), "sparse", "0"), cameras, images, points)
    os.makedirs(os.path.join(str(tmp_path), "images"))
    rng = np.random.default_rng(9)
    pictures = np.stack([dc.content("smooth", 64, 96, 3, seed=k) for k in range(4)])
    pictures[1, 20:40, 30:60] = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    dev = torch.from_numpy(pictures).cuda()
    blobs = [jpeg.to_bytes(dev[0:1], 90, "4:2:0")[0], jpeg.to_bytes(dev[1:2], 75, "4:4:4")[0],
             jpeg.to_bytes(dev[2:3], 50, "4:2:0")[0]]
    for k, blob in enumerate(blobs):
        with open(os.path.join(str(tmp_path), "images", f"{k:03d}.jpg"), "wb") as f:
            f.write(blob)
    np.save(os.path.join(str(tmp_path), "images", "003.npy"), pictures[3])
    read = []

    def reader(path):
        read.append(os.path.basename(path))
        if path.endswith(".npy"):
            return np.load(path)
        with open(path, "rb") as f:
            return dc.decode(f.read())

    want = scene.load_colmap_scene(str(tmp_path), resolution=2, image_reader=reader)
    assert sorted(read) == ["000.jpg", "001.jpg", "002.jpg", "003.npy"]
    del read[:]
    got = scene.load_colmap_scene(str(tmp_path), resolution=2, image_reader=reader, device_jpeg=True)
    assert read == ["003.npy"]                                          # the three .jpg files never met the reader
    assert got.gt_images.shape == (4, 3, 32, 48) and torch.equal(got.gt_images, want.gt_images)
    assert got.image_names == want.image_names == ["000", "001", "002", "003"]


# ------------------------------------------------------------------------------------------------- 7. videos
def test_read_frames_of_a_motion_jpeg_avi(gpu, tmp_path):
    import torch
    from deblurgs_amd import video
    frames = np.stack([jc.image_for(34, 50, "4:2:0", seed=s) for s in range(3)])
    path = str(tmp_path / "clip.avi")
    video.write_video(torch.from_numpy(frames).cuda(), path, fps=24)
    with open(path, "rb") as f:
        data = f.read()
    _, files = video.parse_avi(data)
    assert len(files) == 3
    want = np.stack([dc.decode(f) for f in files])
    got = video.read_frames(path)
    assert got.shape == (3, 34, 50, 3) and got.device.type == "cuda"
    _same(got.cpu().numpy(), want, "frames")
    assert torch.equal(video.read_frames(data), got)

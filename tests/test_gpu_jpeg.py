"""JPEG files made on the device (dgs_jpeg_encode, deblurgs_amd/jpeg.py) against the numpy restatement of the byte
specification (tests/jpeg_cases.py, itself held against Pillow in tests/test_jpeg_host.py): device bytes == restatement bytes,
exactly.  There is no tolerance anywhere."""
import numpy as np
import pytest

import jpeg_cases as jc
from deblurgs_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SUB = {"gray": 0, "4:4:4": 0, "4:2:0": 1}
# the row kernel takes an MCU row JPEG_UNIT = 32 MCUs at a time (16 at 4:2:0): 256 pixels either way
UNIT_PX = 256
LARGEST = {}                    # mode -> (bytes, bound, what) of the largest file any case below produced


def _encode(images, quality, mode, image_stride=None, src_offset=0, what=""):
    """dgs_jpeg_encode through ctypes with guard bytes around files, sizes and tmp and a file stride that is no multiple of
    16.  images uint8 [n,h,w,c] (numpy).  Returns the list of file bytes; asserts the guards, sizes <= bound, that sizes[i]
    is the length the parser finds, and the untouched slot tails."""
    import torch
    from deblurgs_amd import jpeg
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
    bound = L.dgs_jpeg_bound(w, h, c, SUB[mode])
    stride_f = bound + 7 if (bound + 7) % 16 else bound + 9       # file i starts at any alignment
    assert bound > 0 and stride_f % 16 != 0
    g = 67
    files = torch.full((g + n * stride_f + g,), GUARD, dtype=torch.uint8, device=dev)
    sizes = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    tmp_bytes = L.dgs_jpeg_tmp_bytes(n, w, h, c, SUB[mode])
    assert tmp_bytes > 0
    tmp = torch.full((g + tmp_bytes + g,), GUARD, dtype=torch.uint8, device=dev)
    _lib.check(L.dgs_jpeg_encode(src.data_ptr() + src_offset, n, w, h, c, stride_i, quality, SUB[mode], files.data_ptr() + g,
                                 stride_f, sizes.data_ptr() + 8, tmp.data_ptr() + g, _stream(dev)), "dgs_jpeg_encode")
    torch.cuda.synchronize()
    files, sizes, tmp = files.cpu().numpy(), sizes.cpu().numpy(), tmp.cpu().numpy()
    assert sizes[0] == -7 and sizes[-1] == -7
    assert (files[:g] == GUARD).all() and (files[g + n * stride_f:] == GUARD).all()
    assert (tmp[:g] == GUARD).all() and (tmp[g + tmp_bytes:] == GUARD).all()
    out = []
    for i in range(n):
        size = int(sizes[1 + i])
        assert 334 < size <= bound, (size, bound)
        slot = files[g + i * stride_f:g + (i + 1) * stride_f]
        assert (slot[size:] == GUARD).all(), "bytes of the slot past sizes[i] were written"
        data = slot[:size].tobytes()
        assert list(jpeg.segments(data))[-1] == (0xD9, b"") and data.endswith(b"\xff\xd9")       # the parser ends at sizes[i]
        if size > LARGEST.get(mode, (0,))[0]:
            LARGEST[mode] = (size, bound, what or f"{h}x{w} q{quality}")
        out.append(data)
    return out


def _image(h, w, mode, seed):
    image = jc.image_for(h, w, mode, seed)
    return image[..., None] if mode == "gray" else image


def _same(got, want, what):
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} device bytes, {len(want)} expected, first difference at byte {first}")


# ------------------------------------------------------------------------------------------------- 1. sizes, qualities
@pytest.mark.parametrize("mode", jc.MODES)
@pytest.mark.parametrize("h,w", jc.HOST_SIZES)
def test_bytes_equal_the_restatement_at_quality_90(gpu, h, w, mode):
    image = _image(h, w, mode, seed=1000 * h + w)
    data, = _encode(image[None], 90, mode)
    _same(data, jc.encode(image, 90, mode), f"{h}x{w} {mode}")
    decoded = jc.decode(data)
    assert decoded.size == (w, h)


@pytest.mark.parametrize("mode", jc.MODES)
@pytest.mark.parametrize("quality", [1, 50, 100])
def test_bytes_equal_the_restatement_at_other_qualities(gpu, quality, mode):
    image = _image(17, 33, mode, seed=17033)
    data, = _encode(image[None], quality, mode)
    _same(data, jc.encode(image, quality, mode), f"q{quality} {mode}")


# ------------------------------------------------------------------------------------------------- 2. gray [n,h,w]
def test_gray_without_a_channel_axis(gpu):
    import torch
    from deblurgs_amd import jpeg
    images = np.stack([jc.image_for(20, 31, "gray", seed=s) for s in (1, 2)])
    assert images.shape == (2, 20, 31)
    blobs = jpeg.to_bytes(torch.from_numpy(images).cuda(), quality=75)
    for i in range(2):
        _same(blobs[i], jc.encode(images[i], 75, "gray"), f"gray {i}")
        assert jc.decode(blobs[i]).mode == "L"
    assert jpeg.to_bytes(torch.from_numpy(images[..., None]).cuda(), quality=75, subsampling="4:4:4") == blobs


# ------------------------------------------------------------------------------------------------- 3. units, RST wrap
@pytest.mark.parametrize("h,w,mode", [(8, 1040, "gray"), (8, 1040, "4:4:4"), (16, 2064, "4:2:0")])
def test_one_mcu_row_wider_than_two_units(gpu, h, w, mode):
    assert w > 2 * UNIT_PX * (2 if mode == "4:2:0" else 1) and w % UNIT_PX != 0       # a third (fifth) unit, not a full one
    image = _image(h, w, mode, seed=w)
    image[:, 500:700] = jc.random_image(h, 200, image.shape[2], seed=3)               # bits that straddle the unit edges
    data, = _encode(image[None], 90, mode)
    _same(data, jc.encode(image, 90, mode), f"{h}x{w} {mode}")


@pytest.mark.parametrize("h,w,mode", [(80, 8, "4:4:4"), (144, 16, "4:2:0")])
def test_more_than_eight_mcu_rows_wrap_the_rst_index(gpu, h, w, mode):
    image = _image(h, w, mode, seed=h)
    data, = _encode(image[None], 90, mode)
    _same(data, jc.encode(image, 90, mode), f"{h}x{w} {mode}")
    rows = h // (16 if mode == "4:2:0" else 8)
    markers = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert rows > 8 and markers == [0xD0 + (r & 7) for r in range(rows - 1)]


# ------------------------------------------------------------------------------------------------- 4. constructed content
def test_a_block_whose_only_ac_level_is_the_last(gpu):
    image = jc.last_coefficient_block()
    zz, = [b for b, _ in jc.mcu_rows(image, 50, "gray")[0]]
    assert not zz[1:63].any() and zz[63] != 0                            # three ZRLs, no EOB
    data, = _encode(image[None, ..., None], 50, "gray")
    _same(data, jc.encode(image, 50, "gray"), "last coefficient")


def test_a_dc_difference_of_category_11(gpu):
    image = jc.black_beside_white()
    dcs = [int(b[0]) for b, _ in jc.mcu_rows(image, 100, "gray")[0]]
    assert (dcs[1] - dcs[0]).bit_length() == 11
    data, = _encode(image[None, ..., None], 100, "gray")
    _same(data, jc.encode(image, 100, "gray"), "black beside white")
    rgb = np.repeat(image[..., None], 3, axis=2)                          # the chroma tables code a flat 128
    for mode in ("4:4:4", "4:2:0"):
        _same(_encode(rgb[None], 100, mode)[0], jc.encode(rgb, 100, mode), mode)


@pytest.fixture(scope="module")
def noise():
    return jc.random_image(64, 64, 3, seed=1)


@pytest.mark.parametrize("mode", jc.MODES)
def test_noise_at_quality_100_stuffing_and_full_blocks(gpu, noise, mode):
    image = noise[..., :1] if mode == "gray" else noise
    assert any(b"\xff\x00" in row for row in jc.scan_rows(image, 100, mode))
    assert any(b[1:].all() for row in jc.mcu_rows(image, 100, mode) for b, _ in row)      # all 63 AC levels non-zero
    data, = _encode(image[None], 100, mode, what="64x64 noise q100")
    _same(data, jc.encode(image, 100, mode), f"noise {mode}")


def test_the_predictor_resets_in_every_mcu_row(gpu):
    image = np.full((24, 8), 200, np.uint8)
    rows = jc.mcu_rows(image, 50, "gray")
    assert len(rows) == 3 and len({jc.row_bits(r) for r in rows}) == 1
    data, = _encode(image[None, ..., None], 50, "gray")
    _same(data, jc.encode(image, 50, "gray"), "constant 200")
    rgb = np.full((40, 24, 3), 200, np.uint8)
    _same(_encode(rgb[None], 50, "4:2:0")[0], jc.encode(rgb, 50, "4:2:0"), "constant 200 4:2:0")


# ------------------------------------------------------------------------------------------------- 5. the bound
def test_the_largest_file_stays_inside_the_bound(gpu, noise):
    """_encode holds every file of every case to sizes[i] <= dgs_jpeg_bound, to the parser's length and to an untouched
    tail; here the noise images run (again, if this test runs alone) and the largest file of the module is reported."""
    for mode in jc.MODES:
        image = noise[..., :1] if mode == "gray" else noise
        data, = _encode(image[None], 100, mode, what="64x64 noise q100")
        assert len(data) <= _lib.lib().dgs_jpeg_bound(64, 64, image.shape[2], SUB[mode])
    for mode, (size, bound, what) in LARGEST.items():
        print(f"largest {mode} file: {size} of {bound} bytes ({what})")
        assert size <= bound


# ------------------------------------------------------------------------------------------------- 6. batch, determinism
def test_batch_strides_alignment_and_determinism(gpu):
    import torch
    from deblurgs_amd import jpeg
    images = np.stack([jc.smooth_patch(33, 211, 3, seed=8), jc.random_image(33, 211, 3, seed=9),
                       np.full((33, 211, 3), 7, np.uint8)])
    per = images[0].size
    want = [jc.encode(images[i], 90, "4:2:0") for i in range(3)]
    batch = _encode(images, 90, "4:2:0", image_stride=per + 13)
    for i in range(3):
        _same(batch[i], want[i], f"image {i} of the batch")
        assert _encode(images[i:i + 1], 90, "4:2:0") == [batch[i]], i    # file i of the batch = a call of its own
    assert _encode(images, 90, "4:2:0", image_stride=per + 13) == batch               # a second call
    assert _encode(images, 90, "4:2:0", image_stride=per + 13, src_offset=1) == batch   # a source one byte off alignment
    # a sliced files= buffer through the front end: rows of a wider tensor, starting 5 bytes in
    need = jpeg.bound(211, 33, 3, "4:2:0")
    wide = torch.full((3, need + 40), GUARD, dtype=torch.uint8, device="cuda")
    files, sizes = jpeg.encode(torch.from_numpy(images).cuda(), 90, "4:2:0", files=wide[:, 5:5 + need + 3])
    host, host_sizes = wide.cpu().numpy(), sizes.view(torch.int64).cpu().tolist()
    for i in range(3):
        assert host[i, 5:5 + host_sizes[i]].tobytes() == want[i]
        assert (host[i, :5] == GUARD).all() and (host[i, 5 + host_sizes[i]:] == GUARD).all()


# ------------------------------------------------------------------------------------------------- 7. the front end
def test_python_front_end(gpu, tmp_path):
    import torch
    from deblurgs_amd import jpeg
    images = np.stack([jc.smooth_patch(20, 31, 3, seed=10), jc.random_image(20, 31, 3, seed=11)])
    dev = torch.from_numpy(images).cuda()
    files, sizes = jpeg.encode(dev)
    assert files.dtype == torch.uint8 and sizes.dtype == torch.uint64 and files.shape[1] >= jpeg.bound(31, 20, 3)
    blobs = jpeg.to_bytes(dev)
    for i in range(2):
        _same(blobs[i], jc.encode(images[i], 90, "4:2:0"), f"default arguments {i}")
    assert jpeg.to_bytes(dev, 60, "4:4:4")[1] == jc.encode(images[1], 60, "4:4:4")
    paths = jpeg.write_files(dev, [str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")])
    assert [open(p, "rb").read() for p in paths] == blobs
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.encode(torch.from_numpy(images))
    with pytest.raises(ValueError, match="uint8"):
        jpeg.encode(dev.float())
    with pytest.raises(ValueError, match="channels"):
        jpeg.encode(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="quality"):
        jpeg.encode(dev, quality=0)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg.encode(dev, subsampling="4:2:2")
    with pytest.raises(ValueError, match="one path"):
        jpeg.write_files(dev, ["only-one.jpg"])
    assert jpeg.encode(dev[:0])[1].numel() == 0

"""The front end the device encoders share (deblurgs_amd/device_files.py), as far as it goes without a GPU: its refusals.
The device side is held to the files' own bytes in tests/test_gpu_png.py, test_gpu_jpeg.py and test_gpu_video.py."""
import pytest
import torch

import jpeg_cases as jc
from deblurgs_amd import device_files, jpeg, png, video


class _AsOnDevice:
    """A host tensor that says it is on a HIP device: what the checks behind the device check read of a tensor."""

    def __init__(self, t):
        self.device, self.dtype, self.shape, self.dim = torch.device("cuda"), t.dtype, t.shape, t.dim


def test_tensors_the_encoders_refuse():
    u8 = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    for module in (png, jpeg):
        with pytest.raises(RuntimeError, match=f"{module.__name__.split('.')[-1]}.encode needs .*no CPU fallback"):
            module.encode(u8)
        with pytest.raises(ValueError, match="takes a uint8"):
            module.encode(_AsOnDevice(u8.float()))
        with pytest.raises(ValueError, match="takes a uint8"):
            module.encode(_AsOnDevice(u8[0, 0]))
    with pytest.raises(ValueError, match="channels, not 5"):
        png.encode(_AsOnDevice(torch.zeros((1, 4, 4, 5), dtype=torch.uint8)))
    for c in (2, 4):
        with pytest.raises(ValueError, match=f"channels, not {c}"):
            jpeg.encode(_AsOnDevice(torch.zeros((1, 4, 4, c), dtype=torch.uint8)))
    with pytest.raises(ValueError):
        png.bound(4, 4, 5)                               # (the format's own bound refuses them as well)


def test_files_buffers_the_encoders_refuse():
    cpu = torch.device("cpu")
    need = 100
    assert device_files.files_buffer(None, 3, need, cpu).shape == (3, 112)          # rows rounded up to 16
    wide = torch.zeros((3, 140), dtype=torch.uint8)
    assert device_files.files_buffer(wide[:, 5:5 + need], 3, need, cpu).stride(0) == 140
    # too narrow, too few rows, another type, one or three dimensions, an inner stride of two
    for bad in (wide[:, :need - 1], wide[:2], wide.float(), wide[0], wide[:, :need, None], torch.zeros((3, 2 * need), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match=f"files must be a uint8 \\[n, >= {need}\\]"):
            device_files.files_buffer(bad, 3, need, cpu)
    with pytest.raises(ValueError, match="files must be a uint8"):
        device_files.files_buffer(wide, 3, need, torch.device("cuda"))              # another device than the images'


def test_write_files_wants_one_path_per_image():
    with pytest.raises(ValueError, match="one path per image"):
        device_files.write_files(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), ["only-one.png"], lambda images: [])


def test_the_writer_adds_finished_files_of_one_size(tmp_path):
    big = [jc.encode(jc.smooth_patch(16, 24, 3, seed=s), 90, "4:2:0") for s in range(3)]
    small = jc.encode(jc.smooth_patch(8, 8, 3, seed=0), 90, "4:4:4")
    with video.MjpegAviWriter(str(tmp_path / "added.avi"), 20) as w:
        w.add(big[0], (24, 16))
        w.add(big[1])
        with pytest.raises(ValueError, match="one size"):
            w.add(small, (8, 8))
        with pytest.raises(ValueError, match="one size"):
            w.add(small)
        w.append(big[2])
    assert video.parse_avi(open(tmp_path / "added.avi", "rb").read())[1] == big
    with pytest.raises(ValueError, match="closed"):
        w.add(big[0])

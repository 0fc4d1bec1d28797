"""JPEG files made on the device (dgs_jpeg_encode, deblurgs_amd/csrc/jpeg.hip).

    encode(images, quality, subsampling)   uint8 [n,h,w,3], [n,h,w,1] or [n,h,w] on the device -> (files [n,stride] uint8,
                               sizes [n] uint64), both on the device: file i is files[i, :sizes[i]], a complete baseline JFIF
                               .jpg (its own quantisation and Huffman tables, one restart interval per MCU row).  No host
                               pass over the bytes, no synchronisation.
    to_bytes(images, ...)      the files as a list of bytes: one read of the sizes, then a copy of sizes[i] bytes each.
    write_files(images, paths, ...)   to_bytes, written.  (All three are thin: the tensor checks, the buffers and the
                               download are deblurgs_amd/device_files.py's, shared with png.py.)
    segments(data)             a small HOST parser of a JPEG byte string: (marker, payload) per segment, the entropy-coded
                               bytes as the payload of the SOS entry's successor (tests, tools).

and decoded there (dgs_jpeg_decode, deblurgs_amd/csrc/jpeg_decode.hip): baseline files -- SOF0, one scan, gray or 4:4:4 /
4:2:2 / 4:2:0, with or without restart markers, any Huffman tables -- to Pillow's pixels, bit for bit.

    probe(data)                what the decoder would do with a file, from its plan (host only): size, channels,
                               subsampling, restart interval, intervals.  Raises Unsupported (a ValueError) with the reason
                               for a file it does not take, ValueError for a corrupt one.
    decode(files, device)      a list of bytes of one size -> uint8 [n,h,w,c] on the device: one upload of files and plans,
                               one read of the per-file status.  A scan is decoded one lane per restart interval: a file
                               without DRI on ONE lane.
    read_files(paths)          decode of the files named.
    plan(data)                 the plan itself (dgs_jpeg_decode_plan): scene.py makes it once per file and hands it to decode.

Three channels are RGB, one is gray.  subsampling "4:4:4" or "4:2:0" (ignored for gray); quality 1..100 scales the Annex K
tables the way libjpeg does.  Colour conversion, the 8 x 8 transform and the quantiser are integer arithmetic stated in
include/dgs_hip.h: the bytes are a function of the pixels (tests/jpeg_cases.py restates them in numpy).  Opt-in: video.py
wraps the files into a Motion-JPEG AVI, render_path.write_frames_video writes a camera path.
"""
import ctypes

import numpy as np

from . import _lib, device_files

SUBSAMPLING = {"4:4:4": 0, "4:2:0": 1}      # DGS_JPEG_444, DGS_JPEG_420
SOI, EOI, SOS = 0xD8, 0xD9, 0xDA
SCAN = -1                                   # the "marker" segments() gives the entropy-coded bytes


def _subsampling(subsampling):
    try:
        return SUBSAMPLING[subsampling]
    except (KeyError, TypeError):
        raise ValueError(f"subsampling must be '4:4:4' or '4:2:0' (got {subsampling!r})") from None


def bound(w, h, c, subsampling="4:2:0"):
    """The bytes one file can take (dgs_jpeg_bound): 625 (334 gray) + 416 per 8 x 8 block + 2 per MCU row + 2."""
    b = _lib.lib().dgs_jpeg_bound(int(w), int(h), int(c), _subsampling(subsampling))
    if b == 0:
        raise ValueError(f"no JPEG of {w} x {h} x {c}: sizes must be 1..65535, channels 1 or 3")
    return b


def encode(images, quality=90, subsampling="4:2:0", files=None):
    """(files [n,stride] uint8, sizes [n] uint64) on the device; stride >= bound(w, h, c, subsampling).  files: a uint8
    device tensor [n,stride] to write into (e.g. a reused buffer); bytes of a row past sizes[i] are left as they are."""
    images = device_files.as_nhwc(images, "jpeg.encode", "[n,h,w,3], [n,h,w,1] or [n,h,w]", (1, 3))
    sub = _subsampling(subsampling)
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality must be 1..100 (got {quality})")
    n, h, w, c = (int(s) for s in images.shape)
    L = _lib.lib()
    return device_files.encode(
        images, bound(w, h, c, subsampling), L.dgs_jpeg_tmp_bytes(n, w, h, c, sub), files,
        lambda src, *out: L.dgs_jpeg_encode(src, n, w, h, c, h * w * c, quality, sub, *out), "dgs_jpeg_encode")


def to_bytes(images, quality=90, subsampling="4:2:0"):
    """The n files as a list of bytes (one host read of the sizes, then sizes[i] bytes of each file)."""
    return device_files.download(*encode(images, quality, subsampling))


def write_files(images, paths, quality=90, subsampling="4:2:0"):
    """images [n,...] -> the n files named by paths.  Returns the paths."""
    return device_files.write_files(images, paths, lambda images: to_bytes(images, quality, subsampling))


# ------------------------------------------------------------------------------------------------- decoding
class Unsupported(ValueError):
    """A valid JPEG of a kind the device decoder does not take (progressive, CMYK, ...): hand it to a host reader."""


def plan(data):
    """The decode plan of one file (dgs_jpeg_decode_plan, on the host): a uint8 numpy array that starts with a
    _lib.DgsJpegPlan.  Raises Unsupported with the reason, ValueError for a stream that breaks the format."""
    data = bytes(data)
    L = _lib.lib()
    need = ctypes.c_size_t()
    rc = L.dgs_jpeg_decode_plan_bytes(data, len(data), ctypes.byref(need))
    if rc == 0:
        out = np.zeros(need.value // 8, dtype=np.uint64).view(np.uint8)      # (8-byte aligned)
        rc = L.dgs_jpeg_decode_plan(data, len(data), out.ctypes.data, out.size)
        if rc == 0:
            return out
    reason = L.dgs_last_error().decode("utf-8", "replace")
    if rc == _lib.E_JPEG_UNSUPPORTED:
        raise Unsupported(reason)
    if rc == _lib.E_JPEG_CORRUPT:
        raise ValueError(f"corrupt JPEG: {reason}")
    raise RuntimeError(f"libdgs_hip dgs_jpeg_decode_plan failed (code {rc}): {reason}")


def _head(plan_bytes):
    return _lib.DgsJpegPlan.from_buffer_copy(plan_bytes[:ctypes.sizeof(_lib.DgsJpegPlan)].tobytes())


def probe(data):
    """What the device decoder would do with the file: a dict -- width, height, channels, subsampling ("gray", "4:4:4",
    "4:2:2" or "4:2:0"), restart_interval (MCUs, 0 = none), intervals (the lanes its scan is decoded on).  No GPU needed.
    Raises Unsupported (a ValueError) with the reason for a file the decoder does not take."""
    p = _head(plan(data))
    sub = "gray" if p.channels == 1 else {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}[p.hs, p.vs]
    return {"width": p.w, "height": p.h, "channels": p.channels, "subsampling": sub, "restart_interval": p.restart_interval,
            "intervals": p.n_intervals}


def decode(files, device="cuda", out=None, plans=None):
    """files: a list of JPEG byte strings of one size and channel count -> uint8 [n,h,w,c] on the device (c = 3: RGB, 1:
    gray), Pillow's pixels.  The plans are made on the host, files and plans go up in ONE copy, the kernels run
    (dgs_jpeg_decode) and the per-file status comes back in ONE read.  out: a uint8 [n,h,w,c] device tensor to write into;
    plans: what plan() gave for each file, where the caller has them already.  Raises Unsupported / ValueError from the
    parser (naming the file's index) and ValueError naming the files whose scans turned out malformed on the device."""
    import torch
    from .raster_call import _ptr, _stream
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("jpeg.decode needs a HIP device (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    files = [bytes(f) for f in files]
    n = len(files)
    if n == 0:
        raise ValueError("jpeg.decode needs at least one file")
    if plans is None:
        plans = []
        for i, f in enumerate(files):
            try:
                plans.append(plan(f))
            except Unsupported as e:
                raise Unsupported(f"file {i}: {e}") from None
            except ValueError as e:
                raise ValueError(f"file {i}: {e}") from None
    heads = [_head(p) for p in plans]
    w, h, c = heads[0].w, heads[0].h, heads[0].channels
    for i, p in enumerate(heads):
        if (p.w, p.h, p.channels) != (w, h, c):
            raise ValueError(f"the files of one decode call share one size: file {i} is {p.w} x {p.h} x {p.channels}, "
                             f"file 0 is {w} x {h} x {c}")
    # one host buffer: the index (file offset, plan offset per image), the plans (8-byte aligned), the files (4-byte)
    host, at = device_files.pack([(p, 8) for p in plans] + [(np.frombuffer(f, dtype=np.uint8), 4) for f in files],
                                 reserve=16 * n)
    host.numpy()[:16 * n] = np.array([at[n:], at[:n]], dtype=np.uint64).T.reshape(-1).view(np.uint8)
    with torch.cuda.device(device):
        dev = host.to(device, non_blocking=True)
        if out is None:
            out = torch.empty((n, h, w, c), dtype=torch.uint8, device=device)
        elif (out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, c) or out.device != device or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 [{n},{h},{w},{c}] tensor on {device}")
        L = _lib.lib()
        stride = (h * w * c + 3) // 4 * 4           # (packed stores: every image starts on a dword)
        if n > 1 and stride != h * w * c:
            target = torch.empty((n, stride), dtype=torch.uint8, device=device)      # rows of a padded buffer, compacted below
        else:
            target = out
        status = torch.empty(n, dtype=torch.int32, device=device)
        tmp = torch.empty(max(L.dgs_jpeg_decode_tmp_bytes(n, w, h, c), 16), dtype=torch.uint8, device=device)
        _lib.check(L.dgs_jpeg_decode(_ptr(dev), dev.numel(), _ptr(dev), n, w, h, c, max(p.n_intervals for p in heads),
                                     _ptr(target), stride, _ptr(status), _ptr(tmp), _stream(device)), "dgs_jpeg_decode")
        if target is not out:
            out.view(n, -1).copy_(target[:, :h * w * c])
        bad = status.cpu().tolist()
    if any(bad):
        raise ValueError("corrupt JPEG scan: " + ", ".join(
            f"file {i} ({_lib.JPEG_STATUS.get(s, s)})" for i, s in enumerate(bad) if s))
    return out


def read_files(paths, device="cuda"):
    """The .jpg files named by paths (one size, one channel count) -> uint8 [n,h,w,c] on the device."""
    blobs = []
    for path in paths:
        with open(path, "rb") as f:
            blobs.append(f.read())
    return decode(blobs, device)


def segments(data):
    """Yields (marker, payload) for every segment of the JPEG byte string `data`, from SOI to EOI (both with an empty
    payload); the entropy-coded bytes that follow SOS -- stuffed, with their RST markers -- come as (SCAN, bytes).  Raises
    ValueError on a stream that does not start with SOI, on a segment that runs past the end and on a missing EOI."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG: no SOI")
    yield SOI, b""
    at = 2
    while True:
        if at + 2 > len(data):
            raise ValueError("truncated JPEG: no EOI")
        if data[at] != 0xFF:
            raise ValueError(f"not a JPEG marker at byte {at}")
        marker = data[at + 1]
        if marker == EOI:
            yield EOI, b""
            return
        if at + 4 > len(data):
            raise ValueError("truncated JPEG segment header")
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if length < 2 or at + 2 + length > len(data):
            raise ValueError("JPEG segment runs past the end")
        yield marker, data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == SOS:
            end = at
            while True:         # the scan ends at the first marker that is neither a stuffed 0xFF nor an RST
                end = data.find(b"\xff", end)
                if end < 0 or end + 1 >= len(data):
                    raise ValueError("truncated JPEG scan")
                if data[end + 1] == 0 or 0xD0 <= data[end + 1] <= 0xD7:
                    end += 2
                    continue
                break
            yield SCAN, data[at:end]
            at = end

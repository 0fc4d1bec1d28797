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

Three channels are RGB, one is gray.  subsampling "4:4:4" or "4:2:0" (ignored for gray); quality 1..100 scales the Annex K
tables the way libjpeg does.  Colour conversion, the 8 x 8 transform and the quantiser are integer arithmetic stated in
include/dgs_hip.h: the bytes are a function of the pixels (tests/jpeg_cases.py restates them in numpy).  Opt-in: video.py
wraps the files into a Motion-JPEG AVI, render_path.write_frames_video writes a camera path.
"""
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

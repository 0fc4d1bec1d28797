"""PNG files made on the device (dgs_png_encode, deblurgs_amd/csrc/png.hip).

    encode(images)             uint8 [n,h,w,c] or [n,h,w] on the device -> (files [n,stride] uint8, sizes [n] uint64), both
                               on the device: file i is files[i, :sizes[i]], a complete .png (signature, IHDR, one IDAT,
                               IEND, every CRC).  No host pass over the bytes, no synchronisation.
    to_bytes(images)           the files as a list of bytes: one read of the sizes, then a copy of sizes[i] bytes each.
    write_files(images, paths) to_bytes, written.  (All three are thin: the tensor checks, the buffers and the download are
                               deblurgs_amd/device_files.py's, shared with jpeg.py.)
    chunks(data)               a small HOST parser of a PNG byte string: (type, payload, crc_ok) per chunk (tests, tools).

c = 1 / 2 / 3 / 4 is gray / gray + alpha / RGB / RGBA.  Row filters by the smallest sum of |residual as int8|, deflate in
independent DGS_PNG_SEGMENT-byte segments with zlib's Z_RLE tokens and a dynamic Huffman code per segment
(include/dgs_hip.h has the rules); the bytes are a function of the pixels.  Opt-in: report.write_view_report /
traj_render / evaluation.evaluate take device_png=True, render_path.write_frames_png writes a camera path.
"""
import struct
import zlib

from . import _lib, device_files

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}      # channels -> IHDR colour type


def bound(w, h, c):
    """The bytes one file can take (dgs_png_bound): 63 + F + 5 ceil(F / DGS_PNG_SEGMENT), F = h (1 + w c)."""
    b = _lib.lib().dgs_png_bound(int(w), int(h), int(c))
    if b == 0:
        raise ValueError(f"no PNG of {w} x {h} x {c}: sizes must be at least 1, channels 1..4, h (1 + w c) below 2^31")
    return b


def encode(images, files=None):
    """(files [n,stride] uint8, sizes [n] uint64) on the device; stride >= bound(w, h, c).  files: a uint8 device tensor
    [n,stride] to write into (e.g. a reused buffer); bytes of a row past sizes[i] are left as they are."""
    images = device_files.as_nhwc(images, "png.encode", "[n,h,w,c] or [n,h,w]", COLOR_TYPE)
    n, h, w, c = (int(s) for s in images.shape)
    L = _lib.lib()
    return device_files.encode(
        images, bound(w, h, c), L.dgs_png_tmp_bytes(n, w, h, c), files,
        lambda src, *out: L.dgs_png_encode(src, n, w, h, c, h * w * c, *out), "dgs_png_encode")


def to_bytes(images):
    """The n files as a list of bytes (one host read of the sizes, then sizes[i] bytes of each file)."""
    return device_files.download(*encode(images))


def write_files(images, paths):
    """images [n,...] -> the n files named by paths.  Returns the paths."""
    return device_files.write_files(images, paths, to_bytes)


def chunks(data):
    """Yields (type, payload, crc_ok) for every chunk of the PNG byte string `data`; raises ValueError on a wrong signature
    or a chunk that runs past the end."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG: wrong signature")
    at = 8
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError("truncated PNG chunk header")
        length, = struct.unpack(">I", data[at:at + 4])
        end = at + 12 + length
        if end > len(data):
            raise ValueError("PNG chunk runs past the end")
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + length]
        crc, = struct.unpack(">I", data[end - 4:end])
        yield kind, payload, zlib.crc32(kind + payload) == crc
        at = end

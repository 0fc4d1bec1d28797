"""Videos of device frames: a Motion-JPEG AVI whose frames are the .jpg files dgs_jpeg_encode makes (deblurgs_amd/jpeg.py).

    MjpegAviWriter(path, fps, quality, subsampling)   append(frames): a device uint8 [n,h,w,3] is encoded on the device and
                               sizes[i] bytes per frame cross to the host through the writer's pinned buffer (one
                               device_files.Download, its three steps back to back); bytes (or a list of bytes) are taken
                               as finished JPEG files, so the container needs no GPU.  add(data, (w, h)) takes one finished
                               file whose size the caller knows (render_path.write_frames_video).  close() writes the index
                               and the header counts.  A context manager.
    write_video(frames, path, fps, ...)   the one-shot form for a device tensor.
    make_video(imgs, path, fps=32)        the reference's make_video (utils/export_utils.py:153): numpy arrays, lists of
                               frames or host tensors are uploaded in groups; device tensors are taken as they are.  It fits
                               the writer= parameter of render_path.render_spiral / render_trainview.
    parse_avi(data)            a small HOST parser: (header dict, [frame bytes]) (tests, tools).
    read_frames(path_or_bytes, device)    the frames of a Motion-JPEG AVI as a device uint8 [n,h,w,3]: parse_avi, then
                               jpeg.decode (one upload, the frames decoded on the device).

The container is built on the host: it is 8 bytes per frame plus an index.  AVI 1.0: RIFF 'AVI ' { LIST 'hdrl' { avih,
LIST 'strl' { strh (vids / MJPG, dwScale / dwRate = the frame rate as a reduced fraction), strf (BITMAPINFOHEADER, MJPG,
24 bits) } }, LIST 'movi' { 00dc chunks padded to even length }, idx1 (16 bytes per frame: 00dc, AVIIF_KEYFRAME, the offset
from the 'movi' fourcc, the size) }.  Every frame is a key frame and a complete .jpg with its own tables.  All frames of
a file share one size.  A file stays below 2 GiB (OpenDML's extended index is not written): append raises before the frame
that would cross it.  No audio.
"""
import struct
from fractions import Fraction

import numpy as np

from . import device_files, jpeg

MAX_FILE_BYTES = 1 << 31            # RIFF sizes are 32-bit and players treat them as signed
HEADER_BYTES = 224                  # everything before the first 00dc chunk
MOVI_AT = 220                       # offset of the 'movi' fourcc: index offsets count from here
UPLOAD_GROUP = 8                    # frames make_video uploads per encode call
HOST_BYTES = 1 << 16                # what a pinned host buffer for JPEG files starts with (jpeg.bound is the worst case of
                                    # noise at quality 100; the buffer doubles to what the frames really take)
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10


def frame_rate(fps):
    """fps as a reduced fraction (dwRate, dwScale): 32 -> (32, 1), 29.97 -> (2997, 100), 30000 / 1001 -> (30000, 1001)."""
    f = fps if isinstance(fps, Fraction) else Fraction(str(fps))
    f = f.limit_denominator(1 << 16)
    if f <= 0:
        raise ValueError(f"fps must be positive (got {fps!r})")
    return f.numerator, f.denominator


def jpeg_size(data):
    """(w, h) from the SOF0 segment of a JPEG byte string."""
    for marker, payload in jpeg.segments(data):
        if marker == 0xC0:
            h, w = struct.unpack(">HH", payload[1:5])
            return w, h
    raise ValueError("no SOF0 segment: not a baseline JPEG")


def _header(w, h, rate, scale, n_frames, largest, movi_bytes):
    """The HEADER_BYTES bytes before the first frame chunk.  movi_bytes: the size field of LIST 'movi'."""
    usec = (1000000 * scale + rate // 2) // rate
    avih = struct.pack("<14I", usec, (largest * rate + scale - 1) // scale, 0, AVIF_HASINDEX, n_frames, 0, 1, largest, w, h,
                       0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n_frames, largest, 0xFFFFFFFF, 0,
                       0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", 3 * w * h, 0, 0, 0, 0)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    riff_bytes = 4 + 8 + len(hdrl) + 8 + movi_bytes + 8 + 16 * n_frames
    out = (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
           b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
    assert len(out) == HEADER_BYTES and out[MOVI_AT:MOVI_AT + 4] == b"movi"
    return out


class MjpegAviWriter:
    def __init__(self, path, fps, quality=90, subsampling="4:2:0"):
        self.rate, self.scale = frame_rate(fps)
        self.quality, self.subsampling = int(quality), subsampling
        self.path = path
        self.size = None                    # (w, h) of the first frame
        self.index = []                     # (offset from the 'movi' fourcc, size) per frame
        self._download = None               # device_files.Download, made by the first device tensor
        self._f = open(path, "wb")
        self._f.write(bytes(HEADER_BYTES))
        self._at = HEADER_BYTES

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def n_frames(self):
        return len(self.index)

    def add(self, data, size=None):
        """One finished JPEG file as a 00dc chunk.  size: its (w, h) where the caller knows it (else read from its SOF0)."""
        if self._f is None:
            raise ValueError("the writer is closed")
        size = jpeg_size(data) if size is None else size
        if self.size is None:
            self.size = size
        elif size != self.size:
            raise ValueError(f"all frames of a file share one size: {self.size[0]} x {self.size[1]}, got {size[0]} x {size[1]}")
        padded = len(data) + (len(data) & 1)
        if self._at + 8 + padded + 8 + 16 * (len(self.index) + 1) >= MAX_FILE_BYTES:
            raise ValueError(f"{self.path}: frame {len(self.index)} would take the file to 2 GiB (AVI 1.0; OpenDML is not "
                             "written): close this file and start another")
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1))
        self.index.append((self._at - MOVI_AT, len(data)))
        self._at += 8 + padded

    def append(self, frames):
        """frames: a uint8 [n,h,w,3] tensor on a HIP device (encoded there), or finished JPEG bytes / a list of them."""
        if isinstance(frames, (bytes, bytearray, memoryview)):
            return self.add(bytes(frames))
        if isinstance(frames, (list, tuple)) and all(isinstance(f, (bytes, bytearray, memoryview)) for f in frames):
            for f in frames:
                self.add(bytes(f))
            return None
        import torch
        if not isinstance(frames, torch.Tensor):
            raise TypeError("append takes a device uint8 [n,h,w,3] tensor or JPEG bytes (make_video uploads host arrays)")
        if frames.device.type != "cuda":
            raise RuntimeError("MjpegAviWriter.append needs a tensor on a HIP device (no CPU fallback)")
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("MjpegAviWriter.append takes a uint8 [n,h,w,3] tensor")
        if self._download is None:
            self._download = device_files.Download(HOST_BYTES)
        self._download.read_sizes(*jpeg.encode(frames, self.quality, self.subsampling))
        self._download.copy_bytes()
        for data in self._download.blobs():
            self.add(data, (int(frames.shape[2]), int(frames.shape[1])))
        return None

    def close(self):
        """Writes idx1 and the header with the final counts.  A writer that got no frame leaves an empty movi list."""
        if self._f is None:
            return self.path
        f, self._f = self._f, None
        with f:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
            for offset, size in self.index:
                f.write(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, offset, size))
            w, h = self.size or (0, 0)
            largest = max((s for _, s in self.index), default=0)
            f.seek(0)
            f.write(_header(w, h, self.rate, self.scale, len(self.index), largest, self._at - MOVI_AT))
        return self.path


def write_video(frames, path, fps, quality=90, subsampling="4:2:0"):
    """frames: a uint8 [n,h,w,3] tensor on a HIP device -> one .avi.  Returns the path."""
    with MjpegAviWriter(path, fps, quality, subsampling) as w:
        w.append(frames)
    return path


def make_video(imgs, path, fps=32, quality=90, subsampling="4:2:0", device="cuda"):
    """The reference's make_video(imgs, path, fps): imgs is a uint8 [n,h,w,3] numpy array, a sequence of [h,w,3] frames or a
    host tensor (uploaded UPLOAD_GROUP frames at a time), or a device tensor.  The file is a Motion-JPEG AVI whatever the
    path says: a path ending in .mp4 (the reference's names) is written as .avi.  Returns the path written."""
    import torch
    if str(path).lower().endswith(".mp4"):
        path = str(path)[:-4] + ".avi"
    with MjpegAviWriter(path, fps, quality, subsampling) as w:
        if isinstance(imgs, torch.Tensor) and imgs.device.type == "cuda":
            w.append(imgs)
        else:
            if not isinstance(imgs, (np.ndarray, torch.Tensor)):
                imgs = np.stack([np.asarray(f) for f in imgs])
            host = imgs if isinstance(imgs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(imgs))
            if host.dtype != torch.uint8 or host.dim() != 4 or host.shape[3] != 3:
                raise ValueError("make_video takes uint8 frames [n,h,w,3]")
            for b in range(0, int(host.shape[0]), UPLOAD_GROUP):
                w.append(host[b:b + UPLOAD_GROUP].to(device))
    return path


def parse_avi(data):
    """(header, frames) of the bytes of an AVI 1.0 file as this module writes them: header is a dict -- riff_bytes, avih and
    strh and strf (dicts of their fields), movi_at (offset of the 'movi' fourcc), movi_bytes, index ([(fourcc, flags,
    offset, size)]) -- and frames the payloads of the 00dc chunks in file order.  Raises ValueError on anything that is not
    framed as RIFF 'AVI ', on a chunk that runs past its parent and on a missing header, movi list or index."""
    data = bytes(data)
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("not an AVI: no RIFF 'AVI ' header")
    riff_bytes, = struct.unpack("<I", data[4:8])
    if 8 + riff_bytes > len(data):
        raise ValueError("truncated AVI: the RIFF chunk runs past the end")
    header = {"riff_bytes": riff_bytes}
    frames = []

    def walk(at, end, inside):
        while at < end:
            if at + 8 > end:
                raise ValueError(f"truncated chunk header at byte {at}")
            kind, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
            body, stop = at + 8, at + 8 + size
            if stop > end:
                raise ValueError(f"chunk {kind!r} at byte {at} runs past its parent")
            if kind == b"LIST":
                if size < 4:
                    raise ValueError(f"LIST at byte {at} has no type")
                name = data[body:body + 4]
                if name == b"movi":
                    header["movi_at"], header["movi_bytes"] = body, size
                walk(body + 4, stop, name)
            elif kind == b"avih":
                f = struct.unpack("<14I", data[body:stop])
                header["avih"] = dict(zip(("usec_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames",
                                           "initial_frames", "streams", "suggested_buffer", "width", "height"), f))
            elif kind == b"strh":
                f = struct.unpack("<4s4sIHHIIIIIIII4H", data[body:stop])
                header["strh"] = dict(zip(("type", "handler", "flags", "priority", "language", "initial_frames", "scale",
                                           "rate", "start", "length", "suggested_buffer", "quality", "sample_size"), f))
            elif kind == b"strf":
                f = struct.unpack("<IiiHH4sIiiII", data[body:stop])
                header["strf"] = dict(zip(("size", "width", "height", "planes", "bit_count", "compression", "size_image"), f))
            elif kind == b"idx1":
                if size % 16:
                    raise ValueError("idx1 is not a whole number of entries")
                header["index"] = [struct.unpack("<4sIII", data[body + k:body + k + 16]) for k in range(0, size, 16)]
            elif kind == b"00dc" and inside == b"movi":
                frames.append(data[body:stop])
            at = stop + (size & 1)

    try:
        walk(12, 8 + riff_bytes, b"AVI ")
    except struct.error as e:
        raise ValueError(f"malformed AVI header chunk: {e}") from None
    for key in ("avih", "strh", "strf", "movi_at", "index"):
        if key not in header:
            raise ValueError(f"not a complete AVI: no {key}")
    return header, frames


def read_frames(path_or_bytes, device="cuda"):
    """The frames of a Motion-JPEG AVI -- a path, or the file's bytes -- as uint8 [n,h,w,3] on the device: parse_avi on the
    host, then jpeg.decode of the frame files (Pillow's pixels of each).  Raises ValueError for a file without frames and
    what parse_avi and jpeg.decode raise."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    _, frames = parse_avi(data)
    if not frames:
        raise ValueError("the AVI holds no frame")
    return jpeg.decode(frames, device)

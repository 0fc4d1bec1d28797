"""Images in, files out: what the device encoders (deblurgs_amd/png.py, jpeg.py) and their callers share -- the tensor check
(as_nhwc), the buffers around the one library call (encode), the way the files reach the host (Download: sizes first, then
sizes[i] bytes of each file, packed end to end; download() for a single call) and write_files.  Files in: pack, the one
pinned buffer jpeg.decode uploads."""
import torch

from . import _lib
from .raster_call import _ptr, _stream


def as_nhwc(images, who, takes, channels):
    """uint8 [n,h,w,c] or [n,h,w] on the device -> contiguous [n,h,w,c].  who and takes (the shapes, in words) are for
    the messages; channels: the channel counts the format has."""
    if images.device.type != "cuda":
        raise RuntimeError(f"{who} needs a tensor on a HIP device (no CPU fallback)")
    if images.dtype != torch.uint8 or images.dim() not in (3, 4):
        raise ValueError(f"{who} takes a uint8 {takes} tensor")
    c = 1 if images.dim() == 3 else int(images.shape[3])
    if c not in channels:
        raise ValueError(f"{who} takes {' / '.join(str(k) for k in channels)} channels, not {c}")
    return (images[..., None] if images.dim() == 3 else images).contiguous()


def files_buffer(files, n, need, device):
    """The [n, >= need] uint8 buffer the files are written into: `files` checked, or a new one (rows rounded up to 16)."""
    if files is None:
        return torch.empty((n, (need + 15) // 16 * 16), dtype=torch.uint8, device=device)
    if (files.dtype != torch.uint8 or files.dim() != 2 or files.shape[0] != n or files.shape[1] < need or
            files.device != device or files.stride(1) != 1):
        raise ValueError(f"files must be a uint8 [n, >= {need}] tensor on the images' device")
    return files


def encode(images, need, tmp_bytes, files, call, what):
    """(files [n,stride] uint8, sizes [n] uint64) on the device.  images: from as_nhwc; need: the format's bound for one
    file; call(images, files, file stride, sizes, tmp, stream): its library call, named `what` in the error message."""
    n = int(images.shape[0])
    files = files_buffer(files, n, need, images.device)
    sizes = torch.empty(n, dtype=torch.uint64, device=images.device)
    tmp = torch.empty(max(tmp_bytes, 16), dtype=torch.uint8, device=images.device)
    _lib.check(call(_ptr(images), _ptr(files), max(int(files.stride(0)), int(files.shape[1])), _ptr(sizes), _ptr(tmp),
                    _stream(images.device)), what)
    return files, sizes


def _pinned(n, dtype):
    return torch.empty(n, dtype=dtype, pin_memory=n > 0)


def pack(chunks, reserve=0):
    """Files on their way to the device (jpeg.decode): chunks [(uint8 numpy array, alignment)] laid end to end in ONE pinned
    host buffer after `reserve` leading bytes of the caller's (an index of the offsets, say), each at a multiple of its
    alignment, the gaps zero, the total rounded up to 16.  Returns (the host uint8 tensor, the offsets): one .to(device)
    uploads everything."""
    offsets, at = [], reserve
    for data, align in chunks:
        at = (at + align - 1) // align * align
        offsets.append(at)
        at += int(data.size)
    host = _pinned((at + 15) // 16 * 16, torch.uint8)
    view = host.numpy()
    view[:] = 0
    for (data, _), off in zip(chunks, offsets):
        view[off:off + int(data.size)] = data
    return host, offsets


class Download:
    """The files of one encode call on their way to the host, in three steps that each end in a recorded event:
    read_sizes enqueues the copy of the sizes; copy_bytes waits for it and enqueues a copy of sizes[i] bytes per file;
    blobs waits for those and returns the files as a list of bytes.  The host buffers are pinned (the copies do not
    block); capacity: the bytes the one for the files starts with -- one that is too small is replaced by one of twice
    the need.

    On one instance the next call's read_sizes may come before this call's blobs (a pipeline enqueues group g before it
    writes g - 2) but not before its copy_bytes, and the next copy_bytes comes after this blobs.  A host buffer is replaced
    only at the start of the step that fills it, so no copy into the old one is outstanding then."""

    def __init__(self, capacity):
        self.host, self.host_sizes = _pinned(capacity, torch.uint8), _pinned(0, torch.int64)
        self.sized, self.copied = torch.cuda.Event(), torch.cuda.Event()

    def read_sizes(self, files, sizes):
        if self.host_sizes.numel() < sizes.numel():
            self.host_sizes = _pinned(sizes.numel(), torch.int64)
        self.files = files
        self.host_sizes[:sizes.numel()].copy_(sizes.view(torch.int64), non_blocking=True)
        self.sized.record(torch.cuda.current_stream(files.device))

    def copy_bytes(self):
        self.sized.synchronize()
        self.sizes = self.host_sizes[:self.files.shape[0]].tolist()
        if self.host.numel() < sum(self.sizes):
            self.host = _pinned(2 * sum(self.sizes), torch.uint8)
        at = 0
        for k, size in enumerate(self.sizes):
            self.host[at:at + size].copy_(self.files[k, :size], non_blocking=True)
            at += size
        self.copied.record(torch.cuda.current_stream(self.files.device))
        self.files = None                   # (the stream keeps the memory until the copies have run)

    def blobs(self):
        self.copied.synchronize()
        host, out, at = self.host.numpy(), [], 0
        for size in self.sizes:
            out.append(host[at:at + size].tobytes())
            at += size
        return out


def download(files, sizes):
    """File i = files[i, :sizes[i]] as bytes, for a single call: the three steps back to back.  (The pinned buffers come
    from torch's caching host allocator: a second call of the same size allocates nothing.)"""
    d = Download(0)
    d.read_sizes(files, sizes)
    d.copy_bytes()
    return d.blobs()


def write_files(images, paths, to_bytes):
    """images [n,...] -> the n files named by paths, their bytes from to_bytes(images).  Returns the paths."""
    paths = list(paths)
    if len(paths) != int(images.shape[0]):
        raise ValueError("one path per image")
    for path, data in zip(paths, to_bytes(images)):
        with open(path, "wb") as f:
            f.write(data)
    return paths

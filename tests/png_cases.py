"""Shared pieces of the PNG tests (tests/test_png_host.py, tests/test_gpu_png.py): the row-filter rule restated in numpy, the
test images, and the checks a finished file has to pass.  The oracle is the format's own decoders: zlib.decompress raises
on a malformed, over-subscribed or incomplete Huffman code and on a wrong Adler-32, PIL checks the rest, zlib.crc32 over
type + payload checks every chunk's CRC (IDAT's included, which PIL skips)."""
import heapq
import io
import struct
import zlib

import numpy as np

MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
FILTER_NAMES = ("None", "Sub", "Up", "Average", "Paeth")


# ------------------------------------------------------------------------------------------------- the filter rule
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(image):
    """image uint8 [h,w,c] (or [h,w]) -> (types uint8 [h], filtered uint8 [h, 1 + w c]): per row the five PNG candidates
    with bpp = c and zeros above row 0, the one with the smallest sum of |residual as int8|, the lowest type on a tie."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[..., None]
    h, w, c = image.shape
    rows = image.reshape(h, w * c).astype(np.int64)
    types = np.zeros(h, np.uint8)
    out = np.zeros((h, 1 + w * c), np.uint8)
    above = np.zeros(w * c, np.int64)
    for r in range(h):
        x = rows[r]
        a = np.concatenate([np.zeros(c, np.int64), x[:-c]]) if w > 1 else np.zeros_like(x)
        b = above
        cc = np.concatenate([np.zeros(c, np.int64), b[:-c]]) if w > 1 else np.zeros_like(x)
        cands = [x, x - a, x - b, x - (a + b) // 2, x - _paeth(a, b, cc)]
        cands = [(v & 255).astype(np.int64) for v in cands]
        sums = [int(np.where(v < 128, v, 256 - v).sum()) for v in cands]
        t = int(np.argmin(sums))                      # the first smallest: the lowest filter type on a tie
        types[r] = t
        out[r, 0] = t
        out[r, 1:] = cands[t]
        above = x
    return types, out


def filter_sums(row, above=None, c=1):
    """The five sums of one row (for the preconditions of the skewed case)."""
    x = np.asarray(row).astype(np.int64)
    b = np.zeros_like(x) if above is None else np.asarray(above).astype(np.int64)
    a = np.concatenate([np.zeros(c, np.int64), x[:-c]])
    cc = np.concatenate([np.zeros(c, np.int64), b[:-c]])
    cands = [x, x - a, x - b, x - (a + b) // 2, x - _paeth(a, b, cc)]
    return [int(np.where((v & 255) < 128, v & 255, 256 - (v & 255)).sum()) for v in cands]


# ------------------------------------------------------------------------------------------------- files
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def assemble(image, compress=zlib.compress):
    """A PNG file by hand from filter_rows and zlib.compress (the host restatement PIL has to undo)."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[..., None]
    h, w, c = image.shape
    _, filtered = filter_rows(image)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, COLOR_TYPE[c], 0, 0, 0)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", compress(filtered.tobytes())) +
            chunk(b"IEND", b""))


def pil_pixels(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im.mode, np.asarray(im)


def check_file(data, image, chunks):
    """Every check a finished file has to pass against the image uint8 [h,w,c] it was made from; `chunks` is
    deblurgs_amd.png.chunks.  Returns (filtered stream uint8 [h, 1 + w c], IDAT payload length)."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[..., None]
    h, w, c = image.shape
    parsed = list(chunks(data))
    assert [k for k, _, _ in parsed] == [b"IHDR", b"IDAT", b"IEND"], [k for k, _, _ in parsed]
    assert all(ok for _, _, ok in parsed), "a chunk CRC is wrong"
    assert parsed[0][1] == struct.pack(">IIBBBBB", w, h, 8, COLOR_TYPE[c], 0, 0, 0)
    assert parsed[2][1] == b""
    idat = parsed[1][1]
    filtered = zlib.decompress(idat)          # raises on a bad code, an incomplete set, a wrong Adler-32
    assert len(filtered) == h * (1 + w * c)
    mode, pixels = pil_pixels(data)
    assert mode == MODES[c]
    assert np.array_equal(pixels.reshape(h, w, c), image)
    return np.frombuffer(filtered, np.uint8).reshape(h, 1 + w * c), len(idat)


def rle_reference_size(filtered):
    """zlib's own Z_RLE stream over the filtered bytes in one piece (the size yardstick)."""
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return len(co.compress(np.asarray(filtered).tobytes()) + co.flush())


# Size: for every test image of four or more segments the IDAT payload is compared with rle_reference_size.  Measured
# ratios: smooth-plus-noise 1000 x 17 RGB 0.9892, uniform random 128 x 128 RGB 1.0002 (stored blocks), and
# gray zeros 300 x 301 1.9636 -- 216 bytes against 110: six segments of one run each, where the per-segment code header (some
# 30 bytes) is all there is.  The cap is the worst measured ratio plus a slack of 0.05; images whose yardstick is at least
# 1 % of the filtered stream (the header is not the whole file) are additionally held to the worst ratio measured among
# them, the three 1080p images of tools/png_timing.py included (1.0027, 1.0054 and 1.0176), plus 0.01.  The encoder is
# integer arithmetic with no order dependence: a ratio is a property of the image, not of the run.
SIZE_CAP = 1.9636 + 0.05
SIZE_CAP_DENSE = 1.0176 + 0.01


def check_size(idat_len, filtered):
    ref = rle_reference_size(filtered)
    ratio = idat_len / ref
    print(f"IDAT {idat_len} bytes, Z_RLE in one piece {ref}, ratio {ratio:.4f}")
    assert ratio <= SIZE_CAP, ratio
    if ref * 100 >= np.asarray(filtered).size:
        assert ratio <= SIZE_CAP_DENSE, ratio
    return ratio


# ------------------------------------------------------------------------------------------------- images
def random_image(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def smooth_noise(h, w, c, seed):
    """Smooth blobs plus about 1.5 LSB of noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, c))
    for ch in range(c):
        img[..., ch] = 128 + 90 * np.sin(xx / (7.0 + ch) + ch) * np.cos(yy / (90.0 + 10 * ch))
    img += rng.normal(0.0, 1.5, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


SKEW_COUNTS = (1, 3, 5, 9, 15, 25, 41, 67, 109, 177, 287, 465, 753, 1219, 1973)


def skewed_row():
    """The code-length-limit case: gray, h = 1, w = 10298.  Even positions hold the values 15 ... 1 with SKEW_COUNTS
    occurrences (each count is the two before it plus one; the rarest value is the largest), shuffled with a fixed seed;
    odd positions hold zeros."""
    values = np.concatenate([np.full(n, 15 - k, np.uint8) for k, n in enumerate(SKEW_COUNTS)])
    np.random.default_rng(20240).shuffle(values)
    row = np.zeros(2 * values.size, np.uint8)
    row[0::2] = values
    return row.reshape(1, -1, 1)


def huffman_depth(counts, prefer_shallow):
    """The depth of an unlimited Huffman tree over `counts`; among equal weights the shallower (or the deeper) subtree is
    merged first: the two tie-breaks."""
    sign = 1 if prefer_shallow else -1
    heap = [(int(n), 0, i, 0) for i, n in enumerate(counts)]
    heapq.heapify(heap)
    serial = len(heap)
    while len(heap) > 1:
        n1, _, _, d1 = heapq.heappop(heap)
        n2, _, _, d2 = heapq.heappop(heap)
        depth = max(d1, d2) + 1
        heapq.heappush(heap, (n1 + n2, sign * depth, serial, depth))
        serial += 1
    return heap[0][3]

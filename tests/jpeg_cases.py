"""Shared pieces of the JPEG and video tests (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py, tests/test_gpu_video.py): the
byte specification of dgs_jpeg_encode (include/dgs_hip.h) restated in numpy integers -- the device must produce these bytes
exactly --, the test images, the constructed cases with their preconditions, and the two caps that hold the restatement
against Pillow's encoder.  The oracle of the format is Pillow's decoder (libjpeg-turbo)."""
import io

import numpy as np

MODES = ("gray", "4:4:4", "4:2:0")
HOST_SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (45, 131), (72, 104), (130, 260)]       # h x w
QUALITIES = (50, 75, 90, 100)
# The restatement against Pillow 12.2 / libjpeg-turbo at the same quality and subsampling, over image_for(h, w, mode,
# seed=1000 h + w) of HOST_SIZES x MODES x QUALITIES (tests/test_jpeg_host.py prints and asserts them), as measured + margin.
# dB the decoded restatement may fall below Pillow's own file.  The worst is the 1 x 1 image (4:4:4 and 4:2:0, quality 50:
# 43.36 dB against 52.90 dB), where one code value in one more channel of the single pixel moves the PSNR by that much: it
# measures the rounding of two colour conversions, not the coder ...
PSNR_DEFICIT_CAP = 9.5424 + 0.1
# ... so images of at least one block are held to their own worst as well (16 x 16, 4:4:4, quality 100: 49.31 dB against
# 50.36 dB; every case below quality 100 is within 0.19 dB)
PSNR_DEFICIT_CAP_BLOCK = 1.044 + 0.1
# bytes over Pillow's with restart_marker_rows=1, optimize=False (worst: 72 x 104, 4:2:0, quality 50; every 4:4:4 ratio is
# within 0.993..1.000).  4:2:0 costs more where the image is no multiple of 16: the specification pads by repeating pixels
# and codes those blocks, libjpeg fills an MCU's blocks beyond the image with the DC of the block before and no AC.
SIZE_RATIO_CAP = 1.0819 + 0.02

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# M[u][x] = rint(8192 c(u) / 2 cos((2x + 1) u pi / 16)), c(0) = sqrt(1/2), c(u) = 1 otherwise
M_TABLE = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                    [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                    [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                    [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                    [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                    [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                    [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                    [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int64)
# Annex K.3 - K.6: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(bytes.fromhex(
    "0001020311040521310612415107617113223281081442"
    "91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    return np.rint(8192.0 * c / 2.0 * np.cos((2 * x + 1) * u * np.pi / 16.0)).astype(np.int64)


def quant_tables(quality):
    """(luma, chroma) int64 [64] in natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(table):
    """symbol -> (code, length) of a (bits, values) table: canonical codes in order of length."""
    codes, code, k = {}, 0, 0
    for length, count in enumerate(table[0], start=1):
        for _ in range(count):
            codes[table[1][k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def _components(image, mode):
    """[(plane int64 [H,W] padded to whole MCUs, table selector)] in scan order, and the MCU size in pixels."""
    image = np.asarray(image)
    gray = mode == "gray"
    if image.ndim == 2:
        image = image[..., None]
    assert image.shape[2] == (1 if gray else 3)
    h, w = image.shape[:2]
    m = 16 if mode == "4:2:0" else 8
    px = image.astype(np.int64)
    if gray:
        comps = [px[..., 0]]
    else:
        R, G, B = px[..., 0], px[..., 1], px[..., 2]
        comps = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
                 np.clip((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16, 0, 255),
                 np.clip((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16, 0, 255)]
    comps = [np.pad(p, ((0, -h % m), (0, -w % m)), mode="edge") for p in comps]
    if mode == "4:2:0":
        comps[1:] = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in comps[1:]]
    return list(zip(comps, (0, 1, 1))), m


def block_levels(block, q):
    """The quantised levels int64 [64] (natural order) of an 8 x 8 block of samples."""
    b = block - 128
    t = (b @ M_TABLE.T + 512) >> 10                   # t[y][u]
    F = (M_TABLE @ t + 4096) >> 13                    # F[v][u]: the coefficient times 8
    F = F.reshape(64)
    return np.sign(F) * ((np.abs(F) + 4 * q) // (8 * q))


def mcu_rows(image, quality, mode):
    """[[(levels in zig-zag order, table selector)]]: the blocks of every MCU row in scan order."""
    comps, m = _components(image, mode)
    qt = quant_tables(quality)
    H, W = comps[0][0].shape
    rows = []
    for my in range(H // m):
        row = []
        for mx in range(W // m):
            for ci, (plane, sel) in enumerate(comps):
                k = m // 8 if ci == 0 else 1          # luma blocks per MCU side
                for by in range(k):
                    for bx in range(k):
                        y, x = (my * k + by) * 8, (mx * k + bx) * 8
                        row.append((block_levels(plane[y:y + 8, x:x + 8], qt[sel])[ZIGZAG], ci))
        rows.append(row)
    return rows


_CODES = None


def row_bits(row):
    """(value, bit count) of one MCU row's entropy-coded bits, DC predictors starting at 0, before padding."""
    global _CODES
    if _CODES is None:
        _CODES = [(huffman_codes(DC_LUMA), huffman_codes(AC_LUMA)), (huffman_codes(DC_CHROMA), huffman_codes(AC_CHROMA))]
    acc, n = 0, 0
    pred = [0, 0, 0]

    def put(v, k):
        nonlocal acc, n
        acc, n = (acc << k) | v, n + k

    def magnitude(v):
        size = int(abs(v)).bit_length()
        return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)

    for zz, ci in row:
        dc, ac = _CODES[0 if ci == 0 else 1]
        size, extra = magnitude(int(zz[0]) - pred[ci])
        pred[ci] = int(zz[0])
        put(*dc[size])
        put(extra, size)
        last = 0
        for k in np.nonzero(zz[1:])[0] + 1:
            run = int(k) - last - 1
            for _ in range(run >> 4):
                put(*ac[0xF0])
            size, extra = magnitude(int(zz[k]))
            put(*ac[((run & 15) << 4) | size])
            put(extra, size)
            last = int(k)
        if last != 63:
            put(*ac[0x00])
    return acc, n


def scan_rows(image, quality, mode):
    """The stuffed bytes of every MCU row (no RST markers)."""
    out = []
    for row in mcu_rows(image, quality, mode):
        acc, n = row_bits(row)
        pad = -n % 8
        acc, n = (acc << pad) | ((1 << pad) - 1), n + pad
        out.append(acc.to_bytes(n // 8, "big").replace(b"\xff", b"\xff\x00"))
    return out


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(w, h, quality, mode):
    gray = mode == "gray"
    qt = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, b"".join(bytes([i]) + bytes(qt[i][ZIGZAG].tolist()) for i in range(1 if gray else 2)))
    comps = [(1, 0x11, 0)] if gray else [(1, 0x22 if mode == "4:2:0" else 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)]
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)]) +
                    b"".join(bytes(c) for c in comps))
    for tc_th, table in [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([] if gray else [(0x01, DC_CHROMA), (0x11, AC_CHROMA)]):
        out += _segment(0xC4, bytes([tc_th]) + bytes(table[0]) + bytes(table[1]))
    m = 16 if mode == "4:2:0" else 8
    out += _segment(0xDD, (-(-w // m)).to_bytes(2, "big"))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], 0x11 * c[2]]) for c in comps) + b"\x00\x3f\x00")
    return out


def encode(image, quality=90, mode="4:2:0"):
    """The file dgs_jpeg_encode must produce for one image uint8 [h,w,3], [h,w,1] or [h,w] (mode "gray" for the last two)."""
    image = np.asarray(image)
    h, w = image.shape[:2]
    rows = scan_rows(image, quality, mode)
    scan = b"".join(r + bytes([0xFF, 0xD0 + (i & 7)]) for i, r in enumerate(rows[:-1])) + rows[-1]
    return header(w, h, quality, mode) + scan + b"\xff\xd9"


def mode_of(channels, subsampling):
    return "gray" if channels == 1 else subsampling


# ------------------------------------------------------------------------------------------------- images
def random_image(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c), dtype=np.uint8)


def smooth_patch(h, w, c, seed):
    """A smooth colour field (two low-frequency waves per channel on a gradient) with a patch of uniform noise in its lower
    right quarter: what a render looks like to a JPEG coder, plus the content that costs it bits."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, c))
    for k in range(c):
        fy, fx, p = rs.uniform(0.02, 0.12, 3)
        out[..., k] = 128 + 60 * np.sin(fy * y + 3 * p) * np.cos(fx * x + k) + 50 * (x / max(w - 1, 1) - 0.5) + 3 * rs.randn(h, w)
    out[h // 2:, w // 2:] = rs.uniform(0, 255, (h - h // 2, w - w // 2, c))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def image_for(h, w, mode, seed):
    img = smooth_patch(h, w, 1 if mode == "gray" else 3, seed)
    return img[..., 0] if mode == "gray" else img


def last_coefficient_block():
    """8 x 8 gray whose only non-zero AC level at quality 50 sits at zig-zag 63: three ZRLs, no EOB."""
    a = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    return np.clip(np.rint(128 + 100 * np.outer(a, a)), 0, 255).astype(np.uint8)


def black_beside_white():
    """8 x 16 gray, a black block then a white one: at quality 100 the second DC difference has category 11."""
    return np.concatenate([np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8)], axis=1)


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def pillow_file(image, quality, mode, **kw):
    from PIL import Image
    f = io.BytesIO()
    sub = {} if mode == "gray" else {"subsampling": mode}
    Image.fromarray(np.asarray(image)).save(f, "JPEG", quality=quality, **sub, **kw)
    return f.getvalue()


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)

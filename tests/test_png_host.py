"""The host side of the device PNG encoder (no GPU needed): exports, the segment constant, the bound formula, argument
refusals with their text, the chunk parser, the numpy restatement of the filter rule (undone by PIL), and the preconditions of
the code-length-limit case tests/test_gpu_png.py runs."""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest

import png_cases as pc
from deblurgs_amd import _lib, png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = _lib.PNG_SEGMENT


def test_exports_and_the_segment_constant():
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    assert int(re.search(r"#define DGS_PNG_SEGMENT (\d+)", text).group(1)) == S
    assert S in (16384, 32768, 65536)
    for name in ("dgs_png_bound", "dgs_png_tmp_bytes", "dgs_png_encode"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("w,h,c", [(1, 1, 1), (3, 5, 2), (64, 64, 4), (S - 1, 1, 1), (S, 1, 1), (1920, 1080, 3), (1000, 17, 3)])
def test_bound_formula(w, h, c):
    F = h * (1 + w * c)
    assert _lib.lib().dgs_png_bound(w, h, c) == 63 + F + 5 * -(-F // S) == png.bound(w, h, c)
    assert _lib.lib().dgs_png_tmp_bytes(1, w, h, c) >= 2 * F


def test_refused_sizes():
    L = _lib.lib()
    for w, h, c in [(4, 4, 0), (4, 4, 5), (0, 4, 3), (4, 0, 3), (-1, 4, 3), (4, -2, 1), (1 << 20, 1 << 11, 1), (46341, 46341, 1)]:
        assert L.dgs_png_bound(w, h, c) == 0, (w, h, c)
        assert L.dgs_png_tmp_bytes(1, w, h, c) == 0, (w, h, c)
    assert L.dgs_png_tmp_bytes(-1, 4, 4, 3) == 0
    with pytest.raises(ValueError):
        png.bound(4, 4, 5)


def test_refused_calls_come_back_as_codes_with_text():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 64)()                     # host memory: every call below is refused before any HIP call
    p = ctypes.addressof(buf)
    ok = dict(images=p, n=1, w=4, h=4, c=3, image_stride=48, files=p, file_stride=L.dgs_png_bound(4, 4, 3), sizes=p, tmp=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.dgs_png_encode(a["images"], a["n"], a["w"], a["h"], a["c"], a["image_stride"], a["files"], a["file_stride"],
                              a["sizes"], a["tmp"], None)
        return rc, L.dgs_last_error().decode()

    for kw, word in [(dict(c=0), "channels"), (dict(c=5), "channels"), (dict(w=0), "w and h"), (dict(h=0), "w and h"),
                     (dict(h=-3), "w and h"), (dict(file_stride=ok["file_stride"] - 1), "file_stride"),
                     (dict(images=None), "null"), (dict(files=None), "null"), (dict(sizes=None), "null"),
                     (dict(tmp=None), "null"), (dict(image_stride=47), "image_stride"), (dict(n=-1), "n must"),
                     (dict(sizes=p + 4), "aligned"), (dict(w=1 << 20, h=1 << 11, c=1), "2^31")]:
        rc, text = call(**kw)
        assert rc != 0 and word in text and text.startswith("png_encode"), (kw, rc, text)
    assert call(n=0, images=None, files=None, sizes=None, tmp=None)[0] == 0        # n = 0 succeeds without a launch


def test_cpu_tensors_are_refused():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        png.encode(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))


def test_chunks_parses_a_pil_file():
    from PIL import Image
    image = pc.smooth_noise(9, 11, 3, seed=1)
    f = io.BytesIO()
    Image.fromarray(image).save(f, format="PNG")
    data = f.getvalue()
    parsed = list(png.chunks(data))
    kinds = [k for k, _, _ in parsed]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and b"IDAT" in kinds and all(ok for _, _, ok in parsed)
    assert parsed[0][1][:8] == (11).to_bytes(4, "big") + (9).to_bytes(4, "big")
    broken = bytearray(data)
    broken[20] ^= 1                                    # inside IHDR's payload
    assert [ok for _, _, ok in png.chunks(bytes(broken))][0] is False
    with pytest.raises(ValueError):
        list(png.chunks(b"not a png file at all"))
    with pytest.raises(ValueError):
        list(png.chunks(data[:-5]))


@pytest.mark.parametrize("h,w,c", [(1, 1, 1), (5, 3, 2), (29, 37, 4), (17, 1000, 3), (7, 1, 3)])
def test_the_numpy_filter_restatement_is_undone_by_pil(h, w, c):
    image = pc.smooth_noise(h, w, c, seed=h + w)
    if h > 4:
        image[2] = pc.random_image(1, w, c, seed=2)[0]
        image[4] = image[3]
    types, filtered = pc.filter_rows(image)
    assert filtered.shape == (h, 1 + w * c) and np.array_equal(filtered[:, 0], types) and types.max() <= 4
    data = pc.assemble(image)
    got, idat_len = pc.check_file(data, image, png.chunks)       # PIL opens it to the same pixels
    assert np.array_equal(got, filtered)
    if h > 4:
        assert types[4] == 2 and not filtered[4, 1:].any()       # a repeated row: Up, all zeros


def test_filter_rule_on_rows_worked_by_hand():
    # row 0 of a constant 255 image: None and Up cost 1 a byte, Sub and Paeth cost the first pixel only: Sub (the lower type)
    image = np.full((2, 4, 3), 255, np.uint8)
    types, filtered = pc.filter_rows(image)
    assert types.tolist() == [1, 2]
    assert filtered[0].tolist() == [1, 255, 255, 255] + [0] * 9 and filtered[1].tolist() == [2] + [0] * 12
    # zeros: every candidate costs 0, the lowest type wins
    assert pc.filter_rows(np.zeros((2, 5, 1), np.uint8))[0].tolist() == [0, 0]


def test_preconditions_of_the_code_length_limit_case():
    image = pc.skewed_row()
    assert image.shape == (1, 10298, 1)
    row = image.reshape(-1)
    counts = np.bincount(row[0::2], minlength=16)
    assert counts[1:].tolist() == list(pc.SKEW_COUNTS)[::-1] and not row[1::2].any()
    assert all(pc.SKEW_COUNTS[k] == pc.SKEW_COUNTS[k - 1] + pc.SKEW_COUNTS[k - 2] + 1 for k in range(2, 15))
    sums = pc.filter_sums(row)
    assert (sums[0], sums[1], sums[3]) == (13340, 26680, 18418) and int(np.argmin(sums)) == 0      # None is chosen
    types, filtered = pc.filter_rows(image)
    assert types.tolist() == [0]
    stream = filtered.reshape(-1)
    assert not (stream[1:] == stream[:-1]).any()                  # no two neighbours are equal: no match
    assert stream.size == 10299 <= 16384 <= S                     # one segment
    hist = np.bincount(stream, minlength=256)
    used = hist[hist > 0].tolist() + [1]                          # the bytes plus end-of-block
    assert pc.huffman_depth(used, True) == 16 and pc.huffman_depth(used, False) == 16


def test_the_size_yardstick_is_zlib_s_rle_strategy():
    filtered = pc.filter_rows(pc.smooth_noise(17, 1000, 3, seed=3))[1]
    ref = pc.rle_reference_size(filtered)
    assert 0 < ref < filtered.size
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    assert zlib.decompress(co.compress(filtered.tobytes()) + co.flush()) == filtered.tobytes()

"""The host side of the device JPEG encoder and the Motion-JPEG AVI writer (no GPU needed): the numpy restatement of the byte
specification (tests/jpeg_cases.py) against Pillow's decoder and encoder, the parsers, the container, exports and refusals.
The device is held to the restatement byte for byte in tests/test_gpu_jpeg.py."""
import ctypes
import io
import os
import re
import struct

import numpy as np
import pytest

import jpeg_cases as jc
from deblurgs_amd import _lib, jpeg, video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_MODE = {"gray": "L", "4:4:4": "RGB", "4:2:0": "RGB"}


@pytest.fixture(scope="module")
def files():
    """(h, w, mode, quality) -> (image, restatement file), over the whole size list: made once."""
    out = {}
    for h, w in jc.HOST_SIZES:
        for mode in jc.MODES:
            image = jc.image_for(h, w, mode, seed=1000 * h + w)
            for q in jc.QUALITIES:
                out[h, w, mode, q] = (image, jc.encode(image, q, mode))
    return out


# ------------------------------------------------------------------------------------------------- 1, 2: the tables
def test_transform_literals_equal_the_formula():
    assert np.array_equal(jc.M_TABLE, jc.dct_matrix())
    text = open(os.path.join(ROOT, "deblurgs_amd", "csrc", "jpeg.hip")).read()
    body = re.search(r"const int M\[64\] = \{(.*?)\};", text, re.S).group(1)
    assert [int(v) for v in re.findall(r"-?\d+", re.sub(r"//.*", "", body))] == jc.M_TABLE.reshape(-1).tolist()


def test_quantisation_tables_equal_pillow_s_for_every_quality():
    from PIL import Image
    image = jc.smooth_patch(8, 8, 3, seed=0)
    for q in range(1, 101):
        tables = Image.open(io.BytesIO(jc.pillow_file(image, q, "4:4:4"))).quantization
        luma, chroma = jc.quant_tables(q)
        assert list(tables[0]) == luma.tolist() and list(tables[1]) == chroma.tolist(), q


def test_huffman_tables_equal_the_ones_pillow_writes():
    data = jc.pillow_file(jc.smooth_patch(16, 16, 3, seed=0), 90, "4:2:0", optimize=False)
    theirs = b"".join(p for m, p in jpeg.segments(data) if m == 0xC4)
    ours = b"".join(bytes([k]) + bytes(t[0]) + bytes(t[1]) for k, t in
                    ((0x00, jc.DC_LUMA), (0x10, jc.AC_LUMA), (0x01, jc.DC_CHROMA), (0x11, jc.AC_CHROMA)))
    assert theirs == ours
    for table, n in ((jc.DC_LUMA, 12), (jc.DC_CHROMA, 12), (jc.AC_LUMA, 162), (jc.AC_CHROMA, 162)):
        codes = jc.huffman_codes(table)
        assert len(codes) == n and sum(2.0 ** -length for _, length in codes.values()) < 1.0      # a prefix code
    assert jc.huffman_codes(jc.AC_LUMA)[0xF0][1] == 11 and jc.huffman_codes(jc.AC_CHROMA)[0xF0][1] == 10


# ------------------------------------------------------------------------------------------------- 3: Pillow opens them
def test_every_restatement_file_opens_in_pillow(files):
    for (h, w, mode, q), (image, data) in files.items():
        im = jc.decode(data)
        assert im.size == (w, h) and im.mode == PIL_MODE[mode] and im.format == "JPEG", (h, w, mode, q)
        kinds = [m for m, _ in jpeg.segments(data)]
        n_dht = 2 if mode == "gray" else 4
        assert kinds == [0xD8, 0xE0, 0xDB, 0xC0] + [0xC4] * n_dht + [0xDD, 0xDA, jpeg.SCAN, 0xD9], (h, w, mode, q)


# ------------------------------------------------------------------------------------------------- 4, 5: the two caps
def test_quality_against_pillow_s_encoder(files):
    worst, worst_block = (-99.0,), (-99.0,)
    for (h, w, mode, q), (image, data) in files.items():
        ours = jc.psnr(np.asarray(jc.decode(data)), image)
        theirs = jc.psnr(np.asarray(jc.decode(jc.pillow_file(image, q, mode))), image)
        worst = max(worst, (theirs - ours, h, w, mode, q))
        if h >= 8 and w >= 8:
            worst_block = max(worst_block, (theirs - ours, h, w, mode, q))
    print("largest PSNR deficit against Pillow:", worst, "; among images of at least one block:", worst_block)
    assert worst[0] <= jc.PSNR_DEFICIT_CAP, worst
    assert worst_block[0] <= jc.PSNR_DEFICIT_CAP_BLOCK, worst_block


def test_size_against_pillow_s_encoder(files):
    worst, span444 = (0.0,), [9.0, 0.0]
    for (h, w, mode, q), (image, data) in files.items():
        ratio = len(data) / len(jc.pillow_file(image, q, mode, restart_marker_rows=1, optimize=False))
        worst = max(worst, (ratio, h, w, mode, q))
        if mode == "4:4:4":
            span444 = [min(span444[0], ratio), max(span444[1], ratio)]
    print("largest size ratio against Pillow:", worst, "; 4:4:4 ratios span", span444)
    assert worst[0] <= jc.SIZE_RATIO_CAP, worst


# ------------------------------------------------------------------------------------------------- 6: exact cases
@pytest.mark.parametrize("mode", jc.MODES)
@pytest.mark.parametrize("value", [0, 255])
def test_black_and_white_decode_to_themselves_at_quality_100(mode, value):
    image = np.full((16, 24) if mode == "gray" else (16, 24, 3), value, np.uint8)
    assert np.array_equal(np.asarray(jc.decode(jc.encode(image, 100, mode))), image)


def test_a_one_pixel_checkerboard_decodes_exactly_at_444_quality_100():
    board = ((np.add.outer(np.arange(16), np.arange(24)) & 1) * 255).astype(np.uint8)
    rgb = np.repeat(board[..., None], 3, axis=2)
    assert np.array_equal(np.asarray(jc.decode(jc.encode(rgb, 100, "4:4:4"))), rgb)
    assert np.array_equal(np.asarray(jc.decode(jc.encode(board, 100, "gray"))), board)


def test_preconditions_of_the_constructed_cases():
    zz, = [b for b, _ in jc.mcu_rows(jc.last_coefficient_block(), 50, "gray")[0]]
    assert not zz[1:63].any() and zz[63] != 0                            # three ZRLs, no EOB
    dcs = [int(b[0]) for b, _ in jc.mcu_rows(jc.black_beside_white(), 100, "gray")[0]]
    assert dcs == [-1024, 1016] and (dcs[1] - dcs[0]).bit_length() == 11  # DC difference category 11
    noise = jc.random_image(64, 64, 3, seed=1)
    for mode in jc.MODES:
        image = noise[..., 0] if mode == "gray" else noise
        assert any(b"\xff\x00" in row for row in jc.scan_rows(image, 100, mode)), mode
        assert any(b[1:].all() for row in jc.mcu_rows(image, 100, mode) for b, _ in row), mode
        assert max(int(np.abs(b[1:]).max()) for row in jc.mcu_rows(image, 100, mode) for b, _ in row) < 1024
    rows = jc.mcu_rows(np.full((24, 8), 200, np.uint8), 50, "gray")
    assert len(rows) == 3 and len({jc.row_bits(r) for r in rows}) == 1     # every row codes its DC against 0


# ------------------------------------------------------------------------------------------------- 7: the parsers
def test_segments_on_good_truncated_and_corrupted_streams(files):
    image, data = files[17, 33, "4:2:0", 90]
    parsed = list(jpeg.segments(data))
    assert parsed[0] == (0xD8, b"") and parsed[-1] == (0xD9, b"")
    sof, = [p for m, p in parsed if m == 0xC0]
    assert struct.unpack(">BHHB", sof[:6]) == (8, 17, 33, 3) and sof[6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    dri, = [p for m, p in parsed if m == 0xDD]
    assert dri == (3).to_bytes(2, "big")                                # 33 pixels: three MCUs of 16
    scan, = [p for m, p in parsed if m == jpeg.SCAN]
    assert scan.count(b"\xff\xd0") == 1 and b"".join(jc.scan_rows(image, 90, "4:2:0")) == scan.replace(b"\xff\xd0", b"")
    assert video.jpeg_size(data) == (33, 17)
    assert [m for m, _ in jpeg.segments(jc.pillow_file(image, 90, "4:2:0"))][-1] == 0xD9      # someone else's file
    for bad in (b"", b"\x89PNG\r\n\x1a\n", data[:1], data[:-2], data[:300], data[:len(data) - 1], data[:2] + b"\x00" + data[3:]):
        with pytest.raises(ValueError):
            list(jpeg.segments(bad))
    broken = bytearray(data)
    broken[4:6] = (60000).to_bytes(2, "big")                            # APP0 claims more bytes than the file has
    with pytest.raises(ValueError):
        list(jpeg.segments(bytes(broken)))


def _avi(tmp_path, frames, fps=32, name="a.avi"):
    path = str(tmp_path / name)
    with video.MjpegAviWriter(path, fps) as w:
        w.append(frames[0])                                             # one frame as bytes
        w.append(frames[1:])                                            # the rest as a list
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def frames():
    """Five 4:2:0 frames of 17 x 33 with sizes of both parities."""
    out = [jc.encode(jc.smooth_patch(17, 33, 3, seed=s), 90, "4:2:0") for s in range(5)]
    if len({len(f) & 1 for f in out}) == 1:
        out[0] = jc.encode(jc.smooth_patch(17, 33, 3, seed=0), 89, "4:2:0")
    assert len({len(f) & 1 for f in out}) == 2
    return out


def test_parse_avi_on_good_truncated_and_corrupted_files(tmp_path, frames):
    data = _avi(tmp_path, frames)
    header, got = video.parse_avi(data)
    assert got == frames
    for bad in (b"", data[:11], b"RIFX" + data[4:], data[:8] + b"WAVE" + data[12:], data[:100], data[:-1], data[:len(data) // 2]):
        with pytest.raises(ValueError):
            video.parse_avi(bad)
    broken = bytearray(data)
    broken[video.HEADER_BYTES + 4:video.HEADER_BYTES + 8] = struct.pack("<I", len(data))      # a frame larger than movi
    with pytest.raises(ValueError):
        video.parse_avi(bytes(broken))
    broken = bytearray(data)
    broken[12:16] = b"JUNK"                                             # the header list is gone
    with pytest.raises(ValueError):
        video.parse_avi(bytes(broken))


# ------------------------------------------------------------------------------------------------- 8: the container
@pytest.mark.parametrize("fps,rate,scale", [(10, 10, 1), (32, 32, 1), (29.97, 2997, 100)])
def test_avi_layout_adds_up(tmp_path, frames, fps, rate, scale):
    data = _avi(tmp_path, frames, fps)
    header, got = video.parse_avi(data)
    assert got == frames
    n, largest = len(frames), max(len(f) for f in frames)
    assert header["riff_bytes"] == len(data) - 8
    avih, strh, strf = header["avih"], header["strh"], header["strf"]
    assert (avih["total_frames"], avih["streams"], avih["width"], avih["height"]) == (n, 1, 33, 17)
    assert avih["flags"] & 0x10 and avih["suggested_buffer"] == largest
    assert avih["usec_per_frame"] == round(1e6 * scale / rate)
    assert (strh["type"], strh["handler"], strh["rate"], strh["scale"], strh["length"]) == (b"vids", b"MJPG", rate, scale, n)
    assert strh["suggested_buffer"] == largest
    assert (strf["size"], strf["width"], strf["height"], strf["planes"], strf["bit_count"], strf["compression"],
            strf["size_image"]) == (40, 33, 17, 1, 24, b"MJPG", 3 * 33 * 17)
    # the lists: hdrl is avih + the strl list, movi the padded chunks, and idx1 closes the file
    assert data[12:16] == b"LIST" and data[20:24] == b"hdrl" and struct.unpack("<I", data[16:20])[0] == 4 + 64 + 8 + 4 + 64 + 48
    assert data[88:92] == b"LIST" and data[96:100] == b"strl" and struct.unpack("<I", data[92:96])[0] == 4 + 64 + 48
    movi = header["movi_at"]
    assert movi == video.MOVI_AT and data[movi - 8:movi - 4] == b"LIST" and data[movi:movi + 4] == b"movi"
    assert header["movi_bytes"] == 4 + sum(8 + len(f) + (len(f) & 1) for f in frames)
    idx_at = movi + header["movi_bytes"]
    assert data[idx_at:idx_at + 4] == b"idx1" and struct.unpack("<I", data[idx_at + 4:idx_at + 8])[0] == 16 * n
    assert idx_at + 8 + 16 * n == len(data)
    assert len(header["index"]) == n and any(len(f) & 1 for f in frames)
    for (fourcc, flags, offset, size), f in zip(header["index"], frames):
        at = movi + offset
        assert (fourcc, flags, size) == (b"00dc", 0x10, len(f)) and at % 2 == 0
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == size
        assert data[at + 8:at + 8 + size] == f
        if size & 1:
            assert data[at + 8 + size] == 0                             # the pad byte
    assert video.frame_rate(30000 / 1001) == (30000, 1001)


def test_every_frame_in_the_avi_decodes_to_what_the_lone_file_decodes_to(tmp_path, frames):
    _, got = video.parse_avi(_avi(tmp_path, frames))
    for inside, alone in zip(got, frames):
        assert np.array_equal(np.asarray(jc.decode(inside)), np.asarray(jc.decode(alone)))


def test_writer_refusals(tmp_path, frames, monkeypatch):
    path = str(tmp_path / "small.avi")
    monkeypatch.setattr(video, "MAX_FILE_BYTES", video.HEADER_BYTES + 2 * (8 + len(frames[0]) + 1) + 8 + 16 * 3)
    w = video.MjpegAviWriter(path, 32)
    w.append(frames[0])
    w.append(frames[0])
    with pytest.raises(ValueError, match="2 GiB"):
        w.append(frames[0])                                             # refused BEFORE it is written
    assert w.n_frames == 2
    w.close()
    w.close()                                                           # closing twice is harmless
    header, got = video.parse_avi(open(path, "rb").read())
    assert got == [frames[0]] * 2 and header["avih"]["total_frames"] == 2
    with pytest.raises(ValueError, match="closed"):
        w.append(frames[0])
    monkeypatch.undo()
    with video.MjpegAviWriter(str(tmp_path / "sizes.avi"), 32) as w:
        w.append(frames[0])
        with pytest.raises(ValueError, match="one size"):
            w.append(jc.encode(jc.smooth_patch(8, 8, 3, seed=0), 90, "4:4:4"))
        with pytest.raises(ValueError):
            w.append(b"not a jpeg")
        with pytest.raises(TypeError):
            w.append(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        video.frame_rate(0)


# ------------------------------------------------------------------------------------------------- 9: ABI
def test_exports_and_the_header_constants():
    text = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    assert int(re.search(r"#define DGS_JPEG_444 (\d+)", text).group(1)) == jpeg.SUBSAMPLING["4:4:4"] == 0
    assert int(re.search(r"#define DGS_JPEG_420 (\d+)", text).group(1)) == jpeg.SUBSAMPLING["4:2:0"] == 1
    assert int(re.search(r"#define DGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 15
    for name in ("dgs_jpeg_bound", "dgs_jpeg_tmp_bytes", "dgs_jpeg_encode"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name) and name + "(" in text


@pytest.mark.parametrize("w,h,c,sub", [(1, 1, 1, 0), (1, 1, 3, 0), (1, 1, 3, 1), (33, 17, 3, 1), (33, 17, 3, 0), (33, 17, 1, 1),
                                       (1920, 1080, 3, 1), (1920, 1080, 3, 0), (65535, 65535, 3, 0)])
def test_bound_formula(w, h, c, sub):
    m = 16 if (c == 3 and sub == 1) else 8
    mx, my = -(-w // m), -(-h // m)
    blocks = mx * my * (1 if c == 1 else (6 if m == 16 else 3))
    want = (334 if c == 1 else 625) + 416 * blocks + 2 * my + 2
    assert _lib.lib().dgs_jpeg_bound(w, h, c, sub) == want == jpeg.bound(w, h, c, "4:2:0" if sub else "4:4:4")
    assert _lib.lib().dgs_jpeg_tmp_bytes(2, w, h, c, sub) >= 2 * 416 * blocks
    mode = "gray" if c == 1 else ("4:2:0" if sub else "4:4:4")
    assert len(jc.header(w, h, 90, mode)) == (334 if c == 1 else 625)


def test_refused_sizes():
    L = _lib.lib()
    for w, h, c, sub in [(4, 4, 0, 0), (4, 4, 2, 0), (4, 4, 4, 0), (0, 4, 3, 0), (4, 0, 3, 0), (-1, 4, 3, 0), (65536, 4, 3, 0),
                         (4, 65536, 1, 0), (4, 4, 3, 2), (4, 4, 3, -1)]:
        assert L.dgs_jpeg_bound(w, h, c, sub) == 0, (w, h, c, sub)
        assert L.dgs_jpeg_tmp_bytes(1, w, h, c, sub) == 0, (w, h, c, sub)
    assert L.dgs_jpeg_tmp_bytes(-1, 4, 4, 3, 0) == 0
    with pytest.raises(ValueError):
        jpeg.bound(4, 4, 2)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg.bound(4, 4, 3, "4:2:2")


def test_refused_calls_come_back_as_codes_with_text():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 64)()                     # host memory: every call below is refused before any HIP call
    p = ctypes.addressof(buf)
    ok = dict(images=p, n=1, w=4, h=4, c=3, image_stride=48, quality=90, sub=1, files=p,
              file_stride=L.dgs_jpeg_bound(4, 4, 3, 1), sizes=p, tmp=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.dgs_jpeg_encode(a["images"], a["n"], a["w"], a["h"], a["c"], a["image_stride"], a["quality"], a["sub"],
                               a["files"], a["file_stride"], a["sizes"], a["tmp"], None)
        return rc, L.dgs_last_error().decode()

    for kw, word in [(dict(c=0), "channels"), (dict(c=2), "channels"), (dict(c=4), "channels"), (dict(w=0), "w and h"),
                     (dict(h=0), "w and h"), (dict(h=-3), "w and h"), (dict(w=65536), "w and h"), (dict(sub=2), "subsampling"),
                     (dict(quality=0), "quality"), (dict(quality=101), "quality"),
                     (dict(file_stride=ok["file_stride"] - 1), "file_stride"), (dict(images=None), "null"),
                     (dict(files=None), "null"), (dict(sizes=None), "null"), (dict(tmp=None), "null"),
                     (dict(image_stride=47), "image_stride"), (dict(n=-1), "n must"), (dict(sizes=p + 4), "aligned")]:
        rc, text = call(**kw)
        assert rc != 0 and word in text and text.startswith("jpeg_encode"), (kw, rc, text)
    assert call(n=0, images=None, files=None, sizes=None, tmp=None)[0] == 0        # n = 0 succeeds without a launch


def test_cpu_tensors_are_refused():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.encode(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video.write_video(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), os.devnull, 32)

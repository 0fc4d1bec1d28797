"""The host side of the device JPEG decoder (no GPU needed): the numpy restatement of the pixel specification
(tests/jpeg_decode_cases.py) against Pillow's stored and live pixels; the library's parser (dgs_jpeg_decode_plan) against the
restatement's; every refusal and every class of corrupt header; and the parser plus the interval decoder -- the text the
entropy kernel is compiled from -- as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer over the
fixtures, their truncations and mutations.  The device is held to the restatement in tests/test_gpu_jpeg_decode.py."""
import ctypes
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_cases as dc
from deblurgs_amd import _lib, jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- 1. the restatement
def test_the_table_holds_every_kind_of_case():
    dc.check_table()
    assert os.path.getsize(dc.GOLDEN) < 200 * 1024


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_restatement_equals_pillows_stored_pixels(name):
    data, pixels = dc.golden()[name]
    dc.check_needs(name, data)
    assert np.array_equal(dc.decode(data), pixels)


def test_restatement_equals_live_pillow():
    pytest.importorskip("PIL")
    from PIL import Image
    for name in sorted(dc.CASES):
        data, _ = dc.golden()[name]
        assert np.array_equal(dc.decode(data), np.asarray(Image.open(io.BytesIO(data)))), name      # today's decoder
        fresh, pixels = dc.pillow_file(name)                                                        # today's encoder too
        assert np.array_equal(dc.decode(fresh), pixels), name


# ------------------------------------------------------------------------------------------------- 2. the parser
def _plan(data):
    raw = jpeg.plan(data)
    head = _lib.DgsJpegPlan.from_buffer_copy(raw[:ctypes.sizeof(_lib.DgsJpegPlan)].tobytes())
    table = raw[ctypes.sizeof(_lib.DgsJpegPlan):].view(np.uint32)[:head.n_intervals + 1]
    return head, table.tolist(), raw


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_plan_equals_the_restatements_parse(name):
    data, _ = dc.golden()[name]
    p = dc.parse(data)
    head, table, raw = _plan(data)
    assert head.magic == 0x4E4C504A and head.plan_bytes == raw.size and head.file_bytes == len(data)
    assert (head.w, head.h, head.channels, head.hs, head.vs) == (p.w, p.h, p.channels, p.hs, p.vs)
    assert (head.mcus_x, head.mcus_y, head.restart_interval, head.n_intervals) == (p.mcus_x, p.mcus_y, p.dri, p.n_intervals)
    assert (head.scan_begin, head.scan_end) == (p.scan_begin, p.scan_end) and table == p.interval_at
    for c in range(p.channels):
        assert list(head.quant[c]) == p.quant[c].tolist()
        for table_c, (counts, vals), codes in ((head.huff[c], p.dc_counts[c], p.dc[c]), (head.huff[3 + c], p.ac_counts[c], p.ac[c])):
            assert list(table_c.vals)[:len(vals)] == vals
            for bits, symbol in codes.items():         # every code: through the lookahead, or maxcode / valoff
                if len(bits) <= 8:
                    for fill in range(1 << (8 - len(bits))):
                        assert table_c.look[(int(bits, 2) << (8 - len(bits))) | fill] == (len(bits) << 8) | symbol
                else:
                    assert table_c.look[int(bits[:8], 2)] == 0
                    code = int(bits, 2)
                    assert code <= table_c.maxcode[len(bits)] and table_c.vals[code + table_c.valoff[len(bits)]] == symbol
                    assert all(int(bits[:k], 2) > table_c.maxcode[k] for k in range(9, len(bits)))
    info = jpeg.probe(data)
    assert info == {"width": p.w, "height": p.h, "channels": p.channels, "subsampling": dc.CASES[name]["mode"],
                    "restart_interval": p.dri, "intervals": p.n_intervals}


def test_size_query_and_capacity():
    L = _lib.lib()
    data, _ = dc.golden()["intervals_of_3_4:4:4"]
    need = ctypes.c_size_t()
    assert L.dgs_jpeg_decode_plan_bytes(data, len(data), ctypes.byref(need)) == 0
    head, table, raw = _plan(data)
    assert need.value == raw.size == (ctypes.sizeof(_lib.DgsJpegPlan) + 4 * (head.n_intervals + 1) + 7) // 8 * 8
    small = np.zeros(need.value // 8 - 1, np.uint64)
    assert L.dgs_jpeg_decode_plan(data, len(data), small.ctypes.data, small.nbytes) == -2        # DGS_E_CAPACITY
    assert L.dgs_jpeg_decode_plan(data, len(data), None, 0) == -1 and L.dgs_jpeg_decode_plan_bytes(None, 0, None) == -1
    assert L.dgs_jpeg_decode_plan(data, len(data), small.ctypes.data + 4, small.nbytes - 4) == -1
    assert b"aligned" in L.dgs_last_error()


def _segments(data):
    """[(marker, offset of its 0xFF, payload offset, payload length)] up to SOS."""
    out, at = [], 2
    while True:
        length = int.from_bytes(data[at + 2:at + 4], "big")
        out.append((data[at + 1], at, at + 4, length - 2))
        if data[at + 1] == 0xDA:
            return out
        at += 2 + length


def _find(data, marker):
    return next(s for s in _segments(data) if s[0] == marker)


def _edit(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def _pillow(mode, size=(16, 16), **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(dc.content("smooth", size[1], size[0], 3, 5)).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_every_refusal_has_its_reason():
    rgb, _ = dc.golden()["smooth_17x33_4:4:4"]
    sof, sos, dqt = _find(rgb, 0xC0), _find(rgb, 0xDA), _find(rgb, 0xDB)
    p = dc.parse(rgb)
    cmyk = _pillow("CMYK")
    app14 = _find(cmyk, 0xEE)
    assert cmyk[app14[2]:app14[2] + 5] == b"Adobe"
    four = cmyk[:app14[1]] + cmyk[app14[1] + 4 + app14[3]:]                      # CMYK without its Adobe segment
    adobe_rgb = rgb[:sof[1]] + cmyk[app14[1]:app14[1] + 4 + app14[3]] + rgb[sof[1]:]
    assert adobe_rgb[sof[1] + 4 + 11] == 0                                      # transform 0
    two_scans = rgb[:p.scan_end] + rgb[sos[1]:]                                 # the scan a second time before EOI
    refusals = {
        "progressive": (_pillow("RGB", progressive=True), "progressive"),
        "SOF1": (_edit(rgb, sof[1] + 1, [0xC1]), "SOF1"),
        "lossless": (_edit(rgb, sof[1] + 1, [0xC3]), "above SOF2"),
        "arithmetic": (_edit(rgb, sof[1] + 1, [0xC9]), "above SOF2"),
        "12 bits": (_edit(rgb, sof[2], [12]), "precision"),
        "several scans": (two_scans, "several scans"),
        "16-bit DQT": (_edit(rgb, dqt[2], [0x10 | rgb[dqt[2]]]), "16-bit quantisation"),
        "CMYK": (cmyk, "Adobe APP14"),
        "4 components": (four, "4 components"),
        "4:1:1": (_edit(rgb, sof[2] + 7, [0x41]), "sampling factors"),
        "4:4:0": (_edit(rgb, sof[2] + 7, [0x12]), "sampling factors"),
        "subsampled chroma": (_edit(rgb, sof[2] + 10, [0x21]), "sampling factors"),
        "Adobe transform 0": (adobe_rgb, "transform 0"),
        "ids RGB": (_edit(_edit(rgb, sof[2] + 6, b"R\x11\x00G\x11\x01B"), sos[2] + 1, b"R\x00G\x11B"), "R, G, B"),
    }
    for what, (data, reason) in refusals.items():
        with pytest.raises(jpeg.Unsupported, match=reason):
            jpeg.probe(data)
        assert issubclass(jpeg.Unsupported, ValueError), what
    assert jpeg.probe(_pillow("L"))["subsampling"] == "gray"


def test_every_class_of_corrupt_header():
    rgb, _ = dc.golden()["smooth_17x33_4:4:4"]
    dri, _ = dc.golden()["intervals_of_3_4:4:4"]
    sof, sos, dqt, dht = _find(rgb, 0xC0), _find(rgb, 0xDA), _find(rgb, 0xDB), _find(rgb, 0xC4)
    p, pd = dc.parse(rgb), dc.parse(dri)
    first_rst = pd.interval_at[1] - 2
    ddri = _find(dri, 0xDD)
    corrupt = {
        "no SOI": (b"\x00" + rgb[1:], "no SOI"),
        "segment length past the end": (_edit(rgb, dqt[1] + 2, [0xFF, 0xFF]), "length runs past the end"),
        "segment length below 2": (_edit(rgb, dqt[1] + 2, [0, 1]), "length runs past the end"),
        "DHT counts past 256": (_edit(rgb, dht[2] + 1, [200, 100]), "sum past 256"),
        "DHT counts that overflow a length": (_edit(rgb, dht[2] + 1, [3]), "(prefix code|past its segment)"),
        "DHT table id": (_edit(rgb, dht[2], [0x07]), "DHT class above 1 or table id above 3"),
        "DHT class": (_edit(rgb, dht[2], [0x20]), "DHT class above 1 or table id above 3"),
        "DQT table id": (_edit(rgb, dqt[2], [0x05]), "DQT table id above 3"),
        "component quantisation id": (_edit(rgb, sof[2] + 8, [4]), "quantisation table id above 3"),
        "undefined quantisation table": (_edit(rgb, sof[2] + 8, [3]), "quantisation table that is not defined"),
        "scan Huffman id": (_edit(rgb, sos[2] + 2, [0x40]), "Huffman table id above 3"),
        "undefined Huffman table": (_edit(rgb, sos[2] + 2, [0x30]), "Huffman table that is not defined"),
        "unknown scan component": (_edit(rgb, sos[2] + 1, [9]), "names a component"),
        "zero width": (_edit(rgb, sof[2] + 3, [0, 0]), "zero dimension"),
        "zero height": (_edit(rgb, sof[2] + 1, [0, 0]), "zero dimension"),
        "sampling factor 0": (_edit(rgb, sof[2] + 7, [0x01]), "sampling factor outside"),
        "SOF length": (_edit(rgb, sof[1] + 2, [0, 14]), "(SOF0 length|marker)"),
        "no EOI": (rgb[:-2], "no EOI"),
        "truncated scan": (rgb[:p.scan_begin + 5], "(no EOI|too short)"),
        "picture larger than the file": (_edit(rgb, sof[2] + 1, [0xFF, 0xFF, 0xFF, 0xFF]), "too short for the picture"),
        "a restart marker removed": (dri[:first_rst] + dri[first_rst + 2:], "(fewer restart intervals|out of order)"),
        "a restart marker added": (dri[:pd.scan_end] + b"\xff" + bytes([0xD0 + (pd.n_intervals - 1) % 8]) + dri[pd.scan_end:],
                                   "more restart intervals"),
        "restart markers out of order": (_edit(dri, first_rst + 1, [0xD3]), "out of order"),
        "DRI that disagrees": (_edit(dri, ddri[2], [0, 2]), "(restart intervals|out of order)"),
        "restart marker without DRI": (rgb[:p.scan_begin + 9] + b"\xff\xd0" + rgb[p.scan_begin + 9:], "more restart intervals"),
        "spectral selection": (_edit(rgb, sos[2] + 7, [0, 5, 0]), "spectral selection"),
    }
    for what, (data, reason) in corrupt.items():
        with pytest.raises(ValueError, match=reason) as e:
            jpeg.probe(data)
        assert not isinstance(e.value, jpeg.Unsupported) and "corrupt JPEG" in str(e.value), what
    # APPn and COM are skipped, fill bytes before a marker too
    extra = rgb[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe5\x00\x04xy" + b"\xff\xff" + rgb[2:]
    assert jpeg.probe(extra) == jpeg.probe(rgb)


# ------------------------------------------------------------------------------------------------- 3. exports
def test_abi_15_and_prototypes_in_step():
    header = open(os.path.join(ROOT, "include", "dgs_hip.h")).read()
    assert "#define DGS_ABI_VERSION 15" in header and _lib.ABI_VERSION == 15 and _lib.lib().dgs_abi_version() == 15
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("dgs_jpeg_decode_plan_bytes", 3), ("dgs_jpeg_decode_plan", 4), ("dgs_jpeg_decode_tmp_bytes", 4),
                         ("dgs_jpeg_decode", 13)):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(args.split(",")) == n_args == len(_lib.EXPORTS[name][1]), name
    for define, value in (("DGS_E_JPEG_UNSUPPORTED", _lib.E_JPEG_UNSUPPORTED), ("DGS_E_JPEG_CORRUPT", _lib.E_JPEG_CORRUPT)):
        assert int(re.search(r"#define %s \((-?\d+)\)" % define, header).group(1)) == value
    assert sorted(_lib.JPEG_STATUS) == sorted(int(v) for k, v in re.findall(r"#define (DGS_JPEG_S_[A-Z_]+) (\d+)", header)
                                              if k != "DGS_JPEG_S_OK")
    assert ctypes.sizeof(_lib.DgsJpegHuff) == 912 and ctypes.sizeof(_lib.DgsJpegPlan) == 5728       # jpeg_decode.hip asserts both
    from deblurgs_amd import build
    assert build.SOURCES["jpeg_decode.hip"] == ["-fwrapv"]
    L = _lib.lib()
    assert L.dgs_jpeg_decode_tmp_bytes(2, 17, 33, 3) == 32 + 2 * 3 * 4 * 6 * 192
    assert L.dgs_jpeg_decode_tmp_bytes(1, 0, 8, 3) == 0 and L.dgs_jpeg_decode_tmp_bytes(1, 8, 8, 2) == 0
    assert L.dgs_jpeg_decode_tmp_bytes(1 << 30, 65535, 65535, 3) == 0
    # refused before anything is enqueued: no GPU needed
    dummy = np.zeros(64, np.uint64)
    a = dummy.ctypes.data
    assert L.dgs_jpeg_decode(a, 64, a, 0, 8, 8, 3, 1, a, 192, a, a, None) == 0
    for args, text in (((a, 64, a, 1, 8, 8, 2, 1, a, 192, a, a, None), b"channels"),
                       ((a, 64, a, 1, 8, 0, 3, 1, a, 192, a, a, None), b"1..65535"),
                       ((a, 64, a, -1, 8, 8, 3, 1, a, 192, a, a, None), b"negative"),
                       ((None, 64, a, 1, 8, 8, 3, 1, a, 192, a, a, None), b"null"),
                       ((a + 4, 64, a, 1, 8, 8, 3, 1, a, 192, a, a, None), b"16-byte"),
                       ((a, 64, a, 1, 8, 8, 3, 1, a + 2, 192, a, a, None), b"multiple of 4"),
                       ((a, 64, a, 1, 8, 8, 3, 1, a, 190, a, a, None), b"multiple of 4"),
                       ((a, 64, a, 1, 8, 8, 3, 1, a, 188, a, a, None), b"below h w channels"),
                       ((a, 64, a, 1, 8, 8, 3, 0, a, 192, a, a, None), b"max_intervals")):
        assert L.dgs_jpeg_decode(*args) == -1 and text in L.dgs_last_error(), text


def test_python_front_end_refusals_need_no_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.decode([dc.golden()["smooth_8x8_gray"][0]], device="cpu")


# ------------------------------------------------------------------------------------------------- 4. under the sanitizers
def test_parser_and_interval_decoder_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/jpeg_decode_host_main.cpp, its own main) around csrc/jpeg_decode_core.h, built with the
    host compiler and -fsanitize=address,undefined and run as a plain process: every fixture must give the restatement's
    coefficients, the three malformed scans their status, and every truncation of three fixtures and 300 fixed-seed
    single-byte mutations of every file must be refused or decoded without a report."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "jpeg_decode_host"
    # (the sanitizer runtimes linked statically: the program needs nothing preloaded and minds nothing that is)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "jpeg_decode_host_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    first = ["noise_q100_4:4:4", "intervals_of_1_4:2:0", "noise_optimized_gray"]        # the three that are truncated
    names = first + [n for n in sorted(dc.CASES) if n not in first]
    blob = struct.pack("<I", len(names) + 3)
    for name in names:
        data = dc.golden()[name][0]
        coef = dc.coefficients(data).reshape(-1)
        blob += struct.pack("<III", 0, len(data), coef.size) + data + coef.astype("<i2").tobytes()
    for name, (data, status) in dc.malformed_scans().items():
        blob += struct.pack("<III", 1, len(data), status) + data
    blob += struct.pack("<III", 3, 300, 0x9E3779B9)
    cases = tmp_path / "cases.bin"
    cases.write_bytes(blob)
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith(f"fixtures {len(names)} decoded 3 stopped")

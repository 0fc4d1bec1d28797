"""The JPEG decoder's pixel specification (include/dgs_hip.h, "JPEG files decoded on the device") restated in numpy, and the
ONE table of cases its tests share.

    parse(data)        the headers and the walk over the scan: size, sampling, tables, DRI, the byte range of every interval
    coefficients(data) the entropy decoding: int16 [blocks, 64] in natural order, laid out as the library lays them out
                       (component after component, each a row-major grid of blocks), and what the scan exercised (STATS)
    decode(data)       the pixels: uint8 [h,w,3] or [h,w], equal to np.asarray(PIL.Image.open(...)) bit for bit
    CASES              name -> how Pillow makes the file (tests/golden/make_golden_jpeg_decode.py) and the preconditions
                       ("needs") the file must meet, asserted by check_needs: a case that stops exercising what it is
                       there for fails instead of passing quietly
    malformed_scans()  three files the parser accepts and the entropy decoder must refuse

tests/test_jpeg_decode_host.py holds the restatement against Pillow's stored and live pixels and the host parser and
interval decoder against the restatement; tests/test_gpu_jpeg_decode.py holds the device against the restatement.  Equality
is exact everywhere.
"""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode_golden.npz")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), "gray": (1, 1)}
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


class Parsed:
    pass


# ------------------------------------------------------------------------------------------------- the file
def huffman_codes(counts, vals):
    """Annex C: {bit string: symbol} of the canonical code the 16 counts and the symbols define."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[format(code, f"0{length}b")] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return codes


def parse(data):
    """The supported files only (the refusals are the library's: tests/test_jpeg_decode_host.py)."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    p = Parsed()
    p.dri, quant, huff, at = 0, {}, {}, 2
    while True:
        assert data[at] == 0xFF
        marker = data[at + 1]
        length = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                table = np.zeros(64, np.int64)
                table[ZIGZAG] = list(body[1:65])
                quant[body[0] & 15] = table
                body = body[65:]
        elif marker == 0xC4:
            while body:
                counts = list(body[1:17])
                huff[body[0]] = (counts, list(body[17:17 + sum(counts)]))
                body = body[17 + sum(counts):]
        elif marker == 0xC0:
            assert body[0] == 8
            p.h, p.w, p.channels = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(p.channels)]
        elif marker == 0xDD:
            p.dri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            assert body[0] == p.channels
            p.tables = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(p.channels)]
            break
        else:
            assert marker not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "unsupported"
    p.hs, p.vs = (1, 1) if p.channels == 1 else comps[0][1:3]
    assert p.channels == 1 or all(c[1:3] == (1, 1) for c in comps[1:])
    p.quant = [quant[c[3]] for c in comps]
    p.dc_counts = [huff[td] for td, _ in p.tables]
    p.ac_counts = [huff[0x10 | ta] for _, ta in p.tables]
    p.dc = [huffman_codes(*t) for t in p.dc_counts]
    p.ac = [huffman_codes(*t) for t in p.ac_counts]
    p.mcus_x, p.mcus_y = -(-p.w // (8 * p.hs)), -(-p.h // (8 * p.vs))
    mcus = p.mcus_x * p.mcus_y
    p.n_intervals = -(-mcus // p.dri) if p.dri else 1
    # the walk: an interval ends at the 0xFF of a marker that is not a stuffed zero
    p.scan_begin, p.interval_at = at, [at]
    while True:
        at = data.index(b"\xff", at)
        if data[at + 1] == 0:
            at += 2
        elif 0xD0 <= data[at + 1] <= 0xD7:
            assert data[at + 1] == 0xD0 + (len(p.interval_at) - 1) % 8
            at += 2
            p.interval_at.append(at)
        else:
            assert data[at + 1] == 0xD9
            break
    p.scan_end = at
    p.interval_at.append(at + 2)           # interval i = bytes [interval_at[i], interval_at[i+1] - 2)
    assert len(p.interval_at) == p.n_intervals + 1
    # the blocks: component c is a grid of by[c] x bx[c] blocks from block first[c]
    p.bx = [p.mcus_x * (p.hs if c == 0 else 1) for c in range(p.channels)]
    p.by = [p.mcus_y * (p.vs if c == 0 else 1) for c in range(p.channels)]
    p.first = [sum(p.bx[k] * p.by[k] for k in range(c)) for c in range(p.channels)]
    p.blocks = sum(x * y for x, y in zip(p.bx, p.by))
    return p


# ------------------------------------------------------------------------------------------------- rule 1: entropy
def _symbol(bits, at, codes, stats):
    for length in range(1, 17):
        s = codes.get(bits[at:at + length])
        if s is not None and len(bits) >= at + length:
            stats["longest_code"] = max(stats["longest_code"], length)
            return s, at + length
    raise ValueError("invalid Huffman code")


def _extend(bits, at, size):
    if size == 0:
        return 0, at
    v = int(bits[at:at + size], 2)
    return (v if v >= 1 << (size - 1) else v - (1 << size) + 1), at + size


def coefficients(data, with_stats=False):
    data = bytes(data)
    p = parse(data)
    coef = np.zeros((p.blocks, 64), np.int16)
    stats = {"longest_code": 0, "zrl": 0, "no_eob": 0, "dc_category": 0, "stuffed": 0}
    per = p.dri if p.dri else p.mcus_x * p.mcus_y
    for i in range(p.n_intervals):
        raw = data[p.interval_at[i]:p.interval_at[i + 1] - 2]
        stats["stuffed"] += raw.count(b"\xff\x00")
        bits = "".join(format(b, "08b") for b in raw.replace(b"\xff\x00", b"\xff"))
        at, pred = 0, [0] * p.channels
        for m in range(i * per, min((i + 1) * per, p.mcus_x * p.mcus_y)):
            my, mx = divmod(m, p.mcus_x)
            for c in range(p.channels):
                nh, nv = (p.hs, p.vs) if c == 0 else (1, 1)
                for v in range(nv):
                    for h in range(nh):
                        block = coef[p.first[c] + (my * nv + v) * p.bx[c] + mx * nh + h]
                        size, at = _symbol(bits, at, p.dc[c], stats)
                        assert size <= 11
                        stats["dc_category"] = max(stats["dc_category"], size)
                        diff, at = _extend(bits, at, size)
                        pred[c] += diff
                        block[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs, at = _symbol(bits, at, p.ac[c], stats)
                            run, size = rs >> 4, rs & 15
                            if size == 0:
                                if run != 15:
                                    break
                                stats["zrl"] += 1
                                k += 16
                                continue
                            k += run
                            assert k <= 63
                            block[ZIGZAG[k]], at = _extend(bits, at, size)
                            k += 1
                        else:
                            stats["no_eob"] += 1
        assert len(bits) - at < 8 and set(bits[at:]) <= {"1"}      # the padding of the last byte
    return (coef, p, stats) if with_stats else coef


# ------------------------------------------------------------------------------------------------- rule 2: the transform
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(i, n):
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i7, i5, i3, i1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1 = z1 * -7373
    z2 = z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    return [_descale(x, n) for x in (t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d)]


def idct_blocks(coef, quant):
    """int [N,64] coefficients, int [64] table -> uint8 [N,8,8] samples."""
    x = (coef.astype(np.int64) * quant[None, :]).reshape(-1, 8, 8)
    cols = np.stack(_idct_1d([x[:, r, :] for r in range(8)], 11), axis=1)           # over the 8 columns: along the rows axis
    rows = np.stack(_idct_1d([cols[:, :, c] for c in range(8)], 18), axis=2)        # then over the 8 rows
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def planes(data):
    """The component planes, padding included: [uint8 [by * 8, bx * 8]] and the Parsed."""
    coef, p, _ = coefficients(data, with_stats=True)
    out = []
    for c in range(p.channels):
        n = p.bx[c] * p.by[c]
        blocks = idct_blocks(coef[p.first[c]:p.first[c] + n], p.quant[c])
        out.append(blocks.reshape(p.by[c], p.bx[c], 8, 8).transpose(0, 2, 1, 3).reshape(p.by[c] * 8, p.bx[c] * 8))
    return out, p


# ------------------------------------------------------------------------------------------------- rule 3: upsampling
def upsample(P, hs, vs, w, h):
    """The dh x dw picture part of a chroma plane -> h x w (int)."""
    dh, dw = -(-h // vs), -(-w // hs)
    P = P[:dh, :dw].astype(np.int64)
    if hs == 1:
        return P[:h, :w]
    if dw <= 2:
        return np.repeat(np.repeat(P, vs, axis=0), 2, axis=1)[:h, :w]
    x = np.arange(dw)
    left, right = np.maximum(x - 1, 0), np.minimum(x + 1, dw - 1)
    if vs == 1:
        out = np.zeros((dh, 2 * dw), np.int64)
        out[:, 0::2] = (3 * P + P[:, left] + 1) >> 2
        out[:, 1::2] = (3 * P + P[:, right] + 2) >> 2
        out[:, 0], out[:, -1] = P[:, 0], P[:, -1]
        return out[:h, :w]
    r = np.arange(dh)
    out = np.zeros((2 * dh, 2 * dw), np.int64)
    for parity, nbr in ((0, np.maximum(r - 1, 0)), (1, np.minimum(r + 1, dh - 1))):
        S = 3 * P + P[nbr]
        rows = np.zeros((dh, 2 * dw), np.int64)
        rows[:, 0::2] = (3 * S + S[:, left] + 8) >> 4
        rows[:, 1::2] = (3 * S + S[:, right] + 7) >> 4
        rows[:, 0], rows[:, -1] = (4 * S[:, 0] + 8) >> 4, (4 * S[:, -1] + 7) >> 4
        out[parity::2] = rows
    return out[:h, :w]


# ------------------------------------------------------------------------------------------------- rule 4: colour
def decode(data):
    """uint8 [h,w,3] (RGB) or [h,w] (gray): what np.asarray(PIL.Image.open(...)) gives."""
    pl, p = planes(data)
    Y = pl[0][:p.h, :p.w].astype(np.int64)
    if p.channels == 1:
        return Y.astype(np.uint8)
    cb = upsample(pl[1], p.hs, p.vs, p.w, p.h) - 128
    cr = upsample(pl[2], p.hs, p.vs, p.w, p.h) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- the cases
def content(kind, h, w, c, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "checker":           # 8 x 8 blocks of 0 and 255: DC differences of the largest categories
        y, x = np.mgrid[:h, :w]
        return np.repeat(((((y // 8) + (x // 8)) % 2) * 255).astype(np.uint8)[..., None], c, axis=2)
    assert kind == "smooth"
    y, x = np.mgrid[:h, :w].astype(np.float64)
    ch = [127.5 + 120 * np.sin(0.11 * x * (k + 1) + rng.uniform(0, 6)) * np.cos(0.07 * y * (k + 2) + rng.uniform(0, 6))
          for k in range(c)]
    return np.clip(np.stack(ch, axis=2) + rng.normal(0, 3, (h, w, c)), 0, 255).astype(np.uint8)


def _case(h, w, kind, quality, mode, needs=(), **save):
    return {"h": h, "w": w, "content": kind, "quality": quality, "mode": mode, "needs": tuple(needs), "save": save}


CASES = {}
for _mode in ("4:4:4", "4:2:2", "4:2:0", "gray"):
    for _h, _w in ((1, 1), (8, 8), (9, 9), (17, 33)):
        CASES[f"smooth_{_h}x{_w}_{_mode}"] = _case(_h, _w, "smooth", 85, _mode, ["no_dri", _mode] + (["odd"] if _h % 2 else []))
for _mode in ("4:2:2", "4:2:0"):
    for _w, _dw in ((2, 1), (3, 2), (5, 3)):
        CASES[f"chroma_width_{_dw}_{_mode}"] = _case(5, _w, "noise", 90, _mode, [f"chroma_width_{_dw}", _mode])
CASES.update({
    "noise_q100_4:4:4": _case(48, 64, "noise", 100, "4:4:4", ["stuffed", "no_eob"]),
    "noise_optimized_4:2:0": _case(61, 83, "noise", 90, "4:2:0", ["code_12_bits", "odd"], optimize=True),
    "noise_optimized_gray": _case(61, 83, "noise", 90, "gray", ["code_12_bits"], optimize=True),
    "noise_q30_4:2:2": _case(15, 31, "noise", 30, "4:2:2", ["zrl", "odd"]),
    "checker_q100_gray": _case(16, 32, "checker", 100, "gray", ["dc_category_10"]),
    "intervals_of_3_4:4:4": _case(100, 131, "smooth", 75, "4:4:4", ["intervals_65", "intervals_9", "short_last_interval"],
                                  restart_marker_blocks=3),
    "intervals_of_1_4:2:0": _case(9, 130, "noise", 75, "4:2:0", ["dri_1", "intervals_9"], restart_marker_blocks=1),
    "interval_rows_gray": _case(37, 53, "smooth", 85, "gray", ["dri"], restart_marker_rows=1),
    "interval_rows_4:2:0": _case(48, 64, "smooth", 50, "4:2:0", ["dri"], restart_marker_rows=1),
    "interval_rows_4:2:2": _case(31, 15, "noise", 85, "4:2:2", ["dri", "odd"], restart_marker_rows=1),
})
NEEDED = {"stuffed", "code_12_bits", "zrl", "no_eob", "dc_category_10", "dri_1", "intervals_65", "intervals_9",
          "short_last_interval", "no_dri", "4:4:4", "4:2:2", "4:2:0", "gray", "chroma_width_1", "chroma_width_2",
          "chroma_width_3", "odd"}
SIZES_NEEDED = {(1, 1), (8, 8), (9, 9), (17, 33)}


def check_needs(name, data):
    """Asserts every precondition the case `name` records, on the file itself."""
    case = CASES[name]
    _, p, stats = coefficients(data, with_stats=True)
    mcus = p.mcus_x * p.mcus_y
    holds = {
        "stuffed": stats["stuffed"] > 0, "code_12_bits": stats["longest_code"] >= 12, "zrl": stats["zrl"] > 0,
        "no_eob": stats["no_eob"] > 0, "dc_category_10": stats["dc_category"] >= 10, "dri": p.dri > 0, "dri_1": p.dri == 1,
        "intervals_65": p.n_intervals > 64, "intervals_9": p.n_intervals > 8,
        "short_last_interval": p.dri > 0 and mcus % p.dri != 0, "no_dri": p.dri == 0 and p.n_intervals == 1,
        "4:4:4": p.channels == 3 and (p.hs, p.vs) == (1, 1), "4:2:2": p.channels == 3 and (p.hs, p.vs) == (2, 1),
        "4:2:0": p.channels == 3 and (p.hs, p.vs) == (2, 2), "gray": p.channels == 1,
        "odd": p.h % 2 == 1 and p.w % 2 == 1,
    }
    for k in (1, 2, 3):
        holds[f"chroma_width_{k}"] = p.channels == 3 and p.hs == 2 and -(-p.w // 2) == k
    assert (p.h, p.w) == (case["h"], case["w"])
    for need in case["needs"]:
        assert holds[need], f"{name}: the file no longer meets its precondition {need!r} ({stats})"


def check_table():
    """The table as a whole holds every kind of case the decoder's tests must contain."""
    have = set().union(*(c["needs"] for c in CASES.values()))
    assert NEEDED <= have, NEEDED - have
    assert SIZES_NEEDED <= {(c["h"], c["w"]) for c in CASES.values()}


def pillow_file(name):
    """(bytes, Pillow's pixels) of the case, made now (the golden generator and the live test)."""
    import io

    from PIL import Image
    case = CASES[name]
    gray = case["mode"] == "gray"
    image = content(case["content"], case["h"], case["w"], 1 if gray else 3, seed=zlib.crc32(name.encode()))
    kw = dict(case["save"])
    if not gray:
        kw["subsampling"] = PIL_SUBSAMPLING[case["mode"]]
    buf = io.BytesIO()
    Image.fromarray(image[..., 0] if gray else image).save(buf, "JPEG", quality=case["quality"], **kw)
    return buf.getvalue(), np.asarray(Image.open(io.BytesIO(buf.getvalue())))


_golden = None


def golden():
    """name -> (file bytes, Pillow's pixels) from tests/golden/jpeg_decode_golden.npz: read once, shared."""
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {name: (z[f"file/{name}"].tobytes(), z[f"pixels/{name}"]) for name in CASES}
    return _golden


_wanted = {}


def expected(name):
    """The restatement's pixels of the golden file `name`, as [h,w,c]: computed once."""
    if name not in _wanted:
        px = decode(golden()[name][0])
        _wanted[name] = px[..., None] if px.ndim == 2 else px
    return _wanted[name]


# ------------------------------------------------------------------------------------------------- malformed scans
def _standard_gray_file(scan):
    """An 8 x 8 gray file around `scan` (bytes, already stuffed): the headers of the smooth 8 x 8 gray case (Pillow's
    standard tables, no DRI: one MCU, one interval)."""
    data = golden()["smooth_8x8_gray"][0]
    p = parse(data)
    return data[:p.scan_begin] + scan + b"\xff\xd9", p


def malformed_scans():
    """name -> (file, the DGS_JPEG_S_* status its one interval must end with).  The parser accepts all three: what is
    wrong with them shows only when the scan is decoded."""
    data, pixels = golden()["noise_q100_4:4:4"]
    p = parse(data)
    middle = (p.scan_begin + p.scan_end) // 2
    cut = data[:middle] + data[p.scan_end:]                     # half the scan missing, EOI in place
    _, p8 = _standard_gray_file(b"")
    assert "1" * 16 not in "".join(p8.dc[0])                    # the all-ones prefix is no code of the standard DC table
    bad_code, _ = _standard_gray_file(b"\xff\x00" * 8)
    # DC category 0, then (run 15, size 1) four times: index 16, 32, 48 -- and 64
    dc0 = next(k for k, v in p8.dc[0].items() if v == 0)
    f1 = next(k for k, v in p8.ac[0].items() if v == 0xF1)
    bits = dc0 + (f1 + "1") * 4
    bits += "1" * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    too_long, _ = _standard_gray_file(raw)
    return {"truncated_scan": (cut, 5), "invalid_code": (bad_code, 2), "over_long_block": (too_long, 3)}

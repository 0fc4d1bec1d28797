"""A numpy reference painter for dgs_draw_prims and the cases its tests share (tests/test_progress_host.py,
tests/test_gpu_progress.py).

The painter WALKS: a line is the integer Bresenham walk, step by step, with error term maj - 2 min and the minor step
taken when the error is negative (a tie stays with the start point); records are painted in list order, so a later one
overwrites an earlier one; a disc is its inequality over its bounding box.  It does not use the kernel's closed form for
the minor offset (closed_form_offset below restates that one, for the comparison the host test makes).

A line whose start lies far outside the canvas would take up to 2^30 steps to reach it.  For more than FAR steps the walk's
state at the canvas edge is taken from its invariant instead -- after every step the error e satisfies
-2 min <= e < 2 maj - 2 min and e = maj - 2 min (s + 1) + 2 maj off, which fixes off -- and the walk goes on step by step
from there.  The host test holds that shortcut to the plain walk at distances the plain walk can still cover.
"""
import numpy as np

W, H = 67, 45                       # the draw tests' canvas: no multiple of 64 or 16
MAX_COORD = 1 << 29
MAX_RADIUS = 64
FAR = 4096


def rgb_word(r, g, b):
    return int(r) | int(g) << 8 | int(b) << 16


def skipped(rec):
    x0, y0, x1, y1, r, _ = (int(v) for v in rec)
    if r < 0 or max(abs(x0), abs(y0), abs(x1), abs(y1)) > MAX_COORD:
        return True
    return r > 0 and (x0 != x1 or y0 != y1 or r > MAX_RADIUS)


def walk(x0, y0, x1, y1):
    """Every pixel of the line, in order, from the start point: the plain walk."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
    steep = dy > dx
    maj, mn = (dy, dx) if steep else (dx, dy)
    x, y, e = x0, y0, maj - 2 * mn
    out = [(x, y)]
    for _ in range(maj):
        if e < 0:
            e += 2 * maj
            if steep:
                x += sx
            else:
                y += sy
        e -= 2 * mn
        if steep:
            y += sy
        else:
            x += sx
        out.append((x, y))
    return out


def closed_form_offset(maj, mn, i):
    """The minor offset at step i as include/dgs_hip.h states it."""
    return 0 if maj == 0 else (2 * mn * i + maj - 1) // (2 * maj)


def line_pixels(x0, y0, x1, y1, w, h, far=FAR):
    """The pixels of the walk that lie inside a w x h canvas.  The walk is entered at the first step whose major
    coordinate is inside (by the invariant when that is more than `far` steps away, else by walking) and left at the
    first step whose major coordinate has passed the canvas."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
    steep = dy > dx
    maj, mn = (dy, dx) if steep else (dx, dy)
    m0, n0, sm, sn, lm, ln = (y0, x0, sy, sx, h, w) if steep else (x0, y0, sx, sy, w, h)
    skip = 0
    if sm > 0 and m0 < 0:
        skip = -m0
    elif sm < 0 and m0 > lm - 1:
        skip = m0 - (lm - 1)
    if skip > maj:
        return []
    i, off, e = 0, 0, maj - 2 * mn
    if skip > far:
        i = skip
        off = -((maj - 2 * mn * i) // (2 * maj))            # ceil((2 min i - maj) / (2 maj)): the invariant's only solution
        e = maj - 2 * mn * (i + 1) + 2 * maj * off
        assert -2 * mn <= e < 2 * maj - 2 * mn
    out = []
    while True:
        m, n = m0 + sm * i, n0 + sn * off
        if (sm > 0 and m > lm - 1) or (sm < 0 and m < 0):
            break
        if 0 <= m < lm and 0 <= n < ln:
            out.append((n, m) if steep else (m, n))
        if i == maj:
            break
        if e < 0:
            e += 2 * maj
            off += 1
        e -= 2 * mn
        i += 1
    return out


def paint(img, prims):
    """img uint8 [h,w,3] (a copy is painted and returned), prims int [n,6]: painter's order, record by record."""
    out = img.copy()
    h, w = out.shape[:2]
    for rec in np.asarray(prims).tolist():
        if skipped(rec):
            continue
        x0, y0, x1, y1, r, rgb = rec
        colour = (rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255)
        if r == 0:
            for x, y in line_pixels(x0, y0, x1, y1, w, h):
                out[y, x] = colour
            continue
        for y in range(max(y0 - r, 0), min(y0 + r, h - 1) + 1):
            for x in range(max(x0 - r, 0), min(x0 + r, w - 1) + 1):
                if (x - x0) ** 2 + (y - y0) ** 2 <= r * r:
                    out[y, x] = colour
    return out


def paint_lines_batched(img, prims):
    """paint() for a long list of r == 0 records with near endpoints: the same walk, all records advancing one step per
    iteration (the state of every walk is a numpy vector); a pixel keeps the highest record index that reached it."""
    p = np.asarray(prims).astype(np.int64)
    assert (p[:, 4] == 0).all() and np.abs(p[:, :4]).max() < 1 << 20
    h, w = img.shape[:2]
    x0, y0, x1, y1 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    sx, sy = np.sign(x1 - x0), np.sign(y1 - y0)
    steep = dy > dx
    maj, mn = np.where(steep, dy, dx), np.where(steep, dx, dy)
    x, y, e = x0.copy(), y0.copy(), maj - 2 * mn
    owner = np.zeros(h * w, dtype=np.int64)
    tag = np.arange(1, len(p) + 1)
    for i in range(int(maj.max()) + 1):
        live = i <= maj
        ok = live & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        np.maximum.at(owner, (y * w + x)[ok], tag[ok])
        turn = live & (e < 0)
        e = np.where(turn, e + 2 * maj, e)
        x = np.where(turn & steep, x + sx, x)
        y = np.where(turn & ~steep, y + sy, y)
        e = e - 2 * mn
        x = np.where(~steep, x + sx, x)
        y = np.where(steep, y + sy, y)
    out = img.copy().reshape(-1, 3)
    hit = owner > 0
    rgb = p[owner[hit] - 1, 5]
    out[hit] = np.stack([rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255], axis=1).astype(np.uint8)
    return out.reshape(img.shape)


def canvas(seed=0, w=W, h=H):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _records(rows):
    return np.asarray(rows, dtype=np.int64).reshape(-1, 6).astype(np.int32)


def _colours(n, seed):
    rng = np.random.default_rng(seed)
    return [rgb_word(*rng.integers(0, 256, size=3)) for _ in range(n)]


def _lines(pairs, seed=1):
    cs = _colours(len(pairs), seed)
    return _records([(a[0], a[1], b[0], b[1], 0, c) for (a, b), c in zip(pairs, cs)])


def _both_ways(pairs):
    return [q for a, b in pairs for q in ((a, b), (b, a))]


def draw_cases():
    """name -> int32 [n,6]: the small cases of the 67 x 45 canvas."""
    c = (33, 22)
    far = MAX_COORD
    octants = [(c, (c[0] + dx, c[1] + dy)) for dx, dy in
               ((25, 9), (9, 20), (-9, 20), (-25, 9), (-25, -9), (-9, -20), (9, -20), (25, -9))]
    cases = {
        "octants": _lines(_both_ways(octants)),
        "axis and diagonal": _lines(_both_ways([((3, 5), (60, 5)), ((7, 2), (7, 40)), ((10, 3), (45, 38)),
                                                ((50, 4), (15, 39))])),
        "single point": _lines([((12, 9), (12, 9)), ((0, 0), (0, 0)), ((W - 1, H - 1), (W - 1, H - 1)), ((W, 3), (W, 3)),
                                ((-1, -1), (-1, -1))]),
        "tie forward": _lines([((0, 0), (4, 2))]),
        "tie backward": _lines([((4, 2), (0, 0))]),
        "outside": _lines(_both_ways([((-30, -5), (-2, 60)), ((70, 0), (90, 44)), ((0, -9), (66, -1)), ((0, 45), (66, 80)),
                                      ((-20, 50), (-1, 46)), ((67, -3), (200, -40))])),
        "borders and corners": _lines(_both_ways([((-10, 20), (10, 25)), ((60, 10), (80, 14)), ((30, -8), (33, 8)),
                                                  ((20, 40), (26, 60)), ((-5, -3), (6, 5)), ((72, -6), (60, 7)),
                                                  ((-6, 50), (7, 38)), ((70, 49), (61, 39)), ((-20, 22), (90, 23)),
                                                  ((33, -30), (35, 80)), ((-3, -2), (69, 46))])),
        "far endpoints": _lines(_both_ways([((5, 7), (far, far // 3)), ((40, 30), (-far, -far // 2)), ((20, 10), (far, 11)),
                                            ((30, 44), (31, -far)), ((-far, -far), (far, far)), ((-far, 20), (far, 24)),
                                            ((10, far), (50, -far)), ((-far, far - 60), (far - 120, -far))])),
        "beyond the limit": _lines(_both_ways([((5, 7), (far + 1, 9)), ((3, -far - 1), (3, 40)), ((0, 0), (66, 44))])[:-1]),
        "negative radius": _records([(2, 2, 60, 40, -1, rgb_word(255, 0, 0)), (10, 10, 10, 10, -3, rgb_word(0, 255, 0)),
                                     (5, 40, 60, 3, 0, rgb_word(0, 0, 255)), (0, 0, 66, 44, -2147483648, 7)]),
        "three on one pixel": _records([(0, 10, 66, 10, 0, rgb_word(255, 0, 0)), (30, 0, 30, 44, 0, rgb_word(0, 255, 0)),
                                        (20, 0, 40, 20, 0, rgb_word(0, 0, 255)), (30, 10, 30, 10, 4, rgb_word(9, 8, 7)),
                                        (25, 10, 35, 10, 0, rgb_word(200, 100, 50))]),
        "bad discs": _records([(10, 10, 11, 10, 3, 1), (10, 10, 10, 12, 3, 2), (30, 20, 30, 20, 65, 3),
                               (30, 20, 30, 20, 64, 4), (5, 5, 5, 5, 1, 5)]),
    }
    rng = np.random.default_rng(7)
    pts = rng.integers(-30, 101, size=(300, 4))
    segs = np.concatenate([pts, np.zeros((300, 1), dtype=np.int64), np.asarray(_colours(300, 8))[:, None]], axis=1)
    centre = np.stack([rng.integers(-4, W + 4, size=40), rng.integers(-4, H + 4, size=40)], axis=1)
    discs = np.concatenate([centre, centre, rng.integers(1, 6, size=(40, 1)), np.asarray(_colours(40, 9))[:, None]], axis=1)
    mixed = np.concatenate([segs, discs])
    cases["random"] = _records(mixed[rng.permutation(len(mixed))])
    return cases


def large_case(n=4000, w=1920, h=1080, seed=11):
    """n segments over a w x h canvas, some crossing its border; lengths up to 600 pixels per axis."""
    rng = np.random.default_rng(seed)
    start = np.stack([rng.integers(-100, w + 100, size=n), rng.integers(-100, h + 100, size=n)], axis=1)
    delta = rng.integers(-600, 601, size=(n, 2))
    return _records(np.concatenate([start, start + delta, np.zeros((n, 1), dtype=np.int64),
                                    np.asarray(_colours(n, seed + 1))[:, None]], axis=1))


# ------------------------------------------------------------------------------------------------- camera cones
CONNECTIVITY = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1)]


def cone_reference(view, campos, cone_x, cone_y, scale, render_view, render_proj, w, h):
    """utils/visualization.py:159-185 in float64 numpy for C cameras: view float32 [C,4,4], campos float32 [C,3], the render
    camera's two float32 [4,4] matrices.  Returns (pix float64 [C,5,2], skip bool [C])."""
    pix, skip = [], []
    for V, centre in zip(view, campos):
        c2w = np.eye(4)
        c2w[:3, :3] = V[:3, :3]
        c2w[:3, 3] = centre
        cone = np.pad(np.array([[0.0, 0.0, 0.0], [cone_x, cone_y, 1.0], [cone_x, -cone_y, 1.0], [-cone_x, -cone_y, 1.0],
                                [-cone_x, cone_y, 1.0]]) * scale, ((0, 0), (0, 1)), "constant", constant_values=1.0)
        world = cone @ c2w.T
        cam_hom = cone @ render_view
        skip.append(bool((cam_hom[:, 2] / cam_hom[:, 3] < 0.1).any()))
        ndc_hom = world @ render_proj
        ndc = ndc_hom[:, :3] / ndc_hom[:, 3:]
        pix.append(((ndc[:, :2] + 1.0) * np.array([w, h]).astype(float) - 1.0) * 0.5)
    return np.stack(pix), np.asarray(skip)

"""numpy restatement of box-scaled strength (include/vdmi.h at vd_cells): the cell level of a
box, pixelation with a per-box level, and the scaled smooth blur, all in Python ints, that the
GPU path must match to the bit. Both frame functions have the rect_fn(img, boxes) shape that
mask_ref.shaped_frame expects once level and cells are bound."""
import numpy as np

from oracle import mosaic as omosaic

CELLS_MIN, CELLS_MAX = 2, 64
LEVEL_MAX = 32768


def level(W, H, level, cells):
    """L(b) for a box of unclipped size W x H: `level` with cells off or for an empty box,
    otherwise at least `level` and large enough that the longer side holds at most `cells`
    cells, clamped to 32768."""
    W, H, level, cells = int(W), int(H), int(level), int(cells)
    if cells == 0 or W <= 0 or H <= 0:
        return level
    return max(level, min(LEVEL_MAX, (max(W, H) + cells - 1) // cells))


def box_level(box, lvl, cells):
    x1, y1, x2, y2 = (int(v) for v in box)
    return level(x2 - x1, y2 - y1, lvl, cells)


def _clip(box, h, w):
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, y1, x2, y2 = max(0, x1), max(0, y1), min(w, x2), min(h, y2)
    return (x1, y1, x2, y2) if x2 > x1 and y2 > y1 else None


def mosaic_frame_cells(img, boxes, lvl, cells):
    """oracle.mosaic.mosaic_frame's loop with L(box) in place of the level: boxes in list
    order, each reading the previous box's output."""
    out = img.copy()
    h, w = out.shape[:2]
    for b in boxes:
        c = _clip(b, h, w)
        if c is None:
            continue
        x1, y1, x2, y2 = c
        L = box_level(b, lvl, cells)
        mx = omosaic.mosaic_axis_map(x2 - x1, L)
        my = omosaic.mosaic_axis_map(y2 - y1, L)
        out[y1:y2, x1:x2] = out[y1:y2, x1:x2][my][:, mx]
    return out


def cell_means(region, f):
    """Q8.4 means a[j][i][c] = (16 * S + n // 2) // n of the f x f cells anchored at the
    region's origin (the last cell of a row or column may be partial): int64 [sh][sw][3]."""
    bh, bw = region.shape[:2]
    sw, sh = -(-bw // f), -(-bh // f)
    a = np.zeros((sh, sw, 3), np.int64)
    r = region.astype(np.int64)
    for j in range(sh):
        for i in range(sw):
            cell = r[j * f:min((j + 1) * f, bh), i * f:min((i + 1) * f, bw)]
            n = cell.shape[0] * cell.shape[1]
            S = cell.reshape(-1, 3).sum(0)
            a[j, i] = (16 * S + n // 2) // n
    return a


def _axis(length, f, s):
    """Per position p of an axis: the two clamped cell indices and the weight r in [0, 2f) of
    the second (u = 2p + 1 - f, i0 = floor(u / 2f), r = u - 2f * i0)."""
    p = np.arange(length, dtype=np.int64)
    u = 2 * p + 1 - f
    i0 = u // (2 * f)                                  # numpy floors
    r = u - 2 * f * i0
    return np.clip(i0, 0, s - 1), np.clip(i0 + 1, 0, s - 1), r


def smooth_region(region, f):
    """The scaled smooth blur of one clipped region with cell size f: uint8 [bh][bw][3]."""
    bh, bw = region.shape[:2]
    a = cell_means(region, f)
    sh, sw = a.shape[:2]
    i0, i1, r = _axis(bw, f, sw)
    j0, j1, s = _axis(bh, f, sh)
    # t[j][x][c] = ((2f - r) a(i0, j) + r a(i1, j) + f) / 2f
    t = ((2 * f - r)[None, :, None] * a[:, i0] + r[None, :, None] * a[:, i1] + f) // (2 * f)
    assert t.max() <= 4080
    T = (2 * f - s)[:, None, None] * t[j0] + s[:, None, None] * t[j1]
    assert T.max() < 2 ** 32
    out = (T + 16 * f) // (32 * f)
    assert out.max() <= 255 and out.min() >= 0
    return out.astype(np.uint8)


def smooth_frame(img, boxes, lvl, cells):
    """Every box reads img; a pixel takes the value of the box with the largest f among those
    whose clipped rectangle holds it, ties to the lowest list index; other pixels are img."""
    h, w = img.shape[:2]
    out = img.copy()
    best = np.zeros((h, w), np.int64)                  # f of the owner so far (0: none)
    for b in boxes:
        c = _clip(b, h, w)
        if c is None:
            continue
        x1, y1, x2, y2 = c
        f = box_level(b, lvl, cells)
        res = smooth_region(img[y1:y2, x1:x2], f)
        win = best[y1:y2, x1:x2] < f                   # strictly larger: an equal f keeps the earlier box
        out[y1:y2, x1:x2][win] = res[win]
        best[y1:y2, x1:x2][win] = f
    return out


def grid(box, h, w, lvl, cells):
    """(sw, sh) of the smooth blur's cell grid of a box, or None when it clips to nothing."""
    c = _clip(box, h, w)
    if c is None:
        return None
    f = box_level(box, lvl, cells)
    return -(-(c[2] - c[0]) // f), -(-(c[3] - c[1]) // f)

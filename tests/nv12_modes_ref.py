"""numpy restatement of the NV12 smooth blur and the NV12 ellipse (include/vdmi.h at vd_nv12,
"smooth" and "ellipse"), written from the definitions, that the library must match to the bit.
Frames are nv12_ref's: uint8 [rows, w], H luma rows then H / 2 rows of interleaved U, V."""
import math

import numpy as np

import cells_ref
import mask_ref
import nv12_ref


# ---- the scaled smooth blur for any number of channels ---------------------------------------------

def cell_means(region, f):
    """Q8.4 means a[j][i][c] = (16 * S + n // 2) // n of the f x f cells anchored at the region's
    origin (the last of a row or column may be partial): int64 [sh][sw][C] for a region [bh][bw][C]."""
    bh, bw, C = region.shape
    sw, sh = -(-bw // f), -(-bh // f)
    a = np.zeros((sh, sw, C), np.int64)
    r = region.astype(np.int64)
    for j in range(sh):
        for i in range(sw):
            cell = r[j * f:min((j + 1) * f, bh), i * f:min((i + 1) * f, bw)]
            n = cell.shape[0] * cell.shape[1]
            a[j, i] = (16 * cell.reshape(-1, C).sum(0) + n // 2) // n
    return a


def _axis(length, f, s):
    """Per position p: the two clamped cell indices and the weight r in [0, 2f) of the second
    (u = 2p + 1 - f, i0 = floor(u / 2f), r = u - 2f * i0)."""
    u = 2 * np.arange(length, dtype=np.int64) + 1 - f
    i0 = u // (2 * f)                                  # numpy floors
    return np.clip(i0, 0, s - 1), np.clip(i0 + 1, 0, s - 1), u - 2 * f * i0


def smooth_region(region, f):
    """The scaled smooth blur of one clipped region [bh][bw][C] (or [bh][bw]) with cell size f."""
    flat = region.ndim == 2
    reg = region[:, :, None] if flat else region
    bh, bw = reg.shape[:2]
    a = cell_means(reg, f)
    sh, sw = a.shape[:2]
    i0, i1, r = _axis(bw, f, sw)
    j0, j1, s = _axis(bh, f, sh)
    t = ((2 * f - r)[None, :, None] * a[:, i0] + r[None, :, None] * a[:, i1] + f) // (2 * f)
    out = ((2 * f - s)[:, None, None] * t[j0] + s[:, None, None] * t[j1] + 16 * f) // (32 * f)
    assert out.max() <= 255 and out.min() >= 0
    out = out.astype(np.uint8)
    return out[:, :, 0] if flat else out


def rects(box, h, w):
    """(c, cc) of a box on an h x w frame: the luma clip and its chroma rectangle, or None."""
    c = nv12_ref.clip(box, h, w)
    return None if c is None else (c, nv12_ref.chroma_box(c))


def chroma_level(L):
    return (L + 1) >> 1


def smooth(frame, boxes, level, cells, height=None):
    """The smooth-blurred frame. Every box reads `frame`; per plane the owner of a sample is the box
    with the largest LUMA level L(b) among those whose rectangle of that plane holds it, ties to
    the lowest list index. Bytes outside the two planes' rows are copied unchanged."""
    frame = np.ascontiguousarray(frame)
    out = frame.copy()
    Yi, UVi = nv12_ref.planes(frame, height)
    Yo, UVo = nv12_ref.planes(out, height)
    h, w = Yi.shape
    best = [np.zeros((h, w), np.int64), np.zeros((h // 2, w // 2), np.int64)]   # L of the owner so far (0: none)
    for b in boxes:
        rc = rects(b, h, w)
        if rc is None:
            continue
        L = cells_ref.box_level(b, level, cells)
        for P, (src, dst, q, f) in enumerate(((Yi, Yo, rc[0], L), (UVi, UVo, rc[1], chroma_level(L)))):
            x1, y1, x2, y2 = q
            res = smooth_region(src[y1:y2, x1:x2], f)
            win = best[P][y1:y2, x1:x2] < L            # strictly larger: an equal L keeps the earlier box
            dst[y1:y2, x1:x2][win] = res[win]
            best[P][y1:y2, x1:x2][win] = L
    return out


def chroma_grid(box, h, w, level, cells):
    """((sw, sh) luma, (sw, sh) chroma) of the smooth blur's cell grids of a box, or None."""
    rc = rects(box, h, w)
    if rc is None:
        return None
    L = cells_ref.box_level(box, level, cells)
    (c, cc), fc = rc, chroma_level(L)
    return ((-(-(c[2] - c[0]) // L), -(-(c[3] - c[1]) // L)),
            (-(-(cc[2] - cc[0]) // fc), -(-(cc[3] - cc[1]) // fc)))


# ---- the ellipse on both planes ----------------------------------------------------------------------

def ellipse_mask(h, w, box):
    """mask_ref.ellipse_mask with the predicate evaluated on int64 arrays (every term <= 2^61)."""
    m = np.zeros((h, w), bool)
    c = mask_ref.clip(box, h, w)
    if c is None:
        return m
    x1, y1, x2, y2 = (int(v) for v in box)
    W, H = x2 - x1, y2 - y1
    if W > mask_ref.SIDE_MAX or H > mask_ref.SIDE_MAX:
        m[c[1]:c[3], c[0]:c[2]] = True
        return m
    dx = 2 * np.arange(c[0], c[2], dtype=np.int64) + 1 - (x1 + x2)
    dy = 2 * np.arange(c[1], c[3], dtype=np.int64) + 1 - (y1 + y2)
    m[c[1]:c[3], c[0]:c[2]] = (dx * dx * H * H)[None, :] + (dy * dy * W * W)[:, None] <= W * W * H * H
    return m


def hidden_luma(h, w, grown):
    m = np.zeros((h, w), bool)
    for b in grown:
        m |= ellipse_mask(h, w, b)
    return m


def hidden_chroma(hl):
    """The four-pixel rule, literally: sample (cy, cx) is hidden iff one of the luma pixels
    (2cy + {0, 1}, 2cx + {0, 1}) is."""
    h, w = hl.shape
    hc = np.zeros((h // 2, w // 2), bool)
    for cy in range(h // 2):
        for cx in range(w // 2):
            hc[cy, cx] = hl[2 * cy, 2 * cx] or hl[2 * cy, 2 * cx + 1] or hl[2 * cy + 1, 2 * cx] or hl[2 * cy + 1, 2 * cx + 1]
    return hc


def row_span(box, c, y):
    """[xl, xr) of row y of the clipped rectangle c inside the box's ellipse, as the restore kernels
    find it (q = floor((W^2 H^2 - dy^2 W^2) / H^2), s = floor(sqrt(q)), |2x + 1 - (x1 + x2)| <= s);
    None when y is not a row of c."""
    if not c[1] <= y < c[3]:
        return None
    x1, y1, x2, y2 = (int(v) for v in box)
    W, H = x2 - x1, y2 - y1
    if W > mask_ref.SIDE_MAX or H > mask_ref.SIDE_MAX:
        return c[0], c[2]
    dy, sx = 2 * y + 1 - (y1 + y2), x1 + x2
    s = math.isqrt((W * W * H * H - dy * dy * W * W) // (H * H))
    xl = min(max((sx - s) >> 1, c[0]), c[2])
    return xl, max(min(((sx - 1 + s) >> 1) + 1, c[2]), xl)


def hidden_chroma_spans(h, w, grown):
    """The span form: for box k the hidden samples of chroma row cy are the union of
    [xl >> 1, (xr + 1) >> 1) over the non-empty spans of luma rows 2cy and 2cy + 1."""
    hc = np.zeros((h // 2, w // 2), bool)
    for b in grown:
        c = mask_ref.clip(b, h, w)
        if c is None:
            continue
        for y in range(c[1], c[3]):
            xl, xr = row_span(b, c, y)
            if xl < xr:
                hc[y >> 1, xl >> 1:(xr + 1) >> 1] = True
    return hc


def shaped(frame, boxes, shape, g, rect_fn, height=None):
    """The frame a context with mask (shape, g) writes: rect_fn(frame, grown boxes) is the
    rectangular NV12 pass R (nv12_ref.mosaic or smooth above with their parameters bound); under
    "ellipse" luma is R where hidden and chroma is R where one of the sample's four luma pixels is."""
    grown = mask_ref.grow_list(boxes, g)
    R = rect_fn(frame, grown)
    if shape == "rect":
        return R
    assert shape == "ellipse"
    out = np.array(frame, copy=True)
    Yo, UVo = nv12_ref.planes(out, height)
    Yr, UVr = nv12_ref.planes(R, height)
    h, w = Yo.shape
    hl = hidden_luma(h, w, grown)
    hc = hidden_chroma(hl)
    Yo[hl] = Yr[hl]
    UVo[hc] = UVr[hc]
    return out

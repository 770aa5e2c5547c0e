"""numpy reference for 10- and 12-bit 4:2:0 frames (include/vdmi.h at vd_yuv420_16). Packed frames are
uint16 [n, 3h/2, w] in the layouts of tests/yuv420_ref.py, a word per sample; the value of a word is
(word >> shift) & (2^depth - 1). Here: the re-layout of words, D(S) / lo(S) / hi(S), padded buffers
with byte-counted fields, pixelation by the lo / hi definition, and the scaled smooth blur on values of
`depth` bits (cells_ref.smooth_region asserts 8-bit bounds), written from the definitions."""
import numpy as np

import cells_ref
import nv12_modes_ref as nm
import nv12_ref as nr

LAYOUTS = ("i420", "yv12", "nv12", "nv21")
INTERLEAVED = ("nv12", "nv21")


def default_shift(layout, depth):
    """The P010 convention: high-aligned samples in the interleaved layouts, low-aligned in the planar ones."""
    return 16 - depth if layout in INTERLEAVED else 0


# ---- layouts (words only move) ------------------------------------------------------------------------

def planes_of(frames, layout):
    """(Y [n, h, w], U [n, h/2, w/2], V [n, h/2, w/2]) copies of packed frames in `layout`, any dtype."""
    frames = np.asarray(frames)
    n, rows, w = frames.shape
    assert rows % 3 == 0 and w % 2 == 0 and layout in LAYOUTS
    h = rows // 3 * 2
    c = frames[:, h:].reshape(n, -1)
    if layout in INTERLEAVED:
        p = c.reshape(n, h // 2, w // 2, 2)
        a, b = p[..., 0], p[..., 1]
    else:
        a, b = c[:, :h * w // 4].reshape(n, h // 2, w // 2), c[:, h * w // 4:].reshape(n, h // 2, w // 2)
    U, V = (a, b) if layout in ("i420", "nv12") else (b, a)
    return frames[:, :h].copy(), U.copy(), V.copy()


def pack(Y, U, V, layout):
    """Packed frames [n, 3h/2, w] in `layout` from the three planes (their dtype)."""
    n, h, w = Y.shape
    assert layout in LAYOUTS
    out = np.empty((n, h * 3 // 2, w), Y.dtype)
    out[:, :h] = Y
    a, b = (U, V) if layout in ("i420", "nv12") else (V, U)
    c = out[:, h:].reshape(n, -1)
    if layout in INTERLEAVED:
        p = c.reshape(n, h // 2, w // 2, 2)
        p[..., 0], p[..., 1] = a, b
    else:
        c[:, :h * w // 4] = a.reshape(n, -1)
        c[:, h * w // 4:] = b.reshape(n, -1)
    return out


def relayout(frames, src, dst):
    return pack(*planes_of(frames, src), dst)


# ---- D, lo, hi -------------------------------------------------------------------------------------

def values(frames, depth, shift):
    return (np.asarray(frames, np.uint16) >> shift) & ((1 << depth) - 1)


def D(frames, depth, shift):
    """The 8-bit picture detection sees: v >> (depth - 8), in the same packed layout."""
    return (values(frames, depth, shift) >> (depth - 8)).astype(np.uint8)


def lo(frames):
    return (np.asarray(frames, np.uint16) & 0xFF).astype(np.uint8)


def hi(frames):
    return (np.asarray(frames, np.uint16) >> 8).astype(np.uint8)


def join(low, high):
    return low.astype(np.uint16) | (high.astype(np.uint16) << 8)


def noise(n, h, w, depth, shift, seed):
    """Random values of `depth` bits at `shift`, random bits in every unused position."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << depth, (n, h * 3 // 2, w), dtype=np.uint16)
    junk = rng.integers(0, 1 << 16, v.shape, dtype=np.uint16)
    keep = np.uint16(((1 << depth) - 1) << shift)
    return (v << shift) | (junk & ~keep)


def widen(frames8, depth, shift, seed):
    """16-bit frames S with D(S) = frames8: random low value bits and random unused bits."""
    rng = np.random.default_rng(seed)
    f = np.asarray(frames8, np.uint16)
    v = (f << (depth - 8)) | rng.integers(0, 1 << (depth - 8), f.shape, dtype=np.uint16)
    junk = rng.integers(0, 1 << 16, f.shape, dtype=np.uint16)
    keep = np.uint16(((1 << depth) - 1) << shift)
    return (v << shift) | (junk & ~keep)


# ---- padded buffers: fields in bytes, the buffer in words -------------------------------------------------

def padded(frames, layout, pitch_w, cpitch_w, hpad, v_first, extra_w, fill=0xA5A5, base_pad_w=0):
    """yuv420_ref.padded for words: every *_w argument counts words. -> (uint16 buffer, fields) with the
    fields of vd_yuv420_16 in BYTES (pitch, u_offset, v_offset, chroma_pitch, frame_stride, base) and
    chroma_step in samples."""
    Y, U, V = planes_of(frames, layout)
    n, h, w = Y.shape
    step = 2 if layout in INTERLEAVED else 1
    c0 = hpad * pitch_w
    if step == 2:
        u, v = (c0 + 1, c0) if v_first else (c0, c0 + 1)
        stride = c0 + (h // 2) * cpitch_w + extra_w
    else:
        plane = (h // 2) * cpitch_w
        u, v = (c0 + plane, c0) if v_first else (c0, c0 + plane)
        stride = c0 + 2 * plane + extra_w
    buf = np.full(base_pad_w + n * stride, fill, np.uint16)
    for f in range(n):
        fr = buf[base_pad_w + f * stride:base_pad_w + (f + 1) * stride]
        fr[:h * pitch_w].reshape(h, pitch_w)[:, :w] = Y[f]
        for off, P in ((u, U), (v, V)):
            np.lib.stride_tricks.as_strided(fr[off:], (h // 2, w // 2), (2 * cpitch_w, 2 * step))[...] = P[f]
    return buf, dict(pitch=2 * pitch_w, u_offset=2 * u, v_offset=2 * v, chroma_pitch=2 * cpitch_w, chroma_step=step,
                     frame_stride=2 * stride, base=2 * base_pad_w)


def _plane_views(arr, fields, f, h, w):
    """(Y, U, V) strided views of frame f of a word array laid out by `fields`."""
    fr = arr[fields["base"] // 2 + f * (fields["frame_stride"] // 2):]
    it, step = arr.itemsize, fields["chroma_step"]
    scale = it / 2                      # fields count bytes of uint16 storage
    view = lambda off, rows, cols, pitch, st: np.lib.stride_tricks.as_strided(
        fr[off // 2:], (rows, cols), (int(pitch * scale), int(2 * st * scale)))
    return (view(0, h, w, fields["pitch"], 1), view(fields["u_offset"], h // 2, w // 2, fields["chroma_pitch"], step),
            view(fields["v_offset"], h // 2, w // 2, fields["chroma_pitch"], step))


def unpadded(buf, fields, n, h, w, layout):
    """The packed frames in `layout` holding the words a padded buffer describes."""
    Y = np.empty((n, h, w), np.uint16)
    U = np.empty((n, h // 2, w // 2), np.uint16)
    V = np.empty_like(U)
    for f in range(n):
        Y[f], U[f], V[f] = _plane_views(buf, fields, f, h, w)
    return pack(Y, U, V, layout)


def picture_mask(fields, n, h, w, size):
    """bool [size words]: the words of a padded buffer that belong to the picture."""
    m = np.zeros(size, bool)
    for f in range(n):
        for v in _plane_views(m, fields, f, h, w):
            v[...] = True
    return m


# ---- pixelation: the lo / hi definition -----------------------------------------------------------------

def mosaic(frames_nv12, lists, level, cells):
    """Packed NV12-layout uint16 frames pixelated: the low bytes are nv12_ref.mosaic of lo(S), the high
    bytes that of hi(S), with the same list, level and cells."""
    out = []
    for f, boxes in zip(np.asarray(frames_nv12), lists):
        out.append(join(nr.mosaic(lo(f), boxes, level, cells), nr.mosaic(hi(f), boxes, level, cells)))
    return np.stack(out)


# ---- the scaled smooth blur on values of `depth` bits ---------------------------------------------------------

def smooth_region(region, f, depth):
    """nv12_modes_ref.smooth_region on integer values below 2^depth: Q(depth).4 means, the same t, T and
    result; [bh][bw] int64 in and out."""
    reg = np.asarray(region, np.int64)[:, :, None]
    bh, bw = reg.shape[:2]
    a = nm.cell_means(reg, f)
    sh, sw = a.shape[:2]
    i0, i1, r = nm._axis(bw, f, sw)
    j0, j1, s = nm._axis(bh, f, sh)
    t = ((2 * f - r)[None, :, None] * a[:, i0] + r[None, :, None] * a[:, i1] + f) // (2 * f)
    T = (2 * f - s)[:, None, None] * t[j0] + s[:, None, None] * t[j1] + 16 * f
    assert t.max() <= 16 * ((1 << depth) - 1) and T.max() < 1 << 32      # the width bound of the header
    out = T // (32 * f)
    assert 0 <= out.min() and out.max() < 1 << depth
    return out[:, :, 0]


def smooth(frame_nv12, boxes, level, cells, depth, shift):
    """One packed NV12-layout uint16 frame [rows, w] smooth-blurred on its values: every box reads the
    input; per plane and channel the owner of a sample is the box with the largest luma level among those
    whose rectangle of that plane holds it (ties to the lowest index). An owned sample is result << shift
    with its unused bits zero; any other word is the input's."""
    frame = np.ascontiguousarray(frame_nv12, dtype=np.uint16)
    out = frame.copy()
    Yi, UVi = nr.planes(values(frame, depth, shift))
    Yo, UVo = nr.planes(out)
    h, w = Yi.shape
    best = [np.zeros((h, w), np.int64), np.zeros((h // 2, w // 2), np.int64)]
    for b in boxes:
        rc = nm.rects(b, h, w)
        if rc is None:
            continue
        L = cells_ref.box_level(b, level, cells)
        for P, (q, f) in enumerate(((rc[0], L), (rc[1], nm.chroma_level(L)))):
            x1, y1, x2, y2 = q
            win = best[P][y1:y2, x1:x2] < L
            if P == 0:
                res = smooth_region(Yi[y1:y2, x1:x2], f, depth)
                Yo[y1:y2, x1:x2][win] = (res[win] << shift).astype(np.uint16)
            else:
                for ch in range(2):
                    res = smooth_region(UVi[y1:y2, x1:x2, ch], f, depth)
                    UVo[y1:y2, x1:x2, ch][win] = (res[win] << shift).astype(np.uint16)
            best[P][y1:y2, x1:x2][win] = L
    return out


def shaped(frame_nv12, boxes, shape, g, rect_fn):
    """nv12_modes_ref.shaped on words: rect_fn(frame, grown boxes) is the rectangular pass R; under
    "ellipse" a luma word is R's where hidden, a chroma sample's two words are R's where one of its four
    luma pixels is hidden, and every other word is the input's."""
    import mask_ref
    grown = mask_ref.grow_list(boxes, g)
    R = rect_fn(frame_nv12, grown)
    if shape == "rect":
        return R
    out = np.array(frame_nv12, copy=True)
    Yo, UVo = nr.planes(out)
    Yr, UVr = nr.planes(R)
    hl = nm.hidden_luma(*Yo.shape, grown)
    hc = nm.hidden_chroma(hl)
    Yo[hl] = Yr[hl]
    UVo[hc] = UVr[hc]
    return out

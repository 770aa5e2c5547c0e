"""numpy re-layout between the 8-bit 4:2:0 layouts (include/vdmi.h at vd_yuv420) and NV12, the layout
tests/nv12_ref.py defines everything on. Packed frames are uint8 [n, 3h/2, w] in every layout: h luma
rows, then
  nv12 / nv21   h/2 rows of w bytes of interleaved (U, V) / (V, U) pairs;
  i420 / yv12   the first chroma plane's h/2 * w/2 bytes, then the second's: U, V / V, U.
Nothing is computed here: samples only move."""
import numpy as np

LAYOUTS = ("i420", "yv12", "nv12", "nv21")


def planes_of(frames, layout):
    """(Y [n, h, w], U [n, h/2, w/2], V [n, h/2, w/2]) copies of packed frames in `layout`."""
    frames = np.asarray(frames)
    n, rows, w = frames.shape
    assert rows % 3 == 0 and w % 2 == 0 and layout in LAYOUTS
    h = rows // 3 * 2
    c = frames[:, h:].reshape(n, -1)
    if layout in ("nv12", "nv21"):
        p = c.reshape(n, h // 2, w // 2, 2)
        a, b = p[..., 0], p[..., 1]
    else:
        a, b = c[:, :h * w // 4].reshape(n, h // 2, w // 2), c[:, h * w // 4:].reshape(n, h // 2, w // 2)
    U, V = (a, b) if layout in ("i420", "nv12") else (b, a)
    return frames[:, :h].copy(), U.copy(), V.copy()


def pack(Y, U, V, layout):
    """Packed frames [n, 3h/2, w] in `layout` from the three planes."""
    n, h, w = Y.shape
    assert layout in LAYOUTS
    out = np.empty((n, h * 3 // 2, w), np.uint8)
    out[:, :h] = Y
    a, b = (U, V) if layout in ("i420", "nv12") else (V, U)
    c = out[:, h:].reshape(n, -1)
    if layout in ("nv12", "nv21"):
        p = c.reshape(n, h // 2, w // 2, 2)
        p[..., 0], p[..., 1] = a, b
    else:
        c[:, :h * w // 4] = a.reshape(n, -1)
        c[:, h * w // 4:] = b.reshape(n, -1)
    return out


def to_nv12(frames, layout):
    """N(S): the packed NV12 frames with the same Y, U and V samples."""
    return pack(*planes_of(frames, layout), "nv12")


def from_nv12(frames, layout):
    """Packed frames in `layout` with the samples of packed NV12 frames."""
    return pack(*planes_of(frames, "nv12"), layout)


def padded(frames, layout, pitch, cpitch, hpad, v_first, extra, fill=0xA5, base_pad=0):
    """The samples of packed frames in `layout` laid out in one buffer filled with `fill`: luma rows of
    `pitch` bytes, padded to hpad rows; then the chroma in layout's step (planar: two planes of h/2 rows
    of cpitch bytes, V before U when v_first; interleaved: one plane of cpitch-byte rows, (V, U) pairs
    when v_first), then `extra` bytes to the next frame. base_pad bytes come before frame 0.
    -> (buffer, fields) with fields = dict(pitch, u_offset, v_offset, chroma_pitch, chroma_step,
    frame_stride, base)."""
    Y, U, V = planes_of(frames, layout)
    n, h, w = Y.shape
    step = 2 if layout in ("nv12", "nv21") else 1
    c0 = hpad * pitch
    if step == 2:
        u, v = (c0 + 1, c0) if v_first else (c0, c0 + 1)
        stride = c0 + (h // 2) * cpitch + extra
    else:
        plane = (h // 2) * cpitch
        u, v = (c0 + plane, c0) if v_first else (c0, c0 + plane)
        stride = c0 + 2 * plane + extra
    buf = np.full(base_pad + n * stride, fill, np.uint8)
    for f in range(n):
        fr = buf[base_pad + f * stride:base_pad + (f + 1) * stride]
        fr[:h * pitch].reshape(h, pitch)[:, :w] = Y[f]
        for off, P in ((u, U), (v, V)):
            rows = np.lib.stride_tricks.as_strided(fr[off:], (h // 2, w // 2), (cpitch, step))
            rows[...] = P[f]
    return buf, dict(pitch=pitch, u_offset=u, v_offset=v, chroma_pitch=cpitch, chroma_step=step, frame_stride=stride,
                     base=base_pad)


def unpadded(buf, fields, n, h, w, layout):
    """The packed frames in `layout` holding the samples a padded buffer describes."""
    st, step = fields["frame_stride"], fields["chroma_step"]
    Y = np.empty((n, h, w), np.uint8)
    U = np.empty((n, h // 2, w // 2), np.uint8)
    V = np.empty_like(U)
    for f in range(n):
        fr = buf[fields["base"] + f * st:]
        Y[f] = np.lib.stride_tricks.as_strided(fr, (h, w), (fields["pitch"], 1))
        U[f] = np.lib.stride_tricks.as_strided(fr[fields["u_offset"]:], (h // 2, w // 2), (fields["chroma_pitch"], step))
        V[f] = np.lib.stride_tricks.as_strided(fr[fields["v_offset"]:], (h // 2, w // 2), (fields["chroma_pitch"], step))
    return pack(Y, U, V, layout)


def picture_mask(fields, n, h, w, size):
    """bool [size]: the bytes of a padded buffer that belong to the picture (every other byte is pad)."""
    m = np.zeros(size, bool)
    st, step = fields["frame_stride"], fields["chroma_step"]
    for f in range(n):
        fr = m[fields["base"] + f * st:]
        np.lib.stride_tricks.as_strided(fr, (h, w), (fields["pitch"], 1))[...] = True
        for off in (fields["u_offset"], fields["v_offset"]):
            np.lib.stride_tricks.as_strided(fr[off:], (h // 2, w // 2), (fields["chroma_pitch"], step))[...] = True
    return m

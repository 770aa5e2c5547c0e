"""numpy restatement of the NV12 frame format (include/vdmi.h at vd_nv12): the integer colour
conversion, a test-only inverse, and the plane-wise pixelation built on oracle/mosaic.py with
per-box levels, that the library must match to the bit. A frame is uint8 [rows, w]: H luma rows
(H = 2 * rows / 3 >= h, the padded height) followed by H / 2 chroma rows of interleaved U, V."""
import numpy as np

import cells_ref
from oracle import mosaic as omosaic

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}

# (yoff, cy, crv, cgu, cgv, cbu): the table of include/vdmi.h
COEF = {
    ("bt601", "limited"): (16, 298, 409, -100, -208, 516),
    ("bt709", "limited"): (16, 298, 459, -55, -136, 541),
    ("bt601", "full"): (0, 256, 359, -88, -183, 454),
    ("bt709", "full"): (0, 256, 403, -48, -120, 475),
}


def real_coefficients(matrix, rng):
    """(yoff, cy, crv, cgu, cgv, cbu) as real numbers times 256: Y'CbCr -> R'G'B' for (Kr, Kb) with
    the 255/219 luma and 255/224 chroma excursions in limited range."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if rng == "limited" else (1.0, 1.0)
    return (16 if rng == "limited" else 0, 256 * sy, 256 * sc * 2 * (1 - kr), -256 * sc * 2 * (1 - kb) * kb / kg,
            -256 * sc * 2 * (1 - kr) * kr / kg, 256 * sc * 2 * (1 - kb))


def convert(Y, U, V, matrix="bt709", rng="limited"):
    """C(Y, U, V) on integer arrays -> uint8 [..., 3]."""
    yoff, cy, crv, cgu, cgv, cbu = COEF[(matrix, rng)]
    Y, U, V = (np.asarray(a, np.int32) for a in (Y, U, V))   # every term below stays under 2^18
    t = cy * (Y - yoff) + 128
    u, v = U - 128, V - 128
    rgb = np.stack([(t + crv * v) >> 8, (t + cgu * u + cgv * v) >> 8, (t + cbu * u) >> 8], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def planes(frame, height=None):
    """(Y [h, w], UV [h/2, w/2, 2]) as views of one frame [rows, w]."""
    rows, w = frame.shape
    assert rows % 3 == 0 and w % 2 == 0
    H = rows // 3 * 2
    h = H if height is None else height
    assert h % 2 == 0 and h <= H
    return frame[:h], frame[H:H + h // 2].reshape(h // 2, w // 2, 2)


def to_rgb(frames, matrix="bt709", rng="limited", height=None):
    """rgb(y, x) = C(Y(y, x), U(y, x), V(y, x)) with nearest chroma: [n, rows, w] -> [n, h, w, 3]."""
    frames = np.asarray(frames)
    out = []
    for f in (frames if frames.ndim == 3 else frames[None]):
        Y, UV = planes(f, height)
        up = UV.repeat(2, axis=0).repeat(2, axis=1)
        out.append(convert(Y, up[..., 0], up[..., 1], matrix, rng))
    return np.stack(out)


def from_rgb(rgb, matrix="bt709", rng="limited"):
    """Test-only inverse: [n, h, w, 3] -> packed NV12 [n, 3h/2, w]; real-valued forward matrix,
    chroma averaged over each 2 x 2 block, rounded and clamped."""
    rgb = np.asarray(rgb, np.float64)
    n, h, w, _ = rgb.shape
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y = kr * rgb[..., 0] + kg * rgb[..., 1] + kb * rgb[..., 2]
    cb = (rgb[..., 2] - y) / (2 * (1 - kb))
    cr = (rgb[..., 0] - y) / (2 * (1 - kr))
    sy, sc, yoff = (219.0 / 255.0, 224.0 / 255.0, 16.0) if rng == "limited" else (1.0, 1.0, 0.0)
    pool = lambda a: a.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))
    out = np.empty((n, h * 3 // 2, w), np.uint8)
    out[:, :h] = np.clip(np.rint(y * sy + yoff), 0, 255)
    uv = out[:, h:].reshape(n, h // 2, w // 2, 2)
    uv[..., 0] = np.clip(np.rint(pool(cb) * sc + 128), 0, 255)
    uv[..., 1] = np.clip(np.rint(pool(cr) * sc + 128), 0, 255)
    return out


def clip(box, h, w):
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, y1, x2, y2 = max(0, x1), max(0, y1), min(w, x2), min(h, y2)
    return (x1, y1, x2, y2) if x2 > x1 and y2 > y1 else None


def chroma_box(c):
    """cc of a clipped luma box c: every chroma sample that colours a pixel of c."""
    return (c[0] >> 1, c[1] >> 1, (c[2] + 1) >> 1, (c[3] + 1) >> 1)


def mosaic(frame, boxes, level=8, cells=0, height=None):
    """The pixelated frame: per box b, in list order, the luma plane takes oracle.mosaic's mosaic
    of clip(b) at L(b) and the chroma plane that of cc at (L(b) + 1) >> 1. Bytes outside the two
    planes' [0, w) x rows (pad rows of a padded height) are copied unchanged."""
    out = np.array(frame, copy=True)
    Y, UV = planes(out, height)
    h, w = Y.shape
    for b in boxes:
        c = clip(b, h, w)
        if c is None:
            continue
        L = cells_ref.box_level(b, level, cells)
        Y[:] = omosaic.mosaic_frame(Y, [c], L)
        UV[:] = omosaic.mosaic_frame(UV, [chroma_box(c)], (L + 1) >> 1)
    return out

"""numpy restatement of the Gaussian-blur mode (include/vdmi.h at vd_blur): the integer
definition the GPU path must match to the bit, a float64 version of the same blur, and the
sequential application of a box list (box j reads the output of box j-1)."""
import math

import numpy as np

KSIZE_MAX = 127


def sigma_of(k, sigma):
    """sigma <= 0: cv2's rule from the kernel size. The library takes sigma as a C float."""
    sigma = float(np.float32(sigma))
    return sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8


def weights_f64(k, sigma):
    """w_i = exp(-(i-r)^2 / (2 sigma^2)) / sum, Python floats (C doubles), summed in index order."""
    r, sg = k // 2, sigma_of(k, sigma)
    w = [math.exp(-((i - r) * (i - r)) / (2.0 * sg * sg)) for i in range(k)]
    s = 0.0
    for v in w:
        s += v
    return [v / s for v in w]


def weights_q20(k, sigma):
    """q_i = floor(w_i * 2^20 + 0.5) for i != r; the centre tap takes the remainder of 2^20."""
    r = k // 2
    q = [int(math.floor(v * 1048576.0 + 0.5)) for v in weights_f64(k, sigma)]
    q[r] = (1 << 20) - (sum(q) - q[r])
    return np.asarray(q, np.uint32)


def refl(p, n):
    """OpenCV borderInterpolate, BORDER_REFLECT_101, any number of reflections."""
    if n == 1:
        return 0
    m = 2 * (n - 1)
    p = abs(p) % m
    return m - p if p >= n else p


def _taps(n, k):
    """[n][k] source index of tap i at position x."""
    if n == 1:
        return np.zeros((1, k), np.int64)
    m = 2 * (n - 1)
    p = np.abs(np.arange(n)[:, None] + np.arange(k)[None, :] - k // 2) % m      # refl(), vectorised
    return np.where(p >= n, m - p, p).astype(np.int64)


def blur_region_int(region, q, stats=None):
    """uint8 [bh, bw, c] -> uint8, the fixed-point definition. stats (a dict) receives the
    largest horizontal and vertical sums seen ('t', 's')."""
    region = np.asarray(region, np.uint8)
    bh, bw = region.shape[:2]
    k = len(q)
    q64 = np.asarray(q, np.uint64)
    px = region.astype(np.uint64)
    tx = _taps(bw, k)
    t = np.zeros(px.shape, np.uint64)
    for i in range(k):
        t += q64[i] * px[:, tx[:, i]]
    h = (t + np.uint64(1 << 15)) >> np.uint64(16)
    ty = _taps(bh, k)
    s = np.zeros(px.shape, np.uint64)
    for i in range(k):
        s += q64[i] * h[ty[:, i]]
    out = (s + np.uint64(1 << 23)) >> np.uint64(24)
    if stats is not None:
        stats["t"] = max(stats.get("t", 0), int(t.max()))
        stats["s"] = max(stats.get("s", 0), int(s.max()))
        stats["out"] = max(stats.get("out", 0), int(out.max()))
    return out.astype(np.uint8)


def blur_region_f64(region, k, sigma):
    """The real-valued separable Gaussian of the region alone (float64, not rounded)."""
    px = np.asarray(region, np.float64)
    bh, bw = px.shape[:2]
    w = weights_f64(k, sigma)
    tx, ty = _taps(bw, k), _taps(bh, k)
    t = np.zeros(px.shape, np.float64)
    for i in range(k):
        t += w[i] * px[:, tx[:, i]]
    s = np.zeros(px.shape, np.float64)
    for i in range(k):
        s += w[i] * t[ty[:, i]]
    return s


def clip_box(box, h, w):
    """combine_detect.py:145-151: the clipped box, or None when it is empty."""
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, y1, x2, y2 = max(0, x1), max(0, y1), min(w, x2), min(h, y2)
    return (x1, y1, x2, y2) if x2 > x1 and y2 > y1 else None


def blur_frame(img, boxes, k, sigma, q=None, exact=False):
    """A new array: every box, in order, clipped and replaced by the blur of the clipped
    region of the CURRENT image. q: the tap weights (default: weights_q20(k, sigma));
    exact: the float64 blur rounded half up instead of the integer definition."""
    out = np.array(img, np.uint8, copy=True)
    h, w = out.shape[:2]
    if q is None and not exact:
        q = weights_q20(k, sigma)
    for box in boxes:
        c = clip_box(box, h, w)
        if c is None:
            continue
        x1, y1, x2, y2 = c
        reg = out[y1:y2, x1:x2].copy()
        if exact:
            out[y1:y2, x1:x2] = np.floor(blur_region_f64(reg, k, sigma) + 0.5).clip(0, 255).astype(np.uint8)
        else:
            out[y1:y2, x1:x2] = blur_region_int(reg, q)
    return out

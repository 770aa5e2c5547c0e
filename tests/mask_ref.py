"""numpy restatement of mask shaping (include/vdmi.h at vd_mask): grow, the ellipse predicate
in Python ints, and the composite over a rectangular pass (box j reads the output of box j-1)
that the GPU path must match to the bit."""
import numpy as np

GROW_MAX = 200
COORD_MAX = 1 << 30
SIDE_MAX = 32768


def grow(box, g):
    """grow(b, g): an empty box stays as it is; otherwise each side moves out by the ceiling of
    half the growth and every coordinate is clamped to [-2^30, 2^30]."""
    x1, y1, x2, y2 = (int(v) for v in box)
    W, H = x2 - x1, y2 - y1
    if W <= 0 or H <= 0:
        return (x1, y1, x2, y2)
    gx, gy = (W * g + 199) // 200, (H * g + 199) // 200
    c = lambda v: max(-COORD_MAX, min(COORD_MAX, v))
    return (c(x1 - gx), c(y1 - gy), c(x2 + gx), c(y2 + gy))


def grow_list(boxes, g):
    return [grow(b, g) for b in boxes]


def clip(box, h, w):
    """combine_detect.py:145-151: the clipped box, or None when it is empty."""
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, y1, x2, y2 = max(0, x1), max(0, y1), min(w, x2), min(h, y2)
    return (x1, y1, x2, y2) if x2 > x1 and y2 > y1 else None


def inside(box, x, y):
    """The predicate for pixel (x, y) of the (grown, unclipped) box's clipped rectangle."""
    x1, y1, x2, y2 = (int(v) for v in box)
    W, H = x2 - x1, y2 - y1
    if W > SIDE_MAX or H > SIDE_MAX:
        return True
    dx, dy = 2 * x + 1 - (x1 + x2), 2 * y + 1 - (y1 + y2)
    return dx * dx * H * H + dy * dy * W * W <= W * W * H * H


def ellipse_mask(h, w, box):
    """bool [h][w]: E of the box -- the pixels of its clipped rectangle inside its ellipse."""
    m = np.zeros((h, w), bool)
    c = clip(box, h, w)
    if c is None:
        return m
    for y in range(c[1], c[3]):
        for x in range(c[0], c[2]):
            m[y, x] = inside(box, x, y)
    return m


def shaped_frame(img, boxes, shape, g, rect_fn):
    """The frame a context with mask (shape, g) produces: rect_fn(img, grown boxes) is the
    rectangular pass R (oracle.mosaic.mosaic_frame or gaussian_ref.blur_frame with their
    parameters bound); under "ellipse" out = R inside some box's ellipse, img elsewhere."""
    grown = grow_list(boxes, g)
    R = rect_fn(img, grown)
    if shape == "rect":
        return R
    assert shape == "ellipse"
    h, w = img.shape[:2]
    hidden = np.zeros((h, w), bool)
    for b in grown:
        hidden |= ellipse_mask(h, w, b)
    out = np.array(img, copy=True)
    out[hidden] = R[hidden]
    return out


# The edge cases test_gpu_mask.py runs on a 72 x 100 frame (h, w) and test_mask_ref.py checks the
# coverage guarantee on: boxes clipped by each frame edge so far that the centre of the grown
# box's ellipse lies off the frame, a box wholly outside, an empty and an inverted box.
EDGE_HW = (72, 100)
EDGE_BOXES = [(-30, 20, 12, 45), (88, 18, 140, 40), (40, -30, 70, 9), (45, 62, 80, 130),
              (-25, -20, 9, 11), (200, 200, 240, 230), (60, 30, 60, 50), (70, 50, 65, 58)]

"""Drop-in ``mosaic_rectangle_region_single`` (combine_detect.py:138-161) and the
batched form the MI355X path actually uses (one HIP launch per frame batch,
boxes applied in list order exactly as combine_detect.py:246-249), and their
Gaussian-blur counterparts ``gaussian_blur_region_single`` / ``blur_frames``."""
import threading

import numpy as np

from .context import Context

_ctxs = {}
_ctx_lock = threading.Lock()


def _default_ctx(mask="rect", mask_grow=0, cells=0):
    """One shared context per mask and cells setting (the settings are a context's state, and
    the callers are threads)."""
    key = (mask, int(mask_grow), int(cells))
    with _ctx_lock:
        if key not in _ctxs:
            _ctxs[key] = Context(max_batch=64, mask=mask, mask_grow=mask_grow, cells=cells)
        return _ctxs[key]


def mosaic_rectangle_region_single(img, x1, y1, x2, y2, mosaic_level=8):
    """Same signature/result as the reference: returns a new array with the clipped
    box pixelated by an INTER_NEAREST down/up resize of factor ``mosaic_level``."""
    a = np.ascontiguousarray(img, np.uint8)
    box = np.asarray([[[int(x1), int(y1), int(x2), int(y2)]]], np.int32)
    return _default_ctx().mosaic(a[None], box, np.ones(1, np.int32), level=mosaic_level)[0]


def _box_arrays(n, boxes):
    """Per-frame box lists -> (int32 [n][cap][4], int32 counts [n])."""
    cap = max(1, max((len(b) for b in boxes), default=1))
    xy = np.zeros((n, cap, 4), np.int32)
    cnt = np.zeros(n, np.int32)
    for i, bl in enumerate(boxes):
        cnt[i] = len(bl)
        if len(bl):
            xy[i, :len(bl)] = np.asarray(bl, np.int64).clip(-2**31, 2**31 - 1)
    return xy, cnt


def mosaic_frames(frames, boxes, mosaic_level=8, ctx=None, mask="rect", mask_grow=0, cells=0):
    """frames: uint8 [n,h,w,3]; boxes: list (per frame) of (x1,y1,x2,y2) int tuples.
    Equivalent to applying mosaic_rectangle_region_single per box in order. mask /
    mask_grow: the mask shaping (Context(mask=..., mask_grow=...)) of the shared context
    used when no ctx is given; a given ctx applies its own. cells: box-scaled strength
    (Context(cells=...)) of that shared context: the level follows each box, never below
    mosaic_level."""
    frames = np.ascontiguousarray(frames, np.uint8)
    xy, cnt = _box_arrays(frames.shape[0], boxes)
    return (ctx or _default_ctx(mask, mask_grow, cells)).mosaic(frames, xy, cnt, level=mosaic_level)


def smooth_frames(frames, boxes, mosaic_level=8, cells=16, ctx=None, mask="rect", mask_grow=0):
    """frames: uint8 [n,h,w,3]; boxes: list (per frame) of (x1,y1,x2,y2) int tuples. The scaled
    smooth blur (vd_smooth) of every box: at most `cells` cells along its longer side, their
    means interpolated across the box; where boxes overlap the strongest wins. mask / mask_grow
    as in mosaic_frames."""
    frames = np.ascontiguousarray(frames, np.uint8)
    xy, cnt = _box_arrays(frames.shape[0], boxes)
    return (ctx or _default_ctx(mask, mask_grow)).smooth(frames, xy, cnt, level=mosaic_level, cells=cells)


def gaussian_blur_region_single(img, x1, y1, x2, y2, ksize=31, sigma=0.0):
    """The Gaussian counterpart of mosaic_rectangle_region_single: returns a new array
    with the clipped box replaced by GaussianBlur(region, (ksize, ksize), sigma) of the
    region alone (BORDER_REFLECT_101 at the clipped box's edges), in the library's
    fixed-point definition (include/vdmi.h at vd_blur)."""
    a = np.ascontiguousarray(img, np.uint8)
    box = np.asarray([[[int(x1), int(y1), int(x2), int(y2)]]], np.int32)
    return _default_ctx().blur(a[None], box, np.ones(1, np.int32), ksize=ksize, sigma=sigma)[0]


def blur_frames(frames, boxes, ksize=31, sigma=0.0, ctx=None, mask="rect", mask_grow=0):
    """frames: uint8 [n,h,w,3]; boxes: list (per frame) of (x1,y1,x2,y2) int tuples.
    Equivalent to applying gaussian_blur_region_single per box in order; mask / mask_grow
    as in mosaic_frames."""
    frames = np.ascontiguousarray(frames, np.uint8)
    xy, cnt = _box_arrays(frames.shape[0], boxes)
    return (ctx or _default_ctx(mask, mask_grow)).blur(frames, xy, cnt, ksize=ksize, sigma=sigma)

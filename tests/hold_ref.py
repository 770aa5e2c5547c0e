"""Box hold, the definition (include/vdmi.h "box hold") in numpy / Python ints.

The checker of tests/test_hold_ref.py and tests/test_gpu_hold.py; it never imports vdmi.

Frame t's blur list is B_t = D_t ++ H_t. D_t: the frame's own boxes. H_t: for age
a = 1..K (t - a >= 0), in the order of D_{t-a}, every box of D_{t-a} that is non-empty
after clipping to [0, w] x [0, h] and matches no box of D_t, .., D_{t-a+1}; two non-empty
clipped boxes match iff 100 * inter >= P * union (integers, inclusive). Held boxes are
appended unclipped, as stored.
"""
import numpy as np


def clip_box(b, h, w):
    """combine_detect.py:145-151: the clipped box, or None when nothing is left."""
    x1, y1, x2, y2 = max(0, int(b[0])), max(0, int(b[1])), min(int(w), int(b[2])), min(int(h), int(b[3]))
    if not (x2 > x1 and y2 > y1):
        return None
    return x1, y1, x2, y2


def match(a, b, P):
    """a, b: clipped boxes or None."""
    if a is None or b is None:
        return False
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return False
    inter = iw * ih                       # Python ints: no overflow
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return 100 * inter >= P * union


def _as_list(d):
    return [tuple(int(v) for v in b) for b in np.asarray(d, np.int64).reshape(-1, 4)]


def _clipped(boxes, h, w):
    """int64 [m][4]: the non-empty clipped boxes of a list."""
    c = [clip_box(b, h, w) for b in boxes]
    return np.asarray([x for x in c if x is not None], np.int64).reshape(-1, 4)


def _matches_any(c, seen, P):
    """match(c, s, P) for any row s of `seen` (int64 [m][4], non-empty clipped boxes)."""
    if len(seen) == 0:
        return False
    iw = np.minimum(c[2], seen[:, 2]) - np.maximum(c[0], seen[:, 0])
    ih = np.minimum(c[3], seen[:, 3]) - np.maximum(c[1], seen[:, 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    union = (c[2] - c[0]) * (c[3] - c[1]) + (seen[:, 2] - seen[:, 0]) * (seen[:, 3] - seen[:, 1]) - inter
    return bool(np.any((inter > 0) & (100 * inter >= P * union)))


def hold_lists(seq, h, w, K, P, history=None):
    """seq: per frame, its own boxes D_t (anything reshapeable to [k][4]); history: the D
    lists of the frames before seq[0], oldest first (what an earlier call returned), or None.
    -> (B, H, ages, history): per frame the blur list B_t, the held boxes H_t and their
    ages (lists of int 4-tuples / ints), and the history after the call: the last K lists."""
    past = [list(d) for d in (history or [])][-K:] if K > 0 else []
    B, H, ages = [], [], []
    for d in seq:
        d = _as_list(d)
        frames = past + [d]               # frames[-1] = D_t, frames[-1 - a] = D_{t-a}
        seen = _clipped(d, h, w)
        ht, at = [], []
        for a in range(1, K + 1):
            if a >= len(frames):
                break
            older = frames[-1 - a]
            for b in older:
                c = clip_box(b, h, w)
                if c is not None and not _matches_any(c, seen, P):
                    ht.append(b)
                    at.append(a)
            # candidates of the next age are also compared against this frame
            seen = np.concatenate([seen, _clipped(older, h, w)])
        B.append(d + ht)
        H.append(ht)
        ages.append(at)
        past = (past + [d])[-K:] if K > 0 else []
    return B, H, ages, past

"""Box hold with the linear motion model, the definition (include/vdmi.h "box hold",
DESIGN.md) in Python ints, on top of hold_ref.hold_lists.

The checker of tests/test_hold_motion_ref.py and tests/test_gpu_hold_motion.py; it never
imports vdmi.

Membership, order and ages of H_t are hold_ref's. A box b = D_{t-a}[i] held with age a, with
c = clip(b), looks in D_{t-a-1} for its predecessor: among the boxes p with non-empty clip(p)
and match(c, clip(p)) under the same P, the one of greatest IoU (p1 beats p2 iff
inter1 * union2 > inter2 * union1), the lowest list index on ties. With one, v = c - clip(p)
and q = c + a * v per coordinate, and the held box is the hull of b as stored and q:
(min(b.x1, q.x1), min(b.y1, q.y1), max(b.x2, q.x2), max(b.y2, q.y2)). Without one (no such
frame, or nothing matches) the held box is b.
"""
import numpy as np

import hold_ref as hr


def iou_terms(a, b):
    """(inter, union) of two non-empty clipped boxes; inter 0 when they share no area."""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0, 1
    inter = iw * ih
    return inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter


def clipped_rows(frame, h, w):
    """int64 [m][4]: every box of the list clipped, in list order; (0, 0, 0, 0), which shares
    no area with anything, where nothing is left."""
    return np.asarray([hr.clip_box(p, h, w) or (0, 0, 0, 0) for p in frame], np.int64).reshape(-1, 4)


def predecessor(c, frame, h, w, P, rows=None):
    """The clipped predecessor of the clipped box c in the list `frame`, or None. rows:
    clipped_rows(frame, h, w) if the caller has them (only narrows the search: the boxes that
    share area with c; the comparison itself is on Python ints)."""
    if rows is None:
        rows = clipped_rows(frame, h, w)
    if len(rows) == 0:
        return None
    near = ((rows[:, 0] < c[2]) & (rows[:, 2] > c[0]) & (rows[:, 1] < c[3]) & (rows[:, 3] > c[1])).nonzero()[0]
    best, bi, bu = None, 0, 1
    for i in near:                            # ascending list index
        cp = tuple(int(v) for v in rows[i])
        if not hr.match(c, cp, P):
            continue
        inter, union = iou_terms(c, cp)
        if inter * bu > bi * union:           # strictly greater: ties keep the lowest index
            best, bi, bu = cp, inter, union
    return best


def moved(b, a, frame, h, w, P, rows=None):
    """The held form of b (stored, non-empty after clipping) at age a; frame: D of the frame
    before the sighting, or None when there is no such frame."""
    c = hr.clip_box(b, h, w)
    p = predecessor(c, frame, h, w, P, rows) if frame is not None else None
    if p is None:
        return tuple(b)
    q = [c[k] + a * (c[k] - p[k]) for k in range(4)]
    return min(b[0], q[0]), min(b[1], q[1]), max(b[2], q[2]), max(b[3], q[3])


def hold_motion_lists(seq, h, w, K, P, history=None):
    """As hold_ref.hold_lists, with the held boxes moved. history: the D lists of the frames
    before seq[0], oldest first (what an earlier call returned: up to K + 1 lists), or None.
    -> (B, H, ages, history, stored): blur lists, held boxes (moved), ages, the history after
    the call (the last K + 1 lists) and the held boxes as stored (hold_ref's H)."""
    past = [hr._as_list(d) for d in (history or [])]
    past = past[-(K + 1):] if K > 0 else []
    seq = [hr._as_list(d) for d in seq]
    _, H0, ages, _ = hr.hold_lists(seq, h, w, K, P, past[-K:] if K > 0 else None)
    frames = past + seq
    rows = [clipped_rows(d, h, w) for d in frames]
    B, H = [], []
    for t, d in enumerate(seq):
        ht = []
        for b, a in zip(H0[t], ages[t]):
            i = len(past) + t - a - 1         # the frame before the sighting
            ht.append(moved(b, a, frames[i], h, w, P, rows[i]) if i >= 0 else tuple(b))
        H.append(ht)
        B.append(d + ht)
    return B, H, ages, (frames[-(K + 1):] if K > 0 else []), H0

"""Rescue on tiled nets (include/vdmi.h at vd_rescue_tiles), the definition in numpy: the cross-tile merge
of tests/tiles_ref.py / tests/plate_tiles_ref.py over the per-input lists at the low threshold, the cut
with the net's own comparison, and the rescue of tests/rescue_ref.py over the two parts. Nothing new is
computed here: the three references are composed. It never imports vdmi."""
import numpy as np

import plate_tiles_ref as ptr
import rescue_ref as rr
import tiles_ref as tr

F32 = np.float32


def strong_mask(score, thr, plates):
    """The net's comparison: a face at exactly `confidence` is strong, a plate at exactly `plate_conf` weak."""
    score = np.asarray(score, F32)
    return score > F32(thr) if plates else score >= F32(thr)


def merge_low(lists, origins, A, iou, plates):
    """The merge of one frame's T lists, whatever threshold they were made at. -> merge_frame's tuple
    (xyxy, xyxy_f, score, label, src)."""
    return ptr.merge_frame(lists, origins, iou) if plates else tr.merge_frame(lists, origins, A, iou)


def cut(merged, thr, plates):
    """-> the number of strong boxes of a merged list. They must be a prefix of it (descending scores)."""
    m = strong_mask(merged[2], thr, plates)
    k = int(m.sum())
    assert m[:k].all() and not m[k:].any(), "the strong boxes are not a prefix of the merged list"
    return k


def part(merged, lo, hi):
    """Rows [lo, hi) of a merged list, src included."""
    return tuple(x[lo:hi] for x in merged[:4]) + (merged[4][lo:hi],)


def strong_prefixes(lists, thr, plates):
    """Each input's list cut at the net's threshold (its strong boxes are a prefix of it)."""
    out = []
    for xf, sc, lab in lists:
        m = strong_mask(sc, thr, plates)
        k = int(m.sum())
        assert m[:k].all() and not m[k:].any(), "an input list is not in descending score order"
        out.append((xf[:k], sc[:k], lab[:k] if lab is not None else None))
    return out


def split_frame(lists, origins, A, iou, thr, plates):
    """-> (D, W, merged): the strong prefix and the weak rest of the merged list at low, as merge_frame tuples."""
    merged = merge_low(lists, origins, A, iou, plates)
    k = cut(merged, thr, plates)
    return part(merged, 0, k), part(merged, k, len(merged[2])), merged


def rescue_stream(strong, weak, h, w, W, S, P, history=None):
    """rescue_ref.rescue_lists on per-frame int boxes D_t (faces then plates) and W_t (weak faces then weak
    plates), both as [k][4] arrays. -> (E, since, R, widx, history)."""
    return rr.rescue_lists([np.asarray(d).reshape(-1, 4).tolist() for d in strong],
                           [np.asarray(x).reshape(-1, 4).tolist() for x in weak], h, w, W, S, P, history)


# ---- generated per-input lists (the CPU property tests and the GPU kernel cases share them) ----
FACE_THR, PLATE_THR = 0.5, 0.5
# a small set that holds the threshold itself: a face at 0.5 is strong, a plate at 0.5 is weak; few values,
# so scores repeat across inputs and inside them
SCORES = (0.9, 0.75, 0.5, 0.45, 0.3, 0.2)


class Lists:
    """n * T rows of at most cap boxes, the fields of a HostBoxes (frame f's input t at row f * T + t)."""

    def __init__(self, rows, cap):
        self.n, self.cap = rows, cap
        self.count = np.zeros(rows, np.int32)
        self.xyxy = np.zeros((rows, cap, 4), np.int32)
        self.xyxy_f = np.zeros((rows, cap, 4), F32)
        self.score = np.zeros((rows, cap), F32)
        self.label = np.zeros((rows, cap), np.int32)

    def frame_lists(self, f, T):
        out = []
        for t in range(T):
            r = f * T + t
            k = min(int(self.count[r]), self.cap)
            out.append((self.xyxy_f[r, :k], self.score[r, :k], self.label[r, :k]))
        return out


def random_lists(seed, n, rects, cap, plates=False, scores=SCORES, nc=3, empty=(), objects=None):
    """Per frame `objects` (default: 5 * cap, which fills the (2, 2) tiles) boxes of 8..40 pixels somewhere in the frame; input t lists those that
    lie inside its rectangle (each with probability 0.85, at most cap), moved by up to a pixel, relative to the
    rectangle, each with a score of its own from `scores`, in descending score order. So one object is strong in
    one input and weak in another, and overlapping neighbours make the sweep work. empty: inputs t left empty.
    label: an anchor index below 1000 (faces) or a class below nc (plates), the object's in every input."""
    rng = np.random.default_rng(seed)
    T = len(rects)
    W, H = int(rects[0][2]), int(rects[0][3])
    out = Lists(n * T, cap)
    for f in range(n):
        K = 5 * cap if objects is None else objects
        wh = rng.uniform(8, 40, (K, 2))
        xy = rng.uniform(0, 1, (K, 2)) * (np.asarray([W, H]) - wh)
        lab = rng.integers(0, nc if plates else 1000, K)
        for t in range(T):
            if t in empty:
                continue
            x0, y0, tw, th = (int(v) for v in rects[t])
            inside = (xy[:, 0] >= x0) & (xy[:, 1] >= y0) & (xy[:, 0] + wh[:, 0] <= x0 + tw) & (xy[:, 1] + wh[:, 1] <= y0 + th)
            idx = np.flatnonzero(inside & (rng.random(K) < 0.85))[:cap]
            sc = np.asarray(rng.choice(scores, len(idx)), F32)
            order = np.argsort(-sc, kind="stable")
            idx, sc = idx[order], sc[order]
            jit = rng.uniform(-1, 1, (len(idx), 4))
            box = np.concatenate([xy[idx], xy[idx] + wh[idx]], 1) + jit - np.asarray([x0, y0, x0, y0])
            r = f * T + t
            out.count[r] = len(idx)
            out.xyxy_f[r, :len(idx)] = box.astype(F32)
            out.xyxy[r, :len(idx)] = box.astype(np.int32)
            out.score[r, :len(idx)] = sc
            out.label[r, :len(idx)] = lab[idx]
    return out


def suppressed_by_strong_of_another_input(lists, origins, merged, k, iou, plates):
    """How many weak input boxes are missing from the merged list because a kept STRONG box (merged rows
    [0, k)) of another input suppresses them."""
    kept = set(merged[4])
    hits = 0
    sbox = np.asarray(merged[1][:k], F32).reshape(-1, 4)
    sarea = ((sbox[:, 2] - sbox[:, 0]).astype(F32) * (sbox[:, 3] - sbox[:, 1]).astype(F32)).astype(F32)
    slab = np.asarray(merged[3][:k])
    st = np.asarray([s[0] for s in merged[4][:k]])
    for t, (xf, sc, lab) in enumerate(lists):
        ox, oy = F32(origins[t][0]), F32(origins[t][1])
        for pos in range(len(sc)):
            if (t, pos) in kept or strong_mask(sc[pos], PLATE_THR if plates else FACE_THR, plates):
                continue
            b = np.asarray(xf[pos], F32)
            if t:
                b = np.asarray([b[0] + ox, b[1] + oy, b[2] + ox, b[3] + oy], F32)
            a = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
            m = tr.iou_gt(b, a, sbox, sarea, iou) & (st != t)
            if plates:
                m &= slab == int(lab[pos])
            hits += bool(m.any())
    return hits

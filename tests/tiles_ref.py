"""numpy reference of tiled detection (include/vdmi.h at vd_tiles): the tile geometry and the
cross-tile merge, written from the definition (float32 ops one rounding at a time, in the
stated order), not from the kernel."""
import numpy as np

F32 = np.float32


def _axis(L, K, O):
    t = min(L, (L * (100 + O) + 100 * K - 1) // (100 * K))
    return t, [0 if K == 1 else (k * (L - t)) // (K - 1) for k in range(K)]


def tile_rects(h, w, rows, cols, overlap):
    """int32 [1 + rows * cols][4] of (x, y, w, h): row 0 the frame, row 1 + r * cols + c tile (r, c)."""
    th, ys = _axis(h, rows, overlap)
    tw, xs = _axis(w, cols, overlap)
    out = [(0, 0, w, h)]
    for r in range(rows):
        for c in range(cols):
            out.append((xs[c], ys[r], tw, th))
    return np.asarray(out, np.int32)


def trunc_i32(v):
    """int(x) of a Python float, clamped to int32 (NaN -> 0)."""
    v = F32(v)
    if v != v:
        return 0
    if v >= F32(2147483520.0):
        return 2147483647
    if v <= F32(-2147483648.0):
        return -2147483648
    return int(v)


def iou_gt(a, aa, B, aB, thr):
    """torchvision nms' test of box a (area aa) against the rows of B (areas aB): float32 ops one
    rounding at a time, the quotient compared against a double. -> bool [len(B)]."""
    xx1, yy1 = np.maximum(a[0], B[:, 0]), np.maximum(a[1], B[:, 1])
    xx2, yy2 = np.minimum(a[2], B[:, 2]), np.minimum(a[3], B[:, 3])
    w, h = (xx2 - xx1).astype(F32), (yy2 - yy1).astype(F32)
    w = np.where(w > 0, w, F32(0))
    h = np.where(h > 0, h, F32(0))
    inter = (w * h).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ovr = (inter / ((aa + aB).astype(F32) - inter).astype(F32)).astype(F32)
    return ovr.astype(np.float64) > thr


def merge_frame(lists, origins, A, iou):
    """lists: T tuples (xyxy_f [k][4] f32, score [k] f32, label [k] int or None), boxes relative
    to their rectangle; origins: T (x0, y0). -> (xyxy int32 [m][4], xyxy_f f32 [m][4], score f32
    [m], label int32 [m], sources [m] of (t, pos)) in merged order."""
    cand = []
    for t, (xf, sc, lab) in enumerate(lists):
        xf = np.asarray(xf, F32).reshape(-1, 4)
        sc = np.asarray(sc, F32).reshape(-1)
        ox, oy = F32(origins[t][0]), F32(origins[t][1])
        for pos in range(len(sc)):
            b = xf[pos]
            if t:   # one float32 add per coordinate; input 0 is left as it is
                b = np.asarray([b[0] + ox, b[1] + oy, b[2] + ox, b[3] + oy], F32)
            bits = int(np.asarray(sc[pos], F32).view(np.uint32))
            cand.append(((0xFFFFFFFF - bits, t, pos), b, sc[pos], t * A + (int(lab[pos]) if lab is not None else 0)))
    cand.sort(key=lambda c: c[0])
    box = np.asarray([c[1] for c in cand], F32).reshape(-1, 4)
    area = ((box[:, 2] - box[:, 0]).astype(F32) * (box[:, 3] - box[:, 1]).astype(F32)).astype(F32)
    dead = np.zeros(len(cand), bool)
    kept = []
    for i in range(len(cand)):         # greedy, in order: a kept box suppresses what follows it
        if dead[i]:
            continue
        kept.append(i)
        dead[i + 1:] |= iou_gt(box[i], area[i], box[i + 1:], area[i + 1:], iou)
    m = len(kept)
    xyxy_f = np.zeros((m, 4), F32)
    xyxy = np.zeros((m, 4), np.int32)
    score = np.zeros(m, F32)
    label = np.zeros(m, np.int32)
    src = []
    for o, j in enumerate(kept):
        xyxy_f[o] = cand[j][1]
        xyxy[o] = [trunc_i32(v) for v in cand[j][1]]
        score[o] = cand[j][2]
        label[o] = cand[j][3]
        src.append((cand[j][0][1], cand[j][0][2]))
    return xyxy, xyxy_f, score, label, src


def merge(boxes, n, rects, A, iou):
    """boxes: HostBoxes-like (count, xyxy_f, score, label, cap) of n * T rows; rects: tile_rects.
    -> list of n merge_frame results."""
    T = len(rects)
    out = []
    for f in range(n):
        lists = []
        for t in range(T):
            r = f * T + t
            k = min(int(boxes.count[r]), boxes.cap)
            lists.append((boxes.xyxy_f[r, :k], boxes.score[r, :k], boxes.label[r, :k]))
        out.append(merge_frame(lists, [(int(q[0]), int(q[1])) for q in rects], A, iou))
    return out

"""numpy reference of the tiled plate merge (include/vdmi.h at vd_tiles_nets), written from the
definition (float32 ops one rounding at a time, in the stated order), not from the kernel:
  map    box i of input t > 0 moves by the tile's origin, one float32 add per coordinate;
  order  descending score (bit pattern), ties to the lower t, then to the lower list position;
  NMS    greedy over that order on the mapped boxes: a kept box a suppresses a later box b iff
         label(a) == label(b) and the float32 IoU, as a double, exceeds the threshold; no class
         offset is added;
  emit   the mapped box, its int(), the score, label = the class id. No cap."""
import numpy as np

from tiles_ref import F32, iou_gt, trunc_i32


def merge_frame(lists, origins, iou):
    """lists: T tuples (xyxy_f [k][4] f32, score [k] f32, label [k] int or None = class 0), boxes
    relative to their rectangle; origins: T (x0, y0). -> (xyxy int32 [m][4], xyxy_f f32 [m][4],
    score f32 [m], label int32 [m], sources [m] of (t, pos)) in merged order."""
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
            cand.append(((0xFFFFFFFF - bits, t, pos), b, sc[pos], int(lab[pos]) if lab is not None else 0))
    cand.sort(key=lambda c: c[0])
    box = np.asarray([c[1] for c in cand], F32).reshape(-1, 4)
    cls = np.asarray([c[3] for c in cand], np.int64)
    area = ((box[:, 2] - box[:, 0]).astype(F32) * (box[:, 3] - box[:, 1]).astype(F32)).astype(F32)
    dead = np.zeros(len(cand), bool)
    kept = []
    for i in range(len(cand)):         # greedy, in order: a kept box suppresses later boxes of its class
        if dead[i]:
            continue
        kept.append(i)
        dead[i + 1:] |= iou_gt(box[i], area[i], box[i + 1:], area[i + 1:], iou) & (cls[i + 1:] == cls[i])
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


def merge(boxes, n, rects, iou):
    """boxes: HostBoxes-like (count, xyxy_f, score, label, cap) of n * T rows, frame f's input t
    at row f * T + t; rects: tile_rects. -> list of n merge_frame results."""
    T = len(rects)
    out = []
    for f in range(n):
        lists = []
        for t in range(T):
            r = f * T + t
            k = min(int(boxes.count[r]), boxes.cap)
            lists.append((boxes.xyxy_f[r, :k], boxes.score[r, :k], boxes.label[r, :k]))
        out.append(merge_frame(lists, [(int(q[0]), int(q[1])) for q in rects], iou))
    return out

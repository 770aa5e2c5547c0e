"""Weak-detection rescue, the definition (include/vdmi.h at vd_rescue) in numpy int64 / Python ints.

The checker of tests/test_rescue_ref.py and tests/test_gpu_rescue.py; it never imports vdmi.

Per frame t: D_t the strong boxes (since = 0), W_t the weak boxes. For w in W_t with a non-empty
clip c, m(w) = min of since(e) + a over a = 1..W (t - a >= 0) and e in E_{t-a} whose clip
matches c (the box hold's clip and match); w is rescued iff such an e exists and m(w) <= S, and
then since(w) = m(w). R_t: the rescued boxes in W_t's order; E_t = D_t ++ R_t.
"""
import numpy as np

from hold_ref import _as_list, clip_box


def _clipped(boxes, h, w):
    """int64 [m][4] clipped boxes and bool [m]: non-empty (an empty box keeps a row of zeros)."""
    c = [clip_box(b, h, w) for b in boxes]
    ok = np.asarray([x is not None for x in c], bool)
    return np.asarray([x if x is not None else (0, 0, 0, 0) for x in c], np.int64).reshape(-1, 4), ok


def _best(c, refs, ok, since, P):
    """min of since over the non-empty rows of `refs` that match the clipped box c, or None.
    int64 throughout: exact for coordinates below 2^27 (100 * inter < 2^63)."""
    if len(refs) == 0:
        return None
    iw = np.minimum(c[2], refs[:, 2]) - np.maximum(c[0], refs[:, 0])
    ih = np.minimum(c[3], refs[:, 3]) - np.maximum(c[1], refs[:, 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    union = (c[2] - c[0]) * (c[3] - c[1]) + (refs[:, 2] - refs[:, 0]) * (refs[:, 3] - refs[:, 1]) - inter
    m = ok & (inter > 0) & (100 * inter >= P * union)
    return int(since[m].min()) if m.any() else None


def rescue_lists(strong, weak, h, w, W, S, P, history=None):
    """strong, weak: per frame, D_t and W_t (anything reshapeable to [k][4]; faces then plates).
    history: (E, since) pairs of the frames before frame 0, oldest first (what an earlier call
    returned), or None. -> (E, since, R, widx, history): per frame E_t and its since values,
    R_t, the indices into W_t of the rescued boxes, and the history after the call: the last W
    (E, since) pairs."""
    past = [(list(e), list(s)) for e, s in (history or [])][-W:]
    clipped = [_clipped(e, h, w) + (np.asarray(s, np.int64),) for e, s in past]
    E, SI, R, IDX = [], [], [], []
    for d, wk in zip(strong, weak):
        d, wk = _as_list(d), _as_list(wk)
        rt, st, it = [], [], []
        for i, b in enumerate(wk):
            c = clip_box(b, h, w)
            if c is None:
                continue
            best = None
            for a in range(1, min(W, len(past)) + 1):
                refs, ok, since = clipped[-a]
                m = _best(c, refs, ok, since, P)
                if m is not None and (best is None or m + a < best):
                    best = m + a
            if best is not None and best <= S:
                rt.append(b)
                st.append(best)
                it.append(i)
        et, se = d + rt, [0] * len(d) + st
        E.append(et)
        SI.append(se)
        R.append(rt)
        IDX.append(it)
        past = (past + [(et, se)])[-W:]
        clipped = (clipped + [_clipped(et, h, w) + (np.asarray(se, np.int64),)])[-W:]
    return E, SI, R, IDX, past


A, A2, FAR = (10, 10, 30, 30), (11, 10, 31, 30), (60, 60, 90, 95)
EMPTIES = [(200, 200, 240, 230), (60, 30, 60, 50), (-50, -50, -10, -10)]
# name: (strong, weak, W, S, P, expected R per frame, expected since of R per frame) on a 100 x 100 frame
CRAFTED = {
    "weak_after_strong": ([[A], []], [[], [A2]], 1, 5, 30, [[], [A2]], [[], [1]]),
    "weak_alone": ([[], []], [[A], [A]], 1, 5, 30, [[], []], [[], []]),
    "frame0_rescues_nothing": ([[A]], [[A2]], 2, 5, 30, [[]], [[]]),
    "chain_to_span": ([[A], [], [], [], [], []], [[], [A], [A2], [A], [A2], [A]], 1, 3, 30,
                      [[], [A], [A2], [A], [], []], [[], [1], [2], [3], [], []]),
    "gap_of_W": ([[A], [], []], [[], [], [A2]], 2, 5, 30, [[], [], [A2]], [[], [], [2]]),
    "gap_of_W_plus_1": ([[A], [], [], []], [[], [], [], [A2]], 2, 5, 30, [[], [], [], []], [[], [], [], []]),
    "inclusive_match": ([[(0, 0, 10, 10)], []], [[], [(0, 0, 10, 3)]], 1, 5, 30, [[], [(0, 0, 10, 3)]], [[], [1]]),
    "just_below": ([[(0, 0, 10, 10)], []], [[], [(0, 0, 9, 3)]], 1, 5, 30, [[], []], [[], []]),
    "empties_never_rescued": ([EMPTIES, []], [[], EMPTIES], 1, 5, 1, [[], []], [[], []]),
    "empties_never_match": ([EMPTIES + [FAR], []], [[], [(50, 20, 70, 60)]], 1, 5, 1, [[], []], [[], []]),
    "rescued_unclipped": ([[(0, 0, 10, 10)], []], [[], [(-5, -5, 10, 10)]], 1, 5, 100,
                          [[], [(-5, -5, 10, 10)]], [[], [1]]),
    # the strong list is faces ++ plates: a weak face over a strong plate (the second strong box)
    "weak_face_strong_plate": ([[FAR, A], []], [[], [A2]], 1, 5, 30, [[], [A2]], [[], [1]]),
    "order_of_R": ([[FAR, A], [A], []], [[], [], [A2, (0, 50, 5, 55), (61, 60, 91, 95)]], 2, 5, 30,
                   [[], [], [A2, (61, 60, 91, 95)]], [[], [], [1, 2]]),
    # frame 3: a = 1 reaches a rescued box with since 2 (3 in all), a = 3 the strong box itself (3): the minimum
    # over both; frame 4 then continues the chain at 4
    "minimum_over_the_window": ([[A], [], [], [], []], [[], [A2], [A], [A2], [A]], 3, 9, 30,
                                [[], [A2], [A], [A2], [A]], [[], [1], [2], [3], [4]]),
}


def random_sequence(seed, frames=12, h=120, w=160, most=40):
    """-> (strong, weak, h, w): per frame up to `most` boxes in all. Tracks are strong for a few frames and then
    weak for a few (chains with since 1, 2, ..), missing now and then (gaps), exact copies about half of the time
    (matches at P = 100) and jittered by up to 3 pixels otherwise; around them weak and strong noise with
    coordinates in [-20, 180]: clipped, degenerate and outside boxes among it."""
    rng = np.random.default_rng(seed)
    tracks = []
    for _ in range(10):
        x1, y1 = int(rng.integers(-10, w - 20)), int(rng.integers(-10, h - 20))
        tracks.append([np.asarray([x1, y1, x1 + int(rng.integers(12, 50)), y1 + int(rng.integers(12, 50))]),
                       int(rng.integers(0, 4))])
    strong, weak = [], []
    for t in range(frames):
        s, k = [], []
        for tr in tracks:
            if rng.random() < 0.5:
                tr[0] = tr[0] + rng.integers(-3, 4, 4)
            tr[1] += 1
            phase = tr[1] % 9                             # 0..2 strong, 3..8 weak
            if rng.random() < 0.15:
                continue                                  # missed altogether
            (s if phase < 3 else k).append(tuple(int(v) for v in tr[0]))
        for lst, n in ((s, int(rng.integers(0, 6))), (k, int(rng.integers(0, 12)))):
            for _ in range(n):
                x1, y1 = rng.integers(-20, 181, 2)
                b = np.clip([x1, y1, x1 + rng.integers(-5, 60), y1 + rng.integers(-5, 60)], -20, 180)
                lst.append(tuple(int(v) for v in b))
        order = rng.permutation(len(k))
        k = [k[i] for i in order]
        assert len(s) + len(k) <= most
        strong.append(s)
        weak.append(k)
    return strong, weak, h, w

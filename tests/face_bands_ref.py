"""Letterbox bands of the face stem and layer1, in Python: the row-interval rule (closed form)
and a brute-force propagation of "depends on band rows only" through the same steps.

A canvas of H rows holds image rows [top, top + nh); with left == 0 the rows outside are the pad
colour minus the mean. An output row y of a k x k, stride s, pad p step reads input rows
s y - p .. s y - p + k - 1 clipped to the map. Steps: conv1 7x7/2 pad 3, maxpool 3x3/2 pad 1, then
one 3x3 pad 1 per layer1 bottleneck. Tiles: 6 pool rows in the fused stem, 8 rows in the blocks.
"""
import numpy as np

STEPS = [[(7, 2, 3), (3, 2, 1)], [(3, 1, 1)], [(3, 1, 1)], [(3, 1, 1)]]   # per band op: (k, s, p) steps
TILE_H = [6, 8, 8, 8]


def _out_h(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def rule(canvas_h, top, nh, left):
    """Per band op (top_end, bot_begin, tile_rows, lo, hi): rows [0, top_end) and [bot_begin, h) are
    band rows, tile rows [0, lo) and [hi, tile_rows) band tiles (none: lo = 0, hi = tile_rows)."""
    h, te, bb = canvas_h, top, top + nh
    if left != 0:
        te, bb = 0, h
    out = []
    for steps, th in zip(STEPS, TILE_H):
        for k, s, p in steps:
            oh = _out_h(h, k, s, p)
            # last input row s y - p + k - 1 < te; first input row s y - p >= bb
            te = min(oh, max(0, (te - k + p) // s + 1))
            bb = oh if bb >= h else min(oh, -(-(bb + p) // s))
            h = oh
        tr = -(-h // th)
        lo, hi = te // th, min(tr, -(-bb // th))
        if lo >= hi:
            lo, hi = 0, tr
        out.append((te, bb, tr, lo, hi))
    return out


def brute(canvas_h, top, nh, left):
    """Per band op a bool array over its output rows: the row depends on band rows only."""
    band = np.zeros(canvas_h, bool)
    if left == 0:
        band[:top] = True
        band[top + nh:] = True
    out = []
    for steps in STEPS:
        for k, s, p in steps:
            oh = _out_h(len(band), k, s, p)
            nxt = np.zeros(oh, bool)
            for y in range(oh):
                rows = [r for r in range(s * y - p, s * y - p + k) if 0 <= r < len(band)]
                nxt[y] = all(band[r] for r in rows)
            band = nxt
        out.append(band.copy())
    return out

// box_match.h — the clip and the match predicate of the box hold (hold.hip) and the look-ahead
// hold (lead.hip): one definition, so both directions judge a pair of boxes to the bit alike.
#pragma once
#include "vd_kernel.h"

// combine_detect.py:145-148 clip, :150-151 empty check; an empty box becomes (0, 0, 0, 0),
// which intersects nothing
__device__ __forceinline__ int4 clip_box(int4 b, int w, int h) {
    const int x1 = max(0, b.x), y1 = max(0, b.y), x2 = min(w, b.z), y2 = min(h, b.w);
    if (!(x2 > x1 && y2 > y1)) return make_int4(0, 0, 0, 0);
    return make_int4(x1, y1, x2, y2);
}

// q non-empty and clipped, area aq; r clipped (possibly the empty (0, 0, 0, 0))
__device__ __forceinline__ bool boxes_match(int4 q, long long aq, int4 r, int P) {
    const int iw = min(q.z, r.z) - max(q.x, r.x), ih = min(q.w, r.w) - max(q.y, r.y);
    if (iw <= 0 || ih <= 0) return false;
    const long long inter = (long long)iw * ih;
    const long long uni = aq + (long long)(r.z - r.x) * (r.w - r.y) - inter;
    return 100 * inter >= (long long)P * uni;
}

// motion mode: the same test, handing out inter and union for the best-IoU comparison
__device__ __forceinline__ bool boxes_match_iou(int4 q, long long aq, int4 r, int P, long long* inter_out,
                                                long long* uni_out) {
    const int iw = min(q.z, r.z) - max(q.x, r.x), ih = min(q.w, r.w) - max(q.y, r.y);
    if (iw <= 0 || ih <= 0) return false;
    const long long inter = (long long)iw * ih;
    const long long uni = aq + (long long)(r.z - r.x) * (r.w - r.y) - inter;
    *inter_out = inter;
    *uni_out = uni;
    return 100 * inter >= (long long)P * uni;
}

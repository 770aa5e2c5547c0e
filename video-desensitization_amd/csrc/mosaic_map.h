// mosaic_map.h — the pixelation map of one box, shared by the RGB pass (mosaic.hip) and the NV12
// pass (nv12.hip): a clipped rectangle (x1, y1, x2, y2) and its small size sw | sh << 16; the
// composite down(up(.)) of OpenCV's resizeNN per axis, in its double-precision index rule
// (combine_detect.py:152-158, oracle/mosaic.py).
#pragma once
#include "vd_math.h"

__device__ __forceinline__ bool in_rect(const int4 q, int y, int x) {
    return x >= q.x && x < q.z && y >= q.y && y < q.w;
}

__device__ __forceinline__ double up_factor(int len, int s) {      // resizeNN up:   dst = len, src = s
    return __ddiv_rn(1.0, __ddiv_rn((double)len, (double)s));
}
__device__ __forceinline__ double down_factor(int len, int s) {    // resizeNN down: dst = s, src = len
    return __ddiv_rn(1.0, __ddiv_rn((double)s, (double)len));
}

// p <- down(up(p)) of the box (rect, sw | sh << 16)
__device__ __forceinline__ void apply_rect(const int4 q, uint32_t sz, int& y, int& x) {
    const int sw = (int)(sz & 0xFFFFu), sh = (int)(sz >> 16);
    const int bw = q.z - q.x, bh = q.w - q.y;
    const int ux = min((int)floor(VD_DMUL((double)(x - q.x), up_factor(bw, sw))), sw - 1);
    const int dx = min((int)floor(VD_DMUL((double)ux, down_factor(bw, sw))), bw - 1);
    const int uy = min((int)floor(VD_DMUL((double)(y - q.y), up_factor(bh, sh))), sh - 1);
    const int dy = min((int)floor(VD_DMUL((double)uy, down_factor(bh, sh))), bh - 1);
    x = q.x + dx;
    y = q.y + dy;
}

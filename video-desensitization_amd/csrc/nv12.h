// nv12.h — the NV12 frame format (include/vdmi.h at vd_nv12): the integer colour conversion shared by
// the letterbox kernels (pre.hip) and the host call vd_nv12_to_rgb, the layout rules of a descriptor,
// and the source descriptor the letterbox launchers take. No HIP needed: a plain C++ compiler takes
// this header too (tools/nv12_check.cpp).
#pragma once
#include "../../include/vdmi.h"
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VD_NV12_HD __host__ __device__ inline
#else
#define VD_NV12_HD inline
#endif

// rows of the table in include/vdmi.h: coefficients are round(256 * real coefficient)
struct Nv12Coef { int yoff, cy, crv, cgu, cgv, cbu; };

VD_NV12_HD Nv12Coef vd_nv12_coef(int matrix, int range) {
    if (range == VD_NV12_LIMITED)
        return matrix == VD_NV12_BT601 ? Nv12Coef{16, 298, 409, -100, -208, 516} : Nv12Coef{16, 298, 459, -55, -136, 541};
    return matrix == VD_NV12_BT601 ? Nv12Coef{0, 256, 359, -88, -183, 454} : Nv12Coef{0, 256, 403, -48, -120, 475};
}

VD_NV12_HD int vd_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rgb = C(Y, U, V): int32 arithmetic, arithmetic shifts. The one conversion of the library.
VD_NV12_HD void vd_nv12_rgb(const Nv12Coef& k, int Y, int U, int V, int rgb[3]) {
    const int t = k.cy * (Y - k.yoff) + 128, u = U - 128, v = V - 128;
    rgb[0] = vd_clip8((t + k.crv * v) >> 8);
    rgb[1] = vd_clip8((t + k.cgu * u + k.cgv * v) >> 8);
    rgb[2] = vd_clip8((t + k.cbu * u) >> 8);
}

// An NV12 source of the letterbox (LetterboxArgs::nv; on == 0: packed RGB, nothing else is read):
// LetterboxArgs::src is the first frame's first luma byte, pitch the row pitch of both planes.
struct Nv12Src {
    int on;
    size_t uv_offset, frame_stride;
    Nv12Coef k;
};

// The layout rules of a descriptor for n frames of h x w (colour: matrix and range too). 0, or which
// rule fails: 1 null, 2 n / h / w, 3 pitch, 4 uv_offset, 5 frame_stride, 6 matrix, 7 range. Sizes are
// bounded (pitch < 2^31, offsets < 2^47, n * frame_stride < 2^62) so no product below can wrap.
inline int vd_nv12_layout(const vd_nv12* d, int n, int h, int w, bool colour) {
    if (!d || !d->base) return 1;
    if (n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return 2;
    if (d->pitch < (size_t)w || d->pitch >= ((size_t)1 << 31)) return 3;
    if (d->uv_offset < (size_t)h * d->pitch || d->uv_offset >= ((size_t)1 << 47)) return 4;
    if (d->frame_stride < d->uv_offset + (size_t)(h / 2) * d->pitch || d->frame_stride >= ((size_t)1 << 47)) return 5;
    if (colour && d->matrix != VD_NV12_BT601 && d->matrix != VD_NV12_BT709) return 6;
    if (colour && d->range != VD_NV12_LIMITED && d->range != VD_NV12_FULL) return 7;
    return 0;
}

// C(frame) of n checked frames into packed RGB rows (vd_nv12_to_rgb behind its checks)
inline void vd_nv12_to_rgb_host(const vd_nv12* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch) {
    const Nv12Coef k = vd_nv12_coef(in->matrix, in->range);
    for (int f = 0; f < n; ++f) {
        const uint8_t* yp = in->base + (size_t)f * in->frame_stride;
        const uint8_t* uvp = yp + in->uv_offset;
        for (int y = 0; y < h; ++y) {
            const uint8_t* yr = yp + (size_t)y * in->pitch;
            const uint8_t* ur = uvp + (size_t)(y >> 1) * in->pitch;
            uint8_t* o = rgb + ((size_t)f * h + y) * rgb_pitch;
            for (int x = 0; x < w; ++x) {
                int c[3];
                vd_nv12_rgb(k, yr[x], ur[x & ~1], ur[(x & ~1) + 1], c);
                o[3 * x] = (uint8_t)c[0]; o[3 * x + 1] = (uint8_t)c[1]; o[3 * x + 2] = (uint8_t)c[2];
            }
        }
    }
}

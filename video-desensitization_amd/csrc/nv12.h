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

// A 4:2:0 source of the letterbox (LetterboxArgs::nv; on == 0: packed RGB, nothing else is read):
// LetterboxArgs::src is the first frame's first luma byte, pitch the luma row pitch.
//   on == 1  NV12: the chroma pairs at uv_offset, rows of `pitch` bytes (the other chroma fields are not read)
//   on == 2  any layout of vd_yuv420: U at uv_offset, V at v_offset, rows of cpitch bytes, samples step apart
//   on == 3  any layout of vd_yuv420_16: as 2 with 16-bit words (offsets and pitches in bytes, step in
//            samples); the 8-bit sample of D(S) is (word >> sh16) & 255, sh16 = shift + depth - 8
struct Nv12Src {
    int on;
    size_t uv_offset, frame_stride;
    Nv12Coef k;
    size_t v_offset, cpitch;
    int step;
    int sh16;
};

// A batch of 8-bit 4:2:0 surfaces in device memory (include/vdmi.h at vd_yuv420): luma rows of
// `pitch` bytes at base, U / V sample (cy, cx) at u / v + cy * cpitch + cx * step, frame f at
// + f * stride. The kernels take every layout in this form; nv12() marks the one the NV12-only
// kernels were written for, which those layouts keep running.
// depth != 0: surfaces of 16-bit words (include/vdmi.h at vd_yuv420_16) -- everything above stays in
// bytes, step stays in samples, a sample's value is (word >> shift) & ((1 << depth) - 1).
struct Yuv420Dev {
    uint8_t* base;
    size_t pitch, u, v, cpitch, stride;
    int step;
    int depth = 0, shift = 0;
    bool nv12() const { return step == 2 && v == u + 1 && cpitch == pitch && !depth; }
    // first byte of the chroma storage that 16-B vectors are aligned against (interleaved: the pair)
    size_t c0() const { return u < v ? u : v; }
    int es() const { return depth ? 2 : 1; }   // bytes per sample
};
inline Yuv420Dev vd_yuv420_dev(const vd_yuv420& d) {
    return Yuv420Dev{d.base, d.pitch, d.u_offset, d.v_offset, d.chroma_pitch, d.frame_stride, d.chroma_step};
}
inline Yuv420Dev vd_yuv420_dev(const vd_yuv420_16& d) {
    return Yuv420Dev{d.base, d.pitch, d.u_offset, d.v_offset, d.chroma_pitch, d.frame_stride, d.chroma_step, d.depth, d.shift};
}
inline vd_yuv420 vd_yuv420_of_nv12(const vd_nv12& d) {
    return vd_yuv420{d.base, d.pitch, d.uv_offset, d.uv_offset + 1, d.pitch, d.frame_stride, 2, d.matrix, d.range};
}
// n surfaces packed in layout (step, V first): pitch w samples, the chroma right behind the luma
// (depth != 0: 16-bit words, so every size doubles)
inline Yuv420Dev vd_yuv420_packed(void* p, int h, int w, int step, bool v_first, int depth = 0, int shift = 0) {
    const size_t es = depth ? 2 : 1, y = (size_t)h * w * es, c = (size_t)(h / 2) * (w / 2) * es;
    if (step == 2)
        return Yuv420Dev{(uint8_t*)p, w * es, y + (v_first ? es : 0), y + (v_first ? 0 : es), w * es, y + 2 * c, 2, depth, shift};
    return Yuv420Dev{(uint8_t*)p, w * es, y + (v_first ? c : 0), y + (v_first ? 0 : c), (w / 2) * es, y + 2 * c, 1, depth, shift};
}

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

// The layout rules of a vd_yuv420 descriptor for n frames of h x w (include/vdmi.h at vd_yuv420). 0, or
// which rule fails: 1 null, 2 n / h / w, 3 pitch, 4 chroma_step, 5 chroma_pitch, 6 interleaved offsets,
// 7 u_offset (overlaps the luma plane, or >= 2^47), 8 v_offset (overlaps the luma or the U plane, or
// >= 2^47), 9 frame_stride, 10 matrix, 11 range. The same bounds as above keep every product from wrapping.
struct Yuv420Extent { size_t lo, hi; };   // bytes [lo, hi) of a frame
inline bool vd_extents_meet(Yuv420Extent a, Yuv420Extent b) { return a.lo < b.hi && b.lo < a.hi; }
inline int vd_yuv420_layout(const vd_yuv420* d, int n, int h, int w, bool colour, size_t* frame_end = nullptr) {
    if (!d || !d->base) return 1;
    if (n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return 2;
    if (d->pitch < (size_t)w || d->pitch >= ((size_t)1 << 31)) return 3;
    if (d->chroma_step != 1 && d->chroma_step != 2) return 4;
    const size_t crow = (size_t)(w / 2) * d->chroma_step, crows = (size_t)(h / 2);
    if (d->chroma_pitch < crow || d->chroma_pitch >= ((size_t)1 << 31)) return 5;
    if (d->u_offset >= ((size_t)1 << 47)) return 7;
    if (d->v_offset >= ((size_t)1 << 47)) return 8;
    const Yuv420Extent Y{0, (size_t)(h - 1) * d->pitch + w};
    const size_t cspan = (crows - 1) * d->chroma_pitch;
    size_t end = Y.hi;
    if (d->chroma_step == 2) {
        const size_t lo = d->u_offset < d->v_offset ? d->u_offset : d->v_offset;
        if (d->u_offset + d->v_offset - 2 * lo != 1) return 6;
        const Yuv420Extent C{lo, lo + cspan + crow};
        if (vd_extents_meet(Y, C)) return d->u_offset < d->v_offset ? 7 : 8;
        end = C.hi > end ? C.hi : end;
    } else {
        const Yuv420Extent U{d->u_offset, d->u_offset + cspan + crow}, V{d->v_offset, d->v_offset + cspan + crow};
        if (vd_extents_meet(Y, U)) return 7;
        if (vd_extents_meet(Y, V) || vd_extents_meet(U, V)) return 8;
        end = U.hi > end ? U.hi : end;
        end = V.hi > end ? V.hi : end;
    }
    if (d->frame_stride >= ((size_t)1 << 47) || (n > 1 && d->frame_stride < end)) return 9;
    if (colour && d->matrix != VD_NV12_BT601 && d->matrix != VD_NV12_BT709) return 10;
    if (colour && d->range != VD_NV12_LIMITED && d->range != VD_NV12_FULL) return 11;
    if (frame_end) *frame_end = end;
    return 0;
}

// The layout rules of a vd_yuv420_16 descriptor (include/vdmi.h at vd_yuv420_16): vd_yuv420_layout's on
// the byte extents of 16-bit words. 0, or which rule fails: 1 .. 11 as above (3, 5, 7, 8, 9 also for an
// odd value), 12 depth, 13 shift, 14 base not 2-byte aligned.
inline int vd_yuv420_16_layout(const vd_yuv420_16* d, int n, int h, int w, bool colour, size_t* frame_end = nullptr) {
    if (!d || !d->base) return 1;
    if (n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return 2;
    if (d->depth != 10 && d->depth != 12) return 12;
    if (d->shift < 0 || d->shift > 16 - d->depth) return 13;
    if ((uintptr_t)d->base & 1) return 14;
    if (d->pitch < 2 * (size_t)w || d->pitch >= ((size_t)1 << 31) || (d->pitch & 1)) return 3;
    if (d->chroma_step != 1 && d->chroma_step != 2) return 4;
    const size_t crow = (size_t)w * d->chroma_step, crows = (size_t)(h / 2);   // (w/2) * step words
    if (d->chroma_pitch < crow || d->chroma_pitch >= ((size_t)1 << 31) || (d->chroma_pitch & 1)) return 5;
    if (d->u_offset >= ((size_t)1 << 47)) return 7;
    if (d->v_offset >= ((size_t)1 << 47)) return 8;
    const size_t lo = d->u_offset < d->v_offset ? d->u_offset : d->v_offset;
    if (d->chroma_step == 2 && d->u_offset + d->v_offset - 2 * lo != 2) return 6;
    if (d->u_offset & 1) return 7;
    if (d->v_offset & 1) return 8;
    const Yuv420Extent Y{0, (size_t)(h - 1) * d->pitch + 2 * (size_t)w};
    const size_t cspan = (crows - 1) * d->chroma_pitch;
    size_t end = Y.hi;
    if (d->chroma_step == 2) {
        const Yuv420Extent C{lo, lo + cspan + crow};
        if (vd_extents_meet(Y, C)) return d->u_offset < d->v_offset ? 7 : 8;
        end = C.hi > end ? C.hi : end;
    } else {
        const Yuv420Extent U{d->u_offset, d->u_offset + cspan + crow}, V{d->v_offset, d->v_offset + cspan + crow};
        if (vd_extents_meet(Y, U)) return 7;
        if (vd_extents_meet(Y, V) || vd_extents_meet(U, V)) return 8;
        end = U.hi > end ? U.hi : end;
        end = V.hi > end ? V.hi : end;
    }
    if (d->frame_stride >= ((size_t)1 << 47) || (d->frame_stride & 1) || (n > 1 && d->frame_stride < end)) return 9;
    if (colour && d->matrix != VD_NV12_BT601 && d->matrix != VD_NV12_BT709) return 10;
    if (colour && d->range != VD_NV12_LIMITED && d->range != VD_NV12_FULL) return 11;
    if (frame_end) *frame_end = end;
    return 0;
}

// C(D(frame)) of n checked frames of 16-bit words (vd_yuv420_16_to_rgb behind its checks): the 8-bit
// sample of D is (word >> (shift + depth - 8)) & 255
inline void vd_yuv420_16_to_rgb_host(const vd_yuv420_16* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch) {
    const Nv12Coef k = vd_nv12_coef(in->matrix, in->range);
    const size_t st = (size_t)in->chroma_step;
    const int sh = in->shift + in->depth - 8;
    auto s8 = [sh](const uint8_t* p) { return (int)((((unsigned)p[0] | ((unsigned)p[1] << 8)) >> sh) & 255u); };   // little-endian
    for (int f = 0; f < n; ++f) {
        const uint8_t* yp = in->base + (size_t)f * in->frame_stride;
        for (int y = 0; y < h; ++y) {
            const uint8_t* yr = yp + (size_t)y * in->pitch;
            const uint8_t* ur = yp + in->u_offset + (size_t)(y >> 1) * in->chroma_pitch;
            const uint8_t* vr = yp + in->v_offset + (size_t)(y >> 1) * in->chroma_pitch;
            uint8_t* o = rgb + ((size_t)f * h + y) * rgb_pitch;
            for (int x = 0; x < w; ++x) {
                int c[3];
                const size_t cx = (size_t)(x >> 1) * st * 2;
                vd_nv12_rgb(k, s8(yr + 2 * (size_t)x), s8(ur + cx), s8(vr + cx), c);
                o[3 * x] = (uint8_t)c[0]; o[3 * x + 1] = (uint8_t)c[1]; o[3 * x + 2] = (uint8_t)c[2];
            }
        }
    }
}

// C(frame) of n checked frames of any layout into packed RGB rows (vd_yuv420_to_rgb behind its checks)
inline void vd_yuv420_to_rgb_host(const vd_yuv420* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch) {
    const Nv12Coef k = vd_nv12_coef(in->matrix, in->range);
    const size_t st = (size_t)in->chroma_step;
    for (int f = 0; f < n; ++f) {
        const uint8_t* yp = in->base + (size_t)f * in->frame_stride;
        for (int y = 0; y < h; ++y) {
            const uint8_t* yr = yp + (size_t)y * in->pitch;
            const uint8_t* ur = yp + in->u_offset + (size_t)(y >> 1) * in->chroma_pitch;
            const uint8_t* vr = yp + in->v_offset + (size_t)(y >> 1) * in->chroma_pitch;
            uint8_t* o = rgb + ((size_t)f * h + y) * rgb_pitch;
            for (int x = 0; x < w; ++x) {
                int c[3];
                vd_nv12_rgb(k, yr[x], ur[(size_t)(x >> 1) * st], vr[(size_t)(x >> 1) * st], c);
                o[3 * x] = (uint8_t)c[0]; o[3 * x + 1] = (uint8_t)c[1]; o[3 * x + 2] = (uint8_t)c[2];
            }
        }
    }
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

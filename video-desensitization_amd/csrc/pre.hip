// pre.hip — letterbox/normalise/pack, max-pool and nearest-upsample kernels.
//
// letterbox_kernel replaces, in one HBM pass per frame batch:
//   Retinaface.preprocess (detect_face/face.py:65-88) = letterbox_image
//   (detect_face/utils/utils.py:8-18: cv2.resize INTER_LINEAR [ext] + paste in a
//   128-filled canvas) + preprocess_input (:27-28, subtract (104,117,123) in
//   RGB order) + HWC->CHW + float32 + H2D; and the ultralytics LetterBox
//   (stride-32 auto padding, value 114, BGR<->RGB flip, /255) [ext] of the plate
//   detector call (combine_detect.py:217). Output is NHWC with `cpad` channels
//   (3 real + zeros) so the stem conv reads one 16-byte vector per tap.
//   cv2.resize rounding is restated exactly (oracle/letterbox.py):
//     COPY  (dsize == ssize), AREA2 (exact 2x: (a+b+c+d+2)>>2),
//     LINEAR (11-bit fixed point, SIMD vertical form).
#include "vd_common.h"
#include "vd_math.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

struct Tap { int s0, s1, a0, a1; };

__device__ __forceinline__ Tap linear_tap(int d, int ssize, double scale) {
    // fx = (float)((dx + 0.5) * scale_x - 0.5); sx = floor(fx); fx -= sx; border clamps
    float f = (float)VD_DSUB(VD_DMUL(VD_DADD((double)d, 0.5), scale), 0.5);
    int s = (int)floorf(f);
    f = VD_FSUB(f, (float)s);
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    Tap t;
    t.s0 = s;
    t.s1 = min(s + 1, ssize - 1);
    t.a0 = __float2int_rn(VD_FMUL(VD_FSUB(1.0f, f), 2048.0f));
    t.a1 = __float2int_rn(VD_FMUL(f, 2048.0f));
    return t;
}

// ---- pixel sources: where the letterbox arithmetic takes a source pixel's three channels from.
// A frame in global memory (get(y, x)) and a staged row in LDS (get(x)), each as three packed bytes
// or as an NV12 surface converted by the library's one conversion (nv12.h) at the tap. Everything
// below is written once against these and instantiated for both.
struct FrameRgb {
    const uint8_t* p; size_t pitch;
    __device__ __forceinline__ void get(int y, int x, int o[3]) const {
        const uint8_t* q = p + (size_t)y * pitch + x * 3;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
    }
    __device__ __forceinline__ static int row_bytes(int iw) { return (iw * 3 + 15) / 16 * 16; }   // a staged row
};
// The 4:2:0 sources come in two forms. Whole: the frame, whose first luma pixel sits on a chroma sample
// (no parity fields, the arithmetic of a standalone frame). Rect: a rectangle of a frame at origin
// (y0, x0) -- the luma pointer at (y0, x0), the chroma pointers at (y0 >> 1, x0 >> 1) of the FRAME, and
// the origin's parities (py, px) = (y0 & 1, x0 & 1): local pixel (yy, x) takes chroma row (py + yy) >> 1
// and chroma sample (px + x) >> 1 from there. A rectangle of a 4:2:0 frame is NOT a 4:2:0 frame.
// (cy / cx: a local row / column as counted from the chroma sample the chroma pointers point at)
struct Whole {
    static constexpr bool rect = false;
    __device__ __forceinline__ static int cy(int yy) { return yy; }
    __device__ __forceinline__ static int cx(int x) { return x; }
};
struct Rect {
    static constexpr bool rect = true; int py, px;
    __device__ __forceinline__ int cy(int yy) const { return py + yy; }
    __device__ __forceinline__ int cx(int x) const { return px + x; }
};

__device__ __host__ __forceinline__ constexpr int lb_up16(int b) { return (b + 15) / 16 * 16; }
// chroma samples a staged row of iw pixels can need: ((px + iw + 1) >> 1) <= iw / 2 + 1 in a rectangle
template <typename P> __device__ __host__ __forceinline__ constexpr int lb_csamples_max(int iw) { return P::rect ? iw / 2 + 1 : iw / 2; }

template <typename P>
struct FrameNv12T : P {
    const uint8_t* y; const uint8_t* uv; size_t pitch; Nv12Coef k;
    __device__ __forceinline__ void get(int yy, int x, int o[3]) const {
        const uint8_t* q = uv + (size_t)(P::cy(yy) >> 1) * pitch + (P::cx(x) & ~1);
        vd_nv12_rgb(k, y[(size_t)yy * pitch + x], q[0], q[1], o);
    }
    // a staged row: the luma row, then (16-B aligned) its chroma row. Rect: the chroma row is
    // 2 * ((px + iw + 1) >> 1) <= 2 * (iw / 2 + 1) bytes from the pair of the first pixel, so
    // up16(iw) + up16(2 * (iw / 2 + 1)) <= 2 * iw + 32 bytes: within LB_LDS_MAX whenever
    // iw * 3 <= LB_LDS_MAX (iw >= 32), and iw < 32 is 94 bytes at most.
    __device__ __forceinline__ static int luma_bytes(int iw) { return lb_up16(iw); }
    __device__ __forceinline__ static int row_bytes(int iw) {
        if constexpr (P::rect) return lb_up16(iw) + lb_up16(2 * (iw / 2 + 1));
        else return 2 * ((iw + 15) / 16 * 16);
    }
};
using FrameNv12 = FrameNv12T<Whole>;
struct RowRgb {
    const uint8_t* L;
    __device__ __forceinline__ void get(int x, int o[3]) const { o[0] = L[x * 3]; o[1] = L[x * 3 + 1]; o[2] = L[x * 3 + 2]; }
};
template <typename P>
struct RowNv12T : P {
    const uint8_t* L; int uvo; Nv12Coef k;
    __device__ __forceinline__ void get(int x, int o[3]) const {
        const int c = uvo + (P::cx(x) & ~1);
        vd_nv12_rgb(k, L[x], L[c], L[c + 1], o);
    }
};
using RowNv12 = RowNv12T<Whole>;

// Any 8-bit 4:2:0 layout (include/vdmi.h at vd_yuv420): a luma row, a U row and a V row, chroma
// samples `step` bytes apart (1: planar I420 / YV12; 2: interleaved, where NV21 is simply the V
// pointer one byte below the U pointer). The same conversion at the tap.
template <typename P>
struct FrameYuvT : P {
    const uint8_t* y; const uint8_t* u; const uint8_t* v; size_t pitch, cpitch; int step; Nv12Coef k;
    __device__ __forceinline__ void get(int yy, int x, int o[3]) const {
        const size_t c = (size_t)(P::cy(yy) >> 1) * cpitch + (size_t)(P::cx(x) >> 1) * step;
        vd_nv12_rgb(k, y[(size_t)yy * pitch + x], u[c], v[c], o);
    }
    // A staged row is three 16-B aligned segments: the luma row (iw bytes), then two of cs bytes
    // rounded up, cs = iw / 2 chroma samples (Rect: iw / 2 + 1, the most that ((px + iw + 1) >> 1)
    // can be) -- planar: the U row and the V row; interleaved: both hold the pair row (2 * samples
    // bytes from the lower of the two pointers, which 2 * up16(cs) >= 2 * cs has room for).
    // Whole: at most 2 * iw + 45 bytes, within LB_LDS_MAX whenever iw * 3 <= LB_LDS_MAX (iw >= 46),
    // and iw < 46 is 137 bytes at most. Rect: up16(iw) + 2 * up16(iw / 2 + 1) <= 2 * iw + 47 bytes,
    // within LB_LDS_MAX whenever iw * 3 <= LB_LDS_MAX (iw >= 47), and iw < 47 is 139 bytes at most.
    __device__ __forceinline__ static int luma_bytes(int iw) { return (iw + 15) / 16 * 16; }
    __device__ __forceinline__ static int row_bytes(int iw) { return luma_bytes(iw) + 2 * ((lb_csamples_max<P>(iw) + 15) / 16 * 16); }
};
using FrameYuv = FrameYuvT<Whole>;
template <typename P>
struct RowYuvT : P {
    const uint8_t* L; int uo, vo, step; Nv12Coef k;
    __device__ __forceinline__ void get(int x, int o[3]) const {
        const int c = (P::cx(x) >> 1) * step;
        vd_nv12_rgb(k, L[x], L[uo + c], L[vo + c], o);
    }
};
using RowYuv = RowYuvT<Whole>;

// 10- and 12-bit 4:2:0 (include/vdmi.h at vd_yuv420_16): FrameYuv over 16-bit words -- pitches and
// offsets in bytes, `step` in samples. Detection sees D(S): the 8-bit sample (word >> sh) & 255 with
// sh = shift + depth - 8, which also drops the unused bits. A staged row is reduced to those bytes on
// its way into LDS, so the row slots and the tap code are FrameYuv's and RowYuv's.
template <typename P>
struct FrameYuv16T : P {
    const uint8_t* y; const uint8_t* u; const uint8_t* v; size_t pitch, cpitch; int step, sh; Nv12Coef k;
    __device__ __forceinline__ static int s8(const uint8_t* p, int sh) { return (int)(((unsigned)*(const uint16_t*)p >> sh) & 255u); }
    __device__ __forceinline__ void get(int yy, int x, int o[3]) const {
        const size_t c = (size_t)(P::cy(yy) >> 1) * cpitch + (size_t)(P::cx(x) >> 1) * step * 2;
        vd_nv12_rgb(k, s8(y + (size_t)yy * pitch + 2 * (size_t)x, sh), s8(u + c, sh), s8(v + c, sh), o);
    }
    __device__ __forceinline__ static int luma_bytes(int iw) { return FrameYuvT<P>::luma_bytes(iw); }
    __device__ __forceinline__ static int row_bytes(int iw) { return FrameYuvT<P>::row_bytes(iw); }
};
using FrameYuv16 = FrameYuv16T<Whole>;

// LetterboxArgs::nv.on, and whether the source is a rectangle of the frame (the tile letterbox)
template <int NV, bool R = false> struct SrcOf { using Frame = FrameRgb; using Row = RowRgb; };
template <> struct SrcOf<1, false> { using Frame = FrameNv12; using Row = RowNv12; };
template <> struct SrcOf<2, false> { using Frame = FrameYuv; using Row = RowYuv; };
template <> struct SrcOf<3, false> { using Frame = FrameYuv16; using Row = RowYuv; };
template <> struct SrcOf<1, true> { using Frame = FrameNv12T<Rect>; using Row = RowNv12T<Rect>; };
template <> struct SrcOf<2, true> { using Frame = FrameYuvT<Rect>; using Row = RowYuvT<Rect>; };
template <> struct SrcOf<3, true> { using Frame = FrameYuv16T<Rect>; using Row = RowYuvT<Rect>; };

// frame f of the batch
template <int NV>
__device__ __forceinline__ typename SrcOf<NV>::Frame lb_frame(const LetterboxArgs& a, int f) {
    if constexpr (NV == 3) {
        const uint8_t* b = a.src + (size_t)f * a.nv.frame_stride;
        return FrameYuv16{{}, b, b + a.nv.uv_offset, b + a.nv.v_offset, a.pitch, a.nv.cpitch, a.nv.step, a.nv.sh16, a.nv.k};
    } else if constexpr (NV == 2) {
        const uint8_t* b = a.src + (size_t)f * a.nv.frame_stride;
        return FrameYuv{{}, b, b + a.nv.uv_offset, b + a.nv.v_offset, a.pitch, a.nv.cpitch, a.nv.step, a.nv.k};
    } else if constexpr (NV == 1) {
        const uint8_t* b = a.src + (size_t)f * a.nv.frame_stride;
        return FrameNv12{{}, b, b + a.nv.uv_offset, a.pitch, a.nv.k};
    } else {
        return FrameRgb{a.src + (size_t)f * a.ih * a.pitch, a.pitch};
    }
}

// The rectangle at (y0, x0) of 4:2:0 frame f of the batch (its extent a.ih x a.iw is not read here).
// RGB needs no such form: a rectangle of a pitched frame is a pitched frame.
template <int NV>
__device__ __forceinline__ typename SrcOf<NV, true>::Frame lb_rect(const LetterboxArgs& a, int f, int y0, int x0) {
    const uint8_t* b = a.src + (size_t)f * a.nv.frame_stride;
    const Rect par{y0 & 1, x0 & 1};
    const size_t cy = (size_t)(y0 >> 1), cx = (size_t)(x0 >> 1);
    if constexpr (NV == 3) {
        const size_t c = cy * a.nv.cpitch + cx * a.nv.step * 2;
        return FrameYuv16T<Rect>{par, b + (size_t)y0 * a.pitch + 2 * (size_t)x0, b + a.nv.uv_offset + c, b + a.nv.v_offset + c,
                                 a.pitch, a.nv.cpitch, a.nv.step, a.nv.sh16, a.nv.k};
    } else if constexpr (NV == 2) {
        const size_t c = cy * a.nv.cpitch + cx * a.nv.step;
        return FrameYuvT<Rect>{par, b + (size_t)y0 * a.pitch + x0, b + a.nv.uv_offset + c, b + a.nv.v_offset + c, a.pitch,
                               a.nv.cpitch, a.nv.step, a.nv.k};
    } else {
        static_assert(NV == 1, "4:2:0 sources only");
        return FrameNv12T<Rect>{par, b + (size_t)y0 * a.pitch + x0, b + a.nv.uv_offset + cy * a.pitch + 2 * cx, a.pitch, a.nv.k};
    }
}

// staged row k of `lrow` (rows of RS bytes)
template <int NV>
__device__ __forceinline__ typename SrcOf<NV>::Row lb_row(const LetterboxArgs& a, const uint8_t* lrow, int k, int RS) {
    if constexpr (NV == 2 || NV == 3) {
        const int c0 = FrameYuv::luma_bytes(a.iw);
        if (a.nv.step == 2)   // the pair row from the lower pointer: the other channel is its next byte
            return RowYuv{{}, lrow + k * RS, c0 + (a.nv.uv_offset > a.nv.v_offset ? 1 : 0),
                          c0 + (a.nv.v_offset > a.nv.uv_offset ? 1 : 0), 2, a.nv.k};
        return RowYuv{{}, lrow + k * RS, c0, c0 + (RS - c0) / 2, 1, a.nv.k};
    } else if constexpr (NV == 1) {
        return RowNv12{{}, lrow + k * RS, RS / 2, a.nv.k};
    } else {
        return RowRgb{lrow + k * RS};
    }
}
// ... of a rectangle whose origin has x parity px (the staged chroma row is already the pixel row's)
template <int NV>
__device__ __forceinline__ typename SrcOf<NV, true>::Row lb_rect_row_at(const LetterboxArgs& a, const uint8_t* lrow, int k, int RS,
                                                                        int px) {
    if constexpr (NV == 2 || NV == 3) {
        const int c0 = FrameYuv::luma_bytes(a.iw);
        if (a.nv.step == 2)
            return RowYuvT<Rect>{{0, px}, lrow + k * RS, c0 + (a.nv.uv_offset > a.nv.v_offset ? 1 : 0),
                                 c0 + (a.nv.v_offset > a.nv.uv_offset ? 1 : 0), 2, a.nv.k};
        return RowYuvT<Rect>{{0, px}, lrow + k * RS, c0, c0 + (RS - c0) / 2, 1, a.nv.k};
    } else if constexpr (NV == 1) {
        return RowNv12T<Rect>{{0, px}, lrow + k * RS, FrameNv12T<Rect>::luma_bytes(a.iw), a.nv.k};
    } else {
        return RowRgb{lrow + k * RS};
    }
}

// The 3 channels of resized pixel (y, x) (interpolation taps computed once).
template <typename Frame>
__device__ __forceinline__ void resized_px3(const LetterboxArgs& a, const Frame& img, int y, int x, int out[3]) {
    if (a.mode == LB_COPY) {
        img.get(y, x, out);
        return;
    }
    if (a.mode == LB_AREA2) {
        int p00[3], p01[3], p10[3], p11[3];
        img.get(2 * y, 2 * x, p00); img.get(2 * y, 2 * x + 1, p01);
        img.get(2 * y + 1, 2 * x, p10); img.get(2 * y + 1, 2 * x + 1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
        return;
    }
    const Tap tx = linear_tap(x, a.iw, a.scale_x);
    const Tap ty = linear_tap(y, a.ih, a.scale_y);
    int p00[3], p01[3], p10[3], p11[3];
    img.get(ty.s0, tx.s0, p00); img.get(ty.s0, tx.s1, p01);
    img.get(ty.s1, tx.s0, p10); img.get(ty.s1, tx.s1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int d0 = p00[c] * tx.a0 + p01[c] * tx.a1;
        int d1 = p10[c] * tx.a0 + p11[c] * tx.a1;
        int v = ((((d0 >> 4) * ty.a0) >> 16) + (((d1 >> 4) * ty.a1) >> 16) + 2) >> 2;
        out[c] = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
}

// Normalised canvas pixel (y, x) (resized image or pad value), 3 channels.
template <typename Frame>
__device__ __forceinline__ void canvas_px(const LetterboxArgs& a, const Frame& img, int y, int x, float v[3]) {
    const int ry = y - a.top, rx = x - a.left;
    const bool inside = (unsigned)ry < (unsigned)a.nh && (unsigned)rx < (unsigned)a.nw;
    int p3[3] = {0, 0, 0};
    if (inside) resized_px3(a, img, ry, rx, p3);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int pv = a.flip ? p3[2 - c] : p3[c];
        const float px = inside ? (float)pv : a.pad_value;
        v[c] = VD_FDIV(VD_FSUB(px, a.mean[c]), a.div);
    }
}

// one 2x2 block's 16 values (4 sub-pixels x [3 channels, 0]): bf16, fp16 (a.out_f16:
// the fp32 plan's fused face stem canvas, integer values, exact) or f32 (a.out_f32)
__device__ __forceinline__ void store_s2d(const LetterboxArgs& a, size_t idx, const float (&v)[16]) {
    if (a.out_f32) {   // the fp32 plan's plate canvas: integer values as f32, 64 B per block
        float4* o = (float4*)((float*)a.out + idx * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        return;
    }
    uint4 u[2];
    if (a.out_f16) {
        _Float16 t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = (_Float16)v[i];
        u[0] = *(const uint4*)t; u[1] = *(const uint4*)(t + 8);
    } else {
        __bf16 t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = (__bf16)v[i];
        u[0] = *(const uint4*)t; u[1] = *(const uint4*)(t + 8);
    }
    uint4* out = (uint4*)((uint16_t*)a.out + idx * 16);
    out[0] = u[0];
    out[1] = u[1];
}

// Space-to-depth form (a.s2d): one thread per 2x2 canvas block, 32 B out.
// (img: the frame's pixels; f: the canvas index in a.out)
template <typename Frame>
__device__ __forceinline__ void lb_s2d_block(const LetterboxArgs& a, const Frame& img, int f, int Y, int X) {
    const int OW = a.ow / 2 + 1, OH = a.oh / 2 + 1;
    if (X >= OW) return;
    float t[16];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int y = 2 * Y + (s >> 1) - 1, x = 2 * X + (s & 1) - 1;
        float v[3] = {0.f, 0.f, 0.f};   // conv zero padding outside the canvas
        if ((unsigned)y < (unsigned)a.oh && (unsigned)x < (unsigned)a.ow) canvas_px(a, img, y, x, v);
        t[4 * s + 0] = v[0]; t[4 * s + 1] = v[1]; t[4 * s + 2] = v[2];
        t[4 * s + 3] = 0.f;
    }
    store_s2d(a, ((size_t)f * OH + Y) * OW + X, t);
}

template <int NV>
__global__ __launch_bounds__(256) void letterbox_s2d_kernel(LetterboxArgs a) {
    const int f = blockIdx.z;
    lb_s2d_block(a, lb_frame<NV>(a, f), f, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
}

// Space-to-depth form with the source rows staged in LDS: one workgroup per
// (frame, X' row Y) loads the <= 4 source rows its two canvas rows interpolate from
// with 16-B loads (only rows some output reads: 2 of every 3 at 1080p -> 360), then
// every 2x2 block is computed from LDS. Same arithmetic as resized_px3 / canvas_px.
constexpr int LB_LDS_MAX = 16384;   // max bytes per staged source row (frames up to 5461 px wide)

__device__ __forceinline__ void lb_src_rows(const LetterboxArgs& a, int y, int* r0, int* r1, Tap* ty, bool* inside) {
    const int ry = y - a.top;
    *inside = (unsigned)y < (unsigned)a.oh && (unsigned)ry < (unsigned)a.nh;
    *r0 = *r1 = -1;
    if (!*inside) return;
    if (a.mode == LB_COPY) { *r0 = *r1 = ry; return; }
    if (a.mode == LB_AREA2) { *r0 = 2 * ry; *r1 = 2 * ry + 1; return; }
    *ty = linear_tap(ry, a.ih, a.scale_y);
    *r0 = ty->s0;
    // a zero-weight second row (an exact gather: 1080p -> 640 samples rows 3y + 1 with weights
    // (1, 0)) adds exact zeros, so it is not staged: the pixel reads row r0 twice instead
    *r1 = ty->a1 ? ty->s1 : -1;
}

template <typename Row>
__device__ __forceinline__ void lb_px_lds(const LetterboxArgs& a, const Row& L0, const Row& L1, const Tap& ty,
                                          int x, bool row_in, float v[3]) {
    const int rx = x - a.left;
    const bool inside = row_in && (unsigned)rx < (unsigned)a.nw;
    int p3[3] = {0, 0, 0};
    if (inside) {
        if (a.mode == LB_COPY) {
            L0.get(rx, p3);
        } else if (a.mode == LB_AREA2) {
            int p00[3], p01[3], p10[3], p11[3];
            L0.get(2 * rx, p00); L0.get(2 * rx + 1, p01); L1.get(2 * rx, p10); L1.get(2 * rx + 1, p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) p3[c] = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
        } else if (a.gx_k > 0 && ty.a1 == 0) {
            // exact gather both ways (weights (1, 0): the bilinear sum below reduces to the
            // source byte exactly, ((4 p + 2) >> 2) = p), e.g. 1080p -> 640: column 3 rx + 1
            L0.get(a.gx_k * rx + a.gx_c, p3);
        } else {
            const Tap tx = linear_tap(rx, a.iw, a.scale_x);
            int p00[3], p01[3], p10[3], p11[3];
            L0.get(tx.s0, p00); L0.get(tx.s1, p01); L1.get(tx.s0, p10); L1.get(tx.s1, p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int d0 = p00[c] * tx.a0 + p01[c] * tx.a1;
                const int d1 = p10[c] * tx.a0 + p11[c] * tx.a1;
                const int q = ((((d0 >> 4) * ty.a0) >> 16) + (((d1 >> 4) * ty.a1) >> 16) + 2) >> 2;
                p3[c] = q < 0 ? 0 : (q > 255 ? 255 : q);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int pv = a.flip ? p3[2 - c] : p3[c];
        const float px = inside ? (float)pv : a.pad_value;
        v[c] = VD_FDIV(VD_FSUB(px, a.mean[c]), a.div);
    }
}

// rb bytes of a source row into LDS: 16-B loads where the row start is aligned
__device__ __forceinline__ void lb_stage(uint8_t* dst, const uint8_t* src, int rb) {
    const int nch = (rb + 15) / 16;
    if (((uintptr_t)src & 15) == 0) {
        for (int i = threadIdx.x; i < nch; i += 256) {
            if (16 * i + 16 <= rb) *(uint4*)(dst + 16 * i) = *(const uint4*)(src + 16 * i);
            else for (int b = 16 * i; b < rb; ++b) dst[b] = src[b];
        }
    } else {
        for (int i = threadIdx.x; i < rb; i += 256) dst[i] = src[i];
    }
}

// source row `row` of a frame into a staged-row slot: the pixels' bytes, or the luma row and its chroma row
__device__ __forceinline__ void lb_stage_row(const LetterboxArgs& a, const FrameRgb& img, int row, uint8_t* dst) {
    lb_stage(dst, img.p + (size_t)row * a.pitch, a.iw * 3);
}
// A rectangle's source row `row` takes chroma row (py + row) >> 1 from the chroma pointer, and its iw
// pixels (iw odd or even) the cs = (px + iw + 1) >> 1 samples from the one of its first pixel: the
// last is sample (x0 + iw - 1) >> 1 of the frame, inside it because the rectangle is.
template <typename P>
__device__ __forceinline__ void lb_stage_row(const LetterboxArgs& a, const FrameNv12T<P>& img, int row, uint8_t* dst) {
    lb_stage(dst, img.y + (size_t)row * a.pitch, a.iw);
    if constexpr (P::rect)
        lb_stage(dst + FrameNv12T<P>::luma_bytes(a.iw), img.uv + (size_t)((img.py + row) >> 1) * a.pitch,
                 2 * ((img.px + a.iw + 1) >> 1));
    else
        lb_stage(dst + FrameNv12::row_bytes(a.iw) / 2, img.uv + (size_t)(row >> 1) * a.pitch, a.iw);   // iw is even
}
template <typename P>
__device__ __forceinline__ void lb_stage_row(const LetterboxArgs& a, const FrameYuvT<P>& img, int row, uint8_t* dst) {
    const int c0 = FrameYuv::luma_bytes(a.iw);
    if constexpr (P::rect) {
        const size_t cr = (size_t)((img.py + row) >> 1) * img.cpitch;
        const int cs = (img.px + a.iw + 1) >> 1;
        lb_stage(dst, img.y + (size_t)row * a.pitch, a.iw);
        if (img.step == 2) {
            lb_stage(dst + c0, (img.u < img.v ? img.u : img.v) + cr, 2 * cs);
        } else {
            lb_stage(dst + c0, img.u + cr, cs);
            lb_stage(dst + c0 + (FrameYuvT<P>::row_bytes(a.iw) - c0) / 2, img.v + cr, cs);
        }
    } else {
        const size_t cr = (size_t)(row >> 1) * img.cpitch;
        lb_stage(dst, img.y + (size_t)row * a.pitch, a.iw);
        if (img.step == 2) {
            lb_stage(dst + c0, (img.u < img.v ? img.u : img.v) + cr, a.iw);
        } else {
            lb_stage(dst + c0, img.u + cr, a.iw / 2);   // iw is even
            lb_stage(dst + c0 + (FrameYuv::row_bytes(a.iw) - c0) / 2, img.v + cr, a.iw / 2);
        }
    }
}

// n words of a source row into LDS as the n bytes (word >> sh) & 255: 16-B loads (8 words, 8 bytes
// out) where the row start is aligned
__device__ __forceinline__ void lb_stage16(uint8_t* dst, const uint8_t* src, int n, int sh) {
    if (((uintptr_t)src & 15) == 0) {
        const int nch = (n + 7) / 8;
        for (int i = threadIdx.x; i < nch; i += 256) {
            if (8 * i + 8 <= n) {
                const uint4 v = *(const uint4*)(src + 16 * i);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = ((w[k] >> sh) & 255u) | (((w[k] >> (16 + sh)) & 255u) << 8);
                *(uint2*)(dst + 8 * i) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
            } else {
                for (int x = 8 * i; x < n; ++x) dst[x] = (uint8_t)FrameYuv16::s8(src + 2 * x, sh);
            }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) dst[i] = (uint8_t)FrameYuv16::s8(src + 2 * i, sh);
    }
}
template <typename P>
__device__ __forceinline__ void lb_stage_row(const LetterboxArgs& a, const FrameYuv16T<P>& img, int row, uint8_t* dst) {
    const int c0 = FrameYuv::luma_bytes(a.iw);
    if constexpr (P::rect) {   // as above, in words
        const size_t cr = (size_t)((img.py + row) >> 1) * img.cpitch;
        const int cs = (img.px + a.iw + 1) >> 1;
        lb_stage16(dst, img.y + (size_t)row * a.pitch, a.iw, img.sh);
        if (img.step == 2) {
            lb_stage16(dst + c0, (img.u < img.v ? img.u : img.v) + cr, 2 * cs, img.sh);
        } else {
            lb_stage16(dst + c0, img.u + cr, cs, img.sh);
            lb_stage16(dst + c0 + (FrameYuvT<P>::row_bytes(a.iw) - c0) / 2, img.v + cr, cs, img.sh);
        }
    } else {
        const size_t cr = (size_t)(row >> 1) * img.cpitch;
        lb_stage16(dst, img.y + (size_t)row * a.pitch, a.iw, img.sh);
        if (img.step == 2) {
            lb_stage16(dst + c0, (img.u < img.v ? img.u : img.v) + cr, a.iw, img.sh);
        } else {
            lb_stage16(dst + c0, img.u + cr, a.iw / 2, img.sh);
            lb_stage16(dst + c0 + (FrameYuv::row_bytes(a.iw) - c0) / 2, img.v + cr, a.iw / 2, img.sh);
        }
    }
}

// block row Y of canvas f from the frame at img; lrow: 4 staged rows of RS bytes
template <int NV, bool R = false>
__device__ __forceinline__ void lb_s2d_lds_row(const LetterboxArgs& a, const typename SrcOf<NV, R>::Frame& img, int f, int Y,
                                               uint8_t* lrow) {
    const int OW = a.ow / 2 + 1, OH = a.oh / 2 + 1;
    int rows[4];
    Tap ty[2];
    bool rin[2];
    lb_src_rows(a, 2 * Y - 1, &rows[0], &rows[1], &ty[0], &rin[0]);
    lb_src_rows(a, 2 * Y, &rows[2], &rows[3], &ty[1], &rin[1]);
    const int RS = SrcOf<NV, R>::Frame::row_bytes(a.iw);
    auto row_at = [&](int k) {
        if constexpr (R && NV != 0) return lb_rect_row_at<NV>(a, lrow, k, RS, img.px);
        else return lb_row<NV>(a, lrow, k, RS);
    };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (rows[k] < 0) continue;
        lb_stage_row(a, img, rows[k], lrow + k * RS);
    }
    __syncthreads();
    for (int X = threadIdx.x; X < OW; X += 256) {
        float t[16];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int h = s >> 1;
            const int x = 2 * X + (s & 1) - 1;
            float v[3] = {0.f, 0.f, 0.f};   // conv zero padding outside the canvas
            const int y = 2 * Y + h - 1;
            if ((unsigned)y < (unsigned)a.oh && (unsigned)x < (unsigned)a.ow)
                lb_px_lds(a, row_at(2 * h), row_at(2 * h + (rows[2 * h + 1] >= 0 ? 1 : 0)),
                          ty[h], x, rin[h], v);
            t[4 * s + 0] = v[0]; t[4 * s + 1] = v[1]; t[4 * s + 2] = v[2];
            t[4 * s + 3] = 0.f;
        }
        store_s2d(a, ((size_t)f * OH + Y) * OW + X, t);
    }
}

template <int NV>
__global__ __launch_bounds__(256) void letterbox_s2d_lds_kernel(LetterboxArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lrow[];   // 4 staged rows of RS bytes
    const int f = blockIdx.y;
    lb_s2d_lds_row<NV>(a, lb_frame<NV>(a, f), f, blockIdx.x, lrow);
}

// Two space-to-depth canvases of the same frames in one pass (the face and the
// plate letterbox of vd_process): both resize to the same nw x nh with the same
// filter, so a source row feeds block row Y of canvas a and block row Y - dY of
// canvas b; each source row is staged once and both canvases are written from it.
// Per pixel the arithmetic is exactly letterbox_s2d_lds_kernel's for each canvas.
// Block rows Y run over the union [y0, y0 + gridDim.x), X over [x0, x0 + nx).
template <int NV>
__global__ __launch_bounds__(256) void letterbox_s2d_pair_kernel(LetterboxArgs a, LetterboxArgs b, int dY, int dX,
                                                                 int y0, int x0, int nx) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lrow[];
    const int Y = y0 + (int)blockIdx.x, f = blockIdx.y;
    const int Yb = Y - dY;
    const int OWa = a.ow / 2 + 1, OHa = a.oh / 2 + 1, OWb = b.ow / 2 + 1, OHb = b.oh / 2 + 1;
    const bool ya = (unsigned)Y < (unsigned)OHa, yb = (unsigned)Yb < (unsigned)OHb;
    const typename SrcOf<NV>::Frame img = lb_frame<NV>(a, f);
    int ra[4] = {-1, -1, -1, -1}, rb[4] = {-1, -1, -1, -1};
    Tap tya[2], tyb[2];
    bool rina[2] = {false, false}, rinb[2] = {false, false};
    if (ya) {
        lb_src_rows(a, 2 * Y - 1, &ra[0], &ra[1], &tya[0], &rina[0]);
        lb_src_rows(a, 2 * Y, &ra[2], &ra[3], &tya[1], &rina[1]);
    }
    if (yb) {
        lb_src_rows(b, 2 * Yb - 1, &rb[0], &rb[1], &tyb[0], &rinb[0]);
        lb_src_rows(b, 2 * Yb, &rb[2], &rb[3], &tyb[1], &rinb[1]);
    }
    const int RS = SrcOf<NV>::Frame::row_bytes(a.iw);
    const bool st1[2] = {ra[1] >= 0 || rb[1] >= 0, ra[3] >= 0 || rb[3] >= 0};   // second rows staged
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = ra[k] >= 0 ? ra[k] : rb[k];   // the same source row when both canvases need one
        if (row < 0) continue;
        lb_stage_row(a, img, row, lrow + k * RS);
    }
    __syncthreads();
    for (int X = x0 + (int)threadIdx.x; X < x0 + nx; X += 256) {
#pragma unroll
        for (int cv = 0; cv < 2; ++cv) {
            const LetterboxArgs& c = cv ? b : a;
            const int XX = cv ? X - dX : X, YY = cv ? Yb : Y;
            if (!(cv ? yb : ya) || (unsigned)XX >= (unsigned)(cv ? OWb : OWa)) continue;
            const Tap* ty = cv ? tyb : tya;
            const bool* rin = cv ? rinb : rina;
            float t[16];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int h = s >> 1;
                const int x = 2 * XX + (s & 1) - 1;
                float v[3] = {0.f, 0.f, 0.f};
                const int y = 2 * YY + h - 1;
                if ((unsigned)y < (unsigned)c.oh && (unsigned)x < (unsigned)c.ow)
                    lb_px_lds(c, lb_row<NV>(c, lrow, 2 * h, RS), lb_row<NV>(c, lrow, 2 * h + (st1[h] ? 1 : 0), RS), ty[h], x,
                              rin[h], v);
                t[4 * s + 0] = v[0]; t[4 * s + 1] = v[1]; t[4 * s + 2] = v[2];
                t[4 * s + 3] = 0.f;
            }
            store_s2d(c, ((size_t)f * (cv ? OHb : OHa) + YY) * (cv ? OWb : OWa) + XX, t);   // bf16, fp16 or f32
        }
    }
}

template <typename Frame>
__device__ __forceinline__ void lb_nhwc_px(const LetterboxArgs& a, const Frame& img, int f, int y, int x) {
    if (x >= a.ow) return;
    float v[3];
    canvas_px(a, img, y, x, v);
    const size_t o = (((size_t)f * a.oh + y) * a.ow + x) * a.cpad;
    if (a.out_f32) {
        float* out = (float*)a.out + o;
        float4 w0 = make_float4(v[0], v[1], v[2], 0.f);
        *(float4*)out = w0;
        for (int c = 4; c < a.cpad; c += 4) *(float4*)(out + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else if (a.out_f16) {   // integers in [-123, 151]: exact in fp16 as in bf16
        _Float16* out = (_Float16*)a.out + o;
        _Float16 tmp[8];
        tmp[0] = (_Float16)v[0]; tmp[1] = (_Float16)v[1]; tmp[2] = (_Float16)v[2];
        for (int c = 3; c < 8; ++c) tmp[c] = (_Float16)0.f;
        *(uint4*)out = *(const uint4*)tmp;
        for (int c = 8; c < a.cpad; c += 8) *(uint4*)(out + c) = make_uint4(0, 0, 0, 0);
    } else {
        __bf16* out = (__bf16*)a.out + o;
        __bf16 tmp[8];
        tmp[0] = (__bf16)v[0]; tmp[1] = (__bf16)v[1]; tmp[2] = (__bf16)v[2];
        for (int c = 3; c < 8; ++c) tmp[c] = (__bf16)0.f;
        *(uint4*)out = *(const uint4*)tmp;
        for (int c = 8; c < a.cpad; c += 8) *(uint4*)(out + c) = make_uint4(0, 0, 0, 0);
    }
}

template <int NV>
__global__ __launch_bounds__(256) void letterbox_kernel(LetterboxArgs a) {
    const int f = blockIdx.z;
    lb_nhwc_px(a, lb_frame<NV>(a, f), f, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
}

// Tiled detection (tiles.hip, include/vdmi.h at vd_tiles): the n * T canvases of n frames in one
// launch, the net input on grid axis y. Input i = f * T + t is frame f's rectangle t -- the
// whole frame (t = 0, geometry w) or a tile (geometry tl, all tiles one size) -- read in place
// at the frame's pitch: a rectangle of a pitched RGB frame IS a pitched frame, so each canvas goes
// through the very device functions of the three kernels above and is bit-identical to what
// they write for a standalone frame holding those pixels. A rectangle of a 4:2:0 surface is read
// through the Rect form of its source (the origin's parities, above): its canvas is bit-identical
// to the RGB canvas of the same rectangle of the converted frame. Grid axis x: the canvas's block rows
// (space-to-depth) or rows; a workgroup walks its row 256 pixels at a time, so the source rows
// are read along the row (staged in LDS with 16-B loads where the row start is aligned).
// (block) row Y of canvas i from the rectangle at img, in the canvas form a asks for
template <int NV>
__device__ __forceinline__ void lb_rect_row(const LetterboxArgs& a, const typename SrcOf<NV, true>::Frame& img, int i, int Y,
                                            uint8_t* lrow) {
    if (a.s2d && a.iw * 3 <= LB_LDS_MAX) {
        lb_s2d_lds_row<NV, true>(a, img, i, Y, lrow);
    } else if (a.s2d) {
        for (int X = threadIdx.x; X < a.ow / 2 + 1; X += 256) lb_s2d_block(a, img, i, Y, X);
    } else {
        for (int x = threadIdx.x; x < a.ow; x += 256) lb_nhwc_px(a, img, i, Y, x);
    }
}

template <int NV>
__global__ __launch_bounds__(256) void letterbox_tiles_kernel(LetterboxArgs w, LetterboxArgs tl, TileGrid g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lrow[];
    const int i = blockIdx.y, f = i / g.T, t = i - f * g.T;
    const LetterboxArgs& a = t ? tl : w;
    if constexpr (NV == 0) {
        const FrameRgb img{w.src + ((size_t)f * w.ih + g.y0[t]) * w.pitch + (size_t)g.x0[t] * 3, w.pitch};
        lb_rect_row<0>(a, img, i, blockIdx.x, lrow);
    } else {
        lb_rect_row<NV>(a, lb_rect<NV>(w, f, g.y0[t], g.x0[t]), i, blockIdx.x, lrow);
    }
}

// The tile-only form (tiled plate detection: the plate letterbox's canvas size follows the
// rectangle's aspect, so the whole frame's canvas can differ from the tiles' and is written by
// the plain kernels): canvas i = f * (T - 1) + (t - 1) is tile t >= 1 of frame f (fh rows).
template <int NV>
__global__ __launch_bounds__(256) void letterbox_tile_inputs_kernel(LetterboxArgs tl, TileGrid g, int fh) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lrow[];
    const int RC = g.T - 1;
    const int i = blockIdx.y, f = i / RC, t = 1 + i - f * RC;
    if constexpr (NV == 0) {
        const FrameRgb img{tl.src + ((size_t)f * fh + g.y0[t]) * tl.pitch + (size_t)g.x0[t] * 3, tl.pitch};
        lb_rect_row<0>(tl, img, i, blockIdx.x, lrow);
    } else {
        lb_rect_row<NV>(tl, lb_rect<NV>(tl, f, g.y0[t], g.x0[t]), i, blockIdx.x, lrow);
    }
}

// NHWC max-pool (torch semantics: padded taps ignored), vectorised 16 B per thread.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* x, int xh, int xw, int ldx, int xcoff,
                                                      T* y, int yh, int yw, int ldy, int ycoff,
                                                      int c, int k, int s, int p, int total) {
    constexpr int VEC = 16 / sizeof(T);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cv = c / VEC;
    const int ci = (idx % cv) * VEC;
    int pix = idx / cv;
    const int ox = pix % yw; pix /= yw;
    const int oy = pix % yh;
    const int b = pix / yh;
    float m[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) m[e] = -__builtin_huge_valf();
    for (int dy = 0; dy < k; ++dy) {
        int iy = oy * s - p + dy;
        if ((unsigned)iy >= (unsigned)xh) continue;
        for (int dx = 0; dx < k; ++dx) {
            int ix = ox * s - p + dx;
            if ((unsigned)ix >= (unsigned)xw) continue;
            uint4 u = *(const uint4*)(x + (((size_t)b * xh + iy) * xw + ix) * ldx + xcoff + ci);
            const T* t = (const T*)&u;
#pragma unroll
            for (int e = 0; e < VEC; ++e) m[e] = fmaxf(m[e], (float)t[e]);
        }
    }
    T o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = (T)m[e];
    *(uint4*)(y + (((size_t)b * yh + oy) * yw + ox) * ldy + ycoff + ci) = *(const uint4*)o;
}

// Nearest 2x upsample into a channel slice (ultralytics nn.Upsample + Concat).
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_kernel(const T* x, int xh, int xw, int ldx, int xcoff,
                                                         T* y, int ldy, int ycoff, int c, int total) {
    constexpr int VEC = 16 / sizeof(T);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cv = c / VEC;
    const int ci = (idx % cv) * VEC;
    int pix = idx / cv;
    const int yw = 2 * xw, yh = 2 * xh;
    const int ox = pix % yw; pix /= yw;
    const int oy = pix % yh;
    const int b = pix / yh;
    uint4 u = *(const uint4*)(x + (((size_t)b * xh + (oy >> 1)) * xw + (ox >> 1)) * ldx + xcoff + ci);
    *(uint4*)(y + (((size_t)b * yh + oy) * yw + ox) * ldy + ycoff + ci) = u;
}

}  // namespace

// Same frames, both 16-bit (bf16 / fp16) space-to-depth canvases, the same resize
// (nw, nh, filter) and even relative offsets of the pasted images.
// bytes of one staged source row (RGB: the pixels; NV12: the luma row and its chroma row, 16-B aligned each);
// at most LB_LDS_MAX whenever iw * 3 <= LB_LDS_MAX
// (rect: a rectangle source of the tile letterbox, whose chroma segments hold iw / 2 + 1 samples)
static size_t lb_row_bytes(const LetterboxArgs& a, bool rect = false) {
    const int cs = rect ? a.iw / 2 + 1 : a.iw / 2;
    if (a.nv.on == 2 || a.nv.on == 3) return (size_t)((a.iw + 15) / 16 * 16) + 2 * (size_t)((cs + 15) / 16 * 16);   // FrameYuvT::row_bytes
    if (a.nv.on && rect) return (size_t)((a.iw + 15) / 16 * 16) + (size_t)((2 * cs + 15) / 16 * 16);               // FrameNv12T<Rect>::row_bytes
    return a.nv.on ? 2 * (size_t)((a.iw + 15) / 16 * 16) : (size_t)((a.iw * 3 + 15) / 16 * 16);
}

// a launch of kernel K<nv.on>(args...): the instantiation for the frames' pixel source
#define LB_LAUNCH(K, on, grid, lds, s, ...)                                                          \
    do {                                                                                             \
        if ((on) == 3) hipLaunchKernelGGL(K<3>, grid, dim3(256), lds, s, __VA_ARGS__);               \
        else if ((on) == 2) hipLaunchKernelGGL(K<2>, grid, dim3(256), lds, s, __VA_ARGS__);          \
        else if ((on) == 1) hipLaunchKernelGGL(K<1>, grid, dim3(256), lds, s, __VA_ARGS__);          \
        else hipLaunchKernelGGL(K<0>, grid, dim3(256), lds, s, __VA_ARGS__);                         \
    } while (0)

bool vd_letterbox_pair_ok(const LetterboxArgs& a, const LetterboxArgs& b) {
    return a.s2d && b.s2d && a.src == b.src && a.n == b.n && a.nv.on == b.nv.on &&
           a.ih == b.ih && a.iw == b.iw && a.pitch == b.pitch && a.iw * 3 <= LB_LDS_MAX && a.nw == b.nw &&
           a.nh == b.nh && a.mode == b.mode && a.scale_x == b.scale_x && a.scale_y == b.scale_y &&
           ((a.top - b.top) & 1) == 0 && ((a.left - b.left) & 1) == 0;
}

// linear_tap on the host (the same IEEE round-to-nearest operations as the device): source
// column s0 and second weight a1 of resized column d
static void lb_tap_host(int d, int ssize, double scale, int* s0, int* a1) {
    float f = (float)((((double)d + 0.5) * scale) - 0.5);
    int s = (int)std::floor(f);
    f = f - (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    *s0 = s;
    *a1 = (int)std::nearbyint(f * 2048.0f);
}

// LB_LINEAR columns that are an exact affine gather (every a1 = 0, s0 = k d + c): the kernels'
// gather fast path (checked over every resized column, so it is exact by construction)
static void lb_set_gather(LetterboxArgs& a) {
    a.gx_k = a.gx_c = 0;
    if (a.mode != LB_LINEAR || a.nw < 2) return;
    int s0, s1, a1;
    lb_tap_host(0, a.iw, a.scale_x, &s0, &a1);
    lb_tap_host(1, a.iw, a.scale_x, &s1, &a1);
    const int k = s1 - s0, c = s0;
    if (k <= 0) return;
    for (int d = 0; d < a.nw; ++d) {
        lb_tap_host(d, a.iw, a.scale_x, &s0, &a1);
        if (a1 != 0 || s0 != k * d + c) return;
    }
    a.gx_k = k;
    a.gx_c = c;
}

hipError_t vd_launch_letterbox_pair(const LetterboxArgs& a0, const LetterboxArgs& b0, hipStream_t s) {
    LetterboxArgs a = a0, b = b0;
    lb_set_gather(a);
    lb_set_gather(b);
    if (!vd_letterbox_pair_ok(a, b)) return hipErrorInvalidValue;
    static const bool attr = [] {
        (void)hipFuncSetAttribute((const void*)letterbox_s2d_pair_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_s2d_pair_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_s2d_pair_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_s2d_pair_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        return true;
    }();
    (void)attr;
    const int dY = (a.top - b.top) / 2, dX = (a.left - b.left) / 2;
    const int y0 = std::min(0, dY), y1 = std::max(a.oh / 2 + 1, b.oh / 2 + 1 + dY);
    const int x0 = std::min(0, dX), x1 = std::max(a.ow / 2 + 1, b.ow / 2 + 1 + dX);
    const size_t lds = 4 * lb_row_bytes(a);
    LB_LAUNCH(letterbox_s2d_pair_kernel, a.nv.on, dim3(y1 - y0, a.n), lds, s, a, b, dY, dX, y0, x0, x1 - x0);
    return hipGetLastError();
}

hipError_t vd_launch_letterbox(const LetterboxArgs& a0, hipStream_t s) {
    LetterboxArgs a = a0;
    lb_set_gather(a);
    if (a.s2d && a.iw * 3 <= LB_LDS_MAX) {
        static const bool attr = [] {
            (void)hipFuncSetAttribute((const void*)letterbox_s2d_lds_kernel<0>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 4 * LB_LDS_MAX);
            (void)hipFuncSetAttribute((const void*)letterbox_s2d_lds_kernel<1>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 4 * LB_LDS_MAX);
            (void)hipFuncSetAttribute((const void*)letterbox_s2d_lds_kernel<2>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 4 * LB_LDS_MAX);
            (void)hipFuncSetAttribute((const void*)letterbox_s2d_lds_kernel<3>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 4 * LB_LDS_MAX);
            return true;
        }();
        (void)attr;
        const size_t lds = 4 * lb_row_bytes(a);
        dim3 grid(a.oh / 2 + 1, a.n);
        LB_LAUNCH(letterbox_s2d_lds_kernel, a.nv.on, grid, lds, s, a);
        return hipGetLastError();
    }
    if (a.s2d) {
        dim3 grid((a.ow / 2 + 1 + 255) / 256, a.oh / 2 + 1, a.n);
        LB_LAUNCH(letterbox_s2d_kernel, a.nv.on, grid, 0, s, a);
        return hipGetLastError();
    }
    dim3 grid((a.ow + 255) / 256, a.oh, a.n);
    LB_LAUNCH(letterbox_kernel, a.nv.on, grid, 0, s, a);
    return hipGetLastError();
}

// a 4:2:0 source of the tile letterbox: both geometries read the same surfaces, frames of even h x w
static bool lb_tiles_src_ok(const LetterboxArgs& t, int fh, int fw) {
    if (t.nv.on < 0 || t.nv.on > 3) return false;
    if (!t.nv.on) return true;
    if ((fh & 1) || (fw & 1) || t.pitch < (size_t)fw * (t.nv.on == 3 ? 2 : 1)) return false;
    if (t.nv.on == 1) return true;
    return (t.nv.step == 1 || t.nv.step == 2) && t.nv.cpitch >= (size_t)(fw / 2) * t.nv.step * (t.nv.on == 3 ? 2 : 1);
}

hipError_t vd_launch_letterbox_tiles(const LetterboxArgs& w0, const LetterboxArgs& t0, const TileGrid& g,
                                     hipStream_t s) {
    LetterboxArgs w = w0, t = t0;
    if (w.nv.on != t.nv.on || !lb_tiles_src_ok(w, w.ih, w.iw)) return hipErrorInvalidValue;
    if (w.nv.on && (w.src != t.src || w.pitch != t.pitch)) return hipErrorInvalidValue;
    if (g.T < 2 || g.T > VD_TILE_INPUTS_MAX || w.n <= 0 || w.s2d != t.s2d || w.oh != t.oh || w.ow != t.ow ||
        t.ih != g.th || t.iw != g.tw)
        return hipErrorInvalidValue;
    for (int k = 0; k < g.T; ++k)   // every rectangle inside the frame
        if (g.x0[k] < 0 || g.y0[k] < 0 || g.x0[k] + (k ? g.tw : w.iw) > w.iw || g.y0[k] + (k ? g.th : w.ih) > w.ih)
            return hipErrorInvalidValue;
    lb_set_gather(w);
    lb_set_gather(t);
    static const bool attr = [] {
        (void)hipFuncSetAttribute((const void*)letterbox_tiles_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_tiles_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_tiles_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_tiles_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        return true;
    }();
    (void)attr;
    size_t lds = 0;
    if (w.s2d)
        for (const LetterboxArgs* a : {&w, &t})
            if (a->iw * 3 <= LB_LDS_MAX) lds = std::max(lds, 4 * lb_row_bytes(*a, true));
    const dim3 grid(w.s2d ? w.oh / 2 + 1 : w.oh, w.n * g.T);
    LB_LAUNCH(letterbox_tiles_kernel, w.nv.on, grid, lds, s, w, t, g);
    return hipGetLastError();
}

hipError_t vd_launch_letterbox_tile_inputs(const LetterboxArgs& t0, const TileGrid& g, int n, int fh, int fw,
                                           hipStream_t s) {
    LetterboxArgs t = t0;
    if (!lb_tiles_src_ok(t, fh, fw)) return hipErrorInvalidValue;
    if (g.T < 2 || g.T > VD_TILE_INPUTS_MAX || n <= 0 || t.ih != g.th || t.iw != g.tw ||
        (!t.nv.on && t.pitch < (size_t)fw * 3))
        return hipErrorInvalidValue;
    for (int k = 1; k < g.T; ++k)   // every tile inside the frame
        if (g.x0[k] < 0 || g.y0[k] < 0 || g.x0[k] + g.tw > fw || g.y0[k] + g.th > fh) return hipErrorInvalidValue;
    lb_set_gather(t);
    static const bool attr = [] {
        (void)hipFuncSetAttribute((const void*)letterbox_tile_inputs_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_tile_inputs_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_tile_inputs_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)letterbox_tile_inputs_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * LB_LDS_MAX);
        return true;
    }();
    (void)attr;
    const size_t lds = t.s2d && t.iw * 3 <= LB_LDS_MAX ? 4 * lb_row_bytes(t, true) : 0;
    const dim3 grid(t.s2d ? t.oh / 2 + 1 : t.oh, n * (g.T - 1));
    LB_LAUNCH(letterbox_tile_inputs_kernel, t.nv.on, grid, lds, s, t, g, fh);
    return hipGetLastError();
}

hipError_t vd_launch_maxpool(bool f32, bool f16, const void* x, int n, int xh, int xw, int ldx, int xcoff,
                             void* y, int yh, int yw, int ldy, int ycoff, int c, int k, int st, int p,
                             hipStream_t s) {
    const int vec = f32 ? 4 : 8;
    const int total = n * yh * yw * (c / vec);
    dim3 grid((total + 255) / 256);
    if (f32)
        hipLaunchKernelGGL(maxpool_kernel<float>, grid, dim3(256), 0, s, (const float*)x, xh, xw, ldx, xcoff,
                           (float*)y, yh, yw, ldy, ycoff, c, k, st, p, total);
    else if (f16)
        hipLaunchKernelGGL(maxpool_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)x, xh, xw, ldx, xcoff,
                           (_Float16*)y, yh, yw, ldy, ycoff, c, k, st, p, total);
    else
        hipLaunchKernelGGL(maxpool_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)x, xh, xw, ldx, xcoff,
                           (__bf16*)y, yh, yw, ldy, ycoff, c, k, st, p, total);
    return hipGetLastError();
}

// (a pure copy: the bf16 instantiation moves fp16 bits unchanged)
hipError_t vd_launch_upsample2x(bool f32, const void* x, int n, int xh, int xw, int ldx, int xcoff,
                                void* y, int ldy, int ycoff, int c, hipStream_t s) {
    const int vec = f32 ? 4 : 8;
    const int total = n * 4 * xh * xw * (c / vec);
    dim3 grid((total + 255) / 256);
    if (f32)
        hipLaunchKernelGGL(upsample2x_kernel<float>, grid, dim3(256), 0, s, (const float*)x, xh, xw, ldx, xcoff,
                           (float*)y, ldy, ycoff, c, total);
    else
        hipLaunchKernelGGL(upsample2x_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)x, xh, xw, ldx, xcoff,
                           (__bf16*)y, ldy, ycoff, c, total);
    return hipGetLastError();
}

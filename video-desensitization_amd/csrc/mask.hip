// mask.hip — mask shaping (vd_mask): the boxes a context blurs are grown by a margin and,
// under VD_MASK_ELLIPSE, only the ellipse inscribed in each grown box stays hidden.
//
// Definition (include/vdmi.h at vd_mask, DESIGN.md "Mask shaping"), integers only:
//   grow(b, g)   W = x2 - x1, H = y2 - y1 (64-bit); W <= 0 or H <= 0: b as stored. Otherwise
//                gx = (W*g + 199) / 200, gy = (H*g + 199) / 200 (the ceiling of half the
//                growth), b' = (x1-gx, y1-gy, x2+gx, y2+gy), each coordinate clamped to
//                [-2^30, 2^30].
//   ellipse      pixel (x, y) of b' clipped to the frame is inside iff
//                dx*dx*H*H + dy*dy*W*W <= W*W*H*H, dx = 2x+1-(x1+x2), dy = 2y+1-(y1+y2), W and H
//                of the unclipped b'. Inside the clipped box |dx| <= W and |dy| <= H, so with
//                W, H <= 32768 every term is at most 2^60 and the sum at most 2^61. A box with
//                W > 32768 or H > 32768 is inside everywhere in its clipped rectangle.
//   composite    the rectangular pass (mosaic.hip / blur.hip, unchanged) runs on the grown lists
//                and gives R; out(p) = R(p) where p is inside some box's ellipse, in(p) elsewhere.
//
// mask_grow_kernel: the one or two input lists of a frame (as MosaicArgs takes them, counts
// clamped to cap the same way) -> one merged row of grown boxes and its count. Grid (blocks of
// 256 boxes of the row capacity) x frames: sized from n and the capacities alone.
//
// mask_restore_kernel, after the rectangular pass on the same stream: one workgroup of 256
// threads (4 waves) per (frame, band of BR rows); the grid depends on n and h only. The
// workgroup compacts the boxes whose clipped rectangle meets the band into LDS (at most BCAP;
// the composite does not depend on their order) and finds, once per (box, band row), the span
// of columns inside the ellipse from the predicate itself:
//   q = floor((W*W*H*H - dy*dy*W*W) / (H*H)),  s = floor(sqrt(q)):   inside <=> dx*dx <= q <=> |dx| <= s
// (H*H > 0 and dx*dx is an integer, so the floor loses nothing; the numerator is positive since
// |dy| < H inside the box; s by a 16-step integer bit search). A wave then takes a (box, row) at
// a time, its lanes the row's columns left and right of that span: such a pixel, when it lies in
// no other band box's span of the row either, is copied in -> out, 3 bytes. Two boxes restoring
// one pixel write the same bytes, and nothing else of `out` is touched, so the order of the
// waves cannot matter. A band meeting more than BCAP boxes walks the frame's global row
// instead, with the predicate as written in the definition; no box is dropped.
#include "vd_kernel.h"
#include "vdmi.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int BR = 16;                 // rows per band
constexpr int BCAP = 64;               // band-list capacity; fuller bands walk the global row
constexpr int ROW_NONE = 0x7fffffff;   // span start of a band row outside the box's clipped rectangle
constexpr int COORD_MAX = 1 << 30;

__device__ __forceinline__ int frame_boxes(const MaskArgs& a, int f, int& n0) {
    n0 = a.cnt0 ? min(max(a.cnt0[f], 0), a.cap0) : 0;
    const int n1 = a.cnt1 ? min(max(a.cnt1[f], 0), a.cap1) : 0;
    return n0 + n1;
}

__device__ __forceinline__ int clamp_coord(long long v) {
    return (int)min(max(v, -(long long)COORD_MAX), (long long)COORD_MAX);
}

__device__ __forceinline__ int4 grow_box(int4 b, int g) {
    const long long W = (long long)b.z - b.x, H = (long long)b.w - b.y;
    if (W <= 0 || H <= 0) return b;
    const long long gx = (W * g + 199) / 200, gy = (H * g + 199) / 200;
    return make_int4(clamp_coord(b.x - gx), clamp_coord(b.y - gy), clamp_coord(b.z + gx), clamp_coord(b.w + gy));
}

__global__ __launch_bounds__(THREADS) void mask_grow_kernel(MaskArgs a) {
    const int per = (a.mcap + THREADS - 1) / THREADS;  // blocks per frame
    const int f = blockIdx.x / per;
    const int k = (blockIdx.x % per) * THREADS + threadIdx.x;
    int n0;
    const int nb = frame_boxes(a, f, n0);              // <= cap0 + cap1 <= mcap (launcher)
    if (k == 0) a.m_cnt[f] = nb;
    if (k >= a.mcap) return;
    int4* row = (int4*)a.m_xy + (size_t)f * a.mcap;
    if (k < nb) {
        const int* src = k < n0 ? a.xy0 + ((size_t)f * a.cap0 + k) * 4 : a.xy1 + ((size_t)f * a.cap1 + (k - n0)) * 4;
        row[k] = grow_box(make_int4(src[0], src[1], src[2], src[3]), a.g);
    } else if (a.zero_tail) {
        row[k] = make_int4(0, 0, 0, 0);                // vd_mask_boxes copies whole rows out
    }
}

// combine_detect.py:145-148 clip, :150-151 empty check, as the rectangular passes clip
__device__ __forceinline__ bool clip_box(int4 b, int w, int h, int4& c) {
    c = make_int4(max(0, b.x), max(0, b.y), min(w, b.z), min(h, b.w));
    return c.z > c.x && c.w > c.y;
}

// the definition's predicate for a pixel inside b's clipped rectangle
__device__ __forceinline__ bool in_ellipse(int4 b, int x, int y) {
    const long long W = (long long)b.z - b.x, H = (long long)b.w - b.y;
    if (W > 32768 || H > 32768) return true;
    const long long dx = 2LL * x + 1 - ((long long)b.x + b.z), dy = 2LL * y + 1 - ((long long)b.y + b.w);
    return dx * dx * H * H + dy * dy * W * W <= W * W * H * H;
}

// floor(sqrt(q)) for q <= 2^30, bit by bit
__device__ __forceinline__ int isqrt30(long long q) {
    unsigned r = 0;
    for (unsigned bit = 1u << 15; bit; bit >>= 1) {
        const unsigned t = r | bit;
        if ((long long)t * t <= q) r = t;
    }
    return (int)r;
}

// [xl, xr): the columns of row y of b's clipped rectangle c that are inside b's ellipse (header);
// xl = ROW_NONE when y is not a row of c
__device__ __forceinline__ void row_span(int4 b, int4 c, int y, int& xl, int& xr) {
    xl = xr = ROW_NONE;
    if (y < c.y || y >= c.w) return;
    xl = c.x; xr = c.z;
    const long long W = (long long)b.z - b.x, H = (long long)b.w - b.y;
    if (W > 32768 || H > 32768) return;               // inside everywhere
    const long long dy = 2LL * y + 1 - ((long long)b.y + b.w), sx = (long long)b.x + b.z;
    const long long s = isqrt30((W * W * H * H - dy * dy * W * W) / (H * H));
    // |2x + 1 - sx| <= s  <=>  ceil((sx - 1 - s) / 2) <= x <= floor((sx - 1 + s) / 2); >> 1 floors
    const long long lo = (sx - s) >> 1, hi = ((sx - 1 + s) >> 1) + 1;
    xl = (int)min(max(lo, (long long)c.x), (long long)c.z);
    xr = (int)max(min(hi, (long long)c.z), (long long)xl);
}

__device__ __forceinline__ void restore_px(const MaskArgs& a, int f, int x, int y) {
    const size_t o = ((size_t)f * a.h + y) * a.pitch + (size_t)x * 3;
    a.out[o] = a.in[o];
    a.out[o + 1] = a.in[o + 1];
    a.out[o + 2] = a.in[o + 2];
}

__global__ __launch_bounds__(THREADS) void mask_restore_kernel(MaskArgs a) {
    __shared__ int4 s_box[BCAP];                       // grown boxes meeting the band, unclipped
    // per (band row, band box): the columns inside its ellipse; a row's boxes lie side by side
    // so that the test of a pixel against all of them reads 16-B vectors
    __shared__ __attribute__((aligned(16))) int s_xl[BR][BCAP], s_xr[BR][BCAP];
    __shared__ int s_n;
    const int bands = (a.h + BR - 1) / BR;
    const int f = blockIdx.x / bands, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int by0 = (blockIdx.x % bands) * BR, by1 = min(by0 + BR, a.h);
    const int nb = min(max(a.m_cnt[f], 0), a.mcap);
    const int4* row = (const int4*)a.m_xy + (size_t)f * a.mcap;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int k = tid; k < nb; k += THREADS) {
        const int4 b = row[k];
        int4 c;
        if (clip_box(b, a.w, a.h, c) && c.y < by1 && c.w > by0) {
            const int i = atomicAdd(&s_n, 1);
            if (i < BCAP) s_box[i] = b;
        }
    }
    __syncthreads();
    const int nt = s_n;                                // uniform over the workgroup
    if (nt == 0) return;

    if (nt <= BCAP) {
        const int nt4 = (nt + 3) & ~3;                 // the list padded to whole vectors with empty spans
        for (int p = tid; p < nt4 * BR; p += THREADS) {
            const int k = p % nt4, r = p / nt4;
            int xl = ROW_NONE, xr = ROW_NONE;
            if (k < nt) {
                const int4 b = s_box[k];
                int4 c;
                clip_box(b, a.w, a.h, c);
                row_span(b, c, by0 + r, xl, xr);
            }
            s_xl[r][k] = xl;
            s_xr[r][k] = xr;
        }
        __syncthreads();
        for (int p = wid; p < nt * BR; p += WAVES) {
            const int k = p / BR, r = p % BR;
            const int xl = s_xl[r][k], xr = s_xr[r][k];
            if (xl == ROW_NONE) continue;              // not a row of this box
            const int4 b = s_box[k];
            const int y = by0 + r;
            const int cx1 = max(0, b.x), cx2 = min(a.w, b.z);
            // the row's pixels outside its own ellipse: [cx1, xl) and [xr, cx2)
            const int nl = xl - cx1, no = nl + (cx2 - xr);
            for (int i = lane; i < no; i += 64) {
                const int x = i < nl ? cx1 + i : xr + (i - nl);
                // its own span does not hold x and ROW_NONE holds nothing; no early exit, so
                // the LDS reads of the whole list are in flight together
                const int4* vl = (const int4*)s_xl[r];
                const int4* vr = (const int4*)s_xr[r];
                bool hidden = false;
                for (int j = 0; j < nt4 / 4; ++j) {
                    const int4 l = vl[j], h = vr[j];
                    hidden |= (x >= l.x && x < h.x) | (x >= l.y && x < h.y) | (x >= l.z && x < h.z) |
                              (x >= l.w && x < h.w);
                }
                if (!hidden) restore_px(a, f, x, y);
            }
        }
        return;
    }

    // more boxes than the LDS list holds: the same composite from the global row
    for (int k = 0; k < nb; ++k) {
        const int4 b = row[k];
        int4 c;
        if (!clip_box(b, a.w, a.h, c) || c.y >= by1 || c.w <= by0) continue;
        const int y0 = max(c.y, by0), y1 = min(c.w, by1), bw = c.z - c.x;
        const long long npx = (long long)(y1 - y0) * bw;
        for (long long p = tid; p < npx; p += THREADS) {
            const int y = y0 + (int)(p / bw), x = c.x + (int)(p % bw);
            if (in_ellipse(b, x, y)) continue;
            bool hidden = false;
            for (int j = 0; j < nb && !hidden; ++j) {
                if (j == k) continue;
                const int4 o = row[j];
                int4 oc;
                if (!clip_box(o, a.w, a.h, oc) || x < oc.x || x >= oc.z || y < oc.y || y >= oc.w) continue;
                hidden = in_ellipse(o, x, y);
            }
            if (!hidden) restore_px(a, f, x, y);
        }
    }
}

// ---- NV12 frames (include/vdmi.h at vd_nv12, "ellipse") ----
// The composite on both planes after the rectangular NV12 pass (nv12.hip / smooth.hip) gave R:
//   luma    out_Y(p) = R_Y(p) where p lies in some E_k, in_Y(p) elsewhere: mask_restore_kernel's
//           pass with one byte per pixel;
//   chroma  sample (cy, cx) is hidden iff one of its four luma pixels (2cy + {0, 1}, 2cx + {0, 1})
//           lies in some E_k; out_UV = R_UV where hidden, in_UV elsewhere. In span form: a
//           non-empty span [xl, xr) of luma row 2cy or 2cy + 1 hides chroma samples
//           [xl >> 1, (xr + 1) >> 1) of row cy. Only samples of some box's chroma rectangle cc_k
//           can differ from `in`, so those are the ones tested.
// The same band per workgroup (BR luma rows, BR / 2 chroma rows; BR and h are even, so a chroma
// row's two luma rows lie in one band), the same LDS list and spans; a wave takes a (box, luma
// row) and then a (box, chroma row) at a time. Past BCAP the global row is walked with the
// predicate as written, the four-pixel rule included.
// ES: bytes per sample -- 1, or 2 for surfaces of 16-bit words (include/vdmi.h at vd_yuv420_16), whose
// restore copies whole words (pitches and offsets stay in bytes, steps in samples)
template <int ES>
__device__ __forceinline__ void restore_y(const uint8_t* in_y, uint8_t* out_y, const MaskNv12Args& a, int x, int y) {
    if constexpr (ES == 2)
        *(uint16_t*)(out_y + (size_t)y * a.out_pitch + 2 * (size_t)x) = *(const uint16_t*)(in_y + (size_t)y * a.in_pitch + 2 * (size_t)x);
    else
        out_y[(size_t)y * a.out_pitch + x] = in_y[(size_t)y * a.in_pitch + x];
}

// U and V by their offsets and steps (include/vdmi.h at vd_yuv420; NV12: V the byte after U, step 2)
struct ChromaPtrs { const uint8_t* in_u; const uint8_t* in_v; uint8_t* out_u; uint8_t* out_v; };
template <int ES>
__device__ __forceinline__ void restore_uv(const ChromaPtrs& c, const MaskNv12Args& a, int cx, int cy) {
    const size_t i = (size_t)cy * a.in_cp + (size_t)cx * a.in_step * ES, o = (size_t)cy * a.out_cp + (size_t)cx * a.out_step * ES;
    if constexpr (ES == 2) {
        *(uint16_t*)(c.out_u + o) = *(const uint16_t*)(c.in_u + i);
        *(uint16_t*)(c.out_v + o) = *(const uint16_t*)(c.in_v + i);
    } else {
        c.out_u[o] = c.in_u[i];
        c.out_v[o] = c.in_v[i];
    }
}

template <int ES>
__global__ __launch_bounds__(THREADS) void mask_restore_nv12_kernel(MaskNv12Args a) {
    __shared__ int4 s_box[BCAP];
    __shared__ __attribute__((aligned(16))) int s_xl[BR][BCAP], s_xr[BR][BCAP];
    __shared__ int s_n;
    const int bands = (a.h + BR - 1) / BR;
    const int f = blockIdx.x / bands, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int by0 = (blockIdx.x % bands) * BR, by1 = min(by0 + BR, a.h);   // both even
    const uint8_t* in_y = a.in + (size_t)f * a.in_stride;
    uint8_t* out_y = a.out + (size_t)f * a.out_stride;
    const ChromaPtrs chroma{in_y + a.in_uv, in_y + a.in_v, out_y + a.out_uv, out_y + a.out_v};
    const int nb = min(max(a.m_cnt[f], 0), a.mcap);
    const int4* row = (const int4*)a.m_xy + (size_t)f * a.mcap;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int k = tid; k < nb; k += THREADS) {
        const int4 b = row[k];
        int4 c;
        if (clip_box(b, a.w, a.h, c) && c.y < by1 && c.w > by0) {
            const int i = atomicAdd(&s_n, 1);
            if (i < BCAP) s_box[i] = b;
        }
    }
    __syncthreads();
    const int nt = s_n;                                // uniform over the workgroup
    if (nt == 0) return;

    if (nt <= BCAP) {
        const int nt4 = (nt + 3) & ~3;
        for (int p = tid; p < nt4 * BR; p += THREADS) {
            const int k = p % nt4, r = p / nt4;
            int xl = ROW_NONE, xr = ROW_NONE;
            if (k < nt) {
                const int4 b = s_box[k];
                int4 c;
                clip_box(b, a.w, a.h, c);
                row_span(b, c, by0 + r, xl, xr);
            }
            s_xl[r][k] = xl;
            s_xr[r][k] = xr;
        }
        __syncthreads();
        // luma: the pixels of a box's row outside its own span that no other span of the row holds
        for (int p = wid; p < nt * BR; p += WAVES) {
            const int k = p / BR, r = p % BR;
            const int xl = s_xl[r][k], xr = s_xr[r][k];
            if (xl == ROW_NONE) continue;
            const int4 b = s_box[k];
            const int cx1 = max(0, b.x), cx2 = min(a.w, b.z);
            const int nl = xl - cx1, no = nl + (cx2 - xr);
            for (int i = lane; i < no; i += 64) {
                const int x = i < nl ? cx1 + i : xr + (i - nl);
                const int4* vl = (const int4*)s_xl[r];
                const int4* vr = (const int4*)s_xr[r];
                bool hidden = false;
                for (int j = 0; j < nt4 / 4; ++j) {
                    const int4 l = vl[j], h = vr[j];
                    hidden |= (x >= l.x && x < h.x) | (x >= l.y && x < h.y) | (x >= l.z && x < h.z) |
                              (x >= l.w && x < h.w);
                }
                if (!hidden) restore_y<ES>(in_y, out_y, a, x, by0 + r);
            }
        }
        // chroma: the samples of a box's chroma rectangle that no span of the two luma rows hides
        // (an empty span, xl == xr or ROW_NONE, hides nothing: the l < h terms)
        for (int p = wid; p < nt * (BR / 2); p += WAVES) {
            const int k = p / (BR / 2), rc = p % (BR / 2);
            const int cy = by0 / 2 + rc;
            const int4 b = s_box[k];
            int4 c;
            clip_box(b, a.w, a.h, c);
            if (cy < (c.y >> 1) || cy >= ((c.w + 1) >> 1)) continue;   // not a row of cc_k (or past the frame)
            const int ccx2 = (c.z + 1) >> 1;
            for (int x = (c.x >> 1) + lane; x < ccx2; x += 64) {
                bool hidden = false;
                for (int r = 2 * rc; r < 2 * rc + 2; ++r) {
                    const int4* vl = (const int4*)s_xl[r];
                    const int4* vr = (const int4*)s_xr[r];
                    for (int j = 0; j < nt4 / 4; ++j) {
                        const int4 l = vl[j], h = vr[j];
                        hidden |= (l.x < h.x && x >= (l.x >> 1) && x < ((h.x + 1) >> 1)) |
                                  (l.y < h.y && x >= (l.y >> 1) && x < ((h.y + 1) >> 1)) |
                                  (l.z < h.z && x >= (l.z >> 1) && x < ((h.z + 1) >> 1)) |
                                  (l.w < h.w && x >= (l.w >> 1) && x < ((h.w + 1) >> 1));
                    }
                }
                if (!hidden) restore_uv<ES>(chroma, a, x, cy);
            }
        }
        return;
    }

    // more boxes than the LDS list holds: the same composite from the global row
    auto in_some_ellipse = [&](int x, int y, int skip) {
        for (int j = 0; j < nb; ++j) {
            if (j == skip) continue;
            const int4 o = row[j];
            int4 oc;
            if (!clip_box(o, a.w, a.h, oc) || x < oc.x || x >= oc.z || y < oc.y || y >= oc.w) continue;
            if (in_ellipse(o, x, y)) return true;
        }
        return false;
    };
    for (int k = 0; k < nb; ++k) {
        const int4 b = row[k];
        int4 c;
        if (!clip_box(b, a.w, a.h, c) || c.y >= by1 || c.w <= by0) continue;
        const int y0 = max(c.y, by0), y1 = min(c.w, by1), bw = c.z - c.x;
        const long long npx = (long long)(y1 - y0) * bw;
        for (long long p = tid; p < npx; p += THREADS) {
            const int y = y0 + (int)(p / bw), x = c.x + (int)(p % bw);
            if (in_ellipse(b, x, y)) continue;
            if (!in_some_ellipse(x, y, k)) restore_y<ES>(in_y, out_y, a, x, y);
        }
        // the band's chroma rows of cc_k: by the four luma pixels of each sample
        const int ccx1 = c.x >> 1, cbw = ((c.z + 1) >> 1) - ccx1;
        const int cy0 = max(c.y >> 1, by0 / 2), cy1 = min((c.w + 1) >> 1, by1 / 2);
        const long long ncs = (long long)(cy1 - cy0) * cbw;
        for (long long p = tid; p < ncs; p += THREADS) {
            const int cy = cy0 + (int)(p / cbw), cx = ccx1 + (int)(p % cbw);
            bool hidden = false;
            for (int q = 0; q < 4 && !hidden; ++q) hidden = in_some_ellipse(2 * cx + (q & 1), 2 * cy + (q >> 1), -1);
            if (!hidden) restore_uv<ES>(chroma, a, cx, cy);
        }
    }
}

}  // namespace

hipError_t vd_launch_mask_grow(const MaskArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.g < 0 || a.g > VD_MASK_GROW_MAX || !a.m_cnt || !a.m_xy || a.mcap <= 0)
        return hipErrorInvalidValue;
    if ((a.cnt0 ? a.cap0 : 0) + (a.cnt1 ? a.cap1 : 0) > a.mcap) return hipErrorInvalidValue;
    if ((a.cnt0 && (!a.xy0 || a.cap0 <= 0)) || (a.cnt1 && (!a.xy1 || a.cap1 <= 0))) return hipErrorInvalidValue;
    const long long blocks = (long long)((a.mcap + THREADS - 1) / THREADS) * a.n;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_grow_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t vd_launch_mask_restore(const MaskArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || a.pitch < (size_t)a.w * 3 || !a.in || !a.out || !a.m_cnt || !a.m_xy ||
        a.mcap <= 0)
        return hipErrorInvalidValue;
    const long long blocks = (long long)((a.h + BR - 1) / BR) * a.n;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_restore_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t vd_launch_mask_restore_nv12(const MaskNv12Args& a, hipStream_t s, int es1) {
    const size_t es = es1 == 2 ? 2 : 1;
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || (a.h & 1) || (a.w & 1) || a.in_pitch < (size_t)a.w * es ||
        a.out_pitch < (size_t)a.w * es || !a.in || !a.out || !a.m_cnt || !a.m_xy || a.mcap <= 0 ||
        (a.in_step != 1 && a.in_step != 2) || (a.out_step != 1 && a.out_step != 2) ||
        a.in_cp < (size_t)(a.w / 2) * a.in_step * es || a.out_cp < (size_t)(a.w / 2) * a.out_step * es)
        return hipErrorInvalidValue;
    const long long blocks = (long long)((a.h + BR - 1) / BR) * a.n;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (es == 2) {
        const uintptr_t m = (uintptr_t)a.in | (uintptr_t)a.out | a.in_pitch | a.out_pitch | a.in_cp | a.out_cp | a.in_uv |
                            a.in_v | a.out_uv | a.out_v | a.in_stride | a.out_stride;
        if (m & 1) return hipErrorInvalidValue;           // words would straddle
        hipLaunchKernelGGL(mask_restore_nv12_kernel<2>, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(mask_restore_nv12_kernel<1>, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

// smooth.hip — the box-scaled smooth blur (vd_smooth, and vd_process with cfg.blur_mode =
// VD_BLUR_GAUSSIAN in a context with vd_cells on): what a Gaussian-mode context applies when the
// strength follows the box size.
//
// Definition (include/vdmi.h at vd_cells, DESIGN.md "Box-scaled strength"), integers only. Box k
// with the non-empty clipped rectangle (cx1, cy1, cx2, cy2), bw x bh pixels, f = L(k)
// (vd_cell_level of the box as stored):
//   cells     f x f pixels anchored at the clipped origin, sw = ceil(bw / f) by sh = ceil(bh / f)
//             of them (both at most `cells`); the last of a row or column may be partial
//   mean      a(i, j) = (16 * S + n / 2) / n per channel: Q8.4, S the cell's sum over `in`, n its
//             pixel count
//   across    u = 2x + 1 - f, i0 = floor(u / 2f), r = u - 2f * i0, i0 and i0 + 1 clamped to
//             [0, sw - 1]:  t(x, j) = ((2f - r) * a(i0, j) + r * a(i0 + 1, j) + f) / (2f)
//   down      the same from v = 2y + 1 - f (j0, j1, s):
//             out = ((2f - s) * t(x, j0) + s * t(x, j1) + 16f) / (32f)
//   boxes     every box reads `in`; a pixel takes the value of the box with the largest f among
//             those whose clipped rectangle holds it, ties to the lowest list index; a pixel in
//             no box is out = in.
// Every intermediate but the mean's numerator fits uint32 (4080 * 2 * 32768 < 2^32).
//
// Two launches per call, ordered by the stream alone:
//   smooth_copy_kernel  in -> out, one workgroup per (frame, band of CR rows), 16-B vectors.
//   smooth_box_kernel   grid (SLOTS, frames); the workgroup of slot s takes the frame's boxes
//                       s, s + SLOTS, ... one after the other, so any number of boxes is served
//                       and the grid follows from n alone. A box of more than PART_PX pixels is
//                       shared among up to PARTS workgroups (grid z): each writes a band of whole
//                       cell rows and sums that band and one cell row on either side, which is all
//                       its rows interpolate between; a small box is part 0's alone. Per box: (1) the boxes that beat it
//                       (larger f, or equal f and a lower index) and meet it are collected in
//                       LDS; (2) the box's rows are read once, a thread walking down one byte
//                       column (consecutive lanes = consecutive bytes of a row) with its sum in
//                       a register for the rows of one cell row, then one LDS atomic per cell row
//                       -- the sw x sh x 3 sums are the only state, cells^2 * 12 bytes of LDS,
//                       and a cell hundreds of pixels wide is just many threads adding to one
//                       sum; (3) the sums become the Q8.4 means in place; (4) the same walk
//                       writes: t(x, j0) and t(x, j1) live in registers and are recomputed when
//                       the row enters the next cell row (one division by 2f per column and cell
//                       row). Between two cell-row centres the numerator is linear in y, so the
//                       quotient by 32f and its remainder are carried from row to row (exact: an
//                       add, and one carry at most); a byte costs no division.
//                       A pixel inside a beating box is skipped, so every output pixel of the
//                       pass has exactly one writer (its owner) and overlapping boxes cannot
//                       race; all reads are of `in`. Usually no box beats another and the test
//                       is one uniform branch. More beating boxes than the LDS list holds: the
//                       pixel is tested against the frame's whole list instead.
// Sums: 255 * f^2 fits uint32 up to f = 4096. A larger f means at most 8 x 8 cells (h, w <=
// 32768), whose sums are kept in 64 bits in the same LDS. Integer adds in any order give the
// same sums, so two runs give the same bytes.
// HBM traffic = read + write of every frame (2*W*H*3 bytes) + one read and one write of every
// clipped box.
//
// NV12 frames (vd_smooth_nv12, vd_process_nv12 / vd_mosaic_nv12 in a Gaussian-mode context with
// vd_cells on; include/vdmi.h at vd_nv12). The box pass is one body over the bytes per sample C:
// 3 for RGB, 1 for the luma plane (an h x w image, rectangle c = clip(b), f = L(b)), 2 for the
// chroma plane (an (h/2) x (w/2) image of U, V pairs, rectangle cc = (c.x1 >> 1, c.y1 >> 1,
// (c.x2 + 1) >> 1, (c.y2 + 1) >> 1), fc = (L(b) + 1) >> 1). Only x = bc / C and the owner's
// comparison differ: in both planes the owner of a sample is the box with the largest LUMA level
// L(b) among the boxes whose rectangle of that plane holds it (ties to the lowest index), so both
// planes hide the same box where boxes overlap (L = 7 and L = 8 share fc = 4).
// Chroma grid bound: cw <= bw / 2 + 1 <= N * L / 2 + 1 <= N * fc + 1, so a chroma grid has at
// most N + 1 cells per side, and reaches it (N = 2, level 1, box (1, 0, 5, 4): L = 2, fc = 1,
// cc = (0, 0, 3, 2)); the LDS holds max(N^2 * 3, (N + 1)^2 * 2) sums.
//   smooth_copy_nv12_kernel  [0, w) of every row of both planes in -> out, one workgroup per
//                            (frame, band of CR rows of one plane); 16-B vectors where the two
//                            rows are congruent mod 16, bytes otherwise; pad bytes and the rows
//                            between the planes are never touched.
//   smooth_box_nv12_kernel   grid (SLOTS, frames, 2 * PARTS): the plane is the upper half of z.
// HBM traffic = read + write of every frame at 1.5 B/px + one read and one write of every clipped
// box per plane. No scratch memory.
//
// Other 4:2:0 layouts (include/vdmi.h at vd_yuv420: planar I420 / YV12, NV21, or layouts that differ
// between `in` and `out`). Sums, means and interpolation are per channel, so the pair pass equals the
// C = 1, CHROMA pass run once over U and once over V with the chroma geometry and the luma-level owner
// rule unchanged; STEP gives the bytes between a row's samples on either side (1 planar, 2 one channel
// of interleaved pairs).
//   smooth_box_yuv420_kernel  grid (SLOTS, frames, 3 * PARTS): luma, U, V.
//   the copy                  between two layouts is the pixelation launch of nv12.hip with no lists:
//                             it already streams every sample from the one layout into the other.
//
// 10- and 12-bit 4:2:0 frames (include/vdmi.h at vd_yuv420_16): the formulas above on the values
// v = (word >> shift) & (2^depth - 1) of 16-bit words, Q(depth).4 means, the result written as
// result << shift. The widths are worked out at smooth_box_body (ES == 2) and in DESIGN.md.
//   smooth_box_yuv16_kernel   grid (SLOTS, frames, 3 * PARTS): luma, U, V, each a C = 1 pass over words.
//   the copy                  is the pixelation launch of words with no lists.
#include "vd_kernel.h"
#include "vdmi.h"

#include <algorithm>

namespace {

constexpr int THREADS = 256;
constexpr int CR = 8;            // rows per copy band
constexpr int SLOTS = 32;        // box-pass workgroups per frame
constexpr int PARTS = 8;         // workgroups a large box is shared among (bands of whole cell rows)
constexpr int PART_PX = 16384;   // ... one per this many pixels of the clipped box
constexpr int BEAT_CAP = 128;    // beating boxes listed in LDS; more: the global list is walked per pixel
constexpr int F32_MAX = 4096;    // largest f whose cell sums fit uint32
constexpr int F16_MAX = 1024;    // ... for samples of up to 12 bits: 4095 * 1024^2 < 2^32

// a plane of the batch: frame f at + f * stride, rows of `pitch` bytes
struct SmoothPlane {
    const uint8_t* in; uint8_t* out;
    size_t in_pitch, in_stride, out_pitch, out_stride;
};

struct SmoothArgs {
    SmoothPlane pl[2];                               // RGB: pl[0] alone; NV12: luma, chroma; any 4:2:0 layout: luma, U (V: its own argument)
    int n, h, w;                                     // frames; the frame's (luma) size, which boxes are clipped to
    const int* cnt0; const int* xy0; int cap0;      // list 0 (faces)
    const int* cnt1; const int* xy1; int cap1;      // list 1 (plates, optional)
    int level, cells;
};

__device__ __forceinline__ int frame_boxes(const SmoothArgs& a, int f, int& n0) {
    n0 = a.cnt0 ? min(max(a.cnt0[f], 0), a.cap0) : 0;
    const int n1 = a.cnt1 ? min(max(a.cnt1[f], 0), a.cap1) : 0;
    return n0 + n1;
}

__device__ __forceinline__ int4 raw_box(const SmoothArgs& a, int f, int k, int n0) {
    const int* src = k < n0 ? a.xy0 + ((size_t)f * a.cap0 + k) * 4 : a.xy1 + ((size_t)f * a.cap1 + (k - n0)) * 4;
    return make_int4(src[0], src[1], src[2], src[3]);
}

// combine_detect.py:145-148 clip, :150-151 empty check, as the other rectangular passes clip
__device__ __forceinline__ bool clip_box(int4 b, int w, int h, int4& c) {
    c = make_int4(max(0, b.x), max(0, b.y), min(w, b.z), min(h, b.w));
    return c.z > c.x && c.w > c.y;
}

__device__ __forceinline__ int box_level(const SmoothArgs& a, int4 b) {
    return vd_cell_level_hd((long long)b.z - b.x, (long long)b.w - b.y, a.level, a.cells);
}

// `nbytes` bytes s -> d: a head up to d's 16-B boundary, vectors, a tail (s and d congruent mod 16)
__device__ __forceinline__ void copy_span(uint8_t* d, const uint8_t* s, size_t nbytes, int tid) {
    const size_t head = std::min(nbytes, (size_t)((16 - ((uintptr_t)s & 15)) & 15));
    if ((size_t)tid < head) d[tid] = s[tid];
    const size_t nv = (nbytes - head) >> 4;
    const u32x4* s4 = (const u32x4*)(s + head);
    u32x4* d4 = (u32x4*)(d + head);
    for (size_t i = tid; i < nv; i += 4 * THREADS) {
        u32x4 v0{}, v1{}, v2{}, v3{};
        v0 = s4[i];
        if (i + THREADS < nv) v1 = s4[i + THREADS];
        if (i + 2 * THREADS < nv) v2 = s4[i + 2 * THREADS];
        if (i + 3 * THREADS < nv) v3 = s4[i + 3 * THREADS];
        d4[i] = v0;
        if (i + THREADS < nv) d4[i + THREADS] = v1;
        if (i + 2 * THREADS < nv) d4[i + 2 * THREADS] = v2;
        if (i + 3 * THREADS < nv) d4[i + 3 * THREADS] = v3;
    }
    const size_t tail = head + (nv << 4);
    if (tail + tid < nbytes) d[tail + tid] = s[tail + tid];
}

__global__ __launch_bounds__(THREADS) void smooth_copy_kernel(SmoothArgs a, int vec_ok) {
    const int f = blockIdx.y, y0 = blockIdx.x * CR, tid = threadIdx.x;
    const int rows = min(CR, a.h - y0);
    const size_t row_bytes = (size_t)a.w * 3;
    const size_t pitch = a.pl[0].in_pitch;                 // RGB: one pitch, frames h * pitch apart
    const uint8_t* src = a.pl[0].in + ((size_t)f * a.h + y0) * pitch;
    uint8_t* dst = a.pl[0].out + ((size_t)f * a.h + y0) * pitch;
    if (!vec_ok) {                                         // in and out differ mod 16: bytes
        for (int r = 0; r < rows; ++r)
            for (size_t i = tid; i < row_bytes; i += THREADS) dst[r * pitch + i] = src[r * pitch + i];
        return;
    }
    // the band itself: one span when the rows are packed, else row by row (padding untouched)
    if (pitch == row_bytes) {
        copy_span(dst, src, (size_t)rows * row_bytes, tid);
    } else {
        for (int r = 0; r < rows; ++r) copy_span(dst + r * pitch, src + r * pitch, row_bytes, tid);
    }
}

// NV12: bands [0, by) are luma rows, the rest chroma rows; a row of either plane has w bytes
__global__ __launch_bounds__(THREADS) void smooth_copy_nv12_kernel(SmoothArgs a, int by) {
    const int f = blockIdx.y, tid = threadIdx.x;
    const int P = (int)blockIdx.x >= by ? 1 : 0;
    const int y0 = ((int)blockIdx.x - (P ? by : 0)) * CR;
    const int rows = min(CR, (P ? a.h / 2 : a.h) - y0);
    const SmoothPlane& pl = a.pl[P];
    const size_t row_bytes = (size_t)a.w;
    const uint8_t* src = pl.in + (size_t)f * pl.in_stride + (size_t)y0 * pl.in_pitch;
    uint8_t* dst = pl.out + (size_t)f * pl.out_stride + (size_t)y0 * pl.out_pitch;
    if (pl.in_pitch == row_bytes && pl.out_pitch == row_bytes) {   // packed rows: the band is one span
        const size_t nb = (size_t)rows * row_bytes;
        if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) copy_span(dst, src, nb, tid);
        else for (size_t i = tid; i < nb; i += THREADS) dst[i] = src[i];
        return;
    }
    for (int r = 0; r < rows; ++r) {                       // uniform over the workgroup
        const uint8_t* sr = src + (size_t)r * pl.in_pitch;
        uint8_t* dr = dst + (size_t)r * pl.out_pitch;
        if ((((uintptr_t)sr ^ (uintptr_t)dr) & 15) == 0) copy_span(dr, sr, row_bytes, tid);
        else for (size_t i = tid; i < row_bytes; i += THREADS) dr[i] = sr[i];
    }
}

// t(x, j) of the definition for one channel: the row of means j, the two clamped cell columns
// and the weight r of the second
template <int C>
__device__ __forceinline__ uint32_t across(const uint32_t* mean, int j, int sw, int ia, int ib, uint32_t r,
                                           uint32_t f, int ch) {
    const uint32_t va = mean[(j * sw + ia) * C + ch], vb = mean[(j * sw + ib) * C + ch];
    return ((2u * f - r) * va + r * vb + f) / (2u * f);
}

// The box pass of one plane with C bytes per sample (3: RGB, 1: luma, 2 and CHROMA: the U, V pairs).
// s_cell: [sh][sw][C] sums, then Q8.4 means; s_beat: this plane's rectangles of the boxes beating
// the box in hand.
// STEP (C == 1): the plane's samples lie in_step / out_step bytes apart in a row -- a U or V
// plane of any 4:2:0 layout, planar or the one channel of interleaved pairs. Sums, means and
// interpolation are per channel in every form, so the C = 1, CHROMA, STEP pass over U and then over
// V computes exactly the bytes of the C = 2 pass over the pairs.
// ES == 2 (C == 1 with STEP): the plane holds 16-bit words (include/vdmi.h at vd_yuv420_16), a sample's
// value is v = (word >> shift) & (2^depth - 1), depth <= 12. The same integers one size up: a column's
// partial sum is at most 4095 * 32768 < 2^27, a cell's sum S <= 4095 * f^2 fits uint32 up to F16_MAX
// (64-bit LDS sums above it, for any cell count), a mean is Q12.4 <= 65520, t <= 65520, and
// T = (2f - s) t0 + s t1 + 16f <= 65536 * 65520 + 16 * 32768 < 2^32. A sample is written as
// result << shift, its unused bits zero.
template <int C, bool CHROMA, bool STEP = false, int ES = 1>
__device__ __forceinline__ void smooth_box_body(const SmoothArgs& a, const SmoothPlane& pl, int part, uint32_t* s_cell,
                                                int4* s_beat, int& s_nbeat, int in_step = 1, int out_step = 1,
                                                int depth = 8, int shift = 0) {
    const uint32_t vmask = (1u << depth) - 1u;
    const int fr = blockIdx.y, tid = threadIdx.x;
    int n0;
    const int nb = frame_boxes(a, fr, n0);
    const uint8_t* src = pl.in + (size_t)fr * pl.in_stride;
    uint8_t* dst = pl.out + (size_t)fr * pl.out_stride;
    // the rectangle of this plane of a clipped (luma) box
    auto plane_rect = [](int4 q) { return CHROMA ? make_int4(q.x >> 1, q.y >> 1, (q.z + 1) >> 1, (q.w + 1) >> 1) : q; };

    for (int k = blockIdx.x; k < nb; k += gridDim.x) {     // uniform over the workgroup
        const int4 b = raw_box(a, fr, k, n0);
        int4 c;
        if (!clip_box(b, a.w, a.h, c)) continue;
        c = plane_rect(c);
        const int L = box_level(a, b);                     // what the owner is chosen by, in every plane
        const int f = CHROMA ? (L + 1) >> 1 : L;
        const int bw = c.z - c.x, bh = c.w - c.y;
        const int sw = (bw + f - 1) / f, sh = (bh + f - 1) / f;
        const int ncell = sw * sh * C;
        const bool wide = f > (ES == 2 ? F16_MAX : F32_MAX);   // 64-bit sums (8-bit samples: at most 8 x 8 cells)
        const int gmax = a.cells + (CHROMA ? 1 : 0);       // the chroma grid bound (header)
        if (sw > gmax || sh > gmax || (ES == 1 && wide && ncell > THREADS)) continue;   // the LDS holds that many: cannot happen for h, w <= 32768
        // a large box is cut into bands of whole cell rows, one per part (blockIdx.z)
        const int nparts = min(min(PARTS, sh), max(1, (int)(((long long)bw * bh) / PART_PX)));
        if (part >= nparts) continue;
        unsigned long long* s_cell64 = (unsigned long long*)s_cell;

        __syncthreads();                                   // the previous box's reads of the LDS are done
        for (int i = tid; i < (wide ? 2 * ncell : ncell); i += THREADS) s_cell[i] = 0;
        if (tid == 0) s_nbeat = 0;
        __syncthreads();

        // (1) the boxes that beat this one and meet it
        for (int m = tid; m < nb; m += THREADS) {
            if (m == k) continue;
            const int4 bm = raw_box(a, fr, m, n0);
            int4 cm;
            if (!clip_box(bm, a.w, a.h, cm)) continue;
            cm = plane_rect(cm);
            if (cm.x >= c.z || cm.z <= c.x || cm.y >= c.w || cm.w <= c.y) continue;
            const int fm = box_level(a, bm);
            if (fm > L || (fm == L && m < k)) {
                const int i = atomicAdd(&s_nbeat, 1);
                if (i < BEAT_CAP) s_beat[i] = cm;
            }
        }

        // thread layout of both walks: a row has nbx bytes; a narrow box is cut into RG groups of
        // consecutive rows walked side by side, a wide one is walked CP byte columns at a time
        const int nbx = bw * C;
        const int CP = nbx < THREADS ? nbx : THREADS;
        const int RG = nbx < THREADS ? THREADS / nbx : 1;
        const int rg = tid / CP, col0 = tid - rg * CP;
        // this thread's rows of [lo, hi)
        auto my_rows = [&](int lo, int hi, int& ya, int& yb) {
            const int chunk = (hi - lo + RG - 1) / RG;
            ya = min(lo + rg * chunk, hi);
            yb = rg < RG ? min(ya + chunk, hi) : ya;
        };
        // the part's band: it writes cell rows [jA, jB) and needs the means of one more on either side
        const int jA = part * sh / nparts, jB = (part + 1) * sh / nparts;
        int ya, yb;
        my_rows(max(jA - 1, 0) * f, min((jB + 1) * f, bh), ya, yb);
        const size_t is = STEP ? (size_t)in_step * ES : 1, os = STEP ? (size_t)out_step * ES : 1;   // C == 1 with STEP: bytes
        const uint8_t* sbox = src + (size_t)c.y * pl.in_pitch + (size_t)c.x * C * is;
        uint8_t* dbox = dst + (size_t)c.y * pl.out_pitch + (size_t)c.x * C * os;

        // (2) cell sums
        if (ya < yb)
            for (int bc = col0; bc < nbx; bc += CP) {
                const int x = bc / C, ch = bc - C * x, i = x / f;
                for (int j = ya / f; j * f < yb; ++j) {
                    const int y0 = max(ya, j * f), y1 = min(yb, j * f + f);
                    uint32_t acc = 0;                      // at most 255 * 32768
                    const uint8_t* p = sbox + (size_t)y0 * pl.in_pitch + bc * is;
#pragma unroll 8
                    for (int y = y0; y < y1; ++y, p += pl.in_pitch) {
                        if constexpr (ES == 2) acc += ((uint32_t)*(const uint16_t*)p >> shift) & vmask;
                        else acc += *p;
                    }
                    const int e = (j * sw + i) * C + ch;
                    if (wide) atomicAdd(&s_cell64[e], (unsigned long long)acc);
                    else atomicAdd(&s_cell[e], acc);
                }
            }
        __syncthreads();

        // (3) sums -> Q8.4 means, in place
        auto mean_of = [&](int e, unsigned long long S) -> uint32_t {
            const int cell = e / C, j = cell / sw, i = cell - j * sw;
            const uint32_t n = (uint32_t)(min(i * f + f, bw) - i * f) * (uint32_t)(min(j * f + f, bh) - j * f);
            if ((S >> 27) == 0) return (16u * (uint32_t)S + n / 2) / n;
            return (uint32_t)((16ULL * S + n / 2) / n);
        };
        if (ES == 2 && wide) {
            // any cell count, THREADS sums at a time: mean e overwrites word e, below every unread sum
            for (int e0 = 0; e0 < ncell; e0 += THREADS) {
                const int e = e0 + tid;
                const unsigned long long S = e < ncell ? s_cell64[e] : 0;
                __syncthreads();
                if (e < ncell) s_cell[e] = mean_of(e, S);
                __syncthreads();
            }
        } else if (wide) {
            const unsigned long long S = tid < ncell ? s_cell64[tid] : 0;
            __syncthreads();
            if (tid < ncell) s_cell[tid] = mean_of(tid, S);
        } else {
            for (int e = tid; e < ncell; e += THREADS) s_cell[e] = mean_of(e, s_cell[e]);
        }
        __syncthreads();
        const int nbeat = s_nbeat;

        // (4) interpolate and write what this box owns
        my_rows(jA * f, min(jB * f, bh), ya, yb);
        if (ya < yb) {
            const uint32_t uf = (uint32_t)f, f2 = 2u * uf, d = 32u * uf;
            for (int bc = col0; bc < nbx; bc += CP) {
                const int x = bc / C, ch = bc - C * x;
                const int u = 2 * x + 1 - f;               // > -2f
                const int i0 = u < 0 ? -1 : (int)((uint32_t)u / f2);
                const uint32_t r = (uint32_t)(u - (int)f2 * i0);
                const int ia = min(max(i0, 0), sw - 1), ib = min(max(i0 + 1, 0), sw - 1);
                const int v = 2 * ya + 1 - f;
                int j0 = v < 0 ? -1 : (int)((uint32_t)v / f2);
                uint32_t s = (uint32_t)(v - (int)f2 * j0);
                // Between two cell-row centres T = (2f - s) t0 + s t1 is linear in y: the quotient
                // (T + 16f) / 32f = o and its remainder are carried from row to row, exactly,
                // o += dq, rem += dr with (dq, dr) = floor-divmod(2 (t1 - t0), 32f), one carry at most
                uint32_t o = 0, rem = 0, dr = 0;
                int dq = 0;
                auto cell_rows = [&]() {
                    const int ja = min(max(j0, 0), sh - 1), jb = min(max(j0 + 1, 0), sh - 1);
                    const uint32_t t0 = across<C>(s_cell, ja, sw, ia, ib, r, uf, ch);
                    const uint32_t t1 = jb == ja ? t0 : across<C>(s_cell, jb, sw, ia, ib, r, uf, ch);
                    const uint32_t T = (f2 - s) * t0 + s * t1 + 16u * uf;
                    o = T / d;
                    rem = T - o * d;
                    const int delta = 2 * ((int)t1 - (int)t0);
                    dq = delta >= 0 ? (int)((uint32_t)delta / d) : -(int)(((uint32_t)(-delta) + d - 1) / d);
                    dr = (uint32_t)(delta - dq * (int)d);      // in [0, 32f)
                };
                cell_rows();
                const int gx = c.x + x;
                uint8_t* p = dbox + (size_t)ya * pl.out_pitch + bc * os;
                for (int y = ya; y < yb; ++y, p += pl.out_pitch) {
                    bool mine = true;
                    if (nbeat) {
                        const int gy = c.y + y;
                        if (nbeat <= BEAT_CAP) {
                            for (int q = 0; q < nbeat; ++q) {
                                const int4 m = s_beat[q];
                                if (gx >= m.x && gx < m.z && gy >= m.y && gy < m.w) mine = false;
                            }
                        } else {
                            for (int m = 0; m < nb && mine; ++m) {
                                if (m == k) continue;
                                const int4 bm = raw_box(a, fr, m, n0);
                                int4 cm;
                                if (!clip_box(bm, a.w, a.h, cm)) continue;
                                cm = plane_rect(cm);
                                if (gx < cm.x || gx >= cm.z || gy < cm.y || gy >= cm.w) continue;
                                const int fm = box_level(a, bm);
                                if (fm > L || (fm == L && m < k)) mine = false;
                            }
                        }
                    }
                    if (mine) {
                        if constexpr (ES == 2) *(uint16_t*)p = (uint16_t)(o << shift);
                        else *p = (uint8_t)o;
                    }
                    s += 2;
                    if (s >= f2) {                         // the next row lies past cell row j0 + 1's centre
                        s -= f2;
                        ++j0;
                        cell_rows();
                    } else {
                        o += dq;
                        rem += dr;
                        if (rem >= d) { rem -= d; ++o; }
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void smooth_box_kernel(SmoothArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cell[];
    __shared__ int4 s_beat[BEAT_CAP];
    __shared__ int s_nbeat;
    smooth_box_body<3, false>(a, a.pl[0], blockIdx.z, s_cell, s_beat, s_nbeat);
}

// both planes of NV12 frames: grid z = plane * PARTS + part (uniform over the workgroup)
__global__ __launch_bounds__(THREADS) void smooth_box_nv12_kernel(SmoothArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cell[];
    __shared__ int4 s_beat[BEAT_CAP];
    __shared__ int s_nbeat;
    if (blockIdx.z < PARTS) smooth_box_body<1, false>(a, a.pl[0], blockIdx.z, s_cell, s_beat, s_nbeat);
    else smooth_box_body<2, true>(a, a.pl[1], blockIdx.z - PARTS, s_cell, s_beat, s_nbeat);
}

// the three planes of 4:2:0 frames in any layout: grid z = plane * PARTS + part. a.pl: luma and U, v: the V
// plane; the chroma steps ride beside SmoothArgs, which the RGB and NV12 kernels take as they always did
__global__ __launch_bounds__(THREADS) void smooth_box_yuv420_kernel(SmoothArgs a, SmoothPlane v, int in_step, int out_step) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cell[];
    __shared__ int4 s_beat[BEAT_CAP];
    __shared__ int s_nbeat;
    const int P = blockIdx.z / PARTS, part = blockIdx.z - P * PARTS;
    if (P == 0) smooth_box_body<1, false>(a, a.pl[0], part, s_cell, s_beat, s_nbeat);
    else smooth_box_body<1, true, true>(a, P == 1 ? a.pl[1] : v, part, s_cell, s_beat, s_nbeat, in_step, out_step);
}

// ... of 16-bit words (vd_yuv420_16): the same grid, every plane a C = 1 pass over words
__global__ __launch_bounds__(THREADS) void smooth_box_yuv16_kernel(SmoothArgs a, SmoothPlane v, int in_step, int out_step,
                                                                   int depth, int shift) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cell[];
    __shared__ int4 s_beat[BEAT_CAP];
    __shared__ int s_nbeat;
    const int P = blockIdx.z / PARTS, part = blockIdx.z - P * PARTS;
    if (P == 0) smooth_box_body<1, false, true, 2>(a, a.pl[0], part, s_cell, s_beat, s_nbeat, 1, 1, depth, shift);
    else smooth_box_body<1, true, true, 2>(a, P == 1 ? a.pl[1] : v, part, s_cell, s_beat, s_nbeat, in_step, out_step, depth, shift);
}

}  // namespace

// ... of one plane of 16-bit words: (cells + 1)^2 uint32 sums, or 64-bit sums of the cells a level above
// F16_MAX leaves (h, w <= 32768: at most 32 a side, 33 in a chroma grid)
static size_t smooth_lds_bytes16(int cells) {
    const size_t g = (size_t)cells + 1, g64 = std::min(g, (size_t)33);
    return std::max(g * g * 4, g64 * g64 * 8);
}

// The cell sums of one box: cells^2 * 3 (RGB) or (cells + 1)^2 * 2 (a chroma grid, header) uint32,
// or 64-bit sums of the few cells a level above F32_MAX leaves (RGB and luma: 8 x 8; chroma pairs:
// min(cells + 1, 4) squared, since cw <= 16384 and fc > 4096).
size_t vd_smooth_lds_bytes(int cells) {
    const int c8 = std::min(cells, 8), c4 = std::min(cells + 1, 4);
    const size_t narrow = std::max((size_t)cells * cells * 3 * 4, (size_t)(cells + 1) * (cells + 1) * 2 * 4);
    const size_t wide = std::max((size_t)c8 * c8 * 3 * 8, (size_t)c4 * c4 * 2 * 8);
    return std::max(narrow, wide);
}

hipError_t vd_launch_smooth(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
                            const int* cnt0, const int* xy0, int cap0,
                            const int* cnt1, const int* xy1, int cap1, int level, int cells, int stage,
                            hipStream_t s) {
    if (n <= 0 || h <= 0 || w <= 0) return hipSuccess;
    if (h > 32768 || w > 32768 || level < 1 || level > 32768 || cells < VD_CELLS_MIN || cells > VD_CELLS_MAX ||
        n > 65535 || pitch < (size_t)w * 3)
        return hipErrorInvalidValue;
    SmoothArgs a{};
    a.pl[0] = SmoothPlane{in, out, pitch, (size_t)h * pitch, pitch, (size_t)h * pitch};
    a.n = n; a.h = h; a.w = w;
    a.cnt0 = cnt0; a.xy0 = xy0; a.cap0 = cap0;
    a.cnt1 = cnt1; a.xy1 = xy1; a.cap1 = cap1;
    a.level = level; a.cells = cells;
    if (stage == 0) {
        // vectors need in and out congruent mod 16 (then every row's spans are, at one pitch)
        const int vec_ok = (((uintptr_t)in ^ (uintptr_t)out) & 15) == 0;
        hipLaunchKernelGGL(smooth_copy_kernel, dim3((h + CR - 1) / CR, n), dim3(THREADS), 0, s, a, vec_ok);
    } else if (cnt0 || cnt1) {
        hipLaunchKernelGGL(smooth_box_kernel, dim3(SLOTS, n, PARTS), dim3(THREADS), vd_smooth_lds_bytes(cells), s, a);
    }
    return hipGetLastError();
}

hipError_t vd_launch_smooth_nv12(const Nv12MosaicArgs& v, int stage, hipStream_t s, int depth, int shift) {
    const size_t es = depth ? 2 : 1;
    if (v.n <= 0 || v.h <= 0 || v.w <= 0 || (v.h & 1) || (v.w & 1) || v.h > 32768 || v.w > 32768 || v.level < 1 ||
        v.level > 32768 || v.cells < VD_CELLS_MIN || v.cells > VD_CELLS_MAX || v.n > 65535 ||
        v.in_pitch < (size_t)v.w * es || v.out_pitch < (size_t)v.w * es || !v.in || !v.out ||
        (v.in_step != 1 && v.in_step != 2) || (v.out_step != 1 && v.out_step != 2) ||
        v.in_cp < (size_t)(v.w / 2) * v.in_step * es || v.out_cp < (size_t)(v.w / 2) * v.out_step * es ||
        (depth && (depth < 8 || depth > 12 || shift < 0 || shift + depth > 16)))
        return hipErrorInvalidValue;
    if ((depth || !v.nv12()) && stage == 0) {
        // any other layout pair: the copy is the pixelation launch with no lists (nv12.hip), which
        // moves [0, w) of the luma rows and every chroma sample from the one layout into the other
        Nv12MosaicArgs c = v;
        c.cnt0 = c.cnt1 = nullptr; c.xy0 = c.xy1 = nullptr; c.cap0 = c.cap1 = 0;
        c.level = 1; c.cells = 0;
        return vd_launch_mosaic_nv12(c, s, depth);
    }
    SmoothArgs a{};
    a.pl[0] = SmoothPlane{v.in, v.out, v.in_pitch, v.in_stride, v.out_pitch, v.out_stride};
    a.pl[1] = SmoothPlane{v.in + v.in_uv, v.out + v.out_uv, v.in_cp, v.in_stride, v.out_cp, v.out_stride};
    const SmoothPlane vp{v.in + v.in_v, v.out + v.out_v, v.in_cp, v.in_stride, v.out_cp, v.out_stride};
    a.n = v.n; a.h = v.h; a.w = v.w;
    a.cnt0 = v.cnt0; a.xy0 = v.xy0; a.cap0 = v.cap0;
    a.cnt1 = v.cnt1; a.xy1 = v.xy1; a.cap1 = v.cap1;
    a.level = v.level; a.cells = v.cells;
    if (stage == 0) {
        const int by = (v.h + CR - 1) / CR, bc = (v.h / 2 + CR - 1) / CR;
        hipLaunchKernelGGL(smooth_copy_nv12_kernel, dim3(by + bc, v.n), dim3(THREADS), 0, s, a, by);
    } else if (v.cnt0 || v.cnt1) {
        if (depth)   // (stage 0 was the pixelation launch of words with no lists, which also checked that every size is even)
            hipLaunchKernelGGL(smooth_box_yuv16_kernel, dim3(SLOTS, v.n, 3 * PARTS), dim3(THREADS),
                               smooth_lds_bytes16(v.cells), s, a, vp, v.in_step, v.out_step, depth, shift);
        else if (v.nv12())
            hipLaunchKernelGGL(smooth_box_nv12_kernel, dim3(SLOTS, v.n, 2 * PARTS), dim3(THREADS),
                               vd_smooth_lds_bytes(v.cells), s, a);
        else
            hipLaunchKernelGGL(smooth_box_yuv420_kernel, dim3(SLOTS, v.n, 3 * PARTS), dim3(THREADS),
                               vd_smooth_lds_bytes(v.cells), s, a, vp, v.in_step, v.out_step);
    }
    return hipGetLastError();
}

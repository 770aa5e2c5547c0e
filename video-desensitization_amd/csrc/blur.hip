// blur.hip — out-of-place Gaussian blur of detected boxes (vd_blur, and vd_process with
// cfg.blur_mode = VD_BLUR_GAUSSIAN): the Gaussian counterpart of mosaic.hip.
//
// Per box, in list order (faces, then plates): clip to the frame (combine_detect.py:145-151),
// replace the clipped region by the separable fixed-point Gaussian of the region ALONE
// (BORDER_REFLECT_101 at the clipped box's edges), box j reading the output of box j-1.
// The arithmetic (include/vdmi.h at vd_blur) is exact in uint32, so the order of the taps
// and the way the work is cut cannot change a bit:
//   t = sum_i q_i * px(y, refl(x+i-r, bw));  h = (t + 2^15) >> 16     (Q8.4, <= 4080)
//   s = sum_i q_i * h(refl(y+i-r, bh), x);   out = (s + 2^23) >> 24
//
// Pixelation orders overlapping boxes by a backward gather; a convolution cannot. Instead
// every box gets a LEVEL: 0 when no earlier valid box of the list meets it, else 1 + the
// highest level among the earlier boxes it meets. Then
//   * boxes of one level are pairwise disjoint (of two that met, the later would be deeper);
//   * a box reads only what earlier boxes meeting it wrote, and those are all shallower;
//   * a later box meeting it is deeper.
// So running the levels one after the other, each level's boxes in parallel, IS the
// sequential result. Level 0 reads `in`; a deeper level reads a snapshot of its boxes taken
// from `out` before its pass rewrites them. Levels 0 .. LMAX-1 get a pass each; boxes deeper
// than that (long overlap chains: rare after NMS) are applied serially, in list order.
// Launches per call, ordered only by the stream (no workgroup waits on another):
//   blur_plan_kernel  one workgroup per frame: clips the boxes, finds min(level, LMAX) of each
//                     in LMAX relaxation passes over all earlier boxes (LDS tiles of 1024
//                     rectangles, any number of boxes) and writes the frame's list, grouped
//                     by level, list order kept within a level, with the level counts.
//   blur_band_kernel  level l, one workgroup per (frame, band of rows). Level 0 first copies
//                     the band in -> out (16-B vectors). Then, for every box of the level
//                     meeting the band, the band's rows of it, BCW columns at a time: the H
//                     pass stages BG reflect-extended source rows in LDS and leaves the Q8.4
//                     rows (band rows +- r, 16-bit) in LDS; the V pass reads them and writes
//                     `out`. A thread computes 4 neighbouring outputs from a sliding window,
//                     so a tap costs one data read and one weight read per 4 products.
//   blur_snap_kernel  levels >= 1, before the band pass: the level's boxes out -> snapshot.
//   blur_dep_kernel   one workgroup per frame; frames without boxes deeper than LMAX-1 leave
//                     at once: those boxes in list order, in place on `out`, in strips of BCW
//                     columns through a two-strip global scratch: H(s+1) is computed before
//                     V(s) is written, and since BCW >= r a strip's taps reach one strip to
//                     either side at most, so every H pass reads pixels no V pass has touched.
// A level without boxes costs an empty launch: every workgroup reads one count and leaves.
// Grid and scratch sizes come from n, cap and the frame size only. HBM traffic = read + write
// of every frame (2*W*H*3 bytes) + the box areas' reads (halo rows re-read from L2), snapshots
// and writes.
#include "vd_kernel.h"
#include "vdmi.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int KMAX = VD_BLUR_KSIZE_MAX;
constexpr int BR_MAX = 32;      // rows per band: 32, or 16 for radii whose Q8.4 rows would not fit the LDS
constexpr int LMAX = 4;         // levels 0 .. LMAX-1 run in parallel passes, deeper boxes serially
constexpr int BCW = 64;         // box columns per pass; >= the largest radius (blur_dep_kernel relies on it)
constexpr int BG = 16;          // source rows staged per H step
constexpr int BPAD = 3;         // staged columns past the halo: a thread's 4-output run may read them (results unused)
constexpr int PTILE = 1024;     // rectangles per LDS tile of the plan kernel
static_assert(BCW >= KMAX / 2, "a strip's taps must stay within its neighbours");

struct BlurArgs {
    const uint8_t* in; uint8_t* out; int n, h, w; size_t pitch;
    const int* cnt0; const int* xy0; int cap0;      // list 0 (faces)
    const int* cnt1; const int* xy1; int cap1;      // list 1 (plates, optional)
    int ksize;
    int tcap;
    int level;                                       // the level a band / snapshot launch works on
    int br;                                          // rows per band
    int4* list;                                      // [n][tcap] clipped boxes by level, list order within a level
    int* lvl;                                        // [n][tcap] level of each box (-1: empty), capped at LMAX
    int* counts;                                     // [n][LMAX + 1] boxes per level ([LMAX]: the serial rest)
    uint8_t* snap;                                   // [n][h][pitch] levels >= 1: the boxes' pixels before the pass
    uint16_t* scratch; size_t scratch_frame;         // [n][2 strips][h][BCW * 3] Q8.4 rows of a serial box
    uint32_t q[KMAX];
};

// first entry and length of level l's segment of frame f's list
__device__ __forceinline__ int level_segment(const BlurArgs& a, int f, int l, int& cnt) {
    const int* cn = a.counts + (size_t)f * (LMAX + 1);
    int off = 0;
    for (int j = 0; j < l; ++j) off += cn[j];
    cnt = cn[l];
    return off;
}

__device__ __forceinline__ int frame_boxes(const BlurArgs& a, int f, int& n0) {
    n0 = a.cnt0 ? min(max(a.cnt0[f], 0), a.cap0) : 0;
    const int n1 = a.cnt1 ? min(max(a.cnt1[f], 0), a.cap1) : 0;
    return n0 + n1;
}

// combine_detect.py:145-148 clip, :150-151 empty check (an empty box: the rectangle 0,0,0,0)
__device__ __forceinline__ int4 clip_box(const BlurArgs& a, int f, int k, int n0) {
    const int* src = k < n0 ? a.xy0 + ((size_t)f * a.cap0 + k) * 4 : a.xy1 + ((size_t)f * a.cap1 + (k - n0)) * 4;
    const int x1 = max(0, src[0]), y1 = max(0, src[1]), x2 = min(a.w, src[2]), y2 = min(a.h, src[3]);
    if (!(x2 > x1 && y2 > y1)) return make_int4(0, 0, 0, 0);
    return make_int4(x1, y1, x2, y2);
}

// BORDER_REFLECT_101 (OpenCV borderInterpolate), any number of reflections
__device__ __forceinline__ int refl(int p, int n) {
    if ((unsigned)p < (unsigned)n) return p;
    if (n == 1) return 0;
    const int m = 2 * (n - 1);
    p = (p < 0 ? -p : p) % m;
    return p >= n ? m - p : p;
}

__global__ __launch_bounds__(256) void blur_plan_kernel(BlurArgs a) {
    __shared__ int4 s_r[PTILE];
    __shared__ int s_w[4];
    __shared__ int s_off, s_cnt;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int n0;
    const int nb = frame_boxes(a, f, n0);
    int4* list = a.list + (size_t)f * a.tcap;
    int* lvl = a.lvl + (size_t)f * a.tcap;
    for (int k = tid; k < nb; k += 256) {
        const int4 q = clip_box(a, f, k, n0);
        lvl[k] = q.z > q.x ? 0 : -1;
    }
    if (tid == 0) s_off = 0;
    // pass t raises to t the boxes of level t-1 that an earlier box of level >= t-1 meets
    // (a chain of t boxes ends at them); after LMAX passes lvl = min(level, LMAX)
    for (int t = 1; t <= LMAX; ++t) {
        for (int base = 0; base < nb; base += 256) {          // uniform over the workgroup
            const int k = base + tid;
            const int4 me = k < nb ? clip_box(a, f, k, n0) : make_int4(0, 0, 0, 0);
            bool hit = false;
            // every earlier box, PTILE rectangles at a time (an empty rectangle meets nothing)
            for (int jt = 0; jt < min(base + 256, nb); jt += PTILE) {
                __syncthreads();                              // lvl of the chunks before; s_r free
                for (int i = tid; i < PTILE && jt + i < nb; i += 256)
                    s_r[i] = lvl[jt + i] >= t - 1 ? clip_box(a, f, jt + i, n0) : make_int4(0, 0, 0, 0);
                __syncthreads();
                const bool cand = k < nb && lvl[k] == t - 1;  // only this thread writes lvl[k]
                const int lim = min(PTILE, k - jt);           // j < k
                if (cand)
                    for (int i = 0; i < lim; ++i) {
                        const int4 q = s_r[i];
                        hit |= q.x < me.z && me.x < q.z && q.y < me.w && me.y < q.w;
                    }
            }
            if (hit) lvl[k] = t;
        }
        __syncthreads();
    }
    // ordered compaction, level by level, into the frame's list
    for (int l = 0; l <= LMAX; ++l) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int base = 0; base < nb; base += 256) {
            const int k = base + tid;
            const bool mine = k < nb && lvl[k] == l;
            const uint64_t bal = __ballot(mine);
            if (lane == 0) s_w[wid] = __popcll(bal);
            __syncthreads();
            int o = s_off + s_cnt;
            for (int i = 0; i < wid; ++i) o += s_w[i];
            if (mine) list[o + __popcll(bal & ((1ULL << lane) - 1ULL))] = clip_box(a, f, k, n0);
            __syncthreads();
            if (tid == 0) s_cnt += s_w[0] + s_w[1] + s_w[2] + s_w[3];
            __syncthreads();
        }
        if (tid == 0) {
            a.counts[(size_t)f * (LMAX + 1) + l] = s_cnt;
            s_off += s_cnt;
        }
        __syncthreads();
    }
}

// nbytes from s to d by the whole workgroup: 16-B vectors (four in flight per thread) where
// the two pointers share their alignment, bytes at the ends
__device__ __forceinline__ void copy_span(uint8_t* d, const uint8_t* s, size_t nbytes, int tid) {
    if ((((uintptr_t)d ^ (uintptr_t)s) & 15) != 0) {
        for (size_t i = tid; i < nbytes; i += 256) d[i] = s[i];
        return;
    }
    const size_t head = std::min(nbytes, (size_t)((16 - ((uintptr_t)s & 15)) & 15));
    if ((size_t)tid < head) d[tid] = s[tid];
    const size_t nv = (nbytes - head) >> 4;
    const u32x4* s4 = (const u32x4*)(s + head);
    u32x4* d4 = (u32x4*)(d + head);
    for (size_t i = tid; i < nv; i += 4 * 256) {
        u32x4 v0{}, v1{}, v2{}, v3{};
        v0 = s4[i];
        if (i + 256 < nv) v1 = s4[i + 256];
        if (i + 512 < nv) v2 = s4[i + 512];
        if (i + 768 < nv) v3 = s4[i + 768];
        d4[i] = v0;
        if (i + 256 < nv) d4[i + 256] = v1;
        if (i + 512 < nv) d4[i + 512] = v2;
        if (i + 768 < nv) d4[i + 768] = v3;
    }
    const size_t tail = head + (nv << 4);
    if (tail + tid < nbytes) d[tail + tid] = s[tail + tid];
}

__global__ __launch_bounds__(256) void blur_band_kernel(BlurArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int r = a.ksize >> 1;
    const int hrow = BCW * 3;                              // elements per Q8.4 row
    const int irow = (BCW + 2 * r + BPAD) * 3;             // bytes per staged source row
    uint32_t* s_q = (uint32_t*)smem;                       // [128]
    uint16_t* s_h = (uint16_t*)(smem + 512);               // [br + 2r][hrow]
    uint8_t* s_in = smem + 512 + (size_t)(a.br + 2 * r) * hrow * 2;   // [BG][irow]
    const int f = blockIdx.y, y0 = blockIdx.x * a.br, tid = threadIdx.x;
    const int rows = min(a.br, a.h - y0);
    const int row_bytes = a.w * 3;
    // level 0 reads the caller's frames, a later level the snapshot of its boxes
    const uint8_t* src = (a.level == 0 ? a.in : a.snap) + (size_t)f * a.h * a.pitch;
    uint8_t* dst = a.out + (size_t)f * a.h * a.pitch;
    if (tid < a.ksize) s_q[tid] = a.q[tid];
    if (a.level == 0) {
        // the band itself: one span when the rows are packed, else row by row (padding untouched)
        if (a.pitch == (size_t)row_bytes) {
            copy_span(dst + (size_t)y0 * a.pitch, src + (size_t)y0 * a.pitch, (size_t)rows * row_bytes, tid);
        } else {
            for (int y = y0; y < y0 + rows; ++y)
                copy_span(dst + (size_t)y * a.pitch, src + (size_t)y * a.pitch, row_bytes, tid);
        }
    }
    int ni;
    const int4* il = a.list + (size_t)f * a.tcap + level_segment(a, f, a.level, ni);
    if (ni == 0) return;
    __syncthreads();                                       // the copy's stores precede the box stores below
    for (int b = 0; b < ni; ++b) {                         // uniform over the workgroup
        const int4 q = il[b];
        const int ya = max(y0, q.y), yb = min(y0 + rows, q.w);
        if (ya >= yb) continue;
        const int bw = q.z - q.x, bh = q.w - q.y;
        const int nh = (yb - ya) + 2 * r;                  // Q8.4 rows: virtual box rows v0 .. v0 + nh - 1
        const int v0 = ya - q.y - r;
        for (int cx = 0; cx < bw; cx += BCW) {
            const int cw = min(BCW, bw - cx), cw3 = cw * 3, ncol = cw + 2 * r;
            const int u0 = cx - r;                         // virtual box column of staged column 0
            for (int j0 = 0; j0 < nh; j0 += BG) {
                const int g = min(BG, nh - j0);
                // SB pixels per thread and step: all their loads are issued before the first LDS
                // store (byte stores may alias byte loads for the compiler: one by one, every
                // pixel would wait out its own global latency)
                constexpr int SB = 8;
                for (int e0 = tid; e0 < g * ncol; e0 += 256 * SB) {
                    uint8_t px[SB][3];
                    int at[SB];
#pragma unroll
                    for (int k = 0; k < SB; ++k) {
                        const int e = e0 + 256 * k;
                        at[k] = -1;
                        if (e < g * ncol) {
                            const int gi = e / ncol, u = e - gi * ncol;
                            const uint8_t* sp = src + (size_t)(q.y + refl(v0 + j0 + gi, bh)) * a.pitch +
                                                (q.x + refl(u0 + u, bw)) * 3;
                            px[k][0] = sp[0]; px[k][1] = sp[1]; px[k][2] = sp[2];
                            at[k] = gi * irow + u * 3;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < SB; ++k)
                        if (at[k] >= 0) {
                            uint8_t* ip = s_in + at[k];
                            ip[0] = px[k][0]; ip[1] = px[k][1]; ip[2] = px[k][2];
                        }
                }
                __syncthreads();
                // a thread: 4 consecutive pixels of one channel of one row; each tap costs one
                // byte read (a sliding window of 4) and one weight read for the 4 products
                const int rpr = ((cw + 3) >> 2) * 3;           // runs per row
                for (int e = tid; e < g * rpr; e += 256) {
                    const int gi = e / rpr, rr = e - gi * rpr;
                    const int xg = rr / 3, c = rr - 3 * xg;
                    const uint8_t* ip = s_in + gi * irow + xg * 12 + c;
                    uint32_t p0 = ip[0], p1 = ip[3], p2 = ip[6], t0 = 0, t1 = 0, t2 = 0, t3 = 0;
#pragma unroll 4
                    for (int i = 0; i < a.ksize; ++i) {
                        const uint32_t p3 = ip[3 * (i + 3)], w = s_q[i];
                        t0 += __umul24(w, p0); t1 += __umul24(w, p1); t2 += __umul24(w, p2); t3 += __umul24(w, p3);
                        p0 = p1; p1 = p2; p2 = p3;
                    }
                    uint16_t* hp = s_h + (j0 + gi) * hrow + xg * 12 + c;
                    const int nv = cw - 4 * xg;                // pixels of the run inside the chunk
                    hp[0] = (uint16_t)((t0 + (1u << 15)) >> 16);
                    if (nv > 1) hp[3] = (uint16_t)((t1 + (1u << 15)) >> 16);
                    if (nv > 2) hp[6] = (uint16_t)((t2 + (1u << 15)) >> 16);
                    if (nv > 3) hp[9] = (uint16_t)((t3 + (1u << 15)) >> 16);
                }
                __syncthreads();
            }
            // a thread: one byte column of 4 consecutive rows, the same sliding window downwards
            const int nr = yb - ya;
            for (int e = tid; e < ((nr + 3) >> 2) * cw3; e += 256) {
                const int yg = e / cw3, xc = e - yg * cw3;
                const uint16_t* hp = s_h + yg * 4 * hrow + xc;
                uint32_t p0 = hp[0], p1 = hp[hrow], p2 = hp[2 * hrow], v0s = 0, v1s = 0, v2s = 0, v3s = 0;
#pragma unroll 4
                for (int i = 0; i < a.ksize; ++i) {
                    const uint32_t p3 = hp[(i + 3) * hrow], w = s_q[i];
                    v0s += __umul24(w, p0); v1s += __umul24(w, p1); v2s += __umul24(w, p2); v3s += __umul24(w, p3);
                    p0 = p1; p1 = p2; p2 = p3;
                }
                uint8_t* op = dst + (size_t)(ya + yg * 4) * a.pitch + (size_t)(q.x + cx) * 3 + xc;
                const int nv = nr - 4 * yg;                    // rows of the run inside the band
                op[0] = (uint8_t)((v0s + (1u << 23)) >> 24);
                if (nv > 1) op[a.pitch] = (uint8_t)((v1s + (1u << 23)) >> 24);
                if (nv > 2) op[2 * a.pitch] = (uint8_t)((v2s + (1u << 23)) >> 24);
                if (nv > 3) op[3 * a.pitch] = (uint8_t)((v3s + (1u << 23)) >> 24);
            }
            __syncthreads();                               // s_h is rewritten by the next columns / box
        }
    }
}

// Levels >= 1: the band's rows of the level's boxes, out -> snapshot, before the band pass
// rewrites them in `out` (its workgroups read rows other workgroups write).
__global__ __launch_bounds__(256) void blur_snap_kernel(BlurArgs a) {
    const int f = blockIdx.y, y0 = blockIdx.x * a.br, tid = threadIdx.x;
    int ni;
    const int4* il = a.list + (size_t)f * a.tcap + level_segment(a, f, a.level, ni);
    if (ni == 0) return;
    const int rows = min(a.br, a.h - y0);
    const uint8_t* src = a.out + (size_t)f * a.h * a.pitch;
    uint8_t* dst = a.snap + (size_t)f * a.h * a.pitch;
    for (int b = 0; b < ni; ++b) {
        const int4 q = il[b];
        const int ya = max(y0, q.y), yb = min(y0 + rows, q.w);
        if (ya >= yb) continue;
        const int seg = (q.z - q.x) * 3;
        for (int y = ya; y < yb; ++y) {
            const size_t o = (size_t)y * a.pitch + (size_t)q.x * 3;
            for (int xc = tid; xc < seg; xc += 256) dst[o + xc] = src[o + xc];
        }
    }
}

__global__ __launch_bounds__(1024) void blur_dep_kernel(BlurArgs a) {
    __shared__ uint32_t s_q[128];
    const int f = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    int nd;
    const int4* dl = a.list + (size_t)f * a.tcap + level_segment(a, f, LMAX, nd);
    if (nd == 0) return;                                   // uniform over the workgroup
    const int r = a.ksize >> 1;
    const int hrow = BCW * 3;
    if (tid < a.ksize) s_q[tid] = a.q[tid];
    __syncthreads();
    uint8_t* img = a.out + (size_t)f * a.h * a.pitch;
    uint16_t* sc = a.scratch + (size_t)f * a.scratch_frame;
    for (int b = 0; b < nd; ++b) {
        const int4 q = dl[b];
        const int bw = q.z - q.x, bh = q.w - q.y;
        const int nstrip = (bw + BCW - 1) / BCW;
        // Q8.4 rows of strip s (all bh rows) into scratch slot s & 1
        auto hpass = [&](int s) {
            const int x0 = s * BCW, cw3 = min(BCW, bw - x0) * 3;
            uint16_t* slot = sc + (size_t)(s & 1) * a.h * hrow;
            for (int e = tid; e < bh * cw3; e += nthr) {
                const int y = e / cw3, xc = e - y * cw3;
                const int x = xc / 3, c = xc - 3 * x;
                const uint8_t* row = img + (size_t)(q.y + y) * a.pitch + (size_t)q.x * 3 + c;
                uint32_t t = 0;
#pragma unroll 8
                for (int i = 0; i < a.ksize; ++i) t += __umul24(s_q[i], row[refl(x0 + x + i - r, bw) * 3]);
                slot[(size_t)y * hrow + xc] = (uint16_t)((t + (1u << 15)) >> 16);
            }
        };
        auto vpass = [&](int s) {
            const int x0 = s * BCW, cw3 = min(BCW, bw - x0) * 3;
            const uint16_t* slot = sc + (size_t)(s & 1) * a.h * hrow;
            for (int e = tid; e < bh * cw3; e += nthr) {
                const int y = e / cw3, xc = e - y * cw3;
                uint32_t v = 0;
#pragma unroll 8
                for (int i = 0; i < a.ksize; ++i) v += __umul24(s_q[i], slot[(size_t)refl(y + i - r, bh) * hrow + xc]);
                img[(size_t)(q.y + y) * a.pitch + (size_t)(q.x + x0) * 3 + xc] = (uint8_t)((v + (1u << 23)) >> 24);
            }
        };
        hpass(0);
        for (int s = 0; s < nstrip; ++s) {
            if (s + 1 < nstrip) hpass(s + 1);              // reads strips s .. s + 2: none written yet
            __syncthreads();
            vpass(s);
            __syncthreads();                               // the next box (or H pass) reads these pixels
        }
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

// Q20 weights of the ksize-tap Gaussian (the definition at vd_blur, include/vdmi.h), in double;
// the centre tap takes the rounding remainder so the taps sum to 2^20 exactly.
int vd_blur_weights(int ksize, float sigma, uint32_t* q) {
    if (ksize < 3 || ksize > KMAX || !(ksize & 1) || !std::isfinite(sigma)) return -1;
    const int r = ksize / 2;
    const double sg = sigma > 0.f ? (double)sigma : 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8;
    double w[KMAX], sum = 0.0;
    for (int i = 0; i < ksize; ++i) {
        const double d = (double)(i - r);
        w[i] = std::exp(-(d * d) / (2.0 * sg * sg));
        sum += w[i];
    }
    uint32_t rest = 0;
    for (int i = 0; i < ksize; ++i) {
        if (i == r) continue;
        q[i] = (uint32_t)std::floor(w[i] / sum * 1048576.0 + 0.5);
        rest += q[i];
    }
    q[r] = (1u << 20) - rest;
    return 0;
}

size_t vd_blur_table_bytes(int n, int h, size_t pitch, int tcap) {
    tcap = std::max(1, tcap);
    return align16((size_t)n * tcap * sizeof(int4)) + align16((size_t)n * tcap * sizeof(int)) +
           align16((size_t)n * (LMAX + 1) * sizeof(int)) + align16((size_t)n * 2 * h * BCW * 3 * sizeof(uint16_t)) +
           (size_t)n * h * pitch + 64;
}

hipError_t vd_launch_blur(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
                          const int* cnt0, const int* xy0, int cap0,
                          const int* cnt1, const int* xy1, int cap1, int ksize, const uint32_t* q,
                          void* table, hipStream_t s) {
    if (n <= 0 || h <= 0 || w <= 0) return hipSuccess;
    if (ksize < 3 || ksize > KMAX || !(ksize & 1)) return hipErrorInvalidValue;
    BlurArgs a{};
    a.in = in; a.out = out; a.n = n; a.h = h; a.w = w; a.pitch = pitch;
    a.cnt0 = cnt0; a.xy0 = xy0; a.cap0 = cap0;
    a.cnt1 = cnt1; a.xy1 = xy1; a.cap1 = cap1;
    a.ksize = ksize;
    a.tcap = std::max(1, (cnt0 ? cap0 : 0) + (cnt1 ? cap1 : 0));
    char* p = (char*)table;
    p += (16 - ((uintptr_t)p & 15)) & 15;
    a.list = (int4*)p;
    p += align16((size_t)n * a.tcap * sizeof(int4));
    a.lvl = (int*)p;
    p += align16((size_t)n * a.tcap * sizeof(int));
    a.counts = (int*)p;
    p += align16((size_t)n * (LMAX + 1) * sizeof(int));
    a.scratch = (uint16_t*)p;
    a.scratch_frame = (size_t)2 * h * BCW * 3;
    p += align16((size_t)n * a.scratch_frame * sizeof(uint16_t));
    a.snap = (uint8_t*)p;
    for (int i = 0; i < ksize; ++i) a.q[i] = q[i];
    const int r = ksize / 2;
    // Q8.4 rows of a band +- r, 16-bit: 32-row bands up to r = 47 (55 KB of LDS), 16-row bands above (63 KB)
    a.br = r <= 47 ? BR_MAX : 16;
    const size_t lds = 512 + (size_t)(a.br + 2 * r) * BCW * 3 * 2 + align16((size_t)BG * (BCW + 2 * r + BPAD) * 3);
    const dim3 bands((h + a.br - 1) / a.br, n);
    hipLaunchKernelGGL(blur_plan_kernel, dim3(n), dim3(256), 0, s, a);
    for (int l = 0; l < LMAX; ++l) {
        a.level = l;
        if (l > 0) hipLaunchKernelGGL(blur_snap_kernel, bands, dim3(256), 0, s, a);
        hipLaunchKernelGGL(blur_band_kernel, bands, dim3(256), lds, s, a);
    }
    hipLaunchKernelGGL(blur_dep_kernel, dim3(n), dim3(1024), 0, s, a);
    return hipGetLastError();
}

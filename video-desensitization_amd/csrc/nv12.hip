// nv12.hip — out-of-place pixelation of NV12 frames, both planes in one launch; and, at the end, the
// copy that packs surfaces into the look-ahead ring (vd_launch_nv12_pack).
//
// Definition (include/vdmi.h at vd_nv12): for box b of the list being blurred, c = b clipped to
// the frame and L = L(b) (vd_cell_level_hd of the box as stored): the luma plane takes the mosaic
// of mosaic.hip as an h x w one-channel image with box c at level L; the chroma plane takes it as
// an (h/2) x (w/2) two-channel image with box cc = (c.x1 >> 1, c.y1 >> 1, (c.x2 + 1) >> 1,
// (c.y2 + 1) >> 1) at level (L + 1) >> 1. Per plane box j reads the output of box j - 1, so a
// sample's value is found by walking the list backwards (mosaic_map.h: p <- down(up(p)) for every
// box, last to first, that contains p), then out(p) = in(p'): a pure gather.
//
// One workgroup per (frame, band of NV12_ROWS luma rows and their NV12_ROWS / 2 chroma rows):
//   1. the frame's boxes are clipped into LDS for both planes (rect, sw | sh << 16);
//   2. the boxes that meet the band form the band list, in call order, with the up factors and,
//      per plane, the slice of each box's cells whose rows meet the band;
//   3. one thread per cell of those slices: the cell's source point, the backward walk over the
//      earlier boxes of the frame, one gather (1 B luma, 2 B chroma) into the LDS cell table --
//      every cell's colour is found once, not once per pixel;
//   4. the band is streamed: a lane moves 16 B (16 luma samples or 8 chroma pairs, whole samples,
//      so there is no byte phase to track); a chunk no band box meets is a copy, otherwise each
//      sample takes the colour of its owner's cell (the LAST band box containing it) or its source
//      value. Every output byte inside [0, w) of a row is written exactly once; pad bytes and the
//      rows between the planes are never written.
// Rows are moved with 16-B loads and stores when both surfaces are 16-B aligned throughout (base,
// pitch, uv_offset, frame_stride), otherwise byte by byte; a row's tail past the last whole chunk
// always goes byte by byte.
// Past the capacities below -- a frame of more than NV12_LDS_BOXES boxes, a band that more than
// NV12_BAND_BOXES boxes meet, slices of more than NV12_CELLS cells in a plane -- the band's samples
// walk the whole list themselves (the generic path; same result).
#include "vd_common.h"
#include "vd_kernel.h"
#include "vd_math.h"
#include "mosaic_map.h"

namespace {

constexpr int NV12_ROWS = 16;         // luma rows per band
constexpr int NV12_LDS_BOXES = 256;   // boxes of a frame clipped into LDS
constexpr int NV12_BAND_BOXES = 32;   // boxes in a band's list
constexpr int NV12_CELLS = 4096;      // cell colours per band and plane

struct BandBox {
    int idx;                 // position in the frame's list
    int off[2], uy0[2];      // per plane: first entry in the cell table, first cell row of the slice
    double fux[2], fuy[2];   // per plane: up factors
};

__device__ __forceinline__ int nv_frame_boxes(const Nv12MosaicArgs& a, int f, int& n0) {
    n0 = a.cnt0 ? min(max(a.cnt0[f], 0), a.cap0) : 0;
    const int n1 = a.cnt1 ? min(max(a.cnt1[f], 0), a.cap1) : 0;
    return n0 + n1;
}

// box k of frame f for both planes: q[0] / sz[0] luma, q[1] / sz[1] chroma (empty box: empty rects)
__device__ __forceinline__ void nv_clip(const Nv12MosaicArgs& a, int f, int k, int n0, int4 q[2], uint32_t sz[2]) {
    const int* src = k < n0 ? a.xy0 + ((size_t)f * a.cap0 + k) * 4 : a.xy1 + ((size_t)f * a.cap1 + (k - n0)) * 4;
    const int x1 = max(0, src[0]), y1 = max(0, src[1]), x2 = min(a.w, src[2]), y2 = min(a.h, src[3]);
    if (!(x2 > x1 && y2 > y1)) {
        q[0] = q[1] = make_int4(0, 0, 0, 0);
        sz[0] = sz[1] = 1u | (1u << 16);
        return;
    }
    const int L = vd_cell_level_hd((long long)src[2] - src[0], (long long)src[3] - src[1], a.level, a.cells);
    const int Lc = (L + 1) >> 1;
    q[0] = make_int4(x1, y1, x2, y2);
    q[1] = make_int4(x1 >> 1, y1 >> 1, (x2 + 1) >> 1, (y2 + 1) >> 1);
    sz[0] = (uint32_t)max(1, (x2 - x1) / L) | ((uint32_t)max(1, (y2 - y1) / L) << 16);
    sz[1] = (uint32_t)max(1, (q[1].z - q[1].x) / Lc) | ((uint32_t)max(1, (q[1].w - q[1].y) / Lc) << 16);
}

// the source sample of plane P at (y, x): a luma byte, or a chroma pair as u | v << 8
template <int P>
__device__ __forceinline__ unsigned nv_src(const uint8_t* plane, size_t pitch, int y, int x) {
    const uint8_t* p = plane + (size_t)y * pitch + (P ? 2 * x : x);
    return P ? (unsigned)p[0] | ((unsigned)p[1] << 8) : (unsigned)p[0];
}

__device__ __forceinline__ int up_index(int d, double f, int s) { return min((int)floor(VD_DMUL((double)d, f)), s - 1); }

template <bool VEC>
__global__ __launch_bounds__(256) void nv12_mosaic_kernel(Nv12MosaicArgs a) {
    __shared__ int4 s_q[2][NV12_LDS_BOXES];
    __shared__ uint32_t s_sz[2][NV12_LDS_BOXES];
    __shared__ BandBox s_band[NV12_BAND_BOXES];
    __shared__ uint8_t s_cy[NV12_CELLS];
    __shared__ uint16_t s_cuv[NV12_CELLS];
    __shared__ int s_nband, s_generic, s_tot[2];

    const int f = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const uint8_t* in_y = a.in + (size_t)f * a.in_stride;
    const uint8_t* in_uv = in_y + a.in_uv;
    uint8_t* out_y = a.out + (size_t)f * a.out_stride;
    uint8_t* out_uv = out_y + a.out_uv;
    // the band's rows per plane: luma [r0[0], r1[0]), chroma [r0[1], r1[1]) (h is even)
    const int r0[2] = {band * NV12_ROWS, band * (NV12_ROWS / 2)};
    const int r1[2] = {min(r0[0] + NV12_ROWS, a.h), min(r0[1] + NV12_ROWS / 2, a.h / 2)};
    const int pw[2] = {a.w, a.w / 2};

    int n0;
    const int nb = nv_frame_boxes(a, f, n0);
    const bool lds_boxes = nb <= NV12_LDS_BOXES;
    if (lds_boxes)
        for (int k = tid; k < nb; k += 256) {
            int4 q[2];
            uint32_t sz[2];
            nv_clip(a, f, k, n0, q, sz);
            s_q[0][k] = q[0]; s_q[1][k] = q[1];
            s_sz[0][k] = sz[0]; s_sz[1][k] = sz[1];
        }
    __syncthreads();
    if (tid == 0) {
        int nbd = 0, generic = lds_boxes ? 0 : 1, tot[2] = {0, 0};
        for (int k = 0; k < nb && !generic; ++k) {
            const int4 ql = s_q[0][k];
            // a box meets the band's luma rows iff its chroma rectangle meets the band's chroma rows
            if (!(ql.z > ql.x && ql.y < r1[0] && ql.w > r0[0])) continue;
            if (nbd == NV12_BAND_BOXES) { generic = 1; break; }
            BandBox b;
            b.idx = k;
            for (int P = 0; P < 2; ++P) {
                const int4 q = s_q[P][k];
                const int sw = (int)(s_sz[P][k] & 0xFFFFu), sh = (int)(s_sz[P][k] >> 16);
                b.fux[P] = up_factor(q.z - q.x, sw);
                b.fuy[P] = up_factor(q.w - q.y, sh);
                const int ya = max(q.y, r0[P]), yb = min(q.w, r1[P]) - 1;   // yb >= ya: see above
                const int ua = up_index(ya - q.y, b.fuy[P], sh), ub = up_index(yb - q.y, b.fuy[P], sh);
                b.uy0[P] = ua;
                b.off[P] = tot[P];
                tot[P] += sw * (ub - ua + 1);   // at most w * NV12_ROWS
                if (tot[P] > NV12_CELLS) generic = 1;
            }
            s_band[nbd++] = b;
        }
        s_nband = nbd; s_generic = generic; s_tot[0] = tot[0]; s_tot[1] = tot[1];
    }
    __syncthreads();
    const int nband = s_nband;
    const bool generic = s_generic != 0;

    // box k of plane P: from LDS, or (frames past NV12_LDS_BOXES) clipped from the lists again
    auto box = [&](int P, int k, int4& q, uint32_t& sz) {
        if (lds_boxes) { q = s_q[P][k]; sz = s_sz[P][k]; return; }
        int4 qq[2];
        uint32_t ss[2];
        nv_clip(a, f, k, n0, qq, ss);
        q = qq[P]; sz = ss[P];
    };
    // (y, x) of plane P walked back through boxes [0, from)
    auto walk = [&](int P, int from, int& y, int& x) {
        for (int k = from - 1; k >= 0; --k) {
            int4 q;
            uint32_t sz;
            box(P, k, q, sz);
            if (in_rect(q, y, x)) apply_rect(q, sz, y, x);
        }
    };

    if (!generic && nband) {   // the band's cell colours, each found once
        const int t0 = s_tot[0], t1 = s_tot[1];
        for (int t = tid; t < t0 + t1; t += 256) {
            const int P = t >= t0 ? 1 : 0;
            const int e = P ? t - t0 : t;
            int i = nband - 1;
            while (s_band[i].off[P] > e) --i;
            const BandBox& b = s_band[i];
            const int4 q = s_q[P][b.idx];
            const uint32_t sz = s_sz[P][b.idx];
            const int sw = (int)(sz & 0xFFFFu), sh = (int)(sz >> 16);
            const int c = e - b.off[P];
            const int uy = b.uy0[P] + c / sw, ux = c - (c / sw) * sw;
            const int bw = q.z - q.x, bh = q.w - q.y;
            int x = q.x + min((int)floor(VD_DMUL((double)ux, down_factor(bw, sw))), bw - 1);
            int y = q.y + min((int)floor(VD_DMUL((double)uy, down_factor(bh, sh))), bh - 1);
            walk(P, b.idx, y, x);
            if (P) s_cuv[e] = (uint16_t)nv_src<1>(in_uv, a.in_pitch, y, x);
            else s_cy[e] = (uint8_t)nv_src<0>(in_y, a.in_pitch, y, x);
        }
        __syncthreads();
    }

    // the value of sample (y, x) of plane P, given its source value
    auto sample = [&](int P, int y, int x, unsigned srcv) -> unsigned {
        if (generic) {
            int yy = y, xx = x;
            walk(P, nb, yy, xx);
            if (yy == y && xx == x) return srcv;
            return P ? nv_src<1>(in_uv, a.in_pitch, yy, xx) : nv_src<0>(in_y, a.in_pitch, yy, xx);
        }
        for (int i = nband - 1; i >= 0; --i) {
            const BandBox& b = s_band[i];
            const int4 q = s_q[P][b.idx];
            if (!in_rect(q, y, x)) continue;
            const uint32_t sz = s_sz[P][b.idx];
            const int sw = (int)(sz & 0xFFFFu), sh = (int)(sz >> 16);
            const int ux = up_index(x - q.x, b.fux[P], sw), uy = up_index(y - q.y, b.fuy[P], sh);
            const int e = b.off[P] + (uy - b.uy0[P]) * sw + ux;
            return P ? (unsigned)s_cuv[e] : (unsigned)s_cy[e];
        }
        return srcv;
    };
    // does any band box meet samples [x0, x1) of row y of plane P
    auto touched = [&](int P, int y, int x0, int x1) -> bool {
        if (generic) return nb > 0;
        for (int i = 0; i < nband; ++i) {
            const int4 q = s_q[P][s_band[i].idx];
            if (y >= q.y && y < q.w && x0 < q.z && x1 > q.x) return true;
        }
        return false;
    };

#pragma unroll
    for (int P = 0; P < 2; ++P) {
        const uint8_t* ip = P ? in_uv : in_y;
        uint8_t* op = P ? out_uv : out_y;
        const int EP = P ? 8 : 16;                   // samples per 16-B chunk
        const int nch = (pw[P] + EP - 1) / EP;
        const int rows = r1[P] - r0[P];
        for (int c = tid; c < rows * nch; c += 256) {
            const int row = c / nch, ch = c - row * nch;
            const int y = r0[P] + row, x0 = ch * EP, npx = min(EP, pw[P] - x0);
            const uint8_t* src = ip + (size_t)y * a.in_pitch + (size_t)ch * 16;
            uint8_t* dst = op + (size_t)y * a.out_pitch + (size_t)ch * 16;
            const bool hit = (nband || generic) && touched(P, y, x0, x0 + npx);
            if (VEC && npx == EP) {
                uint4 v = *(const uint4*)src;
                if (hit) {
                    uint32_t wd[4] = {v.x, v.y, v.z, v.w};
                    if (P) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const unsigned sv = (wd[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                            const unsigned nv = sample(1, y, x0 + i, sv);
                            wd[i >> 1] = (wd[i >> 1] & ~(0xFFFFu << (16 * (i & 1)))) | (nv << (16 * (i & 1)));
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const unsigned sv = (wd[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                            const unsigned nv = sample(0, y, x0 + i, sv);
                            wd[i >> 2] = (wd[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | (nv << (8 * (i & 3)));
                        }
                    }
                    v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                }
                *(uint4*)dst = v;
            } else {
                for (int i = 0; i < npx; ++i) {
                    if (P) {
                        unsigned sv = (unsigned)src[2 * i] | ((unsigned)src[2 * i + 1] << 8);
                        if (hit) sv = sample(1, y, x0 + i, sv);
                        dst[2 * i] = (uint8_t)sv; dst[2 * i + 1] = (uint8_t)(sv >> 8);
                    } else {
                        unsigned sv = src[i];
                        if (hit) sv = sample(0, y, x0 + i, sv);
                        dst[i] = (uint8_t)sv;
                    }
                }
            }
        }
    }
}

// ---- the look-ahead ring push: surfaces from one layout into another, [0, w) of every plane row ----
// Grid-y runs over groups of PACK_ROWS (frame, plane row) pairs, one wave per row (a surface's h luma
// rows, then its h / 2 chroma rows); grid-x over the row in steps of 64 lanes x 16 B. A row whose
// source and target starts are congruent mod 16 goes as a byte head up to the first 16-B boundary,
// 16-B loads and stores, and a byte tail; any other row goes byte by byte. Nothing is assumed of w,
// the pitches, the plane offsets or the strides: a packed slot of w = 130 starts its rows at every
// residue. Bytes outside [0, w) of a row are neither read nor written.
constexpr int PACK_ROWS = 4;
constexpr int PACK_STEP = 64 * 16;    // bytes of a row per grid-x step

__device__ __forceinline__ size_t pack_row(int y, int h, size_t pitch, size_t uv) {
    return y < h ? (size_t)y * pitch : uv + (size_t)(y - h) * pitch;
}

__global__ __launch_bounds__(64 * PACK_ROWS) void nv12_pack_kernel(Nv12PackArgs a) {
    const int lane = threadIdx.x, rows = a.h + a.h / 2;
    const long long total = (long long)a.n * rows;
    for (long long r = (long long)blockIdx.y * PACK_ROWS + threadIdx.y; r < total; r += (long long)gridDim.y * PACK_ROWS) {
        const int f = (int)(r / rows), y = (int)(r - (long long)f * rows);
        const uint8_t* s = a.src + (size_t)f * a.src_stride + pack_row(y, a.h, a.src_pitch, a.src_uv);
        uint8_t* d = a.dst + (size_t)f * a.dst_stride + pack_row(y, a.h, a.dst_pitch, a.dst_uv);
        const bool vec = (((uintptr_t)s ^ (uintptr_t)d) & 15) == 0;
        const int head = vec ? min(a.w, (int)((16 - ((uintptr_t)s & 15)) & 15)) : a.w;
        const int nvec = (a.w - head) >> 4, tail0 = head + (nvec << 4);
        const int v = blockIdx.x * 64 + lane;
        if (v < nvec) *(uint4*)(d + head + ((size_t)v << 4)) = *(const uint4*)(s + head + ((size_t)v << 4));
        // the head and the tail (fewer than 16 bytes each), or the whole row
        const int nbytes = head + (a.w - tail0);
        const int b1 = min(nbytes, (int)(blockIdx.x + 1) * PACK_STEP);
        for (int i = blockIdx.x * PACK_STEP + lane; i < b1; i += 64) {
            const int x = i < head ? i : tail0 + (i - head);
            d[x] = s[x];
        }
    }
}

}  // namespace

hipError_t vd_launch_nv12_pack(const Nv12PackArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || (a.h & 1) || (a.w & 1) || a.src_pitch < (size_t)a.w ||
        a.dst_pitch < (size_t)a.w || !a.src || !a.dst)
        return hipErrorInvalidValue;
    const long long groups = ((long long)a.n * (a.h + a.h / 2) + PACK_ROWS - 1) / PACK_ROWS;
    const dim3 grid((a.w + PACK_STEP - 1) / PACK_STEP, (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(nv12_pack_kernel, grid, dim3(64, PACK_ROWS), 0, s, a);
    return hipGetLastError();
}

hipError_t vd_launch_mosaic_nv12(const Nv12MosaicArgs& a, hipStream_t s) {
    // sw | sh << 16 holds 16 bits per axis; even sizes only (the chroma plane is (h/2) x (w/2) pairs)
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || (a.h & 1) || (a.w & 1) || a.h > 65534 || a.w > 65534 || a.level < 1 ||
        a.in_pitch < (size_t)a.w || a.out_pitch < (size_t)a.w)
        return hipErrorInvalidValue;
    const uintptr_t align = (uintptr_t)a.in | (uintptr_t)a.out | a.in_pitch | a.in_uv | a.in_stride | a.out_pitch |
                            a.out_uv | a.out_stride;
    const dim3 grid((a.h + NV12_ROWS - 1) / NV12_ROWS, a.n);
    if ((align & 15) == 0) hipLaunchKernelGGL(nv12_mosaic_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(nv12_mosaic_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

// nv12.hip — out-of-place pixelation of 8-bit 4:2:0 frames (NV12, and every layout of vd_yuv420), all
// planes in one launch; and, at the end, the copies that pack surfaces into the look-ahead ring: NV12
// (vd_launch_nv12_pack) and every other layout, 8-bit or 16-bit words (vd_launch_yuv420_pack).
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
// Other layouts (include/vdmi.h at vd_yuv420): the chroma plane stays one two-channel (h/2) x (w/2)
// image whose sample is the pair u | v << 8 -- every box, cell and owner decision above is shared by
// U and V -- and only the addresses differ: the gathers read U and V at their own offsets, chroma_step
// apart, and in the band stream a lane moves 8 pairs between two interleaved surfaces and otherwise
// 16 samples, as 16 B of the U plane and 16 B of the V plane on a planar side and 32 B of pairs on
// an interleaved one, split and joined in registers. The steps of input and output are template
// parameters, so no streaming loop branches on the layout; the NV12 -> NV12 instantiation is the
// kernel as it was. 16-B accesses need base, both pitches, the plane offsets and the stride of
// a surface aligned; otherwise, and in row tails, samples go byte by byte.
// 10- and 12-bit surfaces (include/vdmi.h at vd_yuv420_16): the same kernel with ES = 2, a sample being a
// 16-bit word -- pixelation copies whole words, so depth and shift play no part; see at ld16 below.
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

// Layouts (include/vdmi.h at vd_yuv420). The kernel below is instantiated per chroma step of the
// input (IS) and of the output (OS): 1 planar, 2 interleaved; SW: an interleaved side may hold V
// first (NV21), told by its offsets. <2, 2, false> is the NV12 kernel. In every form a chroma
// sample is the pair u | v << 8, so boxes, cells and owners are decided once for both channels;
// only the addresses differ.
// chroma sample (y, x) of a surface with U at pu, V at pv, rows of cp bytes, samples ST apart
template <int ST>
__device__ __forceinline__ unsigned yuv_src(const uint8_t* pu, const uint8_t* pv, size_t cp, int y, int x) {
    const size_t o = (size_t)y * cp + (size_t)x * ST;
    return (unsigned)pu[o] | ((unsigned)pv[o] << 8);
}
// two words of interleaved pairs (a0 b0 a1 b1 | a2 b2 a3 b3) <-> a word of a's and a word of b's
__device__ __forceinline__ void yuv_split(uint32_t w0, uint32_t w1, uint32_t& a, uint32_t& b) {
    a = (w0 & 0xFFu) | ((w0 >> 8) & 0xFF00u) | ((w1 & 0xFFu) << 16) | ((w1 & 0xFF0000u) << 8);
    b = ((w0 >> 8) & 0xFFu) | ((w0 >> 16) & 0xFF00u) | ((w1 << 8) & 0xFF0000u) | (w1 & 0xFF000000u);
}
__device__ __forceinline__ void yuv_join(uint32_t a, uint32_t b, uint32_t& w0, uint32_t& w1) {
    w0 = (a & 0xFFu) | ((b & 0xFFu) << 8) | ((a & 0xFF00u) << 8) | ((b & 0xFF00u) << 16);
    w1 = ((a >> 16) & 0xFFu) | (((b >> 16) & 0xFFu) << 8) | ((a >> 24) << 16) | ((b >> 24) << 24);
}
__device__ __forceinline__ uint32_t yuv_swap16(uint32_t w) { return ((w & 0x00FF00FFu) << 8) | ((w >> 8) & 0x00FF00FFu); }

__device__ __forceinline__ int up_index(int d, double f, int s) { return min((int)floor(VD_DMUL((double)d, f)), s - 1); }

// 16-bit words (include/vdmi.h at vd_yuv420_16; ES == 2 below): pixelation is a copy of whole words, so
// the kernel is the one above with a sample of 2 bytes -- a luma word, or a chroma pair u | v << 16 --
// and every offset and pitch still in bytes. A lane moves 16 B of luma (8 words) and 8 chroma samples:
// 16 B of the U plane and 16 B of the V plane on a planar side, 32 B of pairs on an interleaved one.
__device__ __forceinline__ unsigned ld16(const uint8_t* p) { return *(const uint16_t*)p; }
// two words of interleaved pairs (a0 b0 | a1 b1) <-> a word of a's and a word of b's
__device__ __forceinline__ void yuv_split16(uint32_t w0, uint32_t w1, uint32_t& a, uint32_t& b) {
    a = (w0 & 0xFFFFu) | (w1 << 16);
    b = (w0 >> 16) | (w1 & 0xFFFF0000u);
}
__device__ __forceinline__ void yuv_join16(uint32_t a, uint32_t b, uint32_t& w0, uint32_t& w1) {
    w0 = (a & 0xFFFFu) | (b << 16);
    w1 = (a >> 16) | (b & 0xFFFF0000u);
}

template <int ES> struct CellOf { using Y = uint8_t; using C = uint16_t; };
template <> struct CellOf<2> { using Y = uint16_t; using C = uint32_t; };

// ES: bytes per sample (1: the 8-bit kernels, 2: 16-bit words in and out, always with SW)
template <bool VEC, int IS, int OS, bool SW, int ES = 1>
__global__ __launch_bounds__(256) void nv12_mosaic_kernel(Nv12MosaicArgs a) {
    __shared__ int4 s_q[2][NV12_LDS_BOXES];
    __shared__ uint32_t s_sz[2][NV12_LDS_BOXES];
    __shared__ BandBox s_band[NV12_BAND_BOXES];
    __shared__ typename CellOf<ES>::Y s_cy[NV12_CELLS];
    __shared__ typename CellOf<ES>::C s_cuv[NV12_CELLS];
    __shared__ int s_nband, s_generic, s_tot[2];

    const int f = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const uint8_t* in_y = a.in + (size_t)f * a.in_stride;
    const uint8_t* in_u = in_y + a.in_uv;
    const uint8_t* in_v = in_y + a.in_v;
    uint8_t* out_y = a.out + (size_t)f * a.out_stride;
    uint8_t* out_u = out_y + a.out_uv;
    uint8_t* out_v = out_y + a.out_v;
    // an interleaved side: its pairs start at the lower offset; V first there means swapped pairs
    const bool isw = SW && IS == 2 && a.in_v < a.in_uv, osw = SW && OS == 2 && a.out_v < a.out_uv;
    const uint8_t* in_c = isw ? in_v : in_u;
    uint8_t* out_c = osw ? out_v : out_u;
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
    // the source sample of plane P at (y, x)
    auto gather = [&](int P, int y, int x) -> unsigned {
        if constexpr (ES == 2) {
            const size_t o = (size_t)y * a.in_cp + (size_t)x * (2 * IS);
            return P ? ld16(in_u + o) | (ld16(in_v + o) << 16) : ld16(in_y + (size_t)y * a.in_pitch + 2 * (size_t)x);
        } else {
            return P ? yuv_src<IS>(in_u, in_v, a.in_cp, y, x) : nv_src<0>(in_y, a.in_pitch, y, x);
        }
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
            if (P) s_cuv[e] = (typename CellOf<ES>::C)gather(1, y, x);
            else s_cy[e] = (typename CellOf<ES>::Y)gather(0, y, x);
        }
        __syncthreads();
    }

    // the value of sample (y, x) of plane P, given its source value
    auto sample = [&](int P, int y, int x, unsigned srcv) -> unsigned {
        if (generic) {
            int yy = y, xx = x;
            walk(P, nb, yy, xx);
            if (yy == y && xx == x) return srcv;
            return gather(P, yy, xx);
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

    if constexpr (ES == 2) {
        // luma: 8 words per 16-B chunk
        const int nch = (a.w + 7) / 8;
        const int rows = r1[0] - r0[0];
        for (int c = tid; c < rows * nch; c += 256) {
            const int row = c / nch, ch = c - row * nch;
            const int y = r0[0] + row, x0 = ch * 8, npx = min(8, a.w - x0);
            const uint8_t* src = in_y + (size_t)y * a.in_pitch + (size_t)ch * 16;
            uint8_t* dst = out_y + (size_t)y * a.out_pitch + (size_t)ch * 16;
            const bool hit = (nband || generic) && touched(0, y, x0, x0 + npx);
            if (VEC && npx == 8) {
                uint4 v = *(const uint4*)src;
                if (hit) {
                    uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int sh = 16 * (i & 1);
                        const unsigned nv = sample(0, y, x0 + i, (wd[i >> 1] >> sh) & 0xFFFFu);
                        wd[i >> 1] = (wd[i >> 1] & ~(0xFFFFu << sh)) | (nv << sh);
                    }
                    v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                }
                *(uint4*)dst = v;
            } else {
                for (int i = 0; i < npx; ++i) {
                    unsigned sv = ld16(src + 2 * i);
                    if (hit) sv = sample(0, y, x0 + i, sv);
                    *(uint16_t*)(dst + 2 * i) = (uint16_t)sv;
                }
            }
        }
        // chroma: 8 samples per lane, as U words and V words in registers
        const int cw = a.w / 2;
        const int cch = (cw + 7) / 8;
        const int crows = r1[1] - r0[1];
        for (int c = tid; c < crows * cch; c += 256) {
            const int row = c / cch, ch = c - row * cch;
            const int y = r0[1] + row, x0 = ch * 8, npx = min(8, cw - x0);
            const bool hit = (nband || generic) && touched(1, y, x0, x0 + npx);
            const size_t irow = (size_t)y * a.in_cp, orow = (size_t)y * a.out_cp;
            if (VEC && npx == 8) {
                uint32_t uu[4], vv[4];
                if constexpr (IS == 1) {
                    const uint4 p = *(const uint4*)(in_u + irow + (size_t)ch * 16);
                    const uint4 q = *(const uint4*)(in_v + irow + (size_t)ch * 16);
                    uu[0] = p.x; uu[1] = p.y; uu[2] = p.z; uu[3] = p.w;
                    vv[0] = q.x; vv[1] = q.y; vv[2] = q.z; vv[3] = q.w;
                } else {
                    const uint4 p = *(const uint4*)(in_c + irow + (size_t)ch * 32);
                    const uint4 q = *(const uint4*)(in_c + irow + (size_t)ch * 32 + 16);
                    uint32_t* fa = isw ? vv : uu;       // the pairs' first words
                    uint32_t* fb = isw ? uu : vv;
                    yuv_split16(p.x, p.y, fa[0], fb[0]); yuv_split16(p.z, p.w, fa[1], fb[1]);
                    yuv_split16(q.x, q.y, fa[2], fb[2]); yuv_split16(q.z, q.w, fa[3], fb[3]);
                }
                if (hit) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int sh = 16 * (i & 1);
                        const unsigned sv = ((uu[i >> 1] >> sh) & 0xFFFFu) | (((vv[i >> 1] >> sh) & 0xFFFFu) << 16);
                        const unsigned nv = sample(1, y, x0 + i, sv);
                        uu[i >> 1] = (uu[i >> 1] & ~(0xFFFFu << sh)) | ((nv & 0xFFFFu) << sh);
                        vv[i >> 1] = (vv[i >> 1] & ~(0xFFFFu << sh)) | ((nv >> 16) << sh);
                    }
                }
                if constexpr (OS == 1) {
                    *(uint4*)(out_u + orow + (size_t)ch * 16) = make_uint4(uu[0], uu[1], uu[2], uu[3]);
                    *(uint4*)(out_v + orow + (size_t)ch * 16) = make_uint4(vv[0], vv[1], vv[2], vv[3]);
                } else {
                    const uint32_t* fa = osw ? vv : uu;
                    const uint32_t* fb = osw ? uu : vv;
                    uint32_t o[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) yuv_join16(fa[i], fb[i], o[2 * i], o[2 * i + 1]);
                    *(uint4*)(out_c + orow + (size_t)ch * 32) = make_uint4(o[0], o[1], o[2], o[3]);
                    *(uint4*)(out_c + orow + (size_t)ch * 32 + 16) = make_uint4(o[4], o[5], o[6], o[7]);
                }
            } else {
                for (int i = 0; i < npx; ++i) {
                    const size_t xi = (size_t)(x0 + i) * (2 * IS), xo = (size_t)(x0 + i) * (2 * OS);
                    unsigned sv = ld16(in_u + irow + xi) | (ld16(in_v + irow + xi) << 16);
                    if (hit) sv = sample(1, y, x0 + i, sv);
                    *(uint16_t*)(out_u + orow + xo) = (uint16_t)sv;
                    *(uint16_t*)(out_v + orow + xo) = (uint16_t)(sv >> 16);
                }
            }
        }
        return;
    }
    // luma: 16 samples per 16-B chunk
    {
        const int nch = (a.w + 15) / 16;
        const int rows = r1[0] - r0[0];
        for (int c = tid; c < rows * nch; c += 256) {
            const int row = c / nch, ch = c - row * nch;
            const int y = r0[0] + row, x0 = ch * 16, npx = min(16, a.w - x0);
            const uint8_t* src = in_y + (size_t)y * a.in_pitch + (size_t)ch * 16;
            uint8_t* dst = out_y + (size_t)y * a.out_pitch + (size_t)ch * 16;
            const bool hit = (nband || generic) && touched(0, y, x0, x0 + npx);
            if (VEC && npx == 16) {
                uint4 v = *(const uint4*)src;
                if (hit) {
                    uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const unsigned sv = (wd[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                        const unsigned nv = sample(0, y, x0 + i, sv);
                        wd[i >> 2] = (wd[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | (nv << (8 * (i & 3)));
                    }
                    v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                }
                *(uint4*)dst = v;
            } else {
                for (int i = 0; i < npx; ++i) {
                    unsigned sv = src[i];
                    if (hit) sv = sample(0, y, x0 + i, sv);
                    dst[i] = (uint8_t)sv;
                }
            }
        }
    }
    // chroma: a lane moves 8 pairs (16 B in, 16 B out) between two interleaved surfaces, else 16
    // samples (16 B of each plane on a planar side, 32 B of pairs on an interleaved one)
    {
        constexpr int EP = (IS == 2 && OS == 2) ? 8 : 16;
        const int cw = a.w / 2;
        const int nch = (cw + EP - 1) / EP;
        const int rows = r1[1] - r0[1];
        for (int c = tid; c < rows * nch; c += 256) {
            const int row = c / nch, ch = c - row * nch;
            const int y = r0[1] + row, x0 = ch * EP, npx = min(EP, cw - x0);
            const bool hit = (nband || generic) && touched(1, y, x0, x0 + npx);
            const size_t irow = (size_t)y * a.in_cp, orow = (size_t)y * a.out_cp;
            if (VEC && npx == EP) {
                if constexpr (IS == 2 && OS == 2) {
                    uint4 v = *(const uint4*)(in_c + irow + (size_t)ch * 16);
                    uint32_t wd[4] = {v.x, v.y, v.z, v.w};
                    if (hit) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            unsigned sv = (wd[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                            if (isw) sv = yuv_swap16(sv) & 0xFFFFu;
                            unsigned nv = sample(1, y, x0 + i, sv);
                            if (osw) nv = yuv_swap16(nv) & 0xFFFFu;
                            wd[i >> 1] = (wd[i >> 1] & ~(0xFFFFu << (16 * (i & 1)))) | (nv << (16 * (i & 1)));
                        }
                    } else if (isw != osw) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) wd[i] = yuv_swap16(wd[i]);
                    }
                    *(uint4*)(out_c + orow + (size_t)ch * 16) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                } else {
                    uint32_t uu[4], vv[4];
                    if constexpr (IS == 1) {
                        const uint4 p = *(const uint4*)(in_u + irow + (size_t)ch * 16);
                        const uint4 q = *(const uint4*)(in_v + irow + (size_t)ch * 16);
                        uu[0] = p.x; uu[1] = p.y; uu[2] = p.z; uu[3] = p.w;
                        vv[0] = q.x; vv[1] = q.y; vv[2] = q.z; vv[3] = q.w;
                    } else {
                        const uint4 p = *(const uint4*)(in_c + irow + (size_t)ch * 32);
                        const uint4 q = *(const uint4*)(in_c + irow + (size_t)ch * 32 + 16);
                        uint32_t* fa = isw ? vv : uu;       // the pairs' first bytes
                        uint32_t* fb = isw ? uu : vv;
                        yuv_split(p.x, p.y, fa[0], fb[0]); yuv_split(p.z, p.w, fa[1], fb[1]);
                        yuv_split(q.x, q.y, fa[2], fb[2]); yuv_split(q.z, q.w, fa[3], fb[3]);
                    }
                    if (hit) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int sh = 8 * (i & 3);
                            const unsigned sv = ((uu[i >> 2] >> sh) & 0xFFu) | (((vv[i >> 2] >> sh) & 0xFFu) << 8);
                            const unsigned nv = sample(1, y, x0 + i, sv);
                            uu[i >> 2] = (uu[i >> 2] & ~(0xFFu << sh)) | ((nv & 0xFFu) << sh);
                            vv[i >> 2] = (vv[i >> 2] & ~(0xFFu << sh)) | ((nv >> 8) << sh);
                        }
                    }
                    if constexpr (OS == 1) {
                        *(uint4*)(out_u + orow + (size_t)ch * 16) = make_uint4(uu[0], uu[1], uu[2], uu[3]);
                        *(uint4*)(out_v + orow + (size_t)ch * 16) = make_uint4(vv[0], vv[1], vv[2], vv[3]);
                    } else {
                        const uint32_t* fa = osw ? vv : uu;
                        const uint32_t* fb = osw ? uu : vv;
                        uint32_t o[8];
#pragma unroll
                        for (int i = 0; i < 4; ++i) yuv_join(fa[i], fb[i], o[2 * i], o[2 * i + 1]);
                        *(uint4*)(out_c + orow + (size_t)ch * 32) = make_uint4(o[0], o[1], o[2], o[3]);
                        *(uint4*)(out_c + orow + (size_t)ch * 32 + 16) = make_uint4(o[4], o[5], o[6], o[7]);
                    }
                }
            } else {
                for (int i = 0; i < npx; ++i) {
                    const size_t xi = (size_t)(x0 + i) * IS, xo = (size_t)(x0 + i) * OS;
                    unsigned sv = (unsigned)in_u[irow + xi] | ((unsigned)in_v[irow + xi] << 8);
                    if (hit) sv = sample(1, y, x0 + i, sv);
                    out_u[orow + xo] = (uint8_t)sv; out_v[orow + xo] = (uint8_t)(sv >> 8);
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

// ---- the same push from the other layouts, and for 16-bit words ----
// The target is always the ring's layout: interleaved pairs, U first. ES: bytes a sample (2: whole 16-bit
// words); CS: the source's chroma step; VF: an interleaved source holds V first. The shape is the kernel's
// above -- one wave a row, PACK_ROWS rows a workgroup, grid-stride over the row groups, grid-x over the
// target row in steps of PACK_STEP bytes -- and so is every luma row and every chroma row of an
// interleaved, U-first source (<1, 2, false> with NV12's pitches is served by the kernel above, not this one).
//   interleaved, V first: the same traffic, the two samples of each pair swapped in registers; the head
//     up to the first 16-B boundary is whole pairs, so a row whose start splits a pair goes pair by pair;
//   planar: a lane reads 8 samples of the U row and 8 of the V row (8 B + 8 B, or 16 B + 16 B of words)
//     and writes their 8 pairs (one or two 16-B stores), from the first 16-B boundary of the target
//     row on, where both source rows are aligned for those loads there; the pairs before it, the
//     pairs past the last whole group, and every pair of any other row go sample by sample.
// Bytes outside a row's samples are neither read nor written.
struct YuvPackArgs {
    const uint8_t* src; uint8_t* dst; int n, h, w;
    size_t src_pitch, src_u, src_v, src_cp, src_stride, dst_pitch, dst_uv, dst_stride;
};

// [0, nb) of a row as the kernel above moves it
__device__ __forceinline__ void pack_copy_row(const uint8_t* s, uint8_t* d, int nb, int lane) {
    const bool vec = (((uintptr_t)s ^ (uintptr_t)d) & 15) == 0;
    const int head = vec ? min(nb, (int)((16 - ((uintptr_t)s & 15)) & 15)) : nb;
    const int nvec = (nb - head) >> 4, tail0 = head + (nvec << 4);
    const int v = blockIdx.x * 64 + lane;
    if (v < nvec) *(uint4*)(d + head + ((size_t)v << 4)) = *(const uint4*)(s + head + ((size_t)v << 4));
    const int nbytes = head + (nb - tail0);
    const int b1 = min(nbytes, (int)(blockIdx.x + 1) * PACK_STEP);
    for (int i = blockIdx.x * PACK_STEP + lane; i < b1; i += 64) {
        const int x = i < head ? i : tail0 + (i - head);
        d[x] = s[x];
    }
}

// pair x of a target row from its two samples
template <int ES>
__device__ __forceinline__ void pack_pair(const uint8_t* su, const uint8_t* sv, uint8_t* d, int x) {
    if constexpr (ES == 2) {
        *(uint16_t*)(d + 4 * (size_t)x) = *(const uint16_t*)(su + 2 * (size_t)x);
        *(uint16_t*)(d + 4 * (size_t)x + 2) = *(const uint16_t*)(sv + 2 * (size_t)x);
    } else {
        d[2 * (size_t)x] = su[x];
        d[2 * (size_t)x + 1] = sv[x];
    }
}

template <int ES, int CS, bool VF>
__global__ __launch_bounds__(64 * PACK_ROWS) void yuv420_pack_kernel(YuvPackArgs a) {
    constexpr int PB = 2 * ES;                      // bytes of a pair
    const int lane = threadIdx.x, rows = a.h + a.h / 2, np = a.w / 2;
    const long long total = (long long)a.n * rows;
    for (long long r = (long long)blockIdx.y * PACK_ROWS + threadIdx.y; r < total; r += (long long)gridDim.y * PACK_ROWS) {
        const int f = (int)(r / rows), y = (int)(r - (long long)f * rows);
        const uint8_t* sf = a.src + (size_t)f * a.src_stride;
        uint8_t* d = a.dst + (size_t)f * a.dst_stride + pack_row(y, a.h, a.dst_pitch, a.dst_uv);
        if (y < a.h) {
            pack_copy_row(sf + (size_t)y * a.src_pitch, d, a.w * ES, lane);
            continue;
        }
        const size_t crow = (size_t)(y - a.h) * a.src_cp;
        if constexpr (CS == 2 && !VF) {
            pack_copy_row(sf + a.src_u + crow, d, a.w * ES, lane);
        } else if constexpr (CS == 2) {             // pairs V, U -> U, V
            const uint8_t* s = sf + a.src_v + crow;
            const bool vec = (((uintptr_t)s ^ (uintptr_t)d) & 15) == 0 && ((uintptr_t)s & (PB - 1)) == 0;
            const int head = vec ? min(np, (int)(((16 - ((uintptr_t)s & 15)) & 15) / PB)) : np;
            const int nvec = (np - head) / (16 / PB), tail0 = head + nvec * (16 / PB);
            const int v = blockIdx.x * 64 + lane;
            if (v < nvec) {
                uint4 q = *(const uint4*)(s + (size_t)head * PB + ((size_t)v << 4));
                if constexpr (ES == 2) {
                    q = make_uint4((q.x << 16) | (q.x >> 16), (q.y << 16) | (q.y >> 16), (q.z << 16) | (q.z >> 16),
                                   (q.w << 16) | (q.w >> 16));
                } else {
                    q = make_uint4(yuv_swap16(q.x), yuv_swap16(q.y), yuv_swap16(q.z), yuv_swap16(q.w));
                }
                *(uint4*)(d + (size_t)head * PB + ((size_t)v << 4)) = q;
            }
            const int npair = head + (np - tail0);
            const int p1 = min(npair, (int)(blockIdx.x + 1) * (PACK_STEP / PB));
            for (int i = blockIdx.x * (PACK_STEP / PB) + lane; i < p1; i += 64) {
                const int x = i < head ? i : tail0 + (i - head);
                const size_t o = (size_t)x * PB;    // U is the pair's second sample
                if constexpr (ES == 2) {
                    const uint16_t sv = *(const uint16_t*)(s + o), su = *(const uint16_t*)(s + o + 2);
                    *(uint16_t*)(d + o) = su; *(uint16_t*)(d + o + 2) = sv;
                } else {
                    const uint8_t sv = s[o], su = s[o + 1];
                    d[o] = su; d[o + 1] = sv;
                }
            }
        } else {                                    // planar: one U row and one V row -> one row of pairs
            const uint8_t* su = sf + a.src_u + crow;
            const uint8_t* sv = sf + a.src_v + crow;
            int head = np;
            if (((uintptr_t)d & (PB - 1)) == 0) {
                const int hp = min(np, (int)(((16 - ((uintptr_t)d & 15)) & 15) / PB));
                if ((((uintptr_t)(su + (size_t)hp * ES) | (uintptr_t)(sv + (size_t)hp * ES)) & (8 * ES - 1)) == 0) head = hp;
            }
            const int nvec = (np - head) >> 3, tail0 = head + (nvec << 3);
            // a lane's group is 16 * ES target bytes: a grid-x step of PACK_STEP bytes holds 64 / ES groups
            const int g0 = blockIdx.x * (64 / ES), g1 = min(nvec, g0 + 64 / ES);
            const int v = g0 + lane;
            if (lane < 64 / ES && v < g1) {
                const uint8_t* pu = su + (size_t)(head + 8 * v) * ES;
                const uint8_t* pv = sv + (size_t)(head + 8 * v) * ES;
                uint8_t* o = d + (size_t)(head + 8 * v) * PB;
                uint32_t w[8];
                if constexpr (ES == 2) {
                    const uint4 p = *(const uint4*)pu, q = *(const uint4*)pv;
                    yuv_join16(p.x, q.x, w[0], w[1]); yuv_join16(p.y, q.y, w[2], w[3]);
                    yuv_join16(p.z, q.z, w[4], w[5]); yuv_join16(p.w, q.w, w[6], w[7]);
                    *(uint4*)o = make_uint4(w[0], w[1], w[2], w[3]);
                    *(uint4*)(o + 16) = make_uint4(w[4], w[5], w[6], w[7]);
                } else {
                    const uint2 p = *(const uint2*)pu, q = *(const uint2*)pv;
                    yuv_join(p.x, q.x, w[0], w[1]); yuv_join(p.y, q.y, w[2], w[3]);
                    *(uint4*)o = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
            const int npair = head + (np - tail0);
            const int p1 = min(npair, (int)(blockIdx.x + 1) * (PACK_STEP / PB));
            for (int i = blockIdx.x * (PACK_STEP / PB) + lane; i < p1; i += 64) {
                const int x = i < head ? i : tail0 + (i - head);
                pack_pair<ES>(su, sv, d, x);
            }
        }
    }
}

template <int ES>
static void launch_yuv420_pack(const YuvPackArgs& a, int step, bool vfirst, dim3 grid, hipStream_t s) {
    const dim3 block(64, PACK_ROWS);
    if (step == 1) hipLaunchKernelGGL((yuv420_pack_kernel<ES, 1, false>), grid, block, 0, s, a);   // U and V by their offsets
    else if (vfirst) hipLaunchKernelGGL((yuv420_pack_kernel<ES, 2, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((yuv420_pack_kernel<ES, 2, false>), grid, block, 0, s, a);
}

}  // namespace

hipError_t vd_launch_yuv420_pack(const Yuv420Dev& src, const Yuv420Dev& ring, int n, int h, int w, hipStream_t s) {
    const size_t es = (size_t)src.es();
    if (n <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1) || !src.base || !ring.base || (src.step != 1 && src.step != 2) ||
        src.pitch < (size_t)w * es || src.cpitch < (size_t)(w / 2) * src.step * es || ring.es() != src.es() ||
        ring.step != 2 || ring.v != ring.u + es || ring.cpitch != ring.pitch || ring.pitch < (size_t)w * es ||
        (size_t)w * es > 0x7fffffffu)
        return hipErrorInvalidValue;
    if (src.nv12()) {   // the kernel NV12 callers have always run
        Nv12PackArgs p{};
        p.src = src.base; p.src_pitch = src.pitch; p.src_uv = src.u; p.src_stride = src.stride;
        p.dst = ring.base; p.dst_pitch = ring.pitch; p.dst_uv = ring.u; p.dst_stride = ring.stride;
        p.n = n; p.h = h; p.w = w;
        return vd_launch_nv12_pack(p, s);
    }
    const uintptr_t even = (uintptr_t)src.base | src.pitch | src.cpitch | src.u | src.v | src.stride | (uintptr_t)ring.base |
                           ring.pitch | ring.u | ring.stride;
    if (es == 2 && (even & 1)) return hipErrorInvalidValue;   // words: the descriptor checks keep every byte quantity even
    if (src.step == 2 && src.u + src.v - 2 * src.c0() != es) return hipErrorInvalidValue;
    YuvPackArgs a{};
    a.src = src.base; a.src_pitch = src.pitch; a.src_u = src.u; a.src_v = src.v; a.src_cp = src.cpitch; a.src_stride = src.stride;
    a.dst = ring.base; a.dst_pitch = ring.pitch; a.dst_uv = ring.u; a.dst_stride = ring.stride;
    a.n = n; a.h = h; a.w = w;
    const long long groups = ((long long)n * (h + h / 2) + PACK_ROWS - 1) / PACK_ROWS;
    const dim3 grid((unsigned)(((size_t)w * es + PACK_STEP - 1) / PACK_STEP), (unsigned)(groups < 65535 ? groups : 65535));
    if (es == 2) launch_yuv420_pack<2>(a, src.step, src.v < src.u, grid, s);
    else launch_yuv420_pack<1>(a, src.step, src.v < src.u, grid, s);
    return hipGetLastError();
}

hipError_t vd_launch_nv12_pack(const Nv12PackArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || (a.h & 1) || (a.w & 1) || a.src_pitch < (size_t)a.w ||
        a.dst_pitch < (size_t)a.w || !a.src || !a.dst)
        return hipErrorInvalidValue;
    const long long groups = ((long long)a.n * (a.h + a.h / 2) + PACK_ROWS - 1) / PACK_ROWS;
    const dim3 grid((a.w + PACK_STEP - 1) / PACK_STEP, (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(nv12_pack_kernel, grid, dim3(64, PACK_ROWS), 0, s, a);
    return hipGetLastError();
}

// every 16-B access of the vector paths is aligned: base, pitches, plane offsets and the stride
static bool yuv_vec_ok(const Yuv420Dev& d) {
    const uintptr_t m = (uintptr_t)d.base | d.pitch | d.cpitch | d.stride | (d.step == 2 ? d.c0() : (d.u | d.v));
    return (m & 15) == 0;
}

template <int IS, int OS, bool SW>
static void launch_mosaic(const Nv12MosaicArgs& a, bool vec, dim3 grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((nv12_mosaic_kernel<true, IS, OS, SW>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((nv12_mosaic_kernel<false, IS, OS, SW>), grid, dim3(256), 0, s, a);
}

template <int IS, int OS>
static void launch_mosaic16(const Nv12MosaicArgs& a, bool vec, dim3 grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((nv12_mosaic_kernel<true, IS, OS, true, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((nv12_mosaic_kernel<false, IS, OS, true, 2>), grid, dim3(256), 0, s, a);
}

hipError_t vd_launch_mosaic_nv12(const Nv12MosaicArgs& a, hipStream_t s, int depth) {
    // sw | sh << 16 holds 16 bits per axis; even sizes only (the chroma planes are (h/2) x (w/2) samples)
    const size_t es = depth ? 2 : 1;
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || (a.h & 1) || (a.w & 1) || a.h > 65534 || a.w > 65534 || a.level < 1 ||
        a.in_pitch < (size_t)a.w * es || a.out_pitch < (size_t)a.w * es || (a.in_step != 1 && a.in_step != 2) ||
        (a.out_step != 1 && a.out_step != 2) || a.in_cp < (size_t)(a.w / 2) * a.in_step * es ||
        a.out_cp < (size_t)(a.w / 2) * a.out_step * es)
        return hipErrorInvalidValue;
    const bool vec = yuv_vec_ok(a.src()) && yuv_vec_ok(a.dst());
    const dim3 grid((a.h + NV12_ROWS - 1) / NV12_ROWS, a.n);
    if (depth) {   // words: every byte quantity even (the descriptor checks), or the word accesses would straddle
        const uintptr_t m = (uintptr_t)a.in | (uintptr_t)a.out | a.in_pitch | a.out_pitch | a.in_cp | a.out_cp | a.in_uv |
                            a.in_v | a.out_uv | a.out_v | a.in_stride | a.out_stride;
        if (m & 1) return hipErrorInvalidValue;
        if (a.in_step == 2 && a.out_step == 2) launch_mosaic16<2, 2>(a, vec, grid, s);
        else if (a.in_step == 2) launch_mosaic16<2, 1>(a, vec, grid, s);
        else if (a.out_step == 2) launch_mosaic16<1, 2>(a, vec, grid, s);
        else launch_mosaic16<1, 1>(a, vec, grid, s);
        return hipGetLastError();
    }
    if (a.nv12()) launch_mosaic<2, 2, false>(a, vec, grid, s);
    else if (a.in_step == 2 && a.out_step == 2) launch_mosaic<2, 2, true>(a, vec, grid, s);
    else if (a.in_step == 2) launch_mosaic<2, 1, true>(a, vec, grid, s);
    else if (a.out_step == 2) launch_mosaic<1, 2, true>(a, vec, grid, s);
    else launch_mosaic<1, 1, true>(a, vec, grid, s);
    return hipGetLastError();
}

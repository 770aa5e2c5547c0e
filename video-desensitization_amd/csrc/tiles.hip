// tiles.hip — tiled face detection: the tile geometry and the cross-tile merge.
//
// Definition (include/vdmi.h at vd_tiles, DESIGN.md "Tiled detection"): with a tiling
// (R, C, O) every frame gives T = 1 + R * C net inputs -- the whole frame and R * C overlapping
// crops at their native scale -- and the per-input keep lists (post.hip, each exactly what
// vd_detect returns for that rectangle as a frame of its own) are merged into one list:
//   map     box i of input t moves by the tile's origin, one float32 add per coordinate
//           (input 0 is left as it is);
//   order   descending score (bit pattern), ties to the lower t, then the lower list position:
//           an ascending sort of the 64-bit keys (~score_bits, t * icap + pos);
//   NMS     the greedy sweep of the post kernel (vd_nms.h) on the mapped boxes, cfg.nms_iou;
//   emit    mapped box, its int(), score, label = t * A + anchor.
// No border rule drops tile boxes near a tile edge: a face cut by a tile edge gives a partial
// box, which the merge either suppresses (IoU with the full box above the threshold) or keeps
// beside it. For an anonymiser, covering more is harmless; dropping a box is not.
//
// tiles_merge_kernel: one 1024-thread workgroup per frame. Up to VD_NMS_LDS_CAND boxes are
// sorted and swept in LDS, more in the per-frame global scratch (as nms_kernel does). The
// merged rows hold T * icap boxes, so nothing is ever dropped. Caller lists are read and
// written with scalar accesses (no alignment assumed).
//
// Tiled plate detection (include/vdmi.h at vd_tiles_nets) merges with the same kernel in its
// PLATE form: the input's label is the box's class, a kept box suppresses boxes of its own class
// only (no class offset: vd_nms.h CLS sweep on the mapped boxes, cfg.plate_iou), and the emitted
// label is the class. With p.split the lists come from two forwards: frame f's whole-frame list
// at row f, its tile t at row n + f * (T - 1) + (t - 1).
#include "vd_common.h"
#include "vd_math.h"
#include "vd_nms.h"

int vd_tile_rects_host(int h, int w, int rows, int cols, int overlap_pct, int32_t* xywh, int* count) {
    if (h <= 0 || w <= 0 || rows < 1 || rows > VD_TILES_MAX || cols < 1 || cols > VD_TILES_MAX || overlap_pct < 0 ||
        overlap_pct > 50)
        return -1;
    // per axis: extent t = min(L, ceil(L * (100 + O) / (100 * K))), origin k = floor(k * (L - t) / (K - 1))
    auto extent = [&](int L, int K) {
        const long long t = ((long long)L * (100 + overlap_pct) + 100LL * K - 1) / (100LL * K);
        return (int)(t < L ? t : L);
    };
    auto origin = [](int L, int t, int K, int k) { return K == 1 ? 0 : (int)(((long long)k * (L - t)) / (K - 1)); };
    const int th = extent(h, rows), tw = extent(w, cols);
    if (xywh) {
        xywh[0] = 0; xywh[1] = 0; xywh[2] = w; xywh[3] = h;
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                int32_t* q = xywh + 4 * (1 + r * cols + c);
                q[0] = origin(w, tw, cols, c);
                q[1] = origin(h, th, rows, r);
                q[2] = tw;
                q[3] = th;
            }
    }
    if (count) *count = 1 + rows * cols;
    return 0;
}

namespace {

// LOW (rescue on a tiled net, p.low_on): the lists are the lists at `low`; the merged rows take the whole
// merged list and m_all its count, m_count / out_count the length of the strong prefix, the caller's arrays
// the strong boxes only -- the split of post.hip's emit(). The merged list is in descending score order, so
// the strong boxes are a prefix of it and the prefix is the merge of the strong prefixes of the inputs. A
// template parameter: the two forms without it keep their instruction streams.
template <bool PLATE, bool LOW>
__global__ __launch_bounds__(VD_NMS_THREADS) void tiles_merge_kernel(TileMergeArgs p) {
    __shared__ __attribute__((aligned(16))) float4 l_box[VD_NMS_LDS_CAND];
    __shared__ __attribute__((aligned(16))) uint64_t l_keys[VD_NMS_LDS_CAND];
    __shared__ float l_area[VD_NMS_LDS_CAND];
    __shared__ int l_cls[PLATE ? VD_NMS_LDS_CAND : 1];
    __shared__ uint8_t l_supp[VD_NMS_LDS_CAND];
    __shared__ uint64_t s_chunk_keep;
    __shared__ int s_nkept;
    __shared__ int s_nstrong;                              // LOW: 1 + the last strong position emitted
    __shared__ int s_off[VD_TILE_INPUTS_MAX + 1];
    const int tid = threadIdx.x;
    const int f = blockIdx.x, T = p.g.T;
    // the row of frame f's input t in the input lists
    auto row = [&](int t) -> size_t {
        if (PLATE && p.split) return t ? (size_t)p.n + (size_t)f * (T - 1) + (t - 1) : (size_t)f;
        return (size_t)f * T + t;
    };
    if (tid == 0) {
        int o = 0;
        for (int t = 0; t < T; ++t) {
            s_off[t] = o;
            o += min(max(p.cnt[row(t)], 0), p.icap);
        }
        s_off[T] = o;
    }
    __syncthreads();
    const int M = s_off[T];                                // <= T * icap <= mcap <= sort_cap
    if (M == 0) {
        if (tid == 0) {
            p.m_count[f] = 0;
            if constexpr (LOW) p.m_all[f] = 0;
            if (p.out_count) p.out_count[f] = 0;
        }
        return;
    }
    const bool lds = M <= VD_NMS_LDS_CAND;
    uint64_t* keys = lds ? l_keys : p.s_keys + (size_t)f * p.sort_cap;
    float4* box = lds ? l_box : p.s_box + (size_t)f * p.mcap;
    float* area = lds ? l_area : p.s_area + (size_t)f * p.mcap;
    uint8_t* supp = lds ? l_supp : p.s_supp + (size_t)f * p.mcap;
    int* cls = PLATE ? (lds ? l_cls : p.s_cls + (size_t)f * p.mcap) : nullptr;
    int P = 1;
    while (P < M) P <<= 1;
    for (int t = 0; t < T; ++t) {
        const int o = s_off[t], c = s_off[t + 1] - o;
        const float* sc = p.score + row(t) * p.icap;
        for (int i = tid; i < c; i += VD_NMS_THREADS)
            keys[o + i] = ((uint64_t)(0xFFFFFFFFu - __float_as_uint(sc[i])) << 32) | (uint32_t)(t * p.icap + i);
    }
    for (int i = M + tid; i < P; i += VD_NMS_THREADS) keys[i] = ~0ULL;
    __syncthreads();
    vd_nms_sort(keys, P);
    for (int i = tid; i < M; i += VD_NMS_THREADS) {
        const int idx = (int)(keys[i] & 0xFFFFFFFFu);
        const int t = idx / p.icap, pos = idx - t * p.icap;
        const float* q = p.xyxy_f + (row(t) * p.icap + pos) * 4;
        float4 bx = make_float4(q[0], q[1], q[2], q[3]);
        if (t) {                                           // one float32 add per coordinate, no FMA
            const float ox = (float)p.g.x0[t], oy = (float)p.g.y0[t];
            bx = make_float4(VD_FADD(bx.x, ox), VD_FADD(bx.y, oy), VD_FADD(bx.z, ox), VD_FADD(bx.w, oy));
        }
        box[i] = bx;
        area[i] = VD_FMUL(VD_FSUB(bx.z, bx.x), VD_FSUB(bx.w, bx.y));
        supp[i] = 0;
        if constexpr (PLATE) cls[i] = p.label ? p.label[row(t) * p.icap + pos] : 0;
    }
    if (tid == 0) {
        s_nkept = 0;
        if constexpr (LOW) s_nstrong = 0;
    }
    __syncthreads();

    vd_nms_greedy_cls<PLATE>(M, box, area, supp, &s_chunk_keep, &s_nkept, p.iou, p.mcap, [&](int pos, int j, const float4& b) {
        const uint64_t key = keys[j];
        const int idx = (int)(key & 0xFFFFFFFFu);
        const int t = idx / p.icap, ipos = idx - t * p.icap;
        const float sc = __uint_as_float(0xFFFFFFFFu - (uint32_t)(key >> 32));
        const int lab = PLATE ? cls[j] : t * p.A + (p.label ? p.label[row(t) * p.icap + ipos] : 0);
        const int4 ib = make_int4(vd_trunc_i32(b.x), vd_trunc_i32(b.y), vd_trunc_i32(b.z), vd_trunc_i32(b.w));
        const size_t k = (size_t)f * p.mcap + pos;
        ((int4*)p.m_xyxy)[k] = ib;
        ((float4*)p.m_xyxy_f)[k] = b;
        p.m_score[k] = sc;
        p.m_label[k] = lab;
        if constexpr (LOW) {                               // the net's own comparison (post.hip emit)
            if (!(PLATE ? sc > p.thr : sc >= p.thr)) return;
            atomicMax(&s_nstrong, pos + 1);
        }
        if (pos >= p.cap || !p.out_xyxy) return;
        const size_t o = (size_t)f * p.cap + pos;
        p.out_xyxy[4 * o + 0] = ib.x; p.out_xyxy[4 * o + 1] = ib.y;
        p.out_xyxy[4 * o + 2] = ib.z; p.out_xyxy[4 * o + 3] = ib.w;
        if (p.out_xyxy_f) {
            p.out_xyxy_f[4 * o + 0] = b.x; p.out_xyxy_f[4 * o + 1] = b.y;
            p.out_xyxy_f[4 * o + 2] = b.z; p.out_xyxy_f[4 * o + 3] = b.w;
        }
        if (p.out_score) p.out_score[o] = sc;
        if (p.out_label) p.out_label[o] = lab;
    }, cls);
    if (tid == 0) {                                        // behind the sweep's last barrier
        if constexpr (LOW) {
            const int own = min(s_nstrong, s_nkept);
            p.m_all[f] = s_nkept;
            p.m_count[f] = own;
            if (p.out_count) p.out_count[f] = own;
        } else {
            p.m_count[f] = s_nkept;
            if (p.out_count) p.out_count[f] = s_nkept;
        }
    }
}

}  // namespace

hipError_t vd_launch_tiles_merge(const TileMergeArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.g.T < 2 || a.g.T > VD_TILE_INPUTS_MAX || a.icap <= 0 || (long long)a.g.T * a.icap > a.mcap ||
        a.sort_cap < a.mcap || (a.sort_cap & (a.sort_cap - 1)) || (long long)a.g.T * a.icap > 0x7fffffffLL)
        return hipErrorInvalidValue;
    if (a.plate && !a.s_cls) return hipErrorInvalidValue;
    if (a.low_on && !a.m_all) return hipErrorInvalidValue;
    const dim3 grid(a.n), block(VD_NMS_THREADS);
    if (a.low_on) {
        if (a.plate) hipLaunchKernelGGL((tiles_merge_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((tiles_merge_kernel<false, true>), grid, block, 0, s, a);
    } else if (a.plate) {
        hipLaunchKernelGGL((tiles_merge_kernel<true, false>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((tiles_merge_kernel<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

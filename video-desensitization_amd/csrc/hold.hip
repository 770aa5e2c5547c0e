// hold.hip — box hold: a box seen in one of the last K frames and matched by nothing since
// stays in the blur list, so one missed detection never shows a face in the clear.
//
// Definition (include/vdmi.h, DESIGN.md "Box hold"): frame t's blur list is B_t = D_t ++ H_t.
// D_t: the frame's own boxes (faces in NMS order, then plates). H_t: for age a = 1..K, in the
// order of D_{t-a}, every box of D_{t-a} that is non-empty after the mosaic's clip
// (combine_detect.py:145-151) and matches no box of D_t .. D_{t-a+1}; two clipped boxes match
// iff 100 * inter >= P * union in 64-bit integers. Every candidate's predicate stands alone
// (no greedy chain), so the kernel is data-parallel over candidates.
//
// Motion mode (vd_hold_motion, HoldArgs::motion; the kernel is instantiated on it, and the
// mode-0 instantiation is the code as it was): membership, order and ages of H_t are unchanged,
// but a kept candidate b = D_{t-a}[i] with clipped box c looks in D_{t-a-1} for its predecessor
// -- among the boxes p whose clip matches c, the one of greatest IoU, compared exactly as
// inter1 * union2 > inter2 * union1 in 64 bits (h, w <= 32768: at most 2^61), lowest list index
// on ties -- and is stored as the hull of b and q = c + a * (c - clip(p)). No predecessor
// (no such frame, or nothing matches): b as stored. The history is K + 1 frames deep then, and
// the clipped boxes of ages 0..K are staged in LDS where they fit (age K + 1, the predecessor
// frame of an age-K candidate, is read and clipped from global memory).
//
// hold_kernel, one launch per call, n + depth workgroups (depth = K, motion: K + 1) of 256
// threads (4 waves of 64):
//   workgroup f < n    frame f. The lists of frames f, f-1, .., f-K come from this call's two
//                      keep lists or, before frame 0, from the history (hold_state.h). The clipped
//                      boxes of frames f .. f-K+1 -- everything a candidate is compared against,
//                      laid out by age, so a candidate of age a reads the prefix [0, off[a]) -- go
//                      to LDS when they number at most LDS_BOXES; otherwise every comparison reads
//                      and clips the box from global memory (L2). D_f is copied to the merged row,
//                      then each age's candidates are taken in rounds of 256, one per lane, looping
//                      over the reference boxes with an early exit; keep flags -> wave ballot +
//                      popcount -> prefix over the 4 waves -> ordered 16-B stores behind a running
//                      offset. The order is therefore age, then list order.
//   workgroup n + j    history slot j of the OTHER buffer: the list of the frame j + 1 before the
//                      next call's frame 0 (a frame of this call, or an old slot shifted by n).
//                      The launch's first K frames still read the old buffer, so nothing is
//                      updated in place.
// hold_gather_kernel copies merged rows into caller-shaped arrays (vd_hold, vd_read_held).
#include "vd_kernel.h"
#include "box_match.h"     // clip_box, boxes_match, boxes_match_iou: shared with lead.hip
#include "hold_state.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int LDS_BOXES = 2048;        // 32 KB of clipped reference boxes

struct Seg {                           // one frame's list: part A then part B
    const int4* a; const int4* b;
    int na, nb;
};

// the list of the frame `age` before frame f (f == n: the frame after the call)
__device__ __forceinline__ Seg seg_of(const HoldArgs& p, int f, int age) {
    Seg s{nullptr, nullptr, 0, 0};
    int idx;
    const int kind = vd_hold_source(f, age, p.hn, &idx);
    if (kind == 1) {
        if (p.cnt0) {
            s.a = (const int4*)p.xy0 + (size_t)idx * p.cap0;
            s.na = min(max(p.cnt0[idx], 0), p.cap0);
        }
        if (p.cnt1) {
            s.b = (const int4*)p.xy1 + (size_t)idx * p.cap1;
            s.nb = min(max(p.cnt1[idx], 0), p.cap1);
        }
    } else if (kind == 2) {
        s.a = (const int4*)p.hist_xy + (size_t)idx * p.hcap;
        s.na = min(max(p.hist_cnt[idx], 0), p.hcap);
    }
    return s;
}

template <int MOTION>
__global__ __launch_bounds__(THREADS) void hold_kernel(HoldArgs p) {
    constexpr int FRM = VD_HOLD_MAX + 1 + MOTION;         // frames a workgroup may name: ages 0..K (motion: 0..K + 1)
    __shared__ __attribute__((aligned(16))) int4 s_ref[LDS_BOXES];
    __shared__ const int4* s_pa[FRM];
    __shared__ const int4* s_pb[FRM];
    __shared__ int s_na[FRM], s_nb[FRM];
    __shared__ int s_off[FRM + 1];
    __shared__ int s_wsum[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int f = blockIdx.x;

    if (f >= p.n) {   // the next history: slot j <- the frame j + 1 before the next call's frame 0
        const int j = f - p.n;
        const Seg s = seg_of(p, p.n, j + 1);
        const int cnt = min(s.na + s.nb, p.hcap);
        int4* dst = (int4*)p.next_xy + (size_t)j * p.hcap;
        for (int i = tid; i < cnt; i += THREADS) dst[i] = i < s.na ? s.a[i] : s.b[i - s.na];
        if (tid == 0) p.next_cnt[j] = cnt;
        return;
    }

    const int last = p.K + MOTION;                        // the oldest frame named: age K (motion: K + 1)
    if (tid <= last) {
        const Seg s = seg_of(p, f, tid);
        s_pa[tid] = s.a; s_pb[tid] = s.b; s_na[tid] = s.na; s_nb[tid] = s.nb;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int j = 0; j <= last; ++j) { s_off[j] = o; o += s_na[j] + s_nb[j]; }
        s_off[last + 1] = o;
    }
    __syncthreads();
    auto load = [&](int j, int i) -> int4 { return i < s_na[j] ? s_pa[j][i] : s_pb[j][i - s_na[j]]; };

    // reference boxes in LDS: frames of age 0..K-1 (motion: 0..K, the predecessor frames of ages 1..K-1 too)
    const int staged = p.K + MOTION;
    const bool in_lds = s_off[staged] <= LDS_BOXES;
    if (in_lds)
        for (int j = 0; j < staged; ++j) {
            const int nj = s_na[j] + s_nb[j], o = s_off[j];
            for (int i = tid; i < nj; i += THREADS) s_ref[o + i] = clip_box(load(j, i), p.w, p.h);
        }
    int4* row = (int4*)p.m_xy + (size_t)f * p.mcap;
    int* age_row = p.m_age + (size_t)f * p.mcap;
    const int own = s_off[1];
    for (int i = tid; i < own; i += THREADS) {             // D_f first, as stored
        row[i] = load(0, i);
        age_row[i] = 0;
    }
    __syncthreads();

    int base = own;
    for (int a = 1; a <= p.K; ++a) {
        const int nc = s_na[a] + s_nb[a];
        for (int c0 = 0; c0 < nc; c0 += THREADS) {         // uniform over the workgroup
            const int c = c0 + tid;
            bool keep = false;
            int4 raw = make_int4(0, 0, 0, 0);
            if (c < nc) {
                raw = load(a, c);
                const int4 q = clip_box(raw, p.w, p.h);
                if (q.z > q.x) {                           // empty after clipping: never held
                    const long long aq = (long long)(q.z - q.x) * (q.w - q.y);
                    keep = true;
                    if (in_lds) {
                        const int nr = s_off[a];
                        for (int i = 0; i < nr; ++i)
                            if (boxes_match(q, aq, s_ref[i], p.P)) { keep = false; break; }
                    } else {
                        for (int j = 0; j < a && keep; ++j) {
                            const int nj = s_na[j] + s_nb[j];
                            for (int i = 0; i < nj; ++i)
                                if (boxes_match(q, aq, clip_box(load(j, i), p.w, p.h), p.P)) { keep = false; break; }
                        }
                    }
                }
            }
            if constexpr (MOTION) {
                if (keep) {                                // keep implies c < nc and q non-empty
                    const int4 q = clip_box(raw, p.w, p.h);
                    const long long aq = (long long)(q.z - q.x) * (q.w - q.y);
                    const int pj = a + 1;                  // the frame before the sighting
                    const int np = s_na[pj] + s_nb[pj];    // 0: no such frame
                    const bool pl = in_lds && pj < staged;
                    const int po = s_off[pj];
                    long long bi = 0, bu = 1;              // best inter / union so far (bi == 0: none)
                    int4 best = q;
                    for (int i = 0; i < np; ++i) {
                        const int4 r = pl ? s_ref[po + i] : clip_box(load(pj, i), p.w, p.h);
                        long long in_, un_;
                        if (boxes_match_iou(q, aq, r, p.P, &in_, &un_) && in_ * bu > bi * un_) {
                            bi = in_; bu = un_; best = r;  // strictly greater: ties keep the lowest index
                        }
                    }
                    // q + a * (q - best) per coordinate; |.| <= 9 * 32768
                    const int px1 = q.x + a * (q.x - best.x), py1 = q.y + a * (q.y - best.y);
                    const int px2 = q.z + a * (q.z - best.z), py2 = q.w + a * (q.w - best.w);
                    raw = make_int4(min(raw.x, px1), min(raw.y, py1), max(raw.z, px2), max(raw.w, py2));
                }
            }
            const uint64_t bal = __ballot(keep);
            if (lane == 0) s_wsum[wid] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int v = 0; v < WAVES; ++v) {
                const int cv = s_wsum[v];
                if (v < wid) before += cv;
                total += cv;
            }
            if (keep) {
                const int pos = base + before + __popcll(bal & ((1ULL << lane) - 1ULL));
                if (pos < p.mcap) {                        // always: mcap = (K + 1) * hcap (vd_common.h)
                    row[pos] = raw;                        // unclipped, as stored (motion: the hull)
                    age_row[pos] = a;
                }
            }
            base += total;
            __syncthreads();                               // s_wsum is rewritten by the next round
        }
    }
    if (tid == 0) {
        p.m_count[f] = base;
        p.m_own[f] = own;
    }
}

__global__ __launch_bounds__(THREADS) void hold_gather_kernel(const int* m_xy, const int* m_age, const int* m_count,
                                                              const int* m_own, int mcap, int held_only,
                                                              int* out_count, int* out_xyxy, int* out_label, int cap) {
    const int f = blockIdx.x;
    const int off = held_only ? m_own[f] : 0;
    const int cnt = m_count[f] - off;
    const int4* src = (const int4*)m_xy + (size_t)f * mcap + off;
    const int* age = m_age + (size_t)f * mcap + off;
    const int k = min(cnt, cap);
    for (int i = threadIdx.x; i < k; i += THREADS) {
        const int4 b = src[i];
        const size_t o = (size_t)f * cap + i;
        out_xyxy[4 * o + 0] = b.x; out_xyxy[4 * o + 1] = b.y;
        out_xyxy[4 * o + 2] = b.z; out_xyxy[4 * o + 3] = b.w;
        if (out_label) out_label[o] = age[i];
    }
    if (threadIdx.x == 0) out_count[f] = cnt;
}

}  // namespace

hipError_t vd_launch_hold(const HoldArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.K <= 0 || a.K > VD_HOLD_MAX || (a.motion != 0 && a.motion != 1)) return hipErrorInvalidValue;
    if (a.motion && (a.h > 32768 || a.w > 32768)) return hipErrorInvalidValue;   // inter * union exact in 64 bits
    if ((a.cnt0 ? a.cap0 : 0) + (a.cnt1 ? a.cap1 : 0) > a.hcap || a.mcap < (a.K + 1) * a.hcap)
        return hipErrorInvalidValue;
    if (a.motion)
        hipLaunchKernelGGL(hold_kernel<1>, dim3(a.n + a.K + 1), dim3(THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(hold_kernel<0>, dim3(a.n + a.K), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t vd_launch_hold_gather(const HoldArgs& a, int n, int held_only, int* out_count, int* out_xyxy,
                                 int* out_label, int cap, hipStream_t s) {
    if (n <= 0 || cap <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hold_gather_kernel, dim3(n), dim3(THREADS), 0, s, (const int*)a.m_xy, (const int*)a.m_age,
                       (const int*)a.m_count, (const int*)a.m_own, a.mcap, held_only, out_count, out_xyxy,
                       out_label, cap);
    return hipGetLastError();
}

// rescue.hip — weak-detection rescue: a box below the net's threshold that continues a track stays
// in the blur list, for at most S frames after the track's last strong sighting.
//
// Definition (include/vdmi.h at vd_rescue, DESIGN.md "Weak-detection rescue"): E_t = D_t ++ R_t.
// D_t: the strong boxes (faces in NMS order, then plates), since = 0. W_t: the weak boxes, per
// net in NMS order. For w in W_t with a non-empty clip c, m(w) = min of since(e) + a over
// a = 1..W and e in E_{t-a} whose clip matches c (box_match.h, the hold's predicate); w is
// rescued iff m(w) <= S, with since(w) = m(w). R_t: the rescued boxes in W_t's order.
//
// Frame f needs R_{f-1}, so the frames of a call cannot all go at once. Two launches per call:
//   rescue_strong_kernel  n workgroups of 256 threads, one per frame. Every weak box against
//       everything that is known before the call runs: the strong lists D of the call's frames
//       f-1 .. f-W (since = 0, so the first matching age is the minimum) and, before frame 0,
//       the history's E rows with their since. The best since so far goes to w_since.
//   rescue_chain_kernel   one workgroup that walks the frames in order: the weak boxes that
//       phase 1 left above a + 1 are tested against the rescued boxes of the call's frames
//       f-1 .. f-W (since >= 1), E_f = D_f ++ R_f is written by an ordered compaction (ballot,
//       popcount, prefix over the waves), and at the end the next history is written into the
//       OTHER buffer (hold_state.h's scheme: slot j is the frame j + 1 before the next call's
//       frame 0; nothing is updated in place).
// In both kernels the clipped reference boxes and their since go to LDS when they number at most
// VD_RESCUE_LDS_BOXES; otherwise every comparison reads and clips the box from global memory.
// rescue_read_kernel copies the weak or the rescued boxes of one net into caller-shaped arrays.
#include "vd_kernel.h"
#include "box_match.h"
#include "hold_state.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int LDS_BOXES = VD_RESCUE_LDS_BOXES;
constexpr int NONE = 0x7fffffff;

struct Seg {                           // one list: part A then part B; since per box, or NULL (all 0)
    const int4* a; const int4* b;
    int na, nb;
    const int* since;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Seg strong_of(const RescueArgs& p, int f) {
    Seg s{nullptr, nullptr, 0, 0, nullptr};
    if (p.cnt0) {
        s.a = (const int4*)p.xy0 + (size_t)f * p.cap0;
        s.na = clampi(p.cnt0[f], 0, p.cap0);
    }
    if (p.cnt1) {
        s.b = (const int4*)p.xy1 + (size_t)f * p.cap1;
        s.nb = clampi(p.cnt1[f], 0, p.cap1);
    }
    return s;
}

__device__ __forceinline__ Seg weak_of(const RescueArgs& p, int f) {
    Seg s{nullptr, nullptr, 0, 0, nullptr};
    if (p.split) {
        if (p.wcnt) {
            s.a = (const int4*)p.wxy + (size_t)f * p.wcap;
            s.na = clampi(p.wcnt[f], 0, p.wcap);
        }
        return s;
    }
    if (p.cnt0 && p.all0) {
        const int o = clampi(p.cnt0[f], 0, p.cap0);
        s.a = (const int4*)p.xy0 + (size_t)f * p.cap0 + o;
        s.na = clampi(p.all0[f], o, p.cap0) - o;
    }
    if (p.cnt1 && p.all1) {
        const int o = clampi(p.cnt1[f], 0, p.cap1);
        s.b = (const int4*)p.xy1 + (size_t)f * p.cap1 + o;
        s.nb = clampi(p.all1[f], o, p.cap1) - o;
    }
    return s;
}

__device__ __forceinline__ Seg hist_of(const RescueArgs& p, int slot) {
    Seg s{nullptr, nullptr, 0, 0, nullptr};
    s.a = (const int4*)p.hist_xy + (size_t)slot * p.hcap;
    s.na = clampi(p.hist_cnt[slot], 0, p.hcap);
    s.since = p.hist_since + (size_t)slot * p.hcap;
    return s;
}

// the rescued boxes of the call's frame g, from its finished E row
__device__ __forceinline__ Seg rescued_of(const RescueArgs& p, int g) {
    Seg s{nullptr, nullptr, 0, 0, nullptr};
    const int own = clampi(p.e_own[g], 0, p.ecap);
    s.a = (const int4*)p.e_xy + (size_t)g * p.ecap + own;
    s.na = clampi(p.e_count[g], own, p.ecap) - own;
    s.since = p.e_since + (size_t)g * p.ecap + own;
    return s;
}

__device__ __forceinline__ int4 seg_box(const Seg& s, int i) { return i < s.na ? s.a[i] : s.b[i - s.na]; }

// Up to W reference lists by age (s_seg[a - 1]: age a, empty where there is no such frame) -> the
// offsets, and the clipped boxes + since in LDS where they fit. Ends with a barrier.
__device__ __forceinline__ bool stage_refs(const RescueArgs& p, const Seg* s_seg, int* s_off, int4* s_ref, int* s_rs) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int o = 0;
        for (int j = 0; j < p.W; ++j) { s_off[j] = o; o += s_seg[j].na + s_seg[j].nb; }
        s_off[p.W] = o;
    }
    __syncthreads();
    const bool in_lds = s_off[p.W] <= LDS_BOXES;
    if (in_lds)
        for (int j = 0; j < p.W; ++j) {
            const Seg s = s_seg[j];
            const int nj = s.na + s.nb, o = s_off[j];
            for (int i = tid; i < nj; i += THREADS) {
                s_ref[o + i] = clip_box(seg_box(s, i), p.w, p.h);
                s_rs[o + i] = s.since ? s.since[i] : 0;
            }
        }
    __syncthreads();
    return in_lds;
}

// min(best, since(e) + a) over the staged lists' boxes that match q. floor_since: the least since a
// reference can have (0: strong boxes present, 1: rescued boxes only), which ends the walk early.
__device__ __forceinline__ int scan_refs(const RescueArgs& p, const Seg* s_seg, const int* s_off, const int4* s_ref,
                                         const int* s_rs, bool in_lds, int4 q, int best, int floor_since) {
    const long long aq = (long long)(q.z - q.x) * (q.w - q.y);
    for (int a = 1; a <= p.W; ++a) {
        if (best <= a + floor_since) break;              // no later age can do better
        const int o = s_off[a - 1], nj = s_off[a] - o;
        if (in_lds) {
            for (int i = 0; i < nj; ++i) {
                const int c = s_rs[o + i] + a;
                if (c < best && boxes_match(q, aq, s_ref[o + i], p.P)) best = c;
            }
        } else {
            const Seg s = s_seg[a - 1];
            for (int i = 0; i < nj; ++i) {
                const int c = (s.since ? s.since[i] : 0) + a;
                if (c < best && boxes_match(q, aq, clip_box(seg_box(s, i), p.w, p.h), p.P)) best = c;
            }
        }
    }
    return best;
}

__global__ __launch_bounds__(THREADS) void rescue_strong_kernel(RescueArgs p) {
    __shared__ __attribute__((aligned(16))) int4 s_ref[LDS_BOXES];
    __shared__ int s_rs[LDS_BOXES];
    __shared__ Seg s_seg[VD_HOLD_MAX];
    __shared__ int s_off[VD_HOLD_MAX + 1];
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    if (tid < p.W) {
        int idx;
        const int kind = vd_hold_source(f, tid + 1, p.hn, &idx);
        s_seg[tid] = kind == 1 ? strong_of(p, idx) : (kind == 2 ? hist_of(p, idx) : Seg{nullptr, nullptr, 0, 0, nullptr});
    }
    __syncthreads();
    const bool in_lds = stage_refs(p, s_seg, s_off, s_ref, s_rs);
    const Seg wk = weak_of(p, f);
    const int nw = min(wk.na + wk.nb, p.wtot);
    int* ws = p.w_since + (size_t)f * p.wtot;
    for (int c = tid; c < nw; c += THREADS) {
        const int4 q = clip_box(seg_box(wk, c), p.w, p.h);
        int best = NONE;
        if (q.z > q.x) best = scan_refs(p, s_seg, s_off, s_ref, s_rs, in_lds, q, best, 0);
        ws[c] = best;
    }
}

__global__ __launch_bounds__(THREADS) void rescue_chain_kernel(RescueArgs p) {
    __shared__ __attribute__((aligned(16))) int4 s_ref[LDS_BOXES];
    __shared__ int s_rs[LDS_BOXES];
    __shared__ Seg s_seg[VD_HOLD_MAX];
    __shared__ int s_off[VD_HOLD_MAX + 1];
    __shared__ int s_wsum[WAVES], s_wsum0[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    for (int f = 0; f < p.n; ++f) {
        if (tid < p.W)
            s_seg[tid] = f - (tid + 1) >= 0 ? rescued_of(p, f - (tid + 1)) : Seg{nullptr, nullptr, 0, 0, nullptr};
        __syncthreads();
        const bool in_lds = stage_refs(p, s_seg, s_off, s_ref, s_rs);
        const bool any = s_off[p.W] > 0;
        const Seg st = strong_of(p, f), wk = weak_of(p, f);
        int4* row = (int4*)p.e_xy + (size_t)f * p.ecap;
        int* since_row = p.e_since + (size_t)f * p.ecap;
        const int own = min(st.na + st.nb, p.ecap);
        for (int i = tid; i < own; i += THREADS) {          // D_f first, as stored
            row[i] = seg_box(st, i);
            since_row[i] = 0;
        }
        const int nw = min(wk.na + wk.nb, p.wtot);
        int* ws = p.w_since + (size_t)f * p.wtot;
        int base = own, nr0 = 0;
        for (int c0 = 0; c0 < nw; c0 += THREADS) {          // uniform over the workgroup
            const int c = c0 + tid;
            bool keep = false;
            int best = NONE;
            int4 raw = make_int4(0, 0, 0, 0);
            if (c < nw) {
                raw = seg_box(wk, c);
                best = ws[c];
                const int4 q = clip_box(raw, p.w, p.h);
                if (q.z > q.x && any) best = scan_refs(p, s_seg, s_off, s_ref, s_rs, in_lds, q, best, 1);
                keep = q.z > q.x && best <= p.S;
                ws[c] = keep ? best : 0;
            }
            const uint64_t bal = __ballot(keep), bal0 = __ballot(keep && c < wk.na);
            if (lane == 0) { s_wsum[wid] = __popcll(bal); s_wsum0[wid] = __popcll(bal0); }
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int v = 0; v < WAVES; ++v) {
                const int cv = s_wsum[v];
                if (v < wid) before += cv;
                total += cv;
                nr0 += s_wsum0[v];
            }
            if (keep) {
                const int pos = base + before + __popcll(bal & ((1ULL << lane) - 1ULL));
                if (pos < p.ecap) {                         // always: ecap >= |D| + |W|
                    row[pos] = raw;
                    since_row[pos] = best;
                }
            }
            base += total;
            __syncthreads();                                // s_wsum is rewritten by the next round
        }
        if (tid == 0) {
            p.e_count[f] = min(base, p.ecap);
            p.e_own[f] = own;
            p.e_nr0[f] = nr0;
        }
        __threadfence_block();                              // the row is read by this workgroup's later frames
        __syncthreads();
    }

    // the next history: slot j <- E of the frame j + 1 before the next call's frame 0
    for (int j = 0; j < p.W; ++j) {
        int idx;
        const int kind = vd_hold_source(p.n, j + 1, p.hn, &idx);
        const int4* sx = nullptr;
        const int* ss = nullptr;
        int cnt = 0;
        if (kind == 1) {
            sx = (const int4*)p.e_xy + (size_t)idx * p.ecap;
            ss = p.e_since + (size_t)idx * p.ecap;
            cnt = clampi(p.e_count[idx], 0, p.ecap);
        } else if (kind == 2) {
            sx = (const int4*)p.hist_xy + (size_t)idx * p.hcap;
            ss = p.hist_since + (size_t)idx * p.hcap;
            cnt = clampi(p.hist_cnt[idx], 0, p.hcap);
        }
        cnt = min(cnt, p.hcap);
        int4* dx = (int4*)p.next_xy + (size_t)j * p.hcap;
        int* ds = p.next_since + (size_t)j * p.hcap;
        for (int i = tid; i < cnt; i += THREADS) { dx[i] = sx[i]; ds[i] = ss[i]; }
        if (tid == 0) p.next_cnt[j] = cnt;
    }
}

__global__ __launch_bounds__(THREADS) void rescue_read_kernel(RescueReadArgs p) {
    __shared__ int s_wsum[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int f = blockIdx.x;
    const int o = clampi(p.cnt[f], 0, p.kcap);
    const int nw = clampi(p.all[f], o, p.kcap) - o;
    int woff = 0;
    if (p.list == 1 && p.cnt_o && p.all_o) {
        const int oo = clampi(p.cnt_o[f], 0, p.kcap_o);
        woff = clampi(p.all_o[f], oo, p.kcap_o) - oo;
    }
    const size_t src = (size_t)f * p.kcap + o;
    const int* ws = p.w_since + (size_t)f * p.wtot + woff;
    auto put = [&](int pos, int i, int lab) {
        if (pos >= p.cap) return;
        const size_t d = (size_t)f * p.cap + pos;
        for (int k = 0; k < 4; ++k) p.out_xyxy[4 * d + k] = p.xy[4 * (src + i) + k];
        if (p.out_xyxy_f) for (int k = 0; k < 4; ++k) p.out_xyxy_f[4 * d + k] = p.xy_f[4 * (src + i) + k];
        if (p.out_score) p.out_score[d] = p.score[src + i];
        if (p.out_label) p.out_label[d] = lab;
    };
    if (p.which == 1) {
        for (int i = tid; i < nw; i += THREADS) put(i, i, p.label[src + i]);
        if (tid == 0) p.out_count[f] = nw;
        return;
    }
    int base = 0;
    for (int c0 = 0; c0 < nw; c0 += THREADS) {
        const int c = c0 + tid;
        const int sn = c < nw && woff + c < p.wtot ? ws[c] : 0;
        const bool keep = sn > 0;
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
        if (keep) put(base + before + __popcll(bal & ((1ULL << lane) - 1ULL)), c, sn);
        base += total;
        __syncthreads();
    }
    if (tid == 0) p.out_count[f] = base;
}

}  // namespace

hipError_t vd_launch_rescue(const RescueArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.W <= 0 || a.W > VD_HOLD_MAX || a.S < 1 || a.hn < 0 || a.hn > a.W) return hipErrorInvalidValue;
    const int strong = (a.cnt0 ? a.cap0 : 0) + (a.cnt1 ? a.cap1 : 0);
    const int weak = a.split ? (a.wcnt ? a.wcap : 0) : strong;
    if ((a.split ? strong + weak : strong) > a.ecap || a.ecap > a.hcap || weak > a.wtot) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rescue_strong_kernel, dim3(a.n), dim3(THREADS), 0, s, a);
    hipLaunchKernelGGL(rescue_chain_kernel, dim3(1), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t vd_launch_rescue_read(const RescueReadArgs& a, int n, hipStream_t s) {
    if (n <= 0 || a.cap <= 0 || !a.cnt || !a.all || !a.w_since) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rescue_read_kernel, dim3(n), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

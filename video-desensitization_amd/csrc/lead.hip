// lead.hip — look-ahead hold: a box first seen in one of the next J frames, and matched by
// nothing before, is already in the blur list, so a face never reaches the output in the clear
// just because its first detection came a frame late.
//
// Definition (include/vdmi.h, DESIGN.md "Look-ahead hold"): frame t's blur list is
// B_t = D_t ++ H_t ++ A_t. D_t ++ H_t is the box hold's row (hold.hip; D_t alone without hold),
// final when frame t is pushed. A_t is the hold list of the time-reversed stream: for age
// a = 1..J, in the order of D_{t+a}, every box of D_{t+a} that is non-empty after the mosaic's
// clip and matches no box of D_t .. D_{t+a-1} (box_match.h: the predicate of hold.hip). Every
// candidate's predicate stands alone, so the kernel is data-parallel over candidates.
//
// Motion mode (vd_lead, LeadArgs::motion; the kernel is instantiated on it): membership, order
// and ages are unchanged, but a kept candidate b = D_{t+a}[i] with clipped box c looks in
// D_{t+a+1} for its predecessor in reversed time -- the box the face becomes one frame later --
// by the rules of hold.hip (greatest exact IoU among the matches, lowest index on ties) and is
// stored as the hull of b and q = c + a * (c - clip(p)): stretched backwards along the way the
// face came. No such frame (the stream ended) or no match: b as stored.
//
// The frames a call can name are the window W = pending ring ++ this call's frames
// (lead_state.h). lead_kernel, one launch per call, m + keep workgroups of 256 threads
// (4 waves of 64):
//   workgroup e < m    emitted frame e = W[e]. The lists of W[e] .. W[e + J] (motion: + 1)
//                      come from the ring's D slots or from this call's two keep lists
//                      (vd_lead_source, the mirror of vd_hold_source). The clipped boxes of
//                      W[e] .. W[e + J - 1] -- everything a candidate is compared against, laid
//                      out by age, so a candidate of age a reads the prefix [0, off[a]) -- go to
//                      LDS when they number at most LDS_BOXES; otherwise every comparison reads
//                      and clips the box from global memory (L2). The frame's stored D ++ H row
//                      is copied to the merged row, then each age's candidates are taken in
//                      rounds of 256, one per lane, with the ballot / popcount / prefix scheme
//                      of hold_kernel. The order is therefore D, H, then A by age and list order.
//   workgroup m + j    slot j of the OTHER ring buffer <- W[m + j]: its D list and its D ++ H
//                      row. The emitted frames still read the old buffer, so nothing is updated
//                      in place.
#include "vd_kernel.h"
#include "box_match.h"
#include "lead_state.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int LDS_BOXES = 2048;        // 32 KB of clipped reference boxes, as in hold.hip

struct Seg {                           // one frame's D list: part A then part B
    const int4* a; const int4* b;
    int na, nb;
};

struct Ring {                          // one ring buffer, taken apart (vd_lead_ring_ints gives its size)
    int* d_cnt; int* dh_cnt; int* dh_own;
    int4* d_xy; int4* dh_xy; int* dh_age;
};

__device__ __forceinline__ Ring ring_of(int* base, int slots, int hcap, int rcap) {
    Ring r;
    r.d_cnt = base; r.dh_cnt = base + slots; r.dh_own = base + 2 * slots;
    r.d_xy = (int4*)(base + VD_LEAD_RING_HEAD);
    r.dh_xy = r.d_xy + (size_t)slots * hcap;
    r.dh_age = (int*)(r.dh_xy + (size_t)slots * rcap);
    return r;
}

// the D list of frame i of the window
__device__ __forceinline__ Seg seg_of(const LeadArgs& p, const Ring& cur, int i) {
    Seg s{nullptr, nullptr, 0, 0};
    int idx;
    const int kind = vd_lead_source(i, p.pend, p.n, &idx);
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
        s.a = cur.d_xy + (size_t)idx * p.hcap;
        s.na = min(max(cur.d_cnt[idx], 0), p.hcap);
    }
    return s;
}

// Copies the stored D ++ H row of window frame i (ring slot, this call's hold row, or -- without
// hold -- this call's D list) to dst / dst_age, at most cap boxes; returns through *cnt / *own.
__device__ __forceinline__ void copy_dh(const LeadArgs& p, const Ring& cur, int i, int4* dst, int* dst_age, int cap,
                                        int tid, int* cnt_out, int* own_out) {
    int idx;
    const int kind = vd_lead_source(i, p.pend, p.n, &idx);
    int cnt = 0, own = 0;
    if (kind == 2) {
        cnt = min(min(max(cur.dh_cnt[idx], 0), p.rcap), cap);
        own = min(max(cur.dh_own[idx], 0), cnt);
        const int4* sx = cur.dh_xy + (size_t)idx * p.rcap;
        const int* sa = cur.dh_age + (size_t)idx * p.rcap;
        for (int k = tid; k < cnt; k += THREADS) { dst[k] = sx[k]; dst_age[k] = sa[k]; }
    } else if (kind == 1 && p.dh_xy) {
        cnt = min(min(max(p.dh_count[idx], 0), p.dh_cap), cap);
        own = min(max(p.dh_own[idx], 0), cnt);
        const int4* sx = (const int4*)p.dh_xy + (size_t)idx * p.dh_cap;
        const int* sa = p.dh_age + (size_t)idx * p.dh_cap;
        for (int k = tid; k < cnt; k += THREADS) { dst[k] = sx[k]; dst_age[k] = sa[k]; }
    } else if (kind == 1) {
        const Seg s = seg_of(p, cur, i);
        cnt = own = min(s.na + s.nb, cap);
        for (int k = tid; k < cnt; k += THREADS) { dst[k] = k < s.na ? s.a[k] : s.b[k - s.na]; dst_age[k] = 0; }
    }
    *cnt_out = cnt;
    *own_out = own;
}

template <int MOTION>
__global__ __launch_bounds__(THREADS) void lead_kernel(LeadArgs p) {
    constexpr int FRM = VD_LEAD_MAX + 1 + MOTION;         // frames a workgroup may name: ages 0..J (motion: 0..J + 1)
    __shared__ __attribute__((aligned(16))) int4 s_ref[LDS_BOXES];
    __shared__ const int4* s_pa[FRM];
    __shared__ const int4* s_pb[FRM];
    __shared__ int s_na[FRM], s_nb[FRM];
    __shared__ int s_off[FRM + 1];
    __shared__ int s_wsum[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int e = blockIdx.x;
    const Ring cur = ring_of(const_cast<int*>(p.ring), p.slots, p.hcap, p.rcap);

    if (e >= p.m) {   // the next ring: slot j <- window frame m + j
        const int j = e - p.m;
        if (j >= p.keep || j >= p.slots) return;
        const Ring nxt = ring_of(p.next, p.slots, p.hcap, p.rcap);
        const Seg s = seg_of(p, cur, p.m + j);
        const int cnt = min(s.na + s.nb, p.hcap);
        int4* dst = nxt.d_xy + (size_t)j * p.hcap;
        for (int i = tid; i < cnt; i += THREADS) dst[i] = i < s.na ? s.a[i] : s.b[i - s.na];
        int dhc, dho;
        copy_dh(p, cur, p.m + j, nxt.dh_xy + (size_t)j * p.rcap, nxt.dh_age + (size_t)j * p.rcap, p.rcap, tid, &dhc,
                &dho);
        if (tid == 0) { nxt.d_cnt[j] = cnt; nxt.dh_cnt[j] = dhc; nxt.dh_own[j] = dho; }
        return;
    }

    const int last = p.J + MOTION;                        // the newest frame named: age J (motion: J + 1)
    if (tid <= last) {
        const Seg s = seg_of(p, cur, e + tid);
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

    // reference boxes in LDS: frames of age 0..J-1 (motion: 0..J, the predecessor frames of ages 1..J-1 too)
    const int staged = p.J + MOTION;
    const bool in_lds = s_off[staged] <= LDS_BOXES;
    if (in_lds)
        for (int j = 0; j < staged; ++j) {
            const int nj = s_na[j] + s_nb[j], o = s_off[j];
            for (int i = tid; i < nj; i += THREADS) s_ref[o + i] = clip_box(load(j, i), p.w, p.h);
        }
    int4* row = (int4*)p.m_xy + (size_t)e * p.mcap;
    int* age_row = p.m_age + (size_t)e * p.mcap;
    int dh, own;
    copy_dh(p, cur, e, row, age_row, p.mcap, tid, &dh, &own);   // D_e ++ H_e first, as stored
    __syncthreads();

    int base = dh;
    for (int a = 1; a <= p.J; ++a) {
        const int nc = s_na[a] + s_nb[a];
        for (int c0 = 0; c0 < nc; c0 += THREADS) {         // uniform over the workgroup
            const int c = c0 + tid;
            bool keep = false;
            int4 raw = make_int4(0, 0, 0, 0);
            if (c < nc) {
                raw = load(a, c);
                const int4 q = clip_box(raw, p.w, p.h);
                if (q.z > q.x) {                           // empty after clipping: never led
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
                    const int pj = a + 1;                  // the frame after the sighting
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
                if (pos < p.mcap) {                        // always: mcap = rcap + J * hcap (vd_common.h)
                    row[pos] = raw;                        // unclipped, as stored (motion: the hull)
                    age_row[pos] = -a;                     // label: led from frame t + a
                }
            }
            base += total;
            __syncthreads();                               // s_wsum is rewritten by the next round
        }
    }
    if (tid == 0) {
        p.m_count[e] = min(base, p.mcap);
        p.m_own[e] = own;
        p.m_dh[e] = dh;
    }
}

}  // namespace

size_t vd_lead_ring_ints(int slots, int hcap, int rcap) {
    return (size_t)VD_LEAD_RING_HEAD + (size_t)slots * hcap * 4 + (size_t)slots * rcap * 4 + (size_t)slots * rcap;
}

hipError_t vd_launch_lead(const LeadArgs& a, hipStream_t s) {
    if (a.J <= 0 || a.J > VD_LEAD_MAX || (a.motion != 0 && a.motion != 1)) return hipErrorInvalidValue;
    if (a.motion && (a.h > 32768 || a.w > 32768)) return hipErrorInvalidValue;   // inter * union exact in 64 bits
    const int delay = a.J + a.motion;
    if (a.n < 0 || a.m < 0 || a.pend < 0 || a.keep < 0 || a.pend > delay || a.keep > delay || a.slots != delay ||
        a.m + a.keep != a.pend + a.n || 3 * a.slots > VD_LEAD_RING_HEAD)
        return hipErrorInvalidValue;
    if ((a.cnt0 ? a.cap0 : 0) + (a.cnt1 ? a.cap1 : 0) > a.hcap || a.rcap < a.hcap || a.mcap < a.rcap + a.J * a.hcap ||
        (a.dh_xy && a.dh_cap > a.rcap))
        return hipErrorInvalidValue;
    if (a.n > 0 && !a.cnt0 && !a.cnt1) return hipErrorInvalidValue;
    if (!a.ring || !a.next || (a.m > 0 && (!a.m_xy || !a.m_age || !a.m_count || !a.m_own || !a.m_dh)))
        return hipErrorInvalidValue;
    if (a.m + a.keep == 0) return hipSuccess;
    if (a.motion)
        hipLaunchKernelGGL(lead_kernel<1>, dim3(a.m + a.keep), dim3(THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(lead_kernel<0>, dim3(a.m + a.keep), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

// track.cpp — lists that follow boxes across frames: box hold, look-ahead hold and
// weak-detection rescue, host side, with their entries.

#include "../../include/vdmi.h"
#include "vd_common.h"
#include "vd_math.h"
#include "nets.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// ---- box hold (hold.hip, hold_state.h) ----
// History buffers of at least `hcap` boxes per slot; the valid slots of a smaller pair are
// carried over (weights loaded, or a wider vd_hold list, after the first holding call).
int Ctx::hold_history(int hcap) {
    if (hcap <= hold_hcap) return VD_OK;
    const int K = hold.depth();                   // slots: hold_frames, one more in motion mode
    int rc = regrow_pair(hold_hist, 64 + (size_t)K * hcap * 16, 64, hold_hist[0] && hold.hn > 0 ? hold.cur : -1,
                         (size_t)K * 4, K, {{(size_t)hold_hcap * 16, (size_t)hcap * 16}}, "hold history");
    if (rc) return rc;
    hold_hcap = hcap;
    return VD_OK;
}

int Ctx::regrow_pair(int* (&buf)[2], size_t bytes, size_t head, int cur, size_t head_copy, int slots,
                     std::initializer_list<PlaneRows> planes, const char* what) {
    int* nb[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i)
        if (hipMalloc((void**)&nb[i], bytes) != hipSuccess) {
            if (nb[0]) hipFree(nb[0]);
            return vd_set_error(VD_ERR_NOMEM, "hipMalloc(%zu) failed (%s)", bytes, what);
        }
    for (int i = 0; i < 2; ++i) VD_CHECK_HIP(hipMemsetAsync(nb[i], 0, head, stream));
    if (cur >= 0) {
        const char* src = (const char*)buf[cur];
        char* dst = (char*)nb[cur];
        VD_CHECK_HIP(hipMemcpyAsync(dst, src, head_copy, hipMemcpyDeviceToDevice, stream));
        src += head; dst += head;
        for (const PlaneRows& p : planes) {
            VD_CHECK_HIP(hipMemcpy2DAsync(dst, p.new_row, src, p.old_row, p.old_row, slots, hipMemcpyDeviceToDevice,
                                          stream));
            src += (size_t)slots * p.old_row; dst += (size_t)slots * p.new_row;
        }
    }
    VD_CHECK_HIP(hipStreamSynchronize(stream));   // a queued launch may still read the old pair
    for (int i = 0; i < 2; ++i) {
        if (buf[i]) hipFree(buf[i]);
        buf[i] = nb[i];
    }
    return VD_OK;
}

// The buffers are sized by the depth (K or K + 1 slots), so a change of mode drops them; the
// next holding call allocates them anew. The last call's merged rows stay readable.
int Ctx::hold_set_motion(int mode) {
    if (mode == hold.motion) return VD_OK;
    VD_CHECK_HIP(hipStreamSynchronize(stream));   // a queued launch may still read the history
    for (int i = 0; i < 2; ++i) {
        if (hold_hist[i]) hipFree(hold_hist[i]);
        hold_hist[i] = nullptr;
    }
    hold_hcap = 0;
    hold.motion = mode;
    hold.reset();
    return VD_OK;
}

int Ctx::launch_hold(int n, int h, int w, const int* cnt0, const int* xy0, int cap0, const int* cnt1, const int* xy1,
                     int cap1) {
    const int K = hold.K;
    if (hold.motion && (h > 32768 || w > 32768))  // inter * union <= 2^61 stays exact in 64 bits
        return vd_set_error(VD_ERR_ARG, "hold motion: frames of at most 32768 x 32768 (got %d x %d)", h, w);
    // rows sized for the loaded detectors' complete keep lists (vd_process never regrows them)
    // and for this call's lists; (K + 1) rows of that size hold D and K complete older lists
    const int nets = (face.loaded ? face_rows_cap() : 0) + (plate.loaded ? plate_rows_cap() : 0);
    const int need = std::max(std::max((cnt0 ? cap0 : 0) + (cnt1 ? cap1 : 0), nets), 1);
    int rc = hold_history(need);
    if (rc) return rc;
    const size_t mcap = (size_t)(K + 1) * hold_hcap;
    if (mcap > 0x7fffffffu) return vd_set_error(VD_ERR_ARG, "hold: list capacity too large");
    const size_t nb = (size_t)n * mcap;
    if ((rc = ensure_staging(&hold_rows, &hold_rows_bytes, nb * 16 + nb * 4 + (size_t)n * 8 + 64))) return rc;
    hold.begin(h, w);
    HoldArgs a{};
    a.n = n; a.h = h; a.w = w; a.K = K; a.P = hold.P; a.motion = hold.motion;
    a.cnt0 = cnt0; a.xy0 = xy0; a.cap0 = cap0;
    a.cnt1 = cnt1; a.xy1 = xy1; a.cap1 = cap1;
    a.hist_cnt = hold_hist[hold.cur]; a.hist_xy = hold_hist[hold.cur] + 16;
    a.next_cnt = hold_hist[hold.cur ^ 1]; a.next_xy = hold_hist[hold.cur ^ 1] + 16;
    a.hcap = hold_hcap; a.hn = hold.hn;
    a.m_xy = (int*)hold_rows; a.m_age = a.m_xy + nb * 4; a.m_count = a.m_age + nb; a.m_own = a.m_count + n;
    a.mcap = (int)mcap;
    t_begin(3, (double)n * (K + 1) * 16);
    hipError_t e = vd_launch_hold(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "hold: %s", hipGetErrorString(e));
    hold.end(n);
    hold_last = a;
    hold_n = n;
    return VD_OK;
}

int Ctx::hold_read(int n, int held_only, vd_boxes* out) {
    if (!hold.K) return vd_set_error(VD_ERR_STATE, "context created with hold_frames == 0");
    if (!hold_n) return vd_set_error(VD_ERR_STATE, "no holding call yet");
    if (!out || !out->count || !out->xyxy || out->cap <= 0) return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    if (n <= 0 || n > hold_n) return vd_set_error(VD_ERR_ARG, "n=%d outside [1, %d frames of the last call]", n, hold_n);
    return rows_out(hold_last, n, held_only, out, "hold");
}

// ---- look-ahead hold (lead.hip, lead_state.h) ----
// The D-list capacity of a ring slot: the loaded detectors' complete keep lists, this call's
// lists, and whatever the hold history already carries (its rows are copied into the ring).
int Ctx::lead_need(int cap0, int cap1) const {
    const int nets = (face.loaded ? face_rows_cap() : 0) + (plate.loaded ? plate_rows_cap() : 0);
    return std::max(std::max(std::max(cap0 + cap1, nets), hold.K ? hold_hcap : 0), 1);
}

// Everything a lead call can be refused for, before any state changes.
int Ctx::lead_check(const char* who, int mode, int n, int h, int w, size_t pitch, int flush, int depth, int shift) {
    if (!lead.J) return vd_set_error(VD_ERR_STATE, "%s: look-ahead hold is off (vd_lead)", who);
    if (n < 0 || (n == 0 && !flush)) return vd_set_error(VD_ERR_ARG, "%s: n == 0 is allowed only with flush", who);
    if (h <= 0 || w <= 0) return vd_set_error(VD_ERR_ARG, "%s: bad geometry %dx%d", who, w, h);
    if ((lead.motion || (hold.K && hold.motion)) && (h > 32768 || w > 32768))
        return vd_set_error(VD_ERR_ARG, "%s: motion needs frames of at most 32768 x 32768 (got %d x %d)", who, w, h);
    if (lead.pend) {
        if (!vd_lead_mode_ok(lead.pend, lead.mode, mode))
            return vd_set_error(VD_ERR_STATE, "%s: %d frames are pending from %s (flush first)", who, lead.pend,
                                vd_lead_mode_caller(lead.mode));
        if (lead.h != h || lead.w != w || (mode == VD_LEAD_MODE_PIXELS && lead.pitch != (unsigned long long)pitch))
            return vd_set_error(VD_ERR_STATE, "%s: %d frames of %dx%d (pitch %llu) are pending; got %dx%d (pitch %zu): "
                                "flush first", who, lead.pend, lead.w, lead.h, lead.pitch, w, h, pitch);
        if (!lead.format_ok(mode, depth, shift))   // the ring holds the words as pushed
            return vd_set_error(VD_ERR_STATE, "%s: %d frames of depth %d, shift %d are pending; got depth %d, shift %d: "
                                "flush first", who, lead.pend, lead.depth, lead.shift, depth, shift);
    }
    return VD_OK;
}

void Ctx::lead_free() {
    for (int i = 0; i < 2; ++i) {
        if (lead_ring[i]) hipFree(lead_ring[i]);
        lead_ring[i] = nullptr;
    }
    if (lead_pix) hipFree(lead_pix);
    lead_pix = nullptr;
    lead_pix_bytes = 0;
    lead_hcap = lead_slots = 0;
}

// Ring buffers of at least `need` boxes per D list, and (frame_bytes > 0) the pixel ring. The
// pending slots of a narrower pair are carried over (a wider vd_lead_lists list, or weights
// loaded, while frames are pending); the slot count changes only while nothing is pending.
int Ctx::lead_buffers(int need, size_t frame_bytes) {
    const int slots = lead.delay();
    if (need > lead_hcap || slots != lead_slots) {
        const size_t rcap = (size_t)(hold.K + 1) * need;
        if (rcap + (size_t)lead.J * need > 0x7fffffffu) return vd_set_error(VD_ERR_ARG, "lead: list capacity too large");
        const size_t oh = (size_t)lead_hcap, orc = (size_t)(hold.K + 1) * oh, head = VD_LEAD_RING_HEAD * 4;
        const bool carry = lead_ring[0] && lead.pend > 0 && slots == lead_slots;
        // the D lists, the hold rows and their ages of every slot
        int rc = regrow_pair(lead_ring, vd_lead_ring_ints(slots, need, (int)rcap) * 4, head, carry ? lead.cur : -1, head,
                             slots, {{oh * 16, (size_t)need * 16}, {orc * 16, rcap * 16}, {orc * 4, rcap * 4}},
                             "lead ring");
        if (rc) return rc;
        lead_hcap = need;
        lead_slots = slots;
    }
    if (frame_bytes) {
        if (lead_pix_bytes < frame_bytes * slots) VD_CHECK_HIP(hipStreamSynchronize(stream));
        int rc = ensure_staging(&lead_pix, &lead_pix_bytes, frame_bytes * slots);
        if (rc) return rc;
    }
    return VD_OK;
}

int Ctx::lead_step(int mode, const uint8_t* din, uint8_t* dout, int n, int h, int w, size_t pitch, int flush,
                   const int* cnt0, const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1,
                   const Nv12Dev* nvin, const Nv12Dev* nvout) {
    const bool pixels = mode == VD_LEAD_MODE_PIXELS, nv12 = mode == VD_LEAD_MODE_NV12 || mode == VD_LEAD_MODE_YUV16;
    // a ring slot: an RGB frame as pushed, or a packed NV12 surface (pitch w, chroma at h * w): half the bytes,
    // or the same of 16-bit words (pitch 2w, chroma at 2 * h * w): 3 * h * w bytes
    const size_t es = mode == VD_LEAD_MODE_YUV16 ? 2 : 1;
    const size_t fb = pixels ? (size_t)h * pitch : nv12 ? (size_t)h * w / 2 * 3 * es : 0;
    int rc = lead_buffers(std::max(lead_hcap, lead_need(cnt0 ? cap0 : 0, cnt1 ? cap1 : 0)), fb);
    if (rc) return rc;
    const int delay = lead.delay(), pend = lead.pend, m = lead.emit(n, flush), keep = pend + n - m;
    const int K = hold.K;
    const size_t rcap = (size_t)(K + 1) * lead_hcap, mcap = rcap + (size_t)lead.J * lead_hcap;
    const size_t nb = (size_t)std::max(m, 1) * mcap;
    if ((rc = ensure_staging(&lead_rows, &lead_rows_bytes, nb * 16 + nb * 4 + (size_t)std::max(m, 1) * 12 + 64))) return rc;
    LeadArgs a{};
    a.n = n; a.m = m; a.pend = pend; a.keep = keep;
    a.h = h; a.w = w; a.J = lead.J; a.P = hold.P; a.motion = lead.motion;
    if (n > 0) {
        a.cnt0 = cnt0; a.xy0 = xy0; a.cap0 = cnt0 ? cap0 : 0;
        a.cnt1 = cnt1; a.xy1 = xy1; a.cap1 = cnt1 ? cap1 : 0;
        if (K) {   // the hold launch of this call ran over exactly these n frames
            a.dh_xy = hold_last.m_xy; a.dh_age = hold_last.m_age; a.dh_count = hold_last.m_count;
            a.dh_own = hold_last.m_own; a.dh_cap = hold_last.mcap;
        }
    }
    a.ring = lead_ring[lead.cur]; a.next = lead_ring[lead.cur ^ 1];
    a.hcap = lead_hcap; a.rcap = (int)rcap; a.slots = delay;
    a.m_xy = (int*)lead_rows; a.m_age = a.m_xy + nb * 4; a.m_count = a.m_age + nb;
    a.m_own = a.m_count + std::max(m, 1); a.m_dh = a.m_own + std::max(m, 1);
    a.mcap = (int)mcap;
    if (m + keep > 0) {
        t_begin(3, (double)(m + keep) * (K + 1 + lead.J) * 16);
        hipError_t e = vd_launch_lead(a, stream);
        t_end();
        if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "lead: %s", hipGetErrorString(e));
    }
    if (pixels) {
        // the emitted frames: the first min(m, pend) from the ring, the rest from `in`
        const int mr = std::min(m, pend), mi = m - mr;
        if (mr && (rc = launch_cfg_pass((const uint8_t*)lead_pix, dout, mr, h, w, pitch, a.m_count, a.m_xy, a.mcap, nullptr,
                                        nullptr, 0)))
            return rc;
        if (mi && (rc = launch_cfg_pass(din, dout + (size_t)mr * fb, mi, h, w, pitch, a.m_count + mr,
                                        a.m_xy + (size_t)mr * mcap * 4, a.mcap, nullptr, nullptr, 0)))
            return rc;
        // the pixel ring, in stream order behind the passes that read it: the frames that stay
        // move down by the number that left (frame by frame, ascending: source and target of one
        // copy never overlap), then this call's kept frames follow them
        uint8_t* ring = (uint8_t*)lead_pix;
        const int stay = pend - mr;
        t_begin(4, (double)keep * fb * 2);
        if (mr)
            for (int j = 0; j < stay; ++j)
                VD_CHECK_HIP(hipMemcpyAsync(ring + (size_t)j * fb, ring + (size_t)(j + mr) * fb, fb,
                                            hipMemcpyDeviceToDevice, stream));
        if (keep - stay > 0)
            VD_CHECK_HIP(hipMemcpyAsync(ring + (size_t)stay * fb, din + (size_t)mi * fb, (size_t)(keep - stay) * fb,
                                        hipMemcpyDeviceToDevice, stream));
        t_end();
    }
    if (nv12) {
        // the same on surfaces: a ring slot is itself a valid surface for the 4:2:0 passes, whatever
        // layout the call's input and output have; 16-bit words keep the depth and shift they came with
        const Nv12Dev& fmt = n > 0 ? *nvin : *nvout;   // a flush alone emits: out is described
        const Nv12Dev ring = vd_yuv420_packed(lead_pix, h, w, 2, false, fmt.depth, fmt.shift);   // interleaved, U first, stride fb
        const int mr = std::min(m, pend), mi = m - mr;
        const int pass = nv12_cfg_pass();
        if (mr && (rc = launch_nv12_pass(ring, *nvout, mr, h, w, a.m_count, a.m_xy, a.mcap, nullptr, nullptr, 0, pass,
                                         cfg.mosaic_level, cells)))
            return rc;
        if (mi) {
            Nv12Dev o = *nvout;
            o.base += (size_t)mr * o.stride;
            if ((rc = launch_nv12_pass(*nvin, o, mi, h, w, a.m_count + mr, a.m_xy + (size_t)mr * mcap * 4, a.mcap, nullptr,
                                       nullptr, 0, pass, cfg.mosaic_level, cells)))
                return rc;
        }
        // the staying slots move down slot by slot (ascending: one copy's source and target never
        // overlap); then one launch packs this call's kept surfaces behind them (nv12.hip)
        const int stay = pend - mr, push = keep - stay;
        if (mr && stay) {
            t_begin(4, (double)stay * fb * 2);
            for (int j = 0; j < stay; ++j)
                VD_CHECK_HIP(hipMemcpyAsync(ring.base + (size_t)j * fb, ring.base + (size_t)(j + mr) * fb, fb,
                                            hipMemcpyDeviceToDevice, stream));
            t_end();
        }
        if (push > 0) {
            Nv12Dev src = *nvin, dst = ring;      // any layout in, the ring's out
            src.base += (size_t)mi * src.stride;
            dst.base += (size_t)stay * fb;
            t_begin(4, (double)push * fb * 2);
            hipError_t e = vd_launch_yuv420_pack(src, dst, push, h, w, stream);
            t_end();
            if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "nv12 ring push: %s", hipGetErrorString(e));
        }
    }
    lead.end(n, flush, mode, h, w, nv12 ? 0 : pitch, mode == VD_LEAD_MODE_YUV16 ? (n > 0 ? nvin : nvout)->depth : 0,
             mode == VD_LEAD_MODE_YUV16 ? (n > 0 ? nvin : nvout)->shift : 0);
    lead_last = a;
    lead_m = m;
    return VD_OK;
}

int Ctx::lead_read(int n, int which, vd_boxes* out) {
    if (!lead.J) return vd_set_error(VD_ERR_STATE, "look-ahead hold is off (vd_lead)");
    if (which != 0 && which != 1) return vd_set_error(VD_ERR_ARG, "which=%d (expected 0 = led boxes, 1 = blur list)", which);
    if (!out || !out->count || !out->xyxy || out->cap <= 0) return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    if (n <= 0 || n > lead_m)
        return vd_set_error(lead_m ? VD_ERR_ARG : VD_ERR_STATE, "n=%d outside [1, %d frames emitted by the last lead call]",
                            n, lead_m);
    HoldArgs g{};                                 // the hold's gather: rows, labels, counts and the offset to skip
    g.m_xy = lead_last.m_xy; g.m_age = lead_last.m_age; g.m_count = lead_last.m_count;
    g.m_own = lead_last.m_dh; g.mcap = lead_last.mcap;
    return rows_out(g, n, which == 0, out, "lead");
}

// ---- weak-detection rescue (rescue.hip) ----
int Ctx::rescue_set(float face_low, float plate_low, int span) {
    if (!(face_low >= 0.f) || !(plate_low >= 0.f))   // NaN fails both comparisons
        return vd_set_error(VD_ERR_ARG, "vd_rescue: thresholds must be >= 0 (got %g, %g)", (double)face_low, (double)plate_low);
    if (face_low >= cfg.confidence || plate_low >= cfg.plate_conf)
        return vd_set_error(VD_ERR_ARG, "vd_rescue: a low threshold must lie below the net's own (face %g < %g, plate "
                            "%g < %g required)", (double)face_low, (double)cfg.confidence, (double)plate_low,
                            (double)cfg.plate_conf);
    if (span < 1 || span > VD_RESCUE_SPAN_MAX)
        return vd_set_error(VD_ERR_ARG, "vd_rescue: span %d outside [1, %d]", span, VD_RESCUE_SPAN_MAX);
    const bool on = face_low > 0.f || plate_low > 0.f;
    if (!on && !rescue_on()) return VD_OK;
    if (on && face_low == rescue_low[0] && plate_low == rescue_low[1] && span == rescue_span) return VD_OK;
    if (lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_rescue: %d frames are pending in the look-ahead ring (flush first)", lead.pend);
    if (on && tiles_on() && !rescue_tiles)
        return vd_set_error(VD_ERR_STATE, "vd_rescue: rescue and tiled detection (vd_tiles) cannot be combined");
    VD_CHECK_HIP(hipStreamSynchronize(stream));   // a queued launch may still read the history
    rescue_low[0] = face_low; rescue_low[1] = plate_low;
    rescue_span = on ? span : 0;
    rescue_hs.reset();
    hold.reset();
    lead.reset();
    rescue_n = 0;
    return VD_OK;
}

// History buffers of at least `hcap` boxes per slot; the valid slots of a smaller pair are carried over.
int Ctx::rescue_history(int hcap) {
    if (hcap <= rescue_hcap) return VD_OK;
    const int W = rescue_hs.K;
    const size_t oh = (size_t)rescue_hcap, nh = (size_t)hcap;
    int rc = regrow_pair(rescue_hist, 64 + (size_t)W * nh * 20, 64, rescue_hist[0] && rescue_hs.hn > 0 ? rescue_hs.cur : -1,
                         (size_t)W * 4, W, {{oh * 16, nh * 16}, {oh * 4, nh * 4}}, "rescue history");
    if (rc) return rc;
    rescue_hcap = hcap;
    return VD_OK;
}

int Ctx::launch_rescue(int n, int h, int w, RescueArgs a) {
    const int W = rescue_hs.K;
    const size_t strong = (size_t)(a.cnt0 ? a.cap0 : 0) + (a.cnt1 ? a.cap1 : 0);
    const size_t weak = a.split ? (size_t)(a.wcnt ? a.wcap : 0) : strong;
    const size_t ecap = std::max(a.split ? strong + weak : strong, (size_t)1), wtot = std::max(weak, (size_t)1);
    // the loaded nets' complete lists: T * kcap merged rows for a tiled net (vd_rescue_tiles)
    const size_t nets = (size_t)(face.loaded ? face_rows_cap() : 0) + (plate.loaded ? plate_rows_cap() : 0);
    if (std::max(ecap, nets) > 0x3fffffffu) return vd_set_error(VD_ERR_ARG, "rescue: list capacity too large");
    int rc = rescue_history((int)std::max(ecap, nets));
    if (rc) return rc;
    const size_t nb = (size_t)n * ecap;
    if (rescue_rows_bytes < nb * 20 + (size_t)n * 12 + (size_t)n * wtot * 4 + 64)
        VD_CHECK_HIP(hipStreamSynchronize(stream));   // a queued reader may still use the old rows
    if ((rc = ensure_staging(&rescue_rows, &rescue_rows_bytes, nb * 20 + (size_t)n * 12 + (size_t)n * wtot * 4 + 64))) return rc;
    rescue_hs.begin(h, w);
    a.n = n; a.h = h; a.w = w; a.W = W; a.P = hold.P; a.S = rescue_span;
    int* cur = rescue_hist[rescue_hs.cur];
    int* nxt = rescue_hist[rescue_hs.cur ^ 1];
    const size_t hx = (size_t)W * rescue_hcap * 4;
    a.hist_cnt = cur; a.hist_xy = cur + 16; a.hist_since = cur + 16 + hx;
    a.next_cnt = nxt; a.next_xy = nxt + 16; a.next_since = nxt + 16 + hx;
    a.hcap = rescue_hcap; a.hn = rescue_hs.hn;
    a.e_xy = (int*)rescue_rows; a.e_since = a.e_xy + nb * 4; a.e_count = a.e_since + nb; a.e_own = a.e_count + n;
    a.e_nr0 = a.e_own + n; a.w_since = a.e_nr0 + n;
    a.ecap = (int)ecap; a.wtot = (int)wtot;
    t_begin(3, (double)n * (W + 1) * 16);
    hipError_t e = vd_launch_rescue(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "rescue: %s", hipGetErrorString(e));
    rescue_hs.end(n);
    rescue_last = a;
    rescue_n = n;
    return VD_OK;
}

int Ctx::rescue_read_rows(int n, vd_boxes* out) {
    HoldArgs g{};                                 // the hold's gather: rows, labels (since), counts
    g.m_xy = rescue_last.e_xy; g.m_age = rescue_last.e_since; g.m_count = rescue_last.e_count;
    g.m_own = rescue_last.e_own; g.mcap = rescue_last.ecap;
    return rows_out(g, n, 0, out, "rescue");
}

extern "C" {

int vd_hold(vd_ctx* h, const vd_boxes* det, int n, int fh, int fw, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->hold.K) return vd_set_error(VD_ERR_STATE, "vd_hold: context created with hold_frames == 0");
    if (ctx->lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_hold: %d frames are pending in the look-ahead ring (flush first)",
                            ctx->lead.pend);
    if (n <= 0 || fh <= 0 || fw <= 0) return vd_set_error(VD_ERR_ARG, "vd_hold: bad geometry");
    if (out && (!out->count || !out->xyxy || out->cap <= 0))
        return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    BoxListIn d;
    int rc = ctx->box_list_in("vd_hold", det, n, true, 0, &d);
    if (rc) return rc;
    if ((rc = ctx->launch_hold(n, fh, fw, d.cnt, d.xy, det->cap, nullptr, nullptr, 0))) return rc;
    if (out && (rc = ctx->hold_read(n, 0, out))) return rc;
    if (d.staged && !(out && out->where == VD_HOST))
        VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // staging reused by the next call
    return VD_OK;
}

int vd_hold_reset(vd_ctx* h) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    ctx->hold.reset();
    ctx->rescue_hs.reset();
    ctx->lead.reset();                            // the pending frames are dropped unemitted
    return VD_OK;
}

int vd_hold_motion(vd_ctx* h, int mode) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (mode != VD_HOLD_MOTION_OFF && mode != VD_HOLD_MOTION_LINEAR)
        return vd_set_error(VD_ERR_ARG, "vd_hold_motion: mode %d (expected 0 = off or 1 = linear)", mode);
    if (!ctx->hold.K) {
        if (mode) return vd_set_error(VD_ERR_STATE, "vd_hold_motion: context created with hold_frames == 0");
        return VD_OK;
    }
    if (mode != ctx->hold.motion && ctx->lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_hold_motion: %d frames are pending in the look-ahead ring (flush first)",
                            ctx->lead.pend);
    return ctx->hold_set_motion(mode);
}

int vd_read_held(vd_ctx* h, int n, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->hold_read(n, 1, out);
}

int vd_lead(vd_ctx* h, int frames, int motion) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (frames < 0 || frames > VD_LEAD_MAX)
        return vd_set_error(VD_ERR_ARG, "vd_lead: frames %d outside [0, %d]", frames, VD_LEAD_MAX);
    if (motion != VD_HOLD_MOTION_OFF && motion != VD_HOLD_MOTION_LINEAR)
        return vd_set_error(VD_ERR_ARG, "vd_lead: motion %d (expected 0 = off or 1 = linear)", motion);
    if (motion && !frames) return vd_set_error(VD_ERR_ARG, "vd_lead: motion needs frames > 0");
    if (frames == ctx->lead.J && motion == ctx->lead.motion) return VD_OK;
    if (ctx->lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_lead: %d frames are pending (flush first)", ctx->lead.pend);
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // a queued launch may still read the rings
    ctx->lead_free();
    ctx->lead.J = frames;
    ctx->lead.motion = motion;
    ctx->lead.reset();
    ctx->lead_m = 0;
    return VD_OK;
}

int vd_lead_pending(vd_ctx* h, int* frames) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!frames) return vd_set_error(VD_ERR_ARG, "vd_lead_pending: null argument");
    *frames = ctx->lead.pend;
    return VD_OK;
}

int vd_lead_lists(vd_ctx* h, const vd_boxes* det, int n, int fh, int fw, int flush, vd_boxes* out, int* n_out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vd_lead_lists";
    if (!ctx->lead.J) return vd_set_error(VD_ERR_STATE, "%s: look-ahead hold is off (vd_lead)", who);
    if (n > 0 && (!det || !det->count || !det->xyxy || det->cap <= 0))
        return vd_set_error(VD_ERR_ARG, "%s: null argument", who);
    if (out && (!out->count || !out->xyxy || out->cap <= 0))
        return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    if (n == 0 && flush && !ctx->lead.pend) {
        if (n_out) *n_out = 0;
        return VD_OK;
    }
    int rc = ctx->lead_check(who, VD_LEAD_MODE_LISTS, n, fh, fw, 0, flush);
    if (rc) return rc;
    BoxListIn d;                                   // n == 0 (flush alone): no list
    if (n > 0 && (rc = ctx->box_list_in(who, det, n, true, 0, &d))) return rc;
    const int m = ctx->lead.emit(n, flush);
    // the hold step exactly as vd_hold runs it: H_t is final when frame t is pushed
    if (n > 0 && ctx->hold.K && (rc = ctx->launch_hold(n, fh, fw, d.cnt, d.xy, det->cap, nullptr, nullptr, 0))) return rc;
    if ((rc = ctx->lead_step(VD_LEAD_MODE_LISTS, nullptr, nullptr, n, fh, fw, 0, flush, d.cnt, d.xy, n > 0 ? det->cap : 0,
                             nullptr, nullptr, 0)))
        return rc;
    if (out && m > 0 && (rc = ctx->lead_read(m, 1, out))) return rc;
    if (d.staged && !(out && m > 0 && out->where == VD_HOST))
        VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // staging reused by the next call
    if (n_out) *n_out = m;
    return VD_OK;
}

int vd_read_lead(vd_ctx* h, int n, int which, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->lead_read(n, which, out);
}

int vd_rescue(vd_ctx* h, float face_low, float plate_low, int span) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->rescue_set(face_low, plate_low, span);
}

int vd_rescue_lists(vd_ctx* h, const vd_boxes* strong, const vd_boxes* weak, int n, int fh, int fw, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vd_rescue_lists";
    if (!ctx->rescue_on()) return vd_set_error(VD_ERR_STATE, "%s: rescue is off (vd_rescue)", who);
    if (ctx->lead.pend)
        return vd_set_error(VD_ERR_STATE, "%s: %d frames are pending in the look-ahead ring (flush first)", who,
                            ctx->lead.pend);
    if (!strong || !strong->count || !strong->xyxy || strong->cap <= 0 || !weak || !weak->count || !weak->xyxy ||
        weak->cap <= 0)
        return vd_set_error(VD_ERR_ARG, "%s: null argument", who);
    if (n <= 0 || fh <= 0 || fw <= 0) return vd_set_error(VD_ERR_ARG, "%s: bad geometry", who);
    if (out && (!out->count || !out->xyxy || out->cap <= 0))
        return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    // host lists are checked before either is staged; both share the staging, the weak list behind the strong
    int rc;
    for (const vd_boxes* b : {strong, weak})
        if (b->where == VD_HOST && (rc = vd_count_check(who, b->count, n, b->cap))) return rc;
    const size_t off = (size_t)((n + 3) / 4) * 16 + (size_t)n * strong->cap * 16;
    const size_t need = off + (size_t)((n + 3) / 4) * 16 + (size_t)n * weak->cap * 16 + 16;
    BoxListIn s, w;
    if ((rc = ctx->box_list_in(who, strong, n, true, 0, &s, need)) || (rc = ctx->box_list_in(who, weak, n, true, off, &w, need)))
        return rc;
    RescueArgs a{};
    a.split = 1;
    a.cnt0 = s.cnt; a.xy0 = s.xy; a.cap0 = strong->cap;
    a.wcnt = w.cnt; a.wxy = w.xy; a.wcap = weak->cap;
    if ((rc = ctx->launch_rescue(n, fh, fw, a))) return rc;
    if (out && (rc = ctx->rescue_read_rows(n, out))) return rc;
    if ((s.staged || w.staged) && !(out && out->where == VD_HOST))
        VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // staging reused by the next call
    return VD_OK;
}

int vd_read_rescue(vd_ctx* h, int net, int n, int which, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->rescue_on()) return vd_set_error(VD_ERR_STATE, "vd_read_rescue: rescue is off (vd_rescue)");
    if (net != VD_NET_RETINAFACE && net != VD_NET_YOLOV8N) return vd_set_error(VD_ERR_ARG, "unknown net %d", net);
    if (which != 0 && which != 1)
        return vd_set_error(VD_ERR_ARG, "which=%d (expected 0 = rescued boxes, 1 = weak boxes)", which);
    if (!out || !out->count || !out->xyxy || out->cap <= 0) return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    const RescueArgs& r = ctx->rescue_last;
    const bool plate = net == VD_NET_YOLOV8N;
    const PostScratch& ps = plate ? ctx->plate.post : ctx->face.post;
    if (!ps.kcount) return vd_set_error(VD_ERR_STATE, "net %d not loaded", net);
    // a tiled net (vd_rescue_tiles): its lists are the merged rows, cut by the merge (tiles.hip)
    const bool mg = plate ? ctx->plate_rows_merged : ctx->face_rows_merged;
    const TileMergeArgs& tm = plate ? ctx->ptiles_last : ctx->tiles_last;
    const int* kcount = mg ? tm.m_count : ps.kcount;
    const int* kall = mg ? (tm.low_on ? tm.m_all : tm.m_count) : (ctx->rescue_low[plate ? 1 : 0] > 0.f ? ps.kall : ps.kcount);
    // W_t is a property of the net's keep list alone; R_t needs the rescue step of vd_process
    const bool stepped = ctx->rescue_n && !r.split && (plate ? r.cnt1 : r.cnt0) == kcount;
    if (which == 0 && !stepped)
        return vd_set_error(VD_ERR_STATE, "vd_read_rescue: net %d took no part in a rescue step of vd_process yet", net);
    const int frames = which == 0 ? ctx->rescue_n : (mg ? (plate ? ctx->ptiles_kn : ctx->tiles_kn) : ps.kn);
    if (n <= 0 || n > frames) return vd_set_error(VD_ERR_ARG, "n=%d outside [1, %d frames of the last call]", n, frames);
    BoxTargets t{};
    int rc;
    if (out->where == VD_DEVICE) {
        t.count = out->count; t.xyxy = out->xyxy; t.xyxy_f = out->xyxy_f; t.score = out->score; t.label = out->label;
    } else {
        if ((rc = ctx->host_box_staging(&ctx->stage_box, &ctx->stage_box_bytes, out->cap, n, t))) return rc;
        if (!out->xyxy_f) t.xyxy_f = nullptr;
        if (!out->score) t.score = nullptr;
        if (!out->label) t.label = nullptr;
    }
    RescueReadArgs a{};
    a.which = which; a.list = plate ? 1 : 0;
    a.cnt = kcount; a.all = kall; a.kcap = mg ? tm.mcap : ps.kcap;   // low == 0: no weak boxes
    a.xy = mg ? tm.m_xyxy : ps.kxyxy; a.xy_f = mg ? tm.m_xyxy_f : ps.kxyxy_f;
    a.score = mg ? tm.m_score : ps.kscore; a.label = mg ? tm.m_label : ps.klabel;
    if (plate && r.cnt0 && r.all0) { a.cnt_o = r.cnt0; a.all_o = r.all0; a.kcap_o = r.cap0; }
    a.w_since = which == 0 ? r.w_since : ps.kcount; a.wtot = which == 0 ? r.wtot : 0;   // which 1 never reads it
    a.cap = out->cap; a.out_count = t.count; a.out_xyxy = t.xyxy; a.out_xyxy_f = t.xyxy_f; a.out_score = t.score;
    a.out_label = t.label;
    hipError_t e = vd_launch_rescue_read(a, n, ctx->stream);
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "rescue read: %s", hipGetErrorString(e));
    return ctx->box_finish(out, n, t);
}

}  // extern "C"

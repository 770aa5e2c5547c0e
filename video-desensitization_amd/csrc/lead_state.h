// lead_state.h — look-ahead hold (lead.hip): the pending-ring bookkeeping shared by the host
// and the kernel. Plain C++ (no HIP types), so tools/lead_state_check.cpp compiles it alone
// under the host sanitizers.
//
// A lead context emits frame t only once D_{t+delay} is known (delay = J, or J + 1 in motion
// mode, where a candidate of age J looks for its predecessor in the frame of age J + 1), or
// the stream has ended. Between calls it keeps the `pend` <= delay frames pushed and not yet
// emitted: their pixels, their D lists and their merged D ++ H rows. The lists live in one of
// two device buffers ("ping-pong") as `delay` slots, oldest first: slot s holds the frame s
// after the oldest unemitted one. A call pushes n frames, so it sees the window
//   W = ring slots 0 .. pend-1  ++  call frames 0 .. n-1          (pend + n frames)
// emits the first m frames of W, and leaves W[m ..) as the next ring. A launch reads the
// current buffer and writes the other one; the host then flips `cur`. Nothing is updated in
// place, because the emitted frames still read the old slots.
#pragma once

#ifdef __HIPCC__
#define VD_LHD __host__ __device__
#else
#define VD_LHD
#endif

#ifndef VD_LEAD_MAX
#define VD_LEAD_MAX 8   // include/vdmi.h
#endif

// Frames a call emits: everything whose look-ahead is complete, or everything at a stream end.
VD_LHD inline int vd_lead_emit(int pend, int n, int delay, int flush) {
    const int m = flush ? pend + n : pend + n - delay;
    return m > 0 ? m : 0;
}

// Where frame i of the window W lives (i >= 0). Returns 2: ring slot *idx, 1: frame *idx of
// this call, 0: no such frame (past the frames pushed so far; an emitted frame names one only
// at a stream end).
VD_LHD inline int vd_lead_source(int i, int pend, int n, int* idx) {
    if (i < pend) { *idx = i; return 2; }
    if (i - pend < n) { *idx = i - pend; return 1; }
    *idx = 0;
    return 0;
}

#define VD_LEAD_MODE_NONE 0     // nothing pending
#define VD_LEAD_MODE_PIXELS 1   // pending frames were pushed by vd_process_lead
#define VD_LEAD_MODE_LISTS 2    // pending lists were pushed by vd_lead_lists
#define VD_LEAD_MODE_NV12 3     // pending 8-bit surfaces (a packed NV12 ring) were pushed by vd_process_lead_nv12 / vd_process_lead_yuv420
#define VD_LEAD_MODE_YUV16 4    // pending surfaces of 16-bit words were pushed by vd_process_lead_yuv420_16

// One stream is pushed by one entry point: a call of mode `call_mode` joins the pending frames
// only when nothing is pending or they were pushed in the same mode (otherwise: flush first).
VD_LHD inline int vd_lead_mode_ok(int pend, int pending_mode, int call_mode) {
    return pend == 0 || pending_mode == call_mode;
}

// The entry point that pushes frames of `mode` (for the refusal's message).
inline const char* vd_lead_mode_caller(int mode) {
    return mode == VD_LEAD_MODE_PIXELS ? "vd_process_lead"
           : mode == VD_LEAD_MODE_LISTS ? "vd_lead_lists"
           : mode == VD_LEAD_MODE_NV12 ? "vd_process_lead_nv12 / vd_process_lead_yuv420"
           : mode == VD_LEAD_MODE_YUV16 ? "vd_process_lead_yuv420_16" : "nothing";
}

struct LeadState {
    int J = 0;          // vd_lead frames (0: off)
    int motion = 0;     // vd_lead motion mode
    int pend = 0;       // pending frames (<= delay)
    int cur = 0;        // the list buffer the next launch reads
    int mode = VD_LEAD_MODE_NONE;
    int h = 0, w = 0;   // geometry of the pending frames
    unsigned long long pitch = 0;
    int depth = 0, shift = 0;   // of pending 16-bit surfaces (VD_LEAD_MODE_YUV16), else 0

    int delay() const { return J + (motion ? 1 : 0); }
    int emit(int n, int flush) const { return vd_lead_emit(pend, n, delay(), flush); }
    void reset() { pend = 0; mode = VD_LEAD_MODE_NONE; h = w = 0; pitch = 0; depth = shift = 0; }
    // may a call of 16-bit surfaces (depth, shift) join the pending ones: the words stay as pushed
    bool format_ok(int call_mode, int d, int s) const {
        return pend == 0 || call_mode != VD_LEAD_MODE_YUV16 || (d == depth && s == shift);
    }
    // after a launch over n pushed frames wrote the other buffer
    void end(int n, int flush, int call_mode, int fh, int fw, unsigned long long fpitch, int fdepth = 0, int fshift = 0) {
        pend = pend + n - emit(n, flush);
        cur ^= 1;
        if (pend == 0) { reset(); return; }
        mode = call_mode; h = fh; w = fw; pitch = fpitch; depth = fdepth; shift = fshift;
    }
};

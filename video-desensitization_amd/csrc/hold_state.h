// hold_state.h — box hold (hold.hip): the history bookkeeping shared by the host and the
// kernel. Plain C++ (no HIP types), so tools/hold_state_check.cpp compiles it alone under
// the host sanitizers.
//
// A hold context keeps the box lists D of the last `depth` frames it has seen: K frames, or
// K + 1 in motion mode (vd_hold_motion), where a candidate of age K looks for its predecessor
// in the frame of age K + 1. They live in one of two device buffers ("ping-pong") as `depth`
// slots: slot s holds the frame s + 1 before the NEXT call's frame 0, and `hn` slots are
// valid. A launch over n frames reads the current buffer and writes the other one; the host
// then flips `cur`. Nothing is updated in place, because the first `depth` frames of the
// launch still read the old slots.
#pragma once

#ifdef __HIPCC__
#define VD_HD __host__ __device__
#else
#define VD_HD
#endif

#ifndef VD_HOLD_MAX
#define VD_HOLD_MAX 8   // include/vdmi.h
#endif

// Where the list of the frame `age` frames before frame f of a call lives (age >= 0,
// f in [0, n]; f == n is the virtual frame after the call, whose ages 1..depth are the next
// history). Returns 1: frame f - age of this call (*idx), 2: history slot *idx, 0: no such
// frame (before the stream's start / the last reset).
VD_HD inline int vd_hold_source(int f, int age, int hn, int* idx) {
    if (f - age >= 0) { *idx = f - age; return 1; }
    const int s = age - f - 1;
    if (s < hn) { *idx = s; return 2; }
    *idx = 0;
    return 0;
}

struct HoldState {
    int K = 0;          // cfg.hold_frames (0: off)
    int P = 30;         // cfg.hold_iou_pct
    int motion = 0;     // vd_hold_motion mode (0: held boxes stay where they were last seen)
    int hn = 0;         // valid history slots
    int cur = 0;        // the buffer the next launch reads
    int h = 0, w = 0;   // frame size of the previous call (0: none)

    int depth() const { return K + (motion ? 1 : 0); }   // history slots
    void reset() { hn = 0; h = w = 0; }
    // before a launch: a call with another frame size starts from an empty history
    void begin(int fh, int fw) {
        if (fh != h || fw != w) hn = 0;
        h = fh; w = fw;
    }
    // after a launch over n frames wrote the other buffer: history = last depth of (old ++ call)
    void end(int n) {
        const int d = depth();
        hn = hn + n < d ? hn + n : d;
        cur ^= 1;
    }
};

// lead_state_check.cpp — host check of the look-ahead hold's pending-ring bookkeeping
// (csrc/lead_state.h): the emission arithmetic and the window-to-slot mapping the kernel and
// the runtime share, run over host arrays that stand for the two device buffers, against a
// plain deque of the frames pushed and not yet emitted; and the rule that one stream is pushed
// by one entry point family (RGB frames, lists, 8-bit surfaces or surfaces of 16-bit words, whose
// depth and shift belong to the pending geometry). Stand-alone, no HIP:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/lead_state_check.cpp -o lead_state_check && ./lead_state_check
//
// Every read and write below goes through exact-size vectors, so an out-of-range slot or
// frame index is an AddressSanitizer error, and a wrong one fails the comparison.
#include "../video-desensitization_amd/csrc/lead_state.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

static unsigned rng_state = 2468u;
static unsigned rnd(unsigned m) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % m;
}

static int fail(const char* what, int delay, int step) {
    std::fprintf(stderr, "FAIL: %s (delay=%d, step %d)\n", what, delay, step);
    return 1;
}

// One stream of calls at this delay: every call size 0..12 in turn (size 0 only as a flush),
// then random sizes, flushes and resets.
static int run(int J, int motion, long* checks) {
    LeadState st;
    st.J = J;
    st.motion = motion;
    const int D = st.delay();
    if (D != J + motion) return fail("delay", D, 0);
    std::vector<int> buf[2] = {std::vector<int>(D, -1), std::vector<int>(D, -1)};   // slot -> frame id
    std::deque<int> model;                                                         // oldest first
    int next_id = 0, emitted = 0;                                                  // frames leave in order
    static const int MODES[4] = {VD_LEAD_MODE_PIXELS, VD_LEAD_MODE_LISTS, VD_LEAD_MODE_NV12, VD_LEAD_MODE_YUV16};
    int depth = 0, shift = 0;                                                      // of a stream of 16-bit words
    int mode = MODES[0];                                                           // the entry point pushing this stream
    for (int step = 0; step < 600; ++step) {
        int n = step < 13 ? step : (int)rnd(13);
        int flush = rnd(8) == 0;
        if (n == 0) flush = 1;                                // n == 0 is allowed only with flush
        if (rnd(32) == 0) {                                   // vd_hold_reset: pending frames dropped unemitted
            emitted += (int)model.size();
            st.reset();
            model.clear();
        }
        if (st.pend != (int)model.size()) return fail("pending count", D, step);
        if (st.pend > D) return fail("pending above delay", D, step);
        // a new stream may come through any entry point; a pending one takes its own alone
        if (st.pend == 0) {
            mode = MODES[rnd(4)];
            depth = mode == VD_LEAD_MODE_YUV16 ? (rnd(2) ? 10 : 12) : 0;
            shift = depth ? (int)rnd(17 - depth) : 0;
        }
        // words stay as pushed: a 16-bit call joins pending surfaces of its own depth and shift only
        for (int d : {10, 12})
            for (int s = 0; s <= 16 - d; ++s) {
                const bool want = st.pend == 0 || (d == depth && s == shift);
                if (st.format_ok(VD_LEAD_MODE_YUV16, d, s) != want) return fail("depth / shift rule", D, step);
                if (!st.format_ok(VD_LEAD_MODE_NV12, d, s)) return fail("depth / shift rule off 16-bit", D, step);
                ++*checks;
            }
        for (int cm : MODES) {
            const int want_ok = st.pend == 0 || cm == mode;
            if (vd_lead_mode_ok(st.pend, st.mode, cm) != want_ok) return fail("mode mismatch rule", D, step);
            ++*checks;
        }
        std::vector<int> call(n);
        for (int f = 0; f < n; ++f) call[f] = next_id++;
        const int m = st.emit(n, flush);
        const int total = st.pend + n;
        const int want_m = flush ? total : (total - D > 0 ? total - D : 0);
        if (m != want_m || m != vd_lead_emit(st.pend, n, D, flush)) return fail("emitted count", D, step);
        const std::vector<int>& cur = buf[st.cur];
        std::vector<int>& nxt = buf[st.cur ^ 1];
        std::vector<int> win(model.begin(), model.end());     // the window W: pending, then the call
        win.insert(win.end(), call.begin(), call.end());
        auto frame = [&](int i, int* got) -> int {
            int idx = -1;
            const int kind = vd_lead_source(i, st.pend, n, &idx);
            *got = kind == 1 ? call.at(idx) : (kind == 2 ? cur.at(idx) : -1);
            return kind;
        };
        // emitted-frame workgroups: frame e and the frames of ages 1 .. D after it
        for (int e = 0; e < m; ++e) {
            if (win.at(e) != emitted + e) return fail("emission order", D, step);
            for (int age = 0; age <= D; ++age) {
                int got = -1;
                const int kind = frame(e + age, &got);
                const int want = e + age < total ? win[e + age] : -1;
                if (got != want) return fail("frame source", D, step);
                if (!flush && kind == 0) return fail("look-ahead incomplete without a stream end", D, step);
                ++*checks;
            }
        }
        // ring workgroups: slot j of the other buffer <- frame m + j of the window
        const int keep = total - m;
        if (keep > D) return fail("ring overflow", D, step);
        for (int j = 0; j < keep; ++j) {
            int got = -1;
            if (!frame(m + j, &got)) return fail("ring source", D, step);
            nxt.at(j) = got;
        }
        emitted += m;
        model.assign(win.begin() + m, win.end());
        // the ring of NV12 surfaces is the library's own, packed: no pitch to remember
        const unsigned long long pitch = mode == VD_LEAD_MODE_PIXELS ? 300 : 0;
        st.end(n, flush, mode, 100, 100, pitch, depth, shift);
        if (st.pend != (int)model.size()) return fail("pending after the call", D, step);
        if (st.mode != (st.pend ? mode : VD_LEAD_MODE_NONE)) return fail("mode", D, step);
        if (st.pitch != (st.pend ? pitch : 0) || st.h != (st.pend ? 100 : 0)) return fail("pending geometry", D, step);
        if (st.depth != (st.pend ? depth : 0) || st.shift != (st.pend ? shift : 0)) return fail("pending depth / shift", D, step);
        for (int j = 0; j < st.pend; ++j)
            if (buf[st.cur].at(j) != model[j]) return fail("shifted ring", D, step);
    }
    return 0;
}

int main() {
    long checks = 0;
    if (std::strcmp(vd_lead_mode_caller(VD_LEAD_MODE_PIXELS), "vd_process_lead") ||
        std::strcmp(vd_lead_mode_caller(VD_LEAD_MODE_LISTS), "vd_lead_lists") ||
        std::strncmp(vd_lead_mode_caller(VD_LEAD_MODE_NV12), "vd_process_lead_nv12", 20) ||
        !std::strstr(vd_lead_mode_caller(VD_LEAD_MODE_NV12), "vd_process_lead_yuv420") ||
        std::strcmp(vd_lead_mode_caller(VD_LEAD_MODE_YUV16), "vd_process_lead_yuv420_16"))
        return fail("mode caller names", 0, 0);
    for (int motion = 0; motion <= 1; ++motion)
        for (int J = 1; J <= VD_LEAD_MAX; ++J)                // delays 1 .. 9
            if (run(J, motion, &checks)) return 1;
    std::printf("lead_state_check: ok (%ld source checks)\n", checks);
    return 0;
}

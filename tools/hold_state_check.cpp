// hold_state_check.cpp — host check of the box-hold history bookkeeping (csrc/hold_state.h):
// the slot arithmetic the kernel and the runtime share, run over host arrays that stand for
// the two device buffers, against a plain deque of the last `depth` frames (K, or K + 1 in
// motion mode, whose predecessor search reads the frame of age K + 1). Stand-alone, no HIP:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/hold_state_check.cpp -o hold_state_check && ./hold_state_check
//
// Every read and write below goes through exact-size vectors, so an out-of-range slot or
// frame index is an AddressSanitizer error, and a wrong one fails the comparison.
#include "../video-desensitization_amd/csrc/hold_state.h"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

static unsigned rng_state = 12345u;
static unsigned rnd(unsigned m) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % m;
}

static int g_motion = 0;
static int fail(const char* what, int K, int step) {
    std::fprintf(stderr, "FAIL: %s (K=%d, motion=%d, step %d)\n", what, K, g_motion, step);
    return 1;
}

int main() {
    long checks = 0;
    for (int motion = 0; motion <= 1; ++motion)
    for (int K = 1; K <= VD_HOLD_MAX; ++K) {
        g_motion = motion;
        HoldState st;
        st.K = K;
        st.motion = motion;
        const int D = st.depth();
        if (D != K + motion) return fail("depth", K, 0);
        std::vector<int> buf[2] = {std::vector<int>(D, -1), std::vector<int>(D, -1)};   // slot -> frame id
        std::deque<int> model;                                                         // newest first
        int next_id = 0, h = 100, w = 100;
        for (int step = 0; step < 400; ++step) {
            const unsigned ev = rnd(16);
            if (ev == 0) { st.reset(); model.clear(); }
            if (ev == 1) { h = 100 + (int)rnd(3); w = 100 + (int)rnd(3); }
            const int n = 1 + (int)rnd(2 * K + 3);                // calls shorter and longer than the depth
            const int oh = st.h, ow = st.w;
            st.begin(h, w);
            if (oh != h || ow != w) model.clear();
            if (st.hn != (int)model.size()) return fail("valid slots", K, step);
            std::vector<int> call(n);
            for (int f = 0; f < n; ++f) call[f] = next_id++;
            const std::vector<int>& cur = buf[st.cur];
            std::vector<int>& nxt = buf[st.cur ^ 1];
            // frame workgroups: the frame `age` before frame f (age D: an age-K candidate's predecessor)
            for (int f = 0; f < n; ++f)
                for (int age = 0; age <= D; ++age) {
                    int idx = -1;
                    const int kind = vd_hold_source(f, age, st.hn, &idx);
                    int got = -1;
                    if (kind == 1) got = call.at(idx);
                    else if (kind == 2) got = cur.at(idx);
                    int want = -1;                                 // model: call frames, then the deque
                    if (f - age >= 0) want = call[f - age];
                    else if (age - f - 1 < (int)model.size()) want = model[age - f - 1];
                    if (got != want) return fail("frame source", K, step);
                    ++checks;
                }
            // history workgroups: slot j of the other buffer <- the frame j + 1 before frame n
            for (int j = 0; j < D; ++j) {
                int idx = -1;
                const int kind = vd_hold_source(n, j + 1, st.hn, &idx);
                nxt.at(j) = kind == 1 ? call.at(idx) : (kind == 2 ? cur.at(idx) : -1);
            }
            for (int f = 0; f < n; ++f) {
                model.push_front(call[f]);
                if ((int)model.size() > D) model.pop_back();
            }
            st.end(n);
            if (st.hn != (int)model.size()) return fail("valid slots after the call", K, step);
            for (int j = 0; j < st.hn; ++j)
                if (buf[st.cur].at(j) != model[j]) return fail("shifted history", K, step);
        }
    }
    std::printf("hold_state_check: ok (%ld source checks)\n", checks);
    return 0;
}

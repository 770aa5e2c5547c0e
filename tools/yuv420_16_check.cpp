// yuv420_16_check.cpp — host check of the vd_yuv420_16 descriptor rules and of the conversion of 10- and
// 12-bit 4:2:0 frames (csrc/nv12.h: the routines behind vd_yuv420_16_to_rgb) on padded, odd-word-pitch
// and swapped layouts. Stand-alone, no HIP:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/yuv420_16_check.cpp -o yuv420_16_check && ./yuv420_16_check
//
// Every surface below is an exact-size vector -- the last word of the last plane row is the buffer's
// last word -- so a read past what the descriptor names is an AddressSanitizer error, and every
// arithmetic step runs under UBSan. The pixels are checked against vd_yuv420_to_rgb_host on D(S), the
// 8-bit surface of the same layout (pitches counted in samples) whose samples are v >> (depth - 8),
// which tools/yuv420_check.cpp pins against the NV12 routine.
#include "../video-desensitization_amd/csrc/nv12.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static unsigned rng_state = 2463534242u;
static unsigned rnd(unsigned m) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % m;
}

static int fail(const char* what, int a, int b) {
    std::fprintf(stderr, "FAIL: %s (%d, %d)\n", what, a, b);
    return 1;
}

int main() {
    // 1. descriptor rules: each rule's boundary accepted on one side, refused on the other (h = 4, w = 6:
    //    the luma plane is bytes [0, 60) at pitch 16, a planar chroma plane 2 rows of 6 bytes)
    {
        alignas(2) static uint8_t bytes[4] = {0, 0, 0, 0};
        struct { int n, h, w; size_t pitch, u, v, cp, stride; int step, matrix, range, depth, shift, want; } cases[] = {
            {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0, 0},  {2, 4, 6, 16, 80, 64, 8, 96, 1, 1, 0, 12, 4, 0},   // planar, V first
            {2, 4, 6, 16, 64, 66, 16, 96, 2, 1, 0, 10, 6, 0}, {2, 4, 6, 16, 66, 64, 16, 96, 2, 0, 1, 12, 0, 0},  // P010, V first
            {2, 4, 6, 16, 60, 74, 8, 88, 1, 1, 0, 10, 3, 0},  {1, 4, 6, 16, 64, 80, 8, 0, 1, 1, 0, 10, 0, 0},    // tight; one frame
            {2, 4, 6, 12, 48, 60, 6, 72, 1, 1, 0, 10, 0, 0},  {1, 2, 2, 4, 8, 10, 2, 12, 1, 0, 0, 12, 4, 0},     // packed; smallest
            {2, 3, 6, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0, 2},  {2, 4, 5, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0, 2},
            {0, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0, 2},
            {2, 4, 6, 10, 64, 80, 8, 96, 1, 1, 0, 10, 0, 3},  {2, 4, 6, 17, 64, 80, 8, 96, 1, 1, 0, 10, 0, 3},   // < 2w; odd
            {2, 4, 6, 16, 64, 80, 8, 96, 0, 1, 0, 10, 0, 4},  {2, 4, 6, 16, 64, 80, 8, 96, 3, 1, 0, 10, 0, 4},
            {2, 4, 6, 16, 64, 80, 4, 96, 1, 1, 0, 10, 0, 5},  {2, 4, 6, 16, 64, 80, 9, 128, 1, 1, 0, 10, 0, 5},
            {2, 4, 6, 16, 64, 66, 10, 96, 2, 1, 0, 10, 6, 5},
            {2, 4, 6, 16, 64, 65, 16, 96, 2, 1, 0, 10, 6, 6}, {2, 4, 6, 16, 64, 68, 16, 96, 2, 1, 0, 10, 6, 6},
            {2, 4, 6, 16, 64, 64, 16, 96, 2, 1, 0, 10, 6, 6},
            {2, 4, 6, 16, 58, 80, 8, 96, 1, 1, 0, 10, 0, 7},  {2, 4, 6, 16, 65, 81, 8, 128, 1, 1, 0, 10, 0, 7},
            {2, 4, 6, 16, 58, 60, 16, 96, 2, 1, 0, 10, 6, 7},
            {2, 4, 6, 16, 80, 58, 8, 128, 1, 1, 0, 10, 0, 8}, {2, 4, 6, 16, 64, 76, 8, 96, 1, 1, 0, 10, 0, 8},
            {2, 4, 6, 16, 64, 81, 8, 128, 1, 1, 0, 10, 0, 8}, {2, 4, 6, 16, 60, 58, 16, 96, 2, 1, 0, 10, 6, 8},
            {2, 4, 6, 16, 64, 80, 8, 92, 1, 1, 0, 10, 0, 9},  {2, 4, 6, 16, 64, 80, 8, 94, 1, 1, 0, 10, 0, 0},
            {2, 4, 6, 16, 64, 80, 8, 97, 1, 1, 0, 10, 0, 9},
            {2, 4, 6, 16, 64, 80, 8, 96, 1, 2, 0, 10, 0, 10}, {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, -1, 10, 0, 11},
            {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 8, 0, 12},  {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 16, 0, 12},
            {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 11, 0, 12},
            {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 10, 7, 13}, {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 12, 5, 13},
            {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 10, -1, 13}, {2, 4, 6, 16, 64, 80, 8, 96, 1, 1, 0, 10, 6, 0},
            {2, 4, 6, (size_t)1 << 31, (size_t)4 << 31, (size_t)5 << 31, 8, (size_t)6 << 31, 1, 1, 0, 10, 0, 3},
            {2, 4, 6, 16, (size_t)1 << 47, 80, 8, 96, 1, 1, 0, 10, 0, 7}, {2, 4, 6, 16, 64, 80, 8, (size_t)1 << 47, 1, 1, 0, 10, 0, 9},
        };
        int i = 0;
        for (const auto& c : cases) {
            vd_yuv420_16 d{bytes, c.pitch, c.u, c.v, c.cp, c.stride, c.step, c.matrix, c.range, c.depth, c.shift};
            if (vd_yuv420_16_layout(&d, c.n, c.h, c.w, true) != c.want) return fail("layout rule", i, c.want);
            ++i;
        }
        vd_yuv420_16 odd_base{bytes + 1, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0};
        if (vd_yuv420_16_layout(&odd_base, 2, 4, 6, true) != 14) return fail("odd base", 0, 14);
        vd_yuv420_16 out_desc{bytes, 16, 64, 80, 8, 96, 1, 77, -3, 10, 0};   // an output descriptor: matrix and range ignored
        if (vd_yuv420_16_layout(&out_desc, 2, 4, 6, false) != 0) return fail("output descriptor", 0, 0);
        vd_yuv420_16 null_base{nullptr, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0};
        if (vd_yuv420_16_layout(nullptr, 2, 4, 6, true) != 1 || vd_yuv420_16_layout(&null_base, 2, 4, 6, true) != 1)
            return fail("null descriptor", 0, 0);
        size_t end = 0;
        vd_yuv420_16 g{bytes, 16, 64, 80, 8, 96, 1, 1, 0, 10, 0};
        if (vd_yuv420_16_layout(&g, 2, 4, 6, true, &end) != 0 || end != 94) return fail("frame end", (int)end, 94);
    }

    // 2. whole frames on edge layouts, each in an exact-size buffer of words: planar and interleaved, U
    //    and V in either order, odd word pitches, a padded luma height, a padded frame stride; depth 10
    //    and 12 at every shift the depth allows, noise in the unused bits. Sizes in words until the descriptor.
    struct { int n, h, w; size_t pitch, cpitch, pad_rows, pad_stride; int step; bool v_first; } lay[] = {
        {1, 2, 2, 2, 1, 0, 0, 1, false},     {1, 2, 2, 2, 2, 0, 0, 2, true},      {2, 6, 10, 10, 5, 0, 0, 1, false},
        {2, 6, 10, 13, 8, 0, 0, 1, true},    {3, 6, 10, 16, 13, 2, 7, 2, true},   {2, 48, 64, 70, 35, 8, 5, 1, true},
        {2, 48, 64, 64, 67, 0, 3, 2, false}, {1, 270, 480, 480, 243, 8, 0, 1, true},
    };
    int li = 0;
    for (const auto& L : lay) {
        const size_t c0 = (size_t)(L.h + L.pad_rows) * L.pitch, crows = (size_t)(L.h / 2);
        const size_t crow = (size_t)(L.w / 2) * L.step, plane = crows * L.cpitch;
        size_t u, v, last_end;
        if (L.step == 2) {
            u = c0 + (L.v_first ? 1 : 0); v = c0 + (L.v_first ? 0 : 1);
            last_end = c0 + (crows - 1) * L.cpitch + crow;
        } else {
            u = c0 + (L.v_first ? plane : 0); v = c0 + (L.v_first ? 0 : plane);
            last_end = c0 + plane + (crows - 1) * L.cpitch + crow;
        }
        const size_t stride = std::max(last_end, c0 + (L.step == 2 ? plane : 2 * plane)) + L.pad_stride;
        std::vector<uint16_t> buf((size_t)(L.n - 1) * stride + last_end);    // nothing behind the last plane row
        for (int depth = 10; depth <= 12; depth += 2)
            for (int shift = 0; shift <= 16 - depth; shift += (16 - depth) / 2) {
                for (auto& b : buf) b = (uint16_t)rnd(65536);
                // D(S): the same layout in bytes, pitches counted in samples
                std::vector<uint8_t> d8(buf.size());
                for (size_t k = 0; k < buf.size(); ++k)
                    d8[k] = (uint8_t)(((buf[k] >> shift) & ((1u << depth) - 1u)) >> (depth - 8));
                const int m = (li + shift) & 1, r = (li >> 1) & 1;
                vd_yuv420_16 d{(uint8_t*)buf.data(), 2 * L.pitch, 2 * u, 2 * v, 2 * L.cpitch, 2 * stride, L.step, m, r, depth, shift};
                vd_yuv420 e{d8.data(), L.pitch, u, v, L.cpitch, stride, L.step, m, r};
                if (vd_yuv420_16_layout(&d, L.n, L.h, L.w, true) != 0) return fail("edge layout refused", li, shift);
                if (vd_yuv420_layout(&e, L.n, L.h, L.w, true) != 0) return fail("D(S) refused", li, shift);
                const size_t rp = (size_t)L.w * 3 + (li & 1);       // an rgb pitch with and without padding
                const size_t rb = (size_t)(L.n * L.h - 1) * rp + (size_t)L.w * 3;
                std::vector<uint8_t> got(rb, 0xEE), want(rb, 0xEE);
                vd_yuv420_16_to_rgb_host(&d, L.n, L.h, L.w, got.data(), rp);
                vd_yuv420_to_rgb_host(&e, L.n, L.h, L.w, want.data(), rp);
                if (got != want) return fail("frame pixels", li, depth * 100 + shift);   // the rgb pad bytes stay 0xEE in both
            }
        ++li;
    }
    std::printf("yuv420_16_check ok\n");
    return 0;
}

// conv_x6.h — what conv_x6.hip, conv_x6_halo.hip and conv_x6_stream.hip (only they include
// it, after vd_kernel.h) share: tile shape, wait counts, operand splits and products, the
// two tile epilogues, and the entry points the dispatch calls across the files.
#pragma once

namespace {

constexpr int KT = 32;                          // K per tile (one bf16 MFMA k-step)
constexpr int kAmaxFrames = 1024;               // LDS reserved for per-frame max slots (frames per launch)

// Two forms: the big tile (256 x BN, 8 waves, two LDS stages, one workgroup per CU)
// for the compute-heavy layers, and the small tile (128 x BN, 4 waves, ONE stage,
// three workgroups per CU) for small-K / small-M layers, where a workgroup's
// load -> compute -> epilogue phases are short and neighbours on the CU overlap them.
// TERMS: 3 = bf16 triples (A and B), 2 = fp16 pairs (A and B), 1 = fp16 pair weights
// with activations exact in fp16 (one A plane: the integer-valued face canvas)
template <int BM_, int BN, int NT_, int NST, int TERMS, int MF = 16> struct X6Shape {
    static constexpr int TA = TERMS == 1 ? 1 : TERMS, TB = TERMS == 1 ? 2 : TERMS;   // A / B planes
    static constexpr int BM = BM_, BNV = BN, NT = NT_, WAVES = NT / 64, TERMSV = TERMS;
    static constexpr int PL_A = BM * 64;                       // bytes per A plane
    static constexpr int PL_B = BN * 64;                       // bytes per B plane
    static constexpr int STAGE = TA * PL_A + TB * PL_B;        // 256 x 128: 73 728 B (3 terms), 49 152 B (2)
    static constexpr int EPR = NST == 2 ? 128 : 64;            // epilogue rows per pass
    static constexpr int EPLD = BN + 4;                        // f32 epilogue row stride
    static constexpr int LDS = NST * STAGE > EPR * EPLD * 4 ? NST * STAGE : EPR * EPLD * 4;
    static constexpr int WAVES_N = BN >= 64 ? 2 : 1;
    static constexpr int WAVES_M = WAVES / WAVES_N;
    static constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    static constexpr int TM = WTM / MF, TN = WTN / MF;            // MFMA blocks per wave tile
    static constexpr int NDMA = TB * BN / 16;                  // 1-KB DMA instructions per K tile
    static constexpr int AROWS = NT / 4;                       // A rows per staging pass
    static constexpr int AITEMS = BM / AROWS;                  // A items (row, 8 k) per thread: 2 (8 waves), 4 (4 waves)
    static_assert(BM % AROWS == 0 && (AITEMS == 2 || AITEMS == 4), "A items per thread");
};

// s_waitcnt vmcnt(n) for n in [0, 23] (immediate operand)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); return;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); return;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); return;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); return;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); return;
        case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); return;
        case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); return;
        case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); return;
        case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); return;
        case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); return;
        case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); return;
        case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); return;
        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); return;
        case 21: asm volatile("s_waitcnt vmcnt(21)" ::: "memory"); return;
        case 22: asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); return;
        case 23: asm volatile("s_waitcnt vmcnt(23)" ::: "memory"); return;
        default: break;
    }
    switch (n < 8 ? n : 7) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    }
}

// s_waitcnt vmcnt(N) for a compile-time N (no branch tree)
template <int N>
__device__ __forceinline__ void wait_vm_k() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// x = hi + mid + lo exactly (truncation split: each term keeps 8 significand bits)
__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned u = __float_as_uint(x);
    const float x0 = __uint_as_float(u & 0xFFFF0000u);
    const float r1 = x - x0;                       // exact
    const unsigned v = __float_as_uint(r1);
    const float x1 = __uint_as_float(v & 0xFFFF0000u);
    const float r2 = r1 - x1;                      // exact, <= 8 significand bits
    h = u >> 16;
    m = v >> 16;
    l = __float_as_uint(r2) >> 16;
}

// The products of one 16x16x32 block on TERMS planes, small terms first: 3 = the six
// bf16 cross terms, 2 = the fp16 pair (vd_kernel.h), 1 = pair weights on one exact A plane
template <int TERMS>
__device__ __forceinline__ f32x4_t mfma_terms(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4_t acc) {
    if constexpr (TERMS == 2) {
        return mfma_pair(a, b, acc);
    } else if constexpr (TERMS == 1) {
        acc = Half16<true>::mfma(a[0], b[1], acc);
        return Half16<true>::mfma(a[0], b[0], acc);
    } else {
        acc = Half16<false>::mfma(a[2], b[0], acc);
        acc = Half16<false>::mfma(a[1], b[1], acc);
        acc = Half16<false>::mfma(a[0], b[2], acc);
        acc = Half16<false>::mfma(a[1], b[0], acc);
        acc = Half16<false>::mfma(a[0], b[1], acc);
        return Half16<false>::mfma(a[0], b[0], acc);
    }
}

typedef float f32x16_t __attribute__((ext_vector_type(16)));

// fp16 pair on the 32x32x16 matrix-core form: the same three products per K step of
// 16, half the MFMA instructions of the 16x16x32 form for the same work, and 24 of
// every 32 issue cycles free for the A split / address VALU (16x16x32: 8 of 16)
__device__ __forceinline__ f32x16_t mfma_pair32(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x16_t acc) {
#define VDH_MFMA32(pa, pb)                                                                               \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a[pa]),                    \
                                                 __builtin_bit_cast(f16x8_t, b[pb]), acc, 0, 0, 0)
    VDH_MFMA32(1, 0);
    VDH_MFMA32(0, 1);
    VDH_MFMA32(0, 0);
#undef VDH_MFMA32
    return acc;
}

// 8 f32 -> TERMS packed 16-B planes (bf16 truncation split, or scaled fp16 pair)
template <int TERMS>
__device__ __forceinline__ void split_pack(const float (&e)[8], float sa, u32x4 (&o)[3]) {
    if constexpr (TERMS == 2) {
        split_pair8(e, sa, o[0], o[1]);
        return;
    }
    unsigned hv[8], mv[8], lv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if constexpr (TERMS == 3) split3(e[j], hv[j], mv[j], lv[j]);
        else { hv[j] = __builtin_bit_cast(unsigned short, pair_hi(e[j], sa)); mv[j] = lv[j] = 0; }
    }
    o[0] = u32x4{hv[0] | (hv[1] << 16), hv[2] | (hv[3] << 16), hv[4] | (hv[5] << 16), hv[6] | (hv[7] << 16)};
    if constexpr (TERMS >= 2)
        o[1] = u32x4{mv[0] | (mv[1] << 16), mv[2] | (mv[3] << 16), mv[4] | (mv[5] << 16), mv[6] | (mv[7] << 16)};
    if constexpr (TERMS == 3)
        o[2] = u32x4{lv[0] | (lv[1] << 16), lv[2] | (lv[3] << 16), lv[4] | (lv[5] << 16), lv[6] | (lv[7] << 16)};
}

// The fused epilogue of the 256 / 128-row tiles: BM / EPR passes of EPR accumulator
// rows through LDS, then BN + residual (incl. the FPN nearest-2x source) +
// activation + 16-B stores + the per-frame max |y| into the output's slots.
template <class S, int MF, class AccT>
__device__ __forceinline__ void x6_epilogue(const ConvArgs& a, AccT (&acc)[S::TM][S::TN], int m0, int n0, int wm,
                                            int wn, int tid, int lane, char* smem, int amax_off) {
    constexpr int BM = S::BM, BN = S::BNV, NT = S::NT, TM = S::TM, TN = S::TN, TERMS = S::TERMSV;
    const int ohw = a.yh * a.yw;
    if (a.dbg & 1) {                                   // timing-only (x6_dbg bit 0): main loop only
        if (acc[0][0][0] == 1234.5f) ((float*)a.y)[tid] = 1.f;
        return;
    }
    // ---- fused epilogue: BM / EPR passes of EPR rows through LDS ([EPR][BN+4] f32)
    constexpr int EPLD = S::EPLD, EPR = S::EPR, CG = BN / 8, ITEMS = EPR * CG / NT;
    static_assert(ITEMS >= 1 && (EPR * CG) % NT == 0, "epilogue items");
    float* ep = (float*)smem;
    const bool vec_ok = ((a.cout & 7) == 0) && ((a.ldy & 7) == 0) && ((a.ycoff & 7) == 0) &&
                        (a.res_mode == VD_RES_NONE || (((a.res_ld | a.res_coff) & 7) == 0));
    unsigned* s_amax = (unsigned*)(smem + amax_off);   // per-frame max |y| of this tile (a.ymax)
    int tfb = -1;                                      // this thread's first frame and its running max;
    float tmax = 0.f;                                  // items of a later frame go to LDS directly (rare)
#pragma unroll
    for (int h = 0; h < BM / EPR; ++h) {
        if (h) __syncthreads();
        const int wrow = wm * S::WTM - h * EPR;        // this wave's first row within the pass
        if (wrow >= 0 && wrow < EPR) {
            if constexpr (MF == 32) {   // 32x32 C layout: row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            ep[(wrow + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)) * EPLD + wn * S::WTN +
                               j * 32 + (lane & 31)] = acc[i][j][r];
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            ep[(wrow + i * 16 + (lane >> 4) * 4 + r) * EPLD + wn * S::WTN + j * 16 + (lane & 15)] =
                                acc[i][j][r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ITEMS; ++q) {              // EPR rows x CG groups of 8 channels / NT threads
            const int it = tid + NT * q;
            const int rr = it / CG, cg = it % CG;
            const int m = m0 + h * EPR + rr;
            const int nb = n0 + cg * 8;
            const bool valid = m < a.M && nb < a.cout;
            const int fb = valid ? m / ohw : -1;
            float vmax = 0.f;
            if (valid) {
            const float* er = ep + rr * EPLD + cg * 8;
            const size_t yo = (size_t)m * a.ldy + a.ycoff + nb;
            const float inv_sa = TERMS != 3 ? __builtin_ldexpf(1.f, -act_scale_exp(a, fb)) : 1.f;
            size_t roff = 0;
            if (a.res_mode != VD_RES_NONE) {
                if (a.res_up) {
                    const int b = m / ohw, rem = m - b * ohw;
                    const int oy = rem / a.yw, ox = rem - oy * a.yw;
                    roff = ((size_t)(b * a.rh + (oy >> 1)) * a.rw + (ox >> 1)) * a.res_ld + a.res_coff + nb;
                } else {
                    roff = (size_t)m * a.res_ld + a.res_coff + nb;
                }
            }
            if (vec_ok) {
                const float4 s0 = *(const float4*)(a.scale + nb), s1 = *(const float4*)(a.scale + nb + 4);
                const float4 h0 = *(const float4*)(a.shift + nb), h1 = *(const float4*)(a.shift + nb + 4);
                const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
                const float4 e0 = *(const float4*)er, e1 = *(const float4*)(er + 4);
                const float ev[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
                float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (a.res_mode != VD_RES_NONE) {
                    const float4 r0 = *(const float4*)((const float*)a.res + roff);
                    const float4 r1 = *(const float4*)((const float*)a.res + roff + 4);
                    rv[0] = r0.x; rv[1] = r0.y; rv[2] = r0.z; rv[3] = r0.w;
                    rv[4] = r1.x; rv[5] = r1.y; rv[6] = r1.z; rv[7] = r1.w;
                }
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float t = (ev[e] * inv_sa) * sc[e] + sh[e];
                    if (a.res_mode == VD_RES_PRE_ACT) t += rv[e];
                    t = act_apply(t, a.act, a.slope);
                    if (a.res_mode == VD_RES_POST_ACT) t += rv[e];
                    v[e] = t;
                    vmax = fmaxf(vmax, fabsf(t));
                }
                *(float4*)((float*)a.y + yo) = make_float4(v[0], v[1], v[2], v[3]);
                *(float4*)((float*)a.y + yo + 4) = make_float4(v[4], v[5], v[6], v[7]);
            } else {
                for (int e = 0; e < 8 && nb + e < a.cout; ++e) {
                    const int n = nb + e;
                    float t = (er[e] * inv_sa) * a.scale[n] + a.shift[n];
                    const float rv = a.res_mode != VD_RES_NONE ? ((const float*)a.res)[roff + e] : 0.f;
                    if (a.res_mode == VD_RES_PRE_ACT) t += rv;
                    t = act_apply(t, a.act, a.slope);
                    if (a.res_mode == VD_RES_POST_ACT) t += rv;
                    ((float*)a.y)[yo + e] = t;
                    vmax = fmaxf(vmax, fabsf(t));
                }
            }
            }   // valid
            if (valid && a.ymax) {
                if (tfb < 0) tfb = fb;
                if (fb == tfb) tmax = fmaxf(tmax, vmax);
                else if (vmax > 0.f) atomicMax(s_amax + fb, __float_as_uint(vmax));
            }
        }
    }
    if (a.ymax) {
        amax_lds_add(s_amax, tfb, tmax);
        __syncthreads();
        amax_lds_flush(s_amax, a.ymax, a.B);
    }
}

// Epilogue of the transposed (TR) tiles straight from registers: the weight rows were
// loaded permuted (x6_tr_row), so MFMA blocks 2jp, 2jp+1 give lane (p = l % 16, q = l / 16)
// the 8 consecutive channels 32 jp + 8 q .. +7 of pixel 16 i + p: BN + residual +
// activation on 8 values, two 16-B stores, no LDS staging and no workgroup barrier
// (only the per-frame max goes through LDS). Same arithmetic as x6_epilogue.
template <class S>
__device__ __forceinline__ void x6_epilogue_tr(const ConvArgs& a, f32x4_t (&acc)[S::TM][S::TN], int m0, int n0,
                                               int wm, int wn, int lane, unsigned* s_amax) {
    constexpr int TM = S::TM, TN = S::TN, NJ = TN / 2;
    static_assert(TN % 2 == 0, "TR tiles pair the channel blocks");
    const int ohw = a.yh * a.yw;
    const int q = lane >> 4, pl = lane & 15;
    const int cb = n0 + wn * S::WTN + 8 * q;
    int fbs[TM];
    unsigned yrow[TM], rrow[TM];                     // byte offsets of the lane's output / residual row (channel 0)
    float inv[TM], vmax[TM];
    const bool res = a.res_mode != VD_RES_NONE;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm * S::WTM + 16 * i + pl;
        const bool ok = m < a.M;
        fbs[i] = ok ? m / ohw : -1;
        inv[i] = __builtin_ldexpf(1.f, -act_scale_exp(a, ok ? fbs[i] : 0));
        vmax[i] = 0.f;
        yrow[i] = ok ? (unsigned)(((size_t)m * a.ldy + a.ycoff) * 4) : 0x80000000u;
        rrow[i] = 0x80000000u;
        if (ok && res) {
            size_t roff;
            if (a.res_up) {
                const int b = fbs[i], rem = m - b * ohw;
                const int oy = rem / a.yw, ox = rem - oy * a.yw;
                roff = ((size_t)(b * a.rh + (oy >> 1)) * a.rw + (ox >> 1)) * a.res_ld;
            } else {
                roff = (size_t)m * a.res_ld;
            }
            rrow[i] = (unsigned)((roff + a.res_coff) * 4);
        }
    }
    // Buffer loads / stores (rows past M, channels past cout: out of range -> zeros /
    // dropped) keep the epilogue straight-line, and column pair jp + 1's residual and
    // BN rows are loaded before pair jp's stores: vmcnt retires loads and stores in issue
    // order, so a residual load issued after a store waited for that store too (the
    // round-5 epilogue waited on every (jp, i) row behind the stores before it).
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, res ? 0x7fffffff : 0,
                                                                         0x00020000);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.scale, 0, a.cout * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void*)a.shift, 0, a.cout * 4, 0x00020000);
    u32x4 rq[2][TM][2], sq[2][4];
    auto fetch = [&](int jp, int slot) {
        const unsigned cbytes = (unsigned)((cb + 32 * jp) * 4);
        sq[slot][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)cbytes, 0, 0));
        sq[slot][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)cbytes, 16, 0));
        sq[slot][2] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rh, (int)cbytes, 0, 0));
        sq[slot][3] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rh, (int)cbytes, 16, 0));
        if (res) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const unsigned o = rrow[i] == 0x80000000u ? rrow[i] : rrow[i] + cbytes;
                rq[slot][i][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, (int)o, 0, 0));
                rq[slot][i][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, (int)o, 16, 0));
            }
        }
    };
    fetch(0, 0);
#pragma unroll
    for (int jp = 0; jp < NJ; ++jp) {
        if (jp + 1 < NJ) fetch(jp + 1, (jp + 1) & 1);
        const int sl = jp & 1;
        const bool cok = cb + 32 * jp < a.cout;
        const unsigned cbytes = (unsigned)((cb + 32 * jp) * 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ev = e < 4 ? acc[i][2 * jp][e] : acc[i][2 * jp + 1][e - 4];
                const float sc = __uint_as_float(sq[sl][e >> 2][e & 3]), sh = __uint_as_float(sq[sl][2 + (e >> 2)][e & 3]);
                const float rv = res ? __uint_as_float(rq[sl][i][e >> 2][e & 3]) : 0.f;
                float t = (ev * inv[i]) * sc + sh;
                if (a.res_mode == VD_RES_PRE_ACT) t += rv;
                t = act_apply(t, a.act, a.slope);
                if (a.res_mode == VD_RES_POST_ACT) t += rv;
                v[e] = t;
                if (cok && fbs[i] >= 0) vmax[i] = fmaxf(vmax[i], fabsf(t));
            }
            const unsigned o = (yrow[i] == 0x80000000u || !cok) ? 0x80000000u : yrow[i] + cbytes;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned,
                                                                      make_float4(v[0], v[1], v[2], v[3])),
                                                   ry, (int)o, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned,
                                                                      make_float4(v[4], v[5], v[6], v[7])),
                                                   ry, (int)o, 16, 0);
        }
    }
    if (a.ymax) {
#pragma unroll
        for (int i = 0; i < TM; ++i) amax_lds_add(s_amax, fbs[i], vmax[i]);
        __syncthreads();
        amax_lds_flush(s_amax, a.ymax, a.B);
    }
}

// the register epilogue (x6_epilogue_tr) addresses y and the residual by 32-bit buffer offsets
static bool tr_bytes_ok(const ConvArgs& a) {
    const double lim = 2147483647.0;
    if ((double)a.M * a.ldy * 4 >= lim) return false;
    if (a.res_mode != VD_RES_NONE && (double)a.M * a.res_ld * 4 >= lim) return false;
    return true;
}

// LDS row -> weight row of a TR tile: row 16 j + i of each 32-row group holds channel
// 8 (i >> 2) + 4 (j & 1) + (i & 3) of the group, so blocks 2jp, 2jp+1 give a lane 8
// consecutive channels (conv1x1_x6_kernel's permutation)
__device__ __forceinline__ int x6_tr_row(int row) {
    const int j = (row >> 4) & 1, i = row & 15;
    return (row & ~31) + 8 * (i >> 2) + 4 * j + (i & 3);
}

}  // namespace

// What the dispatch (conv_x6.hip) calls in the other two files, a.tune and the schedule selectors set
bool vd_x6_halo_ok(const ConvArgs& a);                                     // the halo tiles take this conv
hipError_t vd_launch_x6_halo(const ConvArgs& a, int bn, hipStream_t s);   // N tile bn = 32 / 64 / 128 / 192 / 256
// terms = 2 (pairs) or 3 (triples): TAPS, the SiLU table, the 1x1 slices, in this order;
// true when one took the conv (*err: its launch status)
bool vd_launch_x6_stream(const ConvArgs& a, int terms, hipStream_t s, hipError_t* err);
hipError_t vd_launch_x6_dual(const ConvArgs& a, hipStream_t s);


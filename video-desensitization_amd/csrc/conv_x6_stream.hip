// conv_x6_stream.hip — the streaming kernels of the fp32 plan: 1x1 slices, TAPS, dual (contract and dispatch: conv_x6.hip)
#include "vd_kernel.h"
#include "conv_x6.h"
#include <algorithm>

namespace {

// Streaming 1x1 form for the memory-bound bottleneck convs (K = Cin in {64, 128,
// 256}): the split weight slice of NCH output channels sits in LDS for the whole
// (persistent) workgroup, and every wave streams groups of 16 output pixels with
// no workgroup barrier, so loads, MFMAs and stores of the CU's waves interleave.
// D^T[n][p] = sum_k W[n][k] X[p][k]: A = weight rows (LDS, split planes), B = the
// 16 pixels' 8 channels per lane loaded as 2 x 16 B f32 straight from NHWC and
// split in registers; weight rows are permuted so tiles 2i, 2i+1 give a lane 8
// consecutive output channels (two 16-B f32 stores, residual read in the same shape).
//
// TAPS form (round 4, the YOLO net's narrow KxK layers, K <= 288): each lane's 8-channel
// K chunk of every k-step is one (dy, dx, c) of the filter, fixed per lane, so the
// tap table sits in registers; a pixel's chunk is loaded through a buffer descriptor
// (off the frame -> zeros, conv padding) for every k-step. TERMS = 1: integer-valued
// input (x_exact canvases) on one plane against both weight planes. NTT = 1: 16
// output channels, a lane stores 4 consecutive ones.
// RL (round 6, option x6_stream_rl; plain 1x1 form only): the next group's input refills
// each k-step's registers right after that k-step is split (one register set instead of
// two), and the registers saved carry this group's residual, loaded at the top of the
// group beside the MFMAs instead of in the epilogue where its latency stood exposed.
template <int KS, int NTT, int ACT, int RES, int TERMS, bool TAPS = false, bool RL = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(TAPS ? 4 : 1)))   // TAPS: two workgroups per CU
void conv1x1_x6_kernel(ConvArgs a, int nchunks, int groups) {
    static_assert(!(RL && (TAPS || NTT == 1)), "RL: the plain 1x1 form with 8-channel lanes");
    constexpr int WT = TERMS == 1 ? 2 : TERMS;             // weight planes
    constexpr int NCH = 16 * NTT, PL = KS * NCH * 64;     // bytes per weight plane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_scale = (float*)(smem + WT * PL);
    float* s_shift = s_scale + NCH;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int chunk = local % nchunks;
    const int mblk = (local / nchunks) * 8 + xcd;
    const int nmblk = gridDim.x / nchunks;
    const int n0 = chunk * NCH;
    {   // split weights [n0, n0 + NCH) x K -> LDS [plane][ks][row][64 B]; row 16j + i holds
        // channel 32(j>>1) + 8(i>>2) + 4(j&1) + (i&3)
        const int nk = a.kpad / KT;
        for (int i = tid; i < WT * KS * NCH * 4; i += 512) {
            const int c = i & 3, row = (i >> 2) % NCH, pk = (i >> 2) / NCH, ks = pk % KS, p = pk / KS;
            const int j = row >> 4, ii = row & 15;
            const int chn = NTT == 1 ? row : 32 * (j >> 1) + 8 * (ii >> 2) + 4 * (j & 1) + (ii & 3);
            const u32x4 v = *(const u32x4*)((const char*)a.wx3 + ((((size_t)(n0 + chn) * nk + ks) * WT + p) * 64 + c * 16));
            *(u32x4*)(smem + p * PL + ks * NCH * 64 + swz64(row, c)) = v;
        }
        for (int i = tid; i < NCH; i += 512) {
            s_scale[i] = a.scale[n0 + i];
            s_shift[i] = a.shift[n0 + i];
        }
    }
    unsigned* s_amax = (unsigned*)(s_shift + NCH);        // per-frame max |y| (a.ymax)
    if (a.ymax)
        for (int f = tid; f < a.B; f += 512) s_amax[f] = 0u;
    __syncthreads();
    const int p_lane = lane & 15, q = lane >> 4;
    const int ohw = a.yh * a.yw;
    const int wstride = nmblk * 8;
    // TAPS: this lane's (dy, dx, c) per k-step; a chunk past K gets dy far off the frame
    int tdy[TAPS ? KS : 1], tdx[TAPS ? KS : 1], toff[TAPS ? KS : 1];
    if constexpr (TAPS) {
        const int kreal = a.kh * a.kw * a.cin_pad;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = ks * 32 + q * 8, t = k / a.cin_pad, c = k - t * a.cin_pad;
            const int dy = t / a.kw, dx = t - dy * a.kw;
            tdy[ks] = k < kreal ? dy : (1 << 28);
            tdx[ks] = dx;
            toff[ks] = (dy * a.xw + dx) * a.ldx + c;
        }
    }
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, 0, (int)((long)a.B * a.xh * a.xw * a.ldx * 4), 0x00020000);
    auto load = [&](int g, u32x4 (&xf)[KS][2]) {
        const int mu = g * 16 + p_lane;
        const int m = mu < a.M ? mu : a.M - 1;
        const int b = m / ohw, rem = m - b * ohw;
        const int oy = rem / a.yw, ox = rem - oy * a.yw;
        if constexpr (TAPS) {
            const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
            const int pbase = ((b * a.xh + iy0) * a.xw + ix0) * a.ldx + a.xcoff;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bool ok = ((unsigned)(iy0 + tdy[ks]) < (unsigned)a.xh) & ((unsigned)(ix0 + tdx[ks]) < (unsigned)a.xw);
                const unsigned off = ok ? (unsigned)(pbase + toff[ks]) * 4u : 0x80000000u;
                xf[ks][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)off, 0, 0));
                xf[ks][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)(off + 16u), 0, 0));
            }
        } else {
            const float* xp = (const float*)a.x + (((size_t)b * a.xh + oy * a.stride) * a.xw + ox * a.stride) * a.ldx +
                              a.xcoff + q * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                xf[ks][0] = *(const u32x4*)(xp + ks * 32);
                xf[ks][1] = *(const u32x4*)(xp + ks * 32 + 4);
            }
        }
    };
    (void)rsrc_x;
    u32x4 xf[KS][2];
    int g = mblk * 8 + wid;
    if (g < groups) load(g, xf);
    if constexpr (RL) {
        // pixel m's element offset of its input row (this lane's 8 channels)
        auto xrow = [&](int gg) -> const float* {
            const int mu = gg * 16 + p_lane;
            const int m = mu < a.M ? mu : a.M - 1;
            const int b = m / ohw, rem = m - b * ohw;
            const int oy = rem / a.yw, ox = rem - oy * a.yw;
            return (const float*)a.x + (((size_t)b * a.xh + oy * a.stride) * a.xw + ox * a.stride) * a.ldx + a.xcoff +
                   q * 8;
        };
        // the frame range of the group being split, loaded one group ahead (its load would
        // otherwise sit behind this group's residual loads in the in-order vmcnt)
        // (a buffer load, issued whether or not the range slots exist -- num_records 0 then
        // -- so the compiler's count of younger ops stays exact)
        const __amdgpu_buffer_rsrc_t rsrc_m =
            __builtin_amdgcn_make_buffer_rsrc((void*)a.xmax, 0, a.xmax ? a.B * 4 : 0, 0x00020000);
        auto frame_max = [&](int gg) -> float {
            const int mu = gg * 16 + p_lane;
            const int f = (mu < a.M ? mu : a.M - 1) / ohw;
            const float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc_m, f * 4, 0, 0));
            return a.xmax ? v : a.xbound;
        };
        float xm_cur = g < groups ? frame_max(g) : 0.f;
        const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(
            (void*)a.res, 0, RES != VD_RES_NONE ? (int)std::min<long>((long)a.M * a.res_ld * 4, 0x7fffffffL) : 0,
            0x00020000);
        for (; g < groups; g += wstride) {
            asm volatile("" ::: "memory");
            const int gn = g + wstride;
            const float* xpn = xrow(gn < groups ? gn : g);
            const float xm_next = frame_max(gn < groups ? gn : g);   // unconditional: straight-line vmcnt
            const int mu = g * 16 + p_lane;
            const int mcl = mu < a.M ? mu : a.M - 1;
            // this group's residual rows, in flight under the MFMAs
            float4 rr[NTT / 2][2];
            if constexpr (RES != VD_RES_NONE) {
                size_t roff;
                if (a.res_up) {
                    const int b = mcl / ohw, rem = mcl - b * ohw;
                    const int oy = rem / a.yw, ox = rem - oy * a.yw;
                    roff = ((size_t)(b * a.rh + (oy >> 1)) * a.rw + (ox >> 1)) * a.res_ld;
                } else {
                    roff = (size_t)mcl * a.res_ld;
                }
                roff += a.res_coff + n0 + q * 8;
                // buffer loads (rows past M read zeros): unconditional, issued here, not sunk
                // into the epilogue where their latency would stand exposed again
                const bool okr = mu < a.M;
#pragma unroll
                for (int i = 0; i < NTT / 2; ++i) {
                    const unsigned o = okr ? (unsigned)((roff + 32 * i) * 4) : 0x80000000u;
                    rr[i][0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_r, (int)o, 0, 0));
                    rr[i][1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_r, (int)o, 16, 0));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            f32x4_t acc[NTT];
#pragma unroll
            for (int j = 0; j < NTT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            const int fb = mcl / ohw;
            const int kexp = TERMS == 2 ? act_scale_exp_of(xm_cur) : 0;
            const float sa = __builtin_ldexpf(1.f, kexp), inv_sa = __builtin_ldexpf(1.f, -kexp);
            xm_cur = xm_next;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                float e8[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) e8[e] = __uint_as_float(xf[ks][e >> 2][e & 3]);
                u32x4 xb[3];
                split_pack<TERMS>(e8, sa, xb);
                // refill this k-step's registers with the next group's (the last group re-reads
                // its own rows: no branch, so the compiler counts vmcnt exactly)
                xf[ks][0] = *(const u32x4*)(xpn + ks * 32);
                xf[ks][1] = *(const u32x4*)(xpn + ks * 32 + 4);
#pragma unroll
                for (int j = 0; j < NTT; ++j) {
                    u32x4 wf[3];
#pragma unroll
                    for (int p = 0; p < WT; ++p)
                        wf[p] = *(const u32x4*)(smem + p * PL + ks * NCH * 64 + swz64(16 * j + p_lane, q));
                    acc[j] = mfma_terms<TERMS>(wf, xb, acc[j]);
                }
            }
            float vmax = 0.f;
            if (mu < a.M) {
                const size_t yo = (size_t)mu * a.ldy + a.ycoff + n0 + q * 8;
#pragma unroll
                for (int i = 0; i < NTT / 2; ++i) {
                    const int c = 32 * i + q * 8;
                    const float4 s0 = *(const float4*)(s_scale + c), s1 = *(const float4*)(s_scale + c + 4);
                    const float4 h0 = *(const float4*)(s_shift + c), h1 = *(const float4*)(s_shift + c + 4);
                    const f32x4_t& lo = acc[2 * i];
                    const f32x4_t& hi = acc[2 * i + 1];
                    float v[8] = {(lo[0] * inv_sa) * s0.x + h0.x, (lo[1] * inv_sa) * s0.y + h0.y,
                                  (lo[2] * inv_sa) * s0.z + h0.z, (lo[3] * inv_sa) * s0.w + h0.w,
                                  (hi[0] * inv_sa) * s1.x + h1.x, (hi[1] * inv_sa) * s1.y + h1.y,
                                  (hi[2] * inv_sa) * s1.z + h1.z, (hi[3] * inv_sa) * s1.w + h1.w};
                    float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if constexpr (RES != VD_RES_NONE) {
                        rv[0] = rr[i][0].x; rv[1] = rr[i][0].y; rv[2] = rr[i][0].z; rv[3] = rr[i][0].w;
                        rv[4] = rr[i][1].x; rv[5] = rr[i][1].y; rv[6] = rr[i][1].z; rv[7] = rr[i][1].w;
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float t = v[e];
                        if constexpr (RES == VD_RES_PRE_ACT) t += rv[e];
                        t = act_apply(t, ACT, a.slope);
                        if constexpr (RES == VD_RES_POST_ACT) t += rv[e];
                        v[e] = t;
                        vmax = fmaxf(vmax, fabsf(t));
                    }
                    *(float4*)((float*)a.y + yo + 32 * i) = make_float4(v[0], v[1], v[2], v[3]);
                    *(float4*)((float*)a.y + yo + 32 * i + 4) = make_float4(v[4], v[5], v[6], v[7]);
                }
            }
            if (a.ymax) amax_lds_add(s_amax, mu < a.M ? fb : -1, vmax);
        }
        if (a.ymax) {
            __syncthreads();
            amax_lds_flush(s_amax, a.ymax, a.B);
        }
        return;
    }
    for (; g < groups; g += wstride) {
        asm volatile("" ::: "memory");
        u32x4 xn[KS][2];
        const int gn = g + wstride;
        if (gn < groups) load(gn, xn);
        f32x4_t acc[NTT];
#pragma unroll
        for (int j = 0; j < NTT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const int mu = g * 16 + p_lane;
        const int fb = (mu < a.M ? mu : a.M - 1) / ohw;     // this lane's pixel's frame
        const int kexp = TERMS == 2 ? act_scale_exp(a, fb) : 0;
        const float sa = __builtin_ldexpf(1.f, kexp), inv_sa = __builtin_ldexpf(1.f, -kexp);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float e8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) e8[e] = __uint_as_float(xf[ks][e >> 2][e & 3]);
            u32x4 xb[3];
            split_pack<TERMS>(e8, sa, xb);
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                u32x4 wf[3];
#pragma unroll
                for (int p = 0; p < WT; ++p)
                    wf[p] = *(const u32x4*)(smem + p * PL + ks * NCH * 64 + swz64(16 * j + p_lane, q));
                if constexpr (TERMS == 1) {   // w_lo x + w_hi x (x exact on one plane)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf[1]),
                                                                    __builtin_bit_cast(f16x8_t, xb[0]), acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf[0]),
                                                                    __builtin_bit_cast(f16x8_t, xb[0]), acc[j], 0, 0, 0);
                } else {
                    acc[j] = mfma_terms<TERMS>(wf, xb, acc[j]);
                }
            }
        }
        float vmax = 0.f;
        if (a.dbg & 1) {                                   // timing-only (x6_dbg bit 0): no epilogue
            if (acc[0][0] == 1234.5f) ((float*)a.y)[tid] = 1.f;
        } else if (mu < a.M) {
            const int m = mu;
            size_t roff = 0;
            if constexpr (RES != VD_RES_NONE) {
                if (a.res_up) {
                    const int b = m / ohw, rem = m - b * ohw;
                    const int oy = rem / a.yw, ox = rem - oy * a.yw;
                    roff = ((size_t)(b * a.rh + (oy >> 1)) * a.rw + (ox >> 1)) * a.res_ld;
                } else {
                    roff = (size_t)m * a.res_ld;
                }
                roff += a.res_coff + n0 + q * 8;
            }
            if constexpr (NTT == 1) {   // rows = channels: a lane holds channels 4q .. 4q + 3
                if constexpr (RES != VD_RES_NONE) roff -= q * 4;
                const size_t yo1 = (size_t)m * a.ldy + a.ycoff + n0 + q * 4;
                const int c = q * 4;
                float v[4];
                float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (RES != VD_RES_NONE) r4 = *(const float4*)((const float*)a.res + roff);
                const float rv[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = (acc[0][e] * inv_sa) * s_scale[c + e] + s_shift[c + e];
                    if constexpr (RES == VD_RES_PRE_ACT) t += rv[e];
                    t = act_apply(t, ACT, a.slope);
                    if constexpr (RES == VD_RES_POST_ACT) t += rv[e];
                    v[e] = t;
                    vmax = fmaxf(vmax, fabsf(t));
                }
                *(float4*)((float*)a.y + yo1) = make_float4(v[0], v[1], v[2], v[3]);
            }
            const size_t yo = (size_t)m * a.ldy + a.ycoff + n0 + q * 8;
#pragma unroll
            for (int i = 0; i < NTT / 2; ++i) {
                const int c = 32 * i + q * 8;
                const float4 s0 = *(const float4*)(s_scale + c), s1 = *(const float4*)(s_scale + c + 4);
                const float4 h0 = *(const float4*)(s_shift + c), h1 = *(const float4*)(s_shift + c + 4);
                const f32x4_t& lo = acc[2 * i];
                const f32x4_t& hi = acc[2 * i + 1];
                float v[8] = {(lo[0] * inv_sa) * s0.x + h0.x, (lo[1] * inv_sa) * s0.y + h0.y,
                              (lo[2] * inv_sa) * s0.z + h0.z, (lo[3] * inv_sa) * s0.w + h0.w,
                              (hi[0] * inv_sa) * s1.x + h1.x, (hi[1] * inv_sa) * s1.y + h1.y,
                              (hi[2] * inv_sa) * s1.z + h1.z, (hi[3] * inv_sa) * s1.w + h1.w};
                float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if constexpr (RES != VD_RES_NONE) {
                    const float4 r0 = *(const float4*)((const float*)a.res + roff + 32 * i);
                    const float4 r1 = *(const float4*)((const float*)a.res + roff + 32 * i + 4);
                    rv[0] = r0.x; rv[1] = r0.y; rv[2] = r0.z; rv[3] = r0.w;
                    rv[4] = r1.x; rv[5] = r1.y; rv[6] = r1.z; rv[7] = r1.w;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float t = v[e];
                    if constexpr (RES == VD_RES_PRE_ACT) t += rv[e];
                    t = act_apply(t, ACT, a.slope);
                    if constexpr (RES == VD_RES_POST_ACT) t += rv[e];
                    v[e] = t;
                    vmax = fmaxf(vmax, fabsf(t));
                }
                *(float4*)((float*)a.y + yo + 32 * i) = make_float4(v[0], v[1], v[2], v[3]);
                *(float4*)((float*)a.y + yo + 32 * i + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        if (a.ymax) amax_lds_add(s_amax, mu < a.M ? fb : -1, vmax);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { xf[ks][0] = xn[ks][0]; xf[ks][1] = xn[ks][1]; }
    }
    if (a.ymax) {
        __syncthreads();
        amax_lds_flush(s_amax, a.ymax, a.B);
    }
}

// Dual streaming form (fp16 pairs): a bottleneck's conv3 (+bn3) and its downsample
// (+bn, strided 1x1 over the block input) for the same output pixels in one pass,
// y = relu((bn3(conv3(t2))) + bn_d(ds(x))): the downsample output never goes
// through HBM. The two products keep their own per-frame operand scales (t2's and
// x's producers' max), and the downsample term is rounded to f32 before the add as
// the unfused plan stores it, so the result is bit-identical to conv_ds followed by
// conv3 with a pre-activation residual. Layer1.0 (K 64 + 64).
template <int KS, int KS2, int NTT>
__global__ __launch_bounds__(512) void conv1x1_x6_dual_kernel(ConvArgs a, int nchunks, int groups) {
    constexpr int NCH = 16 * NTT, PL = KS * NCH * 64, PL2 = KS2 * NCH * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* w2s = smem + 2 * PL;
    float* s_scale = (float*)(w2s + 2 * PL2);
    float* s_shift = s_scale + NCH;
    float* s_scale2 = s_shift + NCH;
    float* s_shift2 = s_scale2 + NCH;
    unsigned* s_amax = (unsigned*)(s_shift2 + NCH);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int chunk = local % nchunks;
    const int mblk = (local / nchunks) * 8 + xcd;
    const int nmblk = gridDim.x / nchunks;
    const int n0 = chunk * NCH;
    auto stage_w = [&](const void* wsrc, int kpad, int ks_n, char* dst, int pl) {
        const int nk = kpad / KT;
        for (int i = tid; i < 2 * ks_n * NCH * 4; i += 512) {
            const int c = i & 3, row = (i >> 2) % NCH, pk = (i >> 2) / NCH, ks = pk % ks_n, p = pk / ks_n;
            const int j = row >> 4, ii = row & 15;
            const int chn = 32 * (j >> 1) + 8 * (ii >> 2) + 4 * (j & 1) + (ii & 3);
            const u32x4 v = *(const u32x4*)((const char*)wsrc + ((((size_t)(n0 + chn) * nk + ks) * 2 + p) * 64 + c * 16));
            *(u32x4*)(dst + p * pl + ks * NCH * 64 + swz64(row, c)) = v;
        }
    };
    stage_w(a.wx3, a.kpad, KS, smem, PL);
    stage_w(a.wx3_2, a.kpad2, KS2, w2s, PL2);
    for (int i = tid; i < NCH; i += 512) {
        s_scale[i] = a.scale[n0 + i];
        s_shift[i] = a.shift[n0 + i];
        s_scale2[i] = a.scale2[n0 + i];
        s_shift2[i] = a.shift2[n0 + i];
    }
    if (a.ymax)
        for (int f = tid; f < a.B; f += 512) s_amax[f] = 0u;
    __syncthreads();
    const int p_lane = lane & 15, q = lane >> 4;
    const int ohw = a.yh * a.yw;
    const int wstride = nmblk * 8;
    auto load = [&](int g, u32x4 (&xf)[KS][2], u32x4 (&xf2)[KS2][2]) {
        const int mu = g * 16 + p_lane;
        const int m = mu < a.M ? mu : a.M - 1;
        const int b = m / ohw, rem = m - b * ohw;
        const int oy = rem / a.yw, ox = rem - oy * a.yw;
        const float* xp = (const float*)a.x + (((size_t)b * a.xh + oy * a.stride) * a.xw + ox * a.stride) * a.ldx +
                          a.xcoff + q * 8;
        const float* xp2 = (const float*)a.x2 +
                           (((size_t)b * a.xh2 + oy * a.stride2) * a.xw2 + ox * a.stride2) * a.ldx2 + a.xcoff2 + q * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            xf[ks][0] = *(const u32x4*)(xp + ks * 32);
            xf[ks][1] = *(const u32x4*)(xp + ks * 32 + 4);
        }
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) {
            xf2[ks][0] = *(const u32x4*)(xp2 + ks * 32);
            xf2[ks][1] = *(const u32x4*)(xp2 + ks * 32 + 4);
        }
    };
    auto gemm = [&](f32x4_t (&acc)[NTT], const auto& xf, const char* wl, int pl, float sa) {
        constexpr int ks_n = sizeof(xf) / sizeof(xf[0]);
#pragma unroll
        for (int ks = 0; ks < ks_n; ++ks) {
            float e8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) e8[e] = __uint_as_float(xf[ks][e >> 2][e & 3]);
            u32x4 xb[3];
            split_pack<2>(e8, sa, xb);
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                u32x4 wf[3];
#pragma unroll
                for (int p = 0; p < 2; ++p) wf[p] = *(const u32x4*)(wl + p * pl + ks * NCH * 64 + swz64(16 * j + p_lane, q));
                acc[j] = mfma_pair(wf, xb, acc[j]);
            }
        }
    };
    ConvArgs a2 = a;                                       // the downsample input's range slots
    a2.xmax = a.x2max;
    a2.xbound = a.x2bound;
    u32x4 xf[KS][2], xf2[KS2][2];
    int g = mblk * 8 + wid;
    if (g < groups) load(g, xf, xf2);
    for (; g < groups; g += wstride) {
        asm volatile("" ::: "memory");
        u32x4 xn[KS][2], xn2[KS2][2];
        const int gn = g + wstride;
        if (gn < groups) load(gn, xn, xn2);
        const int mu = g * 16 + p_lane;
        const int fb = (mu < a.M ? mu : a.M - 1) / ohw;
        const int k1 = act_scale_exp(a, fb), k2 = act_scale_exp(a2, fb);
        f32x4_t acc[NTT], acc2[NTT];
#pragma unroll
        for (int j = 0; j < NTT; ++j) acc[j] = acc2[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        gemm(acc, xf, smem, PL, __builtin_ldexpf(1.f, k1));
        gemm(acc2, xf2, w2s, PL2, __builtin_ldexpf(1.f, k2));
        const float inv1 = __builtin_ldexpf(1.f, -k1), inv2 = __builtin_ldexpf(1.f, -k2);
        float vmax = 0.f;
        if (mu < a.M) {
            const size_t yo = (size_t)mu * a.ldy + a.ycoff + n0 + q * 8;
#pragma unroll
            for (int i = 0; i < NTT / 2; ++i) {
                const int c = 32 * i + q * 8;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a1 = (e < 4 ? acc[2 * i][e] : acc[2 * i + 1][e - 4]);
                    const float a2v = (e < 4 ? acc2[2 * i][e] : acc2[2 * i + 1][e - 4]);
                    const float r = (a2v * inv2) * s_scale2[c + e] + s_shift2[c + e];   // the stored ds value
                    float t = (a1 * inv1) * s_scale[c + e] + s_shift[c + e];
                    t += r;
                    t = t > 0.f ? t : 0.f;
                    v[e] = t;
                    vmax = fmaxf(vmax, t);
                }
                *(float4*)((float*)a.y + yo + 32 * i) = make_float4(v[0], v[1], v[2], v[3]);
                *(float4*)((float*)a.y + yo + 32 * i + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        if (a.ymax) amax_lds_add(s_amax, mu < a.M ? fb : -1, vmax);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { xf[ks][0] = xn[ks][0]; xf[ks][1] = xn[ks][1]; }
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) { xf2[ks][0] = xn2[ks][0]; xf2[ks][1] = xn2[ks][1]; }
    }
    if (a.ymax) {
        __syncthreads();
        amax_lds_flush(s_amax, a.ymax, a.B);
    }
}

template <int KS, int KS2, int NTT>
hipError_t launch_dual_x6(const ConvArgs& a0, hipStream_t s) {
    constexpr int NCH = 16 * NTT;
    constexpr int lds = 2 * (KS + KS2) * NCH * 64 + 4 * NCH * 4;
    static const int resident = [] {
        (void)hipFuncSetAttribute((const void*)conv1x1_x6_dual_kernel<KS, KS2, NTT>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds + 4 * kAmaxFrames);
        int dev = 0, cus = 256, per_cu = 1;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv1x1_x6_dual_kernel<KS, KS2, NTT>, 512, lds);
        return std::max(1, cus * std::max(1, per_cu));
    }();
    ConvArgs a = a0;
    a.scale = a.scale_x;                                   // per-channel rescaled BN scales of the pairs
    a.scale2 = a.scale2_x;
    const int nchunks = a.cout / NCH;
    const int groups = (a.M + 15) / 16;
    int k = std::max(1, resident / (8 * nchunks));
    k = std::min(k, std::max(1, (groups + 63) / 64));
    vd_conv_fam_set(VD_FAM_X6_DUAL);
    hipLaunchKernelGGL((conv1x1_x6_dual_kernel<KS, KS2, NTT>), dim3(8 * nchunks * k), dim3(512),
                       lds + (a.ymax ? 4 * a.B : 0), s, a, nchunks, groups);
    return hipGetLastError();
}

template <int KS, int NTT, int ACT, int RES, int TERMS, bool TAPS = false, bool RL = false>
hipError_t launch_stream_x6(const ConvArgs& a, hipStream_t s) {
    // option x6_stream_rl (default 1): the RL form for the layers with a residual (layer3
    // conv3 330 -> 299 us, layer2 conv3 416 -> 404 in x6bench); without one it measured
    // slower (layer2.0 conv1 577 -> 603), so those keep the two-set form
    if constexpr (!TAPS && !RL && NTT >= 2 && TERMS == 2 && RES != VD_RES_NONE) {
        if (a.tune->x6_stream_rl) return launch_stream_x6<KS, NTT, ACT, RES, TERMS, false, true>(a, s);
    }
    constexpr int NCH = 16 * NTT;
    constexpr int lds = (TERMS == 1 ? 2 : TERMS) * KS * NCH * 64 + 2 * NCH * 4;
    static const int resident = [] {
        (void)hipFuncSetAttribute((const void*)conv1x1_x6_kernel<KS, NTT, ACT, RES, TERMS, TAPS, RL>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds + 4 * kAmaxFrames);
        int dev = 0, cus = 256, per_cu = 1;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv1x1_x6_kernel<KS, NTT, ACT, RES, TERMS, TAPS, RL>,
                                                           512, lds);
        return std::max(1, cus * std::max(1, per_cu));
    }();
    const int nchunks = a.cout / NCH;
    const int groups = (a.M + 15) / 16;
    int k = std::max(1, resident / (8 * nchunks));
    k = std::min(k, std::max(1, (groups + 63) / 64));
    vd_conv_fam_set(TAPS ? VD_FAM_X6_TAPS : VD_FAM_X6_STREAM);
    hipLaunchKernelGGL((conv1x1_x6_kernel<KS, NTT, ACT, RES, TERMS, TAPS, RL>), dim3(8 * nchunks * k), dim3(512),
                       lds + (a.ymax ? 4 * a.B : 0), s, a, nchunks, groups);
    return hipGetLastError();
}

// TAPS streaming form (fp16 pairs): the narrow KxK layers of the YOLO net -- Cin a
// multiple of 8, K (padded) <= 160, Cout 16 / 32 as one channel slice, SiLU (the
// C2f bottleneck's shortcut as a post-activation residual) -- and the space-to-depth
// model.0 on its integer canvas (x_exact: one A plane). Returns false when not taken.
static bool launch_taps_x6(const ConvArgs& a, hipStream_t s, hipError_t* err) {
    // plain 1x1 convs go to the streaming form unless their K is padded (model.2's cv2 over
    // the 48-channel C2f concat: K 48 in a 64-wide k range)
    if (!a.tune->x6_taps || (a.kh == 1 && a.kw == 1 && a.pad == 0 && a.stride == 1 && a.kpad == a.cin_pad)) return false;
    if (a.act != VD_ACT_SILU || (a.res_mode != VD_RES_NONE && a.res_mode != VD_RES_POST_ACT)) return false;
    if ((a.cin_pad & 7) || ((a.ldx | a.xcoff) & 3) || ((a.ldy | a.ycoff) & 7)) return false;
    if (a.res_mode != VD_RES_NONE && (a.res_up || ((a.res_ld | a.res_coff) & 7))) return false;
    if (a.kpad > 160 || a.kpad % 32) return false;
    const int ks = a.kpad / 32, co = a.cout;
    const bool post = a.res_mode == VD_RES_POST_ACT;
#define VD_TAPS(KS, NTT, T)                                                                                        \
    do {                                                                                                           \
        *err = post ? launch_stream_x6<KS, NTT, VD_ACT_SILU, VD_RES_POST_ACT, T, true>(a, s)                       \
                    : launch_stream_x6<KS, NTT, VD_ACT_SILU, VD_RES_NONE, T, true>(a, s);                          \
        return true;                                                                                               \
    } while (0)
    if (a.x_exact) {
        if (ks == 2 && co == 16 && !post) {
            *err = launch_stream_x6<2, 1, VD_ACT_SILU, VD_RES_NONE, 1, true>(a, s);
            return true;
        }
        return false;
    }
    // K <= 160 only: at K = 288 (model.3, the 32-channel bottlenecks at 80x48) the
    // two register sets of x need ~210 VGPRs, one workgroup per CU, and the form
    // measured 5-40 % slower than the GEMM / halo tiles
    if (ks == 2 && co == 32) VD_TAPS(2, 2, 2);
    if (ks == 5 && co == 16) VD_TAPS(5, 1, 2);
    if (ks == 5 && co == 32) VD_TAPS(5, 2, 2);
#undef VD_TAPS
    return false;
}

template <int KS, int NTT, int TERMS>
hipError_t stream_mode_x6(const ConvArgs& a, hipStream_t s) {
    if (a.act == VD_ACT_RELU) {
        if (a.res_mode == VD_RES_PRE_ACT) return launch_stream_x6<KS, NTT, VD_ACT_RELU, VD_RES_PRE_ACT, TERMS>(a, s);
        if (a.res_mode == VD_RES_NONE) return launch_stream_x6<KS, NTT, VD_ACT_RELU, VD_RES_NONE, TERMS>(a, s);
    }
    if (a.act == VD_ACT_NONE && a.res_mode == VD_RES_NONE)
        return launch_stream_x6<KS, NTT, VD_ACT_NONE, VD_RES_NONE, TERMS>(a, s);
    return hipErrorInvalidValue;   // excluded by stream_x6_nch
}

// Streaming 1x1 (conv1x1_x6_kernel): 1x1 taps without padding, K = Cin in {64, 128,
// 256} (one channel slice of 128, or 64 at K = 256, fits 96 KB of LDS in three split
// planes), ReLU with / without the pre-activation residual, or no activation.
static int stream_x6_nch(const ConvArgs& a, int terms) {
    if (!a.tune->x6_stream || a.kh != 1 || a.kw != 1 || a.pad != 0 || a.kpad != a.cin_pad) return 0;
    if (a.cin_pad != 64 && a.cin_pad != 128 && a.cin_pad != 256) return 0;
    const bool mode = (a.act == VD_ACT_RELU && (a.res_mode == VD_RES_NONE || a.res_mode == VD_RES_PRE_ACT)) ||
                      (a.act == VD_ACT_NONE && a.res_mode == VD_RES_NONE);
    if (!mode || ((a.ldx | a.xcoff | a.ldy | a.ycoff) & 7)) return 0;
    if (a.res_mode != VD_RES_NONE && ((a.res_ld | a.res_coff) & 7)) return 0;
    const int nch = (a.cin_pad == 256 && terms == 3) ? 64 : 128;
    if (a.cout % nch == 0) return nch;
    return a.cout % 64 == 0 && a.cin_pad <= 128 ? 64 : 0;
}

// the conv stream_x6_nch took, on slices of nch channels
template <int TERMS>
static hipError_t launch_slices_x6(const ConvArgs& a, int nch, hipStream_t s) {
    if constexpr (TERMS == 2) {   // 256-channel slices: each pixel read by half as many workgroups
        if (a.tune->x6_stream256 && a.cout % 256 == 0) {
            if (a.cin_pad == 64) return stream_mode_x6<2, 16, TERMS>(a, s);
            if (a.cin_pad == 128 && a.tune->x6_stream256 > 1) return stream_mode_x6<4, 16, TERMS>(a, s);   // 128 KB LDS
        }
    }
    if (a.cin_pad == 64) return nch == 128 ? stream_mode_x6<2, 8, TERMS>(a, s) : stream_mode_x6<2, 4, TERMS>(a, s);
    if (a.cin_pad == 128) return nch == 128 ? stream_mode_x6<4, 8, TERMS>(a, s) : stream_mode_x6<4, 4, TERMS>(a, s);
    if constexpr (TERMS == 2) return stream_mode_x6<8, 8, TERMS>(a, s);
    return stream_mode_x6<8, 4, TERMS>(a, s);
}

// The streaming decisions of one conv, in this order: TAPS, the SiLU table, the slices
template <int TERMS>
static bool stream_terms(const ConvArgs& a, hipStream_t s, hipError_t* err) {
    if constexpr (TERMS == 2) {
        if (launch_taps_x6(a, s, err)) return true;
        // YOLO's SiLU 1x1 convs (C2f cv1 / cv2, SPPF cv1) on the streaming form
        if (a.tune->x6_stream_silu && a.act == VD_ACT_SILU && a.res_mode == VD_RES_NONE && a.kh == 1 &&
            a.kw == 1 && a.pad == 0 && a.kpad == a.cin_pad && !((a.ldx | a.xcoff | a.ldy | a.ycoff) & 7)) {
            const int k = a.cin_pad, co = a.cout;
            const int nch = co % 128 == 0 ? 128 : (co % 64 == 0 ? 64 : (co % 32 == 0 ? 32 : 0));
            if (nch) {
#define VD_SILU(KS, NTT) return (*err = launch_stream_x6<KS, NTT, VD_ACT_SILU, VD_RES_NONE, 2>(a, s), true)
                if (k == 32 && nch == 32) VD_SILU(1, 2);
                if (k == 32 && nch == 64) VD_SILU(1, 4);
                if (k == 64 && nch == 64) VD_SILU(2, 4);
                if (k == 64 && nch == 128) VD_SILU(2, 8);
                if (k == 96 && nch == 64) VD_SILU(3, 4);
                if (k == 128 && nch == 64) VD_SILU(4, 4);
                if (k == 128 && nch == 128) VD_SILU(4, 8);
                if (k == 192 && nch == 64) VD_SILU(6, 4);
                if (k == 192 && nch == 128) VD_SILU(6, 8);
                if (k == 256 && nch == 128) VD_SILU(8, 8);
#undef VD_SILU
            }
        }
    }
    const int nch = stream_x6_nch(a, TERMS);
    if (nch) *err = launch_slices_x6<TERMS>(a, nch, s);
    return nch != 0;
}

}  // namespace

bool vd_launch_x6_stream(const ConvArgs& a, int terms, hipStream_t s, hipError_t* err) {
    return terms == 2 ? stream_terms<2>(a, s, err) : stream_terms<3>(a, s, err);
}

// fp16 pairs: bottleneck conv3 (1x1, K 64 / 128, ReLU) + downsample (1x1, K 64 / 256,
// strided, no activation) as conv1x1_x6_dual_kernel
bool vd_conv1x1_x6_dual_ok(const ConvArgs& a) {
    if (a.f32_split != 2 || !a.wx3 || !a.wx3_2 || !a.scale_x || !a.scale2_x) return false;
    if (a.kh != 1 || a.kw != 1 || a.pad != 0 || a.stride != 1 || a.kpad != a.cin_pad || a.kpad2 != a.cin2_pad) return false;
    if (a.act != VD_ACT_RELU || a.res_mode != VD_RES_NONE) return false;
    if (((a.ldx | a.xcoff | a.ldy | a.ycoff | a.ldx2 | a.xcoff2) & 7)) return false;
    // layer1.0 only: at layer2.0 (K 128 + 256) the weights of both fit LDS only as
    // 64-channel slices, every pixel is then split for 8 slices instead of 4 and the
    // pass measured level with the two launches (839 vs 424 + 433 us)
    return a.cin_pad == 64 && a.kpad2 == 64 && a.cout % 128 == 0;
}

hipError_t vd_launch_x6_dual(const ConvArgs& a, hipStream_t s) { return launch_dual_x6<2, 2, 8>(a, s); }


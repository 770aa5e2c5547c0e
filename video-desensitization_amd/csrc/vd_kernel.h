// vd_kernel.h — device code shared by the kernel files: vector types, the 16-bit
// operand traits, activations, LDS row swizzles, wait-count helpers, the fp16-pair
// contract of the fp32 plan, and the per-frame max |y| tracking. Host / kernel
// structs and launcher prototypes are in vd_common.h.
#pragma once
#include "vd_common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // native vectors (HIP's uint4 is a struct)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void_t;    // LDS-DMA destination

// The 16-bit operand type of the bf16 plan (F16 = false) and the fp16 plan (VD_PREC_FP16,
// F16 = true): element type, 8-vector, the 16x16x32 matrix-core product, and the two
// elements of a packed 32-bit word as f32. Conversions to T are round-to-nearest-even.
template <bool F16> struct Half16;
template <> struct Half16<false> {
    typedef __bf16 T;
    typedef bf16x8_t V8;
    static __device__ __forceinline__ f32x4_t mfma(const u32x4& a, const u32x4& b, const f32x4_t& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                       c, 0, 0, 0);
    }
    static __device__ __forceinline__ float lo(unsigned u) { return __uint_as_float(u << 16); }
    static __device__ __forceinline__ float hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
};
template <> struct Half16<true> {
    typedef _Float16 T;
    typedef f16x8_t V8;
    static __device__ __forceinline__ f32x4_t mfma(const u32x4& a, const u32x4& b, const f32x4_t& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b),
                                                      c, 0, 0, 0);
    }
    static __device__ __forceinline__ float lo(unsigned u) {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xFFFFu));
    }
    static __device__ __forceinline__ float hi(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }
};

// Activation of the fused epilogues: by the layer's runtime code, or (streaming 1x1
// kernel) by a compile-time one, so the epilogue has no per-element branches.
__device__ __forceinline__ float act_apply(float v, int act, float slope) {
    if (act == VD_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == VD_ACT_LEAKY) return v > 0.f ? v : v * slope;
    if (act == VD_ACT_SILU) return v / (1.0f + __expf(-v));
    return v;
}
template <int ACT>
__device__ __forceinline__ float act_apply(float v, float slope) {
    if constexpr (ACT == VD_ACT_RELU) return v > 0.f ? v : 0.f;
    if constexpr (ACT == VD_ACT_LEAKY) return v > 0.f ? v : v * slope;
    if constexpr (ACT == VD_ACT_SILU) return v / (1.0f + __expf(-v));
    return v;
}

// ---- LDS row swizzles: byte offset of 16-B chunk `chunk` of row `row` ----
// 128-B rows read as MFMA fragments of 16 ALIGNED consecutive rows (GEMM tiles, the
// stem tile): conflict-free ds_read_b128.
__device__ __forceinline__ int swz128(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// 128-B rows read at ANY 16 consecutive rows (the bottleneck kernels' t1 / t2 images:
// stage 2 reads windows shifted by the tap offsets). Each 16-lane LDS group holds all
// 16 rows once, 8 of them at chunk c and 8 at c ^ 1 in a cyclic block of 4 row pairs,
// and this XOR keeps the 8 even (and the 8 odd) rows on distinct 16-B slots for every
// block position (exhaustive check; swz128 is 2-way there).
__device__ __forceinline__ int swz128_any(int row, int chunk) {
    return row * 128 + ((chunk ^ (((row >> 1) & 3) << 1)) << 4);
}
// 64-B rows (32 16-bit elements: one k-step of one operand plane), 16 aligned rows
__device__ __forceinline__ int swz64(int row, int chunk) { return row * 64 + ((chunk ^ (((row >> 3) & 1) * 3)) << 4); }

// s_waitcnt immediate for vmcnt(n), expcnt / lgkmcnt left alone (gfx9 encoding:
// vmcnt[3:0] | vmcnt[5:4] << 14), for __builtin_amdgcn_s_waitcnt
constexpr int vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }

// s_barrier after this wave's LDS ops retire (no global-memory fence)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- The fp16-pair contract of the fp32 plan (f32_split = 2) ----------------------
// Scale. Each frame's activations are scaled by a power of two so their largest
// magnitude (the producer's per-frame running max, or a static bound for the
// letterboxed canvas) lands in [2^14, 2^15): fp16 never overflows and the low term
// stays normal down to 2^-2 of that. A row (pixel) keeps one scale over all of K, so
// the accumulator is scaled back per row in the epilogue (exact: powers of two), and a
// frame's result does not depend on the rest of its batch. The fused kernels apply the
// same rule to a tile's or a pixel's own maximum where the operand never leaves the
// chip (block32.hip, chain32.hip).
// Split. x 2^k is exact, so each term is ONE rounding of a fused multiply-add to fp16
// (v_fma_mixlo_f16): hi = RNE(x 2^k), lo = RNE(x 2^k - hi) (the residual is exact in
// f32); hi + lo keeps 22-24 significand bits of x.
// Product. (a_hi + a_lo)(b_hi + b_lo) without a_lo b_lo: three f16 MFMAs into the f32
// accumulator, small terms first. Operand planes are arrays [0] = hi, [1] = lo.
// The weights' side of the contract is vd_pack_x3h (conv_x6.hip, host).

// the exponent k (operand * 2^k) from a maximum m
__device__ __forceinline__ int act_scale_exp_of(float m) {
    if (!(m > 0.f) || !(m < 3.0e38f)) return 0;
    int e;
    (void)frexpf(m, &e);                              // m < 2^e
    const int k = 15 - e;
    return k < -100 ? -100 : (k > 100 ? 100 : k);
}
// ... of frame b of a conv's input
__device__ __forceinline__ int act_scale_exp(const ConvArgs& a, int b) {
    return act_scale_exp_of(a.xmax ? __uint_as_float(a.xmax[b]) : a.xbound);
}

__device__ __forceinline__ _Float16 pair_hi(float x, float sa) { return (_Float16)__builtin_fmaf(x, sa, 0.f); }
__device__ __forceinline__ _Float16 pair_lo(float x, float sa, _Float16 hi) {
    return (_Float16)__builtin_fmaf(x, sa, -(float)hi);
}
// one operand -> the 16-bit patterns of its pair
__device__ __forceinline__ void split2h(float x, float sa, unsigned& h, unsigned& l) {
    const _Float16 hi = pair_hi(x, sa);
    h = __builtin_bit_cast(unsigned short, hi);
    l = __builtin_bit_cast(unsigned short, pair_lo(x, sa, hi));
}

// Two packers, one per instruction form (callers keep the form they were scheduled
// with). 8 f32 -> two packed 16-B planes, element pairs built in half2 registers
// (v_fma_mixlo / v_fma_mixhi write the halves in place: no shifts or ORs):
__device__ __forceinline__ void split_pair8(const float (&e)[8], float sa, u32x4& H, u32x4& L) {
    unsigned hv[4], lv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        half2_t h, l;
        h[0] = pair_hi(e[2 * j], sa);
        h[1] = pair_hi(e[2 * j + 1], sa);
        l[0] = pair_lo(e[2 * j], sa, h[0]);
        l[1] = pair_lo(e[2 * j + 1], sa, h[1]);
        hv[j] = __builtin_bit_cast(unsigned, h);
        lv[j] = __builtin_bit_cast(unsigned, l);
    }
    H = u32x4{hv[0], hv[1], hv[2], hv[3]};
    L = u32x4{lv[0], lv[1], lv[2], lv[3]};
}
// ... and the 16-bit patterns packed by shifts and ORs (block32.hip): 8 f32 already in
// registers as two u32x4 -> planes o[0] = hi, o[1] = lo; 4 f32 -> 8 B per plane
__device__ __forceinline__ void split_pair8_or(const u32x4& a, const u32x4& b, float sa, u32x4 (&o)[2]) {
    unsigned h[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split2h(__uint_as_float(j < 4 ? a[j] : b[j - 4]), sa, h[j], l[j]);
    o[0] = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    o[1] = u32x4{l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
}
__device__ __forceinline__ void split_pair4_or(const float (&v)[4], float sa, u32x2& hi, u32x2& lo) {
    unsigned h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split2h(v[j], sa, h[j], l[j]);
    hi = u32x2{h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
    lo = u32x2{l[0] | (l[1] << 16), l[2] | (l[3] << 16)};
}

template <int NA, int NB>
__device__ __forceinline__ f32x4_t mfma_pair(const u32x4 (&a)[NA], const u32x4 (&b)[NB], f32x4_t acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a[1]), __builtin_bit_cast(f16x8_t, b[0]),
                                                 acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a[0]), __builtin_bit_cast(f16x8_t, b[1]),
                                                 acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a[0]), __builtin_bit_cast(f16x8_t, b[0]),
                                                 acc, 0, 0, 0);
    return acc;
}
// The same three products in the same order with the operands exchanged: the MFMA
// computes D^T (rows = weight rows / output channels, columns = pixels), so a lane's
// accumulator holds 4 consecutive channels of one pixel (register epilogue, TR tiles)
template <int NA, int NB>
__device__ __forceinline__ f32x4_t mfma_pair_tr(const u32x4 (&a)[NA], const u32x4 (&b)[NB], f32x4_t acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, b[0]), __builtin_bit_cast(f16x8_t, a[1]),
                                                 acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, b[1]), __builtin_bit_cast(f16x8_t, a[0]),
                                                 acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, b[0]), __builtin_bit_cast(f16x8_t, a[0]),
                                                 acc, 0, 0, 0);
    return acc;
}

// ---- Per-frame running max |y| into the output's slots ---------------------------
// (non-negative floats order as their bit patterns; NaNs are ignored). A lane folds
// its outputs into (frame, max) and flushes on a frame change (rows only ascend, so
// rarely); at the end the wave merges the lanes of its lowest frame into one atomic.
struct AmaxTrack {
    int b = -1;
    float m = 0.f;
    __device__ __forceinline__ void add(unsigned* slot, int fb, float v) {
        if (fb != b) {
            if (b >= 0 && m > 0.f) atomicMax(slot + b, __float_as_uint(m));
            b = fb;
            m = 0.f;
        }
        m = fmaxf(m, v);
    }
    __device__ __forceinline__ void publish(unsigned* slot) {
        int lo = b >= 0 ? b : 0x7fffffff;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
        float v = (b == lo) ? m : 0.f;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
        if ((threadIdx.x & 63) == 0 && lo != 0x7fffffff && v > 0.f) atomicMax(slot + lo, __float_as_uint(v));
        if (b >= 0 && b != lo && m > 0.f) atomicMax(slot + b, __float_as_uint(m));
    }
};

// Workgroup-local form for the conv kernels (one launch touches every frame, so
// per-lane global atomics would serialise on 64 addresses): every lane of a wave
// calls amax_lds_add convergently with its output's frame (-1: none) and max |y|;
// the wave merges its lowest frame into one LDS atomic (other frames: rare, per
// lane), and amax_lds_flush moves the workgroup's nonzero slots to global.
__device__ __forceinline__ void amax_lds_add(unsigned* s, int fb, float v) {
    int lo = fb >= 0 ? fb : 0x7fffffff;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
    if (lo == 0x7fffffff) return;                     // wave-uniform
    float m = (fb == lo) ? v : 0.f;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(s + lo, __float_as_uint(m));
    if (fb >= 0 && fb != lo && v > 0.f) atomicMax(s + fb, __float_as_uint(v));
}

__device__ __forceinline__ void amax_lds_flush(const unsigned* s, unsigned* g, int nframes) {
    for (int f = threadIdx.x; f < nframes; f += blockDim.x)
        if (s[f]) atomicMax(g + f, s[f]);
}

// ---- Letterbox bands (BandArgs in vd_common.h) --------------------------
// The conditions frame f's band tiles of this op are computed under in this call: the
// host epoch and the scale exponents of the band ops' inputs up to this op. The slots
// behind `chain` are final when the op starts (their producers ran earlier on the stream).
__device__ __forceinline__ unsigned long long band_tag(const BandArgs& d, int f) {
    unsigned long long t = (unsigned long long)d.epoch << 32;
    for (int i = 0; i < d.nchain; ++i)
        t |= (unsigned long long)((act_scale_exp_of(__uint_as_float(d.chain[i][f])) + 128) & 0xff) << (8 * i);
    return t;
}

// The launch's live tiles. A frame whose tag matches runs its tile rows [lo, hi) only;
// s_pre[f] (B + 1 entries, LDS) = live tiles of the frames before f. Called by the whole
// workgroup; the tags are not written by any kernel of the forward, so every workgroup
// (and every launch of the op) decides alike. Workgroup 0 folds the kept band tiles'
// maximum into the output's slots.
__device__ __forceinline__ void band_prefix(const BandArgs& d, int B, int tpf, int band_tiles, int* s_pre,
                                            unsigned* ymax) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        int carry = 0;
        for (int base = 0; base < B; base += 64) {
            const int f = base + lane;
            int c = 0;
            if (f < B) {
                const bool keep = d.tag[f] == band_tag(d, f);
                c = keep ? tpf - band_tiles : tpf;
                if (keep && blockIdx.x == 0 && ymax && d.bmax[f]) atomicMax(ymax + f, d.bmax[f]);
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(c, o);
                if (lane >= o) c += v;
            }
            if (f < B) s_pre[f + 1] = carry + c;
            carry += __shfl(c, 63);
        }
        if (lane == 0) s_pre[0] = 0;
    }
    __syncthreads();
}

// A wave's position in s_pre (wave-uniform): live tile t -> frame b and tile r0 of the frame.
struct BandWalk {
    int cur, base, next;
    __device__ __forceinline__ void init(const int* s_pre) {
        cur = 0;
        base = 0;
        next = __builtin_amdgcn_readfirstlane(s_pre[1]);
    }
    __device__ __forceinline__ void at(const int* s_pre, int tpf, int lo_tiles, int t, int& b, int& r0) {
        while (t >= next) {
            ++cur;
            base = next;
            next = __builtin_amdgcn_readfirstlane(s_pre[cur + 1]);
        }
        while (t < base) {
            --cur;
            next = base;
            base = __builtin_amdgcn_readfirstlane(s_pre[cur]);
        }
        b = cur;
        r0 = t - base + (next - base != tpf ? lo_tiles : 0);
    }
};

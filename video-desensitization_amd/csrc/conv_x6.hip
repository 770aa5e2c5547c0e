// conv_x6.hip — fp32 convolution on the 16-bit matrix cores by operand decomposition
// (VD_PREC_FP32). Three forms, template parameter TERMS:
//   2  fp16 pairs, the default (option f32_split = 2): activations scaled per frame by
//      a power of two, both operands split into fp16 hi / lo, three products on
//      v_mfma_f32_16x16x32_f16. The contract (scale, split, product order) is
//      vd_kernel.h's; the weights' side is vd_pack_x3h below.
//   1  the same pair weights on inputs exact in fp16 (the integer-valued stem canvases,
//      ConvArgs::x_exact): one A plane, two products.
//   3  exact bf16 triples (f32_split = 1), six products on v_mfma_f32_16x16x32_bf16:
//
// Every f32 operand is split EXACTLY into three bf16 terms, x = x0 + x1 + x2
// (x0 = the top 8 significand bits, x1 the next 8, x2 the last 8: each residual
// is exact in f32 and fits the next term), and the product is the sum of the six
// cross terms with i + j <= 2:
//     a*b ~= a0 b0 + a0 b1 + a1 b0 + a0 b2 + a1 b1 + a2 b0
// Each term is an exact 16-bit product accumulated in f32; the dropped terms
// (a1 b2, a2 b1, a2 b2) are below 2^-22 |ab|, so a K-long dot product carries the
// same error as an f32 fma chain (measured in tests/test_gpu_kernels.py against
// float64: error at the level of the exact-f32 MFMA path). Six bf16 MFMAs (96 cycles
// per 16x16x32 block) replace eight exact-f32 v_mfma_f32_16x16x4_f32 (256 cycles):
// 2.67x the f32 MFMA rate; the pair form halves that again.
//
// Same conv contract as conv.hip (NHWC f32 activations, K = (kh, kw, c) with c
// fastest, fused BN scale/shift + residual + activation, channel-sliced
// in/out); replaces the same reference layers (retinaface.py:71-92 via
// torchvision resnet50 [ext], layers.py:10-114, the YOLOv8n convs).
//
// Schedule of the GEMM tiles (conv_x6_kernel; shapes and LDS sizes: X6Shape, conv_x6.h):
// K tile 32, P operand planes of 64-B rows per LDS stage (pairs 2, triples 3).
//   * A (f32 pixels): global -> registers (two 16-B loads per 8 k), split into P 16-B
//     chunks; loads for tile t+2 are issued while tile t computes.
//   * B (weights): split once at weight load into [Npad][Kpad/32][P][32]; LDS-DMA
//     straight into the stage (source-side swizzle).
//   * 64-B LDS rows, chunk' = chunk ^ (((row >> 3) & 1) * 3) (swz64): conflict-free
//     ds_read_b128 fragment reads for the 16-row MFMA operand pattern.
//
// Halo tiles: conv_x6_halo.hip; streaming 1x1 / TAPS / dual kernels: conv_x6_stream.hip; shared pieces: conv_x6.h.
#include "vd_kernel.h"
#include "conv_x6.h"
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstring>

namespace {

template <int BM, int BN, int NT, int NST, int TERMS, int MF, bool TR = false, bool PF = false>
// MF: MFMA form of the fp16 pairs, 16 = 16x16x32, 32 = 32x32x16 (option x6_mf32)
// 8 waves: two workgroups' worth of waves per SIMD pair (256 VGPRs each); 4 waves (one
// per SIMD, 128 x 128 wave tiles): the whole 512-register file per wave, the
// accumulators in AGPRs
// TR: transposed accumulators (D^T, weight rows permuted by x6_tr_row) and the register
// epilogue x6_epilogue_tr; fp16 pairs on the 16x16x32 form only
__global__ __launch_bounds__(NT, NT == 256 && BM == 256 ? 1 : 2) void conv_x6_kernel(ConvArgs a) {
    static_assert(MF == 16 || (MF == 32 && TERMS == 2), "32x32x16 form: fp16 pairs only");
    static_assert(!TR || (MF == 16 && TERMS == 2), "TR tiles: fp16 pairs on 16x16x32");
    using S = X6Shape<BM, BN, NT, NST, TERMS, MF>;
    constexpr int NA = 2;   // A register sets (K tiles of A loads in flight: NA - 1 besides the one being split)
    constexpr int STAGE = S::STAGE, PL_A = S::PL_A, PL_B = S::PL_B, TM = S::TM, TN = S::TN, WAVES = S::WAVES;
    constexpr int AROWS = S::AROWS, AIT = S::AITEMS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / S::WAVES_N, wn = wid % S::WAVES_N;

    // XCD-aware bijective remap (blocks b, b+8, ... share an XCD)
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    const int tn = wg % a.ntiles_n, tm = wg / a.ntiles_n;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- A staging: thread = (row, k-pair) items; item i: row = (tid >> 2) + AROWS i, pair = tid & 3 (k 8p..8p+7)
    const int apair = tid & 3, arow = tid >> 2;
    const int ohw = a.yh * a.yw;
    int pix0[AIT];                                  // element offsets (xbytes < 2^31: vd_conv_x6_ok)
    int iy0[AIT], ix0[AIT];
    float sa[AIT];                                  // fp16 pair: the row's frame scale 2^k
#pragma unroll
    for (int i = 0; i < AIT; ++i) {
        sa[i] = 1.f;
        const int m = m0 + arow + AROWS * i;
        if (m < a.M) {
            const int b = m / ohw, rem = m - b * ohw;
            const int oy = rem / a.yw, ox = rem - oy * a.yw;
            iy0[i] = oy * a.stride - a.pad;
            ix0[i] = ox * a.stride - a.pad;
            pix0[i] = ((b * a.xh + iy0[i]) * a.xw + ix0[i]) * a.ldx + a.xcoff;
            if constexpr (TERMS != 3) sa[i] = __builtin_ldexpf(1.f, act_scale_exp(a, b));
        } else {
            iy0[i] = -(1 << 28); ix0[i] = 0; pix0[i] = 0;
        }
    }
    const int tap_dy = a.xw * a.ldx;
    const int nk = a.kpad / KT;
    // A through a buffer descriptor: 32-bit byte offsets, and an offset past
    // num_records returns zeros (conv padding, K padding) without a select on the
    // loaded value -- a select would force a wait right at the load
    const long xbytes = (long)a.B * a.xh * a.xw * a.ldx * 4;
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)xbytes, 0x00020000);
    // 1x1 convs without K padding (option x6_one): K tile kt of a row is bytes
    // [128 kt, 128 kt + 128) past the row's pixel, so each load is the row's byte offset
    // (rows past M: out of range) plus a scalar offset -- no per-tile tap stepping
    const bool one = a.one && a.kh == 1 && a.kw == 1 && a.pad == 0 &&
                     a.kpad == a.cin_pad && a.cin_pad % KT == 0;
    if (one) {
#pragma unroll
        for (int i = 0; i < AIT; ++i)
            pix0[i] = m0 + arow + AROWS * i < a.M ? pix0[i] * 4 + apair * 32 : (int)0x80000000;
    }
    int lk = 0;                                     // K tiles loaded so far (one: the scalar offset)
    // NA register sets of A (8 f32 of each of AIT rows): tile t lives in set t % NA,
    // loaded NA iterations before it is split into LDS
    u32x4 ra[NA][AIT][2];                           // [set][item][half]
    // per half h: the (dy, dx, c) of this thread's 4-channel chunk kt*8 + 2*apair + h,
    // advanced by 32 channels per load_a call (tiles are loaded in order): no
    // divisions and no branches in the load path
    int tdy[2], tdx[2], tc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ch0 = (apair * 2 + h) * 4;
        const int t = ch0 / a.cin_pad;
        tc[h] = ch0 - t * a.cin_pad;
        tdy[h] = t / a.kw;
        tdx[h] = t - tdy[h] * a.kw;
    }
    auto load_a_any = [&](u32x4 (&r)[AIT][2]) {
        if (one) {
            const int so = lk * (KT * 4);
#pragma unroll
            for (int i = 0; i < AIT; ++i) {
                r[i][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, pix0[i], so, 0));
                r[i][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, pix0[i] + 16, so, 0));
            }
            ++lk;
            return;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // a chunk past the last tap (K padding) is pushed off the image rows, so
            // one unsigned compare rejects it (selects only: no divergent branch)
            const int dyk = tdy[h] < a.kh ? tdy[h] : (1 << 28);
            const int toff = tdy[h] * tap_dy + tdx[h] * a.ldx + tc[h];
#pragma unroll
            for (int i = 0; i < AIT; ++i) {
                const unsigned iy = (unsigned)(iy0[i] + dyk), ix = (unsigned)(ix0[i] + tdx[h]);
                const bool ok = (iy < (unsigned)a.xh) & (ix < (unsigned)a.xw);
                const unsigned off = ok ? (unsigned)(pix0[i] + toff) * 4u : 0x80000000u;
                r[i][h] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)off, 0, 0));
            }
            tc[h] += KT;
            if (a.cin_pad >= KT) {                  // at most one tap step per tile: selects only
                const bool wrap = tc[h] >= a.cin_pad;
                tc[h] -= wrap ? a.cin_pad : 0;
                tdx[h] += wrap ? 1 : 0;
                const bool wrap2 = tdx[h] >= a.kw;
                tdx[h] -= wrap2 ? a.kw : 0;
                tdy[h] += wrap2 ? 1 : 0;
            } else {
                while (tc[h] >= a.cin_pad) { tc[h] -= a.cin_pad; ++tdx[h]; }
                while (tdx[h] >= a.kw) { tdx[h] -= a.kw; ++tdy[h]; }
            }
        }
    };
    auto store_item = [&](int st, const u32x4 (&r)[AIT][2], int i) {
        char* A = smem + st * STAGE;
        float e[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = __uint_as_float(r[i][0][j]);
            e[4 + j] = __uint_as_float(r[i][1][j]);
        }
        u32x4 o[3];
        split_pack<TERMS>(e, sa[i], o);
        const int off = swz64(arow + AROWS * i, apair);
#pragma unroll
        for (int p = 0; p < S::TA; ++p) *(u32x4*)(A + p * PL_A + off) = o[p];
    };

    // ---- B: LDS-DMA, one instruction = 1 KB = 16 rows of one plane; NDMA per tile,
    // instruction j on wave j % WAVES: plane j / (BN/16), rows 16 * (j % (BN/16)) .. +15
    constexpr int RB = BN / 16;                        // 16-row blocks per plane
    constexpr int NDMA = S::NDMA;
    const int my_dma = NDMA / WAVES + (wid < NDMA % WAVES ? 1 : 0);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7fffffff, 0x00020000);
    auto dma_b = [&](int kt, int st) {
        char* Bs = smem + st * STAGE + S::TA * PL_A;
#pragma unroll
        for (int q = 0; q < (NDMA + WAVES - 1) / WAVES; ++q) {
            const int j = wid + WAVES * q;
            if (NDMA % WAVES == 0 || j < NDMA) {
                const int p = j / RB, r0 = (j % RB) * 16;
                const int row = r0 + (lane >> 2), slot = lane & 3;
                const int chunk = slot ^ (((row >> 3) & 1) * 3);
                const int wrow = TR ? x6_tr_row(row) : row;
                const int ktc = kt < nk ? kt : nk - 1;     // one-barrier tail: the last tile again (a scalar min)
                const unsigned off = (unsigned)((((long)(n0 + wrow) * nk + ktc) * S::TB + p) * 64 + chunk * 16);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_void_t*)(Bs + p * PL_B + r0 * 64), 16, off, 0,
                                                         0, 0);
            }
        }
    };

    using AccT = typename std::conditional<MF == 32, f32x16_t, f32x4_t>::type;
    AccT acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = AccT{};
    if (a.ymax)   // beyond the stages / epilogue image; ordered before use by the main loop's barriers
        for (int f = tid; f < a.B; f += NT) ((unsigned*)(smem + S::LDS))[f] = 0u;

    // one K tile from stage st; the split + LDS write of the next tile's A items are
    // interleaved with the MFMA rows (VALU work beside the matrix cores)
    auto compute = [&](int st, bool split_next, int st_next, const u32x4 (&rn)[AIT][2]) {
        const char* A = smem + st * STAGE;
        const char* Bs = A + S::TA * PL_A;
        const int ch = lane >> 4;
        if constexpr (MF == 32) {   // two K steps of 16: lane l reads row l % 32, 16-B chunk 2 s + l / 32
            const int r32 = lane & 31, c32 = lane >> 5;
#pragma unroll
            for (int sk = 0; sk < 2; ++sk) {
                u32x4 af[TM][3];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        af[i][p] = *(const u32x4*)(A + p * PL_A + swz64(wm * S::WTM + i * 32 + r32, 2 * sk + c32));
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    u32x4 bf[3];
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        bf[p] = *(const u32x4*)(Bs + p * PL_B + swz64(wn * S::WTN + j * 32 + r32, 2 * sk + c32));
#pragma unroll
                    for (int i = 0; i < TM; ++i) acc[i][j] = mfma_pair32(af[i], bf, acc[i][j]);
#pragma unroll
                    for (int q = 0; q < AIT; ++q)
                        if (split_next && sk == q * 2 / AIT && j == (q * 2 % AIT) * TN / AIT) store_item(st_next, rn, q);
                }
            }
        } else if constexpr (TN > TM && PF) {
            // PF (option x6_gemm_pf): B fragments of column block j + 1 read before the MFMAs
            // of block j (two buffers), pinned by scheduling groups (as the halo tiles)
            u32x4 af[TM][3], bq[2][3];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int p = 0; p < S::TA; ++p)
                    af[i][p] = *(const u32x4*)(A + p * PL_A + swz64(wm * S::WTM + i * 16 + (lane & 15), ch));
#pragma unroll
            for (int p = 0; p < S::TB; ++p) bq[0][p] = *(const u32x4*)(Bs + p * PL_B + swz64(wn * S::WTN + (lane & 15), ch));
            __builtin_amdgcn_sched_group_barrier(0x0100, TM * S::TA + S::TB, 0);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (j + 1 < TN) {
#pragma unroll
                    for (int p = 0; p < S::TB; ++p)
                        bq[(j + 1) & 1][p] = *(const u32x4*)(Bs + p * PL_B + swz64(wn * S::WTN + (j + 1) * 16 + (lane & 15), ch));
                    __builtin_amdgcn_sched_group_barrier(0x0100, S::TB, 0);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (TR) acc[i][j] = mfma_pair_tr(af[i], bq[j & 1], acc[i][j]);
                    else acc[i][j] = mfma_terms<TERMS>(af[i], bq[j & 1], acc[i][j]);
                }
                __builtin_amdgcn_sched_group_barrier(0x0008, (TERMS == 3 ? 6 : TERMS == 2 ? 3 : 2) * TM, 0);
#pragma unroll
                for (int q = 0; q < AIT; ++q)
                    if (split_next && j == q * TN / AIT) store_item(st_next, rn, q);
            }
        } else if constexpr (TN > TM) {   // wide wave tile: all A fragments resident, B fragments streamed
            u32x4 af[TM][3];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int p = 0; p < S::TA; ++p)
                    af[i][p] = *(const u32x4*)(A + p * PL_A + swz64(wm * S::WTM + i * 16 + (lane & 15), ch));
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                u32x4 bf[3];
#pragma unroll
                for (int p = 0; p < S::TB; ++p)
                    bf[p] = *(const u32x4*)(Bs + p * PL_B + swz64(wn * S::WTN + j * 16 + (lane & 15), ch));
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (TR) acc[i][j] = mfma_pair_tr(af[i], bf, acc[i][j]);
                    else acc[i][j] = mfma_terms<TERMS>(af[i], bf, acc[i][j]);
                }
#pragma unroll
                for (int q = 0; q < AIT; ++q)
                    if (split_next && j == q * TN / AIT) store_item(st_next, rn, q);
            }
        } else {
            u32x4 bf[TN][3];
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int p = 0; p < S::TB; ++p)
                    bf[j][p] = *(const u32x4*)(Bs + p * PL_B + swz64(wn * S::WTN + j * 16 + (lane & 15), ch));
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                u32x4 af[3];
#pragma unroll
                for (int p = 0; p < S::TA; ++p)
                    af[p] = *(const u32x4*)(A + p * PL_A + swz64(wm * S::WTM + i * 16 + (lane & 15), ch));
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (TR) acc[i][j] = mfma_pair_tr(af, bf[j], acc[i][j]);
                    else acc[i][j] = mfma_terms<TERMS>(af, bf[j], acc[i][j]);
                }
                if constexpr (AIT == 2) {
                    if (split_next && i == 0) store_item(st_next, rn, 0);
                    if (split_next && i == (TM > 2 ? 2 : 1)) store_item(st_next, rn, 1);
                } else {
#pragma unroll
                    for (int q = 0; q < AIT; ++q)
                        if (split_next && i == q * TM / AIT) store_item(st_next, rn, q);
                }
            }
        }
    };

    if constexpr (NST == 2) {
    // ---- main loop, two forms. A(t) lives in register set t % NA.
    // The general loop (every KxK conv; 1x1 convs with option x6_gemm_uni = 0 or on tiles
    // without whole DMA rounds): two barriers per K tile. Per thread VMEM issue order at
    // the end of iteration t: A(t+1+NA) loads (2 AIT, into the set A(t+1) just left),
    // B(t+2) DMA (my_dma); the prologue issues A(0) (split at once), A(1..NA-1), B(0),
    // A(NA), B(1), i.e. the ends of iterations -2 and -1. At the top of iteration t the
    // ops younger than B(t) are those of iteration t-1's end, and A(t+1) is older than
    // B(t), so both retire at vmcnt(2 AIT + my_dma) (fewer when the tail issued less).
    auto main_loop = [&]() {
        load_a_any(ra[0]);
#pragma unroll
        for (int q = 0; q < AIT; ++q) store_item(0, ra[0], q);
#pragma unroll
        for (int j = 1; j < NA; ++j)
            if (j < nk) load_a_any(ra[j]);
        dma_b(0, 0);
        if (NA < nk) load_a_any(ra[0]);
        if (nk > 1) dma_b(1, 1);
        auto iter = [&](int kt, const u32x4 (&rnext)[AIT][2], u32x4 (&rfree)[AIT][2]) {
            if constexpr (S::NDMA % WAVES == 0) {   // immediates: no runtime wait_vm branch tree
                constexpr int MYD = S::NDMA / WAVES;
                if (kt + NA < nk) wait_vm_k<2 * AIT + MYD>();
                else if (kt + 1 < nk) wait_vm_k<MYD>();
                else wait_vm_k<0>();
            } else {
                wait_vm((kt + NA < nk ? 2 * AIT : 0) + (kt + 1 < nk ? my_dma : 0));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this thread's A(kt) ds_writes
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            compute(kt & 1, kt + 1 < nk, (kt + 1) & 1, rnext);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                        // everyone done reading stage kt & 1
            asm volatile("" ::: "memory");
            if (kt + 1 + NA < nk) load_a_any(rfree);              // A(kt+1+NA) into the set A(kt+1) just left
            if (kt + 2 < nk) dma_b(kt + 2, kt & 1);
        };
        // Raw barriers with counted waits: __syncthreads() would add vmcnt(0) and drain
        // the prefetch. Unrolled by NA so the register sets are indexed statically.
        for (int kt = 0; kt < nk; kt += NA) {
#pragma unroll
            for (int u = 0; u < NA; ++u)
                if (kt + u < nk) iter(kt + u, ra[(u + 1) % NA], ra[(u + 1) % NA]);
        }
    };
    // The one-barrier loop (1x1 convs, `one`; option x6_gemm_uni = 2, default; tiles with
    // whole DMA rounds): every iteration issues the same loads and DMA (past nk: the last
    // tile again, L2 hits), branch-free, and the loop runs whole rounds of NA iterations and
    // a tail after it, so the compiler's own waits on the A registers count every younger op
    // -- with the refills under `if`s (and the runtime `one` branch) it assumed none and
    // waited for the NEXT tile's loads (just issued) in the middle of the MFMAs. B(kt+1)'s DMA and
    // A(kt+NA)'s loads are issued right after tile kt's barrier (stage (kt+1) & 1 was last
    // read by tile kt-1, which every wave has finished there), so the barrier after the
    // MFMAs goes.
    auto main_loop_1b = [&]() {
        auto load_a = [&](u32x4 (&r)[AIT][2]) {                  // no tap stepping, no branch
            const int so = (lk < nk ? lk : nk - 1) * (KT * 4);
#pragma unroll
            for (int i = 0; i < AIT; ++i) {
                r[i][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, pix0[i], so, 0));
                r[i][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, pix0[i] + 16, so, 0));
            }
            ++lk;
        };
        load_a(ra[0]);
#pragma unroll
        for (int q = 0; q < AIT; ++q) store_item(0, ra[0], q);
        // VMEM order: A(1..NA-2), B(0), A(NA-1) | per tile kt after its barrier: B(kt+1),
        // A(kt+NA). Younger than B(kt) at the top of kt: A(kt-1+NA) only.
#pragma unroll
        for (int j = 1; j < NA - 1; ++j) load_a(ra[j]);
        dma_b(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        load_a(ra[NA - 1]);
        auto iterb = [&](int kt, const u32x4 (&rnext)[AIT][2], u32x4 (&rfree)[AIT][2]) {
            wait_vm_k<2 * AIT>();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this thread's A(kt) ds_writes
            __builtin_amdgcn_s_barrier();                        // B(kt), A(kt) visible; tile kt-1 done
            asm volatile("" ::: "memory");
            dma_b(kt + 1, (kt + 1) & 1);
            // the wait above counts the A loads as the youngest ops: the scheduler may not
            // interleave them with the DMA (it did, and a DMA left in flight raced the reads)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" ::: "memory");
            load_a(rfree);                                       // A(kt+NA) into the set A(kt) left
            compute(kt & 1, kt + 1 < nk, (kt + 1) & 1, rnext);
        };
        int kt = 0;
        for (; kt + NA <= nk; kt += NA) {
#pragma unroll
            for (int u = 0; u < NA; ++u) iterb(kt + u, ra[(u + 1) % NA], ra[u]);
        }
#pragma unroll
        for (int u = 0; u < NA - 1; ++u)
            if (kt + u < nk) iterb(kt + u, ra[(u + 1) % NA], ra[u]);
        wait_vm_k<0>();                                          // the tail's DMA / loads (past nk)
    };
    if constexpr (S::NDMA % WAVES == 0) {
        if (one && a.gemm_1b) main_loop_1b();
        else main_loop();
    } else {
        main_loop();
    }
    } else {
    // ---- one LDS stage: per tile, B(kt) DMA and the split A(kt) write, then
    // compute; A(kt+1)'s loads run under it (registers), B waits for the stage
    load_a_any(ra[0]);
    auto iter1 = [&](int kt, const u32x4 (&rcur)[AIT][2], u32x4 (&rnext)[AIT][2]) {
        dma_b(kt, 0);
#pragma unroll
        for (int q = 0; q < AIT; ++q) store_item(0, rcur, q);   // compiler waits for A(kt)'s loads
        if (kt + 1 < nk) load_a_any(rnext);
        if (kt + 1 < nk) wait_vm_k<2 * AIT>();                // B(kt) landed (older than A(kt+1))
        else wait_vm_k<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        compute(0, false, 0, rcur);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                        // the stage is free again
        asm volatile("" ::: "memory");
    };
    for (int kt = 0; kt < nk; kt += 2) {
        iter1(kt, ra[0], ra[1]);
        if (kt + 1 < nk) iter1(kt + 1, ra[1], ra[0]);
    }
    }
    if constexpr (TR) {
        if (a.dbg & 1) {                               // timing-only (x6_dbg bit 0): main loop only
            if (acc[0][0][0] == 1234.5f) ((float*)a.y)[tid] = 1.f;
            return;
        }
        x6_epilogue_tr<S>(a, acc, m0, n0, wm, wn, lane, (unsigned*)(smem + S::LDS));
    } else {
        __syncthreads();
        x6_epilogue<S, MF>(a, acc, m0, n0, wm, wn, tid, lane, smem, S::LDS);
    }
}

__global__ void amax_merge_kernel(unsigned* dst, const unsigned* src, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = max(dst[i], src[i]);
}

}  // namespace

// max-pool / upsample outputs of the fp16-pair plan: the output's per-frame range is
// within the input's (plate_net.cpp SPPF / Upsample, the f32 face stem's pool)
hipError_t vd_launch_amax_merge(unsigned* dst, const unsigned* src, int n, hipStream_t s) {
    hipLaunchKernelGGL(amax_merge_kernel, dim3((n + 63) / 64), dim3(64), 0, s, dst, src, n);
    return hipGetLastError();
}

// Eligible: f32 activations with Cin padded to 4, K padded to 32, split weights present.
bool vd_conv_x6_ok(const ConvArgs& a) {
    const double xbytes = (double)a.B * a.xh * a.xw * a.ldx * 4;   // 32-bit buffer offsets
    return a.wx3 != nullptr && (a.kpad % KT) == 0 && (a.cin_pad % 4) == 0 && ((a.ldx | a.xcoff) & 3) == 0 &&
           xbytes < 2147483647.0;
}

template <int BM, int BN, int NT, int NST, int TERMS, int MF = 16, bool TR = false, bool PF = false>
static hipError_t launch_x6(const ConvArgs& a0, hipStream_t s) {
    using S = X6Shape<BM, BN, NT, NST, TERMS, MF>;
    if constexpr (!PF && MF == 16 && NST == 2 && S::TN > S::TM) {
        // option x6_gemm_pf: the wide-wave tiles with pipelined B-fragment reads
        if (a0.tune->x6_gemm_pf) return launch_x6<BM, BN, NT, NST, TERMS, MF, TR, true>(a0, s);
    }
    static const bool attr = [] {
        (void)hipFuncSetAttribute((const void*)conv_x6_kernel<BM, BN, NT, NST, TERMS, MF, TR, PF>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS + 4 * kAmaxFrames);
        return true;
    }();
    (void)attr;
    ConvArgs a = a0;
    a.w = a.wx3;                                   // the kernel reads the split planes
    a.ntiles_n = (a.cout + BN - 1) / BN;
    const int mt = (a.M + BM - 1) / BM;
    const int lds = S::LDS + (a.ymax ? 4 * a.B : 0);
    vd_conv_fam_set(TR ? VD_FAM_X6_TR : VD_FAM_X6_TILE);
    hipLaunchKernelGGL((conv_x6_kernel<BM, BN, NT, NST, TERMS, MF, TR, PF>), dim3(mt * a.ntiles_n), dim3(NT), lds, s, a);
    return hipGetLastError();
}

// TR tiles (option x6_gemm1x1, default): the 1x1 convs the streaming form does not take
// (K >= 512, strided downsamples) on conv_x6_kernel with D^T accumulators and the
// register epilogue (x6_epilogue_tr). Same tiles and products as the untransposed form,
// bit-identical results (tests/test_gpu_kernels.py); the epilogue skips the LDS round
// trip and its two barriers per pass (tools/x6bench, B = 64: layer4 conv3 334 -> 304 us,
// layer3.0 downsample 528 -> 472, layer3 conv1 263 -> 243, FPN output1 553 -> 512).
// Measured and not kept: the pixel operand loaded straight into registers by the two
// waves of its row band (no LDS image, one barrier per K tile with three weight
// stages): its main loop ran 5-10 % slower than the LDS-staged one (layer3 conv1
// 215 -> 235 us without epilogue). Needs 8-channel 16-B output / residual vectors.
static bool x6_tr_ok(const ConvArgs& a) {
    if (a.kh != 1 || a.kw != 1 || a.pad != 0 || a.cout % 128 || !tr_bytes_ok(a)) return false;
    if ((a.ldy | a.ycoff) & 7) return false;
    return a.res_mode == VD_RES_NONE || !((a.res_ld | a.res_coff) & 7);
}

static hipError_t launch_tr(const ConvArgs& a, hipStream_t s) {
    const long t256 = (long)((a.M + 255) / 256) * (a.cout / 256);
    // (Measured and not kept, round 6: Cout >= 512 1x1 layers with K <= 512-2048 on the
    // 128 x 128 tile at two workgroups per CU -- level to 8 % slower, tools/runs/r06y.sh)
    if (a.cout % 256 == 0 && t256 >= 192) return launch_x6<256, 256, 512, 2, 2, 16, true>(a, s);
    if (a.cout == 128 && a.tune->x6_mid && a.kpad <= a.tune->x6_mid) return launch_x6<128, 128, 256, 2, 2, 16, true>(a, s);
    return launch_x6<256, 128, 512, 2, 2, 16, true>(a, s);
}

// N tile follows Cout (weights are packed with Npad a multiple of 128, so every
// tile's rows exist): 32 for the heads, 64 for the 64-channel convs, else 128.
// The small single-stage tile takes the narrow (N <= 64) layers with K <= 256 or
// a grid of fewer than 512 big tiles (measured: stem 2.16 -> 1.87 ms, layer1 conv1
// 640 -> 580 us, SSH level 1/2 and heads 15-25 % faster); at N = 128 it measured
// 30-45 % slower than the big tile (one wave per SIMD at 198 VGPRs) and is not used.
template <int TERMS>
static hipError_t launch_terms(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    if (TERMS == 2) a.scale = a.scale_x;              // the fp16 pair's per-channel rescaled BN scale
    hipError_t err = hipSuccess;
    if (vd_launch_x6_stream(a, TERMS, s, &err)) return err;
    if constexpr (TERMS == 2) {
        if (a.tune->x6_gemm1x1 && x6_tr_ok(a)) return launch_tr(a, s);
    }
    const int bn = a.cout <= 32 ? 32 : (a.cout <= 64 ? 64 : 128);
    const long big_tiles = (long)((a.M + 255) / 256) * ((a.cout + bn - 1) / bn);
    const int small_k = a.tune->x6_small_k, small_tiles = a.tune->x6_small_tiles, small_k2 = a.tune->x6_small_k2;
    const bool force_small = small_k >= (1 << 30);       // test hook: every layer on the small tile
    // fp16 pairs: the 4-wave one-stage tile wins for every N <= 64 layer measured
    // (layer1 conv2 831 -> 603 us, SSH level-0 conv7X7 229 -> 163 us)
    const bool small = force_small || (bn <= 64 && (a.kpad <= (TERMS == 2 ? small_k2 : small_k) ||
                                                    big_tiles < small_tiles));
    if constexpr (TERMS == 2) {   // narrow 3x3 stride-1 layers on the halo form too (two workgroups per CU)
        if (bn <= 64 && a.tune->x6_halo_narrow && vd_x6_halo_ok(a)) return vd_launch_x6_halo(a, bn, s);
    }
    if (small) {
        if constexpr (TERMS == 2) {   // integer-valued canvases (face / plate stems): one A plane, two products
            if (bn == 32 && a.x_exact) return launch_x6<128, 32, 256, 1, 1>(a, s);
            if (bn == 64 && a.x_exact) return launch_x6<128, 64, 256, 1, 1>(a, s);
        }
        if (bn == 32) return launch_x6<128, 32, 256, 1, TERMS>(a, s);
        if (bn == 64) return launch_x6<128, 64, 256, 1, TERMS>(a, s);
        return launch_x6<128, 128, 256, 1, TERMS>(a, s);
    }
    if (bn == 32) return launch_x6<256, 32, 512, 2, TERMS>(a, s);
    if (bn == 64) return launch_x6<256, 64, 512, 2, TERMS>(a, s);
    if constexpr (TERMS == 2) {
        // short-K 1x1 layers (HBM-bound f32 tensors): a 128 x 128 two-stage tile at two
        // workgroups per CU, so one workgroup's epilogue / prologue overlaps the other's
        // main loop, and 4x the tiles of the 256 x 256 form balance the last round
        // (Cout 128 only: layer2 conv1 at K = 512 340 -> 305 us; the Cout 256 layers at
        // K = 512, FPN output1 / layer3.0 conv1, measured 7-13 % slower on it)
        if (a.tune->x6_mid && a.kh == 1 && a.kw == 1 && a.kpad <= a.tune->x6_mid && a.cout == 128)
            return launch_x6<128, 128, 256, 2, TERMS>(a, s);
    }
    if constexpr (TERMS == 2) {   // 64 x 128 wave tiles: 2/3 of the LDS fragment reads per MFMA
        // (layer3/4 and FPN 12-20 % faster than 256 x 128; not below ~200 tiles: FPN output3,
        // 100 tiles, 137 -> 199 us)
        const long t256 = (long)((a.M + 255) / 256) * (a.cout / 256);
        if (a.tune->x6_bn256 && a.cout % 256 == 0 && t256 >= 192) {
            if (vd_x6_halo_ok(a)) return vd_launch_x6_halo(a, 256, s);
            if (a.tune->x6_mf32) return launch_x6<256, 256, 512, 2, TERMS, 32>(a, s);
            return launch_x6<256, 256, 512, 2, TERMS>(a, s);
        }
        // Cout 192 (the fused SSH conv5X5_1 + conv3X3): one 192-wide N tile instead of two
        // 128-wide ones with a quarter of the MFMAs on padding rows (level 0 1716 -> 1264 us,
        // level 1 526 -> 396; not for level 2's 100 tiles: 137 -> 178)
        if (a.tune->x6_bn256 && a.cout == 192 && (a.M + 255) / 256 >= 192) {
            if (vd_x6_halo_ok(a)) return vd_launch_x6_halo(a, 192, s);
            return launch_x6<256, 192, 512, 2, TERMS>(a, s);
        }
        // every eligible layer on the halo form whatever the batch (its K order differs)
        if (vd_x6_halo_ok(a)) return vd_launch_x6_halo(a, 128, s);
        if (a.tune->x6_mf32) return launch_x6<256, 128, 512, 2, TERMS, 32>(a, s);
    }
    return launch_x6<256, 128, 512, 2, TERMS>(a, s);
}

hipError_t vd_launch_conv_x6(const ConvArgs& a0, hipStream_t s) {
    if (!a0.tune) return hipErrorInvalidValue;          // every caller sets it (vd_launch_conv: the defaults)
    ConvArgs a = a0;
    a.one = a.tune->x6_one != 0;
    a.halo_dma = a.tune->x6_halo_dma & 3;
    a.gemm_1b = a.tune->x6_gemm_uni == 2;
    a.halo_1b = a.tune->x6_halo_1b != 0;
    a.dbg = a.tune->x6_dbg & 0x3d;                      // timing-only skips: bits 0 and 2-5
    if (a.grp_co) {   // grouped: the halo form only, one 64-wide N tile per group
        if (a.grp_co != 64 || a.f32_split != 2 || !a.wx3 || !vd_x6_halo_ok(a) || (a.ymax && a.B > kAmaxFrames))
            return hipErrorInvalidValue;
        a.scale = a.scale_x;
        return vd_launch_x6_halo(a, 64, s);
    }
    if (a.x2) {
        if (!vd_conv1x1_x6_dual_ok(a) || (a.ymax && a.B > kAmaxFrames)) return hipErrorInvalidValue;
        return vd_launch_x6_dual(a, s);
    }
    if (a.f32_split == 2) {
        if (!a.scale_x || (a.ymax && a.B > kAmaxFrames)) return hipErrorInvalidValue;
        return launch_terms<2>(a, s);
    }
    ConvArgs b = a;
    b.xmax = nullptr;                                   // the bf16 triple needs no operand scaling
    return launch_terms<3>(b, s);
}

// Host: pack f32 weights [npad][kpad] (k = tap * cin_pad + c) into the split layout
// [npad][kpad / 32][3][32] bf16 (plane 0 = top 8 significand bits; same truncation
// split as the kernel's activations).
static inline unsigned f2u(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static inline float u2f(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }

void vd_pack_x6(const float* w, int npad, int kpad, uint16_t* out) {
    const int nk = kpad / KT;
    for (int n = 0; n < npad; ++n)
        for (int t = 0; t < nk; ++t)
            for (int k = 0; k < KT; ++k) {
                const float x = w[(size_t)n * kpad + t * KT + k];
                const unsigned u = f2u(x);
                const float r1 = x - u2f(u & 0xFFFF0000u);
                const unsigned v = f2u(r1);
                const float r2 = r1 - u2f(v & 0xFFFF0000u);
                uint16_t* o = out + (((size_t)n * nk + t) * 3) * KT + k;
                o[0] = (uint16_t)(u >> 16);
                o[KT] = (uint16_t)(v >> 16);
                o[2 * KT] = (uint16_t)(f2u(r2) >> 16);
            }
}

// Host: the fp16-pair layout [npad][kpad / 32][2][32] fp16 for f32_split = 2: the pair
// contract of vd_kernel.h on the weight rows. Row n is scaled by 2^e[n] so its largest
// |w| lies in [2^14, 2^15) (hi = RNE(w 2^e), lo = RNE(w 2^e - hi)); row_inv[n] = 2^-e[n]
// is folded into the BN scale.
void vd_pack_x3h(const float* w, int npad, int kpad, uint16_t* out, float* row_inv) {
    const int nk = kpad / KT;
    for (int n = 0; n < npad; ++n) {
        float m = 0.f;
        for (int k = 0; k < kpad; ++k) m = std::max(m, std::fabs(w[(size_t)n * kpad + k]));
        int e = 0;
        if (m > 0.f) {
            (void)std::frexp(m, &e);
            e = std::min(100, std::max(-100, 15 - e));
        }
        row_inv[n] = std::ldexp(1.f, -e);
        for (int t = 0; t < nk; ++t)
            for (int k = 0; k < KT; ++k) {
                const float x = std::ldexp(w[(size_t)n * kpad + t * KT + k], e);
                const _Float16 h = (_Float16)x;
                const _Float16 l = (_Float16)(x - (float)h);
                uint16_t* o = out + (((size_t)n * nk + t) * 2) * KT + k;
                std::memcpy(o, &h, 2);
                std::memcpy(o + KT, &l, 2);
            }
    }
}

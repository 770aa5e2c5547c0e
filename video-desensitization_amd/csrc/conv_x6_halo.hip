// conv_x6_halo.hip — the halo tiles of the fp32 plan (fp16 pairs; contract and dispatch: conv_x6.hip)
#include "vd_kernel.h"
#include "conv_x6.h"
#include <algorithm>

namespace {

// 3x3 / stride 1 / pad 1 convs on fp16 pairs with the input split ONCE per 32-channel
// chunk (option x6_halo). The 256 output rows of a tile are 256 consecutive pixels
// m0..m0+255 (any frames); tap (dy, dx) of row r reads input pixel m + dy W + dx, so
// all nine taps of a chunk read inside the linear "halo" m0 - W - 1 .. m0 + 256 + W.
// The K loop runs chunk-major (chunk c, then its nine taps): the halo's f32 rows of
// chunk c are loaded once (registers, during chunk c-1's taps), split into fp16
// hi / lo planes once and written to LDS; each tap's A fragments are then halo rows
// shifted by dy W + dx, a padded tap (off the frame's rows or columns, or past M)
// reads a zero row instead -- the per-lane row address carries the padding. The
// conv_x6_kernel path splits every input element nine times (once per tap) and
// loads it nine times; B (the pre-split weights of tap t, chunk c = K tile t CH + c)
// arrives by LDS-DMA into NSB stages: with two, two barriers per K tile as there;
// with three, the stage a DMA refills was last read two tiles ago, so one barrier per
// K tile (plus one per chunk before the halo is rewritten). Same products, same f32
// accumulation, K summed in another order (chunk-major instead of tap-major).
// Halo planes: A fragments start at any row (base + dy W + dx), so the chunk swizzle
// keys on row bit 2 -- conflict-free ds_read_b128 fragment reads (16 rows, two chunks
// per lane group) for every start row, where swz's bit-3 key is conflict-free only
// for starts that are multiples of 8 (checked exhaustively over the 8 start residues)
__device__ __forceinline__ int swzh(int row, int chunk) { return row * 64 + ((chunk ^ (((row >> 2) & 1) << 1)) << 4); }

// TR (round 4, option x6_halo_tr): the MFMA operands exchanged as on the TR GEMM tiles
// (weight rows permuted by x6_tr_row in the DMA, D^T accumulators), so the epilogue runs
// from registers (x6_epilogue_tr) with no LDS staging passes: bit-identical.
//
// S2 (round 5, option x6_halo_s2): 3x3 / stride 2 / pad 1 by phase decomposition. Input
// pixel (2 yo + dy, 2 xo + dx) of output (yo, xo) lies in phase image (py, px) = (dy != 0,
// dx != 0) -- input rows / columns of one parity, an Ho x Wo image indexed like the
// output -- at phase pixel (yo - (dy < 0), xo - (dx < 0)). So each tap reads its phase
// image at a shift of 0 or -1 row / column, the stride-1 halo trick with the halo rows
// m0 - Wo - 1 .. m0 + 255 of one phase image at a time. Per 32-channel chunk the four
// phase halos are split and staged in turn -- phase (1,1) with taps (+-1, +-1), (1,0)
// with (+-1, 0), (0,1) with (0, +-1), (0,0) with (0, 0) -- each loaded into registers
// under the previous phase's taps. A shift-0 tap never crosses a frame (the phase
// pixel is the output pixel's own), a shift of -1 needs yo > 0 / xo > 0, and an odd
// row / column past an odd-sized input is a zero load. conv_x6_kernel splits every
// input element of a stride-2 3x3 conv ~2.25 times per chunk (once per tap that reads
// it); here ~1.3 (the phase halos' overlap). K runs chunk-major in phase order: a
// fixed order for every output (batch invariance), another f32 summation order than
// the tap-major GEMM.
__host__ __device__ __forceinline__ constexpr int s2_tap(int j) {   // step j of a chunk -> weight tap (dy + 1) * 3 + dx + 1
    return j == 0 ? 8 : j == 1 ? 6 : j == 2 ? 2 : j == 3 ? 0 : j == 4 ? 7 : j == 5 ? 1 : j == 6 ? 5 : j == 7 ? 3 : 4;
}
__host__ __device__ __forceinline__ constexpr bool s2_last(int j) { return j == 3 || j == 5 || j == 7 || j == 8; }   // a phase ends

template <int BN, int NSB, bool TR = false, bool S2 = false, bool PF = false>
__global__ __launch_bounds__(512, BN <= 64 ? 4 : 2) void conv_x6_halo_kernel(ConvArgs a) {
    using S = X6Shape<256, BN, 512, 2, 2>;
    constexpr int BM = 256, NT = 512, TM = S::TM, TN = S::TN, WAVES = S::WAVES, PL_B = S::PL_B;
    constexpr int QI = 4;                           // halo items (row, 8 channels) per thread: HR <= 512
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / S::WAVES_N, wn = wid % S::WAVES_N;
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    const int tn = wg % a.ntiles_n, tm = wg / a.ntiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    static_assert(!S2 || (NSB == 3 && S::NDMA % WAVES == 0), "stride-2 halo: three B stages, whole DMA rounds");
    const int W = a.yw, H = a.yh, HW = H * W;
    const int HR = S2 ? BM + W + 1 : BM + 2 * W + 2, HP = HR + 1;   // halo rows + one zero row (index HR)
    const int PL_H = HP * 64;
    char* Ah = smem + NSB * 2 * PL_B;               // after the B stages
    const int CH = a.cin_pad / 32, nsteps = 9 * CH, nk = a.kpad / KT;
    const int nhalo = S2 ? 4 * CH : CH;             // halos per tile (S2: four phase images per chunk)

    // ---- halo staging: item i = tid + NT q: row hr = i >> 2, 8 channels pr = i & 3
    const long xbytes = (long)a.B * a.xh * a.xw * a.ldx * 4;
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)xbytes, 0x00020000);
    int hoff[QI];                                    // element offset of the item's pixel + channels
    unsigned hexp = 0;                              // the items' frame scale exponents, a byte each
    unsigned hodd = 0;                              // S2: item q's odd input row (bit 2q) / column (2q+1) exists
    const int xg = a.grp_co ? (n0 / a.grp_co) * a.grp_ci : 0;   // grouped conv: this N tile's input group
#pragma unroll
    for (int q = 0; q < QI; ++q) {
        const int it = tid + NT * q, hr = it >> 2, pr = it & 3;
        const int pix = m0 - W - 1 + hr;
        const bool ok = hr < HR && pix >= 0 && pix < a.M;
        if constexpr (S2) {   // phase pixel pix = (b, yo, xo): phase (0, 0) input pixel (b, 2 yo, 2 xo)
            const int b = pix / HW, rem = pix - b * HW, yo = rem / W, xo = rem - yo * W;
            hoff[q] = ok ? ((b * a.xh + 2 * yo) * a.xw + 2 * xo) * a.ldx + a.xcoff + xg + pr * 8 : -1;
            hodd |= (unsigned)((2 * yo + 1 < a.xh ? 1 : 0) | (2 * xo + 1 < a.xw ? 2 : 0)) << (2 * q);
        } else {
            hoff[q] = ok ? pix * a.ldx + a.xcoff + xg + pr * 8 : -1;
        }
        hexp |= (unsigned)((ok ? act_scale_exp(a, pix / HW) : 0) & 0xff) << (8 * q);
    }
    u32x4 hx[QI][2];
    // halo h: chunk h (stride 1); chunk h / 4, phase (py, px) = (1,1) (1,0) (0,1) (0,0) for h % 4 (S2)
    auto load_halo = [&](int h) {
        const int c = S2 ? h >> 2 : h, ph = S2 ? 3 - (h & 3) : 0, py = ph >> 1, px = ph & 1;
        const int dph = (py * a.xw + px) * a.ldx;
        const unsigned need = (unsigned)(py | (px << 1));
#pragma unroll
        for (int q = 0; q < QI; ++q) {
            const bool v = hoff[q] >= 0 && (!S2 || ((hodd >> (2 * q)) & need) == need);
            const unsigned off = v ? (unsigned)(hoff[q] + dph + c * KT) * 4u : 0x80000000u;
            hx[q][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)off, 0, 0));
            hx[q][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)off, 16, 0));
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int q = 0; q < QI; ++q) {
            const int it = tid + NT * q, hr = it >> 2, pr = it & 3;
            if (hr < HR) {
                float e[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e[j] = __uint_as_float(hx[q][0][j]);
                    e[4 + j] = __uint_as_float(hx[q][1][j]);
                }
                u32x4 o[3];
                const int ex = (int)(signed char)((hexp >> (8 * q)) & 0xff);
                split_pack<2>(e, __builtin_ldexpf(1.f, ex), o);
                *(u32x4*)(Ah + swzh(hr, pr)) = o[0];
                *(u32x4*)(Ah + PL_H + swzh(hr, pr)) = o[1];
            }
        }
    };

    // ---- B: LDS-DMA as conv_x6_kernel, K tile of step s = tap * CH + chunk
    constexpr int RB = BN / 16, NDMA = S::NDMA;
    const int my_dma = NDMA / WAVES + (wid < NDMA % WAVES ? 1 : 0);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7fffffff, 0x00020000);
    // piece q of this wave's DMA share of step s's K tile into stage st
    auto dma_piece = [&](int s, int st, int q) {
        const int c = s / 9, j = s - 9 * c, kt = (S2 ? s2_tap(j) : j) * CH + c;
        char* Bs = smem + st * 2 * PL_B;
        const int jd = wid + WAVES * q;
        if (jd < NDMA) {
            const int p = jd / RB, r0 = (jd % RB) * 16;
            const int row = r0 + (lane >> 2), slot = lane & 3;
            const int chunk = slot ^ (((row >> 3) & 1) * 3);
            const int wrow = TR ? x6_tr_row(row) : row;
            const unsigned off = (unsigned)((((long)(n0 + wrow) * nk + kt) * 2 + p) * 64 + chunk * 16);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_void_t*)(Bs + p * PL_B + r0 * 64), 16, off, 0,
                                                     0, 0);
        }
    };
    auto dma_b = [&](int s, int st) {
#pragma unroll
        for (int q = 0; q < (NDMA + WAVES - 1) / WAVES; ++q) dma_piece(s, st, q);
    };
    // where a step issues the DMA of step s + 2 (option x6_halo_dma, whole DMA rounds only):
    // 0 right after the step's barrier, 1 after its MFMAs, 2 one piece between MFMA groups
    constexpr int MYD = S::NDMA % WAVES == 0 ? S::NDMA / WAVES : 0;
    const int hdma = MYD ? a.halo_dma & 3 : 0;
    // timing-only skips (x6_dbg bits 2-5 via vdt_set_debug / x6bench; WRONG results): 1 no B DMA
    // past the prologue, 2 no halo reload, 8 no main-loop barriers
    const int hdbg = (a.dbg >> 2) & 15;

    // ---- per-lane A rows: this lane's output row of each fragment i, its halo row for
    // tap (0, 0) and which neighbours exist (bit 0 y-1, 1 y+1, 2 x-1, 3 x+1, 4 row < M)
    int arow[TM], aflg[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * S::WTM + i * 16 + (lane & 15), m = m0 + r;
        const int rem = m % HW, y = rem / W, x = rem - y * W;
        arow[i] = r + W + 1;
        aflg[i] = (y > 0 ? 1 : 0) | (y < H - 1 ? 2 : 0) | (x > 0 ? 4 : 0) | (x < W - 1 ? 8 : 0) | (m < a.M ? 16 : 0);
    }

    using AccT = f32x4_t;
    AccT acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = AccT{};
    const int amax_off = std::max(NSB * 2 * PL_B + 2 * PL_H, S::EPR * S::EPLD * 4);
    if (a.ymax)
        for (int f = tid; f < a.B; f += NT) ((unsigned*)(smem + amax_off))[f] = 0u;

    auto compute = [&](int st, int dy, int dx, int dstep) {
        const char* Bs = smem + st * 2 * PL_B;
        const int ch = lane >> 4;
        // S2: taps with d = +1 read the phase pixel itself (its own frame; odd rows / columns
        // past the input were loaded as zeros), d = -1 the previous phase row / column
        const int need = S2 ? (dy < 0 ? 1 : 0) | (dx < 0 ? 4 : 0) | 16
                            : (dy < 0 ? 1 : 0) | (dy > 0 ? 2 : 0) | (dx < 0 ? 4 : 0) | (dx > 0 ? 8 : 0) | 16;
        const int shift = S2 ? (dy < 0 ? -W : 0) + (dx < 0 ? -1 : 0) : dy * W + dx;
        if constexpr (TN < TM) {   // narrow N: B fragments resident, A streamed (VGPRs at 4 waves / SIMD)
            u32x4 bf[TN][3];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bf[j][0] = *(const u32x4*)(Bs + swz64(wn * S::WTN + j * 16 + (lane & 15), ch));
                bf[j][1] = *(const u32x4*)(Bs + PL_B + swz64(wn * S::WTN + j * 16 + (lane & 15), ch));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int hr = (aflg[i] & need) == need ? arow[i] + shift : HR;
                const int o = swzh(hr, ch);
                u32x4 af[3];
                af[0] = *(const u32x4*)(Ah + o);
                af[1] = *(const u32x4*)(Ah + PL_H + o);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (TR) acc[i][j] = mfma_pair_tr(af, bf[j], acc[i][j]);
                    else acc[i][j] = mfma_pair(af, bf[j], acc[i][j]);
                }
            }
        } else if constexpr (PF) {
            // PF (option x6_halo_pf): the B fragments of column block j + 1 are read before
            // the MFMAs of block j (two buffers: the registers of the compiler's paired reads),
            // pinned by scheduling groups, so an LDS read's latency hides behind 3 TM MFMAs
            u32x4 af[TM][3], bq[2][3];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int hr = (aflg[i] & need) == need ? arow[i] + shift : HR;
                const int o = swzh(hr, ch);
                af[i][0] = *(const u32x4*)(Ah + o);
                af[i][1] = *(const u32x4*)(Ah + PL_H + o);
            }
            bq[0][0] = *(const u32x4*)(Bs + swz64(wn * S::WTN + (lane & 15), ch));
            bq[0][1] = *(const u32x4*)(Bs + PL_B + swz64(wn * S::WTN + (lane & 15), ch));
            __builtin_amdgcn_sched_group_barrier(0x0100, 2 * TM + 2, 0);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (j + 1 < TN) {
                    bq[(j + 1) & 1][0] = *(const u32x4*)(Bs + swz64(wn * S::WTN + (j + 1) * 16 + (lane & 15), ch));
                    bq[(j + 1) & 1][1] = *(const u32x4*)(Bs + PL_B + swz64(wn * S::WTN + (j + 1) * 16 + (lane & 15), ch));
                    __builtin_amdgcn_sched_group_barrier(0x0100, 2, 0);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (TR) acc[i][j] = mfma_pair_tr(af[i], bq[j & 1], acc[i][j]);
                    else acc[i][j] = mfma_pair(af[i], bq[j & 1], acc[i][j]);
                }
                __builtin_amdgcn_sched_group_barrier(0x0008, 3 * TM, 0);
                if constexpr (MYD > 0 && TN % MYD == 0) {   // x6_halo_dma = 2: a DMA piece per group
                    if (dstep >= 0 && j % (TN / MYD) == 0) dma_piece(dstep, dstep % NSB, j / (TN / MYD));
                }
            }
        } else {
            u32x4 af[TM][3];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int hr = (aflg[i] & need) == need ? arow[i] + shift : HR;
                const int o = swzh(hr, ch);
                af[i][0] = *(const u32x4*)(Ah + o);
                af[i][1] = *(const u32x4*)(Ah + PL_H + o);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                u32x4 bf[3];
                bf[0] = *(const u32x4*)(Bs + swz64(wn * S::WTN + j * 16 + (lane & 15), ch));
                bf[1] = *(const u32x4*)(Bs + PL_B + swz64(wn * S::WTN + j * 16 + (lane & 15), ch));
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (TR) acc[i][j] = mfma_pair_tr(af[i], bf, acc[i][j]);
                    else acc[i][j] = mfma_pair(af[i], bf, acc[i][j]);
                }
                if constexpr (MYD > 0 && TN % MYD == 0) {   // x6_halo_dma = 2: a DMA piece per group
                    if (dstep >= 0 && j % (TN / MYD) == 0) dma_piece(dstep, dstep % NSB, j / (TN / MYD));
                }
            }
        }
    };

    // ---- prologue: chunk 0's halo in LDS (+ the zero row), B of steps 0 and 1 in flight,
    // chunk 1's halo loading into registers
    load_halo(0);
    store_halo();
    if (tid < 8) *(u32x4*)(Ah + (tid >> 2) * PL_H + swzh(HR, tid & 3)) = u32x4{0u, 0u, 0u, 0u};
    dma_b(0, 0);
    const bool one_bar = NSB == 2 && MYD > 0 && a.halo_1b;
    if (nsteps > 1 && !one_bar) dma_b(1, 1);
    if (nhalo > 1) load_halo(1);
    // Per thread VMEM issue order: ... [halo loads of chunk c+2 at the end of step
    // 9c+8], B(s+2) at the end of step s. At the top of step s, younger than B(s):
    // B(s+1) (if issued) and the halo loads issued at the end of step s-1 or (s = 1)
    // in the prologue after B(1).
    if constexpr (NSB == 3 && S::NDMA % WAVES == 0) {
        // This wave's DMA count per step is a compile-time constant, so each step's vmcnt
        // is one of four immediates chosen by two uniform branches (the runtime wait_vm
        // switch costs a tree of scalar branches per step). (Unrolling the nine taps of a
        // chunk as well measured no better and spills on the 192 / 256-wide tiles.)
        int hcur = 0;                                    // the halo in LDS
        for (int s = 0; s < nsteps; ++s) {
            const int tap = s % 9;
            // halo loads younger than B(s): halo hcur+1's, issued at the end of step s-1 when
            // that step ended a halo, or in the prologue after B(1) (s = 0, 1)
            const bool ended = s >= 1 && (S2 ? s2_last(tap == 0 ? 8 : tap - 1) : tap == 0);
            const bool halo_prev = ended ? hcur + 1 < nhalo : (s <= 1 && nhalo > 1);
            if (halo_prev) {
                if (s + 1 < nsteps) wait_vm_k<MYD + 2 * QI>();
                else wait_vm_k<2 * QI>();
            } else {
                if (s + 1 < nsteps) wait_vm_k<MYD>();
                else wait_vm_k<0>();
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (!(hdbg & 8)) __builtin_amdgcn_s_barrier();   // B(s) visible; stage (s + 2) % 3 free
            asm volatile("" ::: "memory");
            const bool rehalo = (S2 ? s2_last(tap) : tap == 8) && hcur + 1 < nhalo;
            const bool dnext = !rehalo && s + 2 < nsteps && !(hdbg & 1);
            const int hd = (TN % (MYD ? MYD : 1) == 0 && TN >= TM) ? hdma : (hdma ? 1 : 0);
            if (dnext && hd == 0) dma_b(s + 2, (s + 2) % 3);
            const int wt = S2 ? s2_tap(tap) : tap;
            const int dy = wt / 3 - 1, dx = wt - (wt / 3) * 3 - 1;
            compute(s % 3, dy, dx, dnext && hd == 2 ? s + 2 : -1);
            if (dnext && hd == 1) dma_b(s + 2, (s + 2) % 3);
            if (rehalo) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (!(hdbg & 8)) __builtin_amdgcn_s_barrier();   // every wave is done with halo hcur
                asm volatile("" ::: "memory");
                if (!(hdbg & 2)) store_halo();
                ++hcur;
                if (hcur + 1 < nhalo && !(hdbg & 2)) load_halo(hcur + 1);
                if (s + 2 < nsteps && !(hdbg & 1)) dma_b(s + 2, (s + 2) % 3);
            }
        }
    } else if constexpr (NSB == 3) {
        // VMEM issue order per step s: [top] B(s+2), except on tap-8 steps, which issue
        // it at the end, after the halo loads of chunk c+2 (the halo stores then wait
        // only on B(s+1), issued a step earlier, not on a DMA just issued). Younger than
        // B(s) at the top of s: B(s+1) and the halo loads issued at the end of s-1 (the
        // prologue's chunk-1 loads follow B(1), so for s = 0 and 1 too).
        for (int s = 0; s < nsteps; ++s) {
            const int c = s / 9, tap = s - 9 * c;
            const bool halo_prev = (s >= 1 && (s - 1) % 9 == 8 && (s - 1) / 9 + 2 < CH) || (s <= 1 && CH > 1);
            const int younger = (s + 1 < nsteps ? my_dma : 0) + (halo_prev ? 2 * QI : 0);
            wait_vm(younger);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                // B(s) visible; stage (s + 2) % 3 free
            asm volatile("" ::: "memory");
            const bool rehalo = tap == 8 && c + 1 < CH;
            if (!rehalo && s + 2 < nsteps) dma_b(s + 2, (s + 2) % 3);
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            compute(s % 3, dy, dx, -1);
            if (rehalo) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();            // every wave is done with chunk c's halo
                asm volatile("" ::: "memory");
                store_halo();
                if (c + 2 < CH) load_halo(c + 2);
                if (s + 2 < nsteps) dma_b(s + 2, (s + 2) % 3);
            }
        }
    } else if (one_bar) {
        // two B stages, ONE barrier per step (option x6_halo_1b): B(s+1)'s DMA is issued
        // after step s's barrier (its stage was last read by step s-1, which every wave has
        // finished there); a halo refill (tap 8) takes a second barrier. Younger than B(s)
        // at the top of s: the halo loads issued at the end of step s-1 (or in the prologue,
        // s = 0), behind the refill barrier's memory clobbers.
        int hcur = 0;
        for (int s = 0; s < nsteps; ++s) {
            const int tap = s % 9;
            const bool halo_prev = s == 0 ? nhalo > 1 : (tap == 0 && hcur + 1 < nhalo);
            if (halo_prev) wait_vm_k<2 * QI>();
            else wait_vm_k<0>();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (!(hdbg & 8)) __builtin_amdgcn_s_barrier();   // B(s) visible; stage (s + 1) & 1 free
            asm volatile("" ::: "memory");
            // B(s+1) right after the barrier (one step of latency cover: measured 3-4 % faster
            // on the 256-wide tiles than pieces between the MFMA groups, r06t)
            if (s + 1 < nsteps && !(hdbg & 1)) dma_b(s + 1, (s + 1) & 1);
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            compute(s & 1, dy, dx, -1);
            if (tap == 8 && hcur + 1 < nhalo) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (!(hdbg & 8)) __builtin_amdgcn_s_barrier();   // every wave is done with halo hcur
                asm volatile("" ::: "memory");
                if (!(hdbg & 2)) store_halo();
                ++hcur;
                if (hcur + 1 < nhalo && !(hdbg & 2)) load_halo(hcur + 1);
            }
        }
    } else {
    for (int s = 0; s < nsteps; ++s) {
        const int c = s / 9, tap = s - 9 * c;
        int younger = s + 1 < nsteps ? my_dma : 0;
        if (s == 0 && CH > 1) younger += 2 * QI;
        if (s == 1 && CH > 1) younger = 2 * QI + (s + 1 < nsteps ? my_dma : 0);
        if (s >= 2 && tap == 0 && c + 1 < CH) younger += 2 * QI;
        wait_vm(younger);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        compute(s & 1, dy, dx, -1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                    // stage s & 1 (and, at tap 8, the halo) are free
        asm volatile("" ::: "memory");
        if (tap == 8 && c + 1 < CH) {
            store_halo();                                // chunk c+1 (its loads were issued 9 steps ago)
            if (c + 2 < CH) load_halo(c + 2);
        }
        if (s + 2 < nsteps) dma_b(s + 2, s & 1);
    }
    }
    if constexpr (TR) {
        x6_epilogue_tr<S>(a, acc, m0, n0, wm, wn, lane, (unsigned*)(smem + amax_off));
    } else {
        __syncthreads();
        x6_epilogue<S, 16>(a, acc, m0, n0, wm, wn, tid, lane, smem, amax_off);
    }
}

template <int BN, int NSB>
static int x6_halo_lds(const ConvArgs& a) {
    using S = X6Shape<256, BN, 512, 2, 2>;
    const int HP = a.stride == 2 ? 256 + a.yw + 2 : 256 + 2 * a.yw + 3;
    return std::max(NSB * 2 * S::PL_B + 2 * HP * 64, S::EPR * S::EPLD * 4) + (a.ymax ? 4 * a.B : 0);
}

template <int BN, int NSB, bool TR, bool S2, bool PF>
static hipError_t launch_x6_halo_pf(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    a.w = a.wx3;
    a.ntiles_n = (a.cout + BN - 1) / BN;
    static const bool attr = [] {
        (void)hipFuncSetAttribute((const void*)conv_x6_halo_kernel<BN, NSB, TR, S2, PF>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        return true;
    }();
    (void)attr;
    const int lds = x6_halo_lds<BN, NSB>(a);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int mt = (a.M + 255) / 256;
    vd_conv_fam_set(S2 ? VD_FAM_X6_HALO_S2 : VD_FAM_X6_HALO);
    hipLaunchKernelGGL((conv_x6_halo_kernel<BN, NSB, TR, S2, PF>), dim3(mt * a.ntiles_n), dim3(512), lds, s, a);
    return hipGetLastError();
}

// option x6_halo_pf: the pipelined B-fragment reads on the 128-256-wide tiles
template <int BN, int NSB, bool TR = false, bool S2 = false>
static hipError_t launch_x6_halo_t(const ConvArgs& a, hipStream_t s) {
    if constexpr (BN >= 128) {
        if (a.tune->x6_halo_pf) return launch_x6_halo_pf<BN, NSB, TR, S2, true>(a, s);
    }
    return launch_x6_halo_pf<BN, NSB, TR, S2, false>(a, s);
}

// TR form where the output (and residual) rows take 8-channel 16-B vectors (option
// x6_halo_tr: 1 the 128 / 192 / 256-wide tiles, 2 the narrow ones too)
template <int BN, int NSB>
static hipError_t launch_x6_halo_n(const ConvArgs& a, hipStream_t s) {
    const bool tr = a.tune->x6_halo_tr >= (BN >= 128 ? 1 : 2) && !((a.ldy | a.ycoff) & 7) && tr_bytes_ok(a) &&
                    (a.res_mode == VD_RES_NONE || !((a.res_ld | a.res_coff) & 7));
    if constexpr (NSB == 3 && BN >= 64) {   // stride 2: the phase halos (vd_x6_halo_ok)
        if (a.stride == 2) return tr ? launch_x6_halo_t<BN, 3, true, true>(a, s) : launch_x6_halo_t<BN, 3, false, true>(a, s);
    }
    if (a.stride != 1) return hipErrorInvalidValue;
    if (tr) return launch_x6_halo_t<BN, NSB, true>(a, s);
    return launch_x6_halo_t<BN, NSB, false>(a, s);
}

// option x6_halo: 1 two B stages, 2 three where they fit LDS beside the halo
template <int BN>
static hipError_t launch_x6_halo(const ConvArgs& a, hipStream_t s) {
    if ((a.tune->x6_halo >= 2 || a.stride == 2) && x6_halo_lds<BN, 3>(a) <= 160 * 1024) return launch_x6_halo_n<BN, 3>(a, s);
    return launch_x6_halo_n<BN, 2>(a, s);
}

}  // namespace

// 3x3 / stride 1 / pad 1, same-size in and out, K = 9 x Cin in whole 32-channel chunks,
// halo of at most 512 rows (W <= 126) that fits LDS beside the B stages; stride 2 (option
// x6_halo_s2): the phase halos of at most 512 rows (Wo <= 254), N tiles of >= 64 (Cout > 32,
// whole DMA rounds), three B stages, dense
bool vd_x6_halo_ok(const ConvArgs& a) {
    if (!a.tune->x6_halo || a.kh != 3 || a.kw != 3 || a.pad != 1) return false;
    if (a.cin_pad % 32 || a.kpad != 9 * a.cin_pad || (a.ymax && a.B > kAmaxFrames)) return false;
    if (a.stride == 2) {
        if (!a.tune->x6_halo_s2 || a.cout <= 32 || a.grp_co) return false;
        if (a.yh != (a.xh - 1) / 2 + 1 || a.yw != (a.xw - 1) / 2 + 1 || 256 + a.yw + 2 > 512) return false;
        return (3 * 2 * 256 * 64 + 2 * (256 + a.yw + 2) * 64 + (a.ymax ? 4 * a.B : 0)) <= 160 * 1024;
    }
    if (a.stride != 1 || a.xh != a.yh || a.xw != a.yw) return false;
    if (256 + 2 * a.yw + 2 > 512) return false;
    return true;
}

hipError_t vd_launch_x6_halo(const ConvArgs& a, int bn, hipStream_t s) {
    if (bn == 32) return launch_x6_halo<32>(a, s);
    if (bn == 64) return launch_x6_halo<64>(a, s);
    if (bn == 128) return launch_x6_halo<128>(a, s);
    if (bn == 192) return launch_x6_halo<192>(a, s);
    if (bn == 256) return launch_x6_halo<256>(a, s);
    return hipErrorInvalidValue;
}

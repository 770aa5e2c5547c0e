// vd_nms.h — the sort and the greedy NMS sweep shared by the per-input post kernel
// (post.hip nms_frame) and the cross-tile merge (tiles.hip): one 1024-thread workgroup per
// list, the rule and the op order of torchvision's nms [ext] (stable descending sort through
// 64-bit keys, IoU in float32 compared against a double, vd_math.h vd_iou_gt).
#pragma once
#include "vd_math.h"

constexpr int VD_NMS_THREADS = 1024;
constexpr int VD_NMS_LDS_CAND = 2048;   // candidates held in LDS; larger lists use global scratch

// keys[0, P) (P a power of two, entries past the list ~0) sorted ascending: a bitonic sort by
// the whole workgroup. Ends with a barrier.
__device__ __forceinline__ void vd_nms_sort(uint64_t* keys, int P) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += VD_NMS_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t ki = keys[i], kj = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((ki > kj) == up) { keys[i] = kj; keys[ixj] = ki; }
                }
            }
            __syncthreads();
        }
    }
}

// Greedy NMS over box[0, M) in list order (area[] and supp[] = 0 filled by the caller, *nkept_s
// = 0, a barrier since), in chunks of 64: wave 0 resolves a chunk with a 64x64 IoU bitmask and a
// readlane sweep, then all 16 waves suppress later candidates against the chunk's kept boxes --
// exactly the sequential greedy keep list. Kept candidate j gets emit_fn(pos, j, box[j]) from
// its lane of wave 0 while pos < limit; *nkept_s ends as the complete keep count.
// CLS (the plate tile merge): cls[0, M) holds each box's class, and a kept box suppresses boxes
// of its own class only; without it cls is never read and the sweep is the one above.
template <bool CLS, typename Emit>
__device__ __forceinline__ void vd_nms_greedy_cls(int M, const float4* box, const float* area, uint8_t* supp,
                                                  uint64_t* chunk_keep, int* nkept_s, double iou, int limit,
                                                  Emit emit_fn, const int* cls) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int c0 = 0; c0 < M; c0 += 64) {
        if (wid == 0) {
            const int j = c0 + lane;
            const bool valid = j < M;
            const float4 bj = valid ? box[j] : make_float4(0, 0, 0, 0);
            const float aj = valid ? area[j] : 0.f;
            const bool alive = valid && !supp[j];
            int cj = 0;
            if constexpr (CLS) cj = valid ? cls[j] : 0;
            uint64_t mask = 0;
            const int lim = min(64, M - c0);
            for (int k = lane + 1; k < lim; ++k) {
                if constexpr (CLS) {
                    if (cls[c0 + k] != cj) continue;
                }
                const float4 bk = box[c0 + k];
                if (vd_iou_gt(bj.x, bj.y, bj.z, bj.w, aj, bk.x, bk.y, bk.z, bk.w, area[c0 + k], iou))
                    mask |= 1ULL << k;
            }
            uint64_t alive_bits = __ballot(alive);
            const uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
            for (int i = 0; i < lim; ++i) {
                if ((alive_bits >> i) & 1ULL) {
                    const uint64_t mi = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mhi, i) << 32) |
                                        (uint32_t)__builtin_amdgcn_readlane((int)mlo, i);
                    alive_bits &= ~mi;
                }
            }
            const int base = *nkept_s;
            if ((alive_bits >> lane) & 1ULL) {
                const int pos = base + __popcll(alive_bits & ((1ULL << lane) - 1ULL));
                if (pos < limit) emit_fn(pos, j, bj);
            }
            if (lane == 0) {
                *nkept_s = base + __popcll(alive_bits);
                *chunk_keep = alive_bits;
            }
        }
        __syncthreads();
        const uint64_t kb = *chunk_keep;
        if (kb) {
            for (int j = c0 + 64 + tid; j < M; j += VD_NMS_THREADS) {
                if (supp[j]) continue;
                const float4 bj = box[j];
                const float aj = area[j];
                int cj = 0;
                if constexpr (CLS) cj = cls[j];
                uint64_t bits = kb;
                while (bits) {
                    const int i = __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    if constexpr (CLS) {
                        if (cls[c0 + i] != cj) continue;
                    }
                    const float4 bi = box[c0 + i];
                    if (vd_iou_gt(bi.x, bi.y, bi.z, bi.w, area[c0 + i], bj.x, bj.y, bj.z, bj.w, aj, iou)) {
                        supp[j] = 1;
                        break;
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <typename Emit>
__device__ __forceinline__ void vd_nms_greedy(int M, const float4* box, const float* area, uint8_t* supp,
                                              uint64_t* chunk_keep, int* nkept_s, double iou, int limit,
                                              Emit emit_fn) {
    vd_nms_greedy_cls<false>(M, box, area, supp, chunk_keep, nkept_s, iou, limit, emit_fn, nullptr);
}

// int(x) of a Python float; values beyond int32 are clamped (the mosaic clips to the frame
// first, combine_detect.py:145-148, so the output is unchanged).
__device__ __forceinline__ int vd_trunc_i32(float v) {
    if (!(v == v)) return 0;
    if (v >= 2147483520.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;   // truncation toward zero
}

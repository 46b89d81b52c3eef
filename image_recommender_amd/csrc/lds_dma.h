// lds_dma.h — global -> LDS DMA helpers shared by every kernel that stages through an LDS-DMA ring
// (knn_tile.h: the fp32 tile core of the top-k, range and filter kernels; knn_b16w.hip: the bf16
// candidate pass; vit_gemm.hip: the ViT GEMMs).
//
// LDS-DMA is issued from inline asm (M0 = wave-uniform LDS destination, set and restored inside the
// statement).  hipcc does not see these as LDS writes, so it inserts no vmcnt(0) in front of the
// fragment ds_reads (it would for __builtin_amdgcn_global_load_lds, serialising the ring: DESIGN.md
// "Kernels"); every wait on them is the explicit counted wait_vmcnt below.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace imgrec {

__device__ __forceinline__ uint32_t lds_u32(const void* p) {
    return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) char*)p);
}

// One 1-KiB piece: 16 B per lane, lane-linear in LDS.
__device__ __forceinline__ void dma16(const float* g, uint32_t lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds)) : "memory");
}
// The same with the non-temporal policy, for bf16 corpus rows that exactly one workgroup reads (a
// launch with one query block): nq = 1 on 1M x 1968 0.695 -> 0.667 ms.  The fp32 corpus of the
// exact kernel runs slower with it (1.94 -> 2.70 ms), so it keeps the default policy.
__device__ __forceinline__ void dma16_nt(const float* g, uint32_t lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds)) : "memory");
}

// Four one-KiB LDS-DMA pieces under one M0 value (instruction offsets move both the global source
// and the LDS destination; the per-lane offsets are pre-reduced by j KiB).
__device__ __forceinline__ void dma4x(const void* sbase, uint32_t lds0, uint32_t v0, uint32_t v1,
                                      uint32_t v2, uint32_t v3) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %5\n\t"
        "global_load_lds_dwordx4 %2, %5 offset:1024\n\t"
        "global_load_lds_dwordx4 %3, %5 offset:2048\n\t"
        "global_load_lds_dwordx4 %4, %5 offset:3072\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds0))
        : "memory");
}

template <int OFF>
__device__ __forceinline__ void dma1(const void* sbase, uint32_t lds0, uint32_t v) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:%4\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds0)), "n"(OFF)
        : "memory");
}

// one piece at instruction offset (j & 3) KiB (the dma4x group member j of a partial issue)
__device__ __forceinline__ void dma1_at(int j, const void* sbase, uint32_t lds0, uint32_t v) {
    switch (j & 3) {
        case 0: dma1<0>(sbase, lds0, v); break;
        case 1: dma1<1024>(sbase, lds0, v); break;
        case 2: dma1<2048>(sbase, lds0, v); break;
        default: dma1<3072>(sbase, lds0, v); break;
    }
}

// one dword per lane (the row norms or the list entries of a tile)
__device__ __forceinline__ void dma4_norm(const float* g, uint32_t lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds)) : "memory");
}

// 2 KiB (two one-KiB pieces, lane l: bytes 16 l .. 16 l + 15 of each) read at agent scope (sc1:
// past the L1, as a relaxed agent-scope atomic load is): words other workgroups update with
// atomics during the launch; every aligned dword arrives whole
__device__ __forceinline__ void dma2_agent(const void* sbase, uint32_t lds0, uint32_t v) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2 sc1\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:1024 sc1\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds0))
        : "memory");
}

// The counted wait of a DMA ring: at most N of this wave's DMA instructions still in flight.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// s_barrier that also orders the compiler's LDS accesses (the intrinsic alone is IntrNoMem).
__device__ __forceinline__ void barrier_lds() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace imgrec

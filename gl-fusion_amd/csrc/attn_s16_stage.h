// What the fused attention kernels of 16-bit storage share (attn_s16.hip: softmax(theta phi^T) g; attn_pair_s16.hip:
// relu(a_i + b_j + c) g): the block geometry, the three-slot ring of LDS-DMA staged tiles with its counted waits, and the
// chunk swizzle of the bf16 [64][64] T tile.
#pragma once
#include "gemm_common.h"
#include "stream_common.h"

namespace {

using glf::pack2;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4_ __attribute__((ext_vector_type(4)));
typedef unsigned short u16;
typedef int v2i_ __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

constexpr int SA_T = 64;                  // outer and inner rows per block
constexpr int SA_NT = 512;
constexpr int SA_MAXCI = 1024;
constexpr int SA_SLOT = 32768 + 512;      // ring slot: 32 KiB of operand tiles + lse / D rows of the inner block
constexpr int SA_NSLOT = 3;

__device__ __forceinline__ void glds16(const u16* src, unsigned char* lds_base) {
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)lds_base, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const float* src, unsigned char* lds_base) {
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)lds_base, 4, 0, 0);
}
// wait until at most n of this wave's vector-memory operations are outstanding (n wave-uniform, 0..5) and its LDS writes are done
// (they are read by other waves behind the barrier that follows)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 5: asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); break;
    }
}
// byte offset of bf16 element (m, k) of a [64][64] tile with the 16-byte chunk swizzle
__device__ __forceinline__ int tt_off(int m, int k) { return m * 128 + ((((k >> 3) ^ (m >> 1)) & 7) << 4) + (k & 7) * 2; }

}  // namespace

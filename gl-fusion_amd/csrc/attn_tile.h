// The tile skeleton shared by the fused attention kernels of the fusion block (attn_softmax.hip: softmax(theta phi^T) g;
// attn_pair.hip: relu(a_i + b_j + c) g): 64-row outer blocks, 64 x 64 score-type tiles contracted over Ci through k-major LDS
// staging tiles, and the 64 x Ci product-type accumulation held in MFMA accumulators.
#pragma once
#include "gemm_common.h"

namespace {

constexpr int AT = 64;            // rows per block (outer and inner)
constexpr int AKC = 32;           // contraction chunk of the score tiles
constexpr int ALD = 65;           // LDS row stride of every [*][64] tile (k-major staging tiles, score tiles)
constexpr int ANT = 256;
constexpr int A_MAXCT = 8;        // 32-column accumulator tiles per wave  => Ci <= 4 * 8 * 32 = 1024

#define GLF_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0)

// stage rows [r0, r0 + 64) x columns [k0, k0 + 32) of a row-major matrix into a k-major LDS tile dst[32][ALD];
// rows beyond L are clamped to L - 1 (their scores are masked / their outputs never stored)
struct Staged { float4 a, b; };
__device__ __forceinline__ Staged stage_load(const float* __restrict__ src, long long ld, int r0, int L, int k0, int tid) {
    const int row = tid >> 3, kq = tid & 7;
    const int ra = min(r0 + row, L - 1), rb = min(r0 + row + 32, L - 1);
    Staged s;
    s.a = *reinterpret_cast<const float4*>(src + (long long)ra * ld + k0 + 4 * kq);
    s.b = *reinterpret_cast<const float4*>(src + (long long)rb * ld + k0 + 4 * kq);
    return s;
}
__device__ __forceinline__ void stage_store(float* __restrict__ dst, const Staged& s, int tid) {
    const int row = tid >> 3, kq = tid & 7;
    float* d = dst + (4 * kq) * ALD + row;
    d[0] = s.a.x; d[ALD] = s.a.y; d[2 * ALD] = s.a.z; d[3 * ALD] = s.a.w;
    d[32] = s.b.x; d[ALD + 32] = s.b.y; d[2 * ALD + 32] = s.b.z; d[3 * ALD + 32] = s.b.w;
}

// S quadrant (rt, ct) of X[x0 .. x0+64) . Y[y0 .. y0+64)^T over `ci` columns.  `stg` = 4 tiles of [32][ALD] (two buffers
// of an X tile and a Y tile).  Every thread of the workgroup must call it (barriers inside).
__device__ __forceinline__ f32x16 score_tile(const float* __restrict__ X, long long ldx, int x0, const float* __restrict__ Y, long long ldy,
                                             int y0, int L, int ci, float* __restrict__ stg, int tid, int lane, int rt, int ct) {
    constexpr int TILE = AKC * ALD;
    f32x16 s = {0};
    Staged sx = stage_load(X, ldx, x0, L, 0, tid), sy = stage_load(Y, ldy, y0, L, 0, tid);
    __syncthreads();                                  // the previous user of the staging tiles is done
    stage_store(stg, sx, tid);
    stage_store(stg + TILE, sy, tid);
    __syncthreads();
    const int nchunk = ci / AKC;
    const int hl = lane >> 5, l31 = lane & 31;
    for (int c = 0; c < nchunk; ++c) {
        const float* xs = stg + (c & 1) * 2 * TILE;
        const float* ys = xs + TILE;
        const bool more = c + 1 < nchunk;
        if (more) {
            sx = stage_load(X, ldx, x0, L, (c + 1) * AKC, tid);
            sy = stage_load(Y, ldy, y0, L, (c + 1) * AKC, tid);
        }
#pragma unroll
        for (int ks = 0; ks < AKC / 2; ++ks) {
            const float a = xs[(2 * ks + hl) * ALD + 32 * rt + l31];
            const float b = ys[(2 * ks + hl) * ALD + 32 * ct + l31];
            s = GLF_MFMA_F32(a, b, s);
        }
        if (more) {
            float* nx = stg + ((c + 1) & 1) * 2 * TILE;
            stage_store(nx, sx, tid);
            stage_store(nx + TILE, sy, tid);
        }
        __syncthreads();
    }
    return s;
}

// acc[rt][jj] += sum_k T[k][32 rt + m] * Z[z0 + k][32 j + n] for this wave's column tiles j = wave + 4 jj:
// A fragments from the k-major LDS tile T ([64][ALD]), B fragments straight from global memory (rows clamped to L - 1:
// the matching T entries are exactly zero).
__device__ __forceinline__ void accumulate(f32x16 (&acc)[2][A_MAXCT], const float* __restrict__ T, const float* __restrict__ Z, long long ldz,
                                           int z0, int L, int nct, int wave, int lane) {
    const int hl = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int jj = 0; jj < A_MAXCT; ++jj) {
        const int j = wave + 4 * jj;
        if (j < nct) {
            const float* zc = Z + 32 * j + l31;
            // B fragments of the next eight k-steps are in flight while the current eight are multiplied; the scheduling
            // barriers keep hipcc from hoisting the loads of ALL column tiles to the top (it spilled 170 registers)
            float b[8], bn[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) b[u] = zc[(long long)min(z0 + 2 * u + hl, L - 1) * ldz];
#pragma unroll 1
            for (int kb = 0; kb < AT / 2; kb += 8) {
                if (kb + 8 < AT / 2) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) bn[u] = zc[(long long)min(z0 + 2 * (kb + 8 + u) + hl, L - 1) * ldz];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float a0 = T[(2 * (kb + u) + hl) * ALD + l31];
                    const float a1 = T[(2 * (kb + u) + hl) * ALD + 32 + l31];
                    acc[0][jj] = GLF_MFMA_F32(a0, b[u], acc[0][jj]);
                    acc[1][jj] = GLF_MFMA_F32(a1, b[u], acc[1][jj]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) b[u] = bn[u];
            }
        }
    }
}

}  // namespace

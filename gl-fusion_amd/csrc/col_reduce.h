// Column reductions over the rows of a channels-last [rows][C] tensor, written once for every access width W (elements per 16-byte
// access: 4 for fp32 storage, 8 for bf16): the grid geometry, what a thread owns, and the epilogue that folds a workgroup's row
// lanes through LDS into ONE f64 atomic (or one atomic max) per column, statistic and workgroup.  Users: norm.hip.
#pragma once
#include "stream_common.h"

namespace glf {

constexpr int RED_THREADS = 256;      // threads of a reduction workgroup
// Grid shape of the single-stage (atomic) reductions (profiles/r04_bn_reduce_sweep.txt): a workgroup covers RED_TPR accesses of W
// columns with 256 / RED_TPR row lanes, ~RED_RPT rows per thread, at most RED_MAX_WG workgroups.  What it optimises is the number of
// f64 atomics that land on ONE address: same-address atomics are serialised by the L2 (~25-30 ns each; 1 024 workgroups adding to
// the same 512 doubles took longer than streaming the tensor), so narrow column blocks -- many blocks, few row slices per block --
// beat whole rows: 193 600 x 256: 37.8 -> 27.5 us, 50 176 x 1 024: 45.4 -> 20.3 us.  More, smaller workgroups only add atomics;
// fewer leave too few loads in flight (these reductions are latency-bound: 512 workgroups of 12 dependent iterations ran at 1 TB/s).
constexpr int RED_TPR = 16, RED_RPT = 16, RED_MAX_WG = 1024;

struct RedGeom { int tpr, rpp, cblocks, slices; };      // threads per row, rows per pass, column blocks, row slices
template <int W>
__host__ __device__ inline RedGeom red_geom(int rows, int c) {
    const int cw = c > W ? c / W : 1;
    RedGeom g;
    g.tpr = cw < RED_TPR ? cw : RED_TPR;
    g.rpp = RED_THREADS / g.tpr;
    g.cblocks = (cw + g.tpr - 1) / g.tpr;
    const int s = (rows + RED_RPT * g.rpp - 1) / (RED_RPT * g.rpp);
    int cap = RED_MAX_WG / g.cblocks;      // one f64 atomic per column and slice
    if (cap < 1) cap = 1;
    g.slices = s < 1 ? 1 : (s > cap ? cap : s);
    return g;
}
inline dim3 red_grid(const RedGeom& g) { return dim3(g.slices, g.cblocks); }

// What a thread of workgroup (blockIdx.x = row slice, blockIdx.y = column block) owns: access cc (columns c0 .. c0 + W - 1) and
// the rows r, r + rpp, ... < r1 of its slice.  tpr_max: the widest column block, in accesses.
struct RedLane { int tpr, rpp, ct, rl, cb, cc, c0, r, r1; bool live; };
template <int W>
__device__ __forceinline__ RedLane red_lane(int rows, int c, int slices, int tpr_max) {
    RedLane L;
    const int cw = c / W;
    L.tpr = cw < tpr_max ? cw : tpr_max;
    L.rpp = RED_THREADS / L.tpr;
    L.ct = threadIdx.x % L.tpr; L.rl = threadIdx.x / L.tpr;
    L.cb = blockIdx.y * L.tpr;
    L.cc = L.cb + L.ct; L.c0 = L.cc * W;
    const int per = (rows + slices - 1) / slices;
    const int r0 = blockIdx.x * per;
    L.r = r0 + L.rl;
    L.r1 = min(rows, r0 + per);
    L.live = L.cc < cw && L.rl < L.rpp;
    return L;
}

// The epilogue: every thread's fp32 partials of two statistics (v[0 .. W - 1] and v[W .. 2 W - 1]) go to LDS as [statistic][row
// lane][column] (sh: 2 * W * RED_THREADS floats); then consecutive threads own consecutive COLUMNS -- a wave's 64 atomics cover
// 512 contiguous bytes (scattered f64 atomics, one thread adding its W columns, ran at a tenth of that rate) -- fold the row lanes
// in double and add the result to out[statistic][c] with one f64 atomic.  MAX: the fold is fmaxf over non-negative floats and ends
// in an atomic max (non-negative floats order like their bit patterns; out zero-filled).  The caller puts a barrier between two
// uses of sh.
template <int W, bool MAX, class Out>
__device__ __forceinline__ void red_fold(float* sh, const RedLane& L, const float (&v)[2 * W], int c, Out* __restrict__ out) {
    const int rpp = L.rpp, ncol = L.tpr * W;
    if (L.rl < rpp) {
#pragma unroll
        for (int j = 0; j < W; ++j) { sh[(0 * rpp + L.rl) * ncol + L.ct * W + j] = v[j]; sh[(1 * rpp + L.rl) * ncol + L.ct * W + j] = v[W + j]; }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * ncol; idx += RED_THREADS) {
        const int st = idx / ncol, col = idx - st * ncol;
        const int gc = L.cb * W + col;
        if (gc < c) {
            if constexpr (MAX) {
                float m = 0.f;
                for (int q = 0; q < rpp; ++q) m = fmaxf(m, sh[(st * rpp + q) * ncol + col]);
                if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(out + st * c + gc), __float_as_uint(m));
            } else {
                double d = 0;
                for (int q = 0; q < rpp; ++q) d += sh[(st * rpp + q) * ncol + col];
                atomicAdd(out + st * c + gc, d);
            }
        }
    }
}

}  // namespace glf

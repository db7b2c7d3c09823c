// What the TN ("reduction form") kernels and their second stage share: which tap a block row contracts, which slice of the
// reduction a workgroup owns (ONE chunk rule for the contraction kernels, the second-stage kernels and the host), the per-row
// state of a gathered reduction row, the fp32 store epilogue, and the summation of the partial slabs.
// gemm_f32.hip, gemm_bf16s.hip and gemm_f16s.hip take all of it; gemm_s16.hip takes the tap, the slice, the slab addressing
// and the launch rule (its second stage sums in fp32 with a grouping of its own).
//
// Every helper is __forceinline__ and takes scalars or a struct of scalars, never GemmArgs (gemm_common.h, GeoS).
#pragma once
#include <type_traits>
#include "gemm_common.h"

namespace {

// ---- the tap of a block row: the n-th set bit of the tap mask (n < popcount(mask)) --------------------------------------------
__device__ __forceinline__ int tn_tap(unsigned mask, int n) {
    for (int i = 0; i < n; ++i) mask &= mask - 1;
    return __ffs(mask) - 1;
}

// gathered B rows of a tap: source pixel = (y * stride + cy, x * stride + cx), two constants per workgroup
__device__ __forceinline__ void tn_tap_offsets(int tap, int kw, int pad, int dil, int& cy, int& cx) {
    int ky = 0, kx = tap;
    while (kx >= kw) { kx -= kw; ++ky; }
    cy = ky * dil - pad; cx = kx * dil - pad;
}

// ---- the slice of a workgroup ---------------------------------------------------------------------------------------------
// output pixels y (of hd) whose source pixel y * stride + o lies inside [0, hs): the band [lo, hi)
__host__ __device__ __forceinline__ void tap_band(int o, int stride, int hs, int hd, int& lo, int& hi) {
    lo = o < 0 ? (-o + stride - 1) / stride : 0;
    const int top = hs - 1 - o;
    hi = top < 0 ? 0 : (top / stride + 1 < hd ? top / stride + 1 : hd);
    if (lo > hi) lo = hi;
}

// Rectangle (y0, x0, h, w) of destination pixels the reduction of `tap` runs over, and its number of reduction rows.
// rect = 0: the whole map, K rows.  rect = 1: only the pixels whose source pixel is inside the map, enumerated image by image,
// row by row -- BAND = false: tap_rect() (stride 1; the fp32-storage kernels), BAND = true: tap_band() per axis (any stride;
// the bf16-storage kernel).
template <bool BAND>
__host__ __device__ __forceinline__ void tn_tap_rows(int rect, int tap, int K, const Geo& g, int& y0, int& x0, int& h, int& w, int& rows) {
    y0 = 0; x0 = 0; h = g.hd; w = g.wd; rows = K;
    if (!rect) return;
    int y1, x1;
    if (BAND) {
        const int ky = tap / g.kw, kx = tap - ky * g.kw;
        tap_band(ky * g.dil - g.pad, g.stride, g.hs, g.hd, y0, y1);
        tap_band(kx * g.dil - g.pad, g.stride, g.ws, g.wd, x0, x1);
    } else {
        tap_rect(1, tap, g.kw, g.pad, g.dil, g.hs, g.ws, g.hd, g.wd, y0, y1, x0, x1);
    }
    h = y1 - y0; w = x1 - x0;
    rows = (BAND ? K / (g.hd * g.wd) : g.n_img) * h * w;
}

// the number of reduction rows alone (the second stage and the host need no more)
template <bool BAND>
__host__ __device__ __forceinline__ int tn_tap_row_count(int rect, int tap, int K, const Geo& g) {
    int y0, x0, h, w, rows;
    tn_tap_rows<BAND>(rect, tap, K, g, y0, x0, h, w, rows);
    return rows;
}

// rows per slice: cut from the FULL reduction length K and rounded up to the K tile, the same for every tap -- a tap with a
// short rectangle uses fewer slices
__host__ __device__ __forceinline__ int tn_chunk(int K, int split, int ktile) {
    const int chunk = (K + split - 1) / split;
    return ((chunk + ktile - 1) / ktile) * ktile;
}

// slices of a tap with `rows` reduction rows that run (the others return early and write no slab)
__host__ __device__ __forceinline__ int tn_valid_slices(int rows, int K, int split, int ktile) {
    const int chunk = tn_chunk(K, split, ktile);
    const int n = chunk > 0 ? (rows + chunk - 1) / chunk : 0;
    return n < split ? n : split;
}

// z = blockIdx.z = bz * split + sl.  Rows [r0, r1) of the tap's `rows`; false = this workgroup has no work (block-uniform).
struct TnSlice { int bz, sl, y0, x0, h, w, rows, r0, r1; };

template <int KTILE, bool BAND>
__device__ __forceinline__ bool tn_slice(TnSlice& s, int z, int split, int K, int rect, int tap, const Geo& g) {
    s.bz = z / split; s.sl = z - s.bz * split;
    tn_tap_rows<BAND>(rect, tap, K, g, s.y0, s.x0, s.h, s.w, s.rows);
    const int chunk = tn_chunk(K, split, KTILE);
    s.r0 = s.sl * chunk;
    s.r1 = min(s.rows, s.r0 + chunk);
    return s.r0 < s.r1;
}

// Partial-sum slabs of the two-stage split-K reduction: every (batch, slice, kept tap) block row stores its own [M][N] slab
// (plain stores, no atomics, no zero fill); the second stage sums the slabs of a tap in a fixed order.  z = bz * split + sl,
// ord = ordinal of the tap among the ntap kept ones; the slices of one tap lie ntap * mn floats apart.
__device__ __forceinline__ float* tn_slab(float* partial, int z, int ntap, int ord, long long mn) {
    return partial + ((long long)z * ntap + ord) * mn;
}
__device__ __forceinline__ const float* tn_slab(const float* partial, int z, int ntap, int ord, long long mn) {
    return partial + ((long long)z * ntap + ord) * mn;
}

// ---- the row state of a staged reduction row --------------------------------------------------------------------------------
// What a gathered row needs of its tap and slice: the rectangle, the maps, and the two constant source offsets.
struct TnGather { int y0, x0, h, w, hs, ws, hd, wd, stride, cy, cx; };

// R rows, STEP rows apart, of the K tile a thread (or, with a wave-uniform first row, a wave) stages next: (n, y, x) inside the
// tap's rectangle.
template <int R> struct TnRows { int n[R], y[R], x[R]; };

// rows r, r + STEP, ...: by division, once
template <int R, int STEP>
__device__ __forceinline__ void tn_rows_init(TnRows<R>& s, int r, const TnGather& t) {
    const int hw = t.h * t.w;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int rj = r + STEP * j;
        s.n[j] = rj / hw;
        const int rem = rj - s.n[j] * hw;
        s.y[j] = rem / t.w; s.x[j] = rem - s.y[j] * t.w;
    }
}
// row j a K tile further on: by carrying (tiles are staged in order)
template <int KTILE, int R>
__device__ __forceinline__ void tn_row_step(TnRows<R>& s, int j, const TnGather& t) {
    s.x[j] += KTILE;
    while (s.x[j] >= t.w) { s.x[j] -= t.w; ++s.y[j]; }
    while (s.y[j] >= t.h) { s.y[j] -= t.h; ++s.n[j]; }
}
// rows of A (the destination pixel) and of B (the tap's source pixel; false = in the padding) of row j
template <int R>
__device__ __forceinline__ long long tn_row_dst(const TnRows<R>& s, int j, const TnGather& t) {
    const int y = t.y0 + s.y[j], x = t.x0 + s.x[j];
    return ((long long)s.n[j] * t.hd + y) * t.wd + x;
}
template <int R>
__device__ __forceinline__ bool tn_row_src(const TnRows<R>& s, int j, const TnGather& t, int& src) {
    const int sy = (t.y0 + s.y[j]) * t.stride + t.cy, sx = (t.x0 + s.x[j]) * t.stride + t.cx;
    src = (s.n[j] * t.hs + sy) * t.ws + sx;
    return (unsigned)sy < (unsigned)t.hs && (unsigned)sx < (unsigned)t.ws;
}

// ---- the fp32 store epilogue --------------------------------------------------------------------------------------------------
// max(*amax_c, cmax) from a wave.  PEEK: thousands of waves, ONE address -- only a wave that raises it issues the atomic.
template <bool PEEK>
__device__ __forceinline__ void tn_amax(float* amax_c, float cmax) {
    if (!amax_c) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
    if ((threadIdx.x & 63) == 0 && cmax > (PEEK ? *reinterpret_cast<volatile float*>(amax_c) : 0.f))
        atomicMax(reinterpret_cast<unsigned*>(amax_c), __float_as_uint(cmax));
}

// Where a workgroup's tile goes: its slab (row stride N) or C_tap of its batch element.  atomic: the one-stage path (split > 1
// or accumulate without a workspace) adds into C.  amax_c is honoured by plain stores into C only.
// tn_out() takes the slab's place from the launch grid itself: (tiles, kept taps, batch * split), as every TN launcher sizes it.
struct TnOut { float* C; float* amax_c; int ldc, M, N, tm, tn; bool atomic; float alpha; };

__device__ __forceinline__ TnOut tn_out(float* partial, float* C, float* amax_c, int M, int N, int ldc, long long bsc, long long tsb,
                                        int bz, int tap, int split, int accumulate, int tm, int tn, float alpha) {
    TnOut o;
    o.C = partial ? tn_slab(partial, blockIdx.z, gridDim.y, blockIdx.y, (long long)M * N) : C + (long long)bz * bsc + (long long)tap * tsb;
    o.ldc = partial ? N : ldc;
    o.atomic = !partial && (split > 1 || accumulate);
    o.amax_c = (partial || o.atomic) ? nullptr : amax_c;
    o.M = M; o.N = N; o.tm = tm; o.tn = tn; o.alpha = alpha;
    return o;
}

// one 32 x 32 accumulator block at (wrow, wcol) of the TBM_ x TBN_ tile: the lane holds column (lane & 31), rows
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
template <int TBM_, int TBN_>
__device__ __forceinline__ void tn_emit(const TnOut& o, const f32x16& acc, int wrow, int wcol, float& cmax) {
    const int lane = threadIdx.x & 63;
    const int col = o.tn * TBN_ + wcol + (lane & 31);
    if (col >= o.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = o.tm * TBM_ + wrow + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < o.M) {
            float* dst = o.C + (long long)row * o.ldc + col;
            const float v = o.alpha * acc[r];
            if (o.atomic) atomicAdd(dst, v); else { *dst = v; cmax = fmaxf(cmax, fabsf(v)); }
        }
    }
}

// ---- the second stage -----------------------------------------------------------------------------------------------------------
// Sum of the nvalid slabs of one float4 group (sp = its place in slice 0), with SL slice lanes.  The slabs are added in double:
// the second stage must not add a rounding walk of its own to the slices' fp32 chains.
//   SL = 1: one thread, slice after slice on top of prev().  No barrier.  AHEAD: four loads in flight, added in the same order
//   (the same bits).  The parameter-layout store, whose threads walk tap after tap, takes it; under tn_reduce_kernel, whose
//   whole grid sweeps one slab at a time, it measured 60 % slower (profiles/tn_walk_ab.txt).
//   SL = 4 / 16: thread (ol, sl) of the 256 adds slices sl, sl + SL, ... in pairs; the lanes meet in LDS (sh) in lane order, prev()
//   is added last.  Two barriers: every thread of the workgroup calls it; the result is valid where sl == 0 && live.
// prev() = the float4 the destination holds, asked for only when accumulate is set.
// With one thread per float4 a layer-1 gradient (64 x 256 outputs, hundreds of slices) was a few thousand threads walking
// hundreds of loads one after the other -- ~100 us for 24 MB; hence the lanes.
template <int SL, bool AHEAD = true, typename Prev>
__device__ __forceinline__ float4 tn_sum_slabs(const float* sp, long long slice_stride, int nvalid, bool live, int accumulate, Prev prev,
                                               double (*sh)[256]) {
    constexpr int OG = 256 / SL;
    double ax = 0, ay = 0, az = 0, aw = 0;
    if constexpr (SL == 1) {
        if (!live) return make_float4(0.f, 0.f, 0.f, 0.f);
        if (accumulate) { const float4 o = prev(); ax = o.x; ay = o.y; az = o.z; aw = o.w; }
        int s_ = 0;
        for (; AHEAD && s_ + 4 <= nvalid; s_ += 4) {
            const float4 v0 = *reinterpret_cast<const float4*>(sp + (long long)s_ * slice_stride);
            const float4 v1 = *reinterpret_cast<const float4*>(sp + (long long)(s_ + 1) * slice_stride);
            const float4 v2 = *reinterpret_cast<const float4*>(sp + (long long)(s_ + 2) * slice_stride);
            const float4 v3 = *reinterpret_cast<const float4*>(sp + (long long)(s_ + 3) * slice_stride);
            ax += v0.x; ay += v0.y; az += v0.z; aw += v0.w;
            ax += v1.x; ay += v1.y; az += v1.z; aw += v1.w;
            ax += v2.x; ay += v2.y; az += v2.z; aw += v2.w;
            ax += v3.x; ay += v3.y; az += v3.z; aw += v3.w;
        }
        for (; s_ < nvalid; ++s_) {
            const float4 v = *reinterpret_cast<const float4*>(sp + (long long)s_ * slice_stride);
            ax += v.x; ay += v.y; az += v.z; aw += v.w;
        }
    } else {
        const int ol = threadIdx.x % OG, sl = threadIdx.x / OG;
        if (live) {
            int s_ = sl;
            for (; s_ + SL < nvalid; s_ += 2 * SL) {
                const float4 v0 = *reinterpret_cast<const float4*>(sp + (long long)s_ * slice_stride);
                const float4 v1 = *reinterpret_cast<const float4*>(sp + (long long)(s_ + SL) * slice_stride);
                ax += (double)v0.x + (double)v1.x; ay += (double)v0.y + (double)v1.y;
                az += (double)v0.z + (double)v1.z; aw += (double)v0.w + (double)v1.w;
            }
            for (; s_ < nvalid; s_ += SL) {
                const float4 v = *reinterpret_cast<const float4*>(sp + (long long)s_ * slice_stride);
                ax += v.x; ay += v.y; az += v.z; aw += v.w;
            }
        }
        sh[0][threadIdx.x] = ax; sh[1][threadIdx.x] = ay; sh[2][threadIdx.x] = az; sh[3][threadIdx.x] = aw;
        __syncthreads();
        if (sl == 0 && live) {
#pragma unroll
            for (int l = 1; l < SL; ++l) { ax += sh[0][l * OG + ol]; ay += sh[1][l * OG + ol]; az += sh[2][l * OG + ol]; aw += sh[3][l * OG + ol]; }
            if (accumulate) { const float4 o = prev(); ax += o.x; ay += o.y; az += o.z; aw += o.w; }
        }
        __syncthreads();
    }
    return make_float4((float)ax, (float)ay, (float)az, (float)aw);
}

__device__ __forceinline__ float amax4(float cmax, const float4 v) {
    return fmaxf(fmaxf(cmax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// ---- the launch rule of the second stage (host) ---------------------------------------------------------------------------------
// Slice lanes per output: enough threads to keep the slabs' loads in flight (work x lanes >= ~64 k threads), at most 16, only in
// the vector form.  work = outputs (float4 groups in the vector form); blocks = 256-thread workgroups that cover them once.
struct TnReducePlan { int lanes; long long blocks; };
inline TnReducePlan tn_reduce_plan(long long work, int split, bool vec) {
    int lanes = 1;
    while (vec && lanes < 16 && lanes * 4 <= split && work * lanes < 65536) lanes *= 4;
    return TnReducePlan{lanes, (work * lanes + 255) / 256};
}
// f(std::integral_constant<int, SL>) for SL = lanes
template <typename F>
inline void tn_by_lanes(int lanes, F&& f) {
    if (lanes == 16) f(std::integral_constant<int, 16>{});
    else if (lanes == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 1>{});
}

}  // namespace

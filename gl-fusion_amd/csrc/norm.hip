// Normalisation kernels of the GL-Fusion path for BOTH storages (HBM-bound; channels-last [rows][C]; fp32 storage: C % 4 == 0,
// bf16 storage -- the glf_s16_* entry points -- C % 8 == 0: 16-byte accesses either way, fp32 arithmetic, bf16 rounded once at the store).
//   * column reductions (BatchNorm statistics, BatchNorm / LayerNorm / bias gradients) share one
//     two-stage scheme: stage 1 streams a slice of rows per workgroup with 16-byte loads and
//     accumulates in f64 (sum / sum-of-squares cancellation-free), stage 2 folds the per-slice
//     partials per channel.  No atomics => bitwise reproducible.
//   * the single-stage reductions (one f64 atomic per column and workgroup: BatchNorm backward of both storages, statistics and
//     column sum of bf16 storage) and the statistics finish are written once for both storages (col_reduce.h, bn_finish).
//   * BatchNorm apply (+residual, +ReLU) and the backward apply are single streaming passes.
//   * the TPAVI tail z = LayerNorm_C(BN(W_z y) + x) runs one wavefront per row with shuffle
//     reductions only (no LDS, no barrier); its backward with every column sum that follows from du is one walk in which a
//     workgroup owns a slab of rows and each wave a quarter of the channels (bn_res_ln_bwd_sums_kernel).
#include "col_reduce.h"
#include "split_f16.h"

using namespace glf;

namespace {

constexpr int RT = RED_THREADS;       // threads of a reduction workgroup
constexpr int MAX_SLICES = 1024;

// row slices of the stage-1 grid: enough workgroups to stream at the HBM rate (grid = slices x channel blocks of
// up to 1024 channels) while the f64 partials stay small (2 x slices x C x 8 B; 33 MB per BatchNorm at C = 2048 with
// 1024 slices made the stage-2 kernels 2 % of the step)
__host__ __device__ inline int n_slices_c(int rows, int c) {
    int s = (rows + 31) / 32;
    int cap = 524288 / (c > 0 ? c : 1);
    if (cap < 128) cap = 128;
    if (cap > MAX_SLICES) cap = MAX_SLICES;
    return s < 1 ? 1 : (s > cap ? cap : s);
}

struct Coef { const float* mean; const float* invstd; const float* gamma; const float* beta; };

// ---- functors: two values per element --------------------------------------------------
struct OpStats {          // (x, x^2)
    const float* x; int ldx;
    __device__ void operator()(int r, int c, float4& a, float4& b) const {
        a = *reinterpret_cast<const float4*>(x + (long long)r * ldx + c);
        b = make_float4(a.x * a.x, a.y * a.y, a.z * a.z, a.w * a.w);
    }
};
struct OpColsum {         // (dy, 0)
    const float* dy; int ld;
    __device__ void operator()(int r, int c, float4& a, float4& b) const {
        a = *reinterpret_cast<const float4*>(dy + (long long)r * ld + c);
        b = make_float4(0.f, 0.f, 0.f, 0.f);
    }
};
struct OpStats16 {        // bf16 storage: (x, x^2)
    const u16* x; int ldx;
    __device__ void operator()(int r, int c, F8& a, F8& b) const {
        a = ld8(x + (long long)r * ldx + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) b.v[j] = a.v[j] * a.v[j];
    }
};
struct OpColsum16 {       // bf16 storage: (dy, 0)
    const u16* dy; int ld;
    __device__ void operator()(int r, int c, F8& a, F8& b) const {
        a = ld8(dy + (long long)r * ld + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) b.v[j] = 0.f;
    }
};
// the forward value of one element; ONE definition so that the ReLU mask recomputed in backward (y == NULL) is the
// mask the forward applied
__device__ __forceinline__ float bn_val(float x, float mu, float is, float ga, float be) { return (x - mu) * is * ga + be; }

// operands of a BatchNorm-backward reduction over storage type T, W = 16 / sizeof(T) elements per access
template <class T> struct BnBwdIn {
    const T* dy; int lddy; const T* x; int ldx; const T* y; int ldy;
    const float* mean; const float* invstd; const float* gamma; const float* beta; int relu;
    const unsigned char* mask; int cw;          // relu with a residual: the forward's sign bits, one byte per access (instead of y)
    const T* dy2; int lddy2;                    // second addend of the incoming gradient (a fan-in not yet summed), or null
};
struct OpBnBwd : BnBwdIn<float> {   // (dy', dy' * xhat), dy' = dy * (y > 0) when relu; y == NULL: the mask is recomputed from x
    __device__ void operator()(int r, int c, float4& a, float4& b) const {
        a = *reinterpret_cast<const float4*>(dy + (long long)r * lddy + c);
        if (dy2) {
            const float4 a2 = *reinterpret_cast<const float4*>(dy2 + (long long)r * lddy2 + c);
            a.x += a2.x; a.y += a2.y; a.z += a2.z; a.w += a2.w;
        }
        const float4 xx = *reinterpret_cast<const float4*>(x + (long long)r * ldx + c);
        const float4 mu = *reinterpret_cast<const float4*>(mean + c);
        const float4 is = *reinterpret_cast<const float4*>(invstd + c);
        if (relu && mask) {
            const unsigned m = mask[(long long)r * cw + (c >> 2)];
            a.x = (m & 1u) ? a.x : 0.f; a.y = (m & 2u) ? a.y : 0.f; a.z = (m & 4u) ? a.z : 0.f; a.w = (m & 8u) ? a.w : 0.f;
        } else if (relu) {
            float4 yy;
            if (y) {
                yy = *reinterpret_cast<const float4*>(y + (long long)r * ldy + c);
            } else {
                const float4 ga = *reinterpret_cast<const float4*>(gamma + c);
                const float4 be = *reinterpret_cast<const float4*>(beta + c);
                yy = make_float4(bn_val(xx.x, mu.x, is.x, ga.x, be.x), bn_val(xx.y, mu.y, is.y, ga.y, be.y),
                                 bn_val(xx.z, mu.z, is.z, ga.z, be.z), bn_val(xx.w, mu.w, is.w, ga.w, be.w));
            }
            a.x = yy.x > 0.f ? a.x : 0.f; a.y = yy.y > 0.f ? a.y : 0.f;
            a.z = yy.z > 0.f ? a.z : 0.f; a.w = yy.w > 0.f ? a.w : 0.f;
        }
        b = make_float4(a.x * (xx.x - mu.x) * is.x, a.y * (xx.y - mu.y) * is.y,
                        a.z * (xx.z - mu.z) * is.z, a.w * (xx.w - mu.w) * is.w);
    }
};
struct OpLnParam {        // (dz * uhat, dz) with u = BN(w) + x and per-row LayerNorm statistics
    const float* dz; const float* w; const float* x; Coef bn; const float* row_mean; const float* row_rstd; int c_total;
    __device__ void operator()(int r, int c, float4& a, float4& b) const {
        const long long o = (long long)r * c_total + c;
        b = *reinterpret_cast<const float4*>(dz + o);
        const float4 ww = *reinterpret_cast<const float4*>(w + o);
        const float4 xx = *reinterpret_cast<const float4*>(x + o);
        const float4 mu = *reinterpret_cast<const float4*>(bn.mean + c);
        const float4 is = *reinterpret_cast<const float4*>(bn.invstd + c);
        const float4 ga = *reinterpret_cast<const float4*>(bn.gamma + c);
        const float4 be = *reinterpret_cast<const float4*>(bn.beta + c);
        const float m = row_mean[r], rs = row_rstd[r];
        const float u0 = (ww.x - mu.x) * is.x * ga.x + be.x + xx.x;
        const float u1 = (ww.y - mu.y) * is.y * ga.y + be.y + xx.y;
        const float u2 = (ww.z - mu.z) * is.z * ga.z + be.z + xx.z;
        const float u3 = (ww.w - mu.w) * is.w * ga.w + be.w + xx.w;
        a = make_float4(b.x * (u0 - m) * rs, b.y * (u1 - m) * rs, b.z * (u2 - m) * rs, b.w * (u3 - m) * rs);
    }
};

// stage 1: partial[0][slice][c], partial[1][slice][c]
// MAXIMA (Op = OpBnBwd): two more per-channel reductions over the same elements, max |dy'| and max |xhat|.  They cost no memory
// traffic (the values are in registers for the sums) and let the finalize kernel bound max |dx| BEFORE dx is written -- which is
// what allows bn_bwd_apply to emit dx directly as the packed pre-split fp16 image the consuming contractions read (the image's
// power-of-two scale must be known when the first element is written).
// pmax[0][slice][c] = max |dy'|, pmax[1][slice][c] = max |xhat| (floats, behind the f64 partials).
template <class Op, bool MAXIMA = false>
__global__ __launch_bounds__(RT) void colreduce_kernel(Op op, int rows, int c, int slices, double* __restrict__ partial, float* __restrict__ pmax) {
    __shared__ double sh_a[RT * 4];
    __shared__ double sh_b[RT * 4];
    __shared__ float sh_m[MAXIMA ? RT * 8 : 1];
    const int tid = threadIdx.x, slice = blockIdx.x;
    const RedLane L = red_lane<4>(rows, c, slices, RT);      // column blocks of up to RT float4
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    float mg[4] = {0.f, 0.f, 0.f, 0.f}, mx[4] = {0.f, 0.f, 0.f, 0.f};
    if (L.live) {
        float4 mu, is;
        if constexpr (MAXIMA) { mu = *reinterpret_cast<const float4*>(op.mean + L.c0); is = *reinterpret_cast<const float4*>(op.invstd + L.c0); }
        for (int r = L.r; r < L.r1; r += L.rpp) {
            float4 a, b;
            op(r, L.c0, a, b);
            a0 += a.x; a1 += a.y; a2 += a.z; a3 += a.w;
            b0 += b.x; b1 += b.y; b2 += b.z; b3 += b.w;
            if constexpr (MAXIMA) {
                const float4 xx = *reinterpret_cast<const float4*>(op.x + (long long)r * op.ldx + L.c0);   // (the load op() made: CSE'd)
                mg[0] = fmaxf(mg[0], fabsf(a.x)); mg[1] = fmaxf(mg[1], fabsf(a.y)); mg[2] = fmaxf(mg[2], fabsf(a.z)); mg[3] = fmaxf(mg[3], fabsf(a.w));
                mx[0] = fmaxf(mx[0], fabsf((xx.x - mu.x) * is.x)); mx[1] = fmaxf(mx[1], fabsf((xx.y - mu.y) * is.y));
                mx[2] = fmaxf(mx[2], fabsf((xx.z - mu.z) * is.z)); mx[3] = fmaxf(mx[3], fabsf((xx.w - mu.w) * is.w));
            }
        }
    }
    sh_a[tid * 4 + 0] = a0; sh_a[tid * 4 + 1] = a1; sh_a[tid * 4 + 2] = a2; sh_a[tid * 4 + 3] = a3;
    sh_b[tid * 4 + 0] = b0; sh_b[tid * 4 + 1] = b1; sh_b[tid * 4 + 2] = b2; sh_b[tid * 4 + 3] = b3;
    if constexpr (MAXIMA) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { sh_m[tid * 8 + j] = mg[j]; sh_m[tid * 8 + 4 + j] = mx[j]; }
    }
    __syncthreads();
    if (L.rl == 0 && L.live) {
#pragma unroll 2      // (left to the compiler, this fold's unrolling took the whole kernel from 8 waves per SIMD to 6)
        for (int q = 1; q < L.rpp; ++q) {
            const int o = (q * L.tpr + L.ct) * 4;
            a0 += sh_a[o]; a1 += sh_a[o + 1]; a2 += sh_a[o + 2]; a3 += sh_a[o + 3];
            b0 += sh_b[o]; b1 += sh_b[o + 1]; b2 += sh_b[o + 2]; b3 += sh_b[o + 3];
            if constexpr (MAXIMA) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { mg[j] = fmaxf(mg[j], sh_m[2 * o + j]); mx[j] = fmaxf(mx[j], sh_m[2 * o + 4 + j]); }
            }
        }
        double* pa = partial + (long long)slice * c + L.c0;
        double* pb = partial + (long long)(slices + slice) * c + L.c0;
        pa[0] = a0; pa[1] = a1; pa[2] = a2; pa[3] = a3;
        pb[0] = b0; pb[1] = b1; pb[2] = b2; pb[3] = b3;
        if constexpr (MAXIMA) {
            *reinterpret_cast<float4*>(pmax + (long long)slice * c + L.c0) = make_float4(mg[0], mg[1], mg[2], mg[3]);
            *reinterpret_cast<float4*>(pmax + (long long)(slices + slice) * c + L.c0) = make_float4(mx[0], mx[1], mx[2], mx[3]);
        }
    }
}

// ---- the same reductions WITHOUT a second stage, for both storages (col_reduce.h: red_geom, red_lane, red_fold): per-thread fp32
// partial sums over its <= ~16-64 rows (four rows' loads in flight at a time), the workgroup's row lanes folded in double through
// LDS, then ONE f64 atomic per column, statistic and workgroup into a zero-filled [2][c] buffer -- the same contract as
// glf_gemm_params.colstats, so a BatchNorm takes its sums from the producing contraction's epilogue or from a kernel here alike,
// and the apply kernels finish the statistics in their prologue: two launches per BatchNorm backward instead of three (the
// finalize kernels were 221 launches of ~14 us per step).

// generic two-value reduction of bf16 storage (statistics, column sum): op(r, c0, a, b)
template <class Op>
__global__ __launch_bounds__(RT) void s16_colreduce_kernel(Op op, int rows, int c, int slices, double* __restrict__ sums) {
    __shared__ float sh[RT * 16];
    const RedLane L = red_lane<8>(rows, c, slices, RED_TPR);
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    if (L.live) {
        const int rpp = L.rpp, c0 = L.c0;
        int r = L.r;
        for (; r + 3 * rpp < L.r1; r += 4 * rpp) {
            F8 a0, b0, a1, b1, a2, b2, a3, b3;
            op(r, c0, a0, b0); op(r + rpp, c0, a1, b1); op(r + 2 * rpp, c0, a2, b2); op(r + 3 * rpp, c0, a3, b3);
#pragma unroll
            for (int j = 0; j < 8; ++j) { acc[j] += (a0.v[j] + a1.v[j]) + (a2.v[j] + a3.v[j]); acc[8 + j] += (b0.v[j] + b1.v[j]) + (b2.v[j] + b3.v[j]); }
        }
        for (; r < L.r1; r += rpp) {
            F8 a, b;
            op(r, c0, a, b);
#pragma unroll
            for (int j = 0; j < 8; ++j) { acc[j] += a.v[j]; acc[8 + j] += b.v[j]; }
        }
    }
    red_fold<8, false>(sh, L, acc, c, sums);
}

// BatchNorm backward: sums[0][c] += sum dy', sums[1][c] += sum dy' xhat with dy' = (dy + dy2) * relu-mask, over storage T with
// W = 16 / sizeof(T) elements per access and W sign bits per mask byte.
// HAS2: second gradient addend; RM: 0 = no ReLU, 1 = sign bytes, 2 = sign recomputed from x, 3 = sign of the saved output y.
// WRES: the masked gradient is stored to dres while it is in registers -- the apply pass then reads that ONE tensor instead of dy,
// dy2 and the sign bytes again (dres must not alias dy, dy2 or x: other rows of them are still to be read).
// fp32 storage with cmax != null: also one atomic max per column for max |dy'| and max |xhat|, which the packed-gradient bound
// needs (bf16 storage has no packed image: compiled out).  bf16 storage instantiates RM 0 .. 2 without WRES.
// The coefficient vectors are loaded once; the loads of FOUR rows (8-12 x 16 bytes per lane) are issued back to back before any
// arithmetic (through a generic op() the compiler emitted one dependent load -> wait chain per row -- five s_waitcnt vmcnt(0)
// per row, 2.3 TB/s -- with the coefficient vectors re-loaded for every row).
template <class T, bool HAS2, int RM, bool WRES>
__global__ __launch_bounds__(RT) void bnbwd_reduce_atomic_kernel(BnBwdIn<T> op, int rows, int c, int slices, double* __restrict__ sums,
                                                                 float* __restrict__ cmax, T* __restrict__ dres, int lddres) {
    constexpr int W = 16 / sizeof(T);
    constexpr bool MAXIMA = sizeof(T) == 4;
    typedef Stream<T, W> S;
    typedef typename S::Raw Raw;
    __shared__ float sh[RT * 2 * W];              // [statistic][row lane][column] for the sums, reused for the maxima
    const RedLane L = red_lane<W>(rows, c, slices, RED_TPR);
    // (sum dy', sum dy' xhat) and (max |dy'|, max |xhat|), each pair as ONE array: as two FV<W> the bf16 <false, 2> instantiation
    // compiled to 160 VGPRs instead of 127 and lost its fourth wave (profiles/bn_merge_resources.txt)
    float acc[2 * W], top[2 * W];
#pragma unroll
    for (int j = 0; j < 2 * W; ++j) acc[j] = top[j] = 0.f;
    if (L.live) {
        const int c0 = L.c0, cc = L.cc, rpp = L.rpp;
        const FV<W> mu = Stream<float, W>::ld(op.mean + c0), is = Stream<float, W>::ld(op.invstd + c0);
        FV<W> ga = mu, be = mu;
        if (RM == 2) { ga = Stream<float, W>::ld(op.gamma + c0); be = Stream<float, W>::ld(op.beta + c0); }
        auto fold = [&](long long row, const Raw qa, const Raw qa2, const Raw qx, const Raw qy, unsigned m) __attribute__((always_inline)) {
            FV<W> a = S::unpack(qa);
            if (HAS2) {
                const FV<W> a2 = S::unpack(qa2);
#pragma unroll
                for (int j = 0; j < W; ++j) a.v[j] += a2.v[j];
            }
            const FV<W> xx = S::unpack(qx);
            if (RM == 2 || RM == 3) {
                const FV<W> yy = S::unpack(qy);
                m = 0;
#pragma unroll
                for (int j = 0; j < W; ++j) m |= ((RM == 2 ? bn_val(xx.v[j], mu.v[j], is.v[j], ga.v[j], be.v[j]) : yy.v[j]) > 0.f ? 1u : 0u) << j;
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                a.v[j] = (RM == 0 || ((m >> j) & 1u)) ? a.v[j] : 0.f;
                acc[j] += a.v[j];
                acc[W + j] += a.v[j] * (xx.v[j] - mu.v[j]) * is.v[j];
            }
            if (WRES) S::st(dres + row * lddres + c0, a);
            if (MAXIMA && cmax) {
#pragma unroll
                for (int j = 0; j < W; ++j) { top[j] = fmaxf(top[j], fabsf(a.v[j])); top[W + j] = fmaxf(top[W + j], fabsf((xx.v[j] - mu.v[j]) * is.v[j])); }
            }
        };
        int r = L.r;
        for (; r + 3 * rpp < L.r1; r += 4 * rpp) {
            Raw qa[4], qa2[4], qx[4], qy[4];
            unsigned m[4] = {0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long row = r + u * rpp;
                qa[u] = S::ldraw(op.dy + row * op.lddy + c0);
                if (HAS2) qa2[u] = S::ldraw(op.dy2 + row * op.lddy2 + c0);
                qx[u] = S::ldraw(op.x + row * op.ldx + c0);
                if (RM == 3) qy[u] = S::ldraw(op.y + row * op.ldy + c0);
                if (RM == 1) m[u] = op.mask[row * op.cw + cc];
            }
            __builtin_amdgcn_sched_barrier(0);       // every load of the four rows is in flight before the first use (hipcc sinks them to their uses)
#pragma unroll
            for (int u = 0; u < 4; ++u) fold(r + u * rpp, qa[u], HAS2 ? qa2[u] : qa[u], qx[u], RM == 3 ? qy[u] : qx[u], m[u]);
        }
        for (; r < L.r1; r += rpp) {
            const long long row = r;
            const Raw qa = S::ldraw(op.dy + row * op.lddy + c0);
            const Raw qa2 = HAS2 ? S::ldraw(op.dy2 + row * op.lddy2 + c0) : qa;
            const Raw qx = S::ldraw(op.x + row * op.ldx + c0);
            const Raw qy = RM == 3 ? S::ldraw(op.y + row * op.ldy + c0) : qx;
            fold(row, qa, qa2, qx, qy, RM == 1 ? op.mask[row * op.cw + cc] : 0u);
        }
    }
    red_fold<W, false>(sh, L, acc, c, sums);
    if (MAXIMA && cmax) {
        __syncthreads();
        red_fold<W, true>(sh, L, top, c, cmax);
    }
}
// one dispatch ladder for both storages: cmax and dres are fp32-storage extras (null for bf16)
template <class T>
int launch_bnbwd_reduce(const BnBwdIn<T>& op, int rows, int c, double* sums, float* cmax, T* dres, int lddres, hipStream_t s, const char* what) {
    constexpr int W = 16 / sizeof(T);
    const RedGeom g = red_geom<W>(rows, c);
    const int rm = !op.relu ? 0 : (op.mask ? 1 : (op.y ? 3 : 2));
#define GLF_BNR(H2, RM_, WR) hipLaunchKernelGGL((bnbwd_reduce_atomic_kernel<T, H2, RM_, WR>), red_grid(g), dim3(RT), 0, s, op, rows, c, g.slices, sums, cmax, dres, lddres)
#define GLF_BNR_RM(H2, WR) do { if (rm == 0) GLF_BNR(H2, 0, WR); else if (rm == 1) GLF_BNR(H2, 1, WR); else if (rm == 2) GLF_BNR(H2, 2, WR); \
                                else if constexpr (W == 4) GLF_BNR(H2, 3, WR); } while (0)
    if constexpr (W == 4) { if (dres) { GLF_BNR_RM(true, true); return glf::check_launch(what); } }
    if (op.dy2) GLF_BNR_RM(true, false); else GLF_BNR_RM(false, false);
#undef GLF_BNR_RM
#undef GLF_BNR
    return glf::check_launch(what);
}

// stage 2: fold the per-slice partials.  One workgroup = 16 channels x 16 slice lanes (a serial loop over
// up to 1024 slices per channel on a single thread was 13% of the whole step in the first profile).
constexpr int FIN_CH = 16, FIN_LANES = 16;

__device__ __forceinline__ void fold_partials(const double* __restrict__ partial, int slices, int c, int ch, int lane,
                                              double& s, double& q, double* sh) {
    s = 0; q = 0;
    if (ch < c) {
        double s1 = 0, q1 = 0, s2 = 0, q2 = 0, s3 = 0, q3 = 0;      // four independent chains: the loop is latency-bound
        int i = lane;
        for (; i + 3 * FIN_LANES < slices; i += 4 * FIN_LANES) {
            s += partial[(long long)i * c + ch];                     q += partial[(long long)(slices + i) * c + ch];
            s1 += partial[(long long)(i + FIN_LANES) * c + ch];      q1 += partial[(long long)(slices + i + FIN_LANES) * c + ch];
            s2 += partial[(long long)(i + 2 * FIN_LANES) * c + ch];  q2 += partial[(long long)(slices + i + 2 * FIN_LANES) * c + ch];
            s3 += partial[(long long)(i + 3 * FIN_LANES) * c + ch];  q3 += partial[(long long)(slices + i + 3 * FIN_LANES) * c + ch];
        }
        for (; i < slices; i += FIN_LANES) {
            s += partial[(long long)i * c + ch];
            q += partial[(long long)(slices + i) * c + ch];
        }
        s += (s1 + s2) + s3; q += (q1 + q2) + q3;
    }
    const int t = threadIdx.x;
    sh[t] = s; sh[256 + t] = q;
    __syncthreads();
    if (lane == 0) {
        for (int l = 1; l < FIN_LANES; ++l) { s += sh[t + l * FIN_CH]; q += sh[256 + t + l * FIN_CH]; }
    }
}

// Finishing a batch statistic, written ONCE: every kernel that turns (sum x, sum x^2) of a channel into mean / invstd -- the
// finalize kernel here and the prologues of bn_apply_sums_kernel and s16_bn_apply_kernel -- calls these, so their results are
// bit-identical by construction (-ffp-contract=fast chooses contractions per context).
struct BnStat { float mean, invstd; double var; };      // var: the biased batch variance, clamped at 0
__device__ __forceinline__ BnStat bn_finish(double sum, double sumsq, int rows, float eps) {
    const double m = sum / rows;
    double var = sumsq / rows - m * m;
    if (var < 0) var = 0;
    return {(float)m, (float)(1.0 / sqrt(var + (double)eps)), var};
}
__device__ __forceinline__ void bn_running_update(const BnStat& st, int rows, float momentum, float& rmean, float& rvar) {
    const double unb = rows > 1 ? st.var * rows / (rows - 1) : st.var;
    rmean = (1.f - momentum) * rmean + momentum * st.mean;
    rvar = (1.f - momentum) * rvar + momentum * (float)unb;
}

__global__ __launch_bounds__(256) void bn_stats_finalize(const double* __restrict__ partial, int slices, int c, int rows, float eps,
                                                         float momentum, float* mean, float* invstd, float* rmean, float* rvar, long long* nbt) {
    __shared__ double sh[512];
    const int cx = threadIdx.x % FIN_CH, lane = threadIdx.x / FIN_CH;
    const int ch = blockIdx.x * FIN_CH + cx;
    double s, q;
    fold_partials(partial, slices, c, ch, lane, s, q, sh);
    if (lane != 0 || ch >= c) return;
    if (ch == 0 && nbt) *nbt += 1;
    const BnStat st = bn_finish(s, q, rows, eps);
    mean[ch] = st.mean;
    invstd[ch] = st.invstd;
    if (rmean) bn_running_update(st, rows, momentum, rmean[ch], rvar[ch]);
}

// out_a[ch] = sum of first partial, out_b[ch] = sum of second (either may be NULL)
__device__ __forceinline__ void sum_finalize_body(const double* __restrict__ partial, int slices, int c, float* out_a, float* out_b) {
    __shared__ double sh[512];
    const int cx = threadIdx.x % FIN_CH, lane = threadIdx.x / FIN_CH;
    const int ch = blockIdx.x * FIN_CH + cx;
    double s, q;
    fold_partials(partial, slices, c, ch, lane, s, q, sh);
    if (lane != 0 || ch >= c) return;
    if (out_a) out_a[ch] = (float)s;
    if (out_b) out_b[ch] = (float)q;
}
__global__ __launch_bounds__(256) void sum_finalize(const double* __restrict__ partial, int slices, int c, float* out_a, float* out_b) {
    sum_finalize_body(partial, slices, c, out_a, out_b);
}

// BatchNorm-backward stage 2 for the packed-dx path: the two sums, and an upper bound of max |dx| over the whole tensor into
// *bound (a zeroed device float; non-negative floats order like their bit patterns):
//   training: |dx| = |gamma invstd| |g - (s1 + xhat s2) / n| <= |gamma invstd| (max|g| + (|s1| + max|xhat| |s2|) / n)   per channel
//   eval    : |dx| = |gamma invstd| |g|
// (x 1.0001: the apply kernel rounds its fp32 expression differently; the image's power-of-two scale leaves two bits of
// fp16 headroom above the bound anyway)
__device__ __forceinline__ void bnbwd_finalize_body(const double* __restrict__ partial, const float* __restrict__ pmax, int slices, int c,
                                                    const float* __restrict__ gamma, const float* __restrict__ invstd, float inv_n,
                                                    int training, float* out_a, float* out_b, float* __restrict__ bound,
                                                    float* __restrict__ keep) {
    __shared__ double sh[512];
    __shared__ float shm[512];
    const int cx = threadIdx.x % FIN_CH, lane = threadIdx.x / FIN_CH;
    const int ch = blockIdx.x * FIN_CH + cx;
    double s, q;
    fold_partials(partial, slices, c, ch, lane, s, q, sh);
    float mg = 0.f, mx = 0.f;
    if (ch < c) {
        float g1 = 0.f, x1 = 0.f, g2 = 0.f, x2 = 0.f, g3 = 0.f, x3 = 0.f;       // independent chains: the loop is latency-bound
        int i = lane;
        for (; i + 3 * FIN_LANES < slices; i += 4 * FIN_LANES) {
            mg = fmaxf(mg, pmax[(long long)i * c + ch]);                      mx = fmaxf(mx, pmax[(long long)(slices + i) * c + ch]);
            g1 = fmaxf(g1, pmax[(long long)(i + FIN_LANES) * c + ch]);        x1 = fmaxf(x1, pmax[(long long)(slices + i + FIN_LANES) * c + ch]);
            g2 = fmaxf(g2, pmax[(long long)(i + 2 * FIN_LANES) * c + ch]);    x2 = fmaxf(x2, pmax[(long long)(slices + i + 2 * FIN_LANES) * c + ch]);
            g3 = fmaxf(g3, pmax[(long long)(i + 3 * FIN_LANES) * c + ch]);    x3 = fmaxf(x3, pmax[(long long)(slices + i + 3 * FIN_LANES) * c + ch]);
        }
        for (; i < slices; i += FIN_LANES) {
            mg = fmaxf(mg, pmax[(long long)i * c + ch]);
            mx = fmaxf(mx, pmax[(long long)(slices + i) * c + ch]);
        }
        mg = fmaxf(fmaxf(mg, g1), fmaxf(g2, g3)); mx = fmaxf(fmaxf(mx, x1), fmaxf(x2, x3));
    }
    shm[threadIdx.x] = mg; shm[256 + threadIdx.x] = mx;
    __syncthreads();
    if (lane != 0 || ch >= c) return;
    for (int l = 1; l < FIN_LANES; ++l) { mg = fmaxf(mg, shm[threadIdx.x + l * FIN_CH]); mx = fmaxf(mx, shm[256 + threadIdx.x + l * FIN_CH]); }
    if (out_a) out_a[ch] = (float)s;
    if (out_b) out_b[ch] = (float)q;
    if (keep) { keep[ch] = (float)s; keep[c + ch] = (float)q; }       // the caller's own copy for a later apply pass (packed_dx = 2)
    const float k = fabsf(gamma[ch] * invstd[ch]);
    const float b = 1.0001f * k * (training ? mg + inv_n * (fabsf((float)s) + mx * fabsf((float)q)) : mg);
    if (bound && b > 0.f && b < 3.0e38f) atomicMax(reinterpret_cast<unsigned*>(bound), __float_as_uint(b));
}
__global__ __launch_bounds__(256) void bnbwd_finalize(const double* __restrict__ partial, const float* __restrict__ pmax, int slices, int c,
                                                      const float* __restrict__ gamma, const float* __restrict__ invstd, float inv_n,
                                                      int training, float* out_a, float* out_b, float* __restrict__ bound,
                                                      float* __restrict__ keep) {
    bnbwd_finalize_body(partial, pmax, slices, c, gamma, invstd, inv_n, training, out_a, out_b, bound, keep);
}
// stage 2 of the fusion-block tail backward (bn_res_ln_bwd_sums_kernel): blockIdx.y = 0 finishes the LayerNorm parameter gradients
// (sum_finalize's work on the first pair of partials), blockIdx.y = 1 the BatchNorm sums, the kept copy and the bound of the packed
// dx image (bnbwd_finalize's work on the second pair) -- one launch
__global__ __launch_bounds__(256) void tail_bwd_finalize(const double* __restrict__ partial, const float* __restrict__ pmax, int slices, int c,
                                                         const float* __restrict__ gamma, const float* __restrict__ invstd, float inv_n,
                                                         int training, float* dln_g, float* dln_b, float* dbn_b, float* dbn_g,
                                                         float* __restrict__ bound, float* __restrict__ keep) {
    if (blockIdx.y == 0) sum_finalize_body(partial, slices, c, dln_g, dln_b);
    else bnbwd_finalize_body(partial + (size_t)2 * slices * c, pmax, slices, c, gamma, invstd, inv_n, training, dbn_b, dbn_g, bound, keep);
}

// running-statistics update of a train-mode BatchNorm replayed from its saved batch statistics (mean, invstd): what a second
// forward over the same input would have done to running_mean / running_var / num_batches_tracked
__global__ void bn_replay_kernel(const float* __restrict__ mean, const float* __restrict__ invstd, int rows, float eps, float momentum,
                                 float* rmean, float* rvar, long long* nbt, int c) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch == 0 && nbt) *nbt += 1;
    if (ch >= c) return;
    const double is = (double)invstd[ch];
    double var = 1.0 / (is * is) - (double)eps;
    if (var < 0) var = 0;
    const double unb = rows > 1 ? var * rows / (rows - 1) : var;
    rmean[ch] = (1.f - momentum) * rmean[ch] + momentum * mean[ch];
    rvar[ch] = (1.f - momentum) * rvar[ch] + momentum * (float)unb;
}

__global__ void bn_eval_coeffs_kernel(const float* rm, const float* rv, float eps, float* mean, float* invstd, int c) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    mean[ch] = rm[ch];
    invstd[ch] = 1.0f / sqrtf(rv[ch] + eps);
}

// ---- streaming applies ------------------------------------------------------------------
// Column-owning form (the layout bnbwd_reduce_atomic_kernel uses): a workgroup covers one column block of `tpr` float4 lanes and
// one slice of rows; a thread owns four consecutive channels for the whole kernel, keeps their coefficients in registers and
// walks down its rows with the loads of four rows issued before the first use.  No division and no coefficient load in the row
// loop (the flat grid-stride form paid a 64-bit division by c4 and four to six coefficient float4 loads per element).
// A full wave per row from 256 channels on (1 KB contiguous per wave and row, 64 contiguous sign bytes), 16 lanes below.
constexpr int APPLY_TPR = 16, APPLY_TPR_WIDE = 64;
constexpr int APPLY_MAXCOL = APPLY_TPR_WIDE * 4;      // channels of the widest column block

struct ColGrid { int tpr, cblocks, slices; };
// grid = row slices x column blocks, as many workgroups as stream_grid gives the flat pass (blockIdx.x = slice * cblocks + block)
inline ColGrid col_grid(int rows, int c) {
    const int c4 = c / 4;
    const int tpr = c4 >= APPLY_TPR_WIDE ? APPLY_TPR_WIDE : (c4 < APPLY_TPR ? c4 : APPLY_TPR);
    const int rpp = 256 / tpr;
    const int cblocks = (c4 + tpr - 1) / tpr;
    long long s = stream_grid((long long)rows * c4, 256) / cblocks;
    const int smax = (rows + rpp - 1) / rpp;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    return {tpr, cblocks, (int)s};
}
inline dim3 col_dim(const ColGrid& g) { return dim3((unsigned)g.slices * (unsigned)g.cblocks); }

// what a thread owns: float4 column cc (channels c0 .. c0 + 3) and rows r, r + rpp, ... < r1
struct ColLane { int cb, slice, cc, c0, r, r1, rpp; bool live; };
__device__ __forceinline__ ColLane col_lane(int rows, int c4, int tpr, int cblocks, int slices) {
    ColLane L;
    L.rpp = 256 / tpr;
    const int ct = threadIdx.x % tpr, rl = threadIdx.x / tpr;
    L.cb = blockIdx.x % cblocks; L.slice = blockIdx.x / cblocks;
    const int per = (rows + slices - 1) / slices;
    const int r0 = L.slice * per;
    L.r1 = min(rows, r0 + per);
    L.r = r0 + rl;
    L.cc = L.cb * tpr + ct; L.c0 = L.cc * 4;
    L.live = L.cc < c4 && rl < L.rpp;
    return L;
}

// the row loop of both forward applies; returns max |y| over the thread's elements (0 for the packed form)
template <bool RES>
__device__ __forceinline__ float bn_apply_rows(const ColLane& L, const float* __restrict__ x, int ldx, const float* __restrict__ res, int ldr,
                                               float* __restrict__ y, int ldy, const float4 mu, const float4 is, const float4 ga, const float4 be,
                                               int c4, int relu, unsigned char* __restrict__ mask, bool packed, float sc) {
    float am = 0.f;
    const int c0 = L.c0, cc = L.cc, rpp = L.rpp;
    auto emit = [&](long long row, const float4 xx, const float4 rr) __attribute__((always_inline)) {
        float4 o = make_float4(bn_val(xx.x, mu.x, is.x, ga.x, be.x), bn_val(xx.y, mu.y, is.y, ga.y, be.y),
                               bn_val(xx.z, mu.z, is.z, ga.z, be.z), bn_val(xx.w, mu.w, is.w, ga.w, be.w));
        if (RES) { o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w; }
        if (mask) mask[row * c4 + cc] = (unsigned char)((o.x > 0.f) | ((o.y > 0.f) << 1) | ((o.z > 0.f) << 2) | ((o.w > 0.f) << 3));
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        if (packed) {
            const SplitH sp = split4h(o, sc);
            const float2 h = __builtin_bit_cast(float2, sp.h), l = __builtin_bit_cast(float2, sp.l);
            o = make_float4(h.x, h.y, l.x, l.y);
        } else {
            am = fmaxf(fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
        }
        *reinterpret_cast<float4*>(y + row * ldy + c0) = o;
    };
    int r = L.r;
    for (; r + 3 * rpp < L.r1; r += 4 * rpp) {
        float4 qx[4], qr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long row = r + u * rpp;
            qx[u] = *reinterpret_cast<const float4*>(x + row * ldx + c0);
            if (RES) qr[u] = *reinterpret_cast<const float4*>(res + row * ldr + c0);
        }
        __builtin_amdgcn_sched_barrier(0);       // every load of the four rows is in flight before the first use
#pragma unroll
        for (int u = 0; u < 4; ++u) emit(r + u * rpp, qx[u], RES ? qr[u] : qx[u]);
    }
    for (; r < L.r1; r += rpp) {
        const long long row = r;
        const float4 qx = *reinterpret_cast<const float4*>(x + row * ldx + c0);
        const float4 qr = RES ? *reinterpret_cast<const float4*>(res + row * ldr + c0) : qx;
        emit(row, qx, qr);
    }
    return am;
}

template <bool RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ res, int ldr,
                                                       float* __restrict__ y, int ldy, Coef k, int rows, int c4, int tpr, int cblocks,
                                                       int slices, int relu, float* __restrict__ amax_out, unsigned char* __restrict__ mask) {
    const ColLane L = col_lane(rows, c4, tpr, cblocks, slices);
    float am = 0.f;
    if (L.live) {
        const float4 mu = *reinterpret_cast<const float4*>(k.mean + L.c0);
        const float4 is = *reinterpret_cast<const float4*>(k.invstd + L.c0);
        const float4 ga = *reinterpret_cast<const float4*>(k.gamma + L.c0);
        const float4 be = *reinterpret_cast<const float4*>(k.beta + L.c0);
        am = bn_apply_rows<RES>(L, x, ldx, res, ldr, y, ldy, mu, is, ga, be, c4, relu, mask, false, 1.f);
    }
    if (amax_out) block_amax(am, amax_out);
}

// BatchNorm apply with the statistics FINISHED IN THE KERNEL: the producing contraction's epilogue left (sum x, sum x^2) per
// channel in `sums` (glf_gemm_params.colstats); every workgroup turns them into mean / invstd for the channels of ITS column
// block in LDS (bn_finish, as bn_stats_finalize does: results are bit-identical to glf_bn_stats_from_sums +
// glf_bn_apply), the workgroup of row slice 0 also writes them out for the backward pass and updates the running statistics of
// its block.  One launch instead of two per BatchNorm, and no tiny kernel on the dependent chain conv -> statistics -> apply ->
// next conv.
constexpr int APPLY_MAX_C = 4096;
template <bool RES>
__global__ __launch_bounds__(256) void bn_apply_sums_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ res, int ldr,
                                                            float* __restrict__ y, int ldy, const double* __restrict__ sums, int rows, int c,
                                                            float eps, float momentum, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ mean_out, float* __restrict__ invstd_out, float* rmean, float* rvar,
                                                            long long* nbt, int tpr, int cblocks, int slices, int relu, float* __restrict__ amax_out,
                                                            unsigned char* __restrict__ mask, const float* __restrict__ colmax) {
    // colmax != null: y is written as the packed pre-split fp16 image (glf_split_f16_packed's format), scaled with an upper
    // bound of max |y| that every workgroup derives from the per-channel maxima of |x| BEFORE writing anything -- the one place
    // where a workgroup still visits ALL channels:
    //   |y_c| <= |gamma_c| invstd_c (max|x_c| + |mean_c|) + |beta_c|        (workgroup 0 stores the bound to *amax_out)
    __shared__ __attribute__((aligned(16))) float s_mean[APPLY_MAXCOL];
    __shared__ __attribute__((aligned(16))) float s_is[APPLY_MAXCOL];
    __shared__ float s_bound[4];
    const int c4 = c >> 2;
    const ColLane L = col_lane(rows, c4, tpr, cblocks, slices);
    const int base = L.cb * tpr * 4, top = min(c, base + tpr * 4);
    float bound = 0.f;
    for (int ch = (colmax ? 0 : base) + threadIdx.x; ch < (colmax ? c : top); ch += blockDim.x) {
        const BnStat st = bn_finish(sums[ch], sums[c + ch], rows, eps);
        if (colmax) bound = fmaxf(bound, fabsf(gamma[ch]) * st.invstd * (colmax[ch] + fabsf(st.mean)) + fabsf(beta[ch]));
        if (ch >= base && ch < top) {
            s_mean[ch - base] = st.mean; s_is[ch - base] = st.invstd;
            if (L.slice == 0) {
                mean_out[ch] = st.mean; invstd_out[ch] = st.invstd;
                if (rmean) bn_running_update(st, rows, momentum, rmean[ch], rvar[ch]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
    float sc = 1.f, sc_inv = 1.f;
    if (colmax) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bound = fmaxf(bound, __shfl_xor(bound, o, 64));
        if ((threadIdx.x & 63) == 0) s_bound[threadIdx.x >> 6] = bound;
    }
    __syncthreads();
    if (colmax) {
        bound = 1.0001f * fmaxf(fmaxf(s_bound[0], s_bound[1]), fmaxf(s_bound[2], s_bound[3]));
        if (blockIdx.x == 0 && threadIdx.x == 0) *amax_out = bound;
        pow2_scale(&bound, sc, sc_inv);
    }
    float am = 0.f;
    if (L.live) {
        const float4 mu = *reinterpret_cast<const float4*>(s_mean + (L.c0 - base));
        const float4 is = *reinterpret_cast<const float4*>(s_is + (L.c0 - base));
        const float4 ga = *reinterpret_cast<const float4*>(gamma + L.c0);
        const float4 be = *reinterpret_cast<const float4*>(beta + L.c0);
        am = bn_apply_rows<RES>(L, x, ldx, res, ldr, y, ldy, mu, is, ga, be, c4, relu, mask, colmax != nullptr, sc);
    }
    if (amax_out && !colmax) block_amax(am, amax_out);
}

// dx = gamma*invstd*(dy' - [sum_dy/n + xhat*sum_dyx/n]) ; dres = dy'
struct BwdApply {
    const float* dy; int lddy; const float* x; int ldx; const float* y; int ldy; Coef k;
    const float* sum_dy; const float* sum_dyx;
    float* dx; int lddx; float* dres; int lddres;
    int rows, c, tpr, cblocks, slices, training; float inv_n;
    float* amax_out; int packed; const unsigned char* mask; const float* dy2; int lddy2;
    const double* fsums; const float* fmax; float* out_dbeta; float* out_dgamma;
};
// HAS2 / RM as in bnbwd_reduce_atomic_kernel; NEEDX: x is read (training, or the ReLU sign recomputed from it).
template <bool HAS2, int RM, bool NEEDX>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BwdApply p) {
    // packed != 0: dx is written as the packed pre-split fp16 image (glf_split_f16_packed's format) scaled by *amax_out, which
    // then holds an upper bound of max |dx| computed by bnbwd_finalize (not a by-product of this kernel)
    // fsums != null (fused form): the reduction left UNFINISHED sums (doubles [2][c]) and, for the packed form, per-channel maxima
    // (fmax [2][c]); every thread finishes the sums of its own four channels in registers, the workgroups of row slice 0 write
    // dbeta / dgamma of their column block, and the packed form's bound (bnbwd_finalize's expression, over ALL channels) is derived
    // by every workgroup before it writes anything
    __shared__ float s_bound[4];
    const int c = p.c, c4 = p.c >> 2;
    const ColLane L = col_lane(p.rows, c4, p.tpr, p.cblocks, p.slices);
    const int c0 = L.c0, cc = L.cc, rpp = L.rpp;
    const int training = p.training, packed = p.packed;
    const float inv_n = p.inv_n;
    float am = 0.f, sc = 1.f, sc_inv = 1.f;
    if (packed && p.fsums) {
        float bound_local = 0.f;
        for (int ch = threadIdx.x; ch < c; ch += blockDim.x) {
            const float a = (float)p.fsums[ch], b = (float)p.fsums[c + ch];
            const float kk = fabsf(p.k.gamma[ch] * p.k.invstd[ch]);
            const float bb = 1.0001f * kk * (training ? p.fmax[ch] + inv_n * (fabsf(a) + p.fmax[c + ch] * fabsf(b)) : p.fmax[ch]);
            if (bb < 3.0e38f) bound_local = fmaxf(bound_local, bb);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bound_local = fmaxf(bound_local, __shfl_xor(bound_local, o, 64));
        if ((threadIdx.x & 63) == 0) s_bound[threadIdx.x >> 6] = bound_local;
        __syncthreads();
        float bnd = fmaxf(fmaxf(s_bound[0], s_bound[1]), fmaxf(s_bound[2], s_bound[3]));
        if (blockIdx.x == 0 && threadIdx.x == 0) *p.amax_out = bnd;
        pow2_scale(&bnd, sc, sc_inv);
    } else if (packed) pow2_scale(p.amax_out, sc, sc_inv);
    if (L.live) {
        const float4 is = *reinterpret_cast<const float4*>(p.k.invstd + c0);
        const float4 ga = *reinterpret_cast<const float4*>(p.k.gamma + c0);
        float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), be = mu, s1 = mu, s2 = mu;
        if (NEEDX) mu = *reinterpret_cast<const float4*>(p.k.mean + c0);
        if (RM == 2) be = *reinterpret_cast<const float4*>(p.k.beta + c0);
        if (p.fsums) {
            s1 = make_float4((float)p.fsums[c0], (float)p.fsums[c0 + 1], (float)p.fsums[c0 + 2], (float)p.fsums[c0 + 3]);
            s2 = make_float4((float)p.fsums[c + c0], (float)p.fsums[c + c0 + 1], (float)p.fsums[c + c0 + 2], (float)p.fsums[c + c0 + 3]);
            if (L.slice == 0 && L.r == 0) {
                if (p.out_dbeta) { p.out_dbeta[c0] = s1.x; p.out_dbeta[c0 + 1] = s1.y; p.out_dbeta[c0 + 2] = s1.z; p.out_dbeta[c0 + 3] = s1.w; }
                if (p.out_dgamma) { p.out_dgamma[c0] = s2.x; p.out_dgamma[c0 + 1] = s2.y; p.out_dgamma[c0 + 2] = s2.z; p.out_dgamma[c0 + 3] = s2.w; }
            }
        } else if (training) {
            s1 = *reinterpret_cast<const float4*>(p.sum_dy + c0);
            s2 = *reinterpret_cast<const float4*>(p.sum_dyx + c0);
        }
        const float* __restrict__ dy = p.dy; const float* __restrict__ dy2 = p.dy2; const float* __restrict__ x = p.x;
        const float* __restrict__ y = p.y; const unsigned char* __restrict__ mask = p.mask;
        float* __restrict__ dx = p.dx; float* __restrict__ dres = p.dres;
        const int lddy = p.lddy, lddy2 = p.lddy2, ldx = p.ldx, ldy = p.ldy, lddx = p.lddx, lddres = p.lddres;
        auto emit = [&](long long row, float4 g, const float4 g2, const float4 xx, const float4 yy, unsigned m) __attribute__((always_inline)) {
            if (HAS2) { g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w; }
            if (RM == 1) {
                g.x = (m & 1u) ? g.x : 0.f; g.y = (m & 2u) ? g.y : 0.f; g.z = (m & 4u) ? g.z : 0.f; g.w = (m & 8u) ? g.w : 0.f;
            } else if (RM != 0) {
                const float4 v = RM == 3 ? yy : make_float4(bn_val(xx.x, mu.x, is.x, ga.x, be.x), bn_val(xx.y, mu.y, is.y, ga.y, be.y),
                                                            bn_val(xx.z, mu.z, is.z, ga.z, be.z), bn_val(xx.w, mu.w, is.w, ga.w, be.w));
                g.x = v.x > 0.f ? g.x : 0.f; g.y = v.y > 0.f ? g.y : 0.f;
                g.z = v.z > 0.f ? g.z : 0.f; g.w = v.w > 0.f ? g.w : 0.f;
            }
            if (dres) *reinterpret_cast<float4*>(dres + row * lddres + c0) = g;
            float4 o;
            if (training) {
                o.x = ga.x * is.x * (g.x - inv_n * (s1.x + (xx.x - mu.x) * is.x * s2.x));
                o.y = ga.y * is.y * (g.y - inv_n * (s1.y + (xx.y - mu.y) * is.y * s2.y));
                o.z = ga.z * is.z * (g.z - inv_n * (s1.z + (xx.z - mu.z) * is.z * s2.z));
                o.w = ga.w * is.w * (g.w - inv_n * (s1.w + (xx.w - mu.w) * is.w * s2.w));
            } else {
                o = make_float4(g.x * ga.x * is.x, g.y * ga.y * is.y, g.z * ga.z * is.z, g.w * ga.w * is.w);
            }
            if (packed) {
                const SplitH sp = split4h(o, sc);
                const float2 h = __builtin_bit_cast(float2, sp.h), l = __builtin_bit_cast(float2, sp.l);
                o = make_float4(h.x, h.y, l.x, l.y);
            } else {
                am = fmaxf(fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
            }
            *reinterpret_cast<float4*>(dx + row * lddx + c0) = o;
        };
        int r = L.r;
        for (; r + 3 * rpp < L.r1; r += 4 * rpp) {
            float4 qg[4], qg2[4], qx[4], qy[4];
            unsigned m[4] = {15u, 15u, 15u, 15u};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long row = r + u * rpp;
                qg[u] = *reinterpret_cast<const float4*>(dy + row * lddy + c0);
                if (HAS2) qg2[u] = *reinterpret_cast<const float4*>(dy2 + row * lddy2 + c0);
                if (NEEDX) qx[u] = *reinterpret_cast<const float4*>(x + row * ldx + c0);
                if (RM == 3) qy[u] = *reinterpret_cast<const float4*>(y + row * ldy + c0);
                if (RM == 1) m[u] = mask[row * c4 + cc];
            }
            __builtin_amdgcn_sched_barrier(0);       // every load of the four rows is in flight before the first use
#pragma unroll
            for (int u = 0; u < 4; ++u) emit(r + u * rpp, qg[u], HAS2 ? qg2[u] : qg[u], NEEDX ? qx[u] : mu, RM == 3 ? qy[u] : mu, m[u]);
        }
        for (; r < L.r1; r += rpp) {
            const long long row = r;
            const float4 qg = *reinterpret_cast<const float4*>(dy + row * lddy + c0);
            const float4 qg2 = HAS2 ? *reinterpret_cast<const float4*>(dy2 + row * lddy2 + c0) : qg;
            const float4 qx = NEEDX ? *reinterpret_cast<const float4*>(x + row * ldx + c0) : mu;
            const float4 qy = RM == 3 ? *reinterpret_cast<const float4*>(y + row * ldy + c0) : mu;
            const unsigned m = RM == 1 ? mask[row * c4 + cc] : 15u;
            emit(row, qg, qg2, qx, qy, m);
        }
    }
    if (p.amax_out && !packed) block_amax(am, p.amax_out);
}

int launch_bwd_apply(const BwdApply& p, int relu, hipStream_t s) {
    const int rm = !relu ? 0 : (p.mask ? 1 : (p.y ? 3 : 2));
    const bool needx = p.training || rm == 2;
    const dim3 grid((unsigned)p.slices * (unsigned)p.cblocks);
#define GLF_BNA(H2, RM_, NX) hipLaunchKernelGGL((bn_bwd_apply_kernel<H2, RM_, NX>), grid, dim3(256), 0, s, p)
#define GLF_BNA_RM(H2, NX) do { if (rm == 0) GLF_BNA(H2, 0, NX); else if (rm == 1) GLF_BNA(H2, 1, NX); else GLF_BNA(H2, 3, NX); } while (0)
    if (rm == 2) { if (p.dy2) GLF_BNA(true, 2, true); else GLF_BNA(false, 2, true); }
    else if (p.dy2) { if (needx) GLF_BNA_RM(true, true); else GLF_BNA_RM(true, false); }
    else { if (needx) GLF_BNA_RM(false, true); else GLF_BNA_RM(false, false); }
#undef GLF_BNA_RM
#undef GLF_BNA
    return glf::check_launch("bn_bwd_apply");
}

// ---- the applies of bf16 storage: the remaining PAIR.  Flat grid-stride passes over 16-byte accesses (eight channels per lane)
// with the coefficients of ALL channels in LDS, fp32 arithmetic, one rounding to bf16 at the store -- not the column-owning
// bodies above.  (Moving them there changes their speed, their column-block tuning and, rarely, the last bf16 bit of the training
// dx, which they evaluate with 1 / n folded into the sums: a change with its own measurements.)
__global__ __launch_bounds__(256) void s16_bn_apply_kernel(const u16* __restrict__ x, int ldx, const u16* __restrict__ res, int ldr,
                                                           u16* __restrict__ y, int ldy, const double* __restrict__ sums, int rows, int c,
                                                           float eps, float momentum, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ mean_io, float* __restrict__ invstd_io, float* rmean, float* rvar,
                                                           long long* nbt, long long total8, int c8, int relu, unsigned char* __restrict__ mask) {
    // sums != null (train): every workgroup turns (sum x, sum x^2) into mean / invstd for all channels in LDS; workgroup 0 writes
    // them to mean_io / invstd_io for the backward pass and updates the running statistics.  sums == null (eval): mean_io /
    // invstd_io are inputs (glf_bn_eval_coeffs).
    extern __shared__ __attribute__((aligned(16))) float s_coef[];       // [2][c]: mean, invstd
    float* s_mu = s_coef;
    float* s_is = s_coef + c;
    for (int ch = threadIdx.x; ch < c; ch += blockDim.x) {
        float mf, isf;
        if (sums) {
            const BnStat st = bn_finish(sums[ch], sums[c + ch], rows, eps);
            mf = st.mean; isf = st.invstd;
            if (blockIdx.x == 0) {
                mean_io[ch] = mf; invstd_io[ch] = isf;
                if (rmean) bn_running_update(st, rows, momentum, rmean[ch], rvar[ch]);
            }
        } else {
            mf = mean_io[ch]; isf = invstd_io[ch];
        }
        s_mu[ch] = mf; s_is[ch] = isf;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt && sums) *nbt += 1;
    __syncthreads();
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / c8;
        const int cc = (int)(i - r * c8) * 8;
        const F8 xx = ld8(x + r * ldx + cc);
        const F8 mu = ldf8(s_mu + cc), is = ldf8(s_is + cc), ga = ldf8(gamma + cc), be = ldf8(beta + cc);
        F8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = bn_val(xx.v[j], mu.v[j], is.v[j], ga.v[j], be.v[j]);
        if (res) {
            const F8 rr = ld8(res + r * ldr + cc);
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] += rr.v[j];
        }
        if (mask) {
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) m |= (o.v[j] > 0.f ? 1u : 0u) << j;
            mask[i] = (unsigned char)m;
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = fmaxf(o.v[j], 0.f);
        }
        st8(y + r * ldy + cc, o);
    }
}

// dx = gamma*invstd*(dy' - [sum_dy/n + xhat*sum_dyx/n]) ; dres = dy'.  The sums arrive unfinished (doubles [2][c] from the
// reduction kernel's atomics); workgroup 0 also writes dgamma = sum dy' xhat and dbeta = sum dy'.
__global__ __launch_bounds__(256) void s16_bnbwd_apply_kernel(const u16* __restrict__ dy, int lddy, const u16* __restrict__ dy2, int lddy2,
                                                              const u16* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const double* __restrict__ sums, u16* __restrict__ dx, int lddx, u16* __restrict__ dres,
                                                              int lddres, float* __restrict__ dgamma, float* __restrict__ dbeta, long long total8, int c8, int c,
                                                              int relu, int training, float inv_n, const unsigned char* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) float s_k[];        // [2][c]: s1 / n, s2 / n
    float* s_s1 = s_k;
    float* s_s2 = s_k + c;
    for (int ch = threadIdx.x; ch < c; ch += blockDim.x) {
        const float a = (float)sums[ch], b = (float)sums[c + ch];
        s_s1[ch] = a * inv_n; s_s2[ch] = b * inv_n;
        if (blockIdx.x == 0) { if (dbeta) dbeta[ch] = a; if (dgamma) dgamma[ch] = b; }
    }
    __syncthreads();
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / c8;
        const int cc = (int)(i - r * c8) * 8;
        F8 g = ld8(dy + r * lddy + cc);
        if (dy2) {
            const F8 g2 = ld8(dy2 + r * lddy2 + cc);
#pragma unroll
            for (int j = 0; j < 8; ++j) g.v[j] += g2.v[j];
        }
        const F8 is = ldf8(invstd + cc), ga = ldf8(gamma + cc);
        F8 xx, mu;
        const bool need_x = training || (relu && !mask);
        if (need_x) { xx = ld8(x + r * ldx + cc); mu = ldf8(mean + cc); }
        unsigned m = 0xffu;
        if (relu && mask) {
            m = mask[i];
        } else if (relu) {
            const F8 be = ldf8(beta + cc);
            m = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) m |= (bn_val(xx.v[j], mu.v[j], is.v[j], ga.v[j], be.v[j]) > 0.f ? 1u : 0u) << j;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) g.v[j] = ((m >> j) & 1u) ? g.v[j] : 0.f;
        if (dres) st8(dres + r * lddres + cc, g);
        F8 o;
        if (training) {
            const F8 s1 = ldf8(s_s1 + cc), s2 = ldf8(s_s2 + cc);
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = ga.v[j] * is.v[j] * (g.v[j] - (s1.v[j] + (xx.v[j] - mu.v[j]) * is.v[j] * s2.v[j]));
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = g.v[j] * ga.v[j] * is.v[j];
        }
        st8(dx + r * lddx + cc, o);
    }
}

__global__ void f64_to_f32_kernel(const double* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

// ---- TPAVI tail: one wavefront per row ---------------------------------------------------
constexpr int LN_NV = 8;      // float4 per lane => C <= 64*4*8 = 2048

template <bool BWD>
__global__ __launch_bounds__(256) void bn_res_ln_kernel(const float* __restrict__ w, const float* __restrict__ x, Coef bn,
                                                        const float* __restrict__ ln_g, const float* __restrict__ ln_b, float eps,
                                                        float* __restrict__ z, float* __restrict__ row_mean, float* __restrict__ row_rstd,
                                                        const float* __restrict__ dz, float* __restrict__ du, int rows, int c,
                                                        float* __restrict__ amax_out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c4 = c >> 2;
    const long long base = (long long)row * c;
    float4 u[LN_NV];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < LN_NV; ++v) {
        const int cc = lane + 64 * v;
        if (cc < c4) {
            const int ch = cc * 4;
            const float4 ww = *reinterpret_cast<const float4*>(w + base + ch);
            const float4 xx = *reinterpret_cast<const float4*>(x + base + ch);
            const float4 mu = *reinterpret_cast<const float4*>(bn.mean + ch);
            const float4 is = *reinterpret_cast<const float4*>(bn.invstd + ch);
            const float4 ga = *reinterpret_cast<const float4*>(bn.gamma + ch);
            const float4 be = *reinterpret_cast<const float4*>(bn.beta + ch);
            u[v] = make_float4((ww.x - mu.x) * is.x * ga.x + be.x + xx.x, (ww.y - mu.y) * is.y * ga.y + be.y + xx.y,
                               (ww.z - mu.z) * is.z * ga.z + be.z + xx.z, (ww.w - mu.w) * is.w * ga.w + be.w + xx.w);
            s += (u[v].x + u[v].y) + (u[v].z + u[v].w);
        } else {
            u[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    float mean, rstd;
    if (!BWD) {
        mean = wave_sum(s) / c;
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < LN_NV; ++v)
            if (lane + 64 * v < c4) {
                const float a = u[v].x - mean, b = u[v].y - mean, cc2 = u[v].z - mean, d = u[v].w - mean;
                q += (a * a + b * b) + (cc2 * cc2 + d * d);
            }
        rstd = 1.0f / sqrtf(wave_sum(q) / c + eps);
        if (lane == 0) { row_mean[row] = mean; row_rstd[row] = rstd; }
        float am = 0.f;
#pragma unroll
        for (int v = 0; v < LN_NV; ++v) {
            const int cc = lane + 64 * v;
            if (cc < c4) {
                const int ch = cc * 4;
                const float4 g = *reinterpret_cast<const float4*>(ln_g + ch);
                const float4 b = *reinterpret_cast<const float4*>(ln_b + ch);
                const float4 o = make_float4((u[v].x - mean) * rstd * g.x + b.x, (u[v].y - mean) * rstd * g.y + b.y,
                                             (u[v].z - mean) * rstd * g.z + b.z, (u[v].w - mean) * rstd * g.w + b.w);
                *reinterpret_cast<float4*>(z + base + ch) = o;
                am = fmaxf(fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
            }
        }
        if (amax_out) {          // max |z| as a by-product (one wave per row: only a row that raises the maximum issues the atomic)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
            if (lane == 0 && am > *reinterpret_cast<volatile float*>(amax_out)) atomicMax(reinterpret_cast<unsigned*>(amax_out), __float_as_uint(am));
        }
    } else {
        mean = row_mean[row]; rstd = row_rstd[row];
        float4 gz[LN_NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < LN_NV; ++v) {
            const int cc = lane + 64 * v;
            if (cc < c4) {
                const int ch = cc * 4;
                const float4 d = *reinterpret_cast<const float4*>(dz + base + ch);
                const float4 g = *reinterpret_cast<const float4*>(ln_g + ch);
                gz[v] = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
                u[v] = make_float4((u[v].x - mean) * rstd, (u[v].y - mean) * rstd, (u[v].z - mean) * rstd, (u[v].w - mean) * rstd);
                s1 += (gz[v].x + gz[v].y) + (gz[v].z + gz[v].w);
                s2 += (gz[v].x * u[v].x + gz[v].y * u[v].y) + (gz[v].z * u[v].z + gz[v].w * u[v].w);
            } else {
                gz[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        const float m1 = wave_sum(s1) / c, m2 = wave_sum(s2) / c;
#pragma unroll
        for (int v = 0; v < LN_NV; ++v) {
            const int cc = lane + 64 * v;
            if (cc < c4)
                *reinterpret_cast<float4*>(du + base + cc * 4) =
                    make_float4(rstd * (gz[v].x - m1 - u[v].x * m2), rstd * (gz[v].y - m1 - u[v].y * m2),
                                rstd * (gz[v].z - m1 - u[v].z * m2), rstd * (gz[v].w - m1 - u[v].w * m2));
        }
    }
}

// ---- TPAVI tail backward in ONE walk: du and the six column reductions that follow from it ------------------------------------
// bn_res_ln_kernel<true> (du), colreduce_kernel<OpLnParam> (the LayerNorm parameter gradients) and the BatchNorm-backward
// reduction over du each walked dz / w / x or du; here the tensors are read once.  A wavefront that owns a whole row has no
// registers left for column accumulators over its 32 channels per lane, so a WORKGROUP owns the rows of its slice, TA_R at a
// time, and each of its four waves a quarter of the channels for all of them: the float4 columns lane + 64 v, v = 2 q and
// 2 q + 1 -- the columns the row-owning lane `lane` visits at steps 2 q and 2 q + 1 of its loop.  Per lane: 8 channels with
// their coefficients in registers for the whole kernel and 4 x 8 fp32 accumulators (the sums and maxima over du, max |what|).
//   du is bit-identical to bn_res_ln_kernel<true>'s: the per-row sums s1 / s2 are rebuilt in that kernel's order.  Every wave
//   leaves its per-lane terms of a row in LDS (wave 0 the sum of its two, which is how the row-owning lane's chain starts); after
//   the barrier every wave adds the seven values per lane in the order v = 0 .. 7 and folds the lanes with the same butterfly.
//   (A column beyond C contributes +0.f, which leaves a chain that starts at +0.f unchanged bit for bit.)
//   The roundings are spelled out, because -ffp-contract=fast lets the compiler choose them per context and the two kernels are
//   different contexts: bn_res_ln_kernel<true> as compiled rounds d ln_g and the products gz uhat before adding them (its s1 / s2
//   pair is evaluated with packed adds), except at column step v = 1, where s2 gets fma(gz.x, uhat.x, gz.y uhat.y) +
//   fma(gz.z, uhat.z, gz.w uhat.w); u is fma((w - mean) invstd, gamma, beta) + x and du is rstd fma(-m2, uhat, gz - m1).
//   rounded() keeps a product out of a contraction.  tests/test_gpu_tail_bwd_fused.py compares du bit for bit at every width.
//   Accumulation: doubles in thread-private LDS cells (no atomics, no barrier; 32 doubles per thread do not fit beside the row
//   data in registers at two waves per SIMD).  The LayerNorm sums are added there element by element, like the pass they
//   replace; the sums over du in fp32 over at most TA_FLUSH rows first, like the BatchNorm reduction they replace.  One set of partials per
//   workgroup in the two-stage layout, partial[stat][slice][c]: stat 0 = sum dz uhat, 1 = sum dz, 2 = sum du, 3 = sum du what;
//   pmax[0][slice][c] = max |du|, pmax[1][slice][c] = max |what| (what = (w - mean) invstd).  Fixed order everywhere.
// LDS: 14 KB of row terms + 64 KB of doubles = 78 KB, two workgroups per CU; the grid is at most that many workgroups.
__device__ __forceinline__ float rounded(float p) { asm volatile("" : "+v"(p)); return p; }
constexpr int TA_R = 3;            // rows of a slice in flight (every load of the TA_R rows is issued before the first use)
constexpr int TA_FLUSH = 15;       // rows of du summed in fp32 before the fold into doubles
constexpr int TA_MAX_SLICES = 512;

inline int tail_slices(int rows) {
    int s = (rows + 4 * TA_R - 1) / (4 * TA_R);
    int cap = 2 * num_cus();
    if (cap > TA_MAX_SLICES) cap = TA_MAX_SLICES;
    return s < 1 ? 1 : (s > cap ? cap : s);
}

__global__ __launch_bounds__(256, 2) void bn_res_ln_bwd_sums_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                                    const float* __restrict__ x, Coef bn, const float* __restrict__ ln_g,
                                                                    const float* __restrict__ row_mean, const float* __restrict__ row_rstd,
                                                                    float* __restrict__ du, int rows, int c, int slices,
                                                                    double* __restrict__ partial, float* __restrict__ pmax) {
    __shared__ float sT[TA_R][2][7][64];          // [row][s1 | s2][chain slot][lane]
    __shared__ double sD[32][256];                // [stat * 8 + column j * 4 + component][thread]
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int c4 = c >> 2;
    const int slice = blockIdx.x;
    const int per = (rows + slices - 1) / slices;
    const int r0 = slice * per, r1 = min(rows, r0 + per);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int ch[2]; bool lv[2];
    float4 mu[2], is[2], ga[2], be[2], lg[2];
    float4 sa[2], sb[2], mg[2], mx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cc = lane + 64 * (2 * q + j);
        lv[j] = cc < c4; ch[j] = cc * 4;
        mu[j] = is[j] = ga[j] = be[j] = lg[j] = zero4;
        if (lv[j]) {
            mu[j] = *reinterpret_cast<const float4*>(bn.mean + ch[j]);
            is[j] = *reinterpret_cast<const float4*>(bn.invstd + ch[j]);
            ga[j] = *reinterpret_cast<const float4*>(bn.gamma + ch[j]);
            be[j] = *reinterpret_cast<const float4*>(bn.beta + ch[j]);
            lg[j] = *reinterpret_cast<const float4*>(ln_g + ch[j]);
        }
        sa[j] = sb[j] = mg[j] = mx[j] = zero4;
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) sD[k][tid] = 0.0;
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float4 v[2] = {sa[j], sb[j]};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                sD[16 + st * 8 + j * 4 + 0][tid] += (double)v[st].x; sD[16 + st * 8 + j * 4 + 1][tid] += (double)v[st].y;
                sD[16 + st * 8 + j * 4 + 2][tid] += (double)v[st].z; sD[16 + st * 8 + j * 4 + 3][tid] += (double)v[st].w;
            }
            sa[j] = sb[j] = zero4;
        }
    };
    int pending = 0;
    for (int rb = r0; rb < r1; rb += TA_R) {
        // gz = dz ln_g, uh = uhat and wh = what of the TA_R rows replace the loaded dz, x and w in place
        float4 gz[TA_R][2], uh[TA_R][2], wh[TA_R][2];
        float rm[TA_R], rs[TA_R];
#pragma unroll
        for (int u = 0; u < TA_R; ++u) {
            const int row = rb + u;
            const bool ok = row < r1;
            const long long base = (long long)row * c;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                gz[u][j] = uh[u][j] = wh[u][j] = zero4;
                if (ok && lv[j]) {
                    gz[u][j] = *reinterpret_cast<const float4*>(dz + base + ch[j]);
                    wh[u][j] = *reinterpret_cast<const float4*>(w + base + ch[j]);
                    uh[u][j] = *reinterpret_cast<const float4*>(x + base + ch[j]);
                }
            }
            rm[u] = ok ? row_mean[row] : 0.f;
            rs[u] = ok ? row_rstd[row] : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);       // every load of the TA_R rows is in flight before the first use
#pragma unroll
        for (int u = 0; u < TA_R; ++u) {
            const bool ok = rb + u < r1;
            const float mean = rm[u], rstd = rs[u];
            float t1[2], t2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 d = gz[u][j], ww = wh[u][j], xx = uh[u][j];
                const float4 wn = make_float4((ww.x - mu[j].x) * is[j].x, (ww.y - mu[j].y) * is[j].y, (ww.z - mu[j].z) * is[j].z, (ww.w - mu[j].w) * is[j].w);
                float4 uu = make_float4(__builtin_fmaf(wn.x, ga[j].x, be[j].x) + xx.x, __builtin_fmaf(wn.y, ga[j].y, be[j].y) + xx.y,
                                        __builtin_fmaf(wn.z, ga[j].z, be[j].z) + xx.z, __builtin_fmaf(wn.w, ga[j].w, be[j].w) + xx.w);
                uu = make_float4((uu.x - mean) * rstd, (uu.y - mean) * rstd, (uu.z - mean) * rstd, (uu.w - mean) * rstd);
                const float4 g = make_float4(rounded(d.x * lg[j].x), rounded(d.y * lg[j].y), rounded(d.z * lg[j].z), rounded(d.w * lg[j].w));
                const float4 pr = make_float4(rounded(g.x * uu.x), rounded(g.y * uu.y), rounded(g.z * uu.z), rounded(g.w * uu.w));
                t1[j] = (g.x + g.y) + (g.z + g.w);
                // column step v = 1 of the row-owning kernel (wave 0, j = 1) is the one whose s2 term was compiled with fused products
                t2[j] = (j == 1 && q == 0) ? __builtin_fmaf(g.x, uu.x, pr.y) + __builtin_fmaf(g.z, uu.z, pr.w) : (pr.x + pr.y) + (pr.z + pr.w);
                // the LayerNorm parameter sums go to their doubles element by element, as colreduce_kernel<OpLnParam> adds them
                // (a row or column that does not exist holds d = 0)
                sD[j * 4 + 0][tid] += (double)(d.x * uu.x); sD[j * 4 + 1][tid] += (double)(d.y * uu.y);
                sD[j * 4 + 2][tid] += (double)(d.z * uu.z); sD[j * 4 + 3][tid] += (double)(d.w * uu.w);
                sD[8 + j * 4 + 0][tid] += (double)d.x; sD[8 + j * 4 + 1][tid] += (double)d.y;
                sD[8 + j * 4 + 2][tid] += (double)d.z; sD[8 + j * 4 + 3][tid] += (double)d.w;
                if (ok && lv[j]) {
                    mx[j].x = fmaxf(mx[j].x, fabsf(wn.x)); mx[j].y = fmaxf(mx[j].y, fabsf(wn.y));
                    mx[j].z = fmaxf(mx[j].z, fabsf(wn.z)); mx[j].w = fmaxf(mx[j].w, fabsf(wn.w));
                }
                gz[u][j] = g; uh[u][j] = uu; wh[u][j] = wn;
            }
            if (q == 0) {
                float p1 = 0.f, p2 = 0.f;
                if (lv[0]) { p1 += t1[0]; p2 += t2[0]; }
                if (lv[1]) { p1 += t1[1]; p2 += t2[1]; }
                sT[u][0][0][lane] = p1; sT[u][1][0][lane] = p2;
            } else {
                sT[u][0][2 * q - 1][lane] = lv[0] ? t1[0] : 0.f; sT[u][1][2 * q - 1][lane] = lv[0] ? t2[0] : 0.f;
                sT[u][0][2 * q][lane] = lv[1] ? t1[1] : 0.f;     sT[u][1][2 * q][lane] = lv[1] ? t2[1] : 0.f;
            }
        }
        __syncthreads();
        float m1[TA_R], m2[TA_R];
#pragma unroll
        for (int u = 0; u < TA_R; ++u) {
            float s1 = sT[u][0][0][lane], s2 = sT[u][1][0][lane];
#pragma unroll
            for (int k = 1; k < 7; ++k) { s1 += sT[u][0][k][lane]; s2 += sT[u][1][k][lane]; }
            m1[u] = wave_sum(s1) / c; m2[u] = wave_sum(s2) / c;
        }
        __syncthreads();                         // the row terms are free for the next TA_R rows
#pragma unroll
        for (int u = 0; u < TA_R; ++u) {
            const int row = rb + u;
            if (row < r1) {
                const float rstd = rs[u];
                const long long base = (long long)row * c;
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (lv[j]) {
                        const float4 g = gz[u][j], uu = uh[u][j], wn = wh[u][j];
                        const float4 o = make_float4(rstd * __builtin_fmaf(-m2[u], uu.x, g.x - m1[u]), rstd * __builtin_fmaf(-m2[u], uu.y, g.y - m1[u]),
                                                     rstd * __builtin_fmaf(-m2[u], uu.z, g.z - m1[u]), rstd * __builtin_fmaf(-m2[u], uu.w, g.w - m1[u]));
                        *reinterpret_cast<float4*>(du + base + ch[j]) = o;
                        sa[j].x += o.x; sa[j].y += o.y; sa[j].z += o.z; sa[j].w += o.w;
                        sb[j].x += o.x * wn.x; sb[j].y += o.y * wn.y; sb[j].z += o.z * wn.z; sb[j].w += o.w * wn.w;
                        mg[j].x = fmaxf(mg[j].x, fabsf(o.x)); mg[j].y = fmaxf(mg[j].y, fabsf(o.y));
                        mg[j].z = fmaxf(mg[j].z, fabsf(o.z)); mg[j].w = fmaxf(mg[j].w, fabsf(o.w));
                    }
            }
        }
        pending += TA_R;
        if (pending + TA_R > TA_FLUSH) { flush(); pending = 0; }
    }
    flush();
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (lv[j]) {
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                double* pd = partial + ((long long)st * slices + slice) * c + ch[j];
                pd[0] = sD[st * 8 + j * 4 + 0][tid]; pd[1] = sD[st * 8 + j * 4 + 1][tid];
                pd[2] = sD[st * 8 + j * 4 + 2][tid]; pd[3] = sD[st * 8 + j * 4 + 3][tid];
            }
            *reinterpret_cast<float4*>(pmax + (long long)slice * c + ch[j]) = mg[j];
            *reinterpret_cast<float4*>(pmax + (long long)(slices + slice) * c + ch[j]) = mx[j];
        }
}

template <class Op>
int launch_colreduce(Op op, int rows, int c, double* ws, hipStream_t s) {
    const int slices = n_slices_c(rows, c);
    const int c4 = c / 4, tpr = c4 < RT ? c4 : RT;
    hipLaunchKernelGGL((colreduce_kernel<Op>), dim3(slices, (c4 + tpr - 1) / tpr), dim3(RT), 0, s, op, rows, c, slices, ws, (float*)nullptr);
    return glf::check_launch("colreduce");
}
template <class Op>
int launch_colreduce16(Op op, int rows, int c, double* sums, hipStream_t s) {
    const RedGeom g = red_geom<8>(rows, c);
    hipLaunchKernelGGL((s16_colreduce_kernel<Op>), red_grid(g), dim3(RT), 0, s, op, rows, c, g.slices, sums);
    return glf::check_launch("s16_colreduce");
}

}  // namespace

extern "C" size_t glf_bn_workspace(int rows, int c) {
    // doubles: 2 x slices x c partial sums, 2 x c finished sums, and (as floats) 2 x slices x c partial maxima of glf_bn_bwd's packed path
    return (size_t)3 * MAX_SLICES * (size_t)(c > 0 ? c : 0) + (size_t)2 * (c > 0 ? c : 0);
}

#define REQ_C4(c) GLF_REQUIRE((c) > 0 && ((c) % 4) == 0, GLF_ERR_BAD_SHAPE, "channel count must be a positive multiple of 4 (got %d)", (c))
#define REQ_LD(ld, name) GLF_REQUIRE(((ld) % 4) == 0, GLF_ERR_BAD_SHAPE, name " must be a multiple of 4")

extern "C" int glf_bn_stats(const float* x, int ldx, int rows, int c, float eps, float momentum,
                            float* mean, float* invstd, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, double* workspace, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && mean && invstd && workspace, GLF_ERR_NULL, "bn_stats: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_stats: rows must be > 0");
    REQ_C4(c); REQ_AL(x, "x"); REQ_LD(ldx, "ldx");
    GLF_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GLF_ERR_NULL, "bn_stats: running_mean/var must both be set or both NULL");
    if (int rc = launch_colreduce(OpStats{x, ldx}, rows, c, workspace, glf::S(s))) return rc;
    hipLaunchKernelGGL(bn_stats_finalize, dim3((c + FIN_CH - 1) / FIN_CH), dim3(256), 0, glf::S(s), workspace, n_slices_c(rows, c), c, rows,
                       eps, momentum, mean, invstd, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked));
    return glf::check_launch("bn_stats_finalize");
}

extern "C" int glf_bn_stats_from_sums(const double* sums, int rows, int c, float eps, float momentum, float* mean, float* invstd,
                                      float* running_mean, float* running_var, int64_t* num_batches_tracked, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(sums && mean && invstd, GLF_ERR_NULL, "bn_stats_from_sums: null argument");
    GLF_REQUIRE(rows > 0 && c > 0, GLF_ERR_BAD_SHAPE, "bn_stats_from_sums: rows and c must be > 0");
    GLF_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GLF_ERR_NULL, "bn_stats_from_sums: running_mean/var must both be set or both NULL");
    hipLaunchKernelGGL(bn_stats_finalize, dim3((c + FIN_CH - 1) / FIN_CH), dim3(256), 0, glf::S(s), sums, 1, c, rows,
                       eps, momentum, mean, invstd, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked));
    return glf::check_launch("bn_stats_from_sums");
}

extern "C" int glf_bn_replay_running(const float* mean, const float* invstd, int rows, int c, float eps, float momentum,
                                     float* running_mean, float* running_var, int64_t* num_batches_tracked, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(mean && invstd && running_mean && running_var, GLF_ERR_NULL, "bn_replay_running: null argument");
    GLF_REQUIRE(rows > 0 && c > 0, GLF_ERR_BAD_SHAPE, "bn_replay_running: rows and c must be > 0");
    hipLaunchKernelGGL(bn_replay_kernel, dim3((c + 255) / 256), dim3(256), 0, glf::S(s), mean, invstd, rows, eps, momentum,
                       running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), c);
    return glf::check_launch("bn_replay_running");
}

extern "C" int glf_bn_eval_coeffs(const float* rm, const float* rv, float eps, float* mean, float* invstd, int c, glf_stream_t s) {
    GLF_REQUIRE(rm && rv && mean && invstd, GLF_ERR_NULL, "bn_eval_coeffs: null argument");
    GLF_REQUIRE(c > 0, GLF_ERR_BAD_SHAPE, "bn_eval_coeffs: c must be > 0");
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((c + 255) / 256), dim3(256), 0, glf::S(s), rm, rv, eps, mean, invstd, c);
    return glf::check_launch("bn_eval_coeffs");
}

extern "C" int glf_bn_apply(const float* x, int ldx, const float* residual, int ldr, float* y, int ldy,
                            const float* mean, const float* invstd, const float* gamma, const float* beta,
                            int rows, int c, int relu, float* amax_out, uint8_t* relu_mask, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && mean && invstd && gamma && beta, GLF_ERR_NULL, "bn_apply: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_apply: rows must be > 0");
    REQ_C4(c); REQ_AL(x, "x"); REQ_AL(y, "y"); REQ_LD(ldx, "ldx"); REQ_LD(ldy, "ldy");
    if (residual) { REQ_AL(residual, "residual"); REQ_LD(ldr, "ldr"); }
    const ColGrid g = col_grid(rows, c);
#define GLF_BNF(RES_) hipLaunchKernelGGL((bn_apply_kernel<RES_>), col_dim(g), dim3(256), 0, glf::S(s), x, ldx, residual, ldr, y, ldy, \
                                         Coef{mean, invstd, gamma, beta}, rows, c / 4, g.tpr, g.cblocks, g.slices, relu, amax_out, relu_mask)
    if (residual) GLF_BNF(true); else GLF_BNF(false);
#undef GLF_BNF
    return glf::check_launch("bn_apply");
}

extern "C" int glf_bn_apply_from_sums(const float* x, int ldx, const float* residual, int ldr, float* y, int ldy, const double* sums,
                                      int rows, int c, float eps, float momentum, const float* gamma, const float* beta,
                                      float* mean, float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                      int relu, float* amax_out, uint8_t* relu_mask, const float* colmax, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && sums && mean && invstd && gamma && beta, GLF_ERR_NULL, "bn_apply_from_sums: null argument");
    GLF_REQUIRE(!colmax || (amax_out && !residual && y != x), GLF_ERR_BAD_SHAPE, "bn_apply_from_sums: the packed output (colmax) needs amax_out, no residual and y != x");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_apply_from_sums: rows must be > 0");
    REQ_C4(c); REQ_AL(x, "x"); REQ_AL(y, "y"); REQ_LD(ldx, "ldx"); REQ_LD(ldy, "ldy");
    GLF_REQUIRE(c <= APPLY_MAX_C, GLF_ERR_UNSUPPORTED, "bn_apply_from_sums: C must be <= %d (use glf_bn_stats_from_sums + glf_bn_apply)", APPLY_MAX_C);
    GLF_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GLF_ERR_NULL, "bn_apply_from_sums: running_mean/var must both be set or both NULL");
    if (residual) { REQ_AL(residual, "residual"); REQ_LD(ldr, "ldr"); }
    const ColGrid g = col_grid(rows, c);
#define GLF_BNF(RES_) hipLaunchKernelGGL((bn_apply_sums_kernel<RES_>), col_dim(g), dim3(256), 0, glf::S(s), x, ldx, residual, ldr, y, ldy, sums, rows, c, \
                                         eps, momentum, gamma, beta, mean, invstd, running_mean, running_var,                                      \
                                         reinterpret_cast<long long*>(num_batches_tracked), g.tpr, g.cblocks, g.slices, relu, amax_out, relu_mask, colmax)
    if (residual) GLF_BNF(true); else GLF_BNF(false);
#undef GLF_BNF
    return glf::check_launch("bn_apply_from_sums");
}

extern "C" int glf_bn_bwd(const float* dy, int lddy, const float* x, int ldx, const float* y, int ldy,
                          const float* mean, const float* invstd, const float* gamma, const float* beta,
                          float* dx, int lddx, float* dres, int lddres, float* dgamma, float* dbeta,
                          int rows, int c, int relu, int training, double* workspace, float* amax_out, int packed_dx,
                          const uint8_t* relu_mask, const float* dy2, int lddy2, double* fused_sums, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && x && mean && invstd && gamma && dx && (workspace || fused_sums), GLF_ERR_NULL, "bn_bwd: null argument");
    if (relu_mask) y = nullptr;
    GLF_REQUIRE(!packed_dx || packed_dx == 4 || amax_out, GLF_ERR_NULL, "bn_bwd: packed_dx needs amax_out (a zeroed device float that receives the bound the image is scaled with)");
    GLF_REQUIRE(!relu || y || beta || relu_mask, GLF_ERR_NULL, "bn_bwd: relu != 0 needs relu_mask, y (the forward output) or beta (to recompute its sign from x)");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_bwd: rows must be > 0");
    REQ_C4(c); REQ_AL(dy, "dy"); REQ_AL(x, "x"); REQ_AL(dx, "dx"); REQ_LD(lddy, "lddy"); REQ_LD(ldx, "ldx"); REQ_LD(lddx, "lddx");
    if (relu && y) { REQ_AL(y, "y"); REQ_LD(ldy, "ldy"); }
    if (dres) { REQ_AL(dres, "dres"); REQ_LD(lddres, "lddres"); }
    if (dy2) { REQ_AL(dy2, "dy2"); REQ_LD(lddy2, "lddy2"); }
    const OpBnBwd op{{dy, lddy, x, ldx, y, ldy, mean, invstd, gamma, beta, relu, relu_mask, c / 4, dy2, lddy2}};
    const ColGrid ag = col_grid(rows, c);
    BwdApply ap{dy, lddy, x, ldx, y, ldy, Coef{mean, invstd, gamma, beta}, nullptr, nullptr, dx, lddx, dres, lddres,
                rows, c, ag.tpr, ag.cblocks, ag.slices, training, 1.0f / (float)rows,
                amax_out, packed_dx == 4 ? 0 : packed_dx, relu_mask, dy2, lddy2, nullptr, nullptr, nullptr, nullptr};
    // packed_dx = 2 / 3: the two halves of the packed three-launch form for SEVERAL layers whose images share one scale (column
    // slices of one buffer): 2 = reduction + finalize only (dgamma / dbeta final, the bound raised into *amax_out by atomic max),
    // 3 = the apply pass only, scaled by *amax_out -- the caller runs every layer's half 2 before the first half 3.  Half 3 reads
    // the sums from `fused_sums` (here 2 c floats the CALLER owns, written by half 2), never from dgamma / dbeta: those are handed
    // on after half 2 and may be summed over ranks or accumulated into before half 3 runs.  4 = half 3 with dx written as plain
    // fp32 (max |dx| raised into *amax_out when given): the apply behind a reduction that left its sums in fused_sums the same way
    // (glf_bn_res_ln_bwd_sums)
    const int phase = packed_dx >= 2 ? packed_dx : 0;
    GLF_REQUIRE(packed_dx >= 0 && packed_dx <= 4, GLF_ERR_BAD_SHAPE, "bn_bwd: packed_dx must be 0 .. 4");
    GLF_REQUIRE(!phase || (workspace && fused_sums), GLF_ERR_NULL, "bn_bwd: packed_dx = 2 / 3 / 4 needs the workspace and fused_sums (2 c floats kept from half 2 to half 3)");
    GLF_REQUIRE(phase != 2 || (dgamma && dbeta), GLF_ERR_NULL, "bn_bwd: packed_dx = 2 needs dgamma and dbeta");
    float* keep = phase ? reinterpret_cast<float*>(fused_sums) : (float*)nullptr;
    if (!phase && fused_sums && c <= APPLY_MAX_C) {
        // two launches: reduction with atomics into the caller's ZERO-FILLED buffer (2 c doubles, then 2 c floats of maxima), apply
        float* fmax = reinterpret_cast<float*>(fused_sums + (size_t)2 * c);
        // a fan-in pair with a residual gradient wanted: the reduction stores the masked sum to dres, and the apply pass reads
        // it back as its (already masked) dy instead of dy, dy2 and the sign bytes -- 28.25 instead of 32.5 bytes per element
        const bool wres = dy2 && dres;
        GLF_REQUIRE(!wres || (dres != dy && dres != dy2 && dres != x), GLF_ERR_BAD_SHAPE, "bn_bwd: dres must not alias dy, dy2 or x");
        if (int rc = launch_bnbwd_reduce<float>(op, rows, c, fused_sums, packed_dx ? fmax : (float*)nullptr, wres ? dres : (float*)nullptr, lddres,
                                                glf::S(s), "bn_bwd_reduce(fused)")) return rc;
        ap.fsums = fused_sums; ap.fmax = fmax; ap.out_dbeta = dbeta; ap.out_dgamma = dgamma;
        if (wres) {
            ap.dy = dres; ap.lddy = lddres; ap.dy2 = nullptr; ap.mask = nullptr; ap.y = nullptr; ap.dres = nullptr;
            return launch_bwd_apply(ap, 0, glf::S(s));
        }
        return launch_bwd_apply(ap, relu, glf::S(s));
    }
    GLF_REQUIRE(workspace, GLF_ERR_NULL, "bn_bwd: the three-launch form needs the workspace");
    const int slices = n_slices_c(rows, c);
    // per-channel sums live behind the partials in the workspace (as floats) when the caller does not want them
    float* sums = reinterpret_cast<float*>(workspace + (size_t)2 * slices * c);
    float* s_dy = dbeta ? dbeta : sums;
    float* s_dyx = dgamma ? dgamma : sums + c;
    if (phase >= 3) {
        s_dy = keep; s_dyx = keep + c;      // the sums are where half 2 kept them, the bound in *amax_out
    } else if (packed_dx) {
        float* pmax = reinterpret_cast<float*>(workspace + (size_t)2 * slices * c + (size_t)2 * c);
        const int c4 = c / 4, tpr = c4 < RT ? c4 : RT;
        hipLaunchKernelGGL((colreduce_kernel<OpBnBwd, true>), dim3(slices, (c4 + tpr - 1) / tpr), dim3(RT), 0, glf::S(s), op, rows, c, slices, workspace, pmax);
        if (int rc = glf::check_launch("bn_bwd_reduce")) return rc;
        hipLaunchKernelGGL(bnbwd_finalize, dim3((c + FIN_CH - 1) / FIN_CH), dim3(256), 0, glf::S(s), workspace, pmax, slices, c, gamma, invstd,
                           1.0f / (float)rows, training, s_dy, s_dyx, amax_out, keep);
    } else {
        if (int rc = launch_colreduce(op, rows, c, workspace, glf::S(s))) return rc;
        hipLaunchKernelGGL(sum_finalize, dim3((c + FIN_CH - 1) / FIN_CH), dim3(256), 0, glf::S(s), workspace, slices, c, s_dy, s_dyx);
    }
    if (int rc = glf::check_launch("bn_bwd_finalize")) return rc;
    if (phase == 2) return GLF_OK;
    ap.sum_dy = s_dy; ap.sum_dyx = s_dyx;
    return launch_bwd_apply(ap, relu, glf::S(s));
}

extern "C" int glf_colsum(const float* dy, int lddy, float* db, int rows, int c, double* workspace, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && db && workspace, GLF_ERR_NULL, "colsum: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "colsum: rows must be > 0");
    REQ_C4(c); REQ_AL(dy, "dy"); REQ_LD(lddy, "lddy");
    if (int rc = launch_colreduce(OpColsum{dy, lddy}, rows, c, workspace, glf::S(s))) return rc;
    hipLaunchKernelGGL(sum_finalize, dim3((c + FIN_CH - 1) / FIN_CH), dim3(256), 0, glf::S(s), workspace, n_slices_c(rows, c), c, db, (float*)nullptr);
    return glf::check_launch("colsum_finalize");
}

// ---- bf16 storage: the same entry points over 16-byte accesses of eight bf16 (C % 8 == 0)
extern "C" int glf_s16_colstats(const void* x, int ldx, int rows, int c, double* sums, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && sums, GLF_ERR_NULL, "s16_colstats: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "s16_colstats: rows must be > 0");
    REQ_C8(c); REQ_AL(x, "x"); REQ_LD8(ldx, "ldx");
    return launch_colreduce16(OpStats16{static_cast<const u16*>(x), ldx}, rows, c, sums, glf::S(s));
}

extern "C" int glf_s16_bn_apply(const void* x, int ldx, const void* residual, int ldr, void* y, int ldy, const double* sums,
                                int rows, int c, float eps, float momentum, const float* gamma, const float* beta,
                                float* mean, float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                int relu, uint8_t* relu_mask, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && mean && invstd && gamma && beta, GLF_ERR_NULL, "s16_bn_apply: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "s16_bn_apply: rows must be > 0");
    REQ_C8(c); REQ_AL(x, "x"); REQ_AL(y, "y"); REQ_LD8(ldx, "ldx"); REQ_LD8(ldy, "ldy");
    GLF_REQUIRE(c <= APPLY_MAX_C, GLF_ERR_UNSUPPORTED, "s16_bn_apply: C must be <= %d", APPLY_MAX_C);
    GLF_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GLF_ERR_NULL, "s16_bn_apply: running_mean/var must both be set or both NULL");
    if (residual) { REQ_AL(residual, "residual"); REQ_LD8(ldr, "ldr"); }
    const long long total8 = (long long)rows * (c / 8);
    hipLaunchKernelGGL(s16_bn_apply_kernel, dim3(stream_grid(total8, 256)), dim3(256), (size_t)2 * c * sizeof(float), glf::S(s),
                       static_cast<const u16*>(x), ldx, static_cast<const u16*>(residual), ldr, static_cast<u16*>(y), ldy, sums, rows, c, eps, momentum,
                       gamma, beta, mean, invstd, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), total8, c / 8, relu,
                       relu_mask);
    return glf::check_launch("s16_bn_apply");
}

extern "C" int glf_s16_bn_bwd(const void* dy, int lddy, const void* dy2, int lddy2, const void* x, int ldx,
                              const float* mean, const float* invstd, const float* gamma, const float* beta,
                              void* dx, int lddx, void* dres, int lddres, float* dgamma, float* dbeta,
                              int rows, int c, int relu, int training, double* sums, const uint8_t* relu_mask, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && x && mean && invstd && gamma && dx && sums, GLF_ERR_NULL, "s16_bn_bwd: null argument");
    GLF_REQUIRE(!relu || beta || relu_mask, GLF_ERR_NULL, "s16_bn_bwd: relu != 0 needs relu_mask or beta (to recompute the sign from x)");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "s16_bn_bwd: rows must be > 0");
    REQ_C8(c); REQ_AL(dy, "dy"); REQ_AL(x, "x"); REQ_AL(dx, "dx"); REQ_LD8(lddy, "lddy"); REQ_LD8(ldx, "ldx"); REQ_LD8(lddx, "lddx");
    GLF_REQUIRE(c <= APPLY_MAX_C, GLF_ERR_UNSUPPORTED, "s16_bn_bwd: C must be <= %d", APPLY_MAX_C);
    if (dres) { REQ_AL(dres, "dres"); REQ_LD8(lddres, "lddres"); }
    if (dy2) { REQ_AL(dy2, "dy2"); REQ_LD8(lddy2, "lddy2"); }
    const BnBwdIn<u16> op{static_cast<const u16*>(dy), lddy, static_cast<const u16*>(x), ldx, nullptr, 0, mean, invstd, gamma, beta,
                          relu, relu_mask, c / 8, static_cast<const u16*>(dy2), lddy2};
    if (int rc = launch_bnbwd_reduce<u16>(op, rows, c, sums, nullptr, nullptr, 0, glf::S(s), "s16_bn_bwd_reduce")) return rc;
    const long long total8 = (long long)rows * (c / 8);
    hipLaunchKernelGGL(s16_bnbwd_apply_kernel, dim3(stream_grid(total8, 256)), dim3(256), (size_t)2 * c * sizeof(float), glf::S(s),
                       static_cast<const u16*>(dy), lddy, static_cast<const u16*>(dy2), lddy2, static_cast<const u16*>(x), ldx, mean, invstd, gamma, beta,
                       sums, static_cast<u16*>(dx), lddx, static_cast<u16*>(dres), lddres, dgamma, dbeta, total8, c / 8, c, relu, training,
                       1.0f / (float)rows, relu_mask);
    return glf::check_launch("s16_bn_bwd_apply");
}

extern "C" int glf_s16_colsum(const void* dy, int lddy, float* db, int rows, int c, double* workspace, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && db && workspace, GLF_ERR_NULL, "s16_colsum: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "s16_colsum: rows must be > 0");
    REQ_C8(c); REQ_AL(dy, "dy"); REQ_LD8(lddy, "lddy");
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)2 * c * sizeof(double), glf::S(s));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "s16_colsum: hipMemsetAsync: %s", hipGetErrorString(e));
    if (int rc = launch_colreduce16(OpColsum16{static_cast<const u16*>(dy), lddy}, rows, c, workspace, glf::S(s))) return rc;
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3((c + 255) / 256), dim3(256), 0, glf::S(s), workspace, db, c);
    return glf::check_launch("s16_colsum");
}

extern "C" int glf_bn_res_ln_fwd(const float* w, const float* x, const float* bn_mean, const float* bn_invstd,
                                 const float* bn_gamma, const float* bn_beta, const float* ln_gamma,
                                 const float* ln_beta, float ln_eps, float* z, float* row_mean, float* row_rstd,
                                 int rows, int c, float* amax_out, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(w && x && bn_mean && bn_invstd && bn_gamma && bn_beta && ln_gamma && ln_beta && z && row_mean && row_rstd,
                GLF_ERR_NULL, "bn_res_ln_fwd: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_res_ln_fwd: rows must be > 0");
    REQ_C4(c); GLF_REQUIRE(c <= 64 * 4 * LN_NV, GLF_ERR_UNSUPPORTED, "bn_res_ln: C must be <= %d", 64 * 4 * LN_NV);
    REQ_AL(w, "w"); REQ_AL(x, "x"); REQ_AL(z, "z");
    hipLaunchKernelGGL((bn_res_ln_kernel<false>), dim3((rows + 3) / 4), dim3(256), 0, glf::S(s), w, x,
                       Coef{bn_mean, bn_invstd, bn_gamma, bn_beta}, ln_gamma, ln_beta, ln_eps, z, row_mean, row_rstd,
                       (const float*)nullptr, (float*)nullptr, rows, c, amax_out);
    return glf::check_launch("bn_res_ln_fwd");
}

extern "C" int glf_bn_res_ln_bwd(const float* dz, const float* w, const float* x, const float* bn_mean,
                                 const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                                 const float* ln_gamma, const float* row_mean, const float* row_rstd,
                                 float* du, float* dln_gamma, float* dln_beta, int rows, int c,
                                 double* workspace, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dz && w && x && bn_mean && bn_invstd && bn_gamma && bn_beta && ln_gamma && row_mean && row_rstd && du &&
                dln_gamma && dln_beta && workspace, GLF_ERR_NULL, "bn_res_ln_bwd: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_res_ln_bwd: rows must be > 0");
    REQ_C4(c); GLF_REQUIRE(c <= 64 * 4 * LN_NV, GLF_ERR_UNSUPPORTED, "bn_res_ln: C must be <= %d", 64 * 4 * LN_NV);
    REQ_AL(dz, "dz"); REQ_AL(w, "w"); REQ_AL(x, "x"); REQ_AL(du, "du");
    const Coef bn{bn_mean, bn_invstd, bn_gamma, bn_beta};
    hipLaunchKernelGGL((bn_res_ln_kernel<true>), dim3((rows + 3) / 4), dim3(256), 0, glf::S(s), w, x, bn, ln_gamma,
                       (const float*)nullptr, 0.f, (float*)nullptr, const_cast<float*>(row_mean), const_cast<float*>(row_rstd),
                       dz, du, rows, c, (float*)nullptr);
    if (int rc = glf::check_launch("bn_res_ln_bwd")) return rc;
    if (int rc = launch_colreduce(OpLnParam{dz, w, x, bn, row_mean, row_rstd, c}, rows, c, workspace, glf::S(s))) return rc;
    hipLaunchKernelGGL(sum_finalize, dim3((c + FIN_CH - 1) / FIN_CH), dim3(256), 0, glf::S(s), workspace, n_slices_c(rows, c), c, dln_gamma, dln_beta);
    return glf::check_launch("ln_param_finalize");
}

extern "C" int glf_bn_res_ln_bwd_sums(const float* dz, const float* w, const float* x, const float* bn_mean,
                                      const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                                      const float* ln_gamma, const float* row_mean, const float* row_rstd,
                                      float* du, float* dln_gamma, float* dln_beta, float* dbn_gamma, float* dbn_beta,
                                      float* bn_sums, float* amax_out, int rows, int c, int training,
                                      double* workspace, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dz && w && x && bn_mean && bn_invstd && bn_gamma && bn_beta && ln_gamma && row_mean && row_rstd && du &&
                dln_gamma && dln_beta && dbn_gamma && dbn_beta && bn_sums && workspace, GLF_ERR_NULL, "bn_res_ln_bwd_sums: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "bn_res_ln_bwd_sums: rows must be > 0");
    REQ_C4(c); GLF_REQUIRE(c <= 64 * 4 * LN_NV, GLF_ERR_UNSUPPORTED, "bn_res_ln: C must be <= %d", 64 * 4 * LN_NV);
    REQ_AL(dz, "dz"); REQ_AL(w, "w"); REQ_AL(x, "x"); REQ_AL(du, "du");
    // du is written TA_R rows at a time while later rows of the inputs are still to be read, by other workgroups too
    GLF_REQUIRE(du != dz && du != w && du != x, GLF_ERR_BAD_SHAPE, "bn_res_ln_bwd_sums: du must not alias dz, w or x");
    const int slices = tail_slices(rows);
    float* pmax = reinterpret_cast<float*>(workspace + (size_t)4 * slices * c);      // 4 S c doubles + 2 S c floats <= glf_bn_workspace
    hipLaunchKernelGGL(bn_res_ln_bwd_sums_kernel, dim3(slices), dim3(256), 0, glf::S(s), dz, w, x, Coef{bn_mean, bn_invstd, bn_gamma, bn_beta},
                       ln_gamma, row_mean, row_rstd, du, rows, c, slices, workspace, pmax);
    if (int rc = glf::check_launch("bn_res_ln_bwd_sums")) return rc;
    hipLaunchKernelGGL(tail_bwd_finalize, dim3((c + FIN_CH - 1) / FIN_CH, 2), dim3(256), 0, glf::S(s), workspace, pmax, slices, c, bn_gamma,
                       bn_invstd, 1.0f / (float)rows, training, dln_gamma, dln_beta, dbn_beta, dbn_gamma, amax_out, bn_sums);
    return glf::check_launch("tail_bwd_finalize");
}

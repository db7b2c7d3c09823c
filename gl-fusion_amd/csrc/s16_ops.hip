// 16-bit-storage ("S16") streaming kernels of the GL-Fusion path that have no fp32-storage counterpart to share a body or a file
// with: the TPAVI tail, the per-frame row sums, the casts and the softmax rows, when activations, saved tensors and activation
// gradients live in HBM as bf16 (BASELINE configs 3 / 5).  All HBM-bound: 16-byte accesses (eight channels per lane), fp32
// arithmetic in registers, one rounding to bf16 at the store.  Channels-last [rows][C], C % 8 == 0.
// (BatchNorm and the column reductions of both storages: norm.hip; the pointwise ops of both: pointwise.hip.)
#include "stream_common.h"

using namespace glf;

namespace {

// ----------------------------------------------------------------------------------------------------------------------
// TPAVI tail z = LayerNorm_C(BN(w) + x): one wavefront per row, C <= 2048
// ----------------------------------------------------------------------------------------------------------------------
constexpr int LN_NV = 4;       // 8 channels x 64 lanes x 4 = 2048
constexpr int LN_ROWS = 64;    // backward: rows per workgroup (4 waves x 16 rows), one slab of column partials per workgroup

__global__ __launch_bounds__(256) void s16_bn_res_ln_fwd_kernel(const u16* __restrict__ w, const u16* __restrict__ x, const float* __restrict__ bn_mean,
                                                                const float* __restrict__ bn_invstd, const float* __restrict__ bn_g,
                                                                const float* __restrict__ bn_b, const float* __restrict__ ln_g,
                                                                const float* __restrict__ ln_b, float eps, u16* __restrict__ z,
                                                                float* __restrict__ row_mean, float* __restrict__ row_rstd, int rows, int c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c8 = c >> 3;
    const long long base = (long long)row * c;
    F8 u[LN_NV];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < LN_NV; ++v) {
        const int cc = lane + 64 * v;
        if (cc < c8) {
            const int ch = cc * 8;
            const F8 ww = ld8(w + base + ch), xx = ld8(x + base + ch);
            const F8 mu = ldf8(bn_mean + ch), is = ldf8(bn_invstd + ch), ga = ldf8(bn_g + ch), be = ldf8(bn_b + ch);
#pragma unroll
            for (int j = 0; j < 8; ++j) { u[v].v[j] = (ww.v[j] - mu.v[j]) * is.v[j] * ga.v[j] + be.v[j] + xx.v[j]; s += u[v].v[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) u[v].v[j] = 0.f;
        }
    }
    const float mean = wave_sum(s) / c;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < LN_NV; ++v)
        if (lane + 64 * v < c8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = u[v].v[j] - mean; q += d * d; }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / c + eps);
    if (lane == 0) { row_mean[row] = mean; row_rstd[row] = rstd; }
#pragma unroll
    for (int v = 0; v < LN_NV; ++v) {
        const int cc = lane + 64 * v;
        if (cc < c8) {
            const int ch = cc * 8;
            const F8 g = ldf8(ln_g + ch), b = ldf8(ln_b + ch);
            F8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = (u[v].v[j] - mean) * rstd * g.v[j] + b.v[j];
            st8(z + base + ch, o);
        }
    }
}

// backward: du (gradient of u = BN(w) + x) per row, and per-workgroup partial column sums (dz * uhat, dz) of its LN_ROWS rows
// into slab[blockIdx.x][2][c] (floats); s16_ln_param_finalize folds the slabs in order.
__global__ __launch_bounds__(256) void s16_bn_res_ln_bwd_kernel(const u16* __restrict__ dz, const u16* __restrict__ w, const u16* __restrict__ x,
                                                                const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd,
                                                                const float* __restrict__ bn_g, const float* __restrict__ bn_b,
                                                                const float* __restrict__ ln_g, const float* __restrict__ row_mean,
                                                                const float* __restrict__ row_rstd, u16* __restrict__ du, float* __restrict__ slab,
                                                                int rows, int c) {
    __shared__ float sh[2 * 2048];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c8 = c >> 3;
    F8 pg[LN_NV], pb[LN_NV];                     // partial sums of dz * uhat and dz over this wave's rows
#pragma unroll
    for (int v = 0; v < LN_NV; ++v)
#pragma unroll
        for (int j = 0; j < 8; ++j) { pg[v].v[j] = 0.f; pb[v].v[j] = 0.f; }
    const int row0 = blockIdx.x * LN_ROWS + wv * (LN_ROWS / 4);
    for (int rr = 0; rr < LN_ROWS / 4; ++rr) {
        const int row = row0 + rr;
        if (row >= rows) break;
        const long long base = (long long)row * c;
        const float mean = row_mean[row], rstd = row_rstd[row];
        F8 uh[LN_NV], gz[LN_NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < LN_NV; ++v) {
            const int cc = lane + 64 * v;
            if (cc < c8) {
                const int ch = cc * 8;
                const F8 ww = ld8(w + base + ch), xx = ld8(x + base + ch), d = ld8(dz + base + ch);
                const F8 mu = ldf8(bn_mean + ch), is = ldf8(bn_invstd + ch), ga = ldf8(bn_g + ch), be = ldf8(bn_b + ch), g = ldf8(ln_g + ch);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float uu = (ww.v[j] - mu.v[j]) * is.v[j] * ga.v[j] + be.v[j] + xx.v[j];
                    uh[v].v[j] = (uu - mean) * rstd;
                    gz[v].v[j] = d.v[j] * g.v[j];
                    s1 += gz[v].v[j];
                    s2 += gz[v].v[j] * uh[v].v[j];
                    pg[v].v[j] += d.v[j] * uh[v].v[j];
                    pb[v].v[j] += d.v[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) { uh[v].v[j] = 0.f; gz[v].v[j] = 0.f; }
            }
        }
        const float m1 = wave_sum(s1) / c, m2 = wave_sum(s2) / c;
#pragma unroll
        for (int v = 0; v < LN_NV; ++v) {
            const int cc = lane + 64 * v;
            if (cc < c8) {
                F8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o.v[j] = rstd * (gz[v].v[j] - m1 - uh[v].v[j] * m2);
                st8(du + base + cc * 8, o);
            }
        }
    }
    // fold the four waves' partials through LDS, wave after wave (same lane <-> channel map in every wave)
    for (int k = 0; k < 4; ++k) {
        if (wv == k) {
#pragma unroll
            for (int v = 0; v < LN_NV; ++v) {
                const int cc = lane + 64 * v;
                if (cc < c8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int ch = cc * 8 + j;
                        if (k == 0) { sh[ch] = pg[v].v[j]; sh[2048 + ch] = pb[v].v[j]; }
                        else { sh[ch] += pg[v].v[j]; sh[2048 + ch] += pb[v].v[j]; }
                    }
                }
            }
        }
        __syncthreads();
    }
    float* dst = slab + (long long)blockIdx.x * 2 * c;
    for (int ch = threadIdx.x; ch < c; ch += 256) { dst[ch] = sh[ch]; dst[c + ch] = sh[2048 + ch]; }
}
__global__ __launch_bounds__(256) void s16_ln_param_finalize(const float* __restrict__ slab, int nslab, int c, float* __restrict__ dg, float* __restrict__ db) {
    // a workgroup = 16 (statistic, channel) columns x 16 slab lanes; every lane adds its slabs in order in double, lane 0 folds the
    // 16 lane sums in order: a fixed summation tree => bitwise reproducible
    __shared__ double sh[256];
    const int cx = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + cx;
    double s = 0;
    if (i < 2 * c)
        for (int k = lane; k < nslab; k += 16) s += slab[(long long)k * 2 * c + i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (lane == 0 && i < 2 * c) {
        for (int l = 1; l < 16; ++l) s += sh[l * 16 + cx];
        if (i < c) dg[i] = (float)s; else db[i - c] = (float)s;
    }
}

// ----------------------------------------------------------------------------------------------------------------------
// per-frame row sums, casts (the other streaming ops share their kernel bodies with fp32 storage: pointwise.hip)
// ----------------------------------------------------------------------------------------------------------------------
// y[n][c] = scale * sum_p x[n][p][c]   (x row stride ld); y bf16 or fp32 (the ASPP pooled branch keeps its N per-frame vectors
// in fp32: its BatchNorm normalises over the N frames, whose averages differ by less than a few bf16 steps)
__global__ __launch_bounds__(256) void s16_sum_rows_kernel(const u16* __restrict__ x, int ld, void* __restrict__ yv, int y_f32, float scale, int p, int c) {
    // workgroup = 32 channel groups of 8 x 8 row lanes; grid (c / 256, n)
    __shared__ float sh[256 * 8];
    const int n = blockIdx.y;
    const int cg = blockIdx.x * 32 + (threadIdx.x & 31);       // group of 8 channels
    const int pl = threadIdx.x >> 5;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (cg * 8 < c) {
        const u16* base = x + (long long)n * p * ld + cg * 8;
        int r = pl;
        for (; r + 24 < p; r += 32) {                                   // four rows' loads in flight
            const uint4 q0 = *reinterpret_cast<const uint4*>(base + (long long)r * ld);
            const uint4 q1 = *reinterpret_cast<const uint4*>(base + (long long)(r + 8) * ld);
            const uint4 q2 = *reinterpret_cast<const uint4*>(base + (long long)(r + 16) * ld);
            const uint4 q3 = *reinterpret_cast<const uint4*>(base + (long long)(r + 24) * ld);
            const F8 v0 = unpack8(q0), v1 = unpack8(q1), v2 = unpack8(q2), v3 = unpack8(q3);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += (v0.v[j] + v1.v[j]) + (v2.v[j] + v3.v[j]);
        }
        for (; r < p; r += 8) {
            const F8 v = ld8(base + (long long)r * ld);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += v.v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[j * 256 + threadIdx.x] = s[j];
    __syncthreads();
    if (pl == 0 && cg * 8 < c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = s[j];
            for (int q = 1; q < 8; ++q) v += sh[j * 256 + q * 32 + (threadIdx.x & 31)];
            v *= scale;
            if (y_f32) static_cast<float*>(yv)[(long long)n * c + cg * 8 + j] = v;
            else static_cast<u16*>(yv)[(long long)n * c + cg * 8 + j] = f2bf(v);
        }
    }
}
__global__ __launch_bounds__(256) void s16_to_f32_kernel(const u16* __restrict__ x, float* __restrict__ y, long long n8) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const F8 v = ld8(x + i * 8);
        *reinterpret_cast<float4*>(y + i * 8) = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
        *reinterpret_cast<float4*>(y + i * 8 + 4) = make_float4(v.v[4], v.v[5], v.v[6], v.v[7]);
    }
}
__global__ __launch_bounds__(256) void s16_from_f32_kernel(const float* __restrict__ x, u16* __restrict__ y, long long n8) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) st8(y + i * 8, ldf8(x + i * 8));
}

// ----------------------------------------------------------------------------------------------------------------------
// row softmax of fp32 scores into a bf16 operand ('gaussian' under 16-bit storage, ops16.py): P = softmax(S) and
// dS = P o (dP - rowsum(P o dP)) with P recomputed from the scores.  TPR threads per row (one wavefront, or the whole
// workgroup for long rows), 8 columns per thread and access; row max / sum (/ sum of P dP) as ONE online pass in fp32, merged
// in a fixed order, then the normalising pass; bf16 once, at the store; the pad columns [cols, ld) are written as zero.
// ----------------------------------------------------------------------------------------------------------------------
struct SmStat { float m, l, d; };      // running maximum, sum of exp(s - m), sum of exp(s - m) dp
__device__ __forceinline__ SmStat sm_merge(const SmStat x, const SmStat y) {
    const float m = fmaxf(x.m, y.m);
    if (m == -INFINITY) return SmStat{m, 0.f, 0.f};
    const float ax = __expf(x.m - m), ay = __expf(y.m - m);
    return SmStat{m, x.l * ax + y.l * ay, x.d * ax + y.d * ay};
}
// columns c0 .. c0 + 7 of a row, `fill` at and beyond cols
__device__ __forceinline__ F8 sm_ld8(const float* __restrict__ r, int c0, int cols, float fill) {
    if (c0 + 8 <= cols) return ldf8(r + c0);
    F8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = c0 + e < cols ? r[c0 + e] : fill;
    return o;
}
template <int TPR, bool BWD>
__device__ __forceinline__ SmStat sm_row_stats(const float* __restrict__ srow, const float* __restrict__ dprow, int cols, int t, SmStat* red) {
    SmStat st{-INFINITY, 0.f, 0.f};
    for (int c0 = 8 * t; c0 < cols; c0 += 8 * TPR) {
        const F8 x = sm_ld8(srow, c0, cols, -INFINITY);
        F8 dp;
        if (BWD) dp = sm_ld8(dprow, c0, cols, 0.f);
        float gm = x.v[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) gm = fmaxf(gm, x.v[e]);
        SmStat g{gm, 0.f, 0.f};                            // (column c0 < cols: the group's maximum is finite)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = __expf(x.v[e] - gm);
            g.l += p;
            if (BWD) g.d = fmaf(p, dp.v[e], g.d);
        }
        st = sm_merge(st, g);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        SmStat y;
        y.m = __shfl_xor(st.m, o, 64); y.l = __shfl_xor(st.l, o, 64); y.d = __shfl_xor(st.d, o, 64);
        st = sm_merge(st, y);
    }
    // one value per wavefront: with contracted multiply-adds the two lanes of a butterfly pair can differ in the last bit
    st.m = __shfl(st.m, 0, 64); st.l = __shfl(st.l, 0, 64); st.d = __shfl(st.d, 0, 64);
    if (TPR > 64) {                                        // one row per workgroup: the four wavefronts' results, in wave order
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = st;
        __syncthreads();
        st = sm_merge(sm_merge(red[0], red[1]), sm_merge(red[2], red[3]));
    }
    return st;
}
template <int TPR, bool BWD>
__global__ __launch_bounds__(256) void s16_softmax_rows_kernel(const float* __restrict__ s, const float* __restrict__ dp, u16* __restrict__ out,
                                                               long long rows, int cols, long long ld_s, long long ld_dp, long long ld_o) {
    __shared__ SmStat red[4];
    const int t = threadIdx.x % TPR;
    const long long row = (long long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    if (row >= rows) return;                               // (whole wavefronts; TPR = 256 launches exactly `rows` workgroups)
    const float* __restrict__ srow = s + row * ld_s;
    const float* __restrict__ dprow = BWD ? dp + row * ld_dp : nullptr;
    const SmStat st = sm_row_stats<TPR, BWD>(srow, dprow, cols, t, red);
    const float inv = 1.f / st.l, dsum = st.d * inv;
    u16* __restrict__ orow = out + row * ld_o;
    for (int c0 = 8 * t; c0 < (int)ld_o; c0 += 8 * TPR) {
        F8 o;
        if (c0 < cols) {
            const F8 x = sm_ld8(srow, c0, cols, -INFINITY);
            F8 d;
            if (BWD) d = sm_ld8(dprow, c0, cols, 0.f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float p = __expf(x.v[e] - st.m) * inv;   // 0 at and beyond cols
                o.v[e] = BWD ? p * (d.v[e] - dsum) : p;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o.v[e] = 0.f;
        }
        st8(orow + c0, o);
    }
}

int softmax16_check(const void* s, const void* dp, const void* out, int64_t rows, int cols, int64_t ld_s, int64_t ld_dp, int64_t ld_o, bool bwd,
                    const char* who) {
    GLF_REQUIRE(s && out && (!bwd || dp), GLF_ERR_NULL, "%s: null argument", who);
    GLF_REQUIRE(rows > 0 && rows < (1LL << 31) && cols > 0 && ld_s >= cols && ld_o >= cols && ld_o < (1LL << 31) && (!bwd || ld_dp >= cols),
                GLF_ERR_BAD_SHAPE, "%s: rows (%lld) / cols (%d) / row strides out of range", who, (long long)rows, cols);
    GLF_REQUIRE(ld_s % 4 == 0 && ld_o % 8 == 0 && al16(s) && al16(out) && (!bwd || (ld_dp % 4 == 0 && al16(dp))), GLF_ERR_UNSUPPORTED,
                "%s: fp32 row strides must be multiples of 4, the bf16 row stride a multiple of 8, every operand 16-byte aligned", who);
    return GLF_OK;
}
template <bool BWD>
void softmax16_launch(const float* s, const float* dp, void* out, int64_t rows, int cols, int64_t ld_s, int64_t ld_dp, int64_t ld_o, glf_stream_t st) {
    if (cols <= 1024)
        hipLaunchKernelGGL((s16_softmax_rows_kernel<64, BWD>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, glf::S(st), s, dp, static_cast<u16*>(out),
                           (long long)rows, cols, (long long)ld_s, (long long)ld_dp, (long long)ld_o);
    else
        hipLaunchKernelGGL((s16_softmax_rows_kernel<256, BWD>), dim3((unsigned)rows), dim3(256), 0, glf::S(st), s, dp, static_cast<u16*>(out),
                           (long long)rows, cols, (long long)ld_s, (long long)ld_dp, (long long)ld_o);
}

}  // namespace

extern "C" int glf_s16_bn_res_ln_fwd(const void* w, const void* x, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                     const float* bn_beta, const float* ln_gamma, const float* ln_beta, float ln_eps, void* z,
                                     float* row_mean, float* row_rstd, int rows, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(w && x && bn_mean && bn_invstd && bn_gamma && bn_beta && ln_gamma && ln_beta && z && row_mean && row_rstd, GLF_ERR_NULL,
                "s16_bn_res_ln_fwd: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "s16_bn_res_ln_fwd: rows must be > 0");
    REQ_C8(c); GLF_REQUIRE(c <= 64 * 8 * LN_NV, GLF_ERR_UNSUPPORTED, "s16_bn_res_ln: C must be <= %d", 64 * 8 * LN_NV);
    REQ_AL(w, "w"); REQ_AL(x, "x"); REQ_AL(z, "z");
    hipLaunchKernelGGL(s16_bn_res_ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, glf::S(s), static_cast<const u16*>(w), static_cast<const u16*>(x),
                       bn_mean, bn_invstd, bn_gamma, bn_beta, ln_gamma, ln_beta, ln_eps, static_cast<u16*>(z), row_mean, row_rstd, rows, c);
    return glf::check_launch("s16_bn_res_ln_fwd");
}

extern "C" size_t glf_s16_bn_res_ln_workspace(int rows, int c) {
    return (size_t)((rows + LN_ROWS - 1) / LN_ROWS) * 2 * (size_t)(c > 0 ? c : 0) * sizeof(float);
}

extern "C" int glf_s16_bn_res_ln_bwd(const void* dz, const void* w, const void* x, const float* bn_mean, const float* bn_invstd,
                                     const float* bn_gamma, const float* bn_beta, const float* ln_gamma, const float* row_mean,
                                     const float* row_rstd, void* du, float* dln_gamma, float* dln_beta, int rows, int c,
                                     float* workspace, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dz && w && x && bn_mean && bn_invstd && bn_gamma && bn_beta && ln_gamma && row_mean && row_rstd && du && dln_gamma && dln_beta &&
                workspace, GLF_ERR_NULL, "s16_bn_res_ln_bwd: null argument");
    GLF_REQUIRE(rows > 0, GLF_ERR_BAD_SHAPE, "s16_bn_res_ln_bwd: rows must be > 0");
    REQ_C8(c); GLF_REQUIRE(c <= 64 * 8 * LN_NV, GLF_ERR_UNSUPPORTED, "s16_bn_res_ln: C must be <= %d", 64 * 8 * LN_NV);
    REQ_AL(dz, "dz"); REQ_AL(w, "w"); REQ_AL(x, "x"); REQ_AL(du, "du");
    const int nslab = (rows + LN_ROWS - 1) / LN_ROWS;
    hipLaunchKernelGGL(s16_bn_res_ln_bwd_kernel, dim3(nslab), dim3(256), 0, glf::S(s), static_cast<const u16*>(dz), static_cast<const u16*>(w),
                       static_cast<const u16*>(x), bn_mean, bn_invstd, bn_gamma, bn_beta, ln_gamma, row_mean, row_rstd, static_cast<u16*>(du), workspace,
                       rows, c);
    if (int rc = glf::check_launch("s16_bn_res_ln_bwd")) return rc;
    hipLaunchKernelGGL(s16_ln_param_finalize, dim3((2 * c + 15) / 16), dim3(256), 0, glf::S(s), workspace, nslab, c, dln_gamma, dln_beta);
    return glf::check_launch("s16_ln_param_finalize");
}

extern "C" int glf_s16_sum_rows(const void* x, int ldx, void* y, int y_dtype, float scale, int n, int p, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "s16_sum_rows: null argument");
    GLF_REQUIRE(n > 0 && p > 0, GLF_ERR_BAD_SHAPE, "s16_sum_rows: bad extents");
    REQ_C8(c); REQ_AL(x, "x"); REQ_LD8(ldx, "ldx");
    GLF_REQUIRE(y_dtype == GLF_DT_F32 || y_dtype == GLF_DT_BF16, GLF_ERR_UNSUPPORTED, "s16_sum_rows: y_dtype must be GLF_DT_F32 or GLF_DT_BF16");
    hipLaunchKernelGGL(s16_sum_rows_kernel, dim3((c + 255) / 256, n), dim3(256), 0, glf::S(s), static_cast<const u16*>(x), ldx, y, y_dtype == GLF_DT_F32, scale, p, c);
    return glf::check_launch("s16_sum_rows");
}
extern "C" int glf_s16_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(src && dst, GLF_ERR_NULL, "s16_cast: null argument");
    GLF_REQUIRE(numel > 0 && numel % 8 == 0, GLF_ERR_BAD_SHAPE, "s16_cast: numel must be a positive multiple of 8");
    REQ_AL(src, "src"); REQ_AL(dst, "dst");
    if (src_dtype == GLF_DT_BF16 && dst_dtype == GLF_DT_F32)
        hipLaunchKernelGGL(s16_to_f32_kernel, dim3(stream_grid(numel / 8, 256)), dim3(256), 0, glf::S(s), static_cast<const u16*>(src), static_cast<float*>(dst),
                           (long long)(numel / 8));
    else if (src_dtype == GLF_DT_F32 && dst_dtype == GLF_DT_BF16)
        hipLaunchKernelGGL(s16_from_f32_kernel, dim3(stream_grid(numel / 8, 256)), dim3(256), 0, glf::S(s), static_cast<const float*>(src), static_cast<u16*>(dst),
                           (long long)(numel / 8));
    else
        return glf::fail(GLF_ERR_UNSUPPORTED, "s16_cast: built for bf16 -> f32 and f32 -> bf16");
    return glf::check_launch("s16_cast");
}

extern "C" int glf_s16_softmax_rows_fwd(const float* s, void* p, int64_t rows, int cols, int64_t ld_s, int64_t ld_p, glf_stream_t stream) {
    if (int rc = softmax16_check(s, nullptr, p, rows, cols, ld_s, 0, ld_p, false, "s16_softmax_rows_fwd")) return rc;
    if (int rc = glf::ensure_init()) return rc;
    softmax16_launch<false>(s, nullptr, p, rows, cols, ld_s, 0, ld_p, stream);
    return glf::check_launch("s16_softmax_rows_fwd");
}
extern "C" int glf_s16_softmax_rows_bwd(const float* s, const float* dp, void* ds, int64_t rows, int cols, int64_t ld_s, int64_t ld_dp, int64_t ld_ds,
                                        glf_stream_t stream) {
    if (int rc = softmax16_check(s, dp, ds, rows, cols, ld_s, ld_dp, ld_ds, true, "s16_softmax_rows_bwd")) return rc;
    if (int rc = glf::ensure_init()) return rc;
    softmax16_launch<true>(s, dp, ds, rows, cols, ld_s, ld_dp, ld_ds, stream);
    return glf::check_launch("s16_softmax_rows_bwd");
}

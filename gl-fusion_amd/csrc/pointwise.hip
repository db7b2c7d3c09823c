// HBM-bound pieces of the GL-Fusion path (gfx950): stem conv (Cin = 1), pooling, local gate,
// view stacking, bilinear up-sampling, loss and metric reductions, weight re-layout.
// All channels-last; 16-byte accesses wherever the channel count allows; 64-wide wavefront
// reductions via __shfl_xor.
//
// The streaming ops between the contractions (ReLU, dropout, axpby, max-pool, gate, frame adds, n-ary sum, row broadcast) exist for
// fp32 and for bf16 storage (glf_* / glf_s16_*): ONE kernel body each, templated on <storage type T, elements per access W> through
// Stream<T, W> (stream_common.h), instantiated as <float, 1> / <float, 4> / <u16, 8>.
#include "stream_common.h"
#include "split_f16.h"

using namespace glf;

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------
// weight re-layout
// ---------------------------------------------------------------------------------------
__global__ void oihw_to_tap_kernel(const float* __restrict__ w, float* __restrict__ out, long long co_ci, int taps) {
    // out[t][i] = w[i][t], i = co*cin + ci
    for (long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x; o < co_ci * taps; o += (long long)gridDim.x * blockDim.x) {
        const long long t = o / co_ci, i = o - t * co_ci;
        out[o] = w[i * taps + t];
    }
}
__global__ void tap_to_oihw_kernel(const float* __restrict__ w, float* __restrict__ out, long long co_ci, int taps) {
    for (long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x; o < co_ci * taps; o += (long long)gridDim.x * blockDim.x) {
        const long long i = o / taps, t = o - i * taps;
        out[o] = w[t * co_ci + i];
    }
}

// out[t][ci][co] = w[co][ci][t]  (the dgrad operand of the split-bf16 path: k = co contiguous)
__global__ void oihw_to_tap_t_kernel(const float* __restrict__ w, float* __restrict__ out, int cout, int cin, int taps) {
    const long long total = (long long)cout * cin * taps;
    for (long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(o % cout); long long r = o / cout;
        const int ci = (int)(r % cin); const int t = (int)(r / cin);
        out[o] = w[((long long)co * cin + ci) * taps + t];
    }
}
// batched 2-D transpose through a padded 32x32 LDS tile: dst[b][c][r] = src[b][r][c]
__global__ __launch_bounds__(256) void transpose2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
    __shared__ float tile[32][33];
    const long long boff = (long long)blockIdx.z * rows * cols;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[boff + (long long)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) dst[boff + (long long)c * rows + r] = tile[tx][i];
    }
}
// the same for 16-bit elements: a 64 x 64 tile (a wavefront reads / writes 128 contiguous bytes either way)
__global__ __launch_bounds__(256) void s16_transpose2d_kernel(const u16* __restrict__ src, u16* __restrict__ dst, int rows, int cols) {
    __shared__ u16 tile[64][66];
    const long long boff = (long long)blockIdx.z * rows * cols;
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[boff + (long long)r * cols + c] : (u16)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) dst[boff + (long long)c * rows + r] = tile[tx][i];
    }
}

// the same with strides: src[b][r][c] at src + b * bs_src + r * ld_src + c; dst[b][c][r] at dst + b * bs_dst + c * ld_dst + r for
// r < rows_pad, ZERO for rows <= r < rows_pad (a reduction dimension padded to the contraction kernels' K granule)
__global__ __launch_bounds__(256) void transpose2d_strided_kernel(const float* __restrict__ src, long long ld_src, long long bs_src,
                                                                  float* __restrict__ dst, long long ld_dst, long long bs_dst, int rows, int cols,
                                                                  int rows_pad) {
    __shared__ float tile[32][33];
    const float* sb = src + (long long)blockIdx.z * bs_src;
    float* db = dst + (long long)blockIdx.z * bs_dst;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? sb[(long long)r * ld_src + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows_pad) db[(long long)c * ld_dst + r] = tile[tx][i];
    }
}

// ... and for 16-bit elements (64 x 64 tiles): the g^T / x^T / dS^T operands of 'gaussian' under 16-bit storage (ops16.py)
__global__ __launch_bounds__(256) void s16_transpose2d_strided_kernel(const u16* __restrict__ src, long long ld_src, long long bs_src,
                                                                      u16* __restrict__ dst, long long ld_dst, long long bs_dst, int rows, int cols,
                                                                      int rows_pad) {
    __shared__ u16 tile[64][66];
    const u16* sb = src + (long long)blockIdx.z * bs_src;
    u16* db = dst + (long long)blockIdx.z * bs_dst;
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? sb[(long long)r * ld_src + c] : (u16)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows_pad) db[(long long)c * ld_dst + r] = tile[tx][i];
    }
}

// ---------------------------------------------------------------------------------------
// stem 7x7, Cin = 1.  One workgroup = 16x16 output pixels; the 22x22 input patch and the
// 49 x Cout weights sit in LDS; each thread owns one pixel x 16 output channels per pass.
// ---------------------------------------------------------------------------------------
constexpr int ST = 16, SP = ST + 6;
// 16-bit storage (glf_s16_stem7x7_*): the conv output / its gradient are bf16; arithmetic stays fp32
template <int COUT, bool OUT16>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       void* __restrict__ yv, int h, int wd, int ho, int wo, int pad) {
    __shared__ float patch[SP * SP];
    __shared__ __attribute__((aligned(16))) float wt[49 * COUT];       // [tap][co]
    __shared__ __attribute__((aligned(16))) float bs[COUT];
    const int tid = threadIdx.x;
    const int n = blockIdx.z, oy0 = blockIdx.y * ST, ox0 = blockIdx.x * ST;
    for (int i = tid; i < 49 * COUT; i += 256) { const int co = i / 49, t = i - co * 49; wt[t * COUT + co] = w[i]; }
    for (int i = tid; i < COUT; i += 256) bs[i] = bias ? bias[i] : 0.f;
    for (int i = tid; i < SP * SP; i += 256) {
        const int py = i / SP, px = i - py * SP;
        const int iy = oy0 - pad + py, ix = ox0 - pad + px;
        patch[i] = (iy >= 0 && iy < h && ix >= 0 && ix < wd) ? x[((long long)n * h + iy) * wd + ix] : 0.f;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    const int oy = oy0 + ty, ox = ox0 + tx;
    float xin[49];
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) xin[ky * 7 + kx] = patch[(ty + ky) * SP + tx + kx];
    if (oy >= ho || ox >= wo) return;
    float* dst = static_cast<float*>(yv) + (((long long)n * ho + oy) * wo + ox) * COUT;
    unsigned short* dst16 = static_cast<unsigned short*>(yv) + (((long long)n * ho + oy) * wo + ox) * COUT;
#pragma unroll 1
    for (int c0 = 0; c0 < COUT; c0 += 16) {
        float4 a0 = *reinterpret_cast<const float4*>(bs + c0), a1 = *reinterpret_cast<const float4*>(bs + c0 + 4);
        float4 a2 = *reinterpret_cast<const float4*>(bs + c0 + 8), a3 = *reinterpret_cast<const float4*>(bs + c0 + 12);
#pragma unroll
        for (int t = 0; t < 49; ++t) {
            const float v = xin[t];
            const float4 w0 = *reinterpret_cast<const float4*>(wt + t * COUT + c0);
            const float4 w1 = *reinterpret_cast<const float4*>(wt + t * COUT + c0 + 4);
            const float4 w2 = *reinterpret_cast<const float4*>(wt + t * COUT + c0 + 8);
            const float4 w3 = *reinterpret_cast<const float4*>(wt + t * COUT + c0 + 12);
            a0.x = fmaf(v, w0.x, a0.x); a0.y = fmaf(v, w0.y, a0.y); a0.z = fmaf(v, w0.z, a0.z); a0.w = fmaf(v, w0.w, a0.w);
            a1.x = fmaf(v, w1.x, a1.x); a1.y = fmaf(v, w1.y, a1.y); a1.z = fmaf(v, w1.z, a1.z); a1.w = fmaf(v, w1.w, a1.w);
            a2.x = fmaf(v, w2.x, a2.x); a2.y = fmaf(v, w2.y, a2.y); a2.z = fmaf(v, w2.z, a2.z); a2.w = fmaf(v, w2.w, a2.w);
            a3.x = fmaf(v, w3.x, a3.x); a3.y = fmaf(v, w3.y, a3.y); a3.z = fmaf(v, w3.z, a3.z); a3.w = fmaf(v, w3.w, a3.w);
        }
        if (OUT16) {
            *reinterpret_cast<uint4*>(dst16 + c0) = make_uint4(pack2(a0.x, a0.y), pack2(a0.z, a0.w), pack2(a1.x, a1.y), pack2(a1.z, a1.w));
            *reinterpret_cast<uint4*>(dst16 + c0 + 8) = make_uint4(pack2(a2.x, a2.y), pack2(a2.z, a2.w), pack2(a3.x, a3.y), pack2(a3.z, a3.w));
        } else {
            *reinterpret_cast<float4*>(dst + c0) = a0; *reinterpret_cast<float4*>(dst + c0 + 4) = a1;
            *reinterpret_cast<float4*>(dst + c0 + 8) = a2; *reinterpret_cast<float4*>(dst + c0 + 12) = a3;
        }
    }
}

// stem wgrad: dW[co][tap] = sum_pixels dy[p][co] * x[p + tap]; db[co] = sum dy.
// One workgroup = one 16x16 output tile of one image; thread = (co = tid & 63, tap group = tid >> 6).
// partial[block][50][64] (49 taps + bias row), folded by stem_wgrad_finalize.
constexpr int STEM_CO = 64;
template <bool DY16>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, const void* __restrict__ dyv, float* __restrict__ partial,
                                                         int h, int wd, int ho, int wo, int pad) {
    const float* __restrict__ dy = static_cast<const float*>(dyv);
    const unsigned short* __restrict__ dy16 = static_cast<const unsigned short*>(dyv);
    __shared__ float patch[SP * SP];
    const int tid = threadIdx.x;
    const int n = blockIdx.z, oy0 = blockIdx.y * ST, ox0 = blockIdx.x * ST;
    for (int i = tid; i < SP * SP; i += 256) {
        const int py = i / SP, px = i - py * SP;
        const int iy = oy0 - pad + py, ix = ox0 - pad + px;
        patch[i] = (iy >= 0 && iy < h && ix >= 0 && ix < wd) ? x[((long long)n * h + iy) * wd + ix] : 0.f;
    }
    __syncthreads();
    const int co = tid & 63, tg = tid >> 6;          // taps tg, tg+4, ... (13 for tg 0, 12 otherwise)
    float acc[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) acc[i] = 0.f;
    float accb = 0.f;
    const int ny = min(ST, ho - oy0), nx = min(ST, wo - ox0);
    for (int py = 0; py < ny; ++py)
        for (int px = 0; px < nx; ++px) {
            const long long go = (((long long)n * ho + oy0 + py) * wo + ox0 + px) * STEM_CO + co;
            const float g = DY16 ? __uint_as_float((unsigned)dy16[go] << 16) : dy[go];
            accb += g;
#pragma unroll
            for (int i = 0; i < 13; ++i) {
                const int t = tg + 4 * i;
                if (t < 49) { const int ky = t / 7, kx = t - ky * 7; acc[i] = fmaf(g, patch[(py + ky) * SP + px + kx], acc[i]); }
            }
        }
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    float* dst = partial + blk * 50 * STEM_CO;
#pragma unroll
    for (int i = 0; i < 13; ++i) { const int t = tg + 4 * i; if (t < 49) dst[t * STEM_CO + co] = acc[i]; }
    if (tg == 0) dst[49 * STEM_CO + co] = accb;
}
// one workgroup per tap row t (64 channels x 16 block-lanes, fixed summation order => bitwise reproducible)
__global__ __launch_bounds__(1024) void stem_wgrad_finalize(const float* __restrict__ partial, long long nblk, float* __restrict__ dw, float* __restrict__ db) {
    __shared__ double sh[16][STEM_CO];
    const int t = blockIdx.x, co = threadIdx.x & 63, ln = threadIdx.x >> 6;
    double s = 0;
    for (long long b = ln; b < nblk; b += 16) s += partial[(b * 50 + t) * STEM_CO + co];
    sh[ln][co] = s;
    __syncthreads();
    if (ln == 0) {
        for (int i = 1; i < 16; ++i) s += sh[i][co];
        if (t < 49) dw[co * 49 + t] = (float)s; else if (db) db[co] = (float)s;
    }
}
// stem dgrad (early_fusion: the stem's input is the learned mix of the views' images, ours.py:2299-2304):
// dx[n][iy][ix] = sum_taps sum_co dy[n][iy - ky + pad][ix - kx + pad][co] * w[co][ky][kx].  One workgroup = 16x16 input pixels, one
// pixel per thread; the weights sit in LDS as [tap][co] and are read at wavefront-uniform addresses (broadcast), the 64 gradients of
// a tap's pixel in 16-byte pieces (neighbouring threads share them through the cache).  Four partial sums, folded (a0 + a1) + (a2 + a3).
template <bool DY16>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const void* __restrict__ dyv, const float* __restrict__ w, float* __restrict__ dx,
                                                         int h, int wd, int ho, int wo, int pad) {
    const float* __restrict__ dy = static_cast<const float*>(dyv);
    const unsigned short* __restrict__ dy16 = static_cast<const unsigned short*>(dyv);
    __shared__ __attribute__((aligned(16))) float wt[49 * STEM_CO];    // [tap][co]
    const int tid = threadIdx.x;
    for (int i = tid; i < 49 * STEM_CO; i += 256) { const int co = i / 49, t = i - co * 49; wt[t * STEM_CO + co] = w[i]; }
    __syncthreads();
    const int n = blockIdx.z, iy = blockIdx.y * ST + (tid >> 4), ix = blockIdx.x * ST + (tid & 15);
    if (iy >= h || ix >= wd) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
        const int oy = iy - ky + pad;
        if (oy < 0 || oy >= ho) continue;
#pragma unroll 1
        for (int kx = 0; kx < 7; ++kx) {
            const int ox = ix - kx + pad;
            if (ox < 0 || ox >= wo) continue;
            const long long p = (((long long)n * ho + oy) * wo + ox) * STEM_CO;
            const float* wr = wt + (ky * 7 + kx) * STEM_CO;
#pragma unroll
            for (int c0 = 0; c0 < STEM_CO; c0 += 8) {
                const F8 g = DY16 ? ld8(dy16 + p + c0) : ldf8(dy + p + c0);
                const float4 w0 = *reinterpret_cast<const float4*>(wr + c0), w1 = *reinterpret_cast<const float4*>(wr + c0 + 4);
                a0 = fmaf(g.v[0], w0.x, a0); a1 = fmaf(g.v[1], w0.y, a1); a2 = fmaf(g.v[2], w0.z, a2); a3 = fmaf(g.v[3], w0.w, a3);
                a0 = fmaf(g.v[4], w1.x, a0); a1 = fmaf(g.v[5], w1.y, a1); a2 = fmaf(g.v[6], w1.z, a2); a3 = fmaf(g.v[7], w1.w, a3);
            }
        }
    }
    dx[((long long)n * h + iy) * wd + ix] = (a0 + a1) + (a2 + a3);
}

// ---------------------------------------------------------------------------------------
// maxpool 3x3 stride 2 pad 1
// ---------------------------------------------------------------------------------------
// W window indices (one byte each), stored and loaded in one W-byte access
template <int W> struct alignas(W) IdxPack { unsigned w[W / 4]; };

template <class T, int W>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx,
                                                          int n, int h, int w, int cw, int ho, int wo) {
    const long long total = (long long)n * ho * wo * cw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); long long p = i / cw;
        const int ox = (int)(p % wo); p /= wo;
        const int oy = (int)(p % ho); const int nn = (int)(p / ho);
        FV<W> best;
        unsigned bi[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { best.v[j] = -INFINITY; bi[j] = 0; }
        bool first = true;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
                if (iy < 0 || iy >= h || ix < 0 || ix >= w) continue;
                const FV<W> v = Stream<T, W>::ld(x + (((long long)nn * h + iy) * w + ix) * (cw * W) + cc * W);
                const unsigned t = ky * 3 + kx;
                // ATen: take the first in-range element, then strictly-greater (or NaN) replaces
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (first || v.v[j] > best.v[j] || v.v[j] != v.v[j]) { best.v[j] = v.v[j]; bi[j] = t; }
                first = false;
            }
        Stream<T, W>::st(y + i * W, best);
        IdxPack<W> pk;
#pragma unroll
        for (int q = 0; q < W / 4; ++q) pk.w[q] = bi[4 * q] | (bi[4 * q + 1] << 8) | (bi[4 * q + 2] << 16) | (bi[4 * q + 3] << 24);
        *reinterpret_cast<IdxPack<W>*>(idx + i * W) = pk;
    }
}
template <class T, int W>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx,
                                                          int n, int h, int w, int cw, int ho, int wo) {
    const long long total = (long long)n * h * w * cw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); long long p = i / cw;
        const int ix = (int)(p % w); p /= w;
        const int iy = (int)(p % h); const int nn = (int)(p / h);
        FV<W> g;
#pragma unroll
        for (int j = 0; j < W; ++j) g.v[j] = 0.f;
        // windows (oy,ox) that contain (iy,ix): iy = 2*oy - 1 + ky
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ny = iy + 1 - ky;
            if (ny < 0 || (ny & 1)) continue;
            const int oy = ny >> 1;
            if (oy >= ho) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int nx = ix + 1 - kx;
                if (nx < 0 || (nx & 1)) continue;
                const int ox = nx >> 1;
                if (ox >= wo) continue;
                const long long o = ((((long long)nn * ho + oy) * wo + ox) * cw + cc) * W;
                const IdxPack<W> t = *reinterpret_cast<const IdxPack<W>*>(idx + o);
                const FV<W> d = Stream<T, W>::ld(dy + o);
                const unsigned me = ky * 3 + kx;
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (((t.w[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) g.v[j] += d.v[j];
            }
        }
        Stream<T, W>::st(dx + i * W, g);
    }
}

// ---------------------------------------------------------------------------------------
// per-frame row sums / broadcasts (ASPP pooling branch)
// ---------------------------------------------------------------------------------------
// y[n][c] = scale * sum_p x[n][p][c]   (row stride ld)
__global__ __launch_bounds__(256) void sum_rows_kernel(const float* __restrict__ x, int ld, float* __restrict__ y, float scale, int p, int c) {
    __shared__ float sh[256];
    const int n = blockIdx.y;
    const int cpb = 64;                                   // channels per block
    const int c0 = blockIdx.x * cpb + (threadIdx.x & 63);
    const int pl = threadIdx.x >> 6;                      // 4 row lanes
    float s = 0.f;
    if (c0 < c)
        for (int r = pl; r < p; r += 4) s += x[((long long)n * p + r) * ld + c0];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (pl == 0 && c0 < c) y[(long long)n * c + c0] = scale * (sh[threadIdx.x] + sh[threadIdx.x + 64] + sh[threadIdx.x + 128] + sh[threadIdx.x + 192]);
}
// 16-byte form: 16 channel quads x 16 row lanes per workgroup, four rows' loads in flight per thread (the scalar form above walks
// 196 dependent 4-byte loads per thread: 2.4 TB/s on the ASPP pooled branch's 411 MB maps)
__global__ __launch_bounds__(256) void sum_rows4_kernel(const float* __restrict__ x, int ld, float* __restrict__ y, float scale, int p, int c4) {
    // sums in double: the ASPP pooled branch feeds these N per-frame averages to a BatchNorm over N samples, which amplifies their
    // rounding by |mean| / spread -- the kernel is memory-bound, the wider adds are free
    __shared__ double sh[4][256];
    const int n = blockIdx.y;
    const int cq = blockIdx.x * 16 + (threadIdx.x & 15);
    const int pl = threadIdx.x >> 4;                      // 16 row lanes
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (cq < c4) {
        const float* base = x + (long long)n * p * ld + 4 * cq;
        int r = pl;
        for (; r + 48 < p; r += 64) {
            const float4 a = *reinterpret_cast<const float4*>(base + (long long)r * ld);
            const float4 b = *reinterpret_cast<const float4*>(base + (long long)(r + 16) * ld);
            const float4 d = *reinterpret_cast<const float4*>(base + (long long)(r + 32) * ld);
            const float4 e = *reinterpret_cast<const float4*>(base + (long long)(r + 48) * ld);
            s0 += ((double)a.x + (double)b.x) + ((double)d.x + (double)e.x);
            s1 += ((double)a.y + (double)b.y) + ((double)d.y + (double)e.y);
            s2 += ((double)a.z + (double)b.z) + ((double)d.z + (double)e.z);
            s3 += ((double)a.w + (double)b.w) + ((double)d.w + (double)e.w);
        }
        for (; r < p; r += 16) {
            const float4 a = *reinterpret_cast<const float4*>(base + (long long)r * ld);
            s0 += a.x; s1 += a.y; s2 += a.z; s3 += a.w;
        }
    }
    sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1; sh[2][threadIdx.x] = s2; sh[3][threadIdx.x] = s3;
    __syncthreads();
    if (pl == 0 && cq < c4) {
#pragma unroll
        for (int q = 1; q < 16; ++q) { s0 += sh[0][q * 16 + threadIdx.x]; s1 += sh[1][q * 16 + threadIdx.x]; s2 += sh[2][q * 16 + threadIdx.x]; s3 += sh[3][q * 16 + threadIdx.x]; }
        const double sc = (double)scale;
        *reinterpret_cast<float4*>(y + (long long)n * 4 * c4 + 4 * cq) = make_float4((float)(sc * s0), (float)(sc * s1), (float)(sc * s2), (float)(sc * s3));
    }
}
// y[n][p][c] = scale * x[n][c]   (y row stride ld, storage T; x storage TX: the ASPP pooled branch stays fp32 up to this broadcast)
template <class T, class TX, int W>
__global__ __launch_bounds__(256) void bcast_rows_kernel(const TX* __restrict__ x, T* __restrict__ y, int ld, float scale, int p, int cw, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); const long long row = i / cw;
        const long long n = row / p;
        FV<W> v = Stream<TX, W>::ld(x + (n * cw + cc) * W);
#pragma unroll
        for (int j = 0; j < W; ++j) v.v[j] *= scale;
        Stream<T, W>::st(y + row * ld + cc * W, v);
    }
}

// y[row][:] += scale * x[row / p][:]: the accumulating form (fp32, C % 4 == 0) -- the gradient of a per-frame average (the ASPP
// pooled branch) added into the input gradient the conv branches already wrote, instead of a tensor of its own plus a sum pass
__global__ __launch_bounds__(256) void bcast_rows_add_kernel(const float* __restrict__ x, float* __restrict__ y, int ld, float scale, int p, int c4, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % c4); const long long row = i / c4;
        const float4 a = *reinterpret_cast<const float4*>(x + ((row / p) * c4 + cc) * 4);
        float4* dst = reinterpret_cast<float4*>(y + row * ld + cc * 4);
        float4 v = *dst;
        v.x = fmaf(scale, a.x, v.x); v.y = fmaf(scale, a.y, v.y); v.z = fmaf(scale, a.z, v.z); v.w = fmaf(scale, a.w, v.w);
        *dst = v;
    }
}

// ---------------------------------------------------------------------------------------
// dropout (counter-based; same mask recomputed in backward from the seed)
// ---------------------------------------------------------------------------------------
template <class T, int W>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, long long n, float p, float scale,
                                                      unsigned long long seed, const unsigned long long* __restrict__ step) {
    // `step`: a device counter the caller advances once per training step.  A launch recorded in a hipGraph replays with the
    // SAME `seed` argument every time; the counter is what gives every replay its own mask (forward and backward of one step
    // read the same value).  n counts accesses of W elements; the hash is taken per ELEMENT index.
    if (step) seed += *step * 0xD1B54A32D192ED03ull;
    const unsigned thr = (unsigned)(p * 16777216.0f);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        FV<W> v = Stream<T, W>::ld(x + i * W);
#pragma unroll
        for (int j = 0; j < W; ++j) v.v[j] = (mix64(seed * 0x100000001B3ull + (unsigned long long)(i * W + j)) >= thr) ? v.v[j] * scale : 0.f;
        Stream<T, W>::st(y + i * W, v);
    }
}

template <class T, int W>
__global__ __launch_bounds__(256) void relu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        FV<W> v = Stream<T, W>::ld(x + i * W);
#pragma unroll
        for (int j = 0; j < W; ++j) v.v[j] = fmaxf(v.v[j], 0.f);
        Stream<T, W>::st(y + i * W, v);
    }
}
template <class T, int W>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        FV<W> g = Stream<T, W>::ld(dy + i * W);
        const FV<W> v = Stream<T, W>::ld(y + i * W);
#pragma unroll
        for (int j = 0; j < W; ++j) g.v[j] = v.v[j] > 0.f ? g.v[j] : 0.f;
        Stream<T, W>::st(dx + i * W, g);
    }
}
// out = a * x + b * y: nw accesses of W elements, then the n - W * nw elements left over one by one
template <class T, int W>
__global__ __launch_bounds__(256) void axpby_kernel(const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out, float a, float b,
                                                    long long nw, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nw; i += (long long)gridDim.x * blockDim.x) {
        FV<W> u = Stream<T, W>::ld(x + i * W);
        const FV<W> v = Stream<T, W>::ld(y + i * W);
#pragma unroll
        for (int j = 0; j < W; ++j) u.v[j] = a * u.v[j] + b * v.v[j];
        Stream<T, W>::st(out + i * W, u);
    }
    for (long long i = W * nw + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        Stream<T, 1>::st(out + i, {{a * Stream<T, 1>::ld(x + i).v[0] + b * Stream<T, 1>::ld(y + i).v[0]}});
}

// ---------------------------------------------------------------------------------------
// local gate
// ---------------------------------------------------------------------------------------
// lane 0 of a gate-backward row: da = sum_c dy * f  ->  the gradients of the class and centre logits
__device__ __forceinline__ void gate_bwd_logits(float da, int lane, int row, float a, const float* __restrict__ cls, int ncls, const float* __restrict__ ctr,
                                                const int* __restrict__ amax, float weight, float* __restrict__ dcls, float* __restrict__ dctr) {
    if (lane != 0) return;
    const int bi = amax[row];
    const float m = sigmoidf_(cls[(long long)row * ncls + bi]);
    const float cc = sigmoidf_(ctr[row]);
    const float dt = da * a * (1.f - a) * weight;            // d/d(m*cc)
    for (int k = 0; k < ncls; ++k) dcls[(long long)row * ncls + k] = (k == bi) ? dt * cc * m * (1.f - m) : 0.f;
    dctr[row] = dt * m * cc * (1.f - cc);
}
template <class T, int W>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ cls, int ncls, const float* __restrict__ ctr,
                                                       const T* __restrict__ f, T* __restrict__ y, float* __restrict__ a_out,
                                                       int* __restrict__ amax, float weight, int rows, int c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    // max over classes of sigmoid(cls): scan order, strictly greater replaces (first maximum wins)
    float best = sigmoidf_(cls[(long long)row * ncls]);
    int bi = 0;
    for (int k = 1; k < ncls; ++k) { const float s = sigmoidf_(cls[(long long)row * ncls + k]); if (s > best) { best = s; bi = k; } }
    const float cc = sigmoidf_(ctr[row]);
    const float a = sigmoidf_(weight * best * cc);
    if (lane == 0) { a_out[row] = a; amax[row] = bi; }
    for (int i = lane; i < c / W; i += 64) {
        FV<W> v = Stream<T, W>::ld(f + (long long)row * c + i * W);
#pragma unroll
        for (int j = 0; j < W; ++j) v.v[j] *= a;
        Stream<T, W>::st(y + (long long)row * c + i * W, v);
    }
}
// The two storage forms of gate backward stay two kernels: the row dot product sum(dy * f) is summed pairwise-of-four per access in
// fp32 and sequentially in bf16, and both orders are kept bit for bit (one body would need a per-type branch in the arithmetic).
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ f, const float* __restrict__ cls, int ncls,
                                                       const float* __restrict__ ctr, const float* __restrict__ a_in, const int* __restrict__ amax,
                                                       float weight, float* __restrict__ df, float* __restrict__ dcls, float* __restrict__ dctr,
                                                       int rows, int c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float a = a_in[row];
    const float4* g4 = reinterpret_cast<const float4*>(dy + (long long)row * c);
    const float4* f4 = reinterpret_cast<const float4*>(f + (long long)row * c);
    float4* d4 = reinterpret_cast<float4*>(df + (long long)row * c);
    float s = 0.f;
    for (int i = lane; i < (c >> 2); i += 64) {
        const float4 g = g4[i], v = f4[i];
        s += (g.x * v.x + g.y * v.y) + (g.z * v.z + g.w * v.w);
        d4[i] = make_float4(g.x * a, g.y * a, g.z * a, g.w * a);
    }
    gate_bwd_logits(wave_sum(s), lane, row, a, cls, ncls, ctr, amax, weight, dcls, dctr);
}
__global__ __launch_bounds__(256) void s16_gate_bwd_kernel(const u16* __restrict__ dy, const u16* __restrict__ f, const float* __restrict__ cls, int ncls,
                                                           const float* __restrict__ ctr, const float* __restrict__ a_in, const int* __restrict__ amax,
                                                           float weight, u16* __restrict__ df, float* __restrict__ dcls, float* __restrict__ dctr,
                                                           int rows, int c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float a = a_in[row];
    float s = 0.f;
    for (int i = lane; i < (c >> 3); i += 64) {
        F8 g = ld8(dy + (long long)row * c + i * 8);
        const F8 v = ld8(f + (long long)row * c + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) { s += g.v[j] * v.v[j]; g.v[j] *= a; }
        st8(df + (long long)row * c + i * 8, g);
    }
    gate_bwd_logits(wave_sum(s), lane, row, a, cls, ncls, ctr, amax, weight, dcls, dctr);
}

// ---------------------------------------------------------------------------------------
// frame-strided copies / adds (frame strides and `inner` in elements)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void copy_frames_kernel(const float4* __restrict__ src, long long sfs, float4* __restrict__ dst, long long dfs,
                                                          long long inner4, long long total4) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / inner4, r = i - n * inner4;
        dst[n * dfs + r] = src[n * sfs + r];
    }
}
// the same copy that also writes the packed pre-split fp16 image of what it copies (scaled by *amax, an upper bound of the
// sources' maxima known BEFORE the copy): the stacked fusion-block input is read by contractions only through that image
__global__ __launch_bounds__(256) void copy_frames_split_kernel(const float4* __restrict__ src, long long sfs, float4* __restrict__ dst,
                                                                float4* __restrict__ dst_pk, long long dfs, long long inner4, long long total4,
                                                                const float* __restrict__ amax) {
    float sc, inv;
    pow2_scale(amax, sc, inv);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / inner4, r = i - n * inner4;
        const float4 v = src[n * sfs + r];
        dst[n * dfs + r] = v;
        const SplitH sp = split4h(v, sc);
        const float2 h = __builtin_bit_cast(float2, sp.h), l = __builtin_bit_cast(float2, sp.l);
        dst_pk[n * dfs + r] = make_float4(h.x, h.y, l.x, l.y);
    }
}
template <class T, int W>
__global__ __launch_bounds__(256) void add_frames_kernel(const T* __restrict__ a, long long afs, const T* __restrict__ b, long long bfs,
                                                         T* __restrict__ dst, long long dfs, long long innerw, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / innerw, r = i - n * innerw;
        FV<W> u = Stream<T, W>::ld(a + n * afs + r * W);
        const FV<W> v = Stream<T, W>::ld(b + n * bfs + r * W);
#pragma unroll
        for (int j = 0; j < W; ++j) u.v[j] += v.v[j];
        Stream<T, W>::st(dst + n * dfs + r * W, u);
    }
}

// n-ary sum (gradient fan-in of a tensor consumed by several branches): one pass, k reads + 1 write
template <class T> struct AddNPtrs { const T* p[8]; };
template <class T, int W>
__global__ __launch_bounds__(256) void add_n_kernel(AddNPtrs<T> in, int k, T* __restrict__ out, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        FV<W> a = Stream<T, W>::ld(in.p[0] + i * W);
        for (int j = 1; j < k; ++j) {
            const FV<W> b = Stream<T, W>::ld(in.p[j] + i * W);
#pragma unroll
            for (int e = 0; e < W; ++e) a.v[e] += b.v[e];
        }
        Stream<T, W>::st(out + i * W, a);
    }
}

// ---------------------------------------------------------------------------------------
// row softmax (embedded mode), one workgroup per row
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(v, o, 64); v = is_max ? fmaxf(v, t) : v + t; }
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[wv] = v;
    __syncthreads();
    float r = sh[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
    return r;
}
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* __restrict__ x, int cols, int ld) {
    __shared__ float sh[4];
    float* row = x + (long long)blockIdx.x * ld;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < cols; i += 256) m = fmaxf(m, row[i]);
    m = block_reduce(m, true, sh);
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) { const float e = expf(row[i] - m); row[i] = e; s += e; }
    s = block_reduce(s, false, sh);
    const float inv = 1.0f / s;
    for (int i = threadIdx.x; i < cols; i += 256) row[i] *= inv;
    for (int i = cols + threadIdx.x; i < ld; i += 256) row[i] = 0.f;          // padding columns of a row stride > cols read as zero probabilities
}
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float* __restrict__ p, float* __restrict__ dp, int cols, int ld) {
    __shared__ float sh[4];
    const float* pr = p + (long long)blockIdx.x * ld;
    float* dr = dp + (long long)blockIdx.x * ld;
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) s += pr[i] * dr[i];
    s = block_reduce(s, false, sh);
    for (int i = threadIdx.x; i < cols; i += 256) dr[i] = pr[i] * (dr[i] - s);
    for (int i = cols + threadIdx.x; i < ld; i += 256) dr[i] = 0.f;
}

// ---------------------------------------------------------------------------------------
// bilinear (align_corners = False), channels-last in -> NCHW out, and the adjoint
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void src_index(int o, float scale, int in_size, int& i0, int& i1, float& l1) {
    float s = ((float)o + 0.5f) * scale - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
}
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int h, int w, int c,
                                                           int ho, int wo, float sy, float sx) {
    const long long total = (long long)n * c * ho * wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(i % wo); long long t = i / wo;
        const int oy = (int)(t % ho); t /= ho;
        const int cc = (int)(t % c); const int nn = (int)(t / c);
        int y0, y1, x0, x1; float ly, lx;
        src_index(oy, sy, h, y0, y1, ly);
        src_index(ox, sx, w, x0, x1, lx);
        const float* b = x + (long long)nn * h * w * c + cc;
        const float v00 = b[((long long)y0 * w + x0) * c], v01 = b[((long long)y0 * w + x1) * c];
        const float v10 = b[((long long)y1 * w + x0) * c], v11 = b[((long long)y1 * w + x1) * c];
        y[i] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    }
}
// gather form of the adjoint: input pixel (iy,ix) collects from every output whose y0/y1 (x0/x1) hits it
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int n, int h, int w, int c,
                                                           int ho, int wo, float sy, float sx, int ry, int rx) {
    const long long total = (long long)n * h * w * c;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % c); long long t = i / c;
        const int ix = (int)(t % w); t /= w;
        const int iy = (int)(t % h); const int nn = (int)(t / h);
        const float* g = dy + ((long long)nn * c + cc) * ho * wo;
        // candidate outputs: o with src in (i-1, i+1)  =>  o in ((i-1+0.5)/scale - 0.5, (i+1+0.5)/scale - 0.5)
        const int oy_lo = max(0, (int)floorf(((float)iy - 0.5f) / sy - 0.5f) - 1), oy_hi = min(ho - 1, oy_lo + ry);
        const int ox_lo = max(0, (int)floorf(((float)ix - 0.5f) / sx - 0.5f) - 1), ox_hi = min(wo - 1, ox_lo + rx);
        float acc = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            int y0, y1; float ly;
            src_index(oy, sy, h, y0, y1, ly);
            float wy = 0.f;
            if (y0 == iy) wy += 1.f - ly;
            if (y1 == iy) wy += ly;
            if (wy == 0.f) continue;
            float rowacc = 0.f;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                int x0, x1; float lx;
                src_index(ox, sx, w, x0, x1, lx);
                float wx = 0.f;
                if (x0 == ix) wx += 1.f - lx;
                if (x1 == ix) wx += lx;
                if (wx != 0.f) rowacc += wx * g[(long long)oy * wo + ox];
            }
            acc += wy * rowacc;
        }
        dx[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------
// BCE-with-logits (sum) and overlap counts
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bce_kernel(const float* __restrict__ x, const float* __restrict__ t, double* __restrict__ loss,
                                                  float* __restrict__ dx, float gscale, const float* __restrict__ gsd, long long n) {
    __shared__ double sh[4];
    double acc = 0;
    if (gsd) gscale *= *gsd;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float xv = x[i], tv = t[i];
        // max(x,0) - x*t + log1p(exp(-|x|))  (the stable form ATen uses)
        acc += (double)(fmaxf(xv, 0.f) - xv * tv + log1pf(expf(-fabsf(xv))));
        if (dx) dx[i] = (sigmoidf_(xv) - tv) * gscale;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, sh[0] + sh[1] + sh[2] + sh[3]);
}
__global__ __launch_bounds__(256) void overlap_kernel(const float* __restrict__ x, const float* __restrict__ t, unsigned long long* __restrict__ counts, long long n) {
    unsigned long long tp = 0, fp = 0, fn = 0, tn = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const bool pr = sigmoidf_(x[i]) > 0.5f;        // main.py:250,385
        const bool gt = t[i] != 0.f;
        tp += pr && gt; fp += pr && !gt; fn += !pr && gt; tn += !pr && !gt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tp += __shfl_xor(tp, o, 64); fp += __shfl_xor(fp, o, 64); fn += __shfl_xor(fn, o, 64); tn += __shfl_xor(tn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { atomicAdd(counts + 0, tp); atomicAdd(counts + 1, fp); atomicAdd(counts + 2, fn); atomicAdd(counts + 3, tn); }
}

// Cross pseudo supervision of two logit maps: each one's hard prediction (overlap_kernel's predicate) is the other's BCE target.
// One pass reads a and b once and yields the loss sum of both directions, the agreement counts and (BWD) both gradients.
struct CpsAcc { double loss; unsigned long long n11, n10, n01, n00; };
__device__ __forceinline__ float bce_term(float xv, float tv) { return fmaxf(xv, 0.f) - xv * tv + log1pf(expf(-fabsf(xv))); }
template <bool BWD>
__device__ __forceinline__ void cps_pair(float av, float bv, float g, CpsAcc& acc, float& dav, float& dbv) {
    const float sa = sigmoidf_(av), sb = sigmoidf_(bv);
    const bool pa = sa > 0.5f, pb = sb > 0.5f;                    // the labels: constants, no gradient through the threshold
    const float ta = pa ? 1.f : 0.f, tb = pb ? 1.f : 0.f;
    acc.loss += (double)bce_term(av, tb);
    acc.loss += (double)bce_term(bv, ta);
    acc.n11 += pa && pb; acc.n10 += pa && !pb; acc.n01 += !pa && pb; acc.n00 += !pa && !pb;
    if (BWD) { dav = (sa - tb) * g; dbv = (sb - ta) * g; }
}
// nv accesses of four elements (every base on 16 bytes, else nv = 0), then the n - 4 nv elements left over one by one
template <bool BWD>
__global__ __launch_bounds__(256) void cps_bce_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ loss,
                                                      unsigned long long* __restrict__ stats, float* __restrict__ da, float* __restrict__ db,
                                                      float gscale, const float* __restrict__ gsd, long long nv, long long n) {
    __shared__ double sh[4];
    __shared__ unsigned long long shn[4][4];
    CpsAcc acc = {0, 0, 0, 0, 0};
    if (BWD && gsd) gscale *= *gsd;
    const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < nv; i += nthr) {
        const float4 av = *reinterpret_cast<const float4*>(a + 4 * i), bv = *reinterpret_cast<const float4*>(b + 4 * i);
        float4 ga, gb;
        cps_pair<BWD>(av.x, bv.x, gscale, acc, ga.x, gb.x); cps_pair<BWD>(av.y, bv.y, gscale, acc, ga.y, gb.y);
        cps_pair<BWD>(av.z, bv.z, gscale, acc, ga.z, gb.z); cps_pair<BWD>(av.w, bv.w, gscale, acc, ga.w, gb.w);
        if (BWD) { *reinterpret_cast<float4*>(da + 4 * i) = ga; *reinterpret_cast<float4*>(db + 4 * i) = gb; }
    }
    for (long long i = 4 * nv + tid; i < n; i += nthr) {
        float ga, gb;
        cps_pair<BWD>(a[i], b[i], gscale, acc, ga, gb);
        if (BWD) { da[i] = ga; db[i] = gb; }
    }
    const double l = wave_sum_d(acc.loss);
    const int wv = threadIdx.x >> 6;
    if (stats) {                                               // (uniform over the grid)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            acc.n11 += __shfl_xor(acc.n11, o, 64); acc.n10 += __shfl_xor(acc.n10, o, 64);
            acc.n01 += __shfl_xor(acc.n01, o, 64); acc.n00 += __shfl_xor(acc.n00, o, 64);
        }
        if ((threadIdx.x & 63) == 0) { shn[wv][0] = acc.n11; shn[wv][1] = acc.n10; shn[wv][2] = acc.n01; shn[wv][3] = acc.n00; }
    }
    if ((threadIdx.x & 63) == 0) sh[wv] = l;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, sh[0] + sh[1] + sh[2] + sh[3]);
    // one int64 atomic per WORKGROUP and counter: the four counters share a cache line, and with one atomic per wave (overlap_kernel's
    // form: 32 768 of them at 2.5 M elements) the counting forward took 0.41 ms where the backward, which counts nothing, takes 0.04
    if (stats && threadIdx.x < 4) atomicAdd(stats + threadIdx.x, shn[0][threadIdx.x] + shn[1][threadIdx.x] + shn[2][threadIdx.x] + shn[3][threadIdx.x]);
}

// ---------------------------------------------------------------------------------------
// one launcher per streaming op; the extern "C" entry points of both families check their arguments and call these
// ---------------------------------------------------------------------------------------
template <class T, int W>
int launch_maxpool_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, hipStream_t s, const char* what) {
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    const long long total = (long long)n * ho * wo * (c / W);
    hipLaunchKernelGGL((maxpool_fwd_kernel<T, W>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y), idx,
                       n, h, w, c / W, ho, wo);
    return glf::check_launch(what);
}
template <class T, int W>
int launch_maxpool_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, hipStream_t s, const char* what) {
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    const long long total = (long long)n * h * w * (c / W);
    hipLaunchKernelGGL((maxpool_bwd_kernel<T, W>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<const T*>(dy), idx, static_cast<T*>(dx),
                       n, h, w, c / W, ho, wo);
    return glf::check_launch(what);
}
template <class T, class TX, int W>
int launch_bcast_rows(const void* x, void* y, int ldy, float scale, int n, int p, int c, hipStream_t s, const char* what) {
    const long long total = (long long)n * p * (c / W);
    hipLaunchKernelGGL((bcast_rows_kernel<T, TX, W>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<const TX*>(x), static_cast<T*>(y), ldy,
                       scale, p, c / W, total);
    return glf::check_launch(what);
}
template <class T, int W>
int launch_dropout(const void* x, void* y, int64_t numel, float p, uint64_t seed, const uint64_t* step_counter, hipStream_t s, const char* what) {
    hipLaunchKernelGGL((dropout_kernel<T, W>), dim3(stream_grid(numel / W, 256)), dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y),
                       (long long)(numel / W), p, 1.0f / (1.0f - p), (unsigned long long)seed, reinterpret_cast<const unsigned long long*>(step_counter));
    return glf::check_launch(what);
}
template <class T, int W>
int launch_relu(const void* dy, const void* y, void* out, int64_t numel, hipStream_t s, const char* what) {       // dy == NULL: forward of y
    const dim3 grid(stream_grid(numel / W, 256));
    if (dy) hipLaunchKernelGGL((relu_bwd_kernel<T, W>), grid, dim3(256), 0, s, static_cast<const T*>(dy), static_cast<const T*>(y), static_cast<T*>(out), (long long)(numel / W));
    else hipLaunchKernelGGL((relu_fwd_kernel<T, W>), grid, dim3(256), 0, s, static_cast<const T*>(y), static_cast<T*>(out), (long long)(numel / W));
    return glf::check_launch(what);
}
template <class T, int W>
int launch_gate_fwd(const float* cls, int ncls, const float* ctr, const void* f, void* y, float* a, int32_t* argmax, float weight, int rows, int c,
                    hipStream_t s, const char* what) {
    hipLaunchKernelGGL((gate_fwd_kernel<T, W>), dim3((rows + 3) / 4), dim3(256), 0, s, cls, ncls, ctr, static_cast<const T*>(f), static_cast<T*>(y), a, argmax,
                       weight, rows, c);
    return glf::check_launch(what);
}
template <class T, int W>
int launch_add_frames(const void* a, int64_t a_fs, const void* b, int64_t b_fs, void* dst, int64_t dst_fs, int n, int64_t inner, hipStream_t s, const char* what) {
    const long long total = (long long)n * (inner / W);
    hipLaunchKernelGGL((add_frames_kernel<T, W>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<const T*>(a), (long long)a_fs,
                       static_cast<const T*>(b), (long long)b_fs, static_cast<T*>(dst), (long long)dst_fs, (long long)(inner / W), total);
    return glf::check_launch(what);
}
template <class T, int W>
int launch_add_n(const void* const* inputs, int k, void* out, int64_t numel, hipStream_t s, const char* what) {
    AddNPtrs<T> in;
    for (int j = 0; j < 8; ++j) in.p[j] = static_cast<const T*>(inputs[j < k ? j : 0]);
    hipLaunchKernelGGL((add_n_kernel<T, W>), dim3(stream_grid(numel / W, 256)), dim3(256), 0, s, in, k, static_cast<T*>(out), (long long)(numel / W));
    return glf::check_launch(what);
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" int glf_oihw_to_tap_major(const float* w, float* out, int cout, int cin, int taps, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(w && out, GLF_ERR_NULL, "oihw_to_tap_major: null argument");
    GLF_REQUIRE(cout > 0 && cin > 0 && taps > 0, GLF_ERR_BAD_SHAPE, "oihw_to_tap_major: bad shape");
    const long long cc = (long long)cout * cin;
    hipLaunchKernelGGL(oihw_to_tap_kernel, dim3(stream_grid(cc * taps, 256)), dim3(256), 0, glf::S(s), w, out, cc, taps);
    return glf::check_launch("oihw_to_tap_major");
}
extern "C" int glf_tap_major_to_oihw(const float* w, float* out, int cout, int cin, int taps, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(w && out, GLF_ERR_NULL, "tap_major_to_oihw: null argument");
    GLF_REQUIRE(cout > 0 && cin > 0 && taps > 0, GLF_ERR_BAD_SHAPE, "tap_major_to_oihw: bad shape");
    const long long cc = (long long)cout * cin;
    hipLaunchKernelGGL(tap_to_oihw_kernel, dim3(stream_grid(cc * taps, 256)), dim3(256), 0, glf::S(s), w, out, cc, taps);
    return glf::check_launch("tap_major_to_oihw");
}

extern "C" int glf_oihw_to_tap_major_t(const float* w, float* out, int cout, int cin, int taps, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(w && out, GLF_ERR_NULL, "oihw_to_tap_major_t: null argument");
    GLF_REQUIRE(cout > 0 && cin > 0 && taps > 0, GLF_ERR_BAD_SHAPE, "oihw_to_tap_major_t: bad shape");
    hipLaunchKernelGGL(oihw_to_tap_t_kernel, dim3(stream_grid((long long)cout * cin * taps, 256)), dim3(256), 0, glf::S(s), w, out, cout, cin, taps);
    return glf::check_launch("oihw_to_tap_major_t");
}
extern "C" int glf_transpose2d(const float* src, float* dst, int rows, int cols, int batch, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(src && dst, GLF_ERR_NULL, "transpose2d: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && batch > 0 && batch <= 65535 && (rows + 31) / 32 <= 65535, GLF_ERR_BAD_SHAPE, "transpose2d: bad shape");
    hipLaunchKernelGGL(transpose2d_kernel, dim3((cols + 31) / 32, (rows + 31) / 32, batch), dim3(256), 0, glf::S(s), src, dst, rows, cols);
    return glf::check_launch("transpose2d");
}
extern "C" int glf_s16_transpose2d(const void* src, void* dst, int rows, int cols, int batch, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(src && dst, GLF_ERR_NULL, "s16_transpose2d: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && batch > 0 && batch <= 65535, GLF_ERR_BAD_SHAPE, "s16_transpose2d: bad extents");
    hipLaunchKernelGGL(s16_transpose2d_kernel, dim3((cols + 63) / 64, (rows + 63) / 64, batch), dim3(256), 0, glf::S(s), static_cast<const u16*>(src),
                       static_cast<u16*>(dst), rows, cols);
    return glf::check_launch("s16_transpose2d");
}

extern "C" int glf_transpose2d_strided(const float* src, int64_t ld_src, int64_t batch_stride_src, float* dst, int64_t ld_dst,
                                       int64_t batch_stride_dst, int rows, int cols, int rows_pad, int batch, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(src && dst, GLF_ERR_NULL, "transpose2d_strided: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && batch > 0 && batch <= 65535 && rows_pad >= rows && (rows_pad + 31) / 32 <= 65535 && ld_src >= cols &&
                ld_dst >= rows_pad, GLF_ERR_BAD_SHAPE, "transpose2d_strided: bad shape");
    hipLaunchKernelGGL(transpose2d_strided_kernel, dim3((cols + 31) / 32, (rows_pad + 31) / 32, batch), dim3(256), 0, glf::S(s), src, (long long)ld_src,
                       (long long)batch_stride_src, dst, (long long)ld_dst, (long long)batch_stride_dst, rows, cols, rows_pad);
    return glf::check_launch("transpose2d_strided");
}

extern "C" int glf_s16_transpose2d_strided(const void* src, int64_t ld_src, int64_t batch_stride_src, void* dst, int64_t ld_dst,
                                           int64_t batch_stride_dst, int rows, int cols, int rows_pad, int batch, glf_stream_t s) {
    GLF_REQUIRE(src && dst, GLF_ERR_NULL, "s16_transpose2d_strided: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && batch > 0 && batch <= 65535 && rows_pad >= rows && (rows_pad + 63) / 64 <= 65535 && ld_src >= cols &&
                ld_dst >= rows_pad, GLF_ERR_BAD_SHAPE, "s16_transpose2d_strided: bad shape");
    if (int rc = glf::ensure_init()) return rc;
    hipLaunchKernelGGL(s16_transpose2d_strided_kernel, dim3((cols + 63) / 64, (rows_pad + 63) / 64, batch), dim3(256), 0, glf::S(s),
                       static_cast<const u16*>(src), (long long)ld_src, (long long)batch_stride_src, static_cast<u16*>(dst), (long long)ld_dst,
                       (long long)batch_stride_dst, rows, cols, rows_pad);
    return glf::check_launch("s16_transpose2d_strided");
}

extern "C" int glf_stem7x7_fwd(const float* x, const float* w, const float* bias, float* y,
                               int n, int h, int wdt, int cout, int pad, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && w && y, GLF_ERR_NULL, "stem7x7_fwd: null argument");
    GLF_REQUIRE(cout == STEM_CO, GLF_ERR_UNSUPPORTED, "stem7x7: Cout must be 64 (got %d)", cout);
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6;
    GLF_REQUIRE(n > 0 && n <= 65535 && ho > 0 && wo > 0 && pad >= 0 && pad <= 3, GLF_ERR_BAD_SHAPE, "stem7x7_fwd: bad shape");
    GLF_REQUIRE(al16(y), GLF_ERR_BAD_SHAPE, "stem7x7_fwd: y must be 16-byte aligned");
    dim3 grid((wo + ST - 1) / ST, (ho + ST - 1) / ST, n);
    hipLaunchKernelGGL((stem_fwd_kernel<STEM_CO, false>), grid, dim3(256), 0, glf::S(s), x, w, bias, y, h, wdt, ho, wo, pad);
    return glf::check_launch("stem7x7_fwd");
}
extern "C" int glf_s16_stem7x7_fwd(const float* x, const float* w, const float* bias, void* y,
                                   int n, int h, int wdt, int cout, int pad, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && w && y, GLF_ERR_NULL, "s16_stem7x7_fwd: null argument");
    GLF_REQUIRE(cout == STEM_CO, GLF_ERR_UNSUPPORTED, "stem7x7: Cout must be 64 (got %d)", cout);
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6;
    GLF_REQUIRE(n > 0 && n <= 65535 && ho > 0 && wo > 0 && pad >= 0 && pad <= 3, GLF_ERR_BAD_SHAPE, "s16_stem7x7_fwd: bad shape");
    GLF_REQUIRE(al16(y), GLF_ERR_BAD_SHAPE, "s16_stem7x7_fwd: y must be 16-byte aligned");
    dim3 grid((wo + ST - 1) / ST, (ho + ST - 1) / ST, n);
    hipLaunchKernelGGL((stem_fwd_kernel<STEM_CO, true>), grid, dim3(256), 0, glf::S(s), x, w, bias, y, h, wdt, ho, wo, pad);
    return glf::check_launch("s16_stem7x7_fwd");
}
// Inference-mode stem in ONE kernel: conv7x7 (Cin = 1) + bias -> BatchNorm (given mean / invstd: the running statistics) -> ReLU ->
// max-pool 3x3 stride 2 pad 1.  One workgroup = a 16 x 16 tile of conv outputs starting one row / column before an even
// coordinate = the 3x3 windows of 7 x 7 pooled outputs (15 of its 16 rows / columns are used).  The conv tile is evaluated like
// stem_fwd_kernel's (same patch, same tap order: bit-identical values), 16 channels at a time, normalised, parked in LDS and
// pooled from there: the [N][Ho][Wo][64] conv output and its normalised copy never reach memory (2 x 3 MB per 112 x 112 frame).
constexpr int SPOOL = 7;                   // pooled outputs per tile edge
__global__ __launch_bounds__(256) void stem_bn_relu_pool_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float* __restrict__ y, int h, int wd, int ho, int wo, int hp, int wp, int pad,
                                                                 float* __restrict__ amax_out) {
    __shared__ float patch[SP * SP];
    __shared__ __attribute__((aligned(16))) float wt[49 * STEM_CO];       // [tap][co]
    __shared__ __attribute__((aligned(16))) float coef[5 * STEM_CO];      // bias, mean, invstd, gamma, beta
    constexpr int TP = ST * ST + 1;                                       // pixel stride of a channel row (odd: no bank conflicts)
    __shared__ float tile[16 * TP];                                       // [16 channels][conv pixel], normalised + ReLU
    const int tid = threadIdx.x;
    const int n = blockIdx.z, py0 = blockIdx.y * SPOOL, px0 = blockIdx.x * SPOOL;
    const int oy0 = 2 * py0 - 1, ox0 = 2 * px0 - 1;                       // first conv row / column of the tile (may be -1)
    for (int i = tid; i < 49 * STEM_CO; i += 256) { const int co = i / 49, t = i - co * 49; wt[t * STEM_CO + co] = w[i]; }
    for (int i = tid; i < STEM_CO; i += 256) {
        coef[i] = bias ? bias[i] : 0.f; coef[STEM_CO + i] = mean[i]; coef[2 * STEM_CO + i] = invstd[i];
        coef[3 * STEM_CO + i] = gamma[i]; coef[4 * STEM_CO + i] = beta[i];
    }
    for (int i = tid; i < SP * SP; i += 256) {
        const int qy = i / SP, qx = i - qy * SP;
        const int iy = oy0 - pad + qy, ix = ox0 - pad + qx;
        patch[i] = (iy >= 0 && iy < h && ix >= 0 && ix < wd) ? x[((long long)n * h + iy) * wd + ix] : 0.f;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    float xin[49];
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) xin[ky * 7 + kx] = patch[(ty + ky) * SP + tx + kx];
    // pooling role of this thread: pooled pixel (tid >> 2) of the 7 x 7 (threads 0 .. 195), channels 4 (tid & 3) .. of the group
    const int pp = tid >> 2, pc = (tid & 3) * 4;
    const int ppy = pp / SPOOL, ppx = pp - ppy * SPOOL;
    const bool pool_ok = pp < SPOOL * SPOOL && py0 + ppy < hp && px0 + ppx < wp;
    float am = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < STEM_CO; c0 += 16) {
        float4 a0 = *reinterpret_cast<const float4*>(coef + c0), a1 = *reinterpret_cast<const float4*>(coef + c0 + 4);
        float4 a2 = *reinterpret_cast<const float4*>(coef + c0 + 8), a3 = *reinterpret_cast<const float4*>(coef + c0 + 12);
#pragma unroll
        for (int t = 0; t < 49; ++t) {
            const float v = xin[t];
            const float4 w0 = *reinterpret_cast<const float4*>(wt + t * STEM_CO + c0);
            const float4 w1 = *reinterpret_cast<const float4*>(wt + t * STEM_CO + c0 + 4);
            const float4 w2 = *reinterpret_cast<const float4*>(wt + t * STEM_CO + c0 + 8);
            const float4 w3 = *reinterpret_cast<const float4*>(wt + t * STEM_CO + c0 + 12);
            a0.x = fmaf(v, w0.x, a0.x); a0.y = fmaf(v, w0.y, a0.y); a0.z = fmaf(v, w0.z, a0.z); a0.w = fmaf(v, w0.w, a0.w);
            a1.x = fmaf(v, w1.x, a1.x); a1.y = fmaf(v, w1.y, a1.y); a1.z = fmaf(v, w1.z, a1.z); a1.w = fmaf(v, w1.w, a1.w);
            a2.x = fmaf(v, w2.x, a2.x); a2.y = fmaf(v, w2.y, a2.y); a2.z = fmaf(v, w2.z, a2.z); a2.w = fmaf(v, w2.w, a2.w);
            a3.x = fmaf(v, w3.x, a3.x); a3.y = fmaf(v, w3.y, a3.y); a3.z = fmaf(v, w3.z, a3.z); a3.w = fmaf(v, w3.w, a3.w);
        }
        // (x - mean) * invstd * gamma + beta, the expression of glf_bn_apply.  Tile positions outside the conv output hold a finite
        // value of no meaning: the pooling loop below skips them by coordinate (selecting here, per element, drove the register
        // allocator to 1.4 KB of scratch per lane)
        auto park = [&](const float4& a, int cb) {
            const float4 mu = *reinterpret_cast<const float4*>(coef + STEM_CO + c0 + cb), is = *reinterpret_cast<const float4*>(coef + 2 * STEM_CO + c0 + cb);
            const float4 ga = *reinterpret_cast<const float4*>(coef + 3 * STEM_CO + c0 + cb), be = *reinterpret_cast<const float4*>(coef + 4 * STEM_CO + c0 + cb);
            const float v0 = (a.x - mu.x) * is.x * ga.x + be.x, v1 = (a.y - mu.y) * is.y * ga.y + be.y;
            const float v2 = (a.z - mu.z) * is.z * ga.z + be.z, v3 = (a.w - mu.w) * is.w * ga.w + be.w;
            tile[(cb + 0) * TP + tid] = fmaxf(v0, 0.f); tile[(cb + 1) * TP + tid] = fmaxf(v1, 0.f);
            tile[(cb + 2) * TP + tid] = fmaxf(v2, 0.f); tile[(cb + 3) * TP + tid] = fmaxf(v3, 0.f);
        };
        park(a0, 0); park(a1, 4); park(a2, 8); park(a3, 12);
        __syncthreads();
        if (pool_ok) {
            float m[4] = {-1.f, -1.f, -1.f, -1.f};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int pix = (2 * ppy + dy) * ST + 2 * ppx + dx;
                    const int cy = oy0 + 2 * ppy + dy, cx = ox0 + 2 * ppx + dx;
                    const bool in = cy >= 0 && cy < ho && cx >= 0 && cx < wo;       // the window hangs over the conv output at the borders
#pragma unroll
                    for (int k = 0; k < 4; ++k) m[k] = in ? fmaxf(m[k], tile[(pc + k) * TP + pix]) : m[k];
                }
            *reinterpret_cast<float4*>(y + (((long long)n * hp + py0 + ppy) * wp + px0 + ppx) * STEM_CO + c0 + pc) = make_float4(m[0], m[1], m[2], m[3]);
            am = fmaxf(fmaxf(am, fmaxf(m[0], m[1])), fmaxf(m[2], m[3]));
        }
        __syncthreads();
    }
    if (amax_out) block_amax(am, amax_out);
}

extern "C" int glf_stem7x7_bn_relu_pool(const float* x, const float* w, const float* bias, const float* mean, const float* invstd,
                                        const float* gamma, const float* beta, float* y, int n, int h, int wdt, int cout, int pad,
                                        float* amax_out, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && w && mean && invstd && gamma && beta && y, GLF_ERR_NULL, "stem7x7_bn_relu_pool: null argument");
    GLF_REQUIRE(cout == STEM_CO, GLF_ERR_UNSUPPORTED, "stem7x7: Cout must be 64 (got %d)", cout);
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6;
    GLF_REQUIRE(n > 0 && n <= 65535 && ho > 0 && wo > 0 && pad >= 0 && pad <= 3, GLF_ERR_BAD_SHAPE, "stem7x7_bn_relu_pool: bad shape");
    const int hp = (ho - 1) / 2 + 1, wp = (wo - 1) / 2 + 1;             // MaxPool2d(3, stride 2, padding 1)
    GLF_REQUIRE(al16(y), GLF_ERR_BAD_SHAPE, "stem7x7_bn_relu_pool: y must be 16-byte aligned");
    dim3 grid((wp + SPOOL - 1) / SPOOL, (hp + SPOOL - 1) / SPOOL, n);
    hipLaunchKernelGGL(stem_bn_relu_pool_kernel, grid, dim3(256), 0, glf::S(s), x, w, bias, mean, invstd, gamma, beta, y, h, wdt, ho, wo, hp, wp, pad, amax_out);
    return glf::check_launch("stem7x7_bn_relu_pool");
}
extern "C" size_t glf_stem7x7_wgrad_workspace(int n, int h, int wdt, int cout, int pad) {
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6;
    if (n <= 0 || ho <= 0 || wo <= 0) return 0;
    return (size_t)n * ((ho + ST - 1) / ST) * ((wo + ST - 1) / ST) * 50 * (size_t)cout;
}
extern "C" int glf_stem7x7_wgrad(const float* x, const float* dy, float* dw, float* db, float* partial,
                                 int n, int h, int wdt, int cout, int pad, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && dy && dw && partial, GLF_ERR_NULL, "stem7x7_wgrad: null argument");
    GLF_REQUIRE(cout == STEM_CO, GLF_ERR_UNSUPPORTED, "stem7x7: Cout must be 64 (got %d)", cout);
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6;
    GLF_REQUIRE(n > 0 && n <= 65535 && ho > 0 && wo > 0 && pad >= 0 && pad <= 3, GLF_ERR_BAD_SHAPE, "stem7x7_wgrad: bad shape");
    dim3 grid((wo + ST - 1) / ST, (ho + ST - 1) / ST, n);
    hipLaunchKernelGGL(stem_wgrad_kernel<false>, grid, dim3(256), 0, glf::S(s), x, dy, partial, h, wdt, ho, wo, pad);
    if (int rc = glf::check_launch("stem7x7_wgrad")) return rc;
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    hipLaunchKernelGGL(stem_wgrad_finalize, dim3(50), dim3(1024), 0, glf::S(s), partial, nblk, dw, db);
    return glf::check_launch("stem7x7_wgrad_finalize");
}
extern "C" int glf_s16_stem7x7_wgrad(const float* x, const void* dy, float* dw, float* db, float* partial,
                                     int n, int h, int wdt, int cout, int pad, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && dy && dw && partial, GLF_ERR_NULL, "s16_stem7x7_wgrad: null argument");
    GLF_REQUIRE(cout == STEM_CO, GLF_ERR_UNSUPPORTED, "stem7x7: Cout must be 64 (got %d)", cout);
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6;
    GLF_REQUIRE(n > 0 && n <= 65535 && ho > 0 && wo > 0 && pad >= 0 && pad <= 3, GLF_ERR_BAD_SHAPE, "s16_stem7x7_wgrad: bad shape");
    dim3 grid((wo + ST - 1) / ST, (ho + ST - 1) / ST, n);
    hipLaunchKernelGGL(stem_wgrad_kernel<true>, grid, dim3(256), 0, glf::S(s), x, dy, partial, h, wdt, ho, wo, pad);
    if (int rc = glf::check_launch("s16_stem7x7_wgrad")) return rc;
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    hipLaunchKernelGGL(stem_wgrad_finalize, dim3(50), dim3(1024), 0, glf::S(s), partial, nblk, dw, db);
    return glf::check_launch("s16_stem7x7_wgrad_finalize");
}
#define REQ_STEM_DGRAD(what) \
    GLF_REQUIRE(dy && w && dx, GLF_ERR_NULL, what ": null argument"); \
    GLF_REQUIRE(cout == STEM_CO, GLF_ERR_UNSUPPORTED, "stem7x7: Cout must be 64 (got %d)", cout); \
    const int ho = h + 2 * pad - 6, wo = wdt + 2 * pad - 6; \
    GLF_REQUIRE(n > 0 && n <= 65535 && ho > 0 && wo > 0 && pad >= 0 && pad <= 3, GLF_ERR_BAD_SHAPE, what ": bad shape"); \
    GLF_REQUIRE(al16(dy), GLF_ERR_BAD_SHAPE, what ": dy must be 16-byte aligned"); \
    dim3 grid((wdt + ST - 1) / ST, (h + ST - 1) / ST, n)
extern "C" int glf_stem7x7_dgrad(const float* dy, const float* w, float* dx, int n, int h, int wdt, int cout, int pad, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_STEM_DGRAD("stem7x7_dgrad");
    hipLaunchKernelGGL(stem_dgrad_kernel<false>, grid, dim3(256), 0, glf::S(s), dy, w, dx, h, wdt, ho, wo, pad);
    return glf::check_launch("stem7x7_dgrad");
}
extern "C" int glf_s16_stem7x7_dgrad(const void* dy, const float* w, float* dx, int n, int h, int wdt, int cout, int pad, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_STEM_DGRAD("s16_stem7x7_dgrad");
    hipLaunchKernelGGL(stem_dgrad_kernel<true>, grid, dim3(256), 0, glf::S(s), dy, w, dx, h, wdt, ho, wo, pad);
    return glf::check_launch("s16_stem7x7_dgrad");
}

extern "C" int glf_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && idx, GLF_ERR_NULL, "maxpool_fwd: null argument");
    GLF_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && (c % 4) == 0, GLF_ERR_BAD_SHAPE, "maxpool_fwd: bad shape (C %% 4 == 0 required)");
    GLF_REQUIRE(al16(x) && al16(y) && ((reinterpret_cast<uintptr_t>(idx) & 3u) == 0), GLF_ERR_BAD_SHAPE, "maxpool_fwd: alignment");
    return launch_maxpool_fwd<float, 4>(x, y, idx, n, h, w, c, glf::S(s), "maxpool_fwd");
}
extern "C" int glf_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && idx && dx, GLF_ERR_NULL, "maxpool_bwd: null argument");
    GLF_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && (c % 4) == 0, GLF_ERR_BAD_SHAPE, "maxpool_bwd: bad shape (C %% 4 == 0 required)");
    GLF_REQUIRE(al16(dy) && al16(dx) && ((reinterpret_cast<uintptr_t>(idx) & 3u) == 0), GLF_ERR_BAD_SHAPE, "maxpool_bwd: alignment");
    return launch_maxpool_bwd<float, 4>(dy, idx, dx, n, h, w, c, glf::S(s), "maxpool_bwd");
}
extern "C" int glf_s16_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && idx, GLF_ERR_NULL, "s16_maxpool_fwd: null argument");
    GLF_REQUIRE(n > 0 && h > 0 && w > 0, GLF_ERR_BAD_SHAPE, "s16_maxpool_fwd: bad extents");
    REQ_C8(c); REQ_AL(x, "x"); REQ_AL(y, "y");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(idx) & 7u) == 0, GLF_ERR_BAD_SHAPE, "s16_maxpool_fwd: idx must be 8-byte aligned");
    return launch_maxpool_fwd<u16, 8>(x, y, idx, n, h, w, c, glf::S(s), "s16_maxpool_fwd");
}
extern "C" int glf_s16_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && dx && idx, GLF_ERR_NULL, "s16_maxpool_bwd: null argument");
    GLF_REQUIRE(n > 0 && h > 0 && w > 0, GLF_ERR_BAD_SHAPE, "s16_maxpool_bwd: bad extents");
    REQ_C8(c); REQ_AL(dy, "dy"); REQ_AL(dx, "dx");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(idx) & 7u) == 0, GLF_ERR_BAD_SHAPE, "s16_maxpool_bwd: idx must be 8-byte aligned");
    return launch_maxpool_bwd<u16, 8>(dy, idx, dx, n, h, w, c, glf::S(s), "s16_maxpool_bwd");
}

extern "C" int glf_sum_rows_fwd(const float* dy, int lddy, float* dx, float scale, int n, int p, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && dx, GLF_ERR_NULL, "sum_rows: null argument");
    GLF_REQUIRE(n > 0 && n <= 65535 && p > 0 && c > 0 && lddy >= c, GLF_ERR_BAD_SHAPE, "sum_rows: bad shape");
    if (c % 4 == 0 && lddy % 4 == 0 && al16(dy) && al16(dx))
        hipLaunchKernelGGL(sum_rows4_kernel, dim3((c / 4 + 15) / 16, n), dim3(256), 0, glf::S(s), dy, lddy, dx, scale, p, c / 4);
    else
        hipLaunchKernelGGL(sum_rows_kernel, dim3((c + 63) / 64, n), dim3(256), 0, glf::S(s), dy, lddy, dx, scale, p, c);
    return glf::check_launch("sum_rows");
}
extern "C" int glf_avgpool_fwd(const float* x, float* y, int n, int p, int c, glf_stream_t s) {
    return glf_sum_rows_fwd(x, c, y, p > 0 ? 1.0f / (float)p : 0.f, n, p, c, s);
}
extern "C" int glf_bcast_rows_scaled(const float* x, float* y, int ldy, float scale, int n, int p, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "bcast_rows: null argument");
    GLF_REQUIRE(n > 0 && p > 0 && c > 0 && ldy >= c, GLF_ERR_BAD_SHAPE, "bcast_rows: bad shape");
    if (c % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y)) return launch_bcast_rows<float, float, 4>(x, y, ldy, scale, n, p, c, glf::S(s), "bcast_rows");
    return launch_bcast_rows<float, float, 1>(x, y, ldy, scale, n, p, c, glf::S(s), "bcast_rows");
}
extern "C" int glf_bcast_rows_add(const float* x, float* y, int ldy, float scale, int n, int p, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "bcast_rows_add: null argument");
    GLF_REQUIRE(n > 0 && p > 0 && c > 0 && ldy >= c, GLF_ERR_BAD_SHAPE, "bcast_rows_add: bad shape");
    GLF_REQUIRE(c % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y), GLF_ERR_UNSUPPORTED, "bcast_rows_add: c and ldy must be multiples of 4 and both tensors 16-byte aligned");
    const long long total = (long long)n * p * (c / 4);
    hipLaunchKernelGGL(bcast_rows_add_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, glf::S(s), x, y, ldy, scale, p, c / 4, total);
    return glf::check_launch("bcast_rows_add");
}
extern "C" int glf_s16_bcast_rows(const void* x, int x_dtype, void* y, int ldy, float scale, int n, int p, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "s16_bcast_rows: null argument");
    GLF_REQUIRE(n > 0 && p > 0, GLF_ERR_BAD_SHAPE, "s16_bcast_rows: bad extents");
    REQ_C8(c); REQ_AL(x, "x"); REQ_AL(y, "y"); REQ_LD8(ldy, "ldy");
    GLF_REQUIRE(x_dtype == GLF_DT_F32 || x_dtype == GLF_DT_BF16, GLF_ERR_UNSUPPORTED, "s16_bcast_rows: x_dtype must be GLF_DT_F32 or GLF_DT_BF16");
    if (x_dtype == GLF_DT_F32) return launch_bcast_rows<u16, float, 8>(x, y, ldy, scale, n, p, c, glf::S(s), "s16_bcast_rows");
    return launch_bcast_rows<u16, u16, 8>(x, y, ldy, scale, n, p, c, glf::S(s), "s16_bcast_rows");
}
extern "C" int glf_bcast_rows_fwd(const float* x, float* y, int ldy, int n, int p, int c, glf_stream_t s) {
    return glf_bcast_rows_scaled(x, y, ldy, 1.0f, n, p, c, s);
}

extern "C" int glf_dropout(const float* x, float* y, int64_t numel, float p, uint64_t seed, const uint64_t* step_counter, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "dropout: null argument");
    GLF_REQUIRE(numel > 0 && p >= 0.f && p < 1.f, GLF_ERR_BAD_SHAPE, "dropout: numel > 0 and 0 <= p < 1 required");
    return launch_dropout<float, 1>(x, y, numel, p, seed, step_counter, glf::S(s), "dropout");
}
extern "C" int glf_s16_dropout(const void* x, void* y, int64_t numel, float p, uint64_t seed, const uint64_t* step_counter, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "s16_dropout: null argument");
    GLF_REQUIRE(numel > 0 && numel % 8 == 0 && p >= 0.f && p < 1.f, GLF_ERR_BAD_SHAPE, "s16_dropout: numel must be a positive multiple of 8, 0 <= p < 1");
    REQ_AL(x, "x"); REQ_AL(y, "y");
    return launch_dropout<u16, 8>(x, y, numel, p, seed, step_counter, glf::S(s), "s16_dropout");
}
__global__ void amax_combine_kernel(const float* a, const float* b, float scale, int sum, float* out) {
    const float va = fabsf(*a), vb = b ? fabsf(*b) : 0.f;
    const float v = scale * (sum ? va + vb : fmaxf(va, vb));
    if (v > *out) *out = v;
}
extern "C" int glf_amax_combine(const float* a, const float* b, float scale, int sum, float* out, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(a && out, GLF_ERR_NULL, "amax_combine: null argument");
    GLF_REQUIRE(scale >= 0.f, GLF_ERR_BAD_SHAPE, "amax_combine: scale must be >= 0");
    hipLaunchKernelGGL(amax_combine_kernel, dim3(1), dim3(1), 0, glf::S(s), a, b, scale, sum, out);
    return glf::check_launch("amax_combine");
}
__global__ void counter_add_kernel(unsigned long long* c, unsigned long long inc) { *c += inc; }
extern "C" int glf_counter_add(uint64_t* counter, uint64_t inc, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(counter, GLF_ERR_NULL, "counter_add: null argument");
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, glf::S(s), reinterpret_cast<unsigned long long*>(counter), (unsigned long long)inc);
    return glf::check_launch("counter_add");
}

extern "C" int glf_relu_fwd(const float* x, float* y, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "relu_fwd: null argument");
    GLF_REQUIRE(numel > 0, GLF_ERR_BAD_SHAPE, "relu_fwd: numel must be > 0");
    return launch_relu<float, 1>(nullptr, x, y, numel, glf::S(s), "relu_fwd");
}
extern "C" int glf_relu_bwd(const float* dy, const float* y, float* dx, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && y && dx, GLF_ERR_NULL, "relu_bwd: null argument");
    GLF_REQUIRE(numel > 0, GLF_ERR_BAD_SHAPE, "relu_bwd: numel must be > 0");
    return launch_relu<float, 1>(dy, y, dx, numel, glf::S(s), "relu_bwd");
}
extern "C" int glf_s16_relu_fwd(const void* x, void* y, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "s16_relu_fwd: null argument");
    GLF_REQUIRE(numel > 0 && numel % 8 == 0, GLF_ERR_BAD_SHAPE, "s16_relu_fwd: numel must be a positive multiple of 8");
    REQ_AL(x, "x"); REQ_AL(y, "y");
    return launch_relu<u16, 8>(nullptr, x, y, numel, glf::S(s), "s16_relu_fwd");
}
extern "C" int glf_s16_relu_bwd(const void* dy, const void* y, void* dx, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && y && dx, GLF_ERR_NULL, "s16_relu_bwd: null argument");
    GLF_REQUIRE(numel > 0 && numel % 8 == 0, GLF_ERR_BAD_SHAPE, "s16_relu_bwd: numel must be a positive multiple of 8");
    REQ_AL(dy, "dy"); REQ_AL(y, "y"); REQ_AL(dx, "dx");
    return launch_relu<u16, 8>(dy, y, dx, numel, glf::S(s), "s16_relu_bwd");
}

// fp32: a float4 body when all three pointers are 16-byte aligned, single elements for the rest (or for everything)
extern "C" int glf_axpby(const float* x, const float* y, float* out, float a, float b, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && out, GLF_ERR_NULL, "axpby: null argument");
    GLF_REQUIRE(numel > 0, GLF_ERR_BAD_SHAPE, "axpby: numel must be > 0");
    const long long n4 = (al16(x) && al16(y) && al16(out)) ? numel / 4 : 0;
    long long blocks = (numel / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
    hipLaunchKernelGGL((axpby_kernel<float, 4>), dim3((unsigned)blocks), dim3(256), 0, glf::S(s), x, y, out, a, b, n4, (long long)numel);
    return glf::check_launch("axpby");
}
extern "C" int glf_s16_axpby(const void* x, const void* y, void* out, float a, float b, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y && out, GLF_ERR_NULL, "s16_axpby: null argument");
    GLF_REQUIRE(numel > 0 && numel % 8 == 0, GLF_ERR_BAD_SHAPE, "s16_axpby: numel must be a positive multiple of 8");
    REQ_AL(x, "x"); REQ_AL(y, "y"); REQ_AL(out, "out");
    hipLaunchKernelGGL((axpby_kernel<u16, 8>), dim3(stream_grid(numel / 8, 256)), dim3(256), 0, glf::S(s), static_cast<const u16*>(x), static_cast<const u16*>(y),
                       static_cast<u16*>(out), a, b, (long long)(numel / 8), (long long)numel);
    return glf::check_launch("s16_axpby");
}

extern "C" int glf_gate_fwd(const float* cls, int ncls, const float* ctr, const float* f, float* y, float* a,
                            int32_t* argmax, float weight, int rows, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(cls && ctr && f && y && a && argmax, GLF_ERR_NULL, "gate_fwd: null argument");
    GLF_REQUIRE(rows > 0 && ncls > 0 && c > 0 && (c % 4) == 0, GLF_ERR_BAD_SHAPE, "gate_fwd: bad shape (C %% 4 == 0 required)");
    GLF_REQUIRE(al16(f) && al16(y), GLF_ERR_BAD_SHAPE, "gate_fwd: alignment");
    return launch_gate_fwd<float, 4>(cls, ncls, ctr, f, y, a, argmax, weight, rows, c, glf::S(s), "gate_fwd");
}
extern "C" int glf_s16_gate_fwd(const float* cls, int ncls, const float* ctr, const void* f, void* y, float* a, int32_t* argmax, float weight,
                                int rows, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(cls && ctr && f && y && a && argmax, GLF_ERR_NULL, "s16_gate_fwd: null argument");
    GLF_REQUIRE(rows > 0 && ncls > 0, GLF_ERR_BAD_SHAPE, "s16_gate_fwd: bad extents");
    REQ_C8(c); REQ_AL(f, "f"); REQ_AL(y, "y");
    return launch_gate_fwd<u16, 8>(cls, ncls, ctr, f, y, a, argmax, weight, rows, c, glf::S(s), "s16_gate_fwd");
}
extern "C" int glf_gate_bwd(const float* dy, const float* f, const float* cls, int ncls, const float* ctr,
                            const float* a, const int32_t* argmax, float weight,
                            float* df, float* dcls, float* dctr, int rows, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && f && cls && ctr && a && argmax && df && dcls && dctr, GLF_ERR_NULL, "gate_bwd: null argument");
    GLF_REQUIRE(rows > 0 && ncls > 0 && c > 0 && (c % 4) == 0, GLF_ERR_BAD_SHAPE, "gate_bwd: bad shape (C %% 4 == 0 required)");
    GLF_REQUIRE(al16(dy) && al16(f) && al16(df), GLF_ERR_BAD_SHAPE, "gate_bwd: alignment");
    hipLaunchKernelGGL(gate_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, glf::S(s), dy, f, cls, ncls, ctr, a, argmax, weight, df, dcls, dctr, rows, c);
    return glf::check_launch("gate_bwd");
}
extern "C" int glf_s16_gate_bwd(const void* dy, const void* f, const float* cls, int ncls, const float* ctr, const float* a, const int32_t* argmax,
                                float weight, void* df, float* dcls, float* dctr, int rows, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && f && cls && ctr && a && argmax && df && dcls && dctr, GLF_ERR_NULL, "s16_gate_bwd: null argument");
    GLF_REQUIRE(rows > 0 && ncls > 0, GLF_ERR_BAD_SHAPE, "s16_gate_bwd: bad extents");
    REQ_C8(c); REQ_AL(dy, "dy"); REQ_AL(f, "f"); REQ_AL(df, "df");
    hipLaunchKernelGGL(s16_gate_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, glf::S(s), static_cast<const u16*>(dy), static_cast<const u16*>(f), cls, ncls,
                       ctr, a, argmax, weight, static_cast<u16*>(df), dcls, dctr, rows, c);
    return glf::check_launch("s16_gate_bwd");
}

extern "C" int glf_copy_frames(const float* src, int64_t src_fs, float* dst, int64_t dst_fs, int n, int64_t inner, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(src && dst, GLF_ERR_NULL, "copy_frames: null argument");
    GLF_REQUIRE(n > 0 && inner > 0 && (inner % 4) == 0 && (src_fs % 4) == 0 && (dst_fs % 4) == 0, GLF_ERR_BAD_SHAPE,
                "copy_frames: sizes and strides must be positive multiples of 4");
    GLF_REQUIRE(al16(src) && al16(dst), GLF_ERR_BAD_SHAPE, "copy_frames: alignment");
    const long long total4 = (long long)n * (inner / 4);
    hipLaunchKernelGGL(copy_frames_kernel, dim3(stream_grid(total4, 256)), dim3(256), 0, glf::S(s), reinterpret_cast<const float4*>(src),
                       (long long)(src_fs / 4), reinterpret_cast<float4*>(dst), (long long)(dst_fs / 4), (long long)(inner / 4), total4);
    return glf::check_launch("copy_frames");
}
extern "C" int glf_copy_frames_split(const float* src, int64_t src_fs, float* dst, float* dst_packed, int64_t dst_fs, int n, int64_t inner,
                                     const float* amax, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(src && dst && dst_packed && amax, GLF_ERR_NULL, "copy_frames_split: null argument");
    GLF_REQUIRE(n > 0 && inner > 0 && (inner % 4) == 0 && (src_fs % 4) == 0 && (dst_fs % 4) == 0, GLF_ERR_BAD_SHAPE,
                "copy_frames_split: sizes and strides must be positive multiples of 4");
    GLF_REQUIRE(al16(src) && al16(dst) && al16(dst_packed), GLF_ERR_BAD_SHAPE, "copy_frames_split: alignment");
    const long long total4 = (long long)n * (inner / 4);
    hipLaunchKernelGGL(copy_frames_split_kernel, dim3(stream_grid(total4, 256)), dim3(256), 0, glf::S(s), reinterpret_cast<const float4*>(src),
                       (long long)(src_fs / 4), reinterpret_cast<float4*>(dst), reinterpret_cast<float4*>(dst_packed), (long long)(dst_fs / 4),
                       (long long)(inner / 4), total4, amax);
    return glf::check_launch("copy_frames_split");
}
extern "C" int glf_add_frames(const float* a, int64_t a_fs, const float* b, int64_t b_fs, float* dst, int64_t dst_fs,
                              int n, int64_t inner, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(a && b && dst, GLF_ERR_NULL, "add_frames: null argument");
    GLF_REQUIRE(n > 0 && inner > 0 && (inner % 4) == 0 && (a_fs % 4) == 0 && (b_fs % 4) == 0 && (dst_fs % 4) == 0, GLF_ERR_BAD_SHAPE,
                "add_frames: sizes and strides must be positive multiples of 4");
    GLF_REQUIRE(al16(a) && al16(b) && al16(dst), GLF_ERR_BAD_SHAPE, "add_frames: alignment");
    return launch_add_frames<float, 4>(a, a_fs, b, b_fs, dst, dst_fs, n, inner, glf::S(s), "add_frames");
}
extern "C" int glf_s16_add_frames(const void* a, int64_t a_fs, const void* b, int64_t b_fs, void* dst, int64_t dst_fs, int n, int64_t inner,
                                  glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(a && b && dst, GLF_ERR_NULL, "s16_add_frames: null argument");
    GLF_REQUIRE(n > 0 && inner > 0 && inner % 8 == 0 && a_fs % 8 == 0 && b_fs % 8 == 0 && dst_fs % 8 == 0, GLF_ERR_BAD_SHAPE,
                "s16_add_frames: inner and the frame strides must be multiples of 8");
    REQ_AL(a, "a"); REQ_AL(b, "b"); REQ_AL(dst, "dst");
    return launch_add_frames<u16, 8>(a, a_fs, b, b_fs, dst, dst_fs, n, inner, glf::S(s), "s16_add_frames");
}

extern "C" int glf_add_n(const float* const* inputs, int k, float* out, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(inputs && out, GLF_ERR_NULL, "add_n: null argument");
    GLF_REQUIRE(k >= 1 && k <= 8 && numel > 0 && (numel % 4) == 0, GLF_ERR_BAD_SHAPE, "add_n: 1 <= k <= 8 and numel %% 4 == 0 required");
    for (int j = 0; j < k; ++j) GLF_REQUIRE(inputs[j] != nullptr && al16(inputs[j]), GLF_ERR_BAD_SHAPE, "add_n: inputs must be non-null and 16-byte aligned");
    GLF_REQUIRE(al16(out), GLF_ERR_BAD_SHAPE, "add_n: out must be 16-byte aligned");
    return launch_add_n<float, 4>(reinterpret_cast<const void* const*>(inputs), k, out, numel, glf::S(s), "add_n");
}
extern "C" int glf_s16_add_n(const void* const* inputs, int k, void* out, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(inputs && out, GLF_ERR_NULL, "s16_add_n: null argument");
    GLF_REQUIRE(k >= 1 && k <= 8 && numel > 0 && numel % 8 == 0, GLF_ERR_BAD_SHAPE, "s16_add_n: 1 <= k <= 8, numel a positive multiple of 8");
    for (int i = 0; i < k; ++i) { GLF_REQUIRE(inputs[i], GLF_ERR_NULL, "s16_add_n: null input"); REQ_AL(inputs[i], "input"); }
    REQ_AL(out, "out");
    return launch_add_n<u16, 8>(inputs, k, out, numel, glf::S(s), "s16_add_n");
}

extern "C" int glf_softmax_rows(float* x, int64_t rows, int cols, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x, GLF_ERR_NULL, "softmax_rows: null argument");
    GLF_REQUIRE(rows > 0 && rows < 2147483647LL && cols > 0, GLF_ERR_BAD_SHAPE, "softmax_rows: bad shape");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, glf::S(s), x, cols, cols);
    return glf::check_launch("softmax_rows");
}
extern "C" int glf_softmax_rows_ld(float* x, int64_t rows, int cols, int ld, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x, GLF_ERR_NULL, "softmax_rows_ld: null argument");
    GLF_REQUIRE(rows > 0 && rows < 2147483647LL && cols > 0 && ld >= cols, GLF_ERR_BAD_SHAPE, "softmax_rows_ld: bad shape");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, glf::S(s), x, cols, ld);
    return glf::check_launch("softmax_rows_ld");
}
extern "C" int glf_softmax_rows_bwd_ld(const float* p, float* dp_inout, int64_t rows, int cols, int ld, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(p && dp_inout, GLF_ERR_NULL, "softmax_rows_bwd_ld: null argument");
    GLF_REQUIRE(rows > 0 && rows < 2147483647LL && cols > 0 && ld >= cols, GLF_ERR_BAD_SHAPE, "softmax_rows_bwd_ld: bad shape");
    hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, glf::S(s), p, dp_inout, cols, ld);
    return glf::check_launch("softmax_rows_bwd_ld");
}
extern "C" int glf_softmax_rows_bwd(const float* p, float* dp_inout, int64_t rows, int cols, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(p && dp_inout, GLF_ERR_NULL, "softmax_rows_bwd: null argument");
    GLF_REQUIRE(rows > 0 && rows < 2147483647LL && cols > 0, GLF_ERR_BAD_SHAPE, "softmax_rows_bwd: bad shape");
    hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, glf::S(s), p, dp_inout, cols, cols);
    return glf::check_launch("softmax_rows_bwd");
}

extern "C" int glf_bilinear_up_fwd(const float* x, float* y, int n, int h, int w, int c, int ho, int wo, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && y, GLF_ERR_NULL, "bilinear_up_fwd: null argument");
    GLF_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && ho > 0 && wo > 0, GLF_ERR_BAD_SHAPE, "bilinear_up_fwd: bad shape");
    const long long total = (long long)n * c * ho * wo;
    hipLaunchKernelGGL(bilinear_fwd_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, glf::S(s), x, y, n, h, w, c, ho, wo,
                       (float)h / (float)ho, (float)w / (float)wo);
    return glf::check_launch("bilinear_up_fwd");
}
extern "C" int glf_bilinear_up_bwd(const float* dy, float* dx, int n, int h, int w, int c, int ho, int wo, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dy && dx, GLF_ERR_NULL, "bilinear_up_bwd: null argument");
    GLF_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && ho >= h && wo >= w, GLF_ERR_BAD_SHAPE, "bilinear_up_bwd: up-sampling only (ho >= h, wo >= w)");
    const long long total = (long long)n * h * w * c;
    // an input pixel is touched by outputs within 2/scale (+ margin) of its centre
    const int ry = (int)(2.0f * (float)ho / (float)h) + 4, rx = (int)(2.0f * (float)wo / (float)w) + 4;
    hipLaunchKernelGGL(bilinear_bwd_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, glf::S(s), dy, dx, n, h, w, c, ho, wo,
                       (float)h / (float)ho, (float)w / (float)wo, ry, rx);
    return glf::check_launch("bilinear_up_bwd");
}

extern "C" int glf_bce_logits_sum(const float* x, const float* t, double* loss_out, float* dx, float grad_scale,
                                  const float* grad_scale_dev, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && t && loss_out, GLF_ERR_NULL, "bce_logits_sum: null argument");
    GLF_REQUIRE(numel > 0, GLF_ERR_BAD_SHAPE, "bce_logits_sum: numel must be > 0");
    hipError_t e = hipMemsetAsync(loss_out, 0, sizeof(double), glf::S(s));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "bce_logits_sum: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(bce_kernel, dim3(stream_grid(numel, 256)), dim3(256), 0, glf::S(s), x, t, loss_out, dx, grad_scale, grad_scale_dev, (long long)numel);
    return glf::check_launch("bce_logits_sum");
}
extern "C" int glf_overlap_counts(const float* logits, const float* target, int64_t* counts, int64_t numel, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(logits && target && counts, GLF_ERR_NULL, "overlap_counts: null argument");
    GLF_REQUIRE(numel > 0, GLF_ERR_BAD_SHAPE, "overlap_counts: numel must be > 0");
    hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), glf::S(s));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "overlap_counts: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(overlap_kernel, dim3(stream_grid(numel, 256)), dim3(256), 0, glf::S(s), logits, target,
                       reinterpret_cast<unsigned long long*>(counts), (long long)numel);
    return glf::check_launch("overlap_counts");
}
extern "C" int glf_cps_bce_sum(const float* a, const float* b, double* loss_out, int64_t* stats, float* da, float* db, float grad_scale,
                               const float* grad_scale_dev, int64_t numel, glf_stream_t s) {
    // every argument check comes before the first HIP call: the refusals need no device
    GLF_REQUIRE(a && b && loss_out && (da != nullptr) == (db != nullptr), GLF_ERR_NULL, "cps_bce_sum: null argument");
    GLF_REQUIRE(numel > 0, GLF_ERR_BAD_SHAPE, "cps_bce_sum: numel must be > 0");
    GLF_REQUIRE(!da || (da != a && db != b && da != db && da != b && db != a), GLF_ERR_BAD_SHAPE, "cps_bce_sum: outputs must not alias");
    if (int rc = glf::ensure_init()) return rc;
    hipError_t e = hipMemsetAsync(loss_out, 0, sizeof(double), glf::S(s));
    if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), glf::S(s));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "cps_bce_sum: memset: %s", hipGetErrorString(e));
    // 16-byte accesses when every base allows them; the scalar loop takes the whole array otherwise, and the tail either way
    const bool vec = glf::al16(a) && glf::al16(b) && (!da || (glf::al16(da) && glf::al16(db)));
    const long long nv = vec ? numel / 4 : 0;
    const dim3 grid(stream_grid(nv ? nv : numel, 256));
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    if (da)
        hipLaunchKernelGGL(cps_bce_kernel<true>, grid, dim3(256), 0, glf::S(s), a, b, loss_out, st, da, db, grad_scale, grad_scale_dev, nv, (long long)numel);
    else
        hipLaunchKernelGGL(cps_bce_kernel<false>, grid, dim3(256), 0, glf::S(s), a, b, loss_out, st, da, db, grad_scale, grad_scale_dev, nv, (long long)numel);
    return glf::check_launch("cps_bce_sum");
}

// The streaming pieces a U-Net needs beside the contractions (gfx950): the 3x3 entry convolution with ONE input channel, the 2x2
// stride-2 max-pool, nearest x2 up-sampling and the two-source channel concatenation (ours.py:2385-2625).  Channels-last, 16-byte
// accesses, fp32 arithmetic; ONE kernel body per operation for fp32 and bf16 storage through Stream<T, W> (stream_common.h), bf16
// rounded once at the store.  No float atomics: the one reduction here (the entry convolution's weight gradient) is per-workgroup
// partials in a caller-provided workspace plus a fixed-order finalize, as glf_stem7x7_wgrad does it.
#include "stream_common.h"

using namespace glf;

namespace {

// ---------------------------------------------------------------------------------------
// Conv2d(1, 64, 3, stride 1, padding 1) + bias.  Siblings of the stem's kernels rather than a generalisation of them: the 7x7 stem
// is compute-heavy enough (49 taps) to want a 16x16 pixel tile with the input patch in LDS and one pixel x 16 channels per thread;
// with 9 taps the op is a pure store stream (256 bytes written per 4 read), so it is a grid-stride pass like the other streaming ops.
// ---------------------------------------------------------------------------------------
constexpr int C1_CO = 64;
constexpr int C1_PIX = 1024;            // pixels one workgroup reduces in wgrad
constexpr int C1_ROWS = 10;             // 9 taps + the bias row

template <class T, int W>
__global__ __launch_bounds__(256) void conv3x3_c1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             T* __restrict__ y, long long npix, int h, int wd) {
    __shared__ __attribute__((aligned(16))) float wt[9 * C1_CO];       // [tap][co]
    __shared__ __attribute__((aligned(16))) float bs[C1_CO];
    for (int i = threadIdx.x; i < 9 * C1_CO; i += 256) { const int co = i / 9, t = i - co * 9; wt[t * C1_CO + co] = w[i]; }
    for (int i = threadIdx.x; i < C1_CO; i += 256) bs[i] = bias ? bias[i] : 0.f;
    __syncthreads();
    constexpr int CW = C1_CO / W;
    const long long total = npix * CW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % CW); const long long p = i / CW;
        const int ix = (int)(p % wd); const int iy = (int)((p / wd) % h);
        FV<W> acc;
#pragma unroll
        for (int j = 0; j < W; ++j) acc.v[j] = bs[cc * W + j];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = iy + ky - 1, xx = ix + kx - 1;
                const float v = (yy >= 0 && yy < h && xx >= 0 && xx < wd) ? x[p + (long long)(ky - 1) * wd + (kx - 1)] : 0.f;
                const float* wr = wt + (ky * 3 + kx) * C1_CO + cc * W;
#pragma unroll
                for (int j = 0; j < W; ++j) acc.v[j] = fmaf(v, wr[j], acc.v[j]);
            }
        Stream<T, W>::st(y + i * W, acc);
    }
}

// dW[co][tap] = sum_p dy[p][co] * x[p + tap], db[co] = sum_p dy[p][co].  One workgroup = C1_PIX consecutive pixels of the flat
// [N*H*W] map; thread = (one 16-byte group of W channels, pixel lane): 16 groups x 16 lanes (fp32), 8 x 32 (bf16), so a wavefront
// reads the 64 gradients of 4 (8) pixels in 16-byte pieces.  The lanes of a wavefront are folded by shuffles, the four wavefronts
// through LDS, in a fixed order.  partial[block][10][64], folded by conv3x3_c1_wgrad_finalize.
template <class T, int W>
__global__ __launch_bounds__(256) void conv3x3_c1_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ dy, float* __restrict__ partial,
                                                               long long npix, int h, int wd) {
    constexpr int CW = C1_CO / W, LANES = 256 / CW;
    __shared__ float sh[4][C1_ROWS * C1_CO];
    const int cg = threadIdx.x % CW, ln = threadIdx.x / CW;
    const long long p0 = (long long)blockIdx.x * C1_PIX;
    const int cnt = (int)(npix - p0 < C1_PIX ? npix - p0 : C1_PIX);
    float acc[C1_ROWS][W];
#pragma unroll
    for (int t = 0; t < C1_ROWS; ++t)
#pragma unroll
        for (int j = 0; j < W; ++j) acc[t][j] = 0.f;
    for (int k = ln; k < cnt; k += LANES) {
        const long long p = p0 + k;
        const int ix = (int)(p % wd); const int iy = (int)((p / wd) % h);
        const FV<W> g = Stream<T, W>::ld(dy + p * C1_CO + cg * W);
        float xv[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = iy + ky - 1, xx = ix + kx - 1;
                xv[ky * 3 + kx] = (yy >= 0 && yy < h && xx >= 0 && xx < wd) ? x[p + (long long)(ky - 1) * wd + (kx - 1)] : 0.f;
            }
#pragma unroll
        for (int j = 0; j < W; ++j) {
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t][j] = fmaf(g.v[j], xv[t], acc[t][j]);
            acc[9][j] += g.v[j];
        }
    }
    // the lanes of one channel group sit CW apart in a wavefront
#pragma unroll
    for (int o = CW; o < 64; o <<= 1)
#pragma unroll
        for (int t = 0; t < C1_ROWS; ++t)
#pragma unroll
            for (int j = 0; j < W; ++j) acc[t][j] += __shfl_xor(acc[t][j], o, 64);
    if ((threadIdx.x & 63) < CW) {
#pragma unroll
        for (int t = 0; t < C1_ROWS; ++t)
#pragma unroll
            for (int j = 0; j < W; ++j) sh[threadIdx.x >> 6][t * C1_CO + cg * W + j] = acc[t][j];
    }
    __syncthreads();
    float* dst = partial + (long long)blockIdx.x * (C1_ROWS * C1_CO);
    for (int r = threadIdx.x; r < C1_ROWS * C1_CO; r += 256) dst[r] = (sh[0][r] + sh[1][r]) + (sh[2][r] + sh[3][r]);
}
// one workgroup per row t (64 channels x 16 block-lanes, fixed summation order => bitwise reproducible)
__global__ __launch_bounds__(1024) void conv3x3_c1_wgrad_finalize(const float* __restrict__ partial, long long nblk, float* __restrict__ dw,
                                                                  float* __restrict__ db) {
    __shared__ double sh[16][C1_CO];
    const int t = blockIdx.x, co = threadIdx.x & 63, ln = threadIdx.x >> 6;
    double s = 0;
    for (long long b = ln; b < nblk; b += 16) s += partial[(b * C1_ROWS + t) * C1_CO + co];
    sh[ln][co] = s;
    __syncthreads();
    if (ln == 0) {
        for (int i = 1; i < 16; ++i) s += sh[i][co];
        if (t < 9) dw[co * 9 + t] = (float)s; else if (db) db[co] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------
// MaxPool2d(2, 2), floor mode
// ---------------------------------------------------------------------------------------
// W window indices (one byte each), stored and loaded in one W-byte access
template <int W> struct alignas(W) IdxPack { unsigned w[W / 4]; };

template <class T, int W>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx,
                                                           int n, int h, int w, int cw, int ho, int wo) {
    const long long total = (long long)n * ho * wo * cw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); long long p = i / cw;
        const int ox = (int)(p % wo); p /= wo;
        const int oy = (int)(p % ho); const int nn = (int)(p / ho);
        const T* src = x + ((((long long)nn * h + 2 * oy) * w + 2 * ox) * cw + cc) * W;
        const long long rs = (long long)w * cw * W;
        const typename Stream<T, W>::Raw r0 = Stream<T, W>::ldraw(src), r1 = Stream<T, W>::ldraw(src + cw * W);
        const typename Stream<T, W>::Raw r2 = Stream<T, W>::ldraw(src + rs), r3 = Stream<T, W>::ldraw(src + rs + cw * W);
        const FV<W> v[4] = {Stream<T, W>::unpack(r0), Stream<T, W>::unpack(r1), Stream<T, W>::unpack(r2), Stream<T, W>::unpack(r3)};
        FV<W> best = v[0];
        unsigned bi[W];
#pragma unroll
        for (int j = 0; j < W; ++j) bi[j] = 0;
        // ATen: the first element, then strictly-greater (or NaN) replaces -- the first maximum in row-major window order wins a tie
#pragma unroll
        for (unsigned t = 1; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (v[t].v[j] > best.v[j] || v[t].v[j] != v[t].v[j]) { best.v[j] = v[t].v[j]; bi[j] = t; }
        Stream<T, W>::st(y + i * W, best);
        IdxPack<W> pk;
#pragma unroll
        for (int q = 0; q < W / 4; ++q) pk.w[q] = bi[4 * q] | (bi[4 * q + 1] << 8) | (bi[4 * q + 2] << 16) | (bi[4 * q + 3] << 24);
        *reinterpret_cast<IdxPack<W>*>(idx + i * W) = pk;
    }
}
// one thread per INPUT element group: every element of dx is written exactly once -- the gradient where this position won its
// window, zero where it lost and in a trailing odd row / column that no window covers
template <class T, int W>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx,
                                                           int n, int h, int w, int cw, int ho, int wo) {
    const long long total = (long long)n * h * w * cw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); long long p = i / cw;
        const int ix = (int)(p % w); p /= w;
        const int iy = (int)(p % h); const int nn = (int)(p / h);
        FV<W> g;
#pragma unroll
        for (int j = 0; j < W; ++j) g.v[j] = 0.f;
        const int oy = iy >> 1, ox = ix >> 1;
        if (oy < ho && ox < wo) {
            const long long o = ((((long long)nn * ho + oy) * wo + ox) * cw + cc) * W;
            const IdxPack<W> t = *reinterpret_cast<const IdxPack<W>*>(idx + o);
            const FV<W> d = Stream<T, W>::ld(dy + o);
            const unsigned me = (unsigned)((iy & 1) * 2 + (ix & 1));
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (((t.w[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) g.v[j] = d.v[j];
        }
        Stream<T, W>::st(dx + i * W, g);
    }
}

// ---------------------------------------------------------------------------------------
// nn.Upsample(scale_factor=2), nearest: y[n][2i+a][2j+b][c] = x[n][i][j][c]
// ---------------------------------------------------------------------------------------
// One thread per SOURCE element group both ways: forward reads once and stores four times, backward reads the four gradients and
// stores their sum ((dy00 + dy01) + (dy10 + dy11): a fixed order).
template <class T, int W>
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int h, int w, int cw, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); long long p = i / cw;
        const int ix = (int)(p % w); p /= w;                              // p = n * h + iy
        const typename Stream<T, W>::Raw r = Stream<T, W>::ldraw(x + i * W);
        const FV<W> v = Stream<T, W>::unpack(r);
        T* dst = y + (((2 * p) * (2LL * w) + 2 * ix) * cw + cc) * W;
        const long long rs = 2LL * w * cw * W;
        Stream<T, W>::st(dst, v); Stream<T, W>::st(dst + cw * W, v);
        Stream<T, W>::st(dst + rs, v); Stream<T, W>::st(dst + rs + cw * W, v);
    }
}
template <class T, int W>
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int h, int w, int cw, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); long long p = i / cw;
        const int ix = (int)(p % w); p /= w;
        const T* src = dy + (((2 * p) * (2LL * w) + 2 * ix) * cw + cc) * W;
        const long long rs = 2LL * w * cw * W;
        const typename Stream<T, W>::Raw r0 = Stream<T, W>::ldraw(src), r1 = Stream<T, W>::ldraw(src + cw * W);
        const typename Stream<T, W>::Raw r2 = Stream<T, W>::ldraw(src + rs), r3 = Stream<T, W>::ldraw(src + rs + cw * W);
        const FV<W> a = Stream<T, W>::unpack(r0), b = Stream<T, W>::unpack(r1), c = Stream<T, W>::unpack(r2), d = Stream<T, W>::unpack(r3);
        FV<W> g;
#pragma unroll
        for (int j = 0; j < W; ++j) g.v[j] = (a.v[j] + b.v[j]) + (c.v[j] + d.v[j]);
        Stream<T, W>::st(dx + i * W, g);
    }
}

// ---------------------------------------------------------------------------------------
// channel concatenation of two row sources, and its two column slices back
// ---------------------------------------------------------------------------------------
// FWD: y[r][0..ca) = a[r * lda + .], y[r][ca..ca+cb) = b[r * ldb + .].  !FWD (a, b are the outputs, contiguous): the slices of y.
template <class T, int W, bool FWD>
__global__ __launch_bounds__(256) void concat2_kernel(T* __restrict__ a, long long lda, T* __restrict__ b, long long ldb, T* __restrict__ y,
                                                      int caw, int cw, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cw); const long long r = i / cw;
        T* part = cc < caw ? a + r * lda + (long long)cc * W : b + r * ldb + (long long)(cc - caw) * W;
        if (FWD) Stream<T, W>::st(y + i * W, Stream<T, W>::ld(part));
        else Stream<T, W>::st(part, Stream<T, W>::ld(y + i * W));
    }
}

// ---------------------------------------------------------------------------------------
// launchers: the extern "C" entry points of both families check their arguments and call these
// ---------------------------------------------------------------------------------------
inline long long c1_blocks(long long npix) { return (npix + C1_PIX - 1) / C1_PIX; }

template <class T, int W>
int launch_c1_fwd(const float* x, const float* w, const float* bias, void* y, int n, int h, int wd, hipStream_t s, const char* what) {
    const long long npix = (long long)n * h * wd;
    hipLaunchKernelGGL((conv3x3_c1_fwd_kernel<T, W>), dim3(stream_grid(npix * (C1_CO / W), 256)), dim3(256), 0, s, x, w, bias, static_cast<T*>(y), npix, h, wd);
    return glf::check_launch(what);
}
template <class T, int W>
int launch_c1_wgrad(const float* x, const void* dy, float* dw, float* db, float* partial, int n, int h, int wd, hipStream_t s, const char* what) {
    const long long npix = (long long)n * h * wd, nblk = c1_blocks(npix);
    hipLaunchKernelGGL((conv3x3_c1_wgrad_kernel<T, W>), dim3((unsigned)nblk), dim3(256), 0, s, x, static_cast<const T*>(dy), partial, npix, h, wd);
    if (int rc = glf::check_launch(what)) return rc;
    hipLaunchKernelGGL(conv3x3_c1_wgrad_finalize, dim3(C1_ROWS), dim3(1024), 0, s, partial, nblk, dw, db);
    return glf::check_launch(what);
}
template <class T, int W>
int launch_maxpool2(const void* a, uint8_t* idx, void* out, int n, int h, int w, int c, bool fwd, hipStream_t s, const char* what) {
    const int ho = h / 2, wo = w / 2;
    if (fwd) {
        hipLaunchKernelGGL((maxpool2_fwd_kernel<T, W>), dim3(stream_grid((long long)n * ho * wo * (c / W), 256)), dim3(256), 0, s,
                           static_cast<const T*>(a), static_cast<T*>(out), idx, n, h, w, c / W, ho, wo);
    } else {
        hipLaunchKernelGGL((maxpool2_bwd_kernel<T, W>), dim3(stream_grid((long long)n * h * w * (c / W), 256)), dim3(256), 0, s,
                           static_cast<const T*>(a), idx, static_cast<T*>(out), n, h, w, c / W, ho, wo);
    }
    return glf::check_launch(what);
}
template <class T, int W>
int launch_upsample2x(const void* in, void* out, int n, int h, int w, int c, bool fwd, hipStream_t s, const char* what) {
    const long long total = (long long)n * h * w * (c / W);
    if (fwd) hipLaunchKernelGGL((upsample2x_fwd_kernel<T, W>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<const T*>(in), static_cast<T*>(out), h, w, c / W, total);
    else hipLaunchKernelGGL((upsample2x_bwd_kernel<T, W>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<const T*>(in), static_cast<T*>(out), h, w, c / W, total);
    return glf::check_launch(what);
}
template <class T, int W, bool FWD>
int launch_concat2(const void* a, int64_t lda, const void* b, int64_t ldb, const void* y, int64_t rows, int ca, int cb, hipStream_t s, const char* what) {
    const long long total = (long long)rows * ((ca + cb) / W);
    hipLaunchKernelGGL((concat2_kernel<T, W, FWD>), dim3(stream_grid(total, 256)), dim3(256), 0, s, static_cast<T*>(const_cast<void*>(a)), (long long)lda,
                       static_cast<T*>(const_cast<void*>(b)), (long long)ldb, static_cast<T*>(const_cast<void*>(y)), ca / W, (ca + cb) / W, total);
    return glf::check_launch(what);
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
#define REQ_C1_SHAPE(what) \
    GLF_REQUIRE(cout == C1_CO, GLF_ERR_UNSUPPORTED, "conv3x3_c1: Cout must be 64 (got %d)", cout); \
    GLF_REQUIRE(n > 0 && h > 0 && wdt > 0, GLF_ERR_BAD_SHAPE, what ": bad shape")

extern "C" int glf_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wdt, int cout, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && w && y, GLF_ERR_NULL, "conv3x3_c1_fwd: null argument");
    REQ_C1_SHAPE("conv3x3_c1_fwd");
    REQ_AL(y, "conv3x3_c1_fwd: y");
    return launch_c1_fwd<float, 4>(x, w, bias, y, n, h, wdt, glf::S(s), "conv3x3_c1_fwd");
}
extern "C" int glf_s16_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, void* y, int n, int h, int wdt, int cout, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && w && y, GLF_ERR_NULL, "s16_conv3x3_c1_fwd: null argument");
    REQ_C1_SHAPE("s16_conv3x3_c1_fwd");
    REQ_AL(y, "s16_conv3x3_c1_fwd: y");
    return launch_c1_fwd<u16, 8>(x, w, bias, y, n, h, wdt, glf::S(s), "s16_conv3x3_c1_fwd");
}
extern "C" size_t glf_conv3x3_c1_wgrad_workspace(int n, int h, int wdt, int cout) {
    if (n <= 0 || h <= 0 || wdt <= 0 || cout <= 0) return 0;
    return (size_t)c1_blocks((long long)n * h * wdt) * C1_ROWS * (size_t)cout;
}
#define REQ_C1_WS() \
    GLF_REQUIRE(partial_floats >= glf_conv3x3_c1_wgrad_workspace(n, h, wdt, cout), GLF_ERR_WORKSPACE, \
                "conv3x3_c1_wgrad: workspace of %zu floats, %zu needed", partial_floats, glf_conv3x3_c1_wgrad_workspace(n, h, wdt, cout))
extern "C" int glf_conv3x3_c1_wgrad(const float* x, const float* dy, float* dw, float* db, float* partial, size_t partial_floats,
                                    int n, int h, int wdt, int cout, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && dy && dw && partial, GLF_ERR_NULL, "conv3x3_c1_wgrad: null argument");
    REQ_C1_SHAPE("conv3x3_c1_wgrad");
    REQ_AL(dy, "conv3x3_c1_wgrad: dy");
    REQ_C1_WS();
    return launch_c1_wgrad<float, 4>(x, dy, dw, db, partial, n, h, wdt, glf::S(s), "conv3x3_c1_wgrad");
}
extern "C" int glf_s16_conv3x3_c1_wgrad(const float* x, const void* dy, float* dw, float* db, float* partial, size_t partial_floats,
                                        int n, int h, int wdt, int cout, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && dy && dw && partial, GLF_ERR_NULL, "s16_conv3x3_c1_wgrad: null argument");
    REQ_C1_SHAPE("s16_conv3x3_c1_wgrad");
    REQ_AL(dy, "s16_conv3x3_c1_wgrad: dy");
    REQ_C1_WS();
    return launch_c1_wgrad<u16, 8>(x, dy, dw, db, partial, n, h, wdt, glf::S(s), "s16_conv3x3_c1_wgrad");
}

// fp32: C % 4, 16-byte tensors, 4-byte index groups; bf16: C % 8, 16-byte tensors, 8-byte index groups
#define REQ_POOL2(what, p0, p1, C_OK, IDX_MASK) \
    GLF_REQUIRE(p0 && p1 && idx, GLF_ERR_NULL, what ": null argument"); \
    GLF_REQUIRE(n > 0 && h >= 2 && w >= 2, GLF_ERR_BAD_SHAPE, what ": bad extents (H, W >= 2 required)"); \
    GLF_REQUIRE(C_OK, GLF_ERR_BAD_SHAPE, what ": the channel count must be a positive multiple of the 16-byte access (got %d)", c); \
    GLF_REQUIRE(al16(p0) && al16(p1) && ((reinterpret_cast<uintptr_t>(idx) & IDX_MASK) == 0), GLF_ERR_BAD_SHAPE, what ": alignment")

extern "C" int glf_maxpool2x2s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_POOL2("maxpool2x2s2_fwd", x, y, c > 0 && (c % 4) == 0, 3u);
    return launch_maxpool2<float, 4>(x, idx, y, n, h, w, c, true, glf::S(s), "maxpool2x2s2_fwd");
}
extern "C" int glf_maxpool2x2s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_POOL2("maxpool2x2s2_bwd", dy, dx, c > 0 && (c % 4) == 0, 3u);
    return launch_maxpool2<float, 4>(dy, const_cast<uint8_t*>(idx), dx, n, h, w, c, false, glf::S(s), "maxpool2x2s2_bwd");
}
extern "C" int glf_s16_maxpool2x2s2_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_POOL2("s16_maxpool2x2s2_fwd", x, y, c > 0 && (c % 8) == 0, 7u);
    return launch_maxpool2<u16, 8>(x, idx, y, n, h, w, c, true, glf::S(s), "s16_maxpool2x2s2_fwd");
}
extern "C" int glf_s16_maxpool2x2s2_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_POOL2("s16_maxpool2x2s2_bwd", dy, dx, c > 0 && (c % 8) == 0, 7u);
    return launch_maxpool2<u16, 8>(dy, const_cast<uint8_t*>(idx), dx, n, h, w, c, false, glf::S(s), "s16_maxpool2x2s2_bwd");
}

#define REQ_UP2(what, p0, p1, C_OK) \
    GLF_REQUIRE(p0 && p1, GLF_ERR_NULL, what ": null argument"); \
    GLF_REQUIRE(n > 0 && h > 0 && w > 0, GLF_ERR_BAD_SHAPE, what ": bad extents"); \
    GLF_REQUIRE(C_OK, GLF_ERR_BAD_SHAPE, what ": the channel count must be a positive multiple of the 16-byte access (got %d)", c); \
    GLF_REQUIRE(al16(p0) && al16(p1), GLF_ERR_BAD_SHAPE, what ": tensors must be 16-byte aligned")

extern "C" int glf_upsample2x_fwd(const float* x, float* y, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_UP2("upsample2x_fwd", x, y, c > 0 && (c % 4) == 0);
    return launch_upsample2x<float, 4>(x, y, n, h, w, c, true, glf::S(s), "upsample2x_fwd");
}
extern "C" int glf_upsample2x_bwd(const float* dy, float* dx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_UP2("upsample2x_bwd", dy, dx, c > 0 && (c % 4) == 0);
    return launch_upsample2x<float, 4>(dy, dx, n, h, w, c, false, glf::S(s), "upsample2x_bwd");
}
extern "C" int glf_s16_upsample2x_fwd(const void* x, void* y, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_UP2("s16_upsample2x_fwd", x, y, c > 0 && (c % 8) == 0);
    return launch_upsample2x<u16, 8>(x, y, n, h, w, c, true, glf::S(s), "s16_upsample2x_fwd");
}
extern "C" int glf_s16_upsample2x_bwd(const void* dy, void* dx, int n, int h, int w, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_UP2("s16_upsample2x_bwd", dy, dx, c > 0 && (c % 8) == 0);
    return launch_upsample2x<u16, 8>(dy, dx, n, h, w, c, false, glf::S(s), "s16_upsample2x_bwd");
}

// Wd = elements per 16-byte access.  Row strides count elements.
#define REQ_CAT2(what, Wd) \
    GLF_REQUIRE(a && b && y, GLF_ERR_NULL, what ": null argument"); \
    GLF_REQUIRE(rows > 0 && ca > 0 && cb > 0, GLF_ERR_BAD_SHAPE, what ": bad extents"); \
    GLF_REQUIRE((ca % Wd) == 0 && (cb % Wd) == 0 && (lda % Wd) == 0 && (ldb % Wd) == 0 && lda >= ca && ldb >= cb, GLF_ERR_BAD_SHAPE, \
                what ": channel counts and row strides must be multiples of the 16-byte access, strides >= widths"); \
    GLF_REQUIRE(al16(a) && al16(b) && al16(y), GLF_ERR_BAD_SHAPE, what ": tensors must be 16-byte aligned")

extern "C" int glf_concat2_fwd(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t rows, int ca, int cb, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_CAT2("concat2_fwd", 4);
    return launch_concat2<float, 4, true>(a, lda, b, ldb, y, rows, ca, cb, glf::S(s), "concat2_fwd");
}
extern "C" int glf_s16_concat2_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t rows, int ca, int cb, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    REQ_CAT2("s16_concat2_fwd", 8);
    return launch_concat2<u16, 8, true>(a, lda, b, ldb, y, rows, ca, cb, glf::S(s), "s16_concat2_fwd");
}
extern "C" int glf_concat2_bwd(const float* dy, float* da, float* db, int64_t rows, int ca, int cb, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    const float* y = dy; float *a = da, *b = db; const int64_t lda = ca, ldb = cb;
    REQ_CAT2("concat2_bwd", 4);
    return launch_concat2<float, 4, false>(a, lda, b, ldb, y, rows, ca, cb, glf::S(s), "concat2_bwd");
}
extern "C" int glf_s16_concat2_bwd(const void* dy, void* da, void* db, int64_t rows, int ca, int cb, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    const void* y = dy; void *a = da, *b = db; const int64_t lda = ca, ldb = cb;
    REQ_CAT2("s16_concat2_bwd", 8);
    return launch_concat2<u16, 8, false>(a, lda, b, ldb, y, rows, ca, cb, glf::S(s), "s16_concat2_bwd");
}

// Fused multi-tensor Adam: torch.optim.Adam as the reference constructs it (main.py:162-165: lr,
// weight_decay as L2-in-gradient, default betas / eps, no amsgrad) over every parameter in ONE launch.
// HBM-bound: 16 B read + 12 B written per element.
// Fused multi-tensor SGD: torch.optim.SGD (main.py:159-161, plus momentum / dampening / nesterov) over the same table,
// 12 B read + 8 B written per element with a momentum buffer, 8 B + 4 B without.
// Global-norm gradient clipping over the same table: one extra read of the gradients (sum of squares per row in double, no
// atomics), a one-workgroup finish that leaves { norm, coef, ok } on the device, and CLIP forms of the two update kernels that
// multiply every gradient element by coef -- or leave everything untouched when the norm is not finite.
#include "glf_common.h"
#include <cmath>

namespace {

// One row per chunk of one parameter: pointers and element count.
struct AdamRow { long long p, g, m, v, n; };

// Same operation order as torch.optim._functional.adam (torch 1.8.1); every operation individually rounded
// (__f*_rn keep hipcc from contracting them into fmas) so the update equals the ATen CPU kernels' bit for bit up to
// the rounding of sqrt / division.
struct AdamK { float b1, b2, omb1, omb2, eps, wd, step_size, sqrt_bc2; };

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamK k) {
    const float b1 = k.b1, b2 = k.b2, eps = k.eps, wd = k.wd, step_size = k.step_size, sqrt_bc2 = k.sqrt_bc2;
    if (wd != 0.f) g = __fadd_rn(g, __fmul_rn(wd, p));
    m = __fadd_rn(__fmul_rn(m, b1), __fmul_rn(k.omb1, g));                       // mul_(beta1).add_(grad, alpha = 1 - beta1)
    v = __fadd_rn(__fmul_rn(v, b2), __fmul_rn(__fmul_rn(k.omb2, g), g));         // mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), sqrt_bc2), eps);
    p = __fadd_rn(p, __fmul_rn(-step_size, __fdiv_rn(m, denom)));
}

// The record glf_grad_clip_coef leaves on the device: the global gradient norm, the clip coefficient and "the norm is finite".
struct ClipRecord { float norm, coef, ok, pad; };

// An individually rounded product: see the note above SgdK.
__device__ __forceinline__ float mul_rn(float a, float b) {
    float t = a * b;
    asm("" : "+v"(t));
    return t;
}

// CLIP: every gradient element becomes g * coef (individually rounded) before the weight decay; a workgroup that finds
// ok == 0 returns before it touches anything.  CLIP = false never looks at `rec`.
template <bool CLIP>
__global__ __launch_bounds__(256) void adam_kernel(const AdamRow* __restrict__ table, int n_rows, const AdamK k,
                                                   const ClipRecord* __restrict__ rec) {
    float coef = 1.f;
    if (CLIP) {
        if (rec->ok == 0.f) return;
        coef = rec->coef;
    }
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const AdamRow r = table[row];
        float* __restrict__ p = reinterpret_cast<float*>(r.p);
        const float* __restrict__ g = reinterpret_cast<const float*>(r.g);
        float* __restrict__ m = reinterpret_cast<float*>(r.m);
        float* __restrict__ v = reinterpret_cast<float*>(r.v);
        const int n = (int)r.n;
        const bool vec = (((r.p | r.g | r.m | r.v) & 15) == 0);
        const int n4 = vec ? n >> 2 : 0;
        for (int i = threadIdx.x; i < n4; i += blockDim.x) {
            float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            float4 gg = reinterpret_cast<const float4*>(g)[i];
            if (CLIP) { gg.x = mul_rn(gg.x, coef); gg.y = mul_rn(gg.y, coef); gg.z = mul_rn(gg.z, coef); gg.w = mul_rn(gg.w, coef); }
            adam1(pp.x, gg.x, mm.x, vv.x, k);
            adam1(pp.y, gg.y, mm.y, vv.y, k);
            adam1(pp.z, gg.z, mm.z, vv.z, k);
            adam1(pp.w, gg.w, mm.w, vv.w, k);
            reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
        }
        for (int i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam1(pp, CLIP ? mul_rn(g[i], coef) : g[i], mm, vv, k);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}

// Same operation order as torch.optim.sgd._single_tensor_sgd, every operation individually rounded.  The build contracts
// a * b + c into an fma in the backend (-ffp-contract=fast), where neither `#pragma clang fp contract(off)` nor __fmul_rn /
// __fadd_rn (plain operators in a header; adam1's products are fused) stop it: each product passes through an empty asm that
// makes it an opaque register value, so the addition that follows cannot absorb it.
struct SgdK { float wd, mom, omd, neg_lr; int first, nesterov; };

template <bool MOM>
__device__ __forceinline__ void sgd1(float& p, float g, float& m, const SgdK k, const bool first) {
    if (k.wd != 0.f) g = g + mul_rn(k.wd, p);                                        // grad.add(param, alpha = weight_decay)
    if (MOM) {
        m = first ? g : mul_rn(m, k.mom) + mul_rn(k.omd, g);                         // clone(grad) | mul_(momentum).add_(grad, alpha = 1 - dampening)
        g = k.nesterov ? g + mul_rn(k.mom, m) : m;                                   // grad.add(buf, alpha = momentum) | buf
    }
    p = p + mul_rn(k.neg_lr, g);                                                     // param.add_(grad, alpha = -lr)
}

// What optim.SGD fills a momentum buffer with that it creates while clipping is on: a quiet NaN whose payload no arithmetic
// produces.  The step that was to write the buffer may be skipped on the device, unknown to the host, which files the buffer
// under "has one" from then on; a row of the CLIP kernel that still finds the mark in its first element is a first step.
constexpr unsigned UNBORN = 0x7fc0dead;

// MOM = false: column m of the table is never dereferenced (it may be 0) and does not count for the alignment test.
// CLIP: as in adam_kernel; the skipped workgroup does not write a first momentum buffer either.
template <bool MOM, bool CLIP>
__global__ __launch_bounds__(256) void sgd_kernel(const AdamRow* __restrict__ table, int n_rows, const SgdK k,
                                                  const ClipRecord* __restrict__ rec) {
    float coef = 1.f;
    if (CLIP) {
        if (rec->ok == 0.f) return;
        coef = rec->coef;
    }
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const AdamRow r = table[row];
        float* __restrict__ p = reinterpret_cast<float*>(r.p);
        const float* __restrict__ g = reinterpret_cast<const float*>(r.g);
        float* __restrict__ m = reinterpret_cast<float*>(r.m);
        const int n = (int)r.n;
        const bool vec = (((r.p | r.g | (MOM ? r.m : 0)) & 15) == 0);
        const int n4 = vec ? n >> 2 : 0;
        bool first = k.first;
        if (CLIP && MOM) {
            if (!first && n > 0) first = __float_as_uint(*reinterpret_cast<const volatile float*>(m)) == UNBORN;
            __syncthreads();                                                         // every thread has looked before one writes m[0]
        }
        for (int i = threadIdx.x; i < n4; i += blockDim.x) {
            float4 pp = reinterpret_cast<float4*>(p)[i], mm = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 gg = reinterpret_cast<const float4*>(g)[i];
            if (CLIP) { gg.x = mul_rn(gg.x, coef); gg.y = mul_rn(gg.y, coef); gg.z = mul_rn(gg.z, coef); gg.w = mul_rn(gg.w, coef); }
            if (MOM && !first) mm = reinterpret_cast<float4*>(m)[i];
            sgd1<MOM>(pp.x, gg.x, mm.x, k, first);
            sgd1<MOM>(pp.y, gg.y, mm.y, k, first);
            sgd1<MOM>(pp.z, gg.z, mm.z, k, first);
            sgd1<MOM>(pp.w, gg.w, mm.w, k, first);
            reinterpret_cast<float4*>(p)[i] = pp;
            if (MOM) reinterpret_cast<float4*>(m)[i] = mm;
        }
        for (int i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
            float pp = p[i], mm = 0.f;
            if (MOM && !first) mm = m[i];
            sgd1<MOM>(pp, CLIP ? mul_rn(g[i], coef) : g[i], mm, k, first);
            p[i] = pp;
            if (MOM) m[i] = mm;
        }
    }
}

// partials[row] = sum of g^2 over the row, in double: each thread's own elements in index order, the 64 lanes of a wave by
// a shuffle tree, the four waves in order.  No atomics: the same bits on every run.
__global__ __launch_bounds__(256) void sumsq_kernel(const AdamRow* __restrict__ table, int n_rows, double* __restrict__ partials) {
    __shared__ double wave_sum[4];
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const AdamRow r = table[row];
        const float* __restrict__ g = reinterpret_cast<const float*>(r.g);
        const int n = (int)r.n;
        const int n4 = (r.g & 15) == 0 ? n >> 2 : 0;
        double acc = 0.0;
        for (int i = threadIdx.x; i < n4; i += blockDim.x) {
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            acc += (double)gg.x * (double)gg.x;
            acc += (double)gg.y * (double)gg.y;
            acc += (double)gg.z * (double)gg.z;
            acc += (double)gg.w * (double)gg.w;
        }
        for (int i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) acc += (double)g[i] * (double)g[i];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partials[row] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
        __syncthreads();                                                             // wave_sum is free for the next row
    }
}

// One workgroup: partials[0..n) added in index order in double (staged through LDS a tile at a time, so the serial chain runs
// on LDS latency), then the record.  coef is torch.nn.utils.clip_grad_norm_'s expression on a float32 norm.
__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ partials, int n, float max_norm,
                                                        ClipRecord* __restrict__ rec, long long* __restrict__ skipped) {
    __shared__ double tile[256];
    double sum = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        tile[threadIdx.x] = i < n ? partials[i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - base < 256 ? n - base : 256;
            for (int j = 0; j < m; ++j) sum += tile[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool ok = isfinite(sum);
        const float norm = (float)sqrt(sum);
        const float q = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
        rec->norm = norm;
        rec->coef = ok ? fminf(1.0f, q) : 0.0f;
        rec->ok = ok ? 1.0f : 0.0f;
        rec->pad = 0.0f;
        if (!ok) *skipped += 1;
    }
}

// g *= coef over the table (glf_grad_scale); nothing is written when the norm is not finite or nothing is to clip.
__global__ __launch_bounds__(256) void grad_scale_kernel(const AdamRow* __restrict__ table, int n_rows, const ClipRecord* __restrict__ rec) {
    if (rec->ok == 0.f) return;
    const float coef = rec->coef;
    if (coef == 1.f) return;
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const AdamRow r = table[row];
        float* __restrict__ g = reinterpret_cast<float*>(r.g);
        const int n = (int)r.n;
        const int n4 = (r.g & 15) == 0 ? n >> 2 : 0;
        for (int i = threadIdx.x; i < n4; i += blockDim.x) {
            float4 gg = reinterpret_cast<float4*>(g)[i];
            gg.x *= coef; gg.y *= coef; gg.z *= coef; gg.w *= coef;
            reinterpret_cast<float4*>(g)[i] = gg;
        }
        for (int i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) g[i] *= coef;
    }
}

// The checks the step functions share with their clipped twins, before any HIP runtime call.
int sgd_args(const char* fn, const int64_t* table, int n_rows, double momentum, double dampening, int nesterov) {
    GLF_REQUIRE(n_rows > 0, GLF_ERR_BAD_SHAPE, "%s: n_rows must be > 0", fn);
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, GLF_ERR_BAD_SHAPE, "%s: table must be 8-byte aligned", fn);
    GLF_REQUIRE(momentum >= 0.0, GLF_ERR_BAD_SHAPE, "%s: momentum must be >= 0", fn);
    GLF_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), GLF_ERR_BAD_SHAPE,
                "%s: nesterov needs a momentum > 0 and zero dampening", fn);
    return GLF_OK;
}

int sgd_launch(const char* fn, const int64_t* table, int n_rows, double lr, double momentum, double dampening, double weight_decay,
               int nesterov, int first, const float* record, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    // scalars exactly as torch derives them: in double on the host, rounded to float once
    SgdK k;
    k.wd = (float)weight_decay; k.mom = (float)momentum; k.omd = (float)(1.0 - dampening); k.neg_lr = (float)(-lr);
    k.first = first != 0; k.nesterov = nesterov != 0;
    const int blocks = n_rows < 8192 ? n_rows : 8192;
    const AdamRow* t = reinterpret_cast<const AdamRow*>(table);
    const ClipRecord* rec = reinterpret_cast<const ClipRecord*>(record);
    if (momentum != 0.0) {
        if (rec) hipLaunchKernelGGL((sgd_kernel<true, true>), dim3(blocks), dim3(256), 0, glf::S(s), t, n_rows, k, rec);
        else     hipLaunchKernelGGL((sgd_kernel<true, false>), dim3(blocks), dim3(256), 0, glf::S(s), t, n_rows, k, rec);
    } else {
        if (rec) hipLaunchKernelGGL((sgd_kernel<false, true>), dim3(blocks), dim3(256), 0, glf::S(s), t, n_rows, k, rec);
        else     hipLaunchKernelGGL((sgd_kernel<false, false>), dim3(blocks), dim3(256), 0, glf::S(s), t, n_rows, k, rec);
    }
    return glf::check_launch(fn);
}

int adam_launch(const char* fn, const int64_t* table, int n_rows, double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step, const float* record, glf_stream_t s) {
    // scalars exactly as torch derives them: in double on the host, rounded to float once
    AdamK k;
    k.b1 = (float)beta1; k.b2 = (float)beta2; k.omb1 = (float)(1.0 - beta1); k.omb2 = (float)(1.0 - beta2);
    k.eps = (float)eps; k.wd = (float)weight_decay;
    k.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    k.sqrt_bc2 = (float)sqrt(1.0 - pow(beta2, (double)step));
    const int blocks = n_rows < 8192 ? n_rows : 8192;
    const AdamRow* t = reinterpret_cast<const AdamRow*>(table);
    const ClipRecord* rec = reinterpret_cast<const ClipRecord*>(record);
    if (rec) hipLaunchKernelGGL(adam_kernel<true>, dim3(blocks), dim3(256), 0, glf::S(s), t, n_rows, k, rec);
    else     hipLaunchKernelGGL(adam_kernel<false>, dim3(blocks), dim3(256), 0, glf::S(s), t, n_rows, k, rec);
    return glf::check_launch(fn);
}

}  // namespace

extern "C" int glf_sgd_step(const int64_t* table, int n_rows, double lr, double momentum, double dampening, double weight_decay,
                            int nesterov, int first, glf_stream_t s) {
    GLF_REQUIRE(table != nullptr, GLF_ERR_NULL, "sgd_step: null table");
    if (int rc = sgd_args("sgd_step", table, n_rows, momentum, dampening, nesterov)) return rc;
    return sgd_launch("sgd_step", table, n_rows, lr, momentum, dampening, weight_decay, nesterov, first, nullptr, s);
}

extern "C" int glf_sgd_step_clipped(const int64_t* table, int n_rows, double lr, double momentum, double dampening,
                                    double weight_decay, int nesterov, int first, const float* record, glf_stream_t s) {
    GLF_REQUIRE(table != nullptr, GLF_ERR_NULL, "sgd_step_clipped: null table");
    GLF_REQUIRE(record != nullptr, GLF_ERR_NULL, "sgd_step_clipped: null record");
    if (int rc = sgd_args("sgd_step_clipped", table, n_rows, momentum, dampening, nesterov)) return rc;
    return sgd_launch("sgd_step_clipped", table, n_rows, lr, momentum, dampening, weight_decay, nesterov, first, record, s);
}

extern "C" int glf_adam_step(const int64_t* table, int n_rows, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int64_t step, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(table != nullptr, GLF_ERR_NULL, "adam_step: null table");
    GLF_REQUIRE(n_rows > 0, GLF_ERR_BAD_SHAPE, "adam_step: n_rows must be > 0");
    GLF_REQUIRE(step >= 1, GLF_ERR_BAD_SHAPE, "adam_step: step counts from 1");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, GLF_ERR_BAD_SHAPE, "adam_step: table must be 8-byte aligned");
    return adam_launch("adam_step", table, n_rows, lr, beta1, beta2, eps, weight_decay, step, nullptr, s);
}

extern "C" int glf_adam_step_clipped(const int64_t* table, int n_rows, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int64_t step, const float* record, glf_stream_t s) {
    GLF_REQUIRE(table != nullptr, GLF_ERR_NULL, "adam_step_clipped: null table");
    GLF_REQUIRE(record != nullptr, GLF_ERR_NULL, "adam_step_clipped: null record");
    GLF_REQUIRE(n_rows > 0, GLF_ERR_BAD_SHAPE, "adam_step_clipped: n_rows must be > 0");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, GLF_ERR_BAD_SHAPE, "adam_step_clipped: table must be 8-byte aligned");
    GLF_REQUIRE(step >= 1, GLF_ERR_BAD_SHAPE, "adam_step_clipped: step counts from 1");
    if (int rc = glf::ensure_init()) return rc;
    return adam_launch("adam_step_clipped", table, n_rows, lr, beta1, beta2, eps, weight_decay, step, record, s);
}

extern "C" int glf_grad_sumsq(const int64_t* table, int n_rows, double* partials, glf_stream_t s) {
    GLF_REQUIRE(table != nullptr, GLF_ERR_NULL, "grad_sumsq: null table");
    GLF_REQUIRE(partials != nullptr, GLF_ERR_NULL, "grad_sumsq: null partials");
    GLF_REQUIRE(n_rows > 0, GLF_ERR_BAD_SHAPE, "grad_sumsq: n_rows must be > 0");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, GLF_ERR_BAD_SHAPE, "grad_sumsq: table must be 8-byte aligned");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0, GLF_ERR_BAD_SHAPE, "grad_sumsq: partials must be 8-byte aligned");
    if (int rc = glf::ensure_init()) return rc;
    const int blocks = n_rows < 8192 ? n_rows : 8192;
    hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(256), 0, glf::S(s), reinterpret_cast<const AdamRow*>(table), n_rows, partials);
    return glf::check_launch("grad_sumsq");
}

extern "C" int glf_grad_clip_coef(const double* partials, int n, double max_norm, float* record, int64_t* skipped, glf_stream_t s) {
    GLF_REQUIRE(partials != nullptr, GLF_ERR_NULL, "grad_clip_coef: null partials");
    GLF_REQUIRE(record != nullptr, GLF_ERR_NULL, "grad_clip_coef: null record");
    GLF_REQUIRE(skipped != nullptr, GLF_ERR_NULL, "grad_clip_coef: null skipped-step counter");
    GLF_REQUIRE(n > 0, GLF_ERR_BAD_SHAPE, "grad_clip_coef: n must be > 0");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0, GLF_ERR_BAD_SHAPE, "grad_clip_coef: partials must be 8-byte aligned");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(record) & 3u) == 0 && (reinterpret_cast<uintptr_t>(skipped) & 7u) == 0, GLF_ERR_BAD_SHAPE,
                "grad_clip_coef: record must be 4-byte and the counter 8-byte aligned");
    GLF_REQUIRE(max_norm >= 0.0, GLF_ERR_BAD_SHAPE, "grad_clip_coef: max_norm must be >= 0 and not NaN (+inf is legal)");
    if (int rc = glf::ensure_init()) return rc;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, glf::S(s), partials, n, (float)max_norm,
                       reinterpret_cast<ClipRecord*>(record), reinterpret_cast<long long*>(skipped));
    return glf::check_launch("grad_clip_coef");
}

extern "C" int glf_grad_scale(const int64_t* table, int n_rows, const float* record, glf_stream_t s) {
    GLF_REQUIRE(table != nullptr, GLF_ERR_NULL, "grad_scale: null table");
    GLF_REQUIRE(record != nullptr, GLF_ERR_NULL, "grad_scale: null record");
    GLF_REQUIRE(n_rows > 0, GLF_ERR_BAD_SHAPE, "grad_scale: n_rows must be > 0");
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, GLF_ERR_BAD_SHAPE, "grad_scale: table must be 8-byte aligned");
    if (int rc = glf::ensure_init()) return rc;
    const int blocks = n_rows < 8192 ? n_rows : 8192;
    hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks), dim3(256), 0, glf::S(s), reinterpret_cast<const AdamRow*>(table), n_rows,
                       reinterpret_cast<const ClipRecord*>(record));
    return glf::check_launch("grad_scale");
}

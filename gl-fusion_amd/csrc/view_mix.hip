// The per-view 1x1 convolutions over the channel concatenation of all views that the classical fusion baselines own (early_fusion:
// Conv2d(V, 1, 1) on the images; late_fusion: Conv2d(5 V, 5, 1) on the head logits; ours.py:2251-2383) as ONE streaming pass (gfx950):
//   y_v[r][o] = b_v[o] + sum_u sum_i W_v[o][u c + i] x_u[r][i]
// with the V inputs and the V outputs as separate contiguous fp32 [rows][c] tensors and the V weights stacked by rows into one
// [V c][V c] matrix.  K = V c is 3 or 15 at three views: no contraction kernel takes that, and the views are separate tensors, so
// every view is read once and every view's output written once here instead.  All data is fp32 under every precision (the images
// and the head logits are fp32 under bf16 storage too): one instantiation per (V, c), no Stream<bf16> twin.  No float atomics.
#include "stream_common.h"

using namespace glf;

namespace {

constexpr int VM_MAX_V = 8, VM_MAX_C = 8, VM_MAX_VC = 40;      // five views x five classes fit, with room
constexpr int VM_WGRAD_ROWS = 1024;     // consecutive rows one workgroup reduces in wgrad (one block of partial sums each)
constexpr int VM_TILE = 64;             // rows of that run staged in LDS at a time
constexpr int VM_FIN_SUMS = 16;         // sums one finalize workgroup folds (x 16 block lanes)

struct VmIn { const float* p[VM_MAX_V]; };
struct VmOut { float* p[VM_MAX_V]; };

constexpr int vm_group(int c) { return (c % 4 == 0) ? 1 : ((c % 2 == 0) ? 2 : 4); }       // 4 / gcd(c, 4)

// One row of the mix in plain scalar code (the rows past the last whole group).
template <int V, int C>
__device__ __forceinline__ void vm_row(const VmIn& in, const VmOut& out, const float* sw, const float* sb, long long r) {
    constexpr int VC = V * C;
    float x[VC];
#pragma unroll
    for (int u = 0; u < V; ++u)
#pragma unroll
        for (int i = 0; i < C; ++i) x[u * C + i] = in.p[u][r * C + i];
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int o = 0; o < C; ++o) {
            float acc = sb[v * C + o];
#pragma unroll
            for (int k = 0; k < VC; ++k) acc = fmaf(sw[(v * C + o) * VC + k], x[k], acc);
            out.p[v][r * C + o] = acc;
        }
}

// A thread owns the smallest run of rows whose bytes are a multiple of 16 -- G = 4 / gcd(C, 4) rows, G C / 4 accesses of 16 bytes per
// view -- reads that run of every view into registers, and writes it for one output view after the other.  The matrix (transposed
// on the way in for dgrad: the same body) and the bias sit in LDS and are read at wavefront-uniform addresses: every lane reads the
// same word, which the LDS broadcasts without a bank conflict.  An output is bias + a chain of V C fused multiply-adds in column order.
template <int V, int C>
__global__ __launch_bounds__(256) void view_mix_kernel(VmIn in, VmOut out, const float* __restrict__ w, const float* __restrict__ bias,
                                                       long long rows, int transposed) {
    constexpr int VC = V * C, G = vm_group(C), Q = G * C / 4;
    __shared__ __attribute__((aligned(16))) float sw[VC * VC];
    __shared__ float sb[VC];
    for (int i = threadIdx.x; i < VC * VC; i += 256) { const int j = i / VC, k = i - j * VC; sw[i] = transposed ? w[k * VC + j] : w[i]; }
    for (int i = threadIdx.x; i < VC; i += 256) sb[i] = bias ? bias[i] : 0.f;
    __syncthreads();
    const long long groups = rows / G;
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        float x[V][G * C];
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float* src = in.p[u] + g * (G * C);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const FV<4> t = Stream<float, 4>::ld(src + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[u][4 * q + e] = t.v[e];
            }
        }
        for (int v = 0; v < V; ++v) {
            float y[G * C];
#pragma unroll
            for (int o = 0; o < C; ++o) {
                const float* wr = sw + (v * C + o) * VC;
                const float b = sb[v * C + o];
#pragma unroll
                for (int r = 0; r < G; ++r) y[r * C + o] = b;
#pragma unroll
                for (int u = 0; u < V; ++u)
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const float wv = wr[u * C + i];
#pragma unroll
                        for (int r = 0; r < G; ++r) y[r * C + o] = fmaf(wv, x[u][r * C + i], y[r * C + o]);
                    }
            }
            float* dst = out.p[v] + g * (G * C);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                FV<4> t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t.v[e] = y[4 * q + e];
                Stream<float, 4>::st(dst + 4 * q, t);
            }
        }
    }
    // the rows left over (fewer than G): one thread each, scalar
    const long long tail0 = groups * G, t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (tail0 + t < rows) vm_row<V, C>(in, out, sw, sb, tail0 + t);
}

// dW[v c + o][u c + i] = sum_r dy_v[r][o] x_u[r][i], db[v c + o] = sum_r dy_v[r][o]: S = VC (VC + 1) sums, the bias as column VC of
// a [VC][VC + 1] matrix (its "input" is 1).  One workgroup = VM_WGRAD_ROWS consecutive rows, staged VM_TILE rows at a time in LDS
// as [row][VC] of x and of dy.  The sums are tiled over the threads: with S <= 256 a thread is (sum, row lane) -- 256 / S lanes share
// the rows of a tile and are folded through LDS in lane order -- and with S > 256 a thread owns up to seven sums (S <= 1640) and
// every row.  A wavefront's lanes read consecutive columns of one x row (consecutive banks) and one or two dy words (broadcast).
// partial[block][S]; view_mix_wgrad_finalize folds the blocks.
__global__ __launch_bounds__(256) void view_mix_wgrad_kernel(VmIn xs, VmIn dys, float* __restrict__ partial, long long rows, int V, int C) {
    constexpr int MAXQ = (VM_MAX_VC * (VM_MAX_VC + 1) + 255) / 256;       // 7
    __shared__ __attribute__((aligned(16))) float sx[VM_TILE * VM_MAX_VC];
    __shared__ __attribute__((aligned(16))) float sd[VM_TILE * VM_MAX_VC];
    __shared__ float red[256];
    const int VC = V * C, S = VC * (VC + 1);
    const int lanes = S <= 256 ? 256 / S : 1;
    const int ln = S <= 256 ? threadIdx.x / S : 0;
    const int s0 = S <= 256 ? threadIdx.x - ln * S : threadIdx.x;
    const bool live = ln < lanes;
    int dj[MAXQ], xk[MAXQ];
    float acc[MAXQ];
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
        const int s = s0 + 256 * q;
        dj[q] = (live && s < S) ? s / (VC + 1) : -1;
        xk[q] = s - (s / (VC + 1)) * (VC + 1);
        acc[q] = 0.f;
    }
    const long long r0 = (long long)blockIdx.x * VM_WGRAD_ROWS;
    const int cnt = (int)(rows - r0 < VM_WGRAD_ROWS ? rows - r0 : VM_WGRAD_ROWS);
    for (int t0 = 0; t0 < cnt; t0 += VM_TILE) {
        const int tn = cnt - t0 < VM_TILE ? cnt - t0 : VM_TILE;
        const int ne = tn * C, n4 = ne / 4;                               // elements of this tile per view; a tile starts 16-byte aligned
        __syncthreads();                                                  // the previous tile has been consumed
        for (int u = 0; u < V; ++u) {
            const float* px = xs.p[u] + (r0 + t0) * C;
            const float* pd = dys.p[u] + (r0 + t0) * C;
            for (int i = threadIdx.x; i < n4; i += 256) {
                const FV<4> a = Stream<float, 4>::ld(px + 4 * i), b = Stream<float, 4>::ld(pd + 4 * i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int el = 4 * i + e, r = el / C, ci = el - r * C;
                    sx[r * VC + u * C + ci] = a.v[e];
                    sd[r * VC + u * C + ci] = b.v[e];
                }
            }
            for (int el = 4 * n4 + threadIdx.x; el < ne; el += 256) {
                const int r = el / C, ci = el - r * C;
                sx[r * VC + u * C + ci] = px[el];
                sd[r * VC + u * C + ci] = pd[el];
            }
        }
        __syncthreads();
        if (S <= 256) {                       // one sum per thread: a plain loop whose LDS reads the compiler can issue ahead
            if (dj[0] >= 0) {
                const int j = dj[0], k = xk[0] < VC ? xk[0] : -1;
                float a = acc[0];
#pragma unroll 4
                for (int r = ln; r < tn; r += lanes) a = fmaf(sd[r * VC + j], k >= 0 ? sx[r * VC + k] : 1.f, a);
                acc[0] = a;
            }
        } else {
            for (int r = 0; r < tn; ++r) {
#pragma unroll
                for (int q = 0; q < MAXQ; ++q)
                    if (dj[q] >= 0) acc[q] = fmaf(sd[r * VC + dj[q]], xk[q] < VC ? sx[r * VC + xk[q]] : 1.f, acc[q]);
            }
        }
    }
    float* dst = partial + (long long)blockIdx.x * S;
    if (S <= 256) {
        red[threadIdx.x] = acc[0];
        __syncthreads();
        if (threadIdx.x < S) {
            float s = red[threadIdx.x];
            for (int l = 1; l < lanes; ++l) s += red[l * S + threadIdx.x];
            dst[threadIdx.x] = s;
        }
    } else {
#pragma unroll
        for (int q = 0; q < MAXQ; ++q)
            if (dj[q] >= 0) dst[s0 + 256 * q] = acc[q];
    }
}
// VM_FIN_SUMS sums x 16 block lanes per workgroup; the blocks of a lane, then the lanes, in float64 in a fixed order
__global__ __launch_bounds__(256) void view_mix_wgrad_finalize(const float* __restrict__ partial, long long nblk, float* __restrict__ dw,
                                                               float* __restrict__ db, int VC) {
    __shared__ double sh[16][VM_FIN_SUMS];
    const int S = VC * (VC + 1);
    const int sl = threadIdx.x % VM_FIN_SUMS, ln = threadIdx.x / VM_FIN_SUMS;
    const int s = blockIdx.x * VM_FIN_SUMS + sl;
    double a = 0;
    if (s < S)
        for (long long b = ln; b < nblk; b += 16) a += (double)partial[b * S + s];
    sh[ln][sl] = a;
    __syncthreads();
    if (ln == 0 && s < S) {
        for (int i = 1; i < 16; ++i) a += sh[i][sl];
        const int j = s / (VC + 1), k = s - j * (VC + 1);
        if (k < VC) dw[j * VC + k] = (float)a; else if (db) db[j] = (float)a;
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
typedef void (*vm_kernel_t)(VmIn, VmOut, const float*, const float*, long long, int);

template <int V, int C> constexpr vm_kernel_t vm_pick_c() { return (V * C <= VM_MAX_VC) ? &view_mix_kernel<(V * C <= VM_MAX_VC ? V : 1), C> : nullptr; }
template <int V> vm_kernel_t vm_pick_v(int c) {
    switch (c) {
        case 1: return vm_pick_c<V, 1>(); case 2: return vm_pick_c<V, 2>(); case 3: return vm_pick_c<V, 3>(); case 4: return vm_pick_c<V, 4>();
        case 5: return vm_pick_c<V, 5>(); case 6: return vm_pick_c<V, 6>(); case 7: return vm_pick_c<V, 7>(); case 8: return vm_pick_c<V, 8>();
        default: return nullptr;
    }
}
vm_kernel_t vm_pick(int v, int c) {
    switch (v) {
        case 1: return vm_pick_v<1>(c); case 2: return vm_pick_v<2>(c); case 3: return vm_pick_v<3>(c); case 4: return vm_pick_v<4>(c);
        case 5: return vm_pick_v<5>(c); case 6: return vm_pick_v<6>(c); case 7: return vm_pick_v<7>(c); case 8: return vm_pick_v<8>(c);
        default: return nullptr;
    }
}

inline long long vm_blocks(long long rows) { return (rows + VM_WGRAD_ROWS - 1) / VM_WGRAD_ROWS; }

int launch_view_mix(const float* const* ins, float* const* outs, const float* w, const float* bias, long long rows, int v, int c,
                    bool transposed, hipStream_t s, const char* what) {
    VmIn in; VmOut out;
    for (int j = 0; j < VM_MAX_V; ++j) { in.p[j] = ins[j < v ? j : 0]; out.p[j] = outs[j < v ? j : 0]; }
    const vm_kernel_t k = vm_pick(v, c);
    if (!k) return glf::fail(GLF_ERR_UNSUPPORTED, "%s: no kernel for v = %d, c = %d", what, v, c);
    const long long groups = rows / vm_group(c);
    hipLaunchKernelGGL(k, dim3(stream_grid(groups, 256)), dim3(256), 0, s, in, out, w, bias, rows, transposed ? 1 : 0);
    return glf::check_launch(what);
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
#define REQ_VM_SHAPE(what) \
    GLF_REQUIRE(rows > 0 && v > 0 && c > 0, GLF_ERR_BAD_SHAPE, what ": rows, v and c must be positive"); \
    GLF_REQUIRE(v <= VM_MAX_V && c <= VM_MAX_C && v * c <= VM_MAX_VC, GLF_ERR_UNSUPPORTED, \
                what ": the limit is c <= 8, V <= 8, V * c <= 40 (got V = %d, c = %d)", v, c)
#define REQ_VM_TABLE(what, tab) \
    for (int j = 0; j < v; ++j) GLF_REQUIRE((tab)[j] != nullptr && al16((tab)[j]), GLF_ERR_BAD_SHAPE, what ": every tensor of " #tab " must be non-null and 16-byte aligned")

extern "C" int glf_view_mix_fwd(const float* const* xs, const float* w, const float* bias, float* const* ys, int64_t rows, int v, int c,
                                glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(xs && w && ys, GLF_ERR_BAD_SHAPE, "view_mix_fwd: null argument");
    REQ_VM_SHAPE("view_mix_fwd");
    REQ_VM_TABLE("view_mix_fwd", xs);
    REQ_VM_TABLE("view_mix_fwd", ys);
    return launch_view_mix(xs, ys, w, bias, rows, v, c, false, glf::S(s), "view_mix_fwd");
}
extern "C" int glf_view_mix_dgrad(const float* const* dys, const float* w, float* const* dxs, int64_t rows, int v, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(dys && w && dxs, GLF_ERR_BAD_SHAPE, "view_mix_dgrad: null argument");
    REQ_VM_SHAPE("view_mix_dgrad");
    REQ_VM_TABLE("view_mix_dgrad", dys);
    REQ_VM_TABLE("view_mix_dgrad", dxs);
    return launch_view_mix(dys, dxs, w, nullptr, rows, v, c, true, glf::S(s), "view_mix_dgrad");
}
extern "C" size_t glf_view_mix_wgrad_workspace(int64_t rows, int v, int c) {
    if (rows <= 0 || v <= 0 || c <= 0 || v > VM_MAX_V || c > VM_MAX_C || v * c > VM_MAX_VC) return 0;
    return (size_t)vm_blocks(rows) * (size_t)(v * c) * (size_t)(v * c + 1) * sizeof(float);
}
extern "C" int glf_view_mix_wgrad(const float* const* xs, const float* const* dys, float* dw, float* db, void* workspace, size_t bytes,
                                  int64_t rows, int v, int c, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(xs && dys && dw && workspace, GLF_ERR_BAD_SHAPE, "view_mix_wgrad: null argument");
    REQ_VM_SHAPE("view_mix_wgrad");
    REQ_VM_TABLE("view_mix_wgrad", xs);
    REQ_VM_TABLE("view_mix_wgrad", dys);
    GLF_REQUIRE(bytes >= glf_view_mix_wgrad_workspace(rows, v, c), GLF_ERR_WORKSPACE, "view_mix_wgrad: workspace of %zu bytes, %zu needed",
                bytes, glf_view_mix_wgrad_workspace(rows, v, c));
    REQ_AL(workspace, "view_mix_wgrad: workspace");
    VmIn x, d;
    for (int j = 0; j < VM_MAX_V; ++j) { x.p[j] = xs[j < v ? j : 0]; d.p[j] = dys[j < v ? j : 0]; }
    const long long nblk = vm_blocks(rows);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(view_mix_wgrad_kernel, dim3((unsigned)nblk), dim3(256), 0, glf::S(s), x, d, partial, (long long)rows, v, c);
    if (int rc = glf::check_launch("view_mix_wgrad")) return rc;
    const int vc = v * c, sums = vc * (vc + 1);
    hipLaunchKernelGGL(view_mix_wgrad_finalize, dim3((sums + VM_FIN_SUMS - 1) / VM_FIN_SUMS), dim3(256), 0, glf::S(s), partial, nblk, dw, db, vc);
    return glf::check_launch("view_mix_wgrad");
}

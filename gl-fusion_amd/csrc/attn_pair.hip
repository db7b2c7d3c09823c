// Fused pairwise-ReLU attention of the fusion block's `concatenate` mode (reference models/ours.py:883-894, 898-900, 902):
//      s_ij = a_i + b_j + c          a = theta w_theta, b = phi w_phi: ONE scalar per position, c = the W_f bias
//      y_i  = (1 / L) sum_j relu(s_ij) g_j
// The reference concatenates theta_i and phi_j into an [N, 2 Ci, L, L] tensor and runs a 1 x 1 convolution over it; the
// score is the sum of two per-position scalars, so here nothing of size L x L is ever written: a 64 x 64 tile of
// relu(s) is computed on the VALU from 64 + 64 scalars, left in LDS and contracted with the g rows into MFMA accumulators.
//
// Backward, given dy:
//      dg_j = (1 / L) sum_i relu(s_ij) dy_i                          (PAIR_DG: the forward skeleton with the roles swapped)
//      t_ij = dy_i . g_j ;  ds_ij = t_ij [s_ij > 0] / L              (PAIR_DS: a score-type MFMA contraction over Ci)
//      da_i = sum_j ds_ij ;  db_j = sum_i ds_ij ;  dc = sum_ij ds_ij
// da is summed over the key blocks in their order inside the workgroup that owns the 64 query rows; db leaves every
// workgroup as one partial row per query block ([frames][ceil(L / 64)][L] floats of caller-owned workspace) that a second
// kernel adds in block order; dc is the sum of da in one workgroup, in a fixed order.  Every output element is written
// exactly once, no atomics, no zero fill: two runs are bitwise equal.
//
// Arithmetic: exact fp32 on v_mfma_f32_32x32x2_f32 under every contraction precision (the mask [s > 0] of the backward
// pass must be the one the forward pass applied: s is evaluated as (a_i + b_j) + c in fp32 in all three kernels).
// The skeleton (64-row outer blocks, tiles through LDS, 64 x Ci accumulators: attn_tile.h) is attn_softmax.hip's.
#include "attn_tile.h"

namespace {

enum PairMode { PAIR_FWD = 0, PAIR_DG = 1 };

struct PairArgs {
    const float* a; const float* b; const float* c;      // [frames * L], [frames * L], one device scalar
    const float* g; const float* dy;                     // rows of length ci, row strides ldg / lddy
    float* out;                                          // FWD: y (row stride ldo); DG: dg
    float* da; float* dbp;                               // DS: da [frames * L], db partials [frames][nblk][L]
    int L, ci;
    long long ldg, lddy, ldo;
    long long fg, fdy, fo;                               // frame strides (elements)
};

// FWD: outer = query rows i, inner = key rows j, acc_i += relu(s_ij) g_j.  DG: outer = key rows j, inner = query rows i,
// acc_j += relu(s_ij) dy_i.  The tile T[k = inner][m = outer] is the A operand of accumulate(); two tiles alternate, so one
// barrier per inner block orders both the writes of this block and the reads of the block before last.
template <int MODE>
__global__ __launch_bounds__(ANT, 1) void attn_pair_kernel(const PairArgs args) {
    const int L = args.L, nct = args.ci / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hl = lane >> 5, l31 = lane & 31;
    const int o0 = blockIdx.x * AT;
    const long long fr = blockIdx.y;
    const float* __restrict__ VO = (MODE == PAIR_FWD ? args.a : args.b) + fr * L;      // the outer rows' scalars
    const float* __restrict__ VI = (MODE == PAIR_FWD ? args.b : args.a) + fr * L;      // the inner rows' scalars
    const float* __restrict__ Z = MODE == PAIR_FWD ? args.g + fr * args.fg : args.dy + fr * args.fdy;
    const long long ldz = MODE == PAIR_FWD ? args.ldg : args.lddy;
    float* __restrict__ OUT = args.out + fr * args.fo;
    const float cc = *args.c;

    __shared__ float Ts[2][AT * ALD];

    f32x16 acc[2][A_MAXCT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < A_MAXCT; ++j) acc[i][j] = f32x16{0};

    // this thread fills column m (one outer row) of 16 tile rows: consecutive lanes, consecutive LDS words
    const int m = tid & 63, kg = tid >> 6;
    const bool o_ok = o0 + m < L;
    const float vo = VO[min(o0 + m, L - 1)];
    const int nblk = (L + AT - 1) / AT;
    for (int ib = 0; ib < nblk; ++ib) {
        const int i0 = ib * AT;
        float* T = Ts[ib & 1];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = 16 * kg + u;
            const float s = (vo + VI[min(i0 + k, L - 1)]) + cc;
            T[k * ALD + m] = (o_ok && i0 + k < L) ? fmaxf(s, 0.f) : 0.f;
        }
        __syncthreads();
        accumulate(acc, T, Z, ldz, i0, L, nct, wave, lane);
    }

    // epilogue: rows o0 + 32 i + (r & 3) + 8 (r >> 2) + 4 hl, columns 32 (wave + 4 jj) + l31; the 1 / L of the reference's
    // f / N is applied once, here
    const float scale = 1.f / (float)L;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = o0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hl;
            if (row < L) {
#pragma unroll
                for (int jj = 0; jj < A_MAXCT; ++jj) {
                    const int j = wave + 4 * jj;
                    if (j < nct) OUT[(long long)row * args.ldo + 32 * j + l31] = acc[i][jj][r] * scale;
                }
            }
        }
    }
}

// DS: a workgroup owns 64 query rows and walks the key blocks.  t = dY G^T over Ci (score_tile), ds = t [s > 0]; the tile is
// left in LDS as [q][key], thread q < 64 adds its row (da, carried across the key blocks), thread 64 + key adds its column
// (this query block's partial of db).
__global__ __launch_bounds__(ANT, 1) void attn_pair_ds_kernel(const PairArgs args) {
    const int L = args.L, ci = args.ci;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rt = wave >> 1, ct = wave & 1;
    const int hl = lane >> 5, l31 = lane & 31;
    const int o0 = blockIdx.x * AT;
    const long long fr = blockIdx.y;
    const float* __restrict__ A = args.a + fr * L;
    const float* __restrict__ B = args.b + fr * L;
    const float* __restrict__ G = args.g + fr * args.fg;
    const float* __restrict__ DY = args.dy + fr * args.fdy;
    const float cc = *args.c;
    const int nblk = (L + AT - 1) / AT;
    float* __restrict__ DBP = args.dbp + (fr * nblk + blockIdx.x) * L;

    __shared__ __attribute__((aligned(16))) float stg[4 * AKC * ALD];
    __shared__ float Ts[AT * ALD];
    __shared__ float As[AT];

    if (tid < AT) As[tid] = A[min(o0 + tid, L - 1)];
    float da = 0.f;
    for (int ib = 0; ib < nblk; ++ib) {
        const int i0 = ib * AT;
        // the first barrier inside score_tile() also orders As and the row / column sums of the previous block before Ts is rewritten
        const f32x16 t = score_tile(DY, args.lddy, o0, G, args.ldg, i0, L, ci, stg, tid, lane, rt, ct);
        const int key = i0 + 32 * ct + l31;
        const bool key_ok = key < L;
        const float bk = B[min(key, L - 1)];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ql = 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * hl;
            const float s = (As[ql] + bk) + cc;
            Ts[ql * ALD + 32 * ct + l31] = (key_ok && o0 + ql < L && s > 0.f) ? t[r] : 0.f;
        }
        __syncthreads();
        if (tid < AT) {
            float sum = 0.f;
#pragma unroll 16
            for (int k = 0; k < AT; ++k) sum += Ts[tid * ALD + k];
            da += sum;
        } else if (tid < 2 * AT) {
            const int col = tid - AT;
            float sum = 0.f;
#pragma unroll 16
            for (int q = 0; q < AT; ++q) sum += Ts[q * ALD + col];
            if (i0 + col < L) DBP[i0 + col] = sum;
        }
    }
    if (tid < AT && o0 + tid < L) args.da[fr * L + o0 + tid] = da / (float)L;
}

// db[fr][j] = (1 / L) sum over the query blocks, in block order, of their partial rows
__global__ __launch_bounds__(256) void attn_pair_db_kernel(const float* __restrict__ dbp, float* __restrict__ db, int frames, int L, int nblk) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)frames * L) return;
    const long long fr = i / L;
    const int j = (int)(i - fr * L);
    const float* p = dbp + fr * nblk * L + j;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += p[(long long)b * L];
    db[i] = s / (float)L;
}

// out[0] = sum of x[0 .. n): one workgroup, thread t adds x[t], x[t + 256], ... in double, then a fixed tree
__global__ __launch_bounds__(256) void attn_pair_total_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += (double)x[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)red[0];
}

// ---- the skinny ends of the mode: theta / phi [rows][Ci] against the two halves of the W_f row ------------------------------
// a[row] = theta[row] . w[0 .. ci), b[row] = phi[row] . w[ci .. 2 ci): one wavefront per row
__global__ __launch_bounds__(256) void pair_proj_fwd_kernel(const float* __restrict__ th, const float* __restrict__ ph, long long ld,
                                                            const float* __restrict__ w, float* __restrict__ a, float* __restrict__ b,
                                                            long long rows, int ci) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float sa = 0.f, sb = 0.f;
    for (int c = lane; c < ci; c += 64) {
        sa = fmaf(th[row * ld + c], w[c], sa);
        sb = fmaf(ph[row * ld + c], w[ci + c], sb);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o, 64);
        sb += __shfl_xor(sb, o, 64);
    }
    if (lane == 0) { a[row] = sa; b[row] = sb; }
}

constexpr int PP_ROWS = 256;      // rows per slab of the W_f gradient's first stage
// dtheta[row][c] = da[row] w[c], dphi[row][c] = db[row] w[ci + c], and the slab's partial of dw[c] = sum_row da[row] theta[row][c]
// (c < ci; phi / db for the second half).  Thread = one of the 2 ci columns, rows of the slab in order.
__global__ __launch_bounds__(256) void pair_proj_bwd_kernel(const float* __restrict__ th, const float* __restrict__ ph, long long ld,
                                                            const float* __restrict__ w, const float* __restrict__ da, const float* __restrict__ db,
                                                            float* __restrict__ dth, float* __restrict__ dph, long long ldd,
                                                            float* __restrict__ part, long long rows, int ci) {
    const int col = blockIdx.y * 256 + threadIdx.x;
    if (col >= 2 * ci) return;
    const bool second = col >= ci;
    const int c = second ? col - ci : col;
    const float* __restrict__ src = (second ? ph : th) + c;
    const float* __restrict__ d = second ? db : da;
    float* __restrict__ dst = (second ? dph : dth) + c;
    const float wc = w[col];
    const long long r0 = (long long)blockIdx.x * PP_ROWS;
    const long long r1 = r0 + PP_ROWS < rows ? r0 + PP_ROWS : rows;
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float dr = d[r];
        s = fmaf(dr, src[r * ld], s);
        dst[r * ldd] = dr * wc;
    }
    part[(long long)blockIdx.x * 2 * ci + col] = s;
}

// dw[col] = sum over the slabs, in slab order, in double
__global__ __launch_bounds__(256) void pair_proj_dw_kernel(const float* __restrict__ part, float* __restrict__ dw, int nslab, int cols) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    double s = 0.0;
    for (int b = 0; b < nslab; ++b) s += (double)part[(long long)b * cols + col];
    dw[col] = (float)s;
}

int pair_check(const glf_attn_pair_params* p, const void* a, const void* b, const void* c, const void* g) {
    GLF_REQUIRE(p && a && b && c && g, GLF_ERR_NULL, "attn_pair_relu: null argument");
    GLF_REQUIRE(p->frames > 0 && p->frames <= 65535 && p->L > 0, GLF_ERR_BAD_SHAPE, "attn_pair_relu: frames (%d) / L (%d) out of range", p->frames, p->L);
    GLF_REQUIRE(p->ci > 0 && p->ci % 32 == 0 && p->ci <= 32 * 4 * A_MAXCT, GLF_ERR_UNSUPPORTED,
                "attn_pair_relu: Ci must be a multiple of 32 and <= %d (got %d)", 32 * 4 * A_MAXCT, p->ci);
    GLF_REQUIRE(p->ldg >= p->ci, GLF_ERR_BAD_SHAPE, "attn_pair_relu: row stride of g < Ci");
    return GLF_OK;
}

PairArgs pair_args(const glf_attn_pair_params* p, const float* a, const float* b, const float* c, const float* g) {
    PairArgs x{};
    x.a = a; x.b = b; x.c = c; x.g = g;
    x.L = p->L; x.ci = p->ci;
    x.ldg = p->ldg; x.fg = (long long)p->L * p->ldg;
    return x;
}

}  // namespace

extern "C" size_t glf_sizeof_attn_pair_params(void) { return sizeof(glf_attn_pair_params); }

extern "C" size_t glf_attn_pair_relu_workspace_bytes(const glf_attn_pair_params* p) {
    if (!p || p->frames <= 0 || p->L <= 0) return 0;
    return (size_t)p->frames * (size_t)((p->L + AT - 1) / AT) * (size_t)p->L * sizeof(float);
}

extern "C" int glf_attn_pair_relu_fwd(const float* a, const float* b, const float* c, const float* g, float* y,
                                      const glf_attn_pair_params* p, glf_stream_t stream) {
    if (int rc = pair_check(p, a, b, c, g)) return rc;
    GLF_REQUIRE(y != nullptr, GLF_ERR_NULL, "attn_pair_relu_fwd: null argument");
    GLF_REQUIRE(p->ldy >= p->ci, GLF_ERR_BAD_SHAPE, "attn_pair_relu_fwd: ldy < Ci");
    if (int rc = glf::ensure_init()) return rc;
    PairArgs x = pair_args(p, a, b, c, g);
    x.out = y; x.ldo = p->ldy; x.fo = (long long)p->L * p->ldy;
    dim3 grid((p->L + AT - 1) / AT, p->frames);
    hipLaunchKernelGGL((attn_pair_kernel<PAIR_FWD>), grid, dim3(ANT), 0, glf::S(stream), x);
    return glf::check_launch("attn_pair_relu_fwd");
}

extern "C" int glf_attn_pair_relu_bwd(const float* a, const float* b, const float* c, const float* g, const float* dy, float* dg,
                                      float* da, float* db, float* dc, float* workspace, int64_t workspace_bytes,
                                      const glf_attn_pair_params* p, glf_stream_t stream) {
    if (int rc = pair_check(p, a, b, c, g)) return rc;
    GLF_REQUIRE(dy && dg && da && db && dc && workspace, GLF_ERR_NULL, "attn_pair_relu_bwd: null argument");
    GLF_REQUIRE(p->lddy >= p->ci && p->lddg >= p->ci, GLF_ERR_BAD_SHAPE, "attn_pair_relu_bwd: row stride of dy / dg < Ci");
    // the t = dY G^T tiles are staged with 16-byte loads
    GLF_REQUIRE(p->ldg % 4 == 0 && p->lddy % 4 == 0 && aligned16(g) && aligned16(dy), GLF_ERR_BAD_SHAPE,
                "attn_pair_relu_bwd: g / dy must be 16-byte aligned with row strides that are multiples of 4");
    GLF_REQUIRE(workspace_bytes >= (int64_t)glf_attn_pair_relu_workspace_bytes(p), GLF_ERR_WORKSPACE,
                "attn_pair_relu_bwd: workspace of %lld bytes, glf_attn_pair_relu_workspace_bytes() asks for %zu", (long long)workspace_bytes,
                glf_attn_pair_relu_workspace_bytes(p));
    if (int rc = glf::ensure_init()) return rc;
    PairArgs x = pair_args(p, a, b, c, g);
    x.dy = dy; x.lddy = p->lddy; x.fdy = (long long)p->L * p->lddy;
    x.out = dg; x.ldo = p->lddg; x.fo = (long long)p->L * p->lddg;
    x.da = da; x.dbp = workspace;
    const int nblk = (p->L + AT - 1) / AT;
    dim3 grid(nblk, p->frames);
    hipLaunchKernelGGL((attn_pair_kernel<PAIR_DG>), grid, dim3(ANT), 0, glf::S(stream), x);
    hipLaunchKernelGGL(attn_pair_ds_kernel, grid, dim3(ANT), 0, glf::S(stream), x);
    const long long rows = (long long)p->frames * p->L;
    hipLaunchKernelGGL(attn_pair_db_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, glf::S(stream), workspace, db, p->frames, p->L, nblk);
    hipLaunchKernelGGL(attn_pair_total_kernel, dim3(1), dim3(256), 0, glf::S(stream), da, rows, dc);
    return glf::check_launch("attn_pair_relu_bwd");
}

extern "C" size_t glf_attn_pair_proj_workspace_bytes(int64_t rows, int ci) {
    if (rows <= 0 || ci <= 0) return 0;
    return (size_t)((rows + PP_ROWS - 1) / PP_ROWS) * 2 * (size_t)ci * sizeof(float);
}

extern "C" int glf_attn_pair_proj_fwd(const float* theta, const float* phi, int64_t ld, const float* w, float* a, float* b, int64_t rows, int ci,
                                      glf_stream_t stream) {
    GLF_REQUIRE(theta && phi && w && a && b, GLF_ERR_NULL, "attn_pair_proj_fwd: null argument");
    GLF_REQUIRE(rows > 0 && rows < (1LL << 33) && ci > 0 && ld >= ci, GLF_ERR_BAD_SHAPE, "attn_pair_proj_fwd: bad shape");
    if (int rc = glf::ensure_init()) return rc;
    hipLaunchKernelGGL(pair_proj_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, glf::S(stream), theta, phi, (long long)ld, w, a, b,
                       (long long)rows, ci);
    return glf::check_launch("attn_pair_proj_fwd");
}

extern "C" int glf_attn_pair_proj_bwd(const float* theta, const float* phi, int64_t ld, const float* w, const float* da, const float* db,
                                      float* dtheta, float* dphi, int64_t ldd, float* dw, float* workspace, int64_t workspace_bytes, int64_t rows,
                                      int ci, glf_stream_t stream) {
    GLF_REQUIRE(theta && phi && w && da && db && dtheta && dphi && dw && workspace, GLF_ERR_NULL, "attn_pair_proj_bwd: null argument");
    GLF_REQUIRE(rows > 0 && ci > 0 && ld >= ci && ldd >= ci, GLF_ERR_BAD_SHAPE, "attn_pair_proj_bwd: bad shape");
    const long long nslab = (rows + PP_ROWS - 1) / PP_ROWS;
    GLF_REQUIRE(nslab < 2147483647LL && (2 * ci + 255) / 256 <= 65535, GLF_ERR_BAD_SHAPE, "attn_pair_proj_bwd: rows / Ci out of range");
    GLF_REQUIRE(workspace_bytes >= (int64_t)glf_attn_pair_proj_workspace_bytes(rows, ci), GLF_ERR_WORKSPACE,
                "attn_pair_proj_bwd: workspace of %lld bytes, glf_attn_pair_proj_workspace_bytes() asks for %zu", (long long)workspace_bytes,
                glf_attn_pair_proj_workspace_bytes(rows, ci));
    if (int rc = glf::ensure_init()) return rc;
    hipLaunchKernelGGL(pair_proj_bwd_kernel, dim3((unsigned)nslab, (2 * ci + 255) / 256), dim3(256), 0, glf::S(stream), theta, phi, (long long)ld, w,
                       da, db, dtheta, dphi, (long long)ldd, workspace, (long long)rows, ci);
    hipLaunchKernelGGL(pair_proj_dw_kernel, dim3((2 * ci + 255) / 256), dim3(256), 0, glf::S(stream), workspace, dw, (int)nslab, 2 * ci);
    return glf::check_launch("attn_pair_proj_bwd");
}

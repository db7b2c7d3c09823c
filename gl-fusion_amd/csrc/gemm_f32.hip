// Implicit-GEMM contraction engine for the GL-Fusion hot path on MI355X (gfx950 / CDNA4).
//
//   * fp32 in / fp32 accumulate on the matrix cores: v_mfma_f32_32x32x2_f32 (exact f32,
//     64 cycles/SIMD, 157 TF chip peak).  One wave owns a 64x64 output tile = 2x2 MFMA tiles
//     (64 accumulator VGPRs); a 256-thread workgroup owns 128x128; K is walked 32 deep.
//   * NHWC, im2col-free: the A rows of a K-tile are gathered straight from the activation
//     tensor with the (tap, stride, pad, dilation) mapping; taps that are out of range for a
//     whole 128-row tile are skipped (ASPP rate 12/24/36 on a 28x28 map is mostly padding).
//   * Operands are staged global -> registers -> LDS (issue-early / write-late, one barrier per
//     K-tile, two LDS buffers).  LDS tiles are k-major ([k][m]) so that every MFMA operand read
//     is a conflict-free ds_read_b32 of 32 consecutive floats; k-contiguous sources are
//     transposed on the way in (row stride 129: conflict-free ds_write_b32), row-contiguous
//     sources go in with ds_write_b128 (row stride 132).
//   * blockIdx -> tile mapping is XCD-aware (8 XCDs, private L2s): each XCD walks a contiguous
//     range of tiles that share A rows.
//
// Three kernels share the MFMA core:
//   gemm_rows_kernel<0>  A[m][k] (gathered rows) x B[n][k]   -> conv forward, 1x1 / linear
//   gemm_rows_kernel<1>  A[m][k] (gathered rows) x B[k][n]   -> conv dgrad, y = theta @ M
//   gemm_tn_kernel       sum_r A[r][m] * B[src(r)][n]        -> conv wgrad, M = phi^T g
#include "gemm_rows_walk.h"
#include "gemm_tn_walk.h"

namespace {

// 64x64 per wave, K = 32 from LDS tiles laid out [k][m] / [k][n].
//  * Two-level accumulation: the 32-deep K-tile is summed by the MFMA chain into fresh accumulators
//    (C = 0), which are then added to the running sums on the VALU.  A single f32 fma chain over
//    K = 9*2048 products has a ~sqrt(K) rounding walk; chains of 32 + K/32 keep the contraction at the
//    accuracy of a blocked CPU GEMM.
//  * The MFMA pipe (64 cycles per instruction) is the roof, so everything else is issued in its shadow:
//    operand ds_reads run one k-step ahead (double-buffered registers); `mid(p)`, p = 0..7, is called
//    between k-steps 4..11 and stages 1/8 of the NEXT K-tile into the other LDS buffer; the last four
//    k-steps run accumulator-major so that the c += t adds of three accumulators overlap the MFMAs of
//    the next one.
// Written as a macro (not a function taking a closure): nested lambdas that capture the staging registers by
// reference made hipcc materialise the closures -- and everything they point to -- in scratch memory.
// MID(pc) is a statement macro of the enclosing kernel; pc is a compile-time constant after unrolling.
#define GLF_LD(x) (x)
// MID(q), q = 0..11, is called after the MFMAs of head k-step q (HEAD_ = 12).
#define GLF_MMA_KTILE(LDA_, LDB_, a_s, b_s, MID)                                                              \
    {                                                                                                         \
        constexpr int NS_ = BK / 2, HEAD_ = NS_ - 4;                                                          \
        f32x16 t00 = {0}, t01 = {0}, t10 = {0}, t11 = {0};                                                    \
        float a0_[2], a1_[2], b0_[2], b1_[2];                                                                 \
        float ta0_[4], ta1_[4], tb0_[4], tb1_[4];                                                             \
        a0_[0] = GLF_LD((a_s)[0]); a1_[0] = GLF_LD((a_s)[32]); b0_[0] = GLF_LD((b_s)[0]); b1_[0] = GLF_LD((b_s)[32]); \
        _Pragma("unroll") for (int st = 0; st < HEAD_; ++st) {                                                \
            const int cur = st & 1, nxt = cur ^ 1;                                                            \
            if (st + 1 < HEAD_) {                                                                             \
                a0_[nxt] = GLF_LD((a_s)[(2 * st + 2) * LDA_]); a1_[nxt] = GLF_LD((a_s)[(2 * st + 2) * LDA_ + 32]); \
                b0_[nxt] = GLF_LD((b_s)[(2 * st + 2) * LDB_]); b1_[nxt] = GLF_LD((b_s)[(2 * st + 2) * LDB_ + 32]); \
            } else {                                                                                          \
                _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                               \
                    ta0_[q] = GLF_LD((a_s)[(2 * (HEAD_ + q)) * LDA_]); ta1_[q] = GLF_LD((a_s)[(2 * (HEAD_ + q)) * LDA_ + 32]); \
                    tb0_[q] = GLF_LD((b_s)[(2 * (HEAD_ + q)) * LDB_]); tb1_[q] = GLF_LD((b_s)[(2 * (HEAD_ + q)) * LDB_ + 32]); \
                }                                                                                             \
            }                                                                                                 \
            __builtin_amdgcn_sched_barrier(0); /* keep the prefetch ahead of this step's MFMAs */             \
            t00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0_[cur], b0_[cur], t00, 0, 0, 0);                     \
            t01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0_[cur], b1_[cur], t01, 0, 0, 0);                     \
            t10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1_[cur], b0_[cur], t10, 0, 0, 0);                     \
            t11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1_[cur], b1_[cur], t11, 0, 0, 0);                     \
            { MID(st) }                                                                                       \
        }                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) t00 = __builtin_amdgcn_mfma_f32_32x32x2f32(ta0_[q], tb0_[q], t00, 0, 0, 0); \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) t01 = __builtin_amdgcn_mfma_f32_32x32x2f32(ta0_[q], tb1_[q], t01, 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        c00 += t00;                                                                                           \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) t10 = __builtin_amdgcn_mfma_f32_32x32x2f32(ta1_[q], tb0_[q], t10, 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        c01 += t01;                                                                                           \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) t11 = __builtin_amdgcn_mfma_f32_32x32x2f32(ta1_[q], tb1_[q], t11, 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        c10 += t10;                                                                                           \
        c11 += t11;                                                                                           \
    }

__device__ __forceinline__ void scatter4(float* dst, int ld, const float4& v) {
    dst[0] = v.x; dst[ld] = v.y; dst[2 * ld] = v.z; dst[3 * ld] = v.w;
}

// ----------------------------------------------------------------------------------------
// rows kernel: C[m][n] = alpha * sum_tap sum_k A[src(m,tap)][k] * B_tap(k,n) + bias[n]
// BMODE 0: B_tap[n][k]; BMODE 1: B_tap[k][n]
// ----------------------------------------------------------------------------------------
template <int BMODE, bool GATHER>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_rows_kernel(const GemmArgs args) {
    // ---- scalar copies of the launch arguments (see GeoS) ----
    const int pM = args.M, pN = args.N, pK = args.K, p_lda = args.lda, p_ldb = args.ldb, p_ldc = args.ldc;
    const int p_taps = args.taps, p_gather = args.gather, p_accumulate = args.accumulate;
    const int p_tiles_n = args.tiles_n, p_vec_a = args.vec_a, p_vec_b = args.vec_b;
    const unsigned p_tap_mask = args.tap_mask;
    const long long p_tsb = args.tap_stride_b, p_bsa = args.bsa, p_bsb = args.bsb, p_bsc = args.bsc;
    const float p_alpha = args.alpha;
    const float* __restrict__ p_A = args.A; const float* __restrict__ p_B = args.B; const float* __restrict__ p_bias = args.bias;
    float* __restrict__ p_C = args.C;
    const RowsGeo G{p_gather, args.g.n_img, args.g.hs, args.g.ws, args.g.hd, args.g.wd, args.g.kw, args.g.stride, args.g.pad, args.g.dil};
    const int p_rect = GATHER ? args.rect : 0;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LDA = LD_T;
    constexpr int LDB = (BMODE == 0) ? LD_T : LD_V;
    constexpr int A_SZ = BK * LDA, B_SZ = BK * LDB;
    float* As = smem;
    float* Bs = smem + 2 * A_SZ;
    unsigned* s_mask = reinterpret_cast<unsigned*>(smem + 2 * A_SZ + 2 * B_SZ);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    int tn;
    RowTile rt{0, pM, 0, 0, G.hd, G.wd, p_tap_mask};    // rect mode: rows and pixels of its tap's rectangle
    rows_tile_order(0, p_tiles_n, tn, rt.tm);
    if (p_rect) rows_locate<BM, false>(1, p_tap_mask, G, rt);
    unsigned mask = rt.mask;
    const int bz = blockIdx.z;
    const float* __restrict__ A = p_A + (long long)bz * p_bsa;
    const float* __restrict__ B = p_B + (long long)bz * p_bsb;
    float* __restrict__ C = p_C + (long long)bz * p_bsc;

    const int ac = tid & 7, ar = tid >> 3;          // k-contiguous staging: 8 float4 per 32-deep row
    const int bc = tid & 31, br = tid >> 5;         // row-contiguous staging (BMODE 1)

    // Fast path (block-uniform): every float4 is in range and 16-byte aligned, so the eight loads of a tile are
    // issued unconditionally from clamped addresses; rows that are padding / out of range are zeroed by a
    // select when the registers are written to LDS (store_piece), i.e. AFTER the loads' latency has been
    // hidden under MFMAs -- a select at load time would make the wave wait for the data right there.  Loads inside per-lane
    // branches make hipcc wait vmcnt(0) at every merge -- eight serialised L2 round trips per K-tile, measured
    // as a 20 % loss on the whole kernel.
    const bool vec_a = p_vec_a, vec_b = p_vec_b;
    const bool fast = vec_a && vec_b && (pK % BK) == 0 && (BMODE == 0 || (pN % 4) == 0);

    RowState<4> rows;                               // rows ar + 32 j of the tile
    rows_init<4, 32, GATHER>(rows, rt.tm * BM + ar, rt, p_lda, G.hd, G.wd);
    const bool fastg = GATHER && rows_fast_gather(G);
    if (fastg) rows_to_fast(rows, G);
    rows_census<BM, 4, GATHER>(rows, mask, fastg, ac == 0, p_taps, p_rect, G, s_mask);

    const int nkc = (pK + BK - 1) / BK;
    const int ntiles = __popc(mask) * nkc;

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};

    float4 ra[4], rb[4];
    unsigned rem_mask = mask;
    int tap = -1, kc = nkc;          // "before the first tile"

    // Both paths take the row pointers of a tap from the shared tap change: pa[j] = float4 #ac of row j's first K-tile, from a
    // clamped address (A's row 0) where the row is padding / out of range; a_ok says which rows are real.
    const float* pa[4];
    const float* pb[4];
    unsigned a_ok = 0;
    const int a_col[4] = {4 * ac, 4 * ac, 4 * ac, 4 * ac};
    auto advance = [&]() __attribute__((always_inline)) {
        if (++kc >= nkc) {
            kc = 0;
            tap = rows_next_tap<4, GATHER>(rows, rem_mask, pa, A, A, p_lda, fastg, G, a_col, &a_ok);
        }
    };
    auto load_tile = [&]() __attribute__((always_inline)) {
        const int kbase = kc * BK + 4 * ac;
        const float* Bt = B + (long long)tap * p_tsb;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            ra[j] = ((a_ok >> j) & 1u) ? ld4(pa[j] + kc * BK, pK - kbase, vec_a) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (BMODE == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = tn * BN + ar + 32 * j;
                rb[j] = (n < pN) ? ld4(Bt + (long long)n * p_ldb + kbase, pK - kbase, vec_b) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            const int n0 = tn * BN + 4 * bc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kc * BK + br + 8 * j;
                rb[j] = (k < pK) ? ld4(Bt + (long long)k * p_ldb + n0, pN - n0, vec_b) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    // piece p of the staged tile -> LDS (p < 4: A float4 #p, else B float4 #(p-4)); static indices only
    // constant array indices only (a lambda parameter index sends ra/rb/a_off to scratch: 3x slower)
#define GLF_SP_A(J)                                                                          \
    {                                                                                        \
        const float4 v = ra[J];                                                              \
        scatter4(As + buf * A_SZ + (4 * ac) * LDA + ar + 32 * J, LDA, v);                    \
    }
#define GLF_SP_B(J)                                                                          \
    {                                                                                        \
        if (BMODE == 0) {                                                                    \
            const float4 v = rb[J];                                                          \
            scatter4(Bs + buf * B_SZ + (4 * ac) * LDB + ar + 32 * J, LDB, v);                \
        } else {                                                                             \
            const float4 v = rb[J];                                                          \
            *reinterpret_cast<float4*>(Bs + buf * B_SZ + (br + 8 * J) * LDB + 4 * bc) = v;   \
        }                                                                                    \
    }
#define GLF_SP(pc)                       \
    switch (pc) {                        \
        case 0: GLF_SP_A(0) break;       \
        case 1: GLF_SP_A(1) break;       \
        case 2: GLF_SP_A(2) break;       \
        case 3: GLF_SP_A(3) break;       \
        case 4: GLF_SP_B(0) break;       \
        case 5: GLF_SP_B(1) break;       \
        case 6: GLF_SP_B(2) break;       \
        default: GLF_SP_B(3) break;      \
    }
#define GLF_SP_NEXT(q) if (has_next && (q) >= 4) { GLF_SP((q) - 4) }

    // ---- fast path state: per-thread source pointers advanced incrementally (no per-tile address maths) ----
    const long long b_step = (BMODE == 0) ? (long long)BK : (long long)BK * p_ldb;
    auto advance_fast = [&]() __attribute__((always_inline)) {
        if (++kc >= nkc) {
            kc = 0;
            tap = rows_next_tap<4, GATHER>(rows, rem_mask, pa, A, A, p_lda, fastg, G, a_col, &a_ok);
            const float* Bt = B + (long long)tap * p_tsb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (BMODE == 0) pb[j] = Bt + (long long)min(tn * BN + ar + 32 * j, pN - 1) * p_ldb + 4 * ac;
                else pb[j] = Bt + (long long)(br + 8 * j) * p_ldb + min(tn * BN + 4 * bc, pN - 4);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { pa[j] += BK; pb[j] += b_step; }
        }
    };
#define GLF_FLP(pc)                                                                         \
    switch (pc) {                                                                           \
        case 0: ra[0] = *reinterpret_cast<const float4*>(pa[0]); break;                     \
        case 1: ra[1] = *reinterpret_cast<const float4*>(pa[1]); break;                     \
        case 2: ra[2] = *reinterpret_cast<const float4*>(pa[2]); break;                     \
        case 3: ra[3] = *reinterpret_cast<const float4*>(pa[3]); break;                     \
        case 4: rb[0] = *reinterpret_cast<const float4*>(pb[0]); break;                     \
        case 5: rb[1] = *reinterpret_cast<const float4*>(pb[1]); break;                     \
        case 6: rb[2] = *reinterpret_cast<const float4*>(pb[2]); break;                     \
        default: rb[3] = *reinterpret_cast<const float4*>(pb[3]); break;                    \
    }
#define GLF_FSP_A(J) scatter4(As + buf * A_SZ + (4 * ac) * LDA + ar + 32 * J, LDA, keep_if((a_ok >> J) & 1u, ra[J]));
#define GLF_FSP_B(J)                                                                                          \
    {                                                                                                         \
        if (BMODE == 0) scatter4(Bs + buf * B_SZ + (4 * ac) * LDB + ar + 32 * J, LDB, keep_if(tn * BN + ar + 32 * J < pN, rb[J])); \
        else *reinterpret_cast<float4*>(Bs + buf * B_SZ + (br + 8 * J) * LDB + 4 * bc) = keep_if(tn * BN + 4 * bc < pN, rb[J]);    \
    }
#define GLF_FSP(pc)                      \
    switch (pc) {                        \
        case 0: GLF_FSP_A(0) break;      \
        case 1: GLF_FSP_A(1) break;      \
        case 2: GLF_FSP_A(2) break;      \
        case 3: GLF_FSP_A(3) break;      \
        case 4: GLF_FSP_B(0) break;      \
        case 5: GLF_FSP_B(1) break;      \
        case 6: GLF_FSP_B(2) break;      \
        default: GLF_FSP_B(3) break;     \
    }
    // k-steps 0..3 issue the eight loads of the next tile (two per step), k-steps 4..11 write them to LDS
#define GLF_FAST_MID(q)                                                       \
    if (has_next) {                                                           \
        if ((q) < 4) { GLF_FLP(2 * (q)) GLF_FLP(2 * (q) + 1) }                \
        else { GLF_FSP((q) - 4) }                                             \
    }

    if (ntiles > 0) {
        const int a_lane = (lane >> 5) * LDA + wm + (lane & 31);
        const int b_lane = (lane >> 5) * LDB + wn + (lane & 31);
        if (fast) {
            advance_fast();
            {
                const int buf = 0;
#pragma unroll
                for (int pc = 0; pc < 8; ++pc) { GLF_FLP(pc) }
#pragma unroll
                for (int pc = 0; pc < 8; ++pc) { GLF_FSP(pc) }
            }
            __syncthreads();
            for (int it = 0; it < ntiles; ++it) {
                const bool has_next = (it + 1) < ntiles;
                if (has_next) advance_fast();
                const float* a_sp = As + (it & 1) * A_SZ + a_lane;
                const float* b_sp = Bs + (it & 1) * B_SZ + b_lane;
                const int buf = (it & 1) ^ 1;      // the staging macros write the OTHER buffer (free since the last barrier)
                GLF_MMA_KTILE(LDA, LDB, a_sp, b_sp, GLF_FAST_MID)
                __syncthreads();
            }
        } else {
            advance();
            load_tile();
            {
                const int buf = 0;
#pragma unroll
                for (int pc = 0; pc < 8; ++pc) { GLF_SP(pc) }
            }
            __syncthreads();
            for (int it = 0; it < ntiles; ++it) {
                const bool has_next = (it + 1) < ntiles;
                if (has_next) { advance(); load_tile(); }
                const float* a_sp = As + (it & 1) * A_SZ + a_lane;
                const float* b_sp = Bs + (it & 1) * B_SZ + b_lane;
                const int buf = (it & 1) ^ 1;
                GLF_MMA_KTILE(LDA, LDB, a_sp, b_sp, GLF_SP_NEXT)
                __syncthreads();
            }
        }
    }

    const RowsOut out{C, p_bias, nullptr, nullptr, nullptr, nullptr, 0, p_bsc, pN, p_ldc, p_accumulate, p_rect, 0, tn, G.hd, G.wd, p_alpha};
    rows_plain_epilogue<BM>(out, rt, c00, c01, c10, c11);
}

// ----------------------------------------------------------------------------------------
// TN kernel: C_tap[m][n] (+)= alpha * sum_{r in slice} A[r][m] * B[src(r,tap)][n]
// grid: x = tiles_m*tiles_n, y = active taps, z = batch*split
// ----------------------------------------------------------------------------------------
template <bool GATHER>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_kernel(const GemmArgs args) {
    // ---- scalar copies of the launch arguments (see GeoS) ----
    const int pM = args.M, pN = args.N, pK = args.K, p_lda = args.lda, p_ldb = args.ldb, p_ldc = args.ldc;
    const int p_accumulate = args.accumulate, p_split = args.split;
    const int p_tiles_n = args.tiles_n, p_vec_a = args.vec_a, p_vec_b = args.vec_b;
    const unsigned p_tap_mask = args.tap_mask;
    const long long p_tsb = args.tap_stride_b, p_bsa = args.bsa, p_bsb = args.bsb, p_bsc = args.bsc;
    const float p_alpha = args.alpha;
    const float* __restrict__ p_A = args.A; const float* __restrict__ p_B = args.B;
    float* __restrict__ p_C = args.C;
    const int g_hs = args.g.hs, g_ws = args.g.ws, g_hd = args.g.hd, g_wd = args.g.wd, g_kw = args.g.kw;
    const int g_stride = args.g.stride, g_pad = args.g.pad, g_dil = args.g.dil;
    const int g_nimg = args.g.n_img, p_rect = GATHER ? args.rect : 0;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LD = LD_V;
    constexpr int T_SZ = BK * LD;
    float* As = smem;
    float* Bs = smem + 2 * T_SZ;
    int* vflag = reinterpret_cast<int*>(smem + 4 * T_SZ);      // [2][32] row-valid flags

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = bid % p_tiles_n, tm = bid / p_tiles_n;
    const int tap = tn_tap(p_tap_mask, blockIdx.y);
    // rect mode: the reduction runs over this tap's rectangle of output pixels only (see tap_rect)
    TnSlice ts;
    if (!tn_slice<BK, false>(ts, blockIdx.z, p_split, pK, p_rect, tap, Geo{g_nimg, g_hs, g_ws, g_hd, g_wd, 0, g_kw, g_stride, g_pad, g_dil})) return;
    const int r_y0 = ts.y0, r_x0 = ts.x0, r_w = ts.w, r0 = ts.r0, r1 = ts.r1;
    const float* __restrict__ A = p_A + (long long)ts.bz * p_bsa;
    const float* __restrict__ B = p_B + (long long)ts.bz * p_bsb;

    const int c4 = tid & 31, rr = tid >> 5;
    const int m0 = tm * BM + 4 * c4, n0 = tn * BN + 4 * c4;
    const bool vec_a = p_vec_a, vec_b = p_vec_b;
    const int hw = GATHER ? ts.h * r_w : 1;

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    float4 ra[4], rb[4];
    int rvalid[4];

    const bool fast = vec_a && vec_b && (pM % 4) == 0 && (pN % 4) == 0;
    const int m0c = min(m0, pM - 4), n0c = min(n0, pN - 4);
    auto load_tile = [&](int rbase) __attribute__((always_inline)) {
        long long src[4], arow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = rbase + rr + 8 * j;
            src[j] = -1;
            arow[j] = min(r, r1 - 1);
            if (GATHER) {
                const int rc = min(r, r1 - 1);
                const int n = rc / hw, rem = rc - n * hw;
                const int yy = rem / r_w;
                const int y = r_y0 + yy, x = r_x0 + rem - yy * r_w;
                arow[j] = ((long long)n * g_hd + y) * g_wd + x;
                if (r < r1) src[j] = map_src(g_hs, g_ws, g_kw, g_stride, g_pad, g_dil, 1, n, y, x, tap);
            } else if (r < r1) {
                src[j] = r;
            }
            rvalid[j] = src[j] >= 0;
        }
        if (fast) {          // unconditional loads from clamped addresses + select (see gemm_rows_kernel)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 va = *reinterpret_cast<const float4*>(A + arow[j] * p_lda + m0c);
                const float4 vb = *reinterpret_cast<const float4*>(B + (src[j] >= 0 ? src[j] : 0) * p_ldb + n0c);
                ra[j] = va;                  // zeroed at store time (rvalid / column range), not here
                rb[j] = vb;
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (src[j] >= 0) {
                ra[j] = ld4(A + arow[j] * p_lda + m0, pM - m0, vec_a);
                rb[j] = ld4(B + src[j] * p_ldb + n0, pN - n0, vec_b);
            } else {
                ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
#define GLF_TP_A(J)                                                                          \
    {                                                                                        \
        const float4 v = keep_if(!fast || (rvalid[J] && m0 < pM), ra[J]);                 \
        *reinterpret_cast<float4*>(As + buf * T_SZ + (rr + 8 * J) * LD + 4 * c4) = v;        \
        if (c4 == 0) vflag[buf * 32 + rr + 8 * J] = rvalid[J];                               \
    }
#define GLF_TP_B(J)                                                                          \
    {                                                                                        \
        const float4 v = keep_if(!fast || (rvalid[J] && n0 < pN), rb[J]);                 \
        *reinterpret_cast<float4*>(Bs + buf * T_SZ + (rr + 8 * J) * LD + 4 * c4) = v;        \
    }
#define GLF_TP(pc)                       \
    switch (pc) {                        \
        case 0: GLF_TP_A(0) break;       \
        case 1: GLF_TP_A(1) break;       \
        case 2: GLF_TP_A(2) break;       \
        case 3: GLF_TP_A(3) break;       \
        case 4: GLF_TP_B(0) break;       \
        case 5: GLF_TP_B(1) break;       \
        case 6: GLF_TP_B(2) break;       \
        default: GLF_TP_B(3) break;      \
    }
#define GLF_TP_NEXT(q) if (has_next && (q) >= 4) { GLF_TP((q) - 4) }

    load_tile(r0);
    {
        const int buf = 0;
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) { GLF_TP(pc) }
    }
    __syncthreads();
    const int a_lane = (lane >> 5) * LD + wm + (lane & 31);
    const int b_lane = (lane >> 5) * LD + wn + (lane & 31);
    int it = 0;
    for (int rbase = r0; rbase < r1; rbase += BK, ++it) {
        const int buf = it & 1;
        const bool has_next = (rbase + BK) < r1;
        if (has_next) load_tile(rbase + BK);
        // all 32 rows of this K-tile in the padding (dilated taps): nothing to add
        const bool any = __ballot(vflag[buf * 32 + (lane & 31)] != 0) != 0ull;
        {
            const float* a_sp = As + buf * T_SZ + a_lane;
            const float* b_sp = Bs + buf * T_SZ + b_lane;
            const int cbuf = buf;
            const int buf = cbuf ^ 1;              // GLF_TP writes the OTHER buffer
            if (any) {
                GLF_MMA_KTILE(LD, LD, a_sp, b_sp, GLF_TP_NEXT)
            } else if (has_next) {
#pragma unroll
                for (int pc = 0; pc < 8; ++pc) { GLF_TP(pc) }
            }
        }
        __syncthreads();
    }

    const TnOut out = tn_out(args.partial, p_C, nullptr, pM, pN, p_ldc, p_bsc, p_tsb, ts.bz, tap, p_split, p_accumulate, tm, tn, p_alpha);
    float cmax = 0.f;                      // (no amax_c in this kernel: never read, the compiler drops the maxima)
    tn_emit<BM, BN>(out, c00, wm, wn, cmax); tn_emit<BM, BN>(out, c01, wm, wn + 32, cmax);
    tn_emit<BM, BN>(out, c10, wm + 32, wn, cmax); tn_emit<BM, BN>(out, c11, wm + 32, wn + 32, cmax);
}

// ----------------------------------------------------------------------------------------
// second stage of the two-stage split-K reduction of glf_gemm_tn: C_tap = (accumulate ? C_tap : 0) + sum over the valid
// slices of their partial slabs, in slice order (bitwise reproducible; tn_sum_slabs).  grid: x over M*N, y = kept-tap ordinal,
// z = batch.  vec = 0: the scalar fallback (N, ldc or C not 4-element aligned).
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ partial, float* __restrict__ Cb, int M, int N, int ldc,
                                                        long long tsb, long long bsc, int split, unsigned tap_mask, int accumulate,
                                                        int K, int rect, Geo g, int vec, float* __restrict__ amax_c) {
    const int tap = tn_tap(tap_mask, blockIdx.y), ntap = gridDim.y, bz = blockIdx.z;
    const int nvalid = tn_valid_slices(tn_tap_row_count<false>(rect, tap, K, g), K, split, BK);
    const long long mn = (long long)M * N;
    const float* __restrict__ src = tn_slab(partial, bz * split, ntap, blockIdx.y, mn);
    const long long slice_stride = (long long)ntap * mn;
    float* __restrict__ C = Cb + (long long)bz * bsc + (long long)tap * tsb;
    float cmax = 0.f;
    if (vec) {
        const int n4 = N >> 2;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)M * n4; i += (long long)gridDim.x * blockDim.x) {
            const long long row = i / n4;
            const int c4 = (int)(i - row * n4) * 4;
            float* dst = C + row * ldc + c4;
            const float4 acc = tn_sum_slabs<1, false>(src + row * N + c4, slice_stride, nvalid, true, accumulate,
                                                      [&] { return *reinterpret_cast<const float4*>(dst); }, nullptr);
            *reinterpret_cast<float4*>(dst) = acc;
            cmax = amax4(cmax, acc);
        }
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < mn; i += (long long)gridDim.x * blockDim.x) {
            const long long row = i / N;
            const int col = (int)(i - row * N);
            float* dst = C + row * ldc + col;
            double accd = accumulate ? (double)*dst : 0.0;
            for (int sl = 0; sl < nvalid; ++sl) accd += src[sl * slice_stride + i];
            const float acc = (float)accd;
            *dst = acc;
            cmax = fmaxf(cmax, fabsf(acc));
        }
    }
    tn_amax<false>(amax_c, cmax);
}

// the vector form with SL = 4 / 16 slice lanes per output
template <int SL>
__global__ __launch_bounds__(256) void tn_reduce_lanes_kernel(const float* __restrict__ partial, float* __restrict__ Cb, int M, int N, int ldc,
                                                              long long tsb, long long bsc, int split, unsigned tap_mask, int accumulate,
                                                              int K, int rect, Geo g, float* __restrict__ amax_c) {
    constexpr int OG = 256 / SL;
    __shared__ double sh[4][256];
    const int tap = tn_tap(tap_mask, blockIdx.y), ntap = gridDim.y, bz = blockIdx.z;
    const int nvalid = tn_valid_slices(tn_tap_row_count<false>(rect, tap, K, g), K, split, BK);
    const long long mn = (long long)M * N;
    const float* __restrict__ src = tn_slab(partial, bz * split, ntap, blockIdx.y, mn);
    const long long slice_stride = (long long)ntap * mn;
    float* __restrict__ C = Cb + (long long)bz * bsc + (long long)tap * tsb;
    const int n4 = N >> 2;
    const long long total = (long long)M * n4;
    const int ol = threadIdx.x % OG, sl = threadIdx.x / OG;
    float cmax = 0.f;
    for (long long base = (long long)blockIdx.x * OG; base < total; base += (long long)gridDim.x * OG) {
        const long long i = base + ol;
        const bool live = i < total;
        const long long row = live ? i / n4 : 0;
        const int c4 = (int)((live ? i : 0) - row * n4) * 4;
        float* dst = C + row * ldc + c4;
        const float4 acc = tn_sum_slabs<SL>(src + row * N + c4, slice_stride, nvalid, live, accumulate,
                                            [&] { return *reinterpret_cast<const float4*>(dst); }, sh);
        if (sl == 0 && live) {
            *reinterpret_cast<float4*>(dst) = acc;
            cmax = amax4(cmax, acc);
        }
    }
    tn_amax<false>(amax_c, cmax);
}

// The second stage storing the PARAMETER layout (glf_gemm_params.c_oihw): out[m][n][tap], the taps of an output element side by
// side, so that a k x k weight's gradient needs neither the tap-major intermediate nor the pass that re-lays it out.  A workgroup
// owns 4 * OG consecutive elements of the [M][N] plane (OG = 256 / SL float4 groups, SL slice lanes per group) for ALL taps.  It
// sums tap after tap with tn_sum_slabs, as the two kernels above do, into an LDS tile laid out as the destination is, and stores
// the tile's 4 * OG * taps floats as one contiguous run of float4 (144 B per float4 group of a 3x3 kernel; a tap per blockIdx.y
// would write 4-byte pieces 36 B apart).  Taps outside tap_mask store 0 (the caller fills nothing), tap `ftap` is copied from fsrc
// [M][fld] when that is given; accumulate adds to what the destination holds.  partial may be null when tap_mask is empty.
template <int SL>
__global__ __launch_bounds__(256) void tn_reduce_oihw_kernel(const float* __restrict__ partial, float* __restrict__ C, int M, int N, int taps, int split,
                                                             unsigned tap_mask, int accumulate, int K, int rect, Geo g,
                                                             const float* __restrict__ fsrc, long long fld, int ftap, float* __restrict__ amax_c) {
    constexpr int OG = 256 / SL;
    extern __shared__ __attribute__((aligned(16))) float tile[];          // [4 * OG][taps]
    __shared__ double sh[SL > 1 ? 4 : 1][256];                            // (SL = 1 sums without meeting anybody: never touched, dropped by the compiler)
    const long long mn = (long long)M * N, slice_stride = (long long)__popc(tap_mask) * mn;
    const int n4 = N >> 2;
    const long long total = (long long)M * n4;
    const int ol = threadIdx.x % OG, sl = threadIdx.x / OG;
    const long long g0 = (long long)blockIdx.x * OG;                      // first float4 group of this workgroup
    const int ngrp = (int)min((long long)OG, total - g0);
    const int nfl = ngrp * 4 * taps;                                      // floats of the tile: a multiple of 4, 16-byte aligned in C
    float* __restrict__ dst = C + g0 * 4 * taps;
    if (accumulate) {
        for (int i = 4 * threadIdx.x; i < nfl; i += 1024) *reinterpret_cast<float4*>(tile + i) = *reinterpret_cast<const float4*>(dst + i);
        __syncthreads();
    }
    const bool live = ol < ngrp;
    const long long row = live ? (g0 + ol) / n4 : 0;
    const int c4 = live ? (int)(g0 + ol - row * n4) * 4 : 0;
    float* to = tile + 4 * ol * taps;                                     // element j of the group, tap t: to[j * taps + t]
    int ord = 0;                                                          // ordinal of tap t among the kept ones (its slab)
    for (int t = 0; t < taps; ++t) {
        auto prev = [&] { return make_float4(to[t], to[taps + t], to[2 * taps + t], to[3 * taps + t]); };
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((tap_mask >> t) & 1u) {
            const int nvalid = tn_valid_slices(tn_tap_row_count<false>(rect, t, K, g), K, split, BK);
            v = tn_sum_slabs<SL>(partial + (long long)ord * mn + row * N + c4, slice_stride, nvalid, live, accumulate, prev, SL > 1 ? sh : nullptr);
            ++ord;
        } else if (sl == 0 && live) {
            if (fsrc && t == ftap) v = *reinterpret_cast<const float4*>(fsrc + row * fld + c4);
            if (accumulate) { const float4 o = prev(); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        }
        if (sl == 0 && live) { to[t] = v.x; to[taps + t] = v.y; to[2 * taps + t] = v.z; to[3 * taps + t] = v.w; }
    }
    __syncthreads();
    float cmax = 0.f;
    for (int i = 4 * threadIdx.x; i < nfl; i += 1024) {
        const float4 v = *reinterpret_cast<const float4*>(tile + i);
        *reinterpret_cast<float4*>(dst + i) = v;
        cmax = amax4(cmax, v);
    }
    tn_amax<false>(amax_c, cmax);
}

constexpr size_t SMEM_ROWS_NT = (2 * BK * LD_T + 2 * BK * LD_T) * sizeof(float) + 16;
constexpr size_t SMEM_ROWS_NN = (2 * BK * LD_T + 2 * BK * LD_V) * sizeof(float) + 16;
constexpr size_t SMEM_TN = (4 * BK * LD_V) * sizeof(float) + 2 * 32 * sizeof(int);

}  // namespace

namespace glf {
int init_gemm_attrs() {
    hipError_t e;
#define SET_ATTR(fn, bytes)                                                                              \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
    if (e != hipSuccess) return fail(GLF_ERR_LAUNCH, "hipFuncSetAttribute(" #fn "): %s", hipGetErrorString(e));
    SET_ATTR((gemm_rows_kernel<0, false>), SMEM_ROWS_NT)
    SET_ATTR((gemm_rows_kernel<0, true>), SMEM_ROWS_NT)
    SET_ATTR((gemm_rows_kernel<1, false>), SMEM_ROWS_NN)
    SET_ATTR((gemm_rows_kernel<1, true>), SMEM_ROWS_NN)
    SET_ATTR((gemm_tn_kernel<false>), SMEM_TN)
    SET_ATTR((gemm_tn_kernel<true>), SMEM_TN)
#undef SET_ATTR
    if (int rc = init_gemm_bf16s_attrs()) return rc;
    return init_gemm_f16s_attrs();
}
}  // namespace glf

namespace {
// f16x3 with amax_a / amax_b == NULL: measure the operands (exactly the elements the call can read) first
int self_amax(GemmArgs& a, const glf_gemm_params* p, bool tn, hipStream_t s) {
    if (a.amax_a && a.amax_b) return GLF_OK;
    float* slots = glf::amax_scratch(2, s);
    GLF_REQUIRE(slots != nullptr, GLF_ERR_WORKSPACE, "gemm(f16x3): no amax scratch");
    hipError_t e = hipMemsetAsync(slots, 0, 2 * sizeof(float), s);
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "hipMemsetAsync(amax): %s", hipGetErrorString(e));
    const long long src_rows = p->gather ? (long long)p->n_img * p->hs * p->ws : 0;
    for (int b = 0; b < p->batch; ++b) {
        if (!a.amax_a) {
            const long long rows = tn ? p->K : (p->gather ? src_rows : p->M);
            const int cols = tn ? p->M : p->K;
            if (int rc = glf::launch_amax(a.A + b * a.bsa, rows, cols, p->lda, a.vec_a, slots, s)) return rc;
        }
        if (!a.amax_b) {
            if (tn) {
                const long long rows = p->gather ? src_rows : p->K;
                if (int rc = glf::launch_amax(a.B + b * a.bsb, rows, p->N, p->ldb, a.vec_b, slots + 1, s)) return rc;
            } else {
                for (unsigned mm = p->tap_mask; mm; mm &= mm - 1) {
                    const int t = __builtin_ctz(mm);
                    if (int rc = glf::launch_amax(a.B + b * a.bsb + t * a.tap_stride_b, p->N, p->K, p->ldb, a.vec_b, slots + 1, s)) return rc;
                }
            }
        }
    }
    if (!a.amax_a) a.amax_a = slots;
    if (!a.amax_b) a.amax_b = slots + 1;
    return GLF_OK;
}
}  // namespace

extern "C" int glf_amax(const float* x, int64_t rows, int cols, int64_t ld, float* out, glf_stream_t stream) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && out, GLF_ERR_NULL, "amax: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && ld >= cols, GLF_ERR_BAD_SHAPE, "amax: bad extents");
    hipError_t e = hipMemsetAsync(out, 0, sizeof(float), glf::S(stream));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "hipMemsetAsync(amax): %s", hipGetErrorString(e));
    return glf::launch_amax(x, rows, cols, ld, aligned16(x) && (ld % 4 == 0), out, glf::S(stream));
}

extern "C" int glf_split_f16_packed(const float* x, int64_t rows, int cols, int64_t ld, const float* amax, float* out, int64_t ldo,
                                    glf_stream_t stream) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && amax && out, GLF_ERR_NULL, "split_f16_packed: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0 && ld % 4 == 0 && ldo % 4 == 0 && ld >= cols && ldo >= cols, GLF_ERR_BAD_SHAPE,
                "split_f16_packed: cols and the row strides must be multiples of 4");
    GLF_REQUIRE(aligned16(x) && aligned16(out), GLF_ERR_BAD_SHAPE, "split_f16_packed: x and out must be 16-byte aligned");
    return glf::launch_split_packed(x, rows, cols, ld, amax, out, ldo, glf::S(stream));
}

extern "C" int glf_split_f16_packed_colsum(const float* x, int rows, int cols, int64_t ld, const float* amax, float* out, int64_t ldo,
                                           float* colsum, double* workspace, glf_stream_t stream) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(x && amax && out && colsum && workspace, GLF_ERR_NULL, "split_f16_packed_colsum: null argument");
    GLF_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0 && ld % 4 == 0 && ldo % 4 == 0 && ld >= cols && ldo >= cols, GLF_ERR_BAD_SHAPE,
                "split_f16_packed_colsum: cols and the row strides must be multiples of 4");
    GLF_REQUIRE(aligned16(x) && aligned16(out), GLF_ERR_BAD_SHAPE, "split_f16_packed_colsum: x and out must be 16-byte aligned");
    GLF_REQUIRE(out != x, GLF_ERR_BAD_SHAPE, "split_f16_packed_colsum: out must not alias x");
    return glf::launch_split_packed_colsum(x, rows, cols, ld, amax, out, ldo, colsum, workspace, glf::S(stream));
}

// ----------------------------------------------------------------------------------------------------------
// Skinny NT: M <= 64 rows (the ASPP pooled branch, deeplabv3.py:123-135: ONE row per frame).  The tile kernels put such a
// shape on one or two workgroups that walk the whole K alone -- 64 dependent global-memory round trips, 0.2 ms for 34 MFLOP
// at 64 x 256 x 2048.  Here a workgroup owns SK_COLS output columns for all rows: thread = (row, one of four k-lanes), the
// B rows are the same address across the rows of a wave (broadcast out of L1), four independent A loads in flight per thread,
// the k-lanes folded with two shuffles.  fp32 FMA arithmetic (exact-fp32 grade under every precision setting).
// ----------------------------------------------------------------------------------------------------------
constexpr int SK_COLS = 2;
__global__ __launch_bounds__(256) void gemm_skinny_nt_kernel(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ bias,
                                                            float* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc, float alpha,
                                                            int accumulate, float* __restrict__ amax_c) {
    const int tid = threadIdx.x, kl = tid & 3, m = tid >> 2;
    const int n0 = blockIdx.x * SK_COLS;
    const float* a = A + (long long)min(m, M - 1) * lda + 4 * kl;
    const float* b[SK_COLS];
#pragma unroll
    for (int j = 0; j < SK_COLS; ++j) b[j] = B + (long long)min(n0 + j, N - 1) * ldb + 4 * kl;
    float acc[SK_COLS] = {};
    int k = 0;
    for (; k + 64 <= K; k += 64) {
        float4 av[4], bv[SK_COLS][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) av[u] = *reinterpret_cast<const float4*>(a + k + 16 * u);
#pragma unroll
        for (int j = 0; j < SK_COLS; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u) bv[j][u] = *reinterpret_cast<const float4*>(b[j] + k + 16 * u);
#pragma unroll
        for (int j = 0; j < SK_COLS; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u)
                acc[j] += av[u].x * bv[j][u].x + av[u].y * bv[j][u].y + av[u].z * bv[j][u].z + av[u].w * bv[j][u].w;
    }
    for (; k < K; k += 16) {
        const float4 av = *reinterpret_cast<const float4*>(a + k);
#pragma unroll
        for (int j = 0; j < SK_COLS; ++j) {
            const float4 bv = *reinterpret_cast<const float4*>(b[j] + k);
            acc[j] += av.x * bv.x + av.y * bv.y + av.z * bv.z + av.w * bv.w;
        }
    }
    float cmax = 0.f;
#pragma unroll
    for (int j = 0; j < SK_COLS; ++j) {
        float v = acc[j];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        if (kl == 0 && m < M && n0 + j < N) {
            v = v * alpha + (bias ? bias[n0 + j] : 0.f);
            float* c = C + (long long)m * ldc + n0 + j;
            if (accumulate) v += *c;
            *c = v;
            cmax = fmaxf(cmax, fabsf(v));
        }
    }
    if (amax_c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, o));
        if ((tid & 63) == 0 && cmax > 0.f) atomicMax(reinterpret_cast<unsigned*>(amax_c), __float_as_uint(cmax));
    }
}

// Segmented region mode (glf_gemm_params.nseg): the SEG instantiations of the 8-wave split-fp16 kernel only.  cols / boff: the column
// groups and B offsets of glf_gemm_nt_seg_cols, null for glf_gemm_nt.  Everything is refused before the first launch.
static int seg_launch(GemmArgs& a, const glf_gemm_params* p, const int32_t* cols, const int64_t* boff, const char* who, glf_stream_t stream) {
    const int prec = call_precision(p);
    GLF_REQUIRE(p->nseg >= 1 && p->nseg <= GLF_SEG_MAX && p->seg != nullptr, GLF_ERR_UNSUPPORTED, "%s: nseg must be in [1, %d] with a segment list", who, GLF_SEG_MAX);
    GLF_REQUIRE(prec >= 2 && glf::f16s_rows_ok(a) && p->a_presplit && p->b_presplit && p->amax_a && p->amax_b, GLF_ERR_UNSUPPORTED,
                "%s: segments need precision 3 / 4, the aligned fast path and both operands pre-split with their amax", who);
    GLF_REQUIRE(!p->gather && p->taps == 1 && !p->rect && !p->accumulate && p->batch == 1, GLF_ERR_UNSUPPORTED,
                "%s: segments extend a plain NT launch (no gather, rect, accumulate or batch)", who);
    // colstats / colmax: every element is stored once through the region-mode epilogue, which counts exactly the rows it stores;
    // colmax comes from the wide-store form of that epilogue only (as for a plain launch)
    GLF_REQUIRE(!p->colmax || (p->colstats && p->ldc % 4 == 0 && p->N % 4 == 0 && aligned16(a.C)), GLF_ERR_UNSUPPORTED,
                "%s: colmax needs colstats and a 16-byte aligned C with ldc and N multiples of 4", who);
    GLF_REQUIRE(p->n_img > 0 && p->hd > 0 && p->wd > 0 && (long long)p->n_img * p->hd * p->wd == p->M && p->K <= p->lda && p->N <= p->ldc,
                GLF_ERR_BAD_SHAPE, "%s: segments need M (%d) == n_img*hd*wd, K <= lda and N <= ldc", who, p->M);
    GLF_REQUIRE(p->seg_kx >= BK && p->seg_kx % BK == 0, GLF_ERR_UNSUPPORTED, "%s: segments need seg_kx %% 32 == 0", who);
    if (boff) {
        // (B's slice of segment s starts boff[s] floats behind the start of the row of each of the segment's columns: the caller
        // vouches for the buffer behind it)
        for (int i = 0; i < p->nseg; ++i)
            GLF_REQUIRE(boff[i] >= 0 && boff[i] % 4 == 0, GLF_ERR_UNSUPPORTED, "%s: segment %d: the B offset must be a non-negative multiple of 4", who, i);
    } else {
        GLF_REQUIRE((long long)p->K + (long long)p->nseg * p->seg_kx <= p->ldb, GLF_ERR_UNSUPPORTED, "%s: segments need K + nseg * seg_kx <= ldb", who);
    }
    if (cols) GLF_REQUIRE(p->N % BN == 0, GLF_ERR_UNSUPPORTED, "%s: column groups need N %% 128 == 0", who);
    for (int i = 0; i < p->nseg; ++i)
        GLF_REQUIRE(p->seg[3 * i + 2] >= 0 && p->seg[3 * i + 2] % 4 == 0 && p->seg[3 * i + 2] + p->seg_kx <= p->lda, GLF_ERR_UNSUPPORTED,
                    "%s: segment %d: acol must be a multiple of 4 with acol + seg_kx <= lda", who, i);
    // (overhang rows walk the zero page from end to end of the chain: the launcher bounds the longest chain of the plan by the page)
    return glf::launch_rows_f16s_seg(a, p, cols, boff, prec == 2 ? 3 : 1, glf::S(stream));
}

extern "C" int glf_gemm_nt(const float* A, const float* B, const float* bias, float* C,
                           const glf_gemm_params* p, glf_stream_t stream) {
    if (int rc = glf::ensure_init()) return rc;
    if (int rc = validate(p, A, B, C)) return rc;
    if (p->gather) GLF_REQUIRE((long long)p->n_img * p->hd * p->wd == p->M, GLF_ERR_BAD_SHAPE,
                               "gemm_nt: M (%d) != n_img*hd*wd", p->M);
    if (p->tap_mask == 0) return glf::fail(GLF_ERR_BAD_SHAPE, "gemm_nt: empty tap_mask");
    GemmArgs a = make_args(A, B, bias, C, p);
    const int prec = call_precision(p);
    a.vec_a = aligned16(A) && (p->lda % 4 == 0) && (p->batch_stride_a % 4 == 0);
    a.vec_b = aligned16(B) && (p->ldb % 4 == 0) && (p->batch_stride_b % 4 == 0) && (p->tap_stride_b % 4 == 0);
    dim3 grid(a.tiles_m * a.tiles_n, 1, p->batch);
    if (p->nseg != 0) return seg_launch(a, p, nullptr, nullptr, "glf_gemm_nt", stream);     // segmented region mode
    if (p->M <= 64 && !p->gather && p->taps == 1 && p->batch == 1 && !p->rect && !p->colstats && !p->a_presplit && !p->b_presplit && a.vec_a &&
        a.vec_b && p->K % 16 == 0 && p->N >= 64) {
        hipLaunchKernelGGL(gemm_skinny_nt_kernel, dim3((p->N + SK_COLS - 1) / SK_COLS), dim3(256), 0, glf::S(stream), A, B, bias, C, p->M, p->N, p->K,
                           p->lda, p->ldb, p->ldc, p->alpha, p->accumulate, p->amax_c);
        return glf::check_launch("gemm_nt(skinny)");
    }
    if (p->rect == 2) {                 // region mode: f16x3 kernels only (see region_of in gemm_common.h)
        GLF_REQUIRE(prec >= 2 && glf::f16s_rows_ok(a), GLF_ERR_UNSUPPORTED,
                    "glf_gemm_nt: rect = 2 (region mode) exists on the f16x3 kernels only (precision 2, K %% 32 == 0, aligned operands)");
        GLF_REQUIRE(p->gather != 0 && p->kh == 3 && p->kw == 3 && p->stride == 1 && p->pad == p->dil && p->hs == p->hd && p->ws == p->wd &&
                    p->batch == 1, GLF_ERR_UNSUPPORTED, "glf_gemm_nt: region mode needs a 3x3 stride-1 conv with pad == dil on equal maps, batch 1");
        a.rect = 2;
    } else if (p->rect) {
        if (int rc = setup_rect(p, bias, a, grid, "glf_gemm_nt")) return rc;
    }
    GLF_REQUIRE(!p->colstats || (prec >= 2 && glf::f16s_rows_ok(a) && p->rect != 1 && p->batch == 1), GLF_ERR_UNSUPPORTED,
                "glf_gemm_nt: colstats is honoured by the f16x3 kernels only (precision 2, K %% 32 == 0, aligned operands, no rect = 1, batch 1)");
    // colmax is produced by the wide-store (LDS-parked) epilogue of the split-fp16 kernels only: refuse it wherever a call would run
    // another epilogue (a zero colmax would make glf_bn_apply_from_sums bound max|y| too low and the packed image overflow its scale)
    GLF_REQUIRE(!p->colmax || (p->colstats && prec >= 2 && glf::f16s_rows_ok(a) && p->rect != 1 && p->ldc % 4 == 0 && p->N % 4 == 0 && aligned16(C) &&
                               p->batch_stride_c % 4 == 0),
                GLF_ERR_UNSUPPORTED, "glf_gemm_nt: colmax needs colstats, precision 3 / 4 on the aligned fast path, no rect = 1, and a 16-byte aligned C with "
                "ldc, N and batch_stride_c multiples of 4 (the wide-store epilogue is the one that folds it)");
    if (prec == 1 && glf::bf16s_rows_ok(a)) return glf::launch_rows_bf16s(a, grid, p->gather != 0, glf::S(stream));
    if (p->a_presplit || p->b_presplit)
        GLF_REQUIRE(prec >= 2 && glf::f16s_rows_ok(a) && (!p->a_presplit || p->amax_a) && (!p->b_presplit || p->amax_b), GLF_ERR_UNSUPPORTED,
                    "glf_gemm_nt: a pre-split operand needs precision 3 / 4, the aligned fast path and the amax it was split with");
    if (prec >= 2 && glf::f16s_rows_ok(a)) {
        if (int rc = self_amax(a, p, false, glf::S(stream))) return rc;
        return glf::launch_rows_f16s(a, grid, p->gather != 0, prec == 2 ? 3 : 1, glf::S(stream));
    }
    if (p->gather)
        hipLaunchKernelGGL((gemm_rows_kernel<0, true>), grid, dim3(NTHREADS), SMEM_ROWS_NT, glf::S(stream), a);
    else
        hipLaunchKernelGGL((gemm_rows_kernel<0, false>), grid, dim3(NTHREADS), SMEM_ROWS_NT, glf::S(stream), a);
    return glf::check_launch("gemm_nt");
}

// glf_gemm_nt in segmented region mode whose segments belong to groups of output columns (include/glfusion.h)
extern "C" int glf_gemm_nt_seg_cols(const float* A, const float* B, float* C, const glf_gemm_params* p, const int32_t* seg_cols,
                                    const int64_t* seg_boff, glf_stream_t stream) {
    GLF_REQUIRE(seg_cols != nullptr, GLF_ERR_NULL, "gemm_nt_seg_cols: null column groups");
    if (int rc = glf::ensure_init()) return rc;
    if (int rc = validate(p, A, B, C)) return rc;
    GemmArgs a = make_args(A, B, nullptr, C, p);
    a.vec_a = aligned16(A) && (p->lda % 4 == 0);
    a.vec_b = aligned16(B) && (p->ldb % 4 == 0);
    return seg_launch(a, p, seg_cols, seg_boff, "glf_gemm_nt_seg_cols", stream);
}

// glf_gemm_nt with the fused output epilogue C = act(alpha * acc + shift[n] (+ residual[m][n])): the EPI instantiations of the
// split-fp16 rows kernels.  Everything that can be refused is refused before the first HIP runtime call.
extern "C" int glf_gemm_nt_epilogue(const float* A, const float* B, float* C, const glf_gemm_params* p, const glf_gemm_epilogue* e,
                                    glf_stream_t stream) {
    GLF_REQUIRE(A && B && C && p && e && e->shift, GLF_ERR_NULL, "gemm_nt_epilogue: null argument");
    if (int rc = validate(p, A, B, C)) return rc;
    if (p->gather) GLF_REQUIRE((long long)p->n_img * p->hd * p->wd == p->M, GLF_ERR_BAD_SHAPE, "gemm_nt_epilogue: M (%d) != n_img*hd*wd", p->M);
    GLF_REQUIRE(p->tap_mask != 0, GLF_ERR_BAD_SHAPE, "gemm_nt_epilogue: empty tap_mask");
    GLF_REQUIRE(p->ldc >= p->N, GLF_ERR_BAD_SHAPE, "gemm_nt_epilogue: ldc (%d) < N (%d)", p->ldc, p->N);
    GLF_REQUIRE(e->relu == 0 || e->relu == 1, GLF_ERR_BAD_SHAPE, "gemm_nt_epilogue: relu must be 0 or 1");
    GLF_REQUIRE(!e->residual || e->ld_res >= p->N, GLF_ERR_BAD_SHAPE, "gemm_nt_epilogue: ld_res (%lld) < N (%d)", (long long)e->ld_res, p->N);
    const int prec = call_precision(p);
    GLF_REQUIRE(prec >= 2, GLF_ERR_UNSUPPORTED, "gemm_nt_epilogue: built on the split-fp16 kernels only (precision 3 / 4, effective %d)", prec + 1);
    GLF_REQUIRE(p->rect != 1 && !p->accumulate && p->split <= 1 && !p->colstats && !p->colmax && p->batch == 1, GLF_ERR_UNSUPPORTED,
                "gemm_nt_epilogue: rect = 1, accumulate, split > 1, colstats / colmax and batch > 1 cannot be combined with the epilogue");
    GemmArgs a = make_args(A, B, e->shift, C, p);
    a.vec_a = aligned16(A) && (p->lda % 4 == 0);
    a.vec_b = aligned16(B) && (p->ldb % 4 == 0) && (p->tap_stride_b % 4 == 0);
    GLF_REQUIRE(a.vec_a && a.vec_b && p->K % BK == 0 && p->K <= glf::ZERO_PAGE_FLOATS, GLF_ERR_UNSUPPORTED,
                "gemm_nt_epilogue: needs the aligned fast path (K %% 32 == 0, 16-byte aligned A / B, lda / ldb / tap_stride_b %% 4 == 0)");
    GLF_REQUIRE((!p->a_presplit || p->amax_a) && (!p->b_presplit || p->amax_b), GLF_ERR_UNSUPPORTED,
                "gemm_nt_epilogue: a pre-split operand needs the amax it was split with");
    if (p->rect == 2) {
        GLF_REQUIRE(p->gather != 0 && p->kh == 3 && p->kw == 3 && p->stride == 1 && p->pad == p->dil && p->hs == p->hd && p->ws == p->wd,
                    GLF_ERR_UNSUPPORTED, "gemm_nt_epilogue: region mode needs a 3x3 stride-1 conv with pad == dil on equal maps");
        a.rect = 2;
    } else {
        GLF_REQUIRE(p->rect == 0, GLF_ERR_UNSUPPORTED, "gemm_nt_epilogue: rect must be 0 or 2");
    }
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(glf::f16s_rows_ok(a), GLF_ERR_UNSUPPORTED, "gemm_nt_epilogue: the split-fp16 rows kernel cannot take this call");
    a.epi = 1; a.res = e->residual; a.ld_res = e->ld_res; a.relu = e->relu;
    if (int rc = self_amax(a, p, false, glf::S(stream))) return rc;
    dim3 grid(a.tiles_m * a.tiles_n, 1, 1);
    return glf::launch_rows_f16s(a, grid, p->gather != 0, prec == 2 ? 3 : 1, glf::S(stream));
}

extern "C" int glf_gemm_nn(const float* A, const float* B, const float* bias, float* C,
                           const glf_gemm_params* p, glf_stream_t stream) {
    if (int rc = glf::ensure_init()) return rc;
    if (int rc = validate(p, A, B, C)) return rc;
    if (p->gather) GLF_REQUIRE((long long)p->n_img * p->hd * p->wd == p->M, GLF_ERR_BAD_SHAPE,
                               "gemm_nn: M (%d) != n_img*hd*wd", p->M);
    if (p->tap_mask == 0) return glf::fail(GLF_ERR_BAD_SHAPE, "gemm_nn: empty tap_mask");
    GemmArgs a = make_args(A, B, bias, C, p);
    a.vec_a = aligned16(A) && (p->lda % 4 == 0) && (p->batch_stride_a % 4 == 0);
    a.vec_b = aligned16(B) && (p->ldb % 4 == 0) && (p->batch_stride_b % 4 == 0) && (p->tap_stride_b % 4 == 0);
    dim3 grid(a.tiles_m * a.tiles_n, 1, p->batch);
    GLF_REQUIRE(!p->colstats, GLF_ERR_UNSUPPORTED, "glf_gemm_nn: colstats is honoured by glf_gemm_nt on the f16x3 kernels only");
    GLF_REQUIRE(p->rect != 2, GLF_ERR_UNSUPPORTED, "glf_gemm_nn: rect = 2 (region mode) is built for glf_gemm_nt on the f16x3 kernels only");
    if (p->rect) {
        if (int rc = setup_rect(p, bias, a, grid, "glf_gemm_nn")) return rc;
    }
    if (p->gather)
        hipLaunchKernelGGL((gemm_rows_kernel<1, true>), grid, dim3(NTHREADS), SMEM_ROWS_NN, glf::S(stream), a);
    else
        hipLaunchKernelGGL((gemm_rows_kernel<1, false>), grid, dim3(NTHREADS), SMEM_ROWS_NN, glf::S(stream), a);
    return glf::check_launch("gemm_nn");
}

extern "C" int glf_gemm_tn(const float* A, const float* B, float* C,
                           const glf_gemm_params* p, glf_stream_t stream) {
    if (int rc = glf::ensure_init()) return rc;
    if (int rc = validate(p, A, B, C)) return rc;
    GLF_REQUIRE(p->gather != 2, GLF_ERR_UNSUPPORTED, "gemm_tn: transposed gather is not defined for the reduction form");
    GLF_REQUIRE(!p->colstats, GLF_ERR_UNSUPPORTED, "gemm_tn: colstats is honoured by glf_gemm_nt on the f16x3 kernels only");
    if (p->gather) GLF_REQUIRE((long long)p->n_img * p->hd * p->wd == p->K, GLF_ERR_BAD_SHAPE,
                               "gemm_tn: K (%d rows) != n_img*hd*wd", p->K);
    GemmArgs a = make_args(A, B, nullptr, C, p);
    const int ntap = __builtin_popcount(p->tap_mask);
    const bool oihw = p->c_oihw != 0;
    if (oihw) {
        GLF_REQUIRE(p->batch == 1 && p->N % 4 == 0 && aligned16(C) && p->taps <= GLF_TN_OIHW_MAX_TAPS, GLF_ERR_UNSUPPORTED,
                    "gemm_tn: c_oihw needs batch 1, N %% 4 == 0, a 16-byte aligned C and taps <= %d", GLF_TN_OIHW_MAX_TAPS);
        GLF_REQUIRE(ntap == 0 || p->workspace != nullptr, GLF_ERR_UNSUPPORTED, "gemm_tn: c_oihw stores through the workspace (two-stage reduction)");
        if (p->foreign_src)
            GLF_REQUIRE(p->foreign_tap >= 0 && p->foreign_tap < p->taps && !((p->tap_mask >> p->foreign_tap) & 1u) && p->foreign_ld >= p->N &&
                        p->foreign_ld % 4 == 0 && aligned16(p->foreign_src), GLF_ERR_BAD_SHAPE,
                        "gemm_tn: the foreign tap must be a tap outside tap_mask, its source 16-byte aligned with a row stride %% 4 == 0 and >= N");
    } else {
        GLF_REQUIRE(!p->foreign_src, GLF_ERR_UNSUPPORTED, "gemm_tn: a foreign tap needs c_oihw");
    }
    auto store_oihw = [&](const TnReducePlan& plan) {
        const size_t lds = (size_t)(1024 / plan.lanes) * p->taps * sizeof(float);
        const dim3 gr((unsigned)plan.blocks);
        tn_by_lanes(plan.lanes, [&](auto sl) {
            hipLaunchKernelGGL((tn_reduce_oihw_kernel<sl()>), gr, dim3(256), lds, glf::S(stream), a.partial, C, p->M, p->N, p->taps, a.split, p->tap_mask,
                               p->accumulate, p->K, a.rect, a.g, p->foreign_src, (long long)p->foreign_ld, p->foreign_tap, p->amax_c);
        });
        return glf::check_launch("gemm_tn(reduce, oihw)");
    };
    if (ntap == 0) return oihw ? store_oihw(tn_reduce_plan((long long)p->M * (p->N / 4), 1, true)) : GLF_OK;       // every tap in the padding: dW stays as the caller left it (c_oihw: zeros + the foreign tap)
    GLF_REQUIRE((long long)p->batch * a.split <= 65535, GLF_ERR_BAD_SHAPE, "gemm_tn: batch*split too large");
    a.vec_a = aligned16(A) && (p->lda % 4 == 0) && (p->batch_stride_a % 4 == 0);
    a.vec_b = aligned16(B) && (p->ldb % 4 == 0) && (p->batch_stride_b % 4 == 0);
    if (p->rect) {
        GLF_REQUIRE(p->gather == 1 && p->stride == 1 && p->batch == 1, GLF_ERR_UNSUPPORTED,
                    "gemm_tn: rect mode needs a stride-1 forward conv gather and batch 1");
        a.rect = 1;
    }
    dim3 grid(a.tiles_m * a.tiles_n, ntap, p->batch * a.split);
    const int prec = call_precision(p);
    const bool two_stage = (a.split > 1 || oihw) && p->workspace != nullptr;
    if (two_stage) {
        GLF_REQUIRE(p->workspace_bytes >= (int64_t)glf_gemm_tn_workspace_bytes(p), GLF_ERR_WORKSPACE,
                    "gemm_tn: workspace of %lld bytes, glf_gemm_tn_workspace_bytes() asks for %zu", (long long)p->workspace_bytes,
                    glf_gemm_tn_workspace_bytes(p));
        GLF_REQUIRE(aligned16(p->workspace), GLF_ERR_WORKSPACE, "gemm_tn: workspace must be 16-byte aligned");
        a.partial = p->workspace;
    }
    if (p->a_presplit || p->b_presplit)
        GLF_REQUIRE(prec >= 2 && glf::f16s_tn_ok(a) && (!p->a_presplit || p->amax_a) && (!p->b_presplit || p->amax_b), GLF_ERR_UNSUPPORTED,
                    "glf_gemm_tn: a pre-split operand needs precision 3 / 4, the aligned fast path and the amax it was split with");
    int rc;
    if (prec == 1 && glf::bf16s_tn_ok(a)) {
        rc = glf::launch_tn_bf16s(a, grid, p->gather != 0, glf::S(stream));
    } else if (prec >= 2 && glf::f16s_tn_ok(a)) {
        if (int rc2 = self_amax(a, p, true, glf::S(stream))) return rc2;
        rc = glf::launch_tn_f16s(a, grid, p->gather != 0, prec == 2 ? 3 : 1, glf::S(stream));
    } else {
        if (p->gather)
            hipLaunchKernelGGL((gemm_tn_kernel<true>), grid, dim3(NTHREADS), SMEM_TN, glf::S(stream), a);
        else
            hipLaunchKernelGGL((gemm_tn_kernel<false>), grid, dim3(NTHREADS), SMEM_TN, glf::S(stream), a);
        rc = glf::check_launch("gemm_tn");
    }
    if (rc != GLF_OK || !two_stage) return rc;
    const int vec = (p->N % 4 == 0) && (p->ldc % 4 == 0) && aligned16(C) && (p->tap_stride_b % 4 == 0) && (p->batch_stride_c % 4 == 0);
    const TnReducePlan plan = tn_reduce_plan(vec ? (long long)p->M * (p->N / 4) : (long long)p->M * p->N, a.split, vec != 0);
    if (oihw) return store_oihw(plan);           // (vec holds: N % 4 == 0 and the alignment of C were required above)
    const long long cap = plan.lanes > 1 ? 4096 : 2048;
    const dim3 gr((unsigned)(plan.blocks < cap ? plan.blocks : cap), ntap, p->batch);
    tn_by_lanes(plan.lanes, [&](auto sl) {
        if constexpr (sl() == 1)
            hipLaunchKernelGGL(tn_reduce_kernel, gr, dim3(256), 0, glf::S(stream), a.partial, C, p->M, p->N, p->ldc, (long long)p->tap_stride_b,
                               (long long)p->batch_stride_c, a.split, p->tap_mask, p->accumulate, p->K, a.rect, a.g, vec, p->amax_c);
        else
            hipLaunchKernelGGL((tn_reduce_lanes_kernel<sl()>), gr, dim3(256), 0, glf::S(stream), a.partial, C, p->M, p->N, p->ldc, (long long)p->tap_stride_b,
                               (long long)p->batch_stride_c, a.split, p->tap_mask, p->accumulate, p->K, a.rect, a.g, p->amax_c);
    });
    return glf::check_launch("gemm_tn(reduce)");
}

extern "C" size_t glf_gemm_tn_workspace_bytes(const glf_gemm_params* p) {
    if (!p || (p->split <= 1 && !p->c_oihw)) return 0;
    const size_t ntap = (size_t)__builtin_popcount(p->tap_mask);
    return (size_t)p->batch * (size_t)(p->split < 1 ? 1 : p->split) * ntap * (size_t)p->M * (size_t)p->N * sizeof(float);
}


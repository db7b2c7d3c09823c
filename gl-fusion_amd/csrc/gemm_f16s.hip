// Split-fp16 ("f16x3") contraction kernels: fp32-class GEMM on the fp16 matrix cores of gfx950 with THREE MFMAs per
// product instead of the six of gemm_bf16s.hip.
//
// Each operand is first multiplied by a power of two s = 2^(13 - floor(log2 amax)) derived from the operand's max
// magnitude (a device scalar: glf_gemm_params.amax_a / amax_b, produced by glf_amax or by the kernel that wrote the
// operand), so that |x s| < 2^14 sits at the top of the fp16 range.  x s is then split into two fp16 pieces
//      x s = h + 2^-11 l + e,      h = rne16(x s),   l = rne16((x s - h) 2^11),   |e| <= 2^-22 |x s|
// (full 22-bit precision for every element within 2^-27 of amax, an absolute error floor of 2^-49 amax below), and
//      a*b ~= ha*hb + 2^-11 (ha*lb + la*hb)                                    (dropped la*lb <= 2^-22 |a*b|)
// is evaluated with three v_mfma_f32_32x32x16_f16 per 16 k: the main product accumulates in one fp32 accumulator,
// the two mixed products in a second one that is folded in (times 2^-11) by the epilogue, where the operand
// powers of two are undone exactly as well.  That is 96 MFMA cycles per 16 k against 192 (bf16x6) and 512 (exact
// fp32 MFMA).  The MFMA sums 16 k per instruction, so the accumulation chain is K/16 long -- no per-tile
// two-level fold is needed to stay at the fp32 kernels' error level (tests/test_gpu_ops.py measure it vs fp64).
// Rows that must read as zero (conv padding, tile overhang) are LOADED from a zero page (args.zeros) instead of
// being masked after the load: no per-element selects in the staging path.
//
// Same tiling, LDS swizzle, software pipeline, gather / tap_mask / rect semantics and XCD-aware tile order as
// gemm_bf16s.hip, with two planes per operand instead of three (96 KB of LDS).  Only the aligned fast path is
// built; everything else stays on the exact-fp32 kernels.
#include "gemm_rows_walk.h"
#include "gemm_tn_walk.h"
#include "split_f16.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace {
using glf::SEG_TAB_REGIONS; using glf::SEG_REGION_INTS; using glf::SEG_TAB_OFFS;

#define GLF_MFMA_F16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
// one A tile-row against both B tile-cols for one 16-deep k-step: main products into c, mixed products into m
// (dependent MFMAs are two apart)
// NP (a compile-time constant of the enclosing kernel) = MFMAs per product: 3 = split-fp16 (fp32-grade results),
// 1 = the high halves only (precision 3, "f16": plain fp16 operands with an amax scale, fp32 accumulate)
#define GLF_ROW3(c0, c1, m0, m1, ah, al, b0h, b0l, b1h, b1l)  \
    c0 = GLF_MFMA_F16(ah, b0h, c0);                         \
    c1 = GLF_MFMA_F16(ah, b1h, c1);                         \
    if (NP == 3) {                                          \
        m0 = GLF_MFMA_F16(al, b0h, m0);                     \
        m1 = GLF_MFMA_F16(al, b1h, m1);                     \
        m0 = GLF_MFMA_F16(ah, b0l, m0);                     \
        m1 = GLF_MFMA_F16(ah, b1l, m1);                     \
    }

// ----------------------------------------------------------------------------------------------------------
// rows kernel, NT.  512 threads = 8 waves (4 x 2), tile 256 x 128 x 32, THREE LDS buffers of 2 x (256 + 128) rows
// (144 KB).
// ----------------------------------------------------------------------------------------------------------
constexpr int BM8 = 256;
constexpr int NT8 = 512;
constexpr int WAVE_ROWS = 4;            // wave rows of the 8-wave NT workgroup (4 x 2 waves of 64 x 64)
#ifndef GLF_IL_ALL          // 1: the slot-interleaved iteration also when neither operand is pre-split
#define GLF_IL_ALL 1
#endif
constexpr int PL_A8 = BM8 * 64, PL_B8 = BN * 64;
constexpr int BUF8 = 2 * PL_A8 + 2 * PL_B8;
#ifdef GLF_STAMPS       // diagnostic build (profiles/ubench/stamps.sh): per-wave s_memtime stamps of 16 main-loop iterations of one workgroup
constexpr size_t SMEM_ROWS_H8 = 3 * BUF8 + 16 + 8192;
#else
constexpr size_t SMEM_ROWS_H8 = 3 * BUF8 + 16;
#endif

// PA / BP: the A / B operand arrives PRE-SPLIT in the packed image glf_split_f16_packed writes: every aligned group of four
// consecutive elements (16 bytes of fp32) is replaced IN PLACE by {h0 h1 h2 h3 l0 l1 l2 l3} (fp16), x * s = h + 2^-11 l with the
// scale of args.amax_a / amax_b.  Same byte size, same strides, same addressing as the fp32 operand -- the staging path keeps its
// loads, pointers, zero page and gather logic and only drops the conversion (a bit-cast instead of ~18 VALU per float4): the
// operand is split ONCE (by glf_split_f16_packed, per tensor) instead of in every tile of every launch that reads it.
// (The variants that were measured and dropped -- deeper register prefetch, ping-pong segments, sched_group_barrier interleave,
// static wave priorities, other tile-group sizes -- are described with their numbers in DESIGN.md section 8; their code is gone.)
// EPI: the fused output epilogue of glf_gemm_nt_epilogue -- C = act(alpha * acc + bias[n] (+ res[m][n])), res indexed by the OUTPUT row
// (after the region mapping) with its own row stride, act = identity or ReLU; amax_c then is the maximum of the value stored.
// Only for launches that store every output element exactly once (no rect = 1, accumulate, colstats: refused by the entry point).
// EPI = false compiles to the code it was before the parameter existed.
// SEG: segmented region mode (glf_gemm_params.nseg; instantiated for GATHER = false, PA = BP = true, EPI = false only).  A plain NT
// contraction over K whose rows are the pixels of an n_img x hd x wd map, extended by extra segments: segment s adds
// sum_j A[pixel + (oy_s, ox_s)][acol_s + j] * B[n][K + s * kx + j] where the shifted pixel is inside the map.  The map is cut into
// rectangles inside each of which the set of in-range segments is constant (glf_gemm_nt_seg_plan; the plan reaches the kernel as a
// small device table, args.seg_tab); a row tile enumerates (frame, pixel of its rectangle) as region mode does, walks the K columns
// and then its rectangle's segments by ascending s -- a segment change is a new A row offset and a new B column offset, nothing
// else -- and stores through the region-mode epilogue: every output element once.  SEG = false compiles to the code it was before.
// With column groups (args.seg_cols; glf_gemm_nt_seg_cols) a segment contributes to a range of whole 128-column tiles only: the
// workgroup walks `region mask & column-tile mask` (one more uniform word of the table).  Both forms take their tile from the host's
// dispatch list when the plan has one (args.seg_cols), and B's slice of a segment is a table entry.
template <bool GATHER, int NP, bool BP, bool PA = false, bool EPI = false, bool SEG = false>
__global__ __launch_bounds__(NT8, 2) void gemm_rows_f16s8_kernel(const GemmArgs args) {
    const int pM = args.M, pN = args.N, pK = args.K, p_lda = args.lda, p_ldb = args.ldb, p_ldc = args.ldc;
    const int p_taps = args.taps, p_gather = args.gather, p_accumulate = args.accumulate;
    const int p_tiles_n = args.tiles_n;
    const unsigned p_tap_mask = args.tap_mask;
    const long long p_tsb = args.tap_stride_b, p_bsa = args.bsa, p_bsb = args.bsb, p_bsc = args.bsc;
    const float* __restrict__ p_A = args.A; const float* __restrict__ p_B = args.B; const float* __restrict__ p_bias = args.bias;
    float* __restrict__ p_C = args.C;
    const float* __restrict__ p_zero = args.zeros;
    const int g_hs = args.g.hs, g_ws = args.g.ws, g_hd = args.g.hd, g_wd = args.g.wd, g_kw = args.g.kw;
    const int g_stride = args.g.stride, g_pad = args.g.pad, g_dil = args.g.dil;
    const int p_rect = SEG ? 2 : (GATHER ? args.rect : 0);
    const int* __restrict__ p_seg = args.seg_tab;
    const int p_kx = args.seg_kx;
    float sc_a, sc_b, inv_a, inv_b;
    pow2_scale(args.amax_a, sc_a, inv_a);
    pow2_scale(args.amax_b, sc_b, inv_b);
    const float p_alpha = args.alpha * inv_a * inv_b;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    unsigned* s_mask = reinterpret_cast<unsigned*>(smem_s + 3 * BUF8);
#if defined(GLF_STAMPS) && GLF_STAMPS == 2     // workgroup-level stamps only: entry, main loop start / end, exit (no per-iteration cost)
    unsigned long long wg_t0 = __builtin_amdgcn_s_memtime(), wg_t1 = 0, wg_t2 = 0;
#endif

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const RowsGeo G{p_gather, args.g.n_img, g_hs, g_ws, g_hd, g_wd, g_kw, g_stride, g_pad, g_dil};
    int tn;
    RowTile rt{0, pM, 0, 0, g_hd, g_wd, p_tap_mask};
    unsigned seg_mask = 0;
    if constexpr (SEG) {
        int r;
        if (args.seg_cols) {
            // the host lists the workgroups longest chain first, balanced over the XCDs (seg_units; with column groups chains differ
            // even across the column tiles of one row tile); this one's (region, column tile, row tile of the region) is entry
            // blockIdx.x of that list
            const int2 u = reinterpret_cast<const int2*>(p_seg + glf::SEG_TAB_INTS)[blockIdx.x];
            const int rc = __builtin_amdgcn_readfirstlane(u.x);
            r = rc >> 16; tn = rc & 0xffff;
            rt.tm = __builtin_amdgcn_readfirstlane(u.y);
        } else {
            rows_tile_order((args.flags >> 8) & 0xff, p_tiles_n, tn, rt.tm);
            // the plan's regions: lane r holds the first row tile of region r (INT_MAX beyond the last), one ballot finds this tile's
            const int start = p_seg[lane];
            r = __builtin_amdgcn_readfirstlane(__popcll(__ballot(rt.tm >= start)) - 1);
            rt.tm -= p_seg[r];
        }
        const int* __restrict__ reg = p_seg + SEG_TAB_REGIONS + SEG_REGION_INTS * r;
        rt.y0 = reg[0]; rt.x0 = reg[1]; rt.h = reg[2]; rt.w = reg[3]; seg_mask = (unsigned)reg[4]; rt.rows = reg[5];
        if (args.seg_cols) seg_mask &= (unsigned)p_seg[glf::SEG_TAB_COLMASK + tn];      // the segments of this tile's column group
    } else {
        rows_tile_order((args.flags >> 8) & 0xff, p_tiles_n, tn, rt.tm);
        if (p_rect && !rows_locate<BM8, true>(p_rect, p_tap_mask, G, rt)) return;
    }
    const int tm = rt.tm, pMe = rt.rows;
    unsigned mask = rt.mask;
    const int bz = blockIdx.z;
    const float* __restrict__ A = p_A + (long long)bz * p_bsa;
    const float* __restrict__ B = p_B + (long long)bz * p_bsb;
    float* __restrict__ C = p_C + (long long)bz * p_bsc;

    const int ac = tid & 7, ar = tid >> 3;              // 8 float4 per 32-deep row; rows ar + 64 j

    RowState<4> rows;
    rows_init<4, 64, GATHER, SEG>(rows, tm * BM8 + ar, rt, p_lda, g_hd, g_wd);
    const bool fastg = GATHER && rows_fast_gather(G);
    if (fastg) rows_to_fast(rows, G);
    rows_census<BM8, 4, GATHER>(rows, mask, fastg, ac == 0, p_taps, p_rect, G, s_mask);

    const int nkc = pK / BK;
    const int ntiles = SEG ? nkc + __popc(seg_mask) * (p_kx / BK) : __popc(mask) * nkc;
    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};      // main products
    f32x16 m00 = {0}, m01 = {0}, m10 = {0}, m11 = {0};      // mixed products (x 2^11)
    float4 ra[4], rb[2];
    unsigned rem_mask = SEG ? seg_mask : mask;
    int tap = -1, kc = nkc;
    int nk_cur = nkc;                   // SEG: K-iterations of the slice being walked (the K columns, then one segment at a time),
    long long ao_cur = 0;               // and that slice's element offsets into A's rows and B's rows
    long long bo_cur = 0;
    const float* pa[4];
    const float* pb[2];
    const int a_col[4] = {4 * ac, 4 * ac, 4 * ac, 4 * ac};

    auto advance = [&]() __attribute__((always_inline)) {
        if constexpr (SEG) {
            if (++kc >= nk_cur) {
                kc = 0;
                if (tap == -1) {
                    tap = 0;                        // the K columns of the plain contraction come first
#pragma unroll
                    for (int j = 0; j < 4; ++j) pa[j] = (rows.off[j] >= 0 ? A + rows.off[j] : p_zero) + 4 * ac;      // overhang rows read the zero page
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int n = tn * BN + ar + 64 * j;
                        pb[j] = (n < pN ? B + (long long)n * p_ldb : p_zero) + 4 * ac;
                    }
                } else {
                    // next segment of the region: ONE uniform step takes every row pointer from the end of the slice it walked to the
                    // start of the segment's (a new pixel offset and column block of A, a new column block of B); the rows that read
                    // the zero page just walk on through it (the launcher bounds the whole chain by the page)
                    const int sg = __builtin_amdgcn_readfirstlane(__ffs(rem_mask) - 1);
                    rem_mask &= rem_mask - 1;
                    const long long ao = reinterpret_cast<const long long*>(p_seg + SEG_TAB_OFFS)[sg];
                    const long long bo = reinterpret_cast<const long long*>(p_seg + glf::SEG_TAB_BOFF)[sg];
                    const long long back = (long long)(nk_cur - 1) * BK;
                    const long long da = ao - ao_cur - back, db = bo - bo_cur - back;
                    ao_cur = ao; bo_cur = bo; nk_cur = p_kx / BK;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pa[j] += (tm * BM8 + ar + 64 * j < pMe) ? da : (long long)BK;
#pragma unroll
                    for (int j = 0; j < 2; ++j) pb[j] += (tn * BN + ar + 64 * j < pN) ? db : (long long)BK;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) pa[j] += BK;
#pragma unroll
                for (int j = 0; j < 2; ++j) pb[j] += BK;
            }
        } else
        if (++kc >= nkc) {
            kc = 0;
            tap = rows_next_tap<4, GATHER>(rows, rem_mask, pa, A, p_zero, p_lda, fastg, G, a_col);
            const float* Bt = B + (long long)tap * p_tsb;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = tn * BN + ar + 64 * j;
                pb[j] = (n < pN ? Bt + (long long)n * p_ldb : p_zero) + 4 * ac;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) pa[j] += BK;
#pragma unroll
            for (int j = 0; j < 2; ++j) pb[j] += BK;
        }
    };
    // swizzled staging offset of this thread inside a 64-byte row: 16-byte chunk (ac>>1) ^ ((row>>2)&3), half ac&1
    const int st_off = ar * 64 + ((((ac >> 1) ^ ((ar >> 2) & 3)) << 4) | ((ac & 1) << 3));
#define GLF_H8_CONV_A(J, buf_)                                                                               \
    {                                                                                                        \
        unsigned char* d = smem_s + (buf_) * BUF8 + st_off + J * 64 * 64;                                    \
        if (PA) {                                                                                            \
            *reinterpret_cast<float2*>(d) = make_float2(ra[J].x, ra[J].y);                                   \
            if (NP == 3) *reinterpret_cast<float2*>(d + PL_A8) = make_float2(ra[J].z, ra[J].w);              \
        } else {                                                                                             \
            const SplitH s = split4h(ra[J], sc_a);                                                           \
            *reinterpret_cast<f16x4*>(d) = s.h; if (NP == 3) *reinterpret_cast<f16x4*>(d + PL_A8) = s.l;     \
        }                                                                                                    \
    }
#define GLF_H8_CONV_B(J, buf_)                                                                               \
    {                                                                                                        \
        unsigned char* d = smem_s + (buf_) * BUF8 + 2 * PL_A8 + st_off + J * 64 * 64;                        \
        if (BP) {                                                                                            \
            *reinterpret_cast<float2*>(d) = make_float2(rb[J].x, rb[J].y);                                   \
            if (NP == 3) *reinterpret_cast<float2*>(d + PL_B8) = make_float2(rb[J].z, rb[J].w);              \
        } else {                                                                                             \
            const SplitH s = split4h(rb[J], sc_b);                                                           \
            *reinterpret_cast<f16x4*>(d) = s.h; if (NP == 3) *reinterpret_cast<f16x4*>(d + PL_B8) = s.l;     \
        }                                                                                                    \
    }
#define GLF_H8_LOAD_B(J) rb[J] = *reinterpret_cast<const float4*>(pb[J]);
    // piece pc (0..5): convert + store registers of tile t+1, then refill them with tile t+2
// A pre-split operand goes from its load registers straight into LDS: the store must stay AHEAD of the load that refills the
// same registers (GLF_H8_PIN).  Left to itself the scheduler hoists the load above the store, the two values then need two
// register sets, and the copy it adds at the loop's back edge waits for loads issued a few hundred cycles earlier --
// s_waitcnt vmcnt(1) in every iteration, the whole global-load latency exposed (measured: the pre-split kernel 4 % faster
// than the splitting one instead of the ~1.4x its instruction count promises).
#define GLF_H8_PIN(P_) if (P_) __builtin_amdgcn_sched_barrier(0);
#define GLF_H8_PIECE(pc, buf_, conv_, load_)                                                                 \
    switch (pc) {                                                                                            \
        case 0: if (conv_) GLF_H8_CONV_A(0, buf_) GLF_H8_PIN(PA) if (load_) ra[0] = *reinterpret_cast<const float4*>(pa[0]); GLF_H8_PIN(PA) break; \
        case 1: if (conv_) GLF_H8_CONV_A(1, buf_) GLF_H8_PIN(PA) if (load_) ra[1] = *reinterpret_cast<const float4*>(pa[1]); GLF_H8_PIN(PA) break; \
        case 2: if (conv_) GLF_H8_CONV_A(2, buf_) GLF_H8_PIN(PA) if (load_) ra[2] = *reinterpret_cast<const float4*>(pa[2]); GLF_H8_PIN(PA) break; \
        case 3: if (conv_) GLF_H8_CONV_A(3, buf_) GLF_H8_PIN(PA) if (load_) ra[3] = *reinterpret_cast<const float4*>(pa[3]); GLF_H8_PIN(PA) break; \
        case 4: if (conv_) GLF_H8_CONV_B(0, buf_) GLF_H8_PIN(BP) if (load_) GLF_H8_LOAD_B(0) GLF_H8_PIN(BP) break;      \
        default: if (conv_) GLF_H8_CONV_B(1, buf_) GLF_H8_PIN(BP) if (load_) GLF_H8_LOAD_B(1) GLF_H8_PIN(BP) break;     \
    }

    if (ntiles > 0) {
        const int sw = (lane >> 2) & 3, hh = lane >> 5;
        const int fo0 = (lane & 31) * 64 + (((0 + hh) ^ sw) << 4);
        const int fo1 = (lane & 31) * 64 + (((2 + hh) ^ sw) << 4);
        // Pipeline state at the top of iteration `it`: tiles it and it+1 sit converted in LDS buffers it%3 and
        // (it+1)%3, tile it+2 raw in registers, the k-step-0 fragments of tile it in f*.  The iteration multiplies
        // tile it, converts tile it+2 into buffer (it+2)%3, loads tile it+3 and -- after its first k-step --
        // prefetches the k-step-0 fragments of tile it+1, so no LDS latency is exposed behind the barrier.
        // Prologue: the loads of the first THREE tiles are issued back to back (the accumulators are not live yet, registers are
        // free), then tiles 0 and 1 are converted: one global-memory latency instead of three in a row (5.7 k of a K = 2048
        // workgroup's 132 k cycles went here, a quarter of a K = 256 one's).
        {
            float4 ta[4], tb[2], ua[4], ub[2];
            const bool more = ntiles > 1, more2 = ntiles > 2;
            advance();
#pragma unroll
            for (int pc = 0; pc < 6; ++pc) { GLF_H8_PIECE(pc, 0, false, true) }
            if (more) {
                advance();
#pragma unroll
                for (int j = 0; j < 4; ++j) ta[j] = *reinterpret_cast<const float4*>(pa[j]);
#pragma unroll
                for (int j = 0; j < 2; ++j) tb[j] = *reinterpret_cast<const float4*>(pb[j]);
            }
            if (more2) {
                advance();
#pragma unroll
                for (int j = 0; j < 4; ++j) ua[j] = *reinterpret_cast<const float4*>(pa[j]);
#pragma unroll
                for (int j = 0; j < 2; ++j) ub[j] = *reinterpret_cast<const float4*>(pb[j]);
            }
#pragma unroll
            for (int pc = 0; pc < 6; ++pc) { GLF_H8_PIECE(pc, 0, true, false) }
            if (more) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ra[j] = ta[j];
#pragma unroll
                for (int j = 0; j < 2; ++j) rb[j] = tb[j];
#pragma unroll
                for (int pc = 0; pc < 6; ++pc) { GLF_H8_PIECE(pc, 1, true, false) }
            }
            if (more2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ra[j] = ua[j];
#pragma unroll
                for (int j = 0; j < 2; ++j) rb[j] = ub[j];
            }
        }
        __syncthreads();
        f16x8 fb0h, fb1h, fb0l, fb1l, fa0h, fa0l, fa1h, fa1l;
#define GLF_H8_FRAGS(P, buf_, fo_)                                                                            \
        {                                                                                                     \
            const unsigned char* ab_ = smem_s + (buf_) * BUF8 + wm * 64 + (fo_);                              \
            const unsigned char* bb_ = smem_s + (buf_) * BUF8 + 2 * PL_A8 + wn * 64 + (fo_);                  \
            P##b0h = *reinterpret_cast<const f16x8*>(bb_);                                                    \
            P##b1h = *reinterpret_cast<const f16x8*>(bb_ + 32 * 64);                                          \
            P##a0h = *reinterpret_cast<const f16x8*>(ab_);                                                    \
            P##a1h = *reinterpret_cast<const f16x8*>(ab_ + 32 * 64);                                          \
            if (NP == 3) {                                                                                    \
                P##a0l = *reinterpret_cast<const f16x8*>(ab_ + PL_A8);                                        \
                P##b0l = *reinterpret_cast<const f16x8*>(bb_ + PL_B8);                                        \
                P##b1l = *reinterpret_cast<const f16x8*>(bb_ + 32 * 64 + PL_B8);                              \
                P##a1l = *reinterpret_cast<const f16x8*>(ab_ + 32 * 64 + PL_A8);                              \
            } else { P##a0l = P##a0h; P##b0l = P##b0h; P##b1l = P##b1h; P##a1l = P##a1h; }                    \
        }
        GLF_H8_FRAGS(f, 0, fo0)
        int cur = 0, nxt = 1, wr = 2;           // LDS buffers of tile it, it+1, it+2
        // CONV_/LOAD_/NEXT_ are compile-time constants: the steady-state body is straight-line code
#if defined(GLF_STAMPS) && GLF_STAMPS == 1
        unsigned long long st_[5] = {0, 0, 0, 0, 0};
        const bool stamp_on = args.partial != nullptr && blockIdx.x == gridDim.x / 2;
        unsigned long long* stamp_lds = reinterpret_cast<unsigned long long*>(smem_s + 3 * BUF8 + 16);
#define GLF_STAMP(k_) { __builtin_amdgcn_sched_barrier(0); st_[k_] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#define GLF_STAMP_FLUSH()                                                                                     \
            if (stamp_on && it >= 16 && it < 32 && lane == 0) {                                               \
                unsigned long long* d_ = stamp_lds + (wave * 16 + (it - 16)) * 8;                             \
                d_[0] = st_[0]; d_[1] = st_[1]; d_[2] = st_[2]; d_[3] = st_[3]; d_[4] = st_[4];               \
            }
#else
#define GLF_STAMP(k_)
#define GLF_STAMP_FLUSH()
#endif
#define GLF_H8_BODY(CONV_, LOAD_, NEXT_)                                                                      \
        {                                                                                                     \
            GLF_STAMP(0)                                                                                      \
            if (LOAD_) advance();                                                                             \
            f16x8 gb0h, gb1h, gb0l, gb1l, ga0h, ga0l, ga1h, ga1l;                                             \
            GLF_H8_FRAGS(g, cur, fo1)                                                                         \
            __builtin_amdgcn_sched_barrier(0);    /* keep the fragment reads up here (hipcc sinks them to their use) */ \
            GLF_H8_PIECE(0, wr, CONV_, LOAD_)                                                                 \
            GLF_ROW3(c00, c01, m00, m01, fa0h, fa0l, fb0h, fb0l, fb1h, fb1l)                                  \
            GLF_STAMP(1)                                                                                      \
            GLF_H8_PIECE(1, wr, CONV_, LOAD_)                                                                 \
            GLF_ROW3(c10, c11, m10, m11, fa1h, fa1l, fb0h, fb0l, fb1h, fb1l)                                  \
            GLF_H8_PIECE(2, wr, CONV_, LOAD_)                                                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            GLF_STAMP(2)                                                                                      \
            if (NEXT_) GLF_H8_FRAGS(f, nxt, fo0)                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            GLF_H8_PIECE(3, wr, CONV_, LOAD_)                                                                 \
            GLF_ROW3(c00, c01, m00, m01, ga0h, ga0l, gb0h, gb0l, gb1h, gb1l)                                  \
            GLF_STAMP(3)                                                                                      \
            GLF_H8_PIECE(4, wr, CONV_, LOAD_)                                                                 \
            GLF_ROW3(c10, c11, m10, m11, ga1h, ga1l, gb0h, gb0l, gb1h, gb1l)                                  \
            GLF_H8_PIECE(5, wr, CONV_, LOAD_)                                                                 \
            { const int t_ = cur; cur = nxt; nxt = wr; wr = t_; }                                             \
            GLF_STAMP(4)                                                                                      \
            __syncthreads();                                                                                  \
            GLF_STAMP_FLUSH()                                                                                 \
        }
// The iteration, instruction by instruction (GLF_IL_*: a slot = what is issued behind one MFMA, pinned by sched_barriers).
// A wave issues in order, so whatever sits between two of ITS MFMAs delays the second one unless it fits the ~24 issue cycles
// the first leaves free; in bursts (the compiler's choice: all fragment reads, then six MFMAs, then a whole conversion
// piece ...) the matrix pipe idles behind every burst -- in-kernel stamps showed 2 575 cycles per iteration for 1 536 cycles
// of MFMA work, and the eight waves' LDS / global bursts colliding.  Per wave and iteration: 24 MFMAs, 16 fragment reads,
// 6 staging pieces.  Slots 1-4: the k-step-1 fragments (two reads each); 5: pointer advance; 6-19: the staging pieces -- a
// pre-split operand's piece is one slot (LDS store of the registers loaded an iteration ago + their refill), a piece that
// still has to be split is cut into three (scale + high halves | residual | low halves + store + refill: 4-6 VALU each);
// 12-18 also carry the next tile's k-step-0 fragments, each into registers whose last reader has issued; the last MFMAs run
// with nothing behind them, so every LDS operation has landed when the barrier is reached.
#define GLF_IL_RD(P, w_, base_, off_) P##w_ = *reinterpret_cast<const f16x8*>((base_) + (off_));
#define GLF_IL_PIN() __builtin_amdgcn_sched_barrier(0);
#define GLF_IL_MM(c_, a_, b_) c_ = GLF_MFMA_F16(a_, b_, c_);
#define GLF_IL_ROW(c0, c1, m0, m1, ah, al, b0h, b0l, b1h, b1l, S1_, S2_, S3_, S4_, S5_, S6_)                   \
            GLF_IL_MM(c0, ah, b0h) GLF_IL_PIN() S1_ GLF_IL_PIN()                                              \
            GLF_IL_MM(c1, ah, b1h) GLF_IL_PIN() S2_ GLF_IL_PIN()                                              \
            if (NP == 3) { GLF_IL_MM(m0, al, b0h) GLF_IL_PIN() } S3_ GLF_IL_PIN()                             \
            if (NP == 3) { GLF_IL_MM(m1, al, b1h) GLF_IL_PIN() } S4_ GLF_IL_PIN()                             \
            if (NP == 3) { GLF_IL_MM(m0, ah, b0l) GLF_IL_PIN() } S5_ GLF_IL_PIN()                             \
            if (NP == 3) { GLF_IL_MM(m1, ah, b1l) GLF_IL_PIN() } S6_ GLF_IL_PIN()
        // the three stages of a piece that is split here (SRC_ = its float4, SC_ = the operand's scale)
        f32x2 sx01_, sx23_, sr01_, sr23_;
        f16x2 sh01_, sh23_;
#define GLF_IL_ST1(SRC_, SC_)                                                                                 \
            { const f32x2 s2_ = {SC_, SC_}; const f32x2 v01_ = {SRC_.x, SRC_.y}, v23_ = {SRC_.z, SRC_.w};     \
              sx01_ = v01_ * s2_; sx23_ = v23_ * s2_;                                                         \
              sh01_ = __builtin_convertvector(sx01_, f16x2); sh23_ = __builtin_convertvector(sx23_, f16x2); }
#define GLF_IL_ST2()                                                                                          \
            { const f32x2 k2_ = {2048.f, 2048.f};                                                             \
              sr01_ = (sx01_ - __builtin_convertvector(sh01_, f32x2)) * k2_;                                  \
              sr23_ = (sx23_ - __builtin_convertvector(sh23_, f32x2)) * k2_; }
#define GLF_IL_ST3(DST_, PL_)                                                                                 \
            { *reinterpret_cast<f16x4*>(DST_) = __builtin_shufflevector(sh01_, sh23_, 0, 1, 2, 3);            \
              if (NP == 3) *reinterpret_cast<f16x4*>((DST_) + (PL_)) =                                        \
                  __builtin_shufflevector(__builtin_convertvector(sr01_, f16x2), __builtin_convertvector(sr23_, f16x2), 0, 1, 2, 3); }
        // stage ST_ (1..3) of A piece J / B piece J of the tile being staged into buffer `wr`
#define GLF_IL_A(J, ST_, CONV_, LOAD_)                                                                        \
            if (PA) { if (ST_ == 3) { GLF_H8_PIECE(J, wr, CONV_, LOAD_) } }                                   \
            else if (CONV_) {                                                                                 \
                if (ST_ == 1) GLF_IL_ST1(ra[J], sc_a)                                                         \
                else if (ST_ == 2) GLF_IL_ST2()                                                               \
                else { GLF_IL_ST3(smem_s + wr * BUF8 + st_off + J * 64 * 64, PL_A8)                           \
                       if (LOAD_) ra[J] = *reinterpret_cast<const float4*>(pa[J]); }                          \
            }
#define GLF_IL_B(J, ST_, CONV_, LOAD_)                                                                        \
            if (BP) { if (ST_ == 3) { GLF_H8_PIECE(4 + J, wr, CONV_, LOAD_) } }                               \
            else if (CONV_) {                                                                                 \
                if (ST_ == 1) GLF_IL_ST1(rb[J], sc_b)                                                         \
                else if (ST_ == 2) GLF_IL_ST2()                                                               \
                else { GLF_IL_ST3(smem_s + wr * BUF8 + 2 * PL_A8 + st_off + J * 64 * 64, PL_B8)               \
                       if (LOAD_) GLF_H8_LOAD_B(J) }                                                          \
            }
// staging work item i_ of the iteration: the A pieces' stages, then the B pieces' (one item per pre-split piece, three per
// piece split here) -- items sit in consecutive slots from slot 6 on, so pre-split operands finish their LDS stores early
#define GLF_IL_ITEM(I_, CONV_, LOAD_)                                                                         \
            {                                                                                                 \
                constexpr int nA_ = PA ? 4 : 12, nB_ = BP ? 2 : 6, i_ = (I_);                                 \
                if constexpr (i_ < nA_) {                                                                     \
                    constexpr int j_ = PA ? i_ : i_ / 3, st_ = PA ? 3 : i_ % 3 + 1;                           \
                    GLF_IL_A(j_, st_, CONV_, LOAD_)                                                           \
                } else if constexpr (i_ < nA_ + nB_) {                                                        \
                    constexpr int k_ = i_ - nA_, j_ = BP ? k_ : k_ / 3, st_ = BP ? 3 : k_ % 3 + 1;            \
                    GLF_IL_B(j_, st_, CONV_, LOAD_)                                                           \
                }                                                                                             \
            }
#define GLF_H8_BODY_IL(CONV_, LOAD_, NEXT_)                                                                   \
        {                                                                                                     \
            GLF_STAMP(0)                                                                                      \
            f16x8 gb0h, gb1h, gb0l, gb1l, ga0h, ga0l, ga1h, ga1l;                                             \
            const unsigned char* ga_ = smem_s + cur * BUF8 + wm * 64 + fo1;                                   \
            const unsigned char* gb_ = smem_s + cur * BUF8 + 2 * PL_A8 + wn * 64 + fo1;                       \
            const unsigned char* na_ = smem_s + nxt * BUF8 + wm * 64 + fo0;                                   \
            const unsigned char* nb_ = smem_s + nxt * BUF8 + 2 * PL_A8 + wn * 64 + fo0;                       \
            GLF_IL_ROW(c00, c01, m00, m01, fa0h, fa0l, fb0h, fb0l, fb1h, fb1l,                                \
                { GLF_IL_RD(g, b0h, gb_, 0) GLF_IL_RD(g, a0h, ga_, 0) },                                      \
                { GLF_IL_RD(g, b1h, gb_, 32 * 64) if (NP == 3) { GLF_IL_RD(g, a0l, ga_, PL_A8) } },           \
                { if (NP == 3) { GLF_IL_RD(g, b0l, gb_, PL_B8) GLF_IL_RD(g, b1l, gb_, 32 * 64 + PL_B8) } },   \
                { GLF_IL_RD(g, a1h, ga_, 32 * 64) if (NP == 3) { GLF_IL_RD(g, a1l, ga_, 32 * 64 + PL_A8) } }, \
                { if (LOAD_) advance(); },                                                                    \
                { GLF_IL_ITEM(0, CONV_, LOAD_) })                                                             \
            GLF_STAMP(1)                                                                                      \
            GLF_IL_ROW(c10, c11, m10, m11, fa1h, fa1l, fb0h, fb0l, fb1h, fb1l,                                \
                { GLF_IL_ITEM(1, CONV_, LOAD_) },                                                             \
                { GLF_IL_ITEM(2, CONV_, LOAD_) },                                                             \
                { GLF_IL_ITEM(3, CONV_, LOAD_) },                                                             \
                { GLF_IL_ITEM(4, CONV_, LOAD_) },                                                             \
                { GLF_IL_ITEM(5, CONV_, LOAD_) },                                                             \
                { GLF_IL_ITEM(6, CONV_, LOAD_) if (NEXT_) { GLF_IL_RD(f, a0h, na_, 0) if (NP == 3) { GLF_IL_RD(f, a0l, na_, PL_A8) } } }) \
            if (NP != 3) { ga0l = ga0h; gb0l = gb0h; gb1l = gb1h; ga1l = ga1h; }                              \
            GLF_STAMP(2)                                                                                      \
            GLF_IL_ROW(c00, c01, m00, m01, ga0h, ga0l, gb0h, gb0l, gb1h, gb1l,                                \
                { GLF_IL_ITEM(7, CONV_, LOAD_) if (NEXT_) { GLF_IL_RD(f, b0h, nb_, 0) GLF_IL_RD(f, b1h, nb_, 32 * 64) } }, \
                { GLF_IL_ITEM(8, CONV_, LOAD_) if (NEXT_ && NP == 3) { GLF_IL_RD(f, b0l, nb_, PL_B8) GLF_IL_RD(f, b1l, nb_, 32 * 64 + PL_B8) } }, \
                { GLF_IL_ITEM(9, CONV_, LOAD_) if (NEXT_) { GLF_IL_RD(f, a1h, na_, 32 * 64) if (NP == 3) { GLF_IL_RD(f, a1l, na_, 32 * 64 + PL_A8) } } }, \
                { GLF_IL_ITEM(10, CONV_, LOAD_) },                                                            \
                { GLF_IL_ITEM(11, CONV_, LOAD_) },                                                            \
                { GLF_IL_ITEM(12, CONV_, LOAD_) })                                                            \
            GLF_STAMP(3)                                                                                      \
            GLF_IL_ROW(c10, c11, m10, m11, ga1h, ga1l, gb0h, gb0l, gb1h, gb1l,                                \
                { GLF_IL_ITEM(13, CONV_, LOAD_) },                                                            \
                { GLF_IL_ITEM(14, CONV_, LOAD_) },                                                            \
                { GLF_IL_ITEM(15, CONV_, LOAD_) },                                                            \
                { GLF_IL_ITEM(16, CONV_, LOAD_) },                                                            \
                { GLF_IL_ITEM(17, CONV_, LOAD_) },                                                            \
                {})                                                                                           \
            if (NP != 3 && NEXT_) { fa0l = fa0h; fb0l = fb0h; fb1l = fb1h; fa1l = fa1h; }                     \
            { const int t_ = cur; cur = nxt; nxt = wr; wr = t_; }                                             \
            GLF_STAMP(4)                                                                                      \
            __syncthreads();                                                                                  \
            GLF_STAMP_FLUSH()                                                                                 \
        }
        int it = 0;
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
        wg_t1 = __builtin_amdgcn_s_memtime();
#endif
        if (PA || BP || GLF_IL_ALL) {
            for (; it + 3 < ntiles; ++it) GLF_H8_BODY_IL(true, true, true)
            if (it + 2 < ntiles) { GLF_H8_BODY_IL(true, false, true) ++it; }
            if (it + 1 < ntiles) { GLF_H8_BODY_IL(false, false, true) ++it; }
            GLF_H8_BODY_IL(false, false, false)
        } else {
            for (; it + 3 < ntiles; ++it) GLF_H8_BODY(true, true, true)
            if (it + 2 < ntiles) { GLF_H8_BODY(true, false, true) ++it; }
            if (it + 1 < ntiles) { GLF_H8_BODY(false, false, true) ++it; }
            GLF_H8_BODY(false, false, false)
        }
#if defined(GLF_STAMPS) && GLF_STAMPS == 1
        if (stamp_on) {
            __syncthreads();
            for (int i = tid; i < 8 * 16 * 8; i += NT8) reinterpret_cast<unsigned long long*>(args.partial)[i] = stamp_lds[i];
        }
#endif
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
        wg_t2 = __builtin_amdgcn_s_memtime();
#endif
    }

    const RowsOut out{C, p_bias, args.res, args.colstats, args.colmax, args.amax_c, args.ld_res, p_bsc,
                      pN, p_ldc, p_accumulate, p_rect, args.relu, tn, g_hd, g_wd, p_alpha};
    rows_f16s_epilogue<BM8, WAVE_ROWS, EPI>(out, rt, smem_s, c00, c01, c10, c11, m00, m01, m10, m11);
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
    if (args.partial != nullptr && blockIdx.x == gridDim.x / 2) {
        __builtin_amdgcn_s_waitcnt(0);          // the stores of this wave's part of C have been accepted
        const unsigned long long wg_t3 = __builtin_amdgcn_s_memtime();
        if (lane == 0) {
            unsigned long long* d_ = reinterpret_cast<unsigned long long*>(args.partial) + wave * 4;
            d_[0] = wg_t0; d_[1] = wg_t1; d_[2] = wg_t2; d_[3] = wg_t3;
        }
    }
#endif
}

// ----------------------------------------------------------------------------------------------------------
// tn kernel: C_tap[m][n] (+)= alpha * sum_{r in slice} A[arow(r)][m] * B[src(r,tap)][n]
// planes [r][128 cols] with 320-byte rows, fragments transposed on the fly by ds_read_b64_tr_b16.
// ----------------------------------------------------------------------------------------------------------
constexpr int RST = 320;
constexpr int PLANE_T = 32 * RST;
constexpr int OPER_T = 2 * PLANE_T;
constexpr size_t SMEM_TN_H = 2 * OPER_T + 32 * sizeof(int);

// SMALL: tile 64 x 64 -- every wave owns ONE 32 x 32 accumulator pair instead of a 64 x 64 quadrant, and a staging pass loads
// 64 columns per operand row instead of 128.  For the layer-1 weight gradients (M, N = 64 ... 256 with one of them 64, K = 193 600
// rows): on the 128 x 128 tile three of four MFMAs multiplied zero-page columns (64 x 64 x 193 600, nine taps: 0.32 ms at 45 TF).
template <bool GATHER, int NP, bool PA = false, bool PB = false, bool SMALL = false>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_f16s_kernel(const GemmArgs args) {
    constexpr int TBM = SMALL ? 64 : BM, TBN = SMALL ? 64 : BN, WT = SMALL ? 32 : 64;
    const int pM = args.M, pN = args.N, pK = args.K, p_lda = args.lda, p_ldb = args.ldb, p_ldc = args.ldc;
    const int p_accumulate = args.accumulate, p_split = args.split;
    const int p_tiles_n = args.tiles_n;
    const unsigned p_tap_mask = args.tap_mask;
    const long long p_tsb = args.tap_stride_b, p_bsa = args.bsa, p_bsb = args.bsb, p_bsc = args.bsc;
    const float* __restrict__ p_A = args.A; const float* __restrict__ p_B = args.B;
    float* __restrict__ p_C = args.C;
    const float* __restrict__ p_zero = args.zeros;
    const int g_hs = args.g.hs, g_ws = args.g.ws, g_hd = args.g.hd, g_wd = args.g.wd, g_kw = args.g.kw;
    const int g_stride = args.g.stride, g_pad = args.g.pad, g_dil = args.g.dil;
    const int g_nimg = args.g.n_img, p_rect = GATHER ? args.rect : 0;
    float sc_a, sc_b, inv_a, inv_b;
    pow2_scale(args.amax_a, sc_a, inv_a);
    pow2_scale(args.amax_b, sc_b, inv_b);
    const float p_alpha = args.alpha * inv_a * inv_b;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    unsigned char* As = smem_s;
    unsigned char* Bs = smem_s + OPER_T;
    int* vflag = reinterpret_cast<int*>(smem_s + 2 * OPER_T);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * WT, wn = (wave & 1) * WT;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = bid % p_tiles_n, tm = bid / p_tiles_n;
    const int tap = tn_tap(p_tap_mask, blockIdx.y);
    TnSlice ts;
    if (!tn_slice<BK, false>(ts, blockIdx.z, p_split, pK, p_rect, tap, Geo{g_nimg, g_hs, g_ws, g_hd, g_wd, 0, g_kw, g_stride, g_pad, g_dil})) return;
    const int r0 = ts.r0, r1 = ts.r1;
    int tap_cy = 0, tap_cx = 0;  // (a const TnGather from offsets computed first: filling cy / cx in afterwards cost the 64 x 64 form two VGPRs)
    if (GATHER) tn_tap_offsets(tap, g_kw, g_pad, g_dil, tap_cy, tap_cx);
    const TnGather tg{ts.y0, ts.x0, ts.h, ts.w, g_hs, g_ws, g_hd, g_wd, g_stride, tap_cy, tap_cx};
    const float* __restrict__ A = p_A + (long long)ts.bz * p_bsa;
    const float* __restrict__ B = p_B + (long long)ts.bz * p_bsb;

    // staging map: a row of the tile is TBM (= TBN) floats = TBM / 4 threads; NTHREADS / (TBM / 4) rows per pass, 32 rows per tile
    constexpr int TPR = TBM / 4, RPP = NTHREADS / TPR, NPASS = 32 / RPP;          // 32 threads x 8 rows x 4 passes | 16 x 16 x 2
    const int c4 = tid % TPR, rr = tid / TPR;
    const int m0 = tm * TBM + 4 * c4, n0 = tn * TBN + 4 * c4;
    const int m0c = min(m0, pM - 4), n0c = min(n0, pN - 4);

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    f32x16 m00 = {0}, m01 = {0}, m10 = {0}, m11 = {0};
    float4 ra[NPASS], rb[NPASS];
    int rvalid[NPASS];

    TnRows<NPASS> gs = {};       // this thread's rows of the NEXT tile to load
    if (GATHER) tn_rows_init<NPASS, RPP>(gs, r0 + rr, tg);
    auto load_tile = [&](int rbase) __attribute__((always_inline)) {
        long long src[NPASS], arow[NPASS];
#pragma unroll
        for (int j = 0; j < NPASS; ++j) {
            const int r = rbase + rr + RPP * j;
            src[j] = -1;
            arow[j] = min(r, r1 - 1);
            if (GATHER) {
                if (r < r1) {
                    int sr;
                    arow[j] = tn_row_dst(gs, j, tg);
                    if (tn_row_src(gs, j, tg, sr)) src[j] = sr;
                }
                tn_row_step<BK>(gs, j, tg);
            } else if (r < r1) {
                src[j] = r;
            }
            rvalid[j] = src[j] >= 0;
        }
#pragma unroll
        for (int j = 0; j < NPASS; ++j) {
            // rows beyond the slice / in the conv padding and the column overhang read the zero page
            ra[j] = *reinterpret_cast<const float4*>((src[j] >= 0 && m0 < pM ? A + arow[j] * p_lda : p_zero) + m0c);
            rb[j] = *reinterpret_cast<const float4*>((src[j] >= 0 && n0 < pN ? B + src[j] * p_ldb : p_zero) + n0c);
        }
    };
#define GLF_HT_STORE(J)                                                                                    \
    {                                                                                                      \
        const SplitH sa = PA ? unpack4h(ra[J]) : split4h(ra[J], sc_a);                                     \
        const SplitH sb = PB ? unpack4h(rb[J]) : split4h(rb[J], sc_b);                                     \
        unsigned char* da = As + (rr + RPP * J) * RST + c4 * 8;                                            \
        unsigned char* db = Bs + (rr + RPP * J) * RST + c4 * 8;                                            \
        *reinterpret_cast<f16x4*>(da) = sa.h; if (NP == 3) *reinterpret_cast<f16x4*>(da + PLANE_T) = sa.l; \
        *reinterpret_cast<f16x4*>(db) = sb.h; if (NP == 3) *reinterpret_cast<f16x4*>(db + PLANE_T) = sb.l; \
        if (c4 == 0) vflag[rr + RPP * J] = rvalid[J];                                                      \
    }

    // transposing fragment read (see gemm_bf16s.hip): group g of 16 lanes: columns 16*(g&1).., k half g>>1
    const int grp = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int tr_off = (8 * (grp >> 1) + q) * RST + (16 * (grp & 1) + 4 * pp) * 2;
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
#define GLF_HTR_FRAG(base, dst)                                                                             \
    {                                                                                                       \
        const s16x4 lo_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(base));                       \
        const s16x4 hi_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)((base) + 4 * RST));          \
        typedef short s16x8_ __attribute__((ext_vector_type(8)));                                           \
        const s16x8_ both_ = __builtin_shufflevector(lo_, hi_, 0, 1, 2, 3, 4, 5, 6, 7);                     \
        dst = __builtin_bit_cast(f16x8, both_);                                                             \
    }

    load_tile(r0);
    for (int rbase = r0; rbase < r1; rbase += BK) {
        GLF_HT_STORE(0) GLF_HT_STORE(1)
        if constexpr (NPASS == 4) { GLF_HT_STORE(2) GLF_HT_STORE(3) }
        __syncthreads();
        if (rbase + BK < r1) load_tile(rbase + BK);
        const bool any = __ballot(vflag[lane & 31] != 0) != 0ull;
        if (any) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const unsigned char* ab = As + s * 16 * RST + wm * 2 + tr_off;
                const unsigned char* bb = Bs + s * 16 * RST + wn * 2 + tr_off;
                if constexpr (SMALL) {
                    f16x8 ah, al, bh, bl;
                    GLF_HTR_FRAG(ab, ah) GLF_HTR_FRAG(ab + PLANE_T, al) GLF_HTR_FRAG(bb, bh) GLF_HTR_FRAG(bb + PLANE_T, bl)
                    c00 = GLF_MFMA_F16(ah, bh, c00);
                    if (NP == 3) { m00 = GLF_MFMA_F16(al, bh, m00); m00 = GLF_MFMA_F16(ah, bl, m00); }
                } else {
                    f16x8 b0h, b0l, b1h, b1l;
                    GLF_HTR_FRAG(bb, b0h) GLF_HTR_FRAG(bb + 64, b1h) GLF_HTR_FRAG(bb + PLANE_T, b0l) GLF_HTR_FRAG(bb + 64 + PLANE_T, b1l)
                    {
                        f16x8 ah, al;
                        GLF_HTR_FRAG(ab, ah) GLF_HTR_FRAG(ab + PLANE_T, al)
                        GLF_ROW3(c00, c01, m00, m01, ah, al, b0h, b0l, b1h, b1l)
                    }
                    {
                        f16x8 ah, al;
                        GLF_HTR_FRAG(ab + 64, ah) GLF_HTR_FRAG(ab + 64 + PLANE_T, al)
                        GLF_ROW3(c10, c11, m10, m11, ah, al, b0h, b0l, b1h, b1l)
                    }
                }
            }
        }
        __syncthreads();
    }

    const TnOut out = tn_out(args.partial, p_C, args.amax_c, pM, pN, p_ldc, p_bsc, p_tsb, ts.bz, tap, p_split, p_accumulate, tm, tn, p_alpha);
    float cmax = 0.f;
    tn_emit<TBM, TBN>(out, c00 + m00 * 0x1p-11f, wm, wn, cmax);
    if constexpr (!SMALL) {
        tn_emit<TBM, TBN>(out, c01 + m01 * 0x1p-11f, wm, wn + 32, cmax);
        tn_emit<TBM, TBN>(out, c10 + m10 * 0x1p-11f, wm + 32, wn, cmax); tn_emit<TBM, TBN>(out, c11 + m11 * 0x1p-11f, wm + 32, wn + 32, cmax);
    }
    tn_amax<true>(out.amax_c, cmax);
}

// ----------------------------------------------------------------------------------------------------------
// tn kernel, 8 waves: tile 256 (A columns) x 128 (B columns) x 32 rows, THREE LDS buffers and the slot-interleaved software
// pipeline of the rows kernel (tile t multiplied out of buffer t%3 with its k-step-0 fragments read before the barrier,
// tile t+2 converted into buffer (t+2)%3, tile t+3 in flight from global memory).  Planes are [r][cols] with dense rows
// (512 bytes for A, 256 for B: 48 KB per buffer) and the 64-byte chunks of a row XOR-swizzled with (row & 3): the
// transposing ds_read_b64_tr_b16 fragment reads (four rows x 64 bytes per half wave) and the 8-byte staging writes are
// conflict-free without padding.  Row coordinates (n, y, x) advance incrementally by 32 per tile; rows outside the slice,
// in the conv padding or in the column overhang are loaded from the zero page.
// Used when M > 128 (otherwise half of the 256-wide tile would be idle and the 128 x 128 kernel above runs).
// ----------------------------------------------------------------------------------------------------------
constexpr int TM8 = 256;
constexpr int RSA = 512, RSB = 256;
constexpr int PA8 = 32 * RSA, PB8 = 32 * RSB;
constexpr int TBUF8 = 2 * PA8 + 2 * PB8;
constexpr size_t SMEM_TN_H8 = 3 * TBUF8;

template <bool GATHER, int NP, bool PA = false, bool PB = false>
__global__ __launch_bounds__(NT8, 2) void gemm_tn_f16s8_kernel(const GemmArgs args) {
    const int pM = args.M, pN = args.N, pK = args.K, p_lda = args.lda, p_ldb = args.ldb, p_ldc = args.ldc;
    const int p_accumulate = args.accumulate, p_split = args.split;
    const int p_tiles_n = args.tiles_n;
    const unsigned p_tap_mask = args.tap_mask;
    const long long p_tsb = args.tap_stride_b, p_bsa = args.bsa, p_bsb = args.bsb, p_bsc = args.bsc;
    const float* __restrict__ p_A = args.A; const float* __restrict__ p_B = args.B;
    float* __restrict__ p_C = args.C;
    const float* __restrict__ p_zero = args.zeros;
    const int g_hs = args.g.hs, g_ws = args.g.ws, g_hd = args.g.hd, g_wd = args.g.wd, g_kw = args.g.kw;
    const int g_stride = args.g.stride, g_pad = args.g.pad, g_dil = args.g.dil;
    const int g_nimg = args.g.n_img, p_rect = GATHER ? args.rect : 0;
    float sc_a, sc_b, inv_a, inv_b;
    pow2_scale(args.amax_a, sc_a, inv_a);
    pow2_scale(args.amax_b, sc_b, inv_b);
    const float p_alpha = args.alpha * inv_a * inv_b;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
    unsigned long long wg_t0 = __builtin_amdgcn_s_memtime(), wg_t1 = 0, wg_t2 = 0;
#endif

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform, and known to be: everything derived from it stays in SGPRs
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = bid % p_tiles_n, tm = bid / p_tiles_n;
    const int tap = tn_tap(p_tap_mask, blockIdx.y);
    TnSlice ts;
    if (!tn_slice<BK, false>(ts, blockIdx.z, p_split, pK, p_rect, tap, Geo{g_nimg, g_hs, g_ws, g_hd, g_wd, 0, g_kw, g_stride, g_pad, g_dil})) return;
    const TnOut out = tn_out(args.partial, p_C, args.amax_c, pM, pN, p_ldc, p_bsc, p_tsb, ts.bz, tap, p_split, p_accumulate, tm, tn, p_alpha);      // (here, not at the stores: one VGPR less)
    const int r0 = ts.r0, r1 = ts.r1;
    int tap_cy = 0, tap_cx = 0;
    if (GATHER) tn_tap_offsets(tap, g_kw, g_pad, g_dil, tap_cy, tap_cx);
    const TnGather tg{ts.y0, ts.x0, ts.h, ts.w, g_hs, g_ws, g_hd, g_wd, g_stride, tap_cy, tap_cx};
    const float* __restrict__ A = p_A + (long long)ts.bz * p_bsa;
    const float* __restrict__ B = p_B + (long long)ts.bz * p_bsb;
    const int ntiles = (r1 - r0 + BK - 1) / BK;

    // staging map: A tile 32 x 256 floats = 4 float4 per thread (rows ra0 + 8 j, column ca), B tile 32 x 128 = 2 (rows rb0 + 16 j).
    // ra0 is the wave index: an A row, its pixel coordinates and its base pointer are WAVE-UNIFORM and live in SGPRs (the
    // kernel sits at the 256-register limit: per-lane copies of that state spilled into the main loop, and a scratch reload
    // between the global loads turns every s_waitcnt vmcnt(5) into vmcnt(0)); a lane adds only its column offset.  Lanes in the
    // column overhang (m0 >= M) read column 0 instead: they feed accumulator columns that are never stored.
    const int ca = tid & 63, ra0 = wave;
    const int cb = tid & 31, rb0 = tid >> 5;
    const int m0 = tm * TM8 + 4 * ca, n0 = tn * BN + 4 * cb;
    const bool a_col_ok = m0 < pM, b_col_ok = n0 < pN;
    const unsigned a_col = a_col_ok ? (unsigned)m0 : 0u;
    const float* __restrict__ Bc = B + (b_col_ok ? n0 : 0);
    const float* __restrict__ zb = p_zero + (b_col_ok ? n0 : 0);

    // current row index and (for conv gathers) its pixel coordinates inside the rectangle, per staged row.  The A rows start at
    // r0 + wave: their state is wave-uniform (outside rect mode row r of A is pixel r: no state at all)
    int ar[4], br[2];
    TnRows<4> as = {};
    TnRows<2> bs = {};
#pragma unroll
    for (int j = 0; j < 4; ++j) ar[j] = r0 + ra0 + 8 * j;
#pragma unroll
    for (int j = 0; j < 2; ++j) br[j] = r0 + rb0 + 16 * j;
    if (GATHER && p_rect) tn_rows_init<4, 8>(as, r0 + ra0, tg);
    if (GATHER) tn_rows_init<2, 16>(bs, r0 + rb0, tg);
    const float* pa[4];          // row bases (uniform); the lane's column offset a_col is added at the load
    const float* pb[2];
    // pointers of the NEXT tile to load, then step every row by 32
    auto advance = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = ar[j] < r1;
            long long arow = ar[j];
            if (GATHER && p_rect) arow = tn_row_dst(as, j, tg);
            pa[j] = ok ? A + arow * p_lda : p_zero;
            ar[j] += BK;
            if (GATHER && p_rect) tn_row_step<BK>(as, j, tg);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            long long src = br[j];
            bool ok = br[j] < r1 && b_col_ok;
            if (GATHER) {
                int sr;
                ok = tn_row_src(bs, j, tg, sr) && ok;
                src = sr;
            }
            pb[j] = ok ? Bc + src * p_ldb : zb;
            br[j] += BK;
            if (GATHER) tn_row_step<BK>(bs, j, tg);
        }
    };

    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    f32x16 m00 = {0}, m01 = {0}, m10 = {0}, m11 = {0};
    float4 ra[4], rb[2];
    // swizzled staging offsets: 8-byte unit ca of row ra0 + 8 j (A) / unit cb of row rb0 + 16 j (B): (row & 3) is the thread's own
    const int st_a = ra0 * RSA + ((((ca >> 3) ^ (ra0 & 3)) << 6) | ((ca & 7) << 3));
    const int st_b = rb0 * RSB + ((((cb >> 3) ^ (rb0 & 3)) << 6) | ((cb & 7) << 3));
#define GLF_T8_CONV_A(J, buf_)                                                                               \
    {                                                                                                        \
        const SplitH s = PA ? unpack4h(ra[J]) : split4h(ra[J], sc_a);                                        \
        unsigned char* d = smem_s + (buf_) * TBUF8 + st_a + J * 8 * RSA;                                     \
        *reinterpret_cast<f16x4*>(d) = s.h; if (NP == 3) *reinterpret_cast<f16x4*>(d + PA8) = s.l;           \
    }
#define GLF_T8_CONV_B(J, buf_)                                                                               \
    {                                                                                                        \
        const SplitH s = PB ? unpack4h(rb[J]) : split4h(rb[J], sc_b);                                        \
        unsigned char* d = smem_s + (buf_) * TBUF8 + 2 * PA8 + st_b + J * 16 * RSB;                          \
        *reinterpret_cast<f16x4*>(d) = s.h; if (NP == 3) *reinterpret_cast<f16x4*>(d + PB8) = s.l;           \
    }
    // (a pre-split piece: the store stays ahead of the load that refills its registers -- see GLF_H8_PIN)
#define GLF_T8_PIECE(pc, buf_, conv_, load_)                                                                 \
    switch (pc) {                                                                                            \
        case 0: if (conv_) GLF_T8_CONV_A(0, buf_) GLF_H8_PIN(PA) if (load_) ra[0] = *reinterpret_cast<const float4*>(pa[0] + a_col); GLF_H8_PIN(PA) break; \
        case 1: if (conv_) GLF_T8_CONV_A(1, buf_) GLF_H8_PIN(PA) if (load_) ra[1] = *reinterpret_cast<const float4*>(pa[1] + a_col); GLF_H8_PIN(PA) break; \
        case 2: if (conv_) GLF_T8_CONV_A(2, buf_) GLF_H8_PIN(PA) if (load_) ra[2] = *reinterpret_cast<const float4*>(pa[2] + a_col); GLF_H8_PIN(PA) break; \
        case 3: if (conv_) GLF_T8_CONV_A(3, buf_) GLF_H8_PIN(PA) if (load_) ra[3] = *reinterpret_cast<const float4*>(pa[3] + a_col); GLF_H8_PIN(PA) break; \
        case 4: if (conv_) GLF_T8_CONV_B(0, buf_) GLF_H8_PIN(PB) if (load_) rb[0] = *reinterpret_cast<const float4*>(pb[0]); GLF_H8_PIN(PB) break; \
        default: if (conv_) GLF_T8_CONV_B(1, buf_) GLF_H8_PIN(PB) if (load_) rb[1] = *reinterpret_cast<const float4*>(pb[1]); GLF_H8_PIN(PB) break; \
    }

    // transposing fragment reads (see gemm_bf16s.hip): group g of 16 lanes: columns 16*(g&1).., k half g>>1; the lane's rows
    // are q and q + 4 (mod 8), so its swizzle key is q
    const int grp = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int tr_in = 32 * (grp & 1) + 8 * pp;
    const int tr_a0 = (8 * (grp >> 1) + q) * RSA + ((((wm >> 5) + 0) ^ q) << 6) + tr_in;       // columns wm .. wm + 31
    const int tr_a1 = (8 * (grp >> 1) + q) * RSA + ((((wm >> 5) + 1) ^ q) << 6) + tr_in;       // columns wm + 32 .. wm + 63
    const int tr_b0 = (8 * (grp >> 1) + q) * RSB + ((((wn >> 5) + 0) ^ q) << 6) + tr_in;
    const int tr_b1 = (8 * (grp >> 1) + q) * RSB + ((((wn >> 5) + 1) ^ q) << 6) + tr_in;
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
#define GLF_T8_FRAG(base, RS_, dst)                                                                         \
    {                                                                                                       \
        const s16x4 lo_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(base));                       \
        const s16x4 hi_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)((base) + 4 * RS_));          \
        typedef short s16x8_ __attribute__((ext_vector_type(8)));                                           \
        const s16x8_ both_ = __builtin_shufflevector(lo_, hi_, 0, 1, 2, 3, 4, 5, 6, 7);                     \
        dst = __builtin_bit_cast(f16x8, both_);                                                             \
    }
    // fragment w_ of set P (f = k-step 0, g = k-step 1) of the tile in buffer buf_
#define GLF_TL_A(P, w_, buf_, ks_, off_, pl_) GLF_T8_FRAG(smem_s + (buf_) * TBUF8 + (ks_) * 16 * RSA + (off_) + (pl_), RSA, P##w_)
#define GLF_TL_B(P, w_, buf_, ks_, off_, pl_) GLF_T8_FRAG(smem_s + (buf_) * TBUF8 + 2 * PA8 + (ks_) * 16 * RSB + (off_) + (pl_), RSB, P##w_)

    if (ntiles <= 0) return;
    // prologue: tiles 0 and 1 -> buffers 0 and 1, tile 2 raw in registers, the k-step-0 fragments of tile 0 in f*
    advance();
#pragma unroll
    for (int pc = 0; pc < 6; ++pc) { GLF_T8_PIECE(pc, 0, false, true) }
    {
        const bool more = ntiles > 1;
        if (more) advance();
#pragma unroll
        for (int pc = 0; pc < 6; ++pc) { GLF_T8_PIECE(pc, 0, true, more) }
        if (more) {
            const bool more2 = ntiles > 2;
            if (more2) advance();
#pragma unroll
            for (int pc = 0; pc < 6; ++pc) { GLF_T8_PIECE(pc, 1, true, more2) }
        }
    }
    __syncthreads();
    f16x8 fb0h, fb1h, fb0l, fb1l, fa0h, fa0l, fa1h, fa1l;
    GLF_TL_B(f, b0h, 0, 0, tr_b0, 0) GLF_TL_B(f, b1h, 0, 0, tr_b1, 0) GLF_TL_A(f, a0h, 0, 0, tr_a0, 0) GLF_TL_A(f, a1h, 0, 0, tr_a1, 0)
    if (NP == 3) {
        GLF_TL_A(f, a0l, 0, 0, tr_a0, PA8) GLF_TL_B(f, b0l, 0, 0, tr_b0, PB8) GLF_TL_B(f, b1l, 0, 0, tr_b1, PB8) GLF_TL_A(f, a1l, 0, 0, tr_a1, PA8)
    } else { fa0l = fa0h; fb0l = fb0h; fb1l = fb1h; fa1l = fa1h; }
    int cur = 0, nxt = 1, wr = 2;           // LDS buffers of tile it, it+1, it+2
    // staging work items as in the rows kernel (GLF_IL_ITEM): one slot per pre-split piece, three per piece split here
    f32x2 sx01_, sx23_, sr01_, sr23_;
    f16x2 sh01_, sh23_;
#define GLF_TL_SA(J, ST_, CONV_, LOAD_)                                                                       \
            if (PA) { if (ST_ == 3) { GLF_T8_PIECE(J, wr, CONV_, LOAD_) } }                                   \
            else if (CONV_) {                                                                                 \
                if (ST_ == 1) GLF_IL_ST1(ra[J], sc_a)                                                         \
                else if (ST_ == 2) GLF_IL_ST2()                                                               \
                else { GLF_IL_ST3(smem_s + wr * TBUF8 + st_a + J * 8 * RSA, PA8)                              \
                       if (LOAD_) ra[J] = *reinterpret_cast<const float4*>(pa[J] + a_col); }                  \
            }
#define GLF_TL_SB(J, ST_, CONV_, LOAD_)                                                                       \
            if (PB) { if (ST_ == 3) { GLF_T8_PIECE(4 + J, wr, CONV_, LOAD_) } }                               \
            else if (CONV_) {                                                                                 \
                if (ST_ == 1) GLF_IL_ST1(rb[J], sc_b)                                                         \
                else if (ST_ == 2) GLF_IL_ST2()                                                               \
                else { GLF_IL_ST3(smem_s + wr * TBUF8 + 2 * PA8 + st_b + J * 16 * RSB, PB8)                   \
                       if (LOAD_) rb[J] = *reinterpret_cast<const float4*>(pb[J]); }                          \
            }
#define GLF_TL_ITEM(I_, CONV_, LOAD_)                                                                         \
            {                                                                                                 \
                constexpr int nA_ = PA ? 4 : 12, nB_ = PB ? 2 : 6, i_ = (I_);                                 \
                if constexpr (i_ < nA_) {                                                                     \
                    constexpr int j_ = PA ? i_ : i_ / 3, st_ = PA ? 3 : i_ % 3 + 1;                           \
                    GLF_TL_SA(j_, st_, CONV_, LOAD_)                                                          \
                } else if constexpr (i_ < nA_ + nB_) {                                                        \
                    constexpr int k_ = i_ - nA_, j_ = PB ? k_ : k_ / 3, st_ = PB ? 3 : k_ % 3 + 1;            \
                    GLF_TL_SB(j_, st_, CONV_, LOAD_)                                                          \
                }                                                                                             \
            }
#define GLF_T8_BODY(CONV_, LOAD_, NEXT_)                                                                      \
    {                                                                                                         \
        f16x8 gb0h, gb1h, gb0l, gb1l, ga0h, ga0l, ga1h, ga1l;                                                 \
        GLF_IL_ROW(c00, c01, m00, m01, fa0h, fa0l, fb0h, fb0l, fb1h, fb1l,                                    \
            { GLF_TL_B(g, b0h, cur, 1, tr_b0, 0) GLF_TL_A(g, a0h, cur, 1, tr_a0, 0) },                        \
            { GLF_TL_B(g, b1h, cur, 1, tr_b1, 0) if (NP == 3) { GLF_TL_A(g, a0l, cur, 1, tr_a0, PA8) } },     \
            { if (NP == 3) { GLF_TL_B(g, b0l, cur, 1, tr_b0, PB8) GLF_TL_B(g, b1l, cur, 1, tr_b1, PB8) } },   \
            { GLF_TL_A(g, a1h, cur, 1, tr_a1, 0) if (NP == 3) { GLF_TL_A(g, a1l, cur, 1, tr_a1, PA8) } },     \
            { if (LOAD_) advance(); },                                                                        \
            { GLF_TL_ITEM(0, CONV_, LOAD_) })                                                                 \
        GLF_IL_ROW(c10, c11, m10, m11, fa1h, fa1l, fb0h, fb0l, fb1h, fb1l,                                    \
            { GLF_TL_ITEM(1, CONV_, LOAD_) },                                                                 \
            { GLF_TL_ITEM(2, CONV_, LOAD_) },                                                                 \
            { GLF_TL_ITEM(3, CONV_, LOAD_) },                                                                 \
            { GLF_TL_ITEM(4, CONV_, LOAD_) },                                                                 \
            { GLF_TL_ITEM(5, CONV_, LOAD_) },                                                                 \
            { GLF_TL_ITEM(6, CONV_, LOAD_) if (NEXT_) { GLF_TL_A(f, a0h, nxt, 0, tr_a0, 0) if (NP == 3) { GLF_TL_A(f, a0l, nxt, 0, tr_a0, PA8) } } }) \
        if (NP != 3) { ga0l = ga0h; gb0l = gb0h; gb1l = gb1h; ga1l = ga1h; }                                  \
        GLF_IL_ROW(c00, c01, m00, m01, ga0h, ga0l, gb0h, gb0l, gb1h, gb1l,                                    \
            { GLF_TL_ITEM(7, CONV_, LOAD_) if (NEXT_) { GLF_TL_B(f, b0h, nxt, 0, tr_b0, 0) GLF_TL_B(f, b1h, nxt, 0, tr_b1, 0) } }, \
            { GLF_TL_ITEM(8, CONV_, LOAD_) if (NEXT_ && NP == 3) { GLF_TL_B(f, b0l, nxt, 0, tr_b0, PB8) GLF_TL_B(f, b1l, nxt, 0, tr_b1, PB8) } }, \
            { GLF_TL_ITEM(9, CONV_, LOAD_) if (NEXT_) { GLF_TL_A(f, a1h, nxt, 0, tr_a1, 0) if (NP == 3) { GLF_TL_A(f, a1l, nxt, 0, tr_a1, PA8) } } }, \
            { GLF_TL_ITEM(10, CONV_, LOAD_) },                                                                \
            { GLF_TL_ITEM(11, CONV_, LOAD_) },                                                                \
            { GLF_TL_ITEM(12, CONV_, LOAD_) })                                                                \
        GLF_IL_ROW(c10, c11, m10, m11, ga1h, ga1l, gb0h, gb0l, gb1h, gb1l,                                    \
            { GLF_TL_ITEM(13, CONV_, LOAD_) },                                                                \
            { GLF_TL_ITEM(14, CONV_, LOAD_) },                                                                \
            { GLF_TL_ITEM(15, CONV_, LOAD_) },                                                                \
            { GLF_TL_ITEM(16, CONV_, LOAD_) },                                                                \
            { GLF_TL_ITEM(17, CONV_, LOAD_) },                                                                \
            {})                                                                                               \
        if (NP != 3 && NEXT_) { fa0l = fa0h; fb0l = fb0h; fb1l = fb1h; fa1l = fa1h; }                         \
        { const int t_ = cur; cur = nxt; nxt = wr; wr = t_; }                                                 \
        __syncthreads();                                                                                      \
    }
    int it = 0;
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
    wg_t1 = __builtin_amdgcn_s_memtime();
#endif
    for (; it + 3 < ntiles; ++it) GLF_T8_BODY(true, true, true)
    if (it + 2 < ntiles) { GLF_T8_BODY(true, false, true) ++it; }
    if (it + 1 < ntiles) { GLF_T8_BODY(false, false, true) ++it; }
    GLF_T8_BODY(false, false, false)
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
    wg_t2 = __builtin_amdgcn_s_memtime();
#endif

    float cmax = 0.f;
    tn_emit<TM8, BN>(out, c00 + m00 * 0x1p-11f, wm, wn, cmax); tn_emit<TM8, BN>(out, c01 + m01 * 0x1p-11f, wm, wn + 32, cmax);
    tn_emit<TM8, BN>(out, c10 + m10 * 0x1p-11f, wm + 32, wn, cmax); tn_emit<TM8, BN>(out, c11 + m11 * 0x1p-11f, wm + 32, wn + 32, cmax);
    tn_amax<true>(out.amax_c, cmax);
#if defined(GLF_STAMPS) && GLF_STAMPS == 2
    if (args.stamps != nullptr && blockIdx.x == gridDim.x / 2 && blockIdx.z == 0 && blockIdx.y == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long wg_t3 = __builtin_amdgcn_s_memtime();
        if (lane == 0) {
            unsigned long long* d_ = args.stamps + 64 + wave * 4;
            d_[0] = wg_t0; d_[1] = wg_t1; d_[2] = wg_t2; d_[3] = wg_t3; if (wave == 0) args.stamps[63] = (unsigned long long)ntiles;
        }
    }
#endif
}

// max |x| over a [rows, cols] view (row stride ld) -> *out (non-negative floats order like their bit patterns)
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long long rows, int cols, long long ld,
                                                   int vec, unsigned* __restrict__ out) {
    const int c4n = vec ? cols >> 2 : 0;
    const long long total4 = rows * c4n;
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / c4n;
        const int c = (int)(i - r * c4n) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    const int tail = cols - 4 * c4n;
    if (tail) {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows * tail; i += (long long)gridDim.x * blockDim.x) {
            const long long r = i / tail;
            m = fmaxf(m, fabsf(x[r * ld + (cols - tail) + (int)(i - r * tail)]));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        if (m > 0.f) atomicMax(out, __float_as_uint(m));
    }
}

// x [rows][cols] (row stride ld, cols % 4 == 0) -> the packed pre-split image out (row stride ldo): every float4 of x
// becomes {h0 h1 h2 h3 l0 l1 l2 l3}, x * s = h + 2^-11 l, s = the power of two pow2_scale() derives from *amax -- exactly
// what the contraction kernels compute in their staging path
__global__ __launch_bounds__(256) void split_packed_kernel(const float* __restrict__ x, long long rows, int cols4, long long ld,
                                                           const float* __restrict__ amax, float* __restrict__ out, long long ldo) {
    float sc, inv;
    pow2_scale(amax, sc, inv);
    const long long total = rows * cols4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cols4;
        const int c = (int)(i - r * cols4) * 4;
        const SplitH s = split4h(*reinterpret_cast<const float4*>(x + r * ld + c), sc);
        const float2 h = __builtin_bit_cast(float2, s.h), l = __builtin_bit_cast(float2, s.l);
        *reinterpret_cast<float4*>(out + r * ldo + c) = make_float4(h.x, h.y, l.x, l.y);
    }
}


// split_packed_kernel that ALSO leaves the column sums of x (a bias gradient read off the pass that packs the output gradient).
// The grid-stride walk above owns no columns, so this one is column-owning like the BatchNorm applies: a workgroup covers `tpr`
// float4 columns and one slice of rows, a thread keeps its four columns for the whole kernel and walks down its rows with four
// rows' loads in flight.  Sums: fp32 over at most 64 of the thread's rows, then double; the workgroup's row lanes are folded in a
// fixed order through LDS into partial[slice][cols]; split_colsum_finalize folds the slices.  No atomics.
constexpr int SC_FLUSH = 64;
__global__ __launch_bounds__(256) void split_packed_colsum_kernel(const float* __restrict__ x, int rows, int cols4, long long ld,
                                                                  const float* __restrict__ amax, float* __restrict__ out, long long ldo,
                                                                  int tpr, int cblocks, int slices, double* __restrict__ partial) {
    __shared__ double sh[256 * 4];
    float sc, inv;
    pow2_scale(amax, sc, inv);
    const int rpp = 256 / tpr;
    const int ct = threadIdx.x % tpr, rl = threadIdx.x / tpr;
    const int cb = blockIdx.x % cblocks, slice = blockIdx.x / cblocks;
    const int per = (rows + slices - 1) / slices;
    const int r0 = slice * per, r1 = min(rows, r0 + per);
    const int cc = cb * tpr + ct, c0 = cc * 4;
    const bool live = cc < cols4 && rl < rpp;
    double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    if (live) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int n = 0;
        auto emit = [&](long long row, const float4 v) __attribute__((always_inline)) {
            const SplitH sp = split4h(v, sc);
            const float2 h = __builtin_bit_cast(float2, sp.h), l = __builtin_bit_cast(float2, sp.l);
            *reinterpret_cast<float4*>(out + row * ldo + c0) = make_float4(h.x, h.y, l.x, l.y);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        };
        auto fold = [&]() __attribute__((always_inline)) {
            d0 += (double)acc.x; d1 += (double)acc.y; d2 += (double)acc.z; d3 += (double)acc.w;
            acc = make_float4(0.f, 0.f, 0.f, 0.f); n = 0;
        };
        int r = r0 + rl;
        for (; r + 3 * rpp < r1; r += 4 * rpp) {
            float4 qv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) qv[u] = *reinterpret_cast<const float4*>(x + (long long)(r + u * rpp) * ld + c0);
            __builtin_amdgcn_sched_barrier(0);       // every load of the four rows is in flight before the first use
#pragma unroll
            for (int u = 0; u < 4; ++u) emit(r + u * rpp, qv[u]);
            n += 4;
            if (n >= SC_FLUSH) fold();
        }
        for (; r < r1; r += rpp) emit(r, *reinterpret_cast<const float4*>(x + (long long)r * ld + c0));      // at most three rows
        fold();
    }
    sh[threadIdx.x * 4 + 0] = d0; sh[threadIdx.x * 4 + 1] = d1; sh[threadIdx.x * 4 + 2] = d2; sh[threadIdx.x * 4 + 3] = d3;
    __syncthreads();
    if (rl == 0 && cc < cols4) {
        for (int k = 1; k < rpp; ++k) {
            const int o = (k * tpr + ct) * 4;
            d0 += sh[o]; d1 += sh[o + 1]; d2 += sh[o + 2]; d3 += sh[o + 3];
        }
        double* pd = partial + (long long)slice * (cols4 * 4) + c0;
        pd[0] = d0; pd[1] = d1; pd[2] = d2; pd[3] = d3;
    }
}

// colsum[c] = sum over slices of partial[slice][c]: 16 columns x 16 slice lanes per workgroup, every order fixed
__global__ __launch_bounds__(256) void split_colsum_finalize(const double* __restrict__ partial, int slices, int cols, float* __restrict__ colsum) {
    __shared__ double sh[256];
    const int cx = threadIdx.x % 16, lane = threadIdx.x / 16;
    const int ch = blockIdx.x * 16 + cx;
    double s = 0, s1 = 0;
    if (ch < cols) {
        int i = lane;
        for (; i + 16 < slices; i += 32) { s += partial[(long long)i * cols + ch]; s1 += partial[(long long)(i + 16) * cols + ch]; }
        if (i < slices) s += partial[(long long)i * cols + ch];
        s += s1;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    if (lane != 0 || ch >= cols) return;
    for (int l = 1; l < 16; ++l) s += sh[threadIdx.x + l * 16];
    colsum[ch] = (float)s;
}

}  // namespace

namespace glf {

int launch_split_packed(const float* x, long long rows, int cols, long long ld, const float* amax, float* out, long long ldo, hipStream_t s) {
    const long long total = rows * (cols / 4);
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(split_packed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, rows, cols / 4, ld, amax, out, ldo);
    return check_launch("split_f16_packed");
}

// slices of the column-owning split pass: as many workgroups as eight per CU, at most 1024 slices (the partials are
// slices x cols doubles of the caller's workspace, glf_bn_workspace(rows, cols))
int launch_split_packed_colsum(const float* x, int rows, int cols, long long ld, const float* amax, float* out, long long ldo,
                               float* colsum, double* workspace, hipStream_t s) {
    const int c4 = cols / 4;
    const int tpr = c4 >= 64 ? 64 : (c4 < 16 ? c4 : 16);
    const int rpp = 256 / tpr;
    const int cblocks = (c4 + tpr - 1) / tpr;
    long long sl = (long long)num_cus() * 8 / cblocks;
    const int smax = (rows + rpp - 1) / rpp;
    if (sl > smax) sl = smax;
    if (sl > 1024) sl = 1024;
    if (sl < 1) sl = 1;
    const int slices = (int)sl;
    hipLaunchKernelGGL(split_packed_colsum_kernel, dim3((unsigned)slices * (unsigned)cblocks), dim3(256), 0, s, x, rows, c4, ld, amax, out, ldo,
                       tpr, cblocks, slices, workspace);
    if (int rc = check_launch("split_f16_packed_colsum")) return rc;
    hipLaunchKernelGGL(split_colsum_finalize, dim3((cols + 15) / 16), dim3(256), 0, s, workspace, slices, cols, colsum);
    return check_launch("split_colsum_finalize");
}

int init_gemm_f16s_attrs() {
    hipError_t e;
#define SET_ATTR(fn, bytes)                                                                              \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
    if (e != hipSuccess) return fail(GLF_ERR_LAUNCH, "hipFuncSetAttribute(" #fn "): %s", hipGetErrorString(e));
#define SET_ROWS(G, NP_, PA_, PB_) SET_ATTR((gemm_rows_f16s8_kernel<G, NP_, PB_, PA_>), SMEM_ROWS_H8) SET_ATTR((gemm_rows_f16s8_kernel<G, NP_, PB_, PA_, true>), SMEM_ROWS_H8)
#define SET_TN(G, NP_, PA_, PB_) SET_ATTR((gemm_tn_f16s_kernel<G, NP_, PA_, PB_>), SMEM_TN_H) SET_ATTR((gemm_tn_f16s_kernel<G, NP_, PA_, PB_, true>), SMEM_TN_H) \
                                 SET_ATTR((gemm_tn_f16s8_kernel<G, NP_, PA_, PB_>), SMEM_TN_H8)
#define SET_ALL(G, NP_) SET_ROWS(G, NP_, false, false) SET_ROWS(G, NP_, true, false) SET_ROWS(G, NP_, false, true) SET_ROWS(G, NP_, true, true) \
                        SET_TN(G, NP_, false, false) SET_TN(G, NP_, true, false) SET_TN(G, NP_, false, true) SET_TN(G, NP_, true, true)
    SET_ALL(false, 3) SET_ALL(true, 3) SET_ALL(false, 1) SET_ALL(true, 1)
    SET_ATTR((gemm_rows_f16s8_kernel<false, 3, true, true, false, true>), SMEM_ROWS_H8)
    SET_ATTR((gemm_rows_f16s8_kernel<false, 1, true, true, false, true>), SMEM_ROWS_H8)
#undef SET_ALL
#undef SET_TN
#undef SET_ROWS
#undef SET_ATTR
    return init_gemm_f16s4_attrs();
}

// Eligibility: the aligned fast path, and every row that can be redirected to the zero page must fit into it.
bool f16s_rows_ok(const GemmArgs& a) {
    return a.vec_a && a.vec_b && (a.K % BK) == 0 && a.K >= BK && a.K <= ZERO_PAGE_FLOATS && zero_page() != nullptr;
}
bool f16s_tn_ok(const GemmArgs& a) {
    return a.vec_a && a.vec_b && (a.M % 4) == 0 && (a.N % 4) == 0 && a.M >= 4 && a.N >= 4 &&
           a.M <= ZERO_PAGE_FLOATS && a.N <= ZERO_PAGE_FLOATS && zero_page() != nullptr;
}

#ifdef GLF_STAMPS
static void* stamps_buffer() {
    static void* p = [] { void* q = nullptr; (void)hipMalloc(&q, 8192); (void)hipMemset(q, 0, 8192); return q; }();
    return p;
}
extern "C" int glf_debug_stamps(void* host_out) {          // [8 waves][16 iterations][8] s_memtime values of the LAST NT launch
    (void)hipDeviceSynchronize();
    return (int)hipMemcpy(host_out, stamps_buffer(), 8192, hipMemcpyDeviceToHost);
}
#endif

int launch_rows_f16s(const GemmArgs& a0, dim3 grid, bool gather, int nprod, hipStream_t s) {
    if (use_f16s4(a0)) return launch_rows_f16s4(a0, grid, gather, nprod, s);      // short reductions: two workgroups per CU
    GemmArgs a = a0;
    a.zeros = zero_page();
    const long long tiles_m = rows_tiles_m<BM8, true>(a.rect, a.M, a.tap_mask, a.g, a.gather);
    if (a.rect == 2 && tiles_m == 0) return GLF_OK;  // every region's tap set is empty under this mask: nothing to add
    a.tiles_m = (int)tiles_m;
    dim3 g2((unsigned)(tiles_m * a.tiles_n), 1, grid.z);
    // tile order: groups of 4 row tiles x all column tiles once there are >= 8 column tiles (more of the streamed operands
    // served from the XCD's L2: +2 % on the N >= 2048 shapes now that the loop is MFMA-bound; -2 % at 4 column tiles)
    const int group_m = (a.rect == 0 && a.tiles_n >= 8) ? 4 : 0;
    a.flags = (group_m & 0xff) << 8;
    const bool pa = a.a_presplit != 0, pb = a.b_presplit != 0;
#ifdef GLF_STAMPS
    a.partial = reinterpret_cast<float*>(stamps_buffer());
#endif
#define GLF_LAUNCH_ROWS(G, NP_, PA_, PB_)                                                                                  \
    { if (a.epi) hipLaunchKernelGGL((gemm_rows_f16s8_kernel<G, NP_, PB_, PA_, true>), g2, dim3(NT8), SMEM_ROWS_H8, s, a); \
      else hipLaunchKernelGGL((gemm_rows_f16s8_kernel<G, NP_, PB_, PA_>), g2, dim3(NT8), SMEM_ROWS_H8, s, a); }
#define GLF_ROWS_P(G, NP_)                                                                     \
    { if (pa && pb) GLF_LAUNCH_ROWS(G, NP_, true, true) else if (pa) GLF_LAUNCH_ROWS(G, NP_, true, false) \
      else if (pb) GLF_LAUNCH_ROWS(G, NP_, false, true) else GLF_LAUNCH_ROWS(G, NP_, false, false) }
    if (nprod == 3) { if (gather) GLF_ROWS_P(true, 3) else GLF_ROWS_P(false, 3) }
    else { if (gather) GLF_ROWS_P(true, 1) else GLF_ROWS_P(false, 1) }
#undef GLF_ROWS_P
#undef GLF_LAUNCH_ROWS
    return check_launch("gemm_nt(f16x3, 256x128)");
}

// ---- segmented region mode (glf_gemm_params.nseg) ----------------------------------------------------------------------
// Host plan: per axis the band edges are the union of {min(d, H - d), max(d, H - d)} over the distinct |offset| values d, so the
// in-range test of every segment is constant inside a band; a region is a product of bands, its segment mask the AND of the two
// axis masks.  Returns the number of regions (dispatch order: descending segment count, stable), or -1 for too many bands.
struct SegRegion { int y0, y1, x0, x1; unsigned mask; long long tiles; };

static int seg_axis_bands(int len, int nseg, const int32_t* seg, int axis, int* lo, int* hi, unsigned* masks) {
    int edges[2 * SEG_MAX + 2], ne = 0;
    edges[ne++] = 0; edges[ne++] = len;
    for (int s = 0; s < nseg; ++s) {
        const int o = seg[3 * s + axis], d = o < 0 ? -o : o;
        if (d == 0) continue;
        const int e[2] = {d < len - d ? d : len - d, d < len - d ? len - d : d};
        for (int i = 0; i < 2; ++i) {
            const int v = e[i] < 0 ? 0 : (e[i] > len ? len : e[i]);
            bool seen = false;
            for (int k = 0; k < ne; ++k) seen |= edges[k] == v;
            if (!seen) edges[ne++] = v;
        }
    }
    for (int i = 1; i < ne; ++i)                    // insertion sort: at most 58 values
        for (int k = i; k > 0 && edges[k - 1] > edges[k]; --k) { const int t = edges[k]; edges[k] = edges[k - 1]; edges[k - 1] = t; }
    const int nb = ne - 1;
    if (nb > SEG_MAX_BANDS) return -1;
    for (int b = 0; b < nb; ++b) {
        lo[b] = edges[b]; hi[b] = edges[b + 1];
        unsigned m = 0;
        for (int s = 0; s < nseg; ++s) {
            const int o = seg[3 * s + axis];
            if (lo[b] + o >= 0 && hi[b] - 1 + o < len) m |= 1u << s;
        }
        masks[b] = m;
    }
    return nb;
}

static int seg_plan(int n_img, int h, int w, int nseg, const int32_t* seg, SegRegion* out, long long* row_tiles) {
    int ylo[SEG_MAX_BANDS], yhi[SEG_MAX_BANDS], xlo[SEG_MAX_BANDS], xhi[SEG_MAX_BANDS];
    unsigned ym[SEG_MAX_BANDS], xm[SEG_MAX_BANDS];
    const int nby = seg_axis_bands(h, nseg, seg, 0, ylo, yhi, ym), nbx = seg_axis_bands(w, nseg, seg, 1, xlo, xhi, xm);
    if (nby < 0 || nbx < 0) return -1;
    int nreg = 0;
    long long total = 0;
    for (int cnt = nseg; cnt >= 0; --cnt)           // descending segment count, row-major inside a count
        for (int by = 0; by < nby; ++by)
            for (int bx = 0; bx < nbx; ++bx) {
                const unsigned m = ym[by] & xm[bx];
                if (__builtin_popcount(m) != cnt) continue;
                SegRegion& r = out[nreg++];
                r.y0 = ylo[by]; r.y1 = yhi[by]; r.x0 = xlo[bx]; r.x1 = xhi[bx]; r.mask = m;
                r.tiles = ((long long)n_img * (r.y1 - r.y0) * (r.x1 - r.x0) + BM8 - 1) / BM8;
                total += r.tiles;
            }
    *row_tiles = total;
    return nreg;
}

static int seg_check(int n_img, int h, int w, int nseg, const int32_t* seg, const char* who) {
    GLF_REQUIRE(seg != nullptr, GLF_ERR_NULL, "%s: null segment list", who);
    GLF_REQUIRE(nseg >= 1 && nseg <= SEG_MAX, GLF_ERR_UNSUPPORTED, "%s: nseg must be in [1, %d] (got %d)", who, SEG_MAX, nseg);
    GLF_REQUIRE(n_img > 0 && h > 0 && w > 0 && (long long)n_img * h * w < 2147483647LL, GLF_ERR_BAD_SHAPE, "%s: bad map geometry", who);
    return GLF_OK;
}

// ---- column groups (glf_gemm_nt_seg_cols) ----
// A segment contributes to the columns [first, first + count) only, whole 128-column tiles: the mask of column tile t holds the
// segments whose range covers it.  Returns false for a range that is not made of whole tiles inside [0, N).
static bool seg_col_masks(int N, int nseg, const int32_t* cols, int tiles_n, unsigned* masks) {
    for (int t = 0; t < tiles_n; ++t) masks[t] = 0;
    for (int s = 0; s < nseg; ++s) {
        const int c0 = cols[2 * s], cn = cols[2 * s + 1];
        if (c0 < 0 || cn <= 0 || c0 % BN != 0 || cn % BN != 0 || (long long)c0 + cn > N) return false;
        for (int t = c0 / BN; t < (c0 + cn) / BN; ++t) masks[t] |= 1u << s;
    }
    return true;
}

// Dispatch list of a launch with column groups.  A workgroup is (region, row tile of the region, column tile); its chain is the
// K columns plus popcount(region mask & column-tile mask) segments, and chains of one row tile differ by up to an order of
// magnitude (an ASPP head: 1 unit of K for the 1x1 columns, up to 9 for the rate-12 ones; the longest workgroup is a third of
// the launch's duration).  Sorted longest chain first, so that a CU's last workgroups are the shortest; inside one chain length
// by region, row tile, column tile.  Workgroups go to the eight XCDs round-robin by blockIdx and an XCD runs its own in order,
// so a run of 8 * sub sorted entries is dealt out as eight GROUPS of `sub` neighbours (sub = 2 with column groups: typically
// the two column tiles of one branch over one row tile, which read that A tile through one L2; the B tiles are shared by every
// neighbour anyway), the heaviest group to the XCD that has been given the least work so far: the XCDs' totals stay within one
// group's weight of each other.  A workgroup weighs w0 + w1 * chain (the K-iterations of the K columns and of one segment).
// The same list serves a launch WITHOUT column groups (every column tile's mask is full, sub = 4): the plain tile order hands
// each XCD one contiguous eighth of the tiles, and with regions sorted by chain length that is the longest eighth for XCD 0.
struct SegUnit { int chain, r, tm, tn; };
static void seg_units(int nreg, const SegRegion* regs, int tiles_n, const unsigned* colmasks, int sub, int w0, int w1, std::vector<SegUnit>& out) {
    std::vector<SegUnit> u;
    for (int r = 0; r < nreg; ++r)
        for (long long tm = 0; tm < regs[r].tiles; ++tm)
            for (int tn = 0; tn < tiles_n; ++tn) u.push_back(SegUnit{__builtin_popcount(regs[r].mask & colmasks[tn]), r, (int)tm, tn});
    std::stable_sort(u.begin(), u.end(), [](const SegUnit& a, const SegUnit& b) {
        if (a.chain != b.chain) return a.chain > b.chain;
        if (a.r != b.r) return a.r < b.r;
        if (a.tm != b.tm) return a.tm < b.tm;
        return a.tn < b.tn;
    });
    out.resize(u.size());
    const size_t n = u.size();
    long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t run = 8 * (size_t)sub;
    for (size_t c0 = 0; c0 < n; c0 += run) {
        if (c0 + run > n) {                         // the last, partial run: the shortest chains, in sorted order
            for (size_t i = c0; i < n; ++i) out[i] = u[i];
            break;
        }
        int xcd[8] = {0, 1, 2, 3, 4, 5, 6, 7};      // by ascending load (insertion sort, stable); group j is the j-th heaviest
        for (int i = 1; i < 8; ++i)
            for (int k = i; k > 0 && load[xcd[k - 1]] > load[xcd[k]]; --k) { const int t = xcd[k]; xcd[k] = xcd[k - 1]; xcd[k - 1] = t; }
        for (int j = 0; j < 8; ++j)
            for (int i = 0; i < sub; ++i) {
                const SegUnit& q = u[c0 + (size_t)sub * j + i];
                out[c0 + 8 * (size_t)i + xcd[j]] = q;
                load[xcd[j]] += w0 + (long long)w1 * q.chain;
            }
    }
}

// device tables of the plans used so far: made once per (device, geometry, lda, segment list, B offsets, column groups), never freed
struct SegPlanDev {
    int dev, n_img, h, w, lda, nseg, has_cols, N, K, kx, listed;
    int32_t seg[3 * SEG_MAX], cols[2 * SEG_MAX];
    long long boff[SEG_MAX];
    int* tab; long long row_tiles; int max_chain;
};
static std::mutex g_seg_mu;
static std::vector<SegPlanDev> g_seg_plans;

int launch_rows_f16s_seg(const GemmArgs& a0, const glf_gemm_params* p, const int32_t* cols, const int64_t* boff_in, int nprod, hipStream_t s) {
    GemmArgs a = a0;
    a.zeros = zero_page();
    const int n_img = p->n_img, h = p->hd, w = p->wd, nseg = p->nseg;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(GLF_ERR_LAUNCH, "gemm_nt(seg): hipGetDevice failed");
    if (cols && a.tiles_n > SEG_MAX_COLTILES) return fail(GLF_ERR_UNSUPPORTED, "gemm_nt(seg): column groups take at most %d column tiles", SEG_MAX_COLTILES);
    SegPlanDev key;
    memset(&key, 0, sizeof(key));
    key.dev = dev; key.n_img = n_img; key.h = h; key.w = w; key.lda = p->lda; key.nseg = nseg; key.has_cols = cols != nullptr; key.N = p->N; key.K = p->K; key.kx = p->seg_kx;
    memcpy(key.seg, p->seg, sizeof(int32_t) * 3 * nseg);
    if (cols) memcpy(key.cols, cols, sizeof(int32_t) * 2 * nseg);
    for (int i = 0; i < nseg; ++i) key.boff[i] = boff_in ? (long long)boff_in[i] : (long long)p->K + (long long)i * p->seg_kx;
    const int* tab = nullptr;
    long long row_tiles = 0;
    int max_chain = nseg, listed = 0;
    {
        std::lock_guard<std::mutex> lk(g_seg_mu);
        for (const SegPlanDev& q : g_seg_plans)
            if (q.dev == dev && q.n_img == n_img && q.h == h && q.w == w && q.lda == p->lda && q.nseg == nseg && q.has_cols == key.has_cols &&
                q.N == key.N && q.K == key.K && q.kx == key.kx && memcmp(q.seg, key.seg, sizeof(key.seg)) == 0 && memcmp(q.cols, key.cols, sizeof(key.cols)) == 0 &&
                memcmp(q.boff, key.boff, sizeof(key.boff)) == 0) { tab = q.tab; row_tiles = q.row_tiles; max_chain = q.max_chain; listed = q.listed; break; }
        if (!tab) {
            SegRegion regs[SEG_MAX_REGIONS];
            const int nreg = seg_plan(n_img, h, w, nseg, p->seg, regs, &row_tiles);
            if (nreg < 0) return fail(GLF_ERR_UNSUPPORTED, "gemm_nt(seg): more than %d bands on an axis", SEG_MAX_BANDS);
            if (row_tiles * a.tiles_n >= 2147483647LL) return fail(GLF_ERR_BAD_SHAPE, "gemm_nt(seg): grid out of range");
            unsigned colmasks[SEG_MAX_COLTILES] = {0};
            std::vector<SegUnit> units;
            if (cols) {
                if (!seg_col_masks(p->N, nseg, cols, a.tiles_n, colmasks))
                    return fail(GLF_ERR_UNSUPPORTED, "gemm_nt(seg): a segment's columns must be whole 128-column tiles inside [0, N)");
                if (row_tiles * a.tiles_n > SEG_MAX_UNITS) return fail(GLF_ERR_UNSUPPORTED, "gemm_nt(seg): too many workgroups for a dispatch list");
                listed = 1;
            } else if (a.tiles_n <= SEG_MAX_COLTILES && row_tiles * a.tiles_n <= SEG_MAX_UNITS) {
                // every segment contributes to every column: the same balanced dispatch list with full column-tile masks (a launch
                // too large for one keeps the plain tile order)
                for (int t = 0; t < a.tiles_n; ++t) colmasks[t] = 0xffffffffu;
                listed = 1;
            }
            if (listed) seg_units(nreg, regs, a.tiles_n, colmasks, cols ? 2 : 4, p->K / BK, p->seg_kx / BK, units);
            max_chain = 0;
            for (int r = 0; r < nreg; ++r)
                for (int t = 0; t < a.tiles_n; ++t) {
                    const int c = __builtin_popcount(regs[r].mask & (listed ? colmasks[t] : 0xffffffffu));
                    max_chain = c > max_chain ? c : max_chain;
                }
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
                return fail(GLF_ERR_UNSUPPORTED, "gemm_nt(seg): the first launch of a plan allocates its table -- run it once before capturing");
            std::vector<int> host(SEG_TAB_INTS + 2 * units.size(), 0);
            long long first = 0;
            for (int r = 0; r < SEG_TAB_REGIONS; ++r) {
                host[r] = r < nreg ? (int)first : 2147483647;
                if (r < nreg) {
                    int* e = host.data() + SEG_TAB_REGIONS + SEG_REGION_INTS * r;
                    e[0] = regs[r].y0; e[1] = regs[r].x0; e[2] = regs[r].y1 - regs[r].y0; e[3] = regs[r].x1 - regs[r].x0;
                    e[4] = (int)regs[r].mask; e[5] = n_img * e[2] * e[3];
                    first += regs[r].tiles;
                }
            }
            long long offs[SEG_MAX] = {0};
            for (int i = 0; i < nseg; ++i) offs[i] = ((long long)p->seg[3 * i] * w + p->seg[3 * i + 1]) * p->lda + p->seg[3 * i + 2];
            memcpy(host.data() + SEG_TAB_OFFS, offs, sizeof(offs));
            memcpy(host.data() + SEG_TAB_BOFF, key.boff, sizeof(key.boff));
            for (int t = 0; t < SEG_MAX_COLTILES; ++t) host[SEG_TAB_COLMASK + t] = (int)colmasks[t];
            for (size_t i = 0; i < units.size(); ++i) {
                host[SEG_TAB_INTS + 2 * i] = (units[i].r << 16) | units[i].tn;
                host[SEG_TAB_INTS + 2 * i + 1] = units[i].tm;
            }
            int* d = nullptr;
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), host.size() * sizeof(int));
            if (e == hipSuccess) e = hipMemcpy(d, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(GLF_ERR_WORKSPACE, "gemm_nt(seg): plan table: %s", hipGetErrorString(e));
            key.tab = d; key.row_tiles = row_tiles; key.max_chain = max_chain; key.listed = listed;
            g_seg_plans.push_back(key);
            tab = d;
        }
    }
    // rows past a ragged tile's end read the zero page and walk through it for the whole chain: K columns, then the segments of the
    // longest chain any workgroup of this plan walks; a chain that does not fit is refused
    if ((long long)p->K + (long long)max_chain * p->seg_kx + BK > ZERO_PAGE_FLOATS)
        return fail(GLF_ERR_UNSUPPORTED, "gemm_nt(seg): a chain of K + %d segments does not fit the zero page (%d floats)", max_chain, ZERO_PAGE_FLOATS);
    a.seg_tab = tab; a.seg_kx = p->seg_kx; a.seg_cols = listed; a.rect = 0; a.accumulate = 0;
    a.tiles_m = (int)row_tiles;
    dim3 g2((unsigned)(row_tiles * a.tiles_n), 1, 1);
    a.flags = ((a.tiles_n >= 8 ? 4 : 0) & 0xff) << 8;          // grouped tile order, as the plain launch (not used with a dispatch list)
    if (nprod == 3) hipLaunchKernelGGL((gemm_rows_f16s8_kernel<false, 3, true, true, false, true>), g2, dim3(NT8), SMEM_ROWS_H8, s, a);
    else hipLaunchKernelGGL((gemm_rows_f16s8_kernel<false, 1, true, true, false, true>), g2, dim3(NT8), SMEM_ROWS_H8, s, a);
    return check_launch("gemm_nt(f16x3, 256x128, segmented)");
}

int launch_tn_f16s(const GemmArgs& a0, dim3 grid, bool gather, int nprod, hipStream_t s) {
    GemmArgs a = a0;
    a.zeros = zero_page();
#ifdef GLF_STAMPS
    a.stamps = reinterpret_cast<unsigned long long*>(stamps_buffer());
#endif
    const bool pa = a.a_presplit != 0, pb = a.b_presplit != 0;
    // 64 x 64 tiles when one extent is <= 64 and the other small too (layer 1: 64 x 64, 256 x 64, 64 x 256): no zero-page columns
    const bool small = (a.M <= 64 || a.N <= 64) && a.M <= 256 && a.N <= 256;
    const bool wide = !small && a.M > BM;   // 256-wide tiles: re-derive the grid
    dim3 g2 = grid;
    if (wide) {
        a.tiles_m = (a.M + TM8 - 1) / TM8;
        g2 = dim3((unsigned)(a.tiles_m * a.tiles_n), grid.y, grid.z);
    } else if (small) {
        a.tiles_m = (a.M + 63) / 64; a.tiles_n = (a.N + 63) / 64;
        g2 = dim3((unsigned)(a.tiles_m * a.tiles_n), grid.y, grid.z);
    }
#define GLF_LAUNCH_TN(G, NP_, PA_, PB_)                                                                                        \
    { if (wide) hipLaunchKernelGGL((gemm_tn_f16s8_kernel<G, NP_, PA_, PB_>), g2, dim3(NT8), SMEM_TN_H8, s, a);                 \
      else if (small) hipLaunchKernelGGL((gemm_tn_f16s_kernel<G, NP_, PA_, PB_, true>), g2, dim3(NTHREADS), SMEM_TN_H, s, a);  \
      else hipLaunchKernelGGL((gemm_tn_f16s_kernel<G, NP_, PA_, PB_>), g2, dim3(NTHREADS), SMEM_TN_H, s, a); }
#define GLF_TN_P(G, NP_)                                                                       \
    { if (pa && pb) GLF_LAUNCH_TN(G, NP_, true, true) else if (pa) GLF_LAUNCH_TN(G, NP_, true, false) \
      else if (pb) GLF_LAUNCH_TN(G, NP_, false, true) else GLF_LAUNCH_TN(G, NP_, false, false) }
    if (nprod == 3) { if (gather) GLF_TN_P(true, 3) else GLF_TN_P(false, 3) }
    else { if (gather) GLF_TN_P(true, 1) else GLF_TN_P(false, 1) }
#undef GLF_TN_P
#undef GLF_LAUNCH_TN
    return check_launch("gemm_tn(f16x3)");
}

// *out = max(*out, max |x|): out must hold a non-negative float (0 to start a fresh maximum)
int launch_amax(const float* x, long long rows, int cols, long long ld, int vec, float* out, hipStream_t s) {
    const long long total4 = rows * (long long)(vec && (cols >> 2) > 0 ? (cols >> 2) : cols);
    long long blocks = (total4 + 256 * 8 - 1) / (256 * 8);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(amax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, rows, cols, ld, vec, reinterpret_cast<unsigned*>(out));
    return check_launch("amax");
}

}  // namespace glf

extern "C" int glf_gemm_nt_seg_plan(int32_t n_img, int32_t h, int32_t w, int32_t nseg, const int32_t* seg, int32_t* regions,
                                    int32_t* n_regions, int64_t* row_tiles) {
    using namespace glf;
    GLF_REQUIRE(regions && n_regions && row_tiles, GLF_ERR_NULL, "gemm_nt_seg_plan: null argument");
    if (int rc = seg_check(n_img, h, w, nseg, seg, "gemm_nt_seg_plan")) return rc;
    SegRegion regs[SEG_MAX_REGIONS];
    long long total = 0;
    const int nreg = seg_plan(n_img, h, w, nseg, seg, regs, &total);
    GLF_REQUIRE(nreg >= 0, GLF_ERR_UNSUPPORTED, "gemm_nt_seg_plan: more than %d bands on an axis", SEG_MAX_BANDS);
    for (int r = 0; r < nreg; ++r) {
        int32_t* e = regions + 6 * r;
        e[0] = regs[r].y0; e[1] = regs[r].y1; e[2] = regs[r].x0; e[3] = regs[r].x1; e[4] = (int32_t)regs[r].mask; e[5] = (int32_t)regs[r].tiles;
    }
    *n_regions = nreg;
    *row_tiles = total;
    return GLF_OK;
}

extern "C" int glf_gemm_nt_seg_plan_cols(int32_t n_img, int32_t h, int32_t w, int32_t nseg, const int32_t* seg, const int32_t* seg_cols, int32_t N,
                                         int32_t* regions, int32_t* n_regions, int64_t* row_tiles, uint32_t* col_masks, int32_t* order,
                                         int64_t order_cap) {
    using namespace glf;
    GLF_REQUIRE(regions && n_regions && row_tiles && seg_cols && col_masks, GLF_ERR_NULL, "gemm_nt_seg_plan_cols: null argument");
    if (int rc = glf_gemm_nt_seg_plan(n_img, h, w, nseg, seg, regions, n_regions, row_tiles)) return rc;
    const int tiles_n = (N + BN - 1) / BN;
    GLF_REQUIRE(N > 0 && tiles_n <= SEG_MAX_COLTILES, GLF_ERR_UNSUPPORTED, "gemm_nt_seg_plan_cols: N must give 1 .. %d column tiles", SEG_MAX_COLTILES);
    GLF_REQUIRE(seg_col_masks(N, nseg, seg_cols, tiles_n, col_masks), GLF_ERR_UNSUPPORTED,
                "gemm_nt_seg_plan_cols: a segment's columns must be whole 128-column tiles inside [0, N)");
    const long long units = *row_tiles * tiles_n;
    GLF_REQUIRE(units <= SEG_MAX_UNITS, GLF_ERR_UNSUPPORTED, "gemm_nt_seg_plan_cols: too many workgroups for a dispatch list");
    if (order) {
        GLF_REQUIRE(order_cap >= units, GLF_ERR_BAD_SHAPE, "gemm_nt_seg_plan_cols: order has room for %lld workgroups, the plan has %lld", (long long)order_cap, units);
        SegRegion regs[SEG_MAX_REGIONS];
        long long total = 0;
        const int nreg = seg_plan(n_img, h, w, nseg, seg, regs, &total);
        std::vector<SegUnit> u;
        seg_units(nreg, regs, tiles_n, col_masks, 2, 1, 1, u);
        for (size_t i = 0; i < u.size(); ++i) { order[3 * i] = u[i].r; order[3 * i + 1] = u[i].tm; order[3 * i + 2] = u[i].tn; }
    }
    return GLF_OK;
}

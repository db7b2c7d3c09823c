// Split-fp16 NT contraction, SECOND tile configuration: 256 threads = 4 waves (2 x 2), tile 128 x 128 x 32, two LDS buffers
// (64 KB) and <= 256 registers per wave -- TWO workgroups per CU.
//
// The 8-wave 256 x 128 kernel of gemm_f16s.hip owns its CU (144 KB of LDS): nothing runs on the matrix pipe while it
// stages its first tiles or stores its results.  Per workgroup that is 10 % of the time at K = 2048 but 45 % at K = 256 and
// 78 % at K = 64 (in-kernel stamps, profiles/r02_stamps_nt_f16x3.txt), and the C2 step spends 60 ms in contractions of that
// kind (profiles/r02_bench_c2_f16x3_per_shape.csv: layer-1 shapes at 30-64 TF, K = 256 ... 512 at 140-280 TF against 375 TF for
// the projections).  With two co-resident workgroups one multiplies while the other stages or stores.  The price is a third
// more operand traffic per FLOP (128-row instead of 256-row A tiles), so the launcher picks this configuration by shape
// (glf::use_f16s4) and the large-K contractions stay on the 8-wave kernel.
//
// Same operand arithmetic (split_f16.h), LDS row swizzle, gather / tap-mask / rectangle / region semantics, wide-store
// epilogue, column statistics and maxima as gemm_f16s.hip (the walk, the row state and the epilogue are the same code:
// gemm_rows_walk.h).  C, colmax and amax_c of the two configurations are bit-identical: an output element sees the same K
// order, tile by tile, in the same accumulators (profiles/ubench/f16s4_probe.py: |sum| difference 0; the digests of
// profiles/ubench/rows_walk_ab.py under GLF_F16S4 = 0 and 2 are equal on every case).  The column statistics differ in their
// last bits wherever a 256-row tile is two 128-row tiles here: the f64 sums are folded in other groups.
#include "gemm_rows_walk.h"
#include "split_f16.h"
#include <cstdlib>

namespace {

#define GLF_MFMA_F16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
#define GLF_ROW3(c0, c1, m0, m1, ah, al, b0h, b0l, b1h, b1l)  \
    c0 = GLF_MFMA_F16(ah, b0h, c0);                         \
    c1 = GLF_MFMA_F16(ah, b1h, c1);                         \
    if (NP == 3) {                                          \
        m0 = GLF_MFMA_F16(al, b0h, m0);                     \
        m1 = GLF_MFMA_F16(al, b1h, m1);                     \
        m0 = GLF_MFMA_F16(ah, b0l, m0);                     \
        m1 = GLF_MFMA_F16(ah, b1l, m1);                     \
    }

constexpr int BM4 = 128;                 // rows of a tile (BN = 128 columns, BK = 32 deep: gemm_common.h)
constexpr int NT4 = 256;                 // threads
constexpr int WAVE_ROWS = 2;             // wave rows of the workgroup (2 x 2 waves of 64 x 64)
constexpr int RS4 = NT4 / 8;             // rows one staging pass covers (8 threads x float4 per 32-deep row)
constexpr int PL4 = 128 * 64;            // one fp16 plane of an operand tile: 128 rows x 64 B
constexpr int BUF4 = 4 * PL4;            // A high, A low, B high, B low
constexpr size_t SMEM_ROWS_H4 = 2 * BUF4 + 16;

// EPI: the fused output epilogue of glf_gemm_nt_epilogue (see gemm_rows_f16s8_kernel)
template <bool GATHER, int NP, bool PA, bool BP, bool EPI = false>
__global__ __launch_bounds__(NT4, 2) void gemm_rows_f16s4_kernel(const GemmArgs args) {
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
    const int p_rect = GATHER ? args.rect : 0;
    float sc_a, sc_b, inv_a, inv_b;
    pow2_scale(args.amax_a, sc_a, inv_a);
    pow2_scale(args.amax_b, sc_b, inv_b);
    const float p_alpha = args.alpha * inv_a * inv_b;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    unsigned* s_mask = reinterpret_cast<unsigned*>(smem_s + 2 * BUF4);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const RowsGeo G{p_gather, args.g.n_img, g_hs, g_ws, g_hd, g_wd, g_kw, g_stride, g_pad, g_dil};
    int tn;
    RowTile rt{0, pM, 0, 0, g_hd, g_wd, p_tap_mask};
    rows_tile_order((args.flags >> 8) & 0xff, p_tiles_n, tn, rt.tm);
    if (p_rect && !rows_locate<BM4, true>(p_rect, p_tap_mask, G, rt)) return;
    const int tm = rt.tm;
    unsigned mask = rt.mask;
    const int bz = blockIdx.z;
    const float* __restrict__ A = p_A + (long long)bz * p_bsa;
    const float* __restrict__ B = p_B + (long long)bz * p_bsb;
    float* __restrict__ C = p_C + (long long)bz * p_bsc;

    const int ac = tid & 7, ar = tid >> 3;              // 8 float4 per 32-deep row; rows ar + RS4 j

    RowState<4> rows;
    rows_init<4, RS4, GATHER>(rows, tm * BM4 + ar, rt, p_lda, g_hd, g_wd);
    const bool fastg = GATHER && rows_fast_gather(G);
    if (fastg) rows_to_fast(rows, G);
    rows_census<BM4, 4, GATHER>(rows, mask, fastg, ac == 0, p_taps, p_rect, G, s_mask);

    const int nkc = pK / BK;
    const int ntiles = __popc(mask) * nkc;
    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};      // main products
    f32x16 m00 = {0}, m01 = {0}, m10 = {0}, m11 = {0};      // mixed products (x 2^11)
    float4 ra[4], rb[4];
    unsigned rem_mask = mask;
    int tap = -1, kc = nkc;
    const float* pa[4];
    const float* pb[4];
    const int a_col[4] = {4 * ac, 4 * ac, 4 * ac, 4 * ac};

    auto advance = [&]() __attribute__((always_inline)) {
        if (++kc >= nkc) {
            kc = 0;
            tap = rows_next_tap<4, GATHER>(rows, rem_mask, pa, A, p_zero, p_lda, fastg, G, a_col);
            const float* Bt = B + (long long)tap * p_tsb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = tn * BN + ar + RS4 * j;
                pb[j] = (n < pN ? Bt + (long long)n * p_ldb : p_zero) + 4 * ac;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) pa[j] += BK;
#pragma unroll
            for (int j = 0; j < 4; ++j) pb[j] += BK;
        }
    };
    // swizzled staging offset of this thread inside a 64-byte row: 16-byte chunk (ac>>1) ^ ((row>>2)&3), half ac&1
    const int st_chunk = ac >> 1;
    const int st_off = ar * 64 + (((st_chunk ^ ((ar >> 2) & 3)) << 4) | ((ac & 1) << 3));
#define GLF_H4_LOAD() \
    { _Pragma("unroll") for (int j = 0; j < 4; ++j) ra[j] = *reinterpret_cast<const float4*>(pa[j]); \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) rb[j] = *reinterpret_cast<const float4*>(pb[j]); }
#define GLF_H4_STORE_A(J, buf_)                                                                              \
    {                                                                                                        \
        unsigned char* d = smem_s + (buf_) * BUF4 + st_off + J * RS4 * 64;                                   \
        if (PA) {                                                                                            \
            *reinterpret_cast<float2*>(d) = make_float2(ra[J].x, ra[J].y);                                   \
            if (NP == 3) *reinterpret_cast<float2*>(d + PL4) = make_float2(ra[J].z, ra[J].w);                \
        } else {                                                                                             \
            const SplitH s = split4h(ra[J], sc_a);                                                           \
            *reinterpret_cast<f16x4*>(d) = s.h; if (NP == 3) *reinterpret_cast<f16x4*>(d + PL4) = s.l;       \
        }                                                                                                    \
    }
#define GLF_H4_STORE_B(J, buf_)                                                                              \
    {                                                                                                        \
        unsigned char* d = smem_s + (buf_) * BUF4 + 2 * PL4 + st_off + J * RS4 * 64;                         \
        if (BP) {                                                                                            \
            *reinterpret_cast<float2*>(d) = make_float2(rb[J].x, rb[J].y);                                   \
            if (NP == 3) *reinterpret_cast<float2*>(d + PL4) = make_float2(rb[J].z, rb[J].w);                \
        } else {                                                                                             \
            const SplitH s = split4h(rb[J], sc_b);                                                           \
            *reinterpret_cast<f16x4*>(d) = s.h; if (NP == 3) *reinterpret_cast<f16x4*>(d + PL4) = s.l;       \
        }                                                                                                    \
    }
#define GLF_H4_STORE(buf_) \
    { GLF_H4_STORE_A(0, buf_) GLF_H4_STORE_A(1, buf_) GLF_H4_STORE_A(2, buf_) GLF_H4_STORE_A(3, buf_) \
      GLF_H4_STORE_B(0, buf_) GLF_H4_STORE_B(1, buf_) GLF_H4_STORE_B(2, buf_) GLF_H4_STORE_B(3, buf_) }
#define GLF_H4_FRAGS(P, buf_, fo_)                                                                            \
        {                                                                                                     \
            const unsigned char* ab_ = smem_s + (buf_) * BUF4 + wm * 64 + (fo_);                              \
            const unsigned char* bb_ = smem_s + (buf_) * BUF4 + 2 * PL4 + wn * 64 + (fo_);                    \
            P##b0h = *reinterpret_cast<const f16x8*>(bb_);                                                    \
            P##b1h = *reinterpret_cast<const f16x8*>(bb_ + 32 * 64);                                          \
            P##a0h = *reinterpret_cast<const f16x8*>(ab_);                                                    \
            P##a1h = *reinterpret_cast<const f16x8*>(ab_ + 32 * 64);                                          \
            if (NP == 3) {                                                                                    \
                P##a0l = *reinterpret_cast<const f16x8*>(ab_ + PL4);                                          \
                P##b0l = *reinterpret_cast<const f16x8*>(bb_ + PL4);                                          \
                P##b1l = *reinterpret_cast<const f16x8*>(bb_ + 32 * 64 + PL4);                                \
                P##a1l = *reinterpret_cast<const f16x8*>(ab_ + 32 * 64 + PL4);                                \
            } else { P##a0l = P##a0h; P##b0l = P##b0h; P##b1l = P##b1h; P##a1l = P##a1h; }                    \
        }
    // Main loop: the classic two-buffer pipeline, one barrier per K-tile, no hand-placed issue slots -- the SECOND workgroup of
    // the CU (64 KB of LDS and 256 registers per wave leave room for exactly two) is what fills this workgroup's barrier waits,
    // LDS latencies, prologue and epilogue with MFMA work.  Tile it is multiplied out of buffer it & 1 while tile it + 1 (in
    // registers since the previous iteration) is staged into the other buffer and tile it + 2 is requested from global memory.
    if (ntiles > 0) {
        const int sw = (lane >> 2) & 3, hh = lane >> 5;
        const int fo0 = (lane & 31) * 64 + (((0 + hh) ^ sw) << 4);
        const int fo1 = (lane & 31) * 64 + (((2 + hh) ^ sw) << 4);
        advance();
        GLF_H4_LOAD()
        GLF_H4_STORE(0)
        if (ntiles > 1) { advance(); GLF_H4_LOAD() }
        __syncthreads();
        for (int it = 0; it < ntiles; ++it) {
            const int cur = it & 1;
            f16x8 fb0h, fb1h, fb0l, fb1l, fa0h, fa0l, fa1h, fa1l;
            f16x8 gb0h, gb1h, gb0l, gb1l, ga0h, ga0l, ga1h, ga1l;
            GLF_H4_FRAGS(f, cur, fo0)
            GLF_H4_FRAGS(g, cur, fo1)
            GLF_ROW3(c00, c01, m00, m01, fa0h, fa0l, fb0h, fb0l, fb1h, fb1l)
            GLF_ROW3(c10, c11, m10, m11, fa1h, fa1l, fb0h, fb0l, fb1h, fb1l)
            if (it + 1 < ntiles) {
                GLF_H4_STORE(cur ^ 1)
                if (it + 2 < ntiles) { advance(); GLF_H4_LOAD() }
            }
            GLF_ROW3(c00, c01, m00, m01, ga0h, ga0l, gb0h, gb0l, gb1h, gb1l)
            GLF_ROW3(c10, c11, m10, m11, ga1h, ga1l, gb0h, gb0l, gb1h, gb1l)
            __syncthreads();
        }
    }

    const RowsOut out{C, p_bias, args.res, args.colstats, args.colmax, args.amax_c, args.ld_res, p_bsc,
                      pN, p_ldc, p_accumulate, p_rect, args.relu, tn, g_hd, g_wd, p_alpha};
    rows_f16s_epilogue<BM4, WAVE_ROWS, EPI>(out, rt, smem_s, c00, c01, c10, c11, m00, m01, m10, m11);
}
}  // namespace

namespace glf {

int init_gemm_f16s4_attrs() {
    hipError_t e;
#define SET_ATTR(fn)                                                                                     \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_ROWS_H4); \
    if (e != hipSuccess) return fail(GLF_ERR_LAUNCH, "hipFuncSetAttribute(" #fn "): %s", hipGetErrorString(e));
#define SET_E(G, NP_, E_) SET_ATTR((gemm_rows_f16s4_kernel<G, NP_, false, false, E_>)) SET_ATTR((gemm_rows_f16s4_kernel<G, NP_, true, false, E_>)) \
                          SET_ATTR((gemm_rows_f16s4_kernel<G, NP_, false, true, E_>)) SET_ATTR((gemm_rows_f16s4_kernel<G, NP_, true, true, E_>))
#define SET_P(G, NP_) SET_E(G, NP_, false) SET_E(G, NP_, true)
    SET_P(false, 3) SET_P(true, 3) SET_P(false, 1) SET_P(true, 1)
#undef SET_E
#undef SET_P
#undef SET_ATTR
    return GLF_OK;
}

// Which NT contractions take the 4-wave / two-workgroups-per-CU configuration.  GLF_F16S4 = 0: never, 2: always (A/B runs),
// default: by shape -- the reduction per output tile (K x kept taps) is short enough that the 8-wave kernel's un-overlapped
// prologue + epilogue would be a large share of its workgroup time.
bool use_f16s4(const GemmArgs& a) {
    static const int mode = [] { const char* e = getenv("GLF_F16S4"); return e ? atoi(e) : 1; }();
    if (mode == 0) return false;
    if (mode == 2) return true;
    const long long kred = (long long)a.K * __builtin_popcount(a.tap_mask);
    return kred <= 256;
}

int launch_rows_f16s4(const GemmArgs& a0, dim3 grid, bool gather, int nprod, hipStream_t s) {
    GemmArgs a = a0;
    a.zeros = zero_page();
    const long long tiles_m = rows_tiles_m<BM4, true>(a.rect, a.M, a.tap_mask, a.g, a.gather);
    if (a.rect == 2 && tiles_m == 0) return GLF_OK;  // every region's tap set is empty under this mask: nothing to add
    a.tiles_m = (int)tiles_m;
    dim3 g2((unsigned)(tiles_m * a.tiles_n), 1, grid.z);
    a.flags = (a.rect == 0 && a.tiles_n >= 8 ? 4 : 0) << 8;          // grouped tile order, as the 8-wave kernel
    const bool pa = a.a_presplit != 0, pb = a.b_presplit != 0;
#define GLF_L4(G, NP_, PA_, PB_)                                                                                          \
    { if (a.epi) hipLaunchKernelGGL((gemm_rows_f16s4_kernel<G, NP_, PA_, PB_, true>), g2, dim3(NT4), SMEM_ROWS_H4, s, a);  \
      else hipLaunchKernelGGL((gemm_rows_f16s4_kernel<G, NP_, PA_, PB_>), g2, dim3(NT4), SMEM_ROWS_H4, s, a); }
#define GLF_L4P(G, NP_)                                                                   \
    { if (pa && pb) GLF_L4(G, NP_, true, true) else if (pa) GLF_L4(G, NP_, true, false) \
      else if (pb) GLF_L4(G, NP_, false, true) else GLF_L4(G, NP_, false, false) }
    if (nprod == 3) { if (gather) GLF_L4P(true, 3) else GLF_L4P(false, 3) }
    else { if (gather) GLF_L4P(true, 1) else GLF_L4P(false, 1) }
#undef GLF_L4P
#undef GLF_L4
    return check_launch("gemm_nt(f16x3, 128x128, 2 workgroups / CU)");
}

}  // namespace glf

// Fused softmax attention of the fusion block's `embedded` mode under 16-bit storage (include/glfusion.h:
// glf_s16_attn_softmax_fwd / _bwd):
//      S = theta phi^T   [L, L] per frame,   P = softmax(S, dim = -1),   y = P g
// theta, phi, g, y, dy and the three gradients are bf16 [L][Ci] rows (column slices of the projection buffers); the [L, L]
// score matrix is never written to memory.  Same four-pass skeleton as attn_softmax.hip (FWD; backward DV, DK, DQ with the
// scores recomputed from theta, phi and the saved row log-sum-exp), on ONE v_mfma bf16 instruction per product.
//
// Arithmetic contract:
//   * S (and dP = dY g^T) on v_mfma_f32_16x16x32_bf16, fp32 accumulation; the same tiles in the same order in every pass,
//     so backward recomputes exactly the forward's fp32 scores.
//   * row max, row sum, online rescaling in fp32; P rounded to bf16 only as the A operand of P g (the row sum adds the fp32 P).
//   * y accumulated in fp32 (v_mfma_f32_32x32x16_bf16), normalised in fp32, stored as bf16 once; lse = m + log(l) fp32.
//   * backward: D = rowsum(dY o Y) in fp32 (attn_s16_rowdot_kernel); dS = P (dP - D) in fp32, rounded to bf16 only as an
//     MFMA operand; every output element is written exactly once (no atomics, no zero fill: bitwise reproducible).
//
// Work decomposition.  A workgroup = 512 threads = 8 waves (two per SIMD) owns 64 outer rows -- query rows in FWD / DQ,
// key rows in DV / DK -- and keeps their 64 x Ci fp32 accumulator block in registers: wave w owns columns
// [128 w, 128 w + 128), 2 x 4 tiles of 32 x 32 = 128 accumulator registers per lane at Ci = 1024.  It walks the 64-row inner
// blocks as one continuous stream of STEPS, each step one slot of a three-slot LDS ring filled by LDS-DMA
// (global_load_lds_dwordx4, one counted vmcnt + one barrier per step, the loads of step t + 2 issued behind it):
//   * Ci / 64 score steps: theta / phi (DK, DQ also dY / g) [64 rows][64 columns] tiles, 128-byte rows, 16-byte chunk c of row
//     r stored at c ^ ((r >> 1) & 7) (source-side swizzle); wave w forms the 16 x 32 strip (query block w & 3, key blocks
//     2 (w >> 2) + {0, 1}) of the 64 x 64 tile with ds_read_b128 fragments, over the whole Ci: no cross-wave sum.
//     The last score step also carries the inner block's lse / D rows (backward, dword LDS-DMA).
//   * the tile goes to LDS as fp32, 8 threads per query row transform it (FWD: online softmax; DV: P = exp(S - lse);
//     DK, DQ: dS) and leave it as a bf16 [outer][inner] tile T, 128-byte rows with the same chunk swizzle;
//   * 4 product steps of 16 inner rows: Z [16 inner rows][Ci] (FWD g, DV dY, DK theta, DQ phi) staged whole, 64-byte chunk k of
//     row r at k ^ zsw(r); acc[64][Ci] += T[64][16] Z[16][Ci] with A fragments by ds_read_b128 from T and B fragments by
//     ds_read_b64_tr_b16 from Z (the reduction index is Z's row).
// LDS: 3 x 33,280 B ring + two fp32 64 x 68 tiles + the 8 KiB T tile + row statistics = 142,080 B, one workgroup per CU.
#include "attn_s16_stage.h"

namespace {

enum S16AttnMode { SA_FWD = 0, SA_DV = 1, SA_DK = 2, SA_DQ = 3 };

constexpr int SA_SLD = 68;                // fp32 row stride of the score tiles (conflict-free stores from the 16x16 layout)
constexpr int SA_RING = SA_NSLOT * SA_SLOT;
constexpr int SA_SS = SA_RING;                                  // S  [64][SA_SLD] fp32
constexpr int SA_DP = SA_SS + SA_T * SA_SLD * 4;                // dP [64][SA_SLD] fp32
constexpr int SA_TT = SA_DP + SA_T * SA_SLD * 4;                // T  [64][64] bf16
constexpr int SA_ROW = SA_TT + SA_T * SA_T * 2;                 // FWD: running max / sum / rescale factor per query row
constexpr size_t SMEM_S16ATTN = SA_ROW + 3 * SA_T * 4;

struct S16AttnArgs {
    const u16* q; const u16* k; const u16* v;             // theta, phi, g
    const u16* dy;
    const float* lse;                                     // backward: [frames * L]
    const float* dsum;                                    // backward: [frames * L] D = rowsum(dy o y)
    u16* out;                                             // FWD y, DV dg, DK dphi, DQ dtheta
    float* lse_out;
    int L, ci, frames, nob;
    long long ldq, ldk, ldv, lddy, ldo;
};

template <int MODE>
__global__ __launch_bounds__(SA_NT, 1) void attn_s16_kernel(const S16AttnArgs args) {
    constexpr bool BWD = MODE != SA_FWD;
    constexpr bool TWO = MODE == SA_DK || MODE == SA_DQ;      // dP tile too
    constexpr bool QOUT = MODE == SA_FWD || MODE == SA_DQ;    // outer rows are query rows
    const int L = args.L, ci = args.ci;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = xcd_remap(blockIdx.x, gridDim.x);        // consecutive outer blocks (one frame) on one XCD: its L2 serves them
    const long long fr = bid / args.nob;
    const int o0 = (bid - (int)fr * args.nob) * SA_T;
    const u16* __restrict__ Q = args.q + fr * L * args.ldq;
    const u16* __restrict__ K = args.k + fr * L * args.ldk;
    const u16* __restrict__ V = args.v + fr * L * args.ldv;
    const u16* __restrict__ DY = BWD ? args.dy + fr * L * args.lddy : nullptr;
    const float* __restrict__ LSE = BWD ? args.lse + fr * L : nullptr;
    const float* __restrict__ DSUM = BWD ? args.dsum + fr * L : nullptr;
    const u16* __restrict__ Z = MODE == SA_FWD ? V : MODE == SA_DV ? DY : MODE == SA_DK ? Q : K;
    const long long ldz = MODE == SA_FWD ? args.ldv : MODE == SA_DV ? args.lddy : MODE == SA_DK ? args.ldq : args.ldk;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Ss = reinterpret_cast<float*>(smem + SA_SS);
    float* Dp = reinterpret_cast<float*>(smem + SA_DP);
    unsigned char* Tt = smem + SA_TT;
    float* rowm = reinterpret_cast<float*>(smem + SA_ROW);
    float* rowl = rowm + SA_T;
    float* rowa = rowl + SA_T;

    const int nsc = ci / 64;                                  // score steps per inner block
    const int per = nsc + 4;                                  // steps per inner block
    const int nblk = (L + SA_T - 1) / SA_T;
    const int zins = ci / 32;                                 // LDS-DMA instructions of a product step (16 rows x Ci)
    const int zcnt = zins > wave ? (zins - wave + 7) / 8 : 0; // ... this wave's share
    const int scnt = TWO ? 4 : 2;                             // ... of a score step

    // score-step staging: wave w fills rows 8 w .. 8 w + 7 of every tile, lane -> row 8 w + (lane >> 3), chunk lane & 7
    const int srow = 8 * wave + (lane >> 3);
    const int scol = ((lane & 7) ^ ((srow >> 1) & 7)) * 8;
    // product-step staging: instruction e (= wave + 8 u) holds 16-byte pieces 64 e + lane of the [16][Ci] image
    const int pr = ci / 8;                                    // pieces per row
    const bool zq = (ci % 128) == 0;
    int zrow[4], zcol[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int pc = (wave + 8 * u) * 64 + lane;
        const int rr = pc / pr, pos = pc - rr * pr;
        const int zs = zq ? (rr & 3) : ((rr >> 1) & 1);
        zrow[u] = rr;
        zcol[u] = ((((pos >> 2) ^ zs)) << 2 | (pos & 3)) * 8;
    }

    auto issue = [&](int ib_, int j_, int slot_) __attribute__((always_inline)) {
        unsigned char* sb = smem + slot_ * SA_SLOT;
        const int i0_ = ib_ * SA_T;
        if (j_ < nsc) {
            const int xr0 = QOUT ? o0 : i0_, yr0 = QOUT ? i0_ : o0;
            const long long rq = min(xr0 + srow, L - 1), rk = min(yr0 + srow, L - 1);
            const int col = j_ * 64 + scol;
            glds16(Q + rq * args.ldq + col, sb + wave * 1024);
            glds16(K + rk * args.ldk + col, sb + 8192 + wave * 1024);
            if (TWO) {
                glds16(DY + rq * args.lddy + col, sb + 16384 + wave * 1024);
                glds16(V + rk * args.ldv + col, sb + 24576 + wave * 1024);
            }
            if (BWD && j_ == nsc - 1 && wave < 2) glds4((wave == 0 ? LSE : DSUM) + min(xr0 + lane, L - 1), sb + 32768 + wave * 256);
        } else {
            const int r0 = i0_ + 16 * (j_ - nsc);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (wave + 8 * u < zins) glds16(Z + (long long)min(r0 + zrow[u], L - 1) * ldz + zcol[u], sb + (wave + 8 * u) * 1024);
            }
        }
    };
    // fragment offsets.  Score strip: query rows 16 (w & 3) + (lane & 15), key rows 16 kb + (lane & 15), kb = 2 (w >> 2) + t;
    // k-step s (32 columns) reads chunk 4 s + (lane >> 4)
    const int l15 = lane & 15, g4 = lane >> 4;
    int fx[2], fy[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int xr = 16 * (wave & 3) + l15;
        fx[s] = xr * 128 + (((4 * s + g4) ^ ((xr >> 1) & 7)) << 4);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int yr = 16 * (2 * (wave >> 2) + t) + l15;
            fy[t][s] = yr * 128 + (((4 * s + g4) ^ ((yr >> 1) & 7)) << 4);
        }
    }
    // product step: A rows 32 i + (lane & 31) of T, chunk 2 s' + (lane >> 5) for the 16-row k-step s'; B by transposed reads:
    // lane 4 q + p of group g addresses Z row 8 (g >> 1) + q (second read + 4), columns 32 jt + 16 (g & 1) + 4 p of the wave's
    // 128 columns
    const int l31 = lane & 31, hl = lane >> 5;
    int tm[2], tsw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { tm[i] = (32 * i + l31) * 128; tsw[i] = ((32 * i + l31) >> 1) & 7; }
    const int trow = 8 * (g4 >> 1) + ((lane & 15) >> 2);
    const int tzs = zq ? (trow & 3) : ((trow >> 1) & 1);
    const int tin = 32 * (g4 & 1) + 8 * (lane & 3);
    const int zrb = ci * 2;                                    // bytes of a Z row in LDS
    int tz[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) tz[jt] = trow * zrb + (((4 * wave + jt) ^ tzs) << 6) + tin;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x16{0};
    f32x4_ sacc[2], dacc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) { sacc[t] = f32x4_{0, 0, 0, 0}; dacc[t] = f32x4_{0, 0, 0, 0}; }
    if (MODE == SA_FWD && tid < SA_T) { rowm[tid] = -INFINITY; rowl[tid] = 0.f; rowa[tid] = 1.f; }

    // the step stream: step t waits for its own loads, passes the barrier, then issues step t + 2 into the slot step t - 1 used
    int slot = 0;                                             // slot of the current step
    int ibf = 0, jf = 2;                                      // step t + 2 (per >= 5: steps 0 .. 2 are all in block 0; issue() maps
                                                              // each to a score or a product step, Ci = 64 has one score step)
    issue(0, 0, 0);
    issue(0, 1, 1);
    auto begin_step = [&](int next_cnt) __attribute__((always_inline)) {
        wait_vm(next_cnt);                                    // this step landed (this wave's part); the next one may fly
        __builtin_amdgcn_s_barrier();                         // ... everyone's part; everyone is done with the previous slot
        asm volatile("" ::: "memory");                        // no LDS access moves across the barrier
        if (ibf < nblk) {
            issue(ibf, jf, slot == 0 ? 2 : slot - 1);
            if (++jf == per) { jf = 0; ++ibf; }
        }
    };
    for (int ib = 0; ib < nblk; ++ib) {
        // ---- score steps: S (and dP) strips over 64 columns each ----
        for (int j = 0; j < nsc; ++j) {
            begin_step(j + 1 < nsc ? scnt + ((BWD && j + 1 == nsc - 1 && wave < 2) ? 1 : 0) : zcnt);
            const unsigned char* sb = smem + slot * SA_SLOT;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(sb + fx[s]);
                const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(sb + 8192 + fy[0][s]);
                const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(sb + 8192 + fy[1][s]);
                sacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, sacc[0], 0, 0, 0);
                sacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, sacc[1], 0, 0, 0);
                if (TWO) {
                    const bf16x8 c = *reinterpret_cast<const bf16x8*>(sb + 16384 + fx[s]);
                    const bf16x8 d0 = *reinterpret_cast<const bf16x8*>(sb + 24576 + fy[0][s]);
                    const bf16x8 d1 = *reinterpret_cast<const bf16x8*>(sb + 24576 + fy[1][s]);
                    dacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c, d0, dacc[0], 0, 0, 0);
                    dacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c, d1, dacc[1], 0, 0, 0);
                }
            }
            slot = slot == 2 ? 0 : slot + 1;
        }
        {
            // ---- the tile is complete: fp32 to LDS, transform, bf16 T tile (the last score step's slot, which holds the lse / D
            // rows, is refilled only behind the next barrier) ----
            const unsigned char* sb = smem + (slot == 0 ? 2 : slot - 1) * SA_SLOT;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int off = (16 * (wave & 3) + 4 * g4 + r) * SA_SLD + 16 * (2 * (wave >> 2) + tt) + l15;
                    Ss[off] = sacc[tt][r];
                    if (TWO) Dp[off] = dacc[tt][r];
                }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) { sacc[tt] = f32x4_{0, 0, 0, 0}; dacc[tt] = f32x4_{0, 0, 0, 0}; }
            __syncthreads();
            const int row = tid >> 3, part = tid & 7;            // query row of the tile, keys 8 part .. 8 part + 7
            const int i0 = ib * SA_T;
            const int q0 = QOUT ? o0 : i0, k0 = QOUT ? i0 : o0;
            float sv[8];
            {
                const float4 x0 = *reinterpret_cast<const float4*>(Ss + row * SA_SLD + 8 * part);
                const float4 x1 = *reinterpret_cast<const float4*>(Ss + row * SA_SLD + 8 * part + 4);
                sv[0] = x0.x; sv[1] = x0.y; sv[2] = x0.z; sv[3] = x0.w; sv[4] = x1.x; sv[5] = x1.y; sv[6] = x1.z; sv[7] = x1.w;
            }
            float pv[8];
            if (MODE == SA_FWD) {
                float mx = -INFINITY;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (k0 + 8 * part + e >= L) sv[e] = -INFINITY;
                    mx = fmaxf(mx, sv[e]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
                const float m_old = rowm[row], m_new = fmaxf(m_old, mx);   // every inner block holds >= 1 valid key
                float sum = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) { pv[e] = __expf(sv[e] - m_new); sum += pv[e]; }
                sum += __shfl_xor(sum, 1, 64);
                sum += __shfl_xor(sum, 2, 64);
                sum += __shfl_xor(sum, 4, 64);
                if (part == 0) {                                 // the row's 8 lanes are one wave: they all read rowm above
                    const float alpha = __expf(m_old - m_new);   // 0 on the first block (m_old = -inf)
                    rowa[row] = alpha;
                    rowm[row] = m_new;
                    rowl[row] = rowl[row] * alpha + sum;
                }
            } else {
                const unsigned char* st = sb + 32768;            // lse / D of the tile's query rows, staged with the last score step
                const float lse = reinterpret_cast<const float*>(st)[row];
                const float dsum = reinterpret_cast<const float*>(st + 256)[row];
                float dpv[8];
                if (TWO) {
                    const float4 x0 = *reinterpret_cast<const float4*>(Dp + row * SA_SLD + 8 * part);
                    const float4 x1 = *reinterpret_cast<const float4*>(Dp + row * SA_SLD + 8 * part + 4);
                    dpv[0] = x0.x; dpv[1] = x0.y; dpv[2] = x0.z; dpv[3] = x0.w; dpv[4] = x1.x; dpv[5] = x1.y; dpv[6] = x1.z; dpv[7] = x1.w;
                }
                const bool qok = q0 + row < L;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool ok = qok && k0 + 8 * part + e < L;
                    float p = ok ? __expf(sv[e] - lse) : 0.f;
                    if (TWO) p = ok ? p * (dpv[e] - dsum) : 0.f;
                    pv[e] = p;
                }
            }
            if (QOUT) {
                // T[q][key]: one 16-byte write of 8 keys
                uint4 o;
                o.x = pack2(pv[0], pv[1]); o.y = pack2(pv[2], pv[3]); o.z = pack2(pv[4], pv[5]); o.w = pack2(pv[6], pv[7]);
                *reinterpret_cast<uint4*>(Tt + tt_off(row, 8 * part)) = o;
            } else {
                // T[key][q]
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const unsigned w2 = pack2(pv[e], pv[e + 1]);
                    *reinterpret_cast<u16*>(Tt + tt_off(8 * part + e, row)) = (u16)(w2 & 0xffffu);
                    *reinterpret_cast<u16*>(Tt + tt_off(8 * part + e + 1, row)) = (u16)(w2 >> 16);
                }
            }
            // the next step's wait + barrier orders these writes before every wave's product reads
        }
        // ---- product steps: acc += T[64][16 inner rows] Z[16 inner rows][Ci] ----
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool last = ib + 1 == nblk && s == 3;
            begin_step(s < 3 ? zcnt : last ? 0 : scnt + ((BWD && nsc == 1 && wave < 2) ? 1 : 0));
            if (MODE == SA_FWD && s == 0) {
                // rescale the accumulators by alpha of their rows -- skipped when no row of the block moved its maximum
                float al[2][16];
                bool moved = false;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const float4 a4 = *reinterpret_cast<const float4*>(rowa + 32 * i + 8 * r4 + 4 * hl);
                        al[i][4 * r4] = a4.x; al[i][4 * r4 + 1] = a4.y; al[i][4 * r4 + 2] = a4.z; al[i][4 * r4 + 3] = a4.w;
                        moved |= a4.x != 1.f || a4.y != 1.f || a4.z != 1.f || a4.w != 1.f;
                    }
                if (__ballot(moved) != 0ull) {
#pragma unroll
                    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[i][jt][r] *= al[i][r];
                }
            }
            if (128 * wave < ci) {
                // all four column tiles, also where Ci % 128 == 64 leaves the last two beyond Ci: their reads stay inside the LDS
                // allocation and their results are never stored (a per-tile branch made hipcc spill the accumulators)
                bf16x8 af[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(Tt + tm[i] + (((2 * s + hl) ^ tsw[i]) << 4));
                // the eight transposing reads and their wait in ONE asm statement: hipcc does not count inline-asm LDS reads, so
                // with a wait in a statement of its own it scheduled MFMAs ahead of their data
                const unsigned zb = lds0 + slot * SA_SLOT;
                const unsigned a0 = zb + tz[0], a1 = zb + tz[1], a2 = zb + tz[2], a3 = zb + tz[3], r4 = 4 * zrb;
                v2i_ rz[4][2];
                asm volatile(
                    "ds_read_b64_tr_b16 %0, %8\n\t"
                    "ds_read_b64_tr_b16 %1, %9\n\t"
                    "ds_read_b64_tr_b16 %2, %10\n\t"
                    "ds_read_b64_tr_b16 %3, %11\n\t"
                    "ds_read_b64_tr_b16 %4, %12\n\t"
                    "ds_read_b64_tr_b16 %5, %13\n\t"
                    "ds_read_b64_tr_b16 %6, %14\n\t"
                    "ds_read_b64_tr_b16 %7, %15\n\t"
                    "s_waitcnt lgkmcnt(0)"
                    : "=&v"(rz[0][0]), "=&v"(rz[0][1]), "=&v"(rz[1][0]), "=&v"(rz[1][1]), "=&v"(rz[2][0]), "=&v"(rz[2][1]), "=&v"(rz[3][0]),
                      "=&v"(rz[3][1])
                    : "v"(a0), "v"(a0 + r4), "v"(a1), "v"(a1 + r4), "v"(a2), "v"(a2 + r4), "v"(a3), "v"(a3 + r4)
                    : "memory");
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    typedef int v4i_ __attribute__((ext_vector_type(4)));
                    const v4i_ bw = {rz[jt][0].x, rz[jt][0].y, rz[jt][1].x, rz[jt][1].y};
                    const bf16x8 b = __builtin_bit_cast(bf16x8, bw);
                    acc[0][jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], b, acc[0][jt], 0, 0, 0);
                    acc[1][jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], b, acc[1][jt], 0, 0, 0);
                }
            }
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    __syncthreads();                                          // rowl final for every row

    // ---- epilogue: rows o0 + 32 i + (r & 3) + 8 (r >> 2) + 4 hl, columns 32 (4 w + jt) + l31; bf16 once ----
    u16* __restrict__ OUT = args.out + fr * L * args.ldo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hl;
            const int row = o0 + rl;
            if (row < L) {
                const float scale = MODE == SA_FWD ? 1.f / rowl[rl] : 1.f;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    const int c = 32 * (4 * wave + jt) + l31;
                    if (c < ci) OUT[(long long)row * args.ldo + c] = (u16)(pack2(acc[i][jt][r] * scale, 0.f) & 0xffffu);
                }
            }
        }
    }
    if (MODE == SA_FWD && tid < SA_T && o0 + tid < L) args.lse_out[fr * L + o0 + tid] = rowm[tid] + logf(rowl[tid]);
}

// D[row] = sum_c dy[row][c] * y[row][c] in fp32: one wavefront per row, 8 columns per lane and load
__global__ __launch_bounds__(256) void attn_s16_rowdot_kernel(const u16* __restrict__ dy, long long lddy, const u16* __restrict__ y, long long ldy,
                                                              float* __restrict__ out, long long rows, int ci) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int c = 8 * lane; c < ci; c += 512) {
        const uint4 a = *reinterpret_cast<const uint4*>(dy + row * lddy + c);
        const uint4 b = *reinterpret_cast<const uint4*>(y + row * ldy + c);
        const unsigned av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s = fmaf(__uint_as_float(av[e] << 16), __uint_as_float(bv[e] << 16), s);
            s = fmaf(__uint_as_float(av[e] & 0xffff0000u), __uint_as_float(bv[e] & 0xffff0000u), s);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = s;
}

bool stride_ok(long long ld, int ci) { return ld >= ci && ld % 8 == 0; }

// argument checks, before any HIP runtime call
// `others_ok`: the entry point's remaining pointers are all non-null, so a null pointer wins over every other error
int s16_attn_check(const glf_attn_params* p, const void* q, const void* k, const void* v, bool others_ok, const char* what) {
    GLF_REQUIRE(p && q && k && v && others_ok, GLF_ERR_NULL, "%s: null argument", what);
    GLF_REQUIRE(p->frames >= 1 && p->L >= 1, GLF_ERR_BAD_SHAPE, "%s: frames (%d) and L (%d) must be >= 1", what, p->frames, p->L);
    GLF_REQUIRE((long long)p->frames * ((p->L + SA_T - 1) / SA_T) < (1ll << 31), GLF_ERR_BAD_SHAPE, "%s: frames * ceil(L / 64) too large", what);
    GLF_REQUIRE(p->ci >= 64 && p->ci % 64 == 0 && p->ci <= SA_MAXCI, GLF_ERR_UNSUPPORTED,
                "%s: Ci must be a multiple of 64 and <= %d (got %d)", what, SA_MAXCI, p->ci);
    GLF_REQUIRE(stride_ok(p->ldq, p->ci) && stride_ok(p->ldk, p->ci) && stride_ok(p->ldv, p->ci) && stride_ok(p->ldy, p->ci), GLF_ERR_UNSUPPORTED,
                "%s: row strides must be multiples of 8 elements and >= Ci", what);
    GLF_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v), GLF_ERR_UNSUPPORTED, "%s: theta / phi / g must be 16-byte aligned", what);
    return GLF_OK;
}

S16AttnArgs s16_attn_args(const glf_attn_params* p, const void* q, const void* k, const void* v) {
    S16AttnArgs a{};
    a.q = static_cast<const u16*>(q); a.k = static_cast<const u16*>(k); a.v = static_cast<const u16*>(v);
    a.L = p->L; a.ci = p->ci; a.frames = p->frames;
    a.nob = (p->L + SA_T - 1) / SA_T;
    a.ldq = p->ldq; a.ldk = p->ldk; a.ldv = p->ldv;
    return a;
}

}  // namespace

namespace glf {
int init_attn_s16_attrs() {
    hipError_t e;
#define SET_ATTR(fn)                                                                                        \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_S16ATTN); \
    if (e != hipSuccess) return fail(GLF_ERR_LAUNCH, "hipFuncSetAttribute(" #fn "): %s", hipGetErrorString(e));
    SET_ATTR((attn_s16_kernel<SA_FWD>))
    SET_ATTR((attn_s16_kernel<SA_DV>))
    SET_ATTR((attn_s16_kernel<SA_DK>))
    SET_ATTR((attn_s16_kernel<SA_DQ>))
#undef SET_ATTR
    return GLF_OK;
}
}  // namespace glf

extern "C" int glf_s16_attn_softmax_fwd(const void* theta, const void* phi, const void* g, void* y, float* lse,
                                        const glf_attn_params* p, glf_stream_t stream) {
    if (int rc = s16_attn_check(p, theta, phi, g, y && lse, "s16_attn_softmax_fwd")) return rc;
    if (int rc = glf::ensure_init()) return rc;
    S16AttnArgs a = s16_attn_args(p, theta, phi, g);
    a.out = static_cast<u16*>(y); a.ldo = p->ldy; a.lse_out = lse;
    const unsigned grid = (unsigned)((long long)a.nob * p->frames);
    hipLaunchKernelGGL((attn_s16_kernel<SA_FWD>), dim3(grid), dim3(SA_NT), SMEM_S16ATTN, glf::S(stream), a);
    return glf::check_launch("s16_attn_softmax_fwd");
}

extern "C" int glf_s16_attn_softmax_bwd(const void* theta, const void* phi, const void* g, const void* y, const void* dy, const float* lse,
                                        void* dtheta, void* dphi, void* dg, float* dsum_ws, const glf_attn_params* p, glf_stream_t stream) {
    if (int rc = s16_attn_check(p, theta, phi, g, y && dy && lse && dtheta && dphi && dg && dsum_ws, "s16_attn_softmax_bwd")) return rc;
    GLF_REQUIRE(stride_ok(p->lddy, p->ci) && stride_ok(p->ldd, p->ci), GLF_ERR_UNSUPPORTED,
                "s16_attn_softmax_bwd: dy / gradient row strides must be multiples of 8 elements and >= Ci");
    GLF_REQUIRE(aligned16(y) && aligned16(dy), GLF_ERR_UNSUPPORTED, "s16_attn_softmax_bwd: y / dy must be 16-byte aligned");
    if (int rc = glf::ensure_init()) return rc;
    const long long rows = (long long)p->frames * p->L;
    hipLaunchKernelGGL(attn_s16_rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, glf::S(stream), static_cast<const u16*>(dy),
                       (long long)p->lddy, static_cast<const u16*>(y), (long long)p->ldy, dsum_ws, rows, p->ci);
    S16AttnArgs a = s16_attn_args(p, theta, phi, g);
    a.dy = static_cast<const u16*>(dy); a.lddy = p->lddy;
    a.lse = lse; a.dsum = dsum_ws;
    a.ldo = p->ldd;
    const unsigned grid = (unsigned)((long long)a.nob * p->frames);
    a.out = static_cast<u16*>(dg);
    hipLaunchKernelGGL((attn_s16_kernel<SA_DV>), dim3(grid), dim3(SA_NT), SMEM_S16ATTN, glf::S(stream), a);
    a.out = static_cast<u16*>(dphi);
    hipLaunchKernelGGL((attn_s16_kernel<SA_DK>), dim3(grid), dim3(SA_NT), SMEM_S16ATTN, glf::S(stream), a);
    a.out = static_cast<u16*>(dtheta);
    hipLaunchKernelGGL((attn_s16_kernel<SA_DQ>), dim3(grid), dim3(SA_NT), SMEM_S16ATTN, glf::S(stream), a);
    return glf::check_launch("s16_attn_softmax_bwd");
}

// Fused pairwise-ReLU attention of the fusion block's `concatenate` mode under 16-bit storage (include/glfusion.h:
// glf_s16_attn_pair_relu_fwd / _bwd, glf_s16_attn_pair_proj_fwd / _bwd).  The mathematics is attn_pair.hip's:
//      s_ij = (a_i + b_j) + c ;  y = relu(s) g / L ;  dg = relu(s)^T dY / L ;  ds = [s > 0] (dY g^T) / L ;
//      da_i = sum_j ds_ij ;  db_j = sum_i ds_ij ;  dc = sum_ij ds_ij
// g, dY, y and dg are bf16 [L][Ci] rows (column slices of the [rows][3 Ci] qkv / dqkv buffers); a, b, da, db stay fp32
// [frames * L] (one scalar per position); c is read through a device pointer.  Nothing of size L x L is written.
//
// Arithmetic contract:
//   * s is evaluated as (a_i + b_j) + c in fp32 in all three kernels, so the backward mask [s > 0] is the forward's.
//   * the relu(s) tile is computed on the VALU in fp32 and rounded to bf16 only as the A operand of
//     v_mfma_f32_32x32x16_bf16; y and dg are accumulated in fp32, scaled by 1 / L in fp32 and stored as bf16 once.
//   * t = dY g^T on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (exact bf16 x bf16 products), masked in fp32 and summed
//     to da / db in a fixed order; dc is the sum of da in one workgroup, a fixed tree in double.
//   * every output element is written exactly once: no atomics, no zero fill, two runs are bitwise equal.
//
// Work decomposition: attn_s16.hip's skeleton.  A workgroup = 512 threads = 8 waves owns 64 outer rows (FWD: query rows i, DG:
// key rows j) and keeps their 64 x Ci fp32 accumulator block in registers (wave w: columns [128 w, 128 w + 128)).  The T tile
// [outer][inner] comes from 64 + 64 scalars, not from a contraction, so FWD and DG have NO score steps: an inner block is 4
// product steps of 16 inner rows, Z (FWD g, DG dY) [16][Ci] staged whole by LDS-DMA into the three-slot ring.  The inner
// scalars of block ib + 1 travel with the last product step of block ib (dword LDS-DMA, wave 0); its tile is built there, into
// the second of two alternating T tiles, so the one barrier per step orders the tile's writes and its reads.
// DS: a workgroup owns 64 query rows and walks the key blocks as a stream of Ci / 64 score steps each (dY and g [64][64]
// tiles); wave w forms the 16 x 32 strip (query block w & 3, key blocks 2 (w >> 2) + {0, 1}).  The masked fp32 tile goes to
// LDS; 8 threads per query row add it to da (carried across the key blocks), thread 64 + key adds its column (this query
// block's partial row of db, [frames][ceil(L / 64)][L] floats of caller-owned workspace that a second kernel adds in block order).
// LDS: FWD / DG 3 x 33,280 B ring + two 8 KiB T tiles = 116,224 B; DS ring + one fp32 64 x 68 tile + 64 scalars = 117,504 B.
#include "attn_s16_stage.h"

namespace {

enum PairS16Mode { PS_FWD = 0, PS_DG = 1 };

constexpr int PS_SLD = 68;                                  // fp32 row stride of the ds tile
constexpr int PS_RING = SA_NSLOT * SA_SLOT;
constexpr int PS_TT = PS_RING;                              // FWD / DG: two bf16 [64][64] T tiles
constexpr size_t SMEM_PAIR_ACC = PS_TT + 2 * SA_T * SA_T * 2;
constexpr int PS_TS = PS_RING;                              // DS: the masked tile [64][PS_SLD] fp32
constexpr int PS_AS = PS_TS + SA_T * PS_SLD * 4;            // DS: a of the 64 query rows
constexpr size_t SMEM_PAIR_DS = PS_AS + SA_T * 4;

struct PairS16Args {
    const float* a; const float* b; const float* c;       // [frames * L], [frames * L], one device scalar
    const u16* g; const u16* dy;                          // bf16 rows of length ci, row strides ldg / lddy
    u16* out;                                             // FWD: y (row stride ldo); DG: dg
    float* da; float* dbp;                                // DS: da [frames * L], db partials [frames][nob][L]
    int L, ci, nob;
    long long ldg, lddy, ldo;
};

// FWD: outer = query rows i, inner = key rows j, acc_i += relu(s_ij) g_j.  DG: outer = key rows j, inner = query rows i,
// acc_j += relu(s_ij) dy_i.
template <int MODE>
__global__ __launch_bounds__(SA_NT, 1) void attn_pair_s16_kernel(const PairS16Args args) {
    const int L = args.L, ci = args.ci;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = xcd_remap(blockIdx.x, gridDim.x);        // consecutive outer blocks (one frame) on one XCD: its L2 serves them
    const long long fr = bid / args.nob;
    const int o0 = (bid - (int)fr * args.nob) * SA_T;
    const float* __restrict__ VO = (MODE == PS_FWD ? args.a : args.b) + fr * L;      // the outer rows' scalars
    const float* __restrict__ VI = (MODE == PS_FWD ? args.b : args.a) + fr * L;      // the inner rows' scalars
    const u16* __restrict__ Z = MODE == PS_FWD ? args.g + fr * L * args.ldg : args.dy + fr * L * args.lddy;
    const long long ldz = MODE == PS_FWD ? args.ldg : args.lddy;
    const float cc = *args.c;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int nblk = (L + SA_T - 1) / SA_T;
    const int zins = ci / 32;                                 // LDS-DMA instructions of a product step (16 rows x Ci)
    const int zcnt = zins > wave ? (zins - wave + 7) / 8 : 0; // ... this wave's share

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
    // step (ib_, j_): Z rows 64 ib_ + 16 j_ .. + 15; the last step of a block also carries the next block's inner scalars
    auto issue = [&](int ib_, int j_, int slot_) __attribute__((always_inline)) {
        unsigned char* sb = smem + slot_ * SA_SLOT;
        const int r0 = ib_ * SA_T + 16 * j_;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (wave + 8 * u < zins) glds16(Z + (long long)min(r0 + zrow[u], L - 1) * ldz + zcol[u], sb + (wave + 8 * u) * 1024);
        }
        if (j_ == 3 && ib_ + 1 < nblk && wave == 0) glds4(VI + min((ib_ + 1) * SA_T + lane, L - 1), sb + 32768);
    };
    // product step: A rows 32 i + (lane & 31) of T, chunk 2 s' + (lane >> 5) for the 16-row k-step s'; B by transposed reads:
    // lane 4 q + p of group g addresses Z row 8 (g >> 1) + q (second read + 4), columns 32 jt + 16 (g & 1) + 4 p of the wave's
    // 128 columns
    const int g4 = lane >> 4;
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

    // the T tile: thread -> outer row tid >> 3, inner rows 8 (tid & 7) .. + 7, one 16-byte write
    const int row = tid >> 3, part = tid & 7;
    const bool o_ok = o0 + row < L;
    const float vo = VO[min(o0 + row, L - 1)];
    auto build = [&](int ib_, const float (&vi)[8]) __attribute__((always_inline)) {
        float pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float s = (vo + vi[e]) + cc;
            pv[e] = (o_ok && ib_ * SA_T + 8 * part + e < L) ? fmaxf(s, 0.f) : 0.f;
        }
        uint4 o;
        o.x = pack2(pv[0], pv[1]); o.y = pack2(pv[2], pv[3]); o.z = pack2(pv[4], pv[5]); o.w = pack2(pv[6], pv[7]);
        *reinterpret_cast<uint4*>(smem + PS_TT + (ib_ & 1) * (SA_T * SA_T * 2) + tt_off(row, 8 * part)) = o;
    };
    {
        float vi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) vi[e] = VI[min(8 * part + e, L - 1)];
        build(0, vi);                                         // block 0's scalars straight from memory, before the ring starts
    }

    // the step stream: step t waits for its own loads, passes the barrier, then issues step t + 2 into the slot step t - 1 used
    int slot = 0;
    int ibf = 0, jf = 2;                                      // step t + 2
    issue(0, 0, 0);
    issue(0, 1, 1);
    auto begin_step = [&](int next_cnt) __attribute__((always_inline)) {
        wait_vm(next_cnt);                                    // this step landed (this wave's part); the next one may fly
        __builtin_amdgcn_s_barrier();                         // ... everyone's part; everyone is done with the previous slot
        asm volatile("" ::: "memory");                        // no LDS access moves across the barrier
        if (ibf < nblk) {
            issue(ibf, jf, slot == 0 ? 2 : slot - 1);
            if (++jf == 4) { jf = 0; ++ibf; }
        }
    };
    for (int ib = 0; ib < nblk; ++ib) {
        const unsigned char* Tt = smem + PS_TT + (ib & 1) * (SA_T * SA_T * 2);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool more = ib + 1 < nblk;
            begin_step((s == 3 && !more) ? 0 : zcnt + ((s == 2 && more && wave == 0) ? 1 : 0));
            if (s == 3 && more) {
                // the other T tile: its last readers (block ib - 1) are behind this block's first barrier
                const float* st = reinterpret_cast<const float*>(smem + slot * SA_SLOT + 32768);
                const float4 x0 = *reinterpret_cast<const float4*>(st + 8 * part);
                const float4 x1 = *reinterpret_cast<const float4*>(st + 8 * part + 4);
                const float vi[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                build(ib + 1, vi);
            }
            if (128 * wave < ci) {
                // all four column tiles, also where Ci % 128 == 64 leaves the last two beyond Ci: their reads stay inside the LDS
                // allocation and their results are never stored
                bf16x8 af[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(Tt + tm[i] + (((2 * s + hl) ^ tsw[i]) << 4));
                // the eight transposing reads and their wait in ONE asm statement (attn_s16.hip)
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

    // ---- epilogue: rows o0 + 32 i + (r & 3) + 8 (r >> 2) + 4 hl, columns 32 (4 w + jt) + l31; 1 / L in fp32, bf16 once ----
    u16* __restrict__ OUT = args.out + fr * L * args.ldo;
    const float scale = 1.f / (float)L;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = o0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hl;
            if (orow < L) {
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    const int c = 32 * (4 * wave + jt) + l31;
                    if (c < ci) OUT[(long long)orow * args.ldo + c] = (u16)(pack2(acc[i][jt][r] * scale, 0.f) & 0xffffu);
                }
            }
        }
    }
}

// DS: t = dY g^T over Ci, ds = t [s > 0]; da carried across the key blocks, db as this query block's partial row
__global__ __launch_bounds__(SA_NT, 1) void attn_pair_s16_ds_kernel(const PairS16Args args) {
    const int L = args.L, ci = args.ci;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long long fr = bid / args.nob;
    const int ob = bid - (int)fr * args.nob;
    const int o0 = ob * SA_T;
    const float* __restrict__ A = args.a + fr * L;
    const float* __restrict__ B = args.b + fr * L;
    const u16* __restrict__ G = args.g + fr * L * args.ldg;
    const u16* __restrict__ DY = args.dy + fr * L * args.lddy;
    const long long ldg = args.ldg, lddy = args.lddy;
    const float cc = *args.c;
    const int nblk = args.nob;
    float* __restrict__ DBP = args.dbp + (fr * nblk + ob) * L;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Ts = reinterpret_cast<float*>(smem + PS_TS);
    float* As = reinterpret_cast<float*>(smem + PS_AS);

    const int nsc = ci / 64;                                  // score steps per key block

    // staging: wave w fills rows 8 w .. 8 w + 7 of both tiles, lane -> row 8 w + (lane >> 3), chunk lane & 7
    const int srow = 8 * wave + (lane >> 3);
    const int scol = ((lane & 7) ^ ((srow >> 1) & 7)) * 8;
    const long long rq = min(o0 + srow, L - 1);
    // step (ib_, j_): dY rows of the query block and g rows of key block ib_, columns 64 j_ .. + 63; the last step of a key
    // block also carries its b scalars
    auto issue = [&](int ib_, int j_, int slot_) __attribute__((always_inline)) {
        unsigned char* sb = smem + slot_ * SA_SLOT;
        const long long rk = min(ib_ * SA_T + srow, L - 1);
        const int col = j_ * 64 + scol;
        glds16(DY + rq * lddy + col, sb + wave * 1024);
        glds16(G + rk * ldg + col, sb + 8192 + wave * 1024);
        if (j_ == nsc - 1 && wave == 0) glds4(B + min(ib_ * SA_T + lane, L - 1), sb + 32768);
    };
    // fragment offsets: query rows 16 (w & 3) + (lane & 15), key rows 16 kb + (lane & 15), kb = 2 (w >> 2) + t; k-step s
    // (32 columns) reads chunk 4 s + (lane >> 4)
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

    if (tid < SA_T) As[tid] = A[min(o0 + tid, L - 1)];        // read behind the first step's barrier
    f32x4_ sacc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) sacc[t] = f32x4_{0, 0, 0, 0};
    float da = 0.f;

    int slot = 0;
    int ibf = 0, jf = 0;                                      // the next step to issue
    auto issue_next = [&](int slot_) __attribute__((always_inline)) {
        if (ibf < nblk) {
            issue(ibf, jf, slot_);
            if (++jf == nsc) { jf = 0; ++ibf; }
        }
    };
    issue_next(0);
    issue_next(1);
    for (int ib = 0; ib < nblk; ++ib) {
        const int i0 = ib * SA_T;
        for (int j = 0; j < nsc; ++j) {
            // the next step: (ib, j + 1), or the first of the next key block, or none
            const bool has_next = j + 1 < nsc || ib + 1 < nblk;
            const int jn = j + 1 < nsc ? j + 1 : 0;
            wait_vm(has_next ? 2 + ((jn == nsc - 1 && wave == 0) ? 1 : 0) : 0);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            issue_next(slot == 0 ? 2 : slot - 1);
            const unsigned char* sb = smem + slot * SA_SLOT;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 x = *reinterpret_cast<const bf16x8*>(sb + fx[s]);
                const bf16x8 y0 = *reinterpret_cast<const bf16x8*>(sb + 8192 + fy[0][s]);
                const bf16x8 y1 = *reinterpret_cast<const bf16x8*>(sb + 8192 + fy[1][s]);
                sacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y0, sacc[0], 0, 0, 0);
                sacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y1, sacc[1], 0, 0, 0);
            }
            if (j == nsc - 1) {
                // the tile is complete: mask in fp32, to LDS as [q][key] (this step's slot, which holds the b scalars, is refilled
                // only behind the next barrier; the row / column sums of the previous tile are behind this step's barrier)
                const float* bs = reinterpret_cast<const float*>(sb + 32768);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const int kl = 16 * (2 * (wave >> 2) + tt) + l15;
                    const float bk = bs[kl];
                    const bool key_ok = i0 + kl < L;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ql = 16 * (wave & 3) + 4 * g4 + r;
                        const float s = (As[ql] + bk) + cc;
                        Ts[ql * PS_SLD + kl] = (key_ok && o0 + ql < L && s > 0.f) ? sacc[tt][r] : 0.f;
                    }
                }
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) sacc[tt] = f32x4_{0, 0, 0, 0};
                __syncthreads();
                {
                    // da: 8 threads per query row, 8 keys each, then a fixed butterfly
                    const int row = tid >> 3, part = tid & 7;
                    const float4 x0 = *reinterpret_cast<const float4*>(Ts + row * PS_SLD + 8 * part);
                    const float4 x1 = *reinterpret_cast<const float4*>(Ts + row * PS_SLD + 8 * part + 4);
                    float sum = ((x0.x + x0.y) + (x0.z + x0.w)) + ((x1.x + x1.y) + (x1.z + x1.w));
                    sum += __shfl_xor(sum, 1, 64);
                    sum += __shfl_xor(sum, 2, 64);
                    sum += __shfl_xor(sum, 4, 64);
                    da += sum;
                }
                if (tid >= SA_T && tid < 2 * SA_T) {
                    const int col = tid - SA_T;
                    float sum = 0.f;
#pragma unroll 16
                    for (int q = 0; q < SA_T; ++q) sum += Ts[q * PS_SLD + col];
                    if (i0 + col < L) DBP[i0 + col] = sum;
                }
            }
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    if ((tid & 7) == 0 && o0 + (tid >> 3) < L) args.da[fr * L + o0 + (tid >> 3)] = da / (float)L;
}

// db[fr][j] = (1 / L) sum over the query blocks, in block order, of their partial rows
__global__ __launch_bounds__(256) void attn_pair_s16_db_kernel(const float* __restrict__ dbp, float* __restrict__ db, int frames, int L, int nblk) {
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
__global__ __launch_bounds__(256) void attn_pair_s16_total_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
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

// ---- the skinny ends of the mode: bf16 theta / phi [rows][Ci] against the two halves of the fp32 W_f row ------------------------
// a[row] = theta[row] . w[0 .. ci), b[row] = phi[row] . w[ci .. 2 ci): one wavefront per row, 8 columns per lane and load, fp32 sums
__global__ __launch_bounds__(256) void pair_s16_proj_fwd_kernel(const u16* __restrict__ th, const u16* __restrict__ ph, long long ld,
                                                                const float* __restrict__ w, float* __restrict__ a, float* __restrict__ b,
                                                                long long rows, int ci) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float sa = 0.f, sb = 0.f;
    for (int c = 8 * lane; c < ci; c += 512) {
        const glf::F8 t = glf::ld8(th + row * ld + c), p = glf::ld8(ph + row * ld + c);
        const glf::F8 wt = glf::ldf8(w + c), wp = glf::ldf8(w + ci + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sa = fmaf(t.v[e], wt.v[e], sa);
            sb = fmaf(p.v[e], wp.v[e], sb);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o, 64);
        sb += __shfl_xor(sb, o, 64);
    }
    if (lane == 0) { a[row] = sa; b[row] = sb; }
}

constexpr int PPS_ROWS = 256;      // rows per slab of the W_f gradient's first stage
// dtheta[row][c] = bf16(da[row] w[c]), dphi[row][c] = bf16(db[row] w[ci + c]), and the slab's partial of
// dw[c] = sum_row da[row] theta[row][c] (c < ci; phi / db for the second half).  Thread = one of the 2 ci columns, rows in order.
__global__ __launch_bounds__(256) void pair_s16_proj_bwd_kernel(const u16* __restrict__ th, const u16* __restrict__ ph, long long ld,
                                                                const float* __restrict__ w, const float* __restrict__ da,
                                                                const float* __restrict__ db, u16* __restrict__ dth, u16* __restrict__ dph,
                                                                long long ldd, float* __restrict__ part, long long rows, int ci) {
    const int col = blockIdx.y * 256 + threadIdx.x;
    if (col >= 2 * ci) return;
    const bool second = col >= ci;
    const int c = second ? col - ci : col;
    const u16* __restrict__ src = (second ? ph : th) + c;
    const float* __restrict__ d = second ? db : da;
    u16* __restrict__ dst = (second ? dph : dth) + c;
    const float wc = w[col];
    const long long r0 = (long long)blockIdx.x * PPS_ROWS;
    const long long r1 = r0 + PPS_ROWS < rows ? r0 + PPS_ROWS : rows;
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float dr = d[r];
        s = fmaf(dr, glf::bf2f(src[r * ld]), s);
        dst[r * ldd] = glf::f2bf(dr * wc);
    }
    part[(long long)blockIdx.x * 2 * ci + col] = s;
}

// dw[col] = sum over the slabs, in slab order, in double
__global__ __launch_bounds__(256) void pair_s16_proj_dw_kernel(const float* __restrict__ part, float* __restrict__ dw, int nslab, int cols) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    double s = 0.0;
    for (int b = 0; b < nslab; ++b) s += (double)part[(long long)b * cols + col];
    dw[col] = (float)s;
}

bool pstride_ok(long long ld, int ci) { return ld >= ci && ld % 8 == 0; }

// NULL, then extents, then support; `others_ok`: the entry point's remaining pointers are all non-null
int pair16_check(const glf_attn_pair_params* p, const void* a, const void* b, const void* c, const void* g, bool others_ok, const char* what) {
    GLF_REQUIRE(p && a && b && c && g && others_ok, GLF_ERR_NULL, "%s: null argument", what);
    GLF_REQUIRE(p->frames >= 1 && p->L >= 1, GLF_ERR_BAD_SHAPE, "%s: frames (%d) and L (%d) must be >= 1", what, p->frames, p->L);
    GLF_REQUIRE((long long)p->frames * ((p->L + SA_T - 1) / SA_T) < (1ll << 31), GLF_ERR_BAD_SHAPE, "%s: frames * ceil(L / 64) too large", what);
    GLF_REQUIRE(p->ci >= 64 && p->ci % 64 == 0 && p->ci <= SA_MAXCI, GLF_ERR_UNSUPPORTED,
                "%s: Ci must be a multiple of 64 and <= %d (got %d)", what, SA_MAXCI, p->ci);
    GLF_REQUIRE(pstride_ok(p->ldg, p->ci) && aligned16(g), GLF_ERR_UNSUPPORTED,
                "%s: g must be 16-byte aligned with a row stride that is a multiple of 8 elements and >= Ci", what);
    return GLF_OK;
}

PairS16Args pair16_args(const glf_attn_pair_params* p, const float* a, const float* b, const float* c, const void* g) {
    PairS16Args x{};
    x.a = a; x.b = b; x.c = c; x.g = static_cast<const u16*>(g);
    x.L = p->L; x.ci = p->ci; x.nob = (p->L + SA_T - 1) / SA_T;
    x.ldg = p->ldg;
    return x;
}

}  // namespace

namespace glf {
int init_attn_pair_s16_attrs() {
    hipError_t e;
#define SET_ATTR(fn, bytes)                                                                                 \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
    if (e != hipSuccess) return fail(GLF_ERR_LAUNCH, "hipFuncSetAttribute(" #fn "): %s", hipGetErrorString(e));
    SET_ATTR((attn_pair_s16_kernel<PS_FWD>), SMEM_PAIR_ACC)
    SET_ATTR((attn_pair_s16_kernel<PS_DG>), SMEM_PAIR_ACC)
    SET_ATTR(attn_pair_s16_ds_kernel, SMEM_PAIR_DS)
#undef SET_ATTR
    return GLF_OK;
}
}  // namespace glf

extern "C" size_t glf_s16_attn_pair_relu_workspace_bytes(const glf_attn_pair_params* p) {
    if (!p || p->frames <= 0 || p->L <= 0) return 0;
    return (size_t)p->frames * (size_t)((p->L + SA_T - 1) / SA_T) * (size_t)p->L * sizeof(float);
}

extern "C" int glf_s16_attn_pair_relu_fwd(const float* a, const float* b, const float* c, const void* g, void* y,
                                          const glf_attn_pair_params* p, glf_stream_t stream) {
    if (int rc = pair16_check(p, a, b, c, g, y != nullptr, "s16_attn_pair_relu_fwd")) return rc;
    GLF_REQUIRE(pstride_ok(p->ldy, p->ci), GLF_ERR_UNSUPPORTED, "s16_attn_pair_relu_fwd: ldy must be a multiple of 8 elements and >= Ci");
    if (int rc = glf::ensure_init()) return rc;
    PairS16Args x = pair16_args(p, a, b, c, g);
    x.out = static_cast<u16*>(y); x.ldo = p->ldy;
    const unsigned grid = (unsigned)((long long)x.nob * p->frames);
    hipLaunchKernelGGL((attn_pair_s16_kernel<PS_FWD>), dim3(grid), dim3(SA_NT), SMEM_PAIR_ACC, glf::S(stream), x);
    return glf::check_launch("s16_attn_pair_relu_fwd");
}

extern "C" int glf_s16_attn_pair_relu_bwd(const float* a, const float* b, const float* c, const void* g, const void* dy, void* dg,
                                          float* da, float* db, float* dc, float* workspace, int64_t workspace_bytes,
                                          const glf_attn_pair_params* p, glf_stream_t stream) {
    if (int rc = pair16_check(p, a, b, c, g, dy && dg && da && db && dc && workspace, "s16_attn_pair_relu_bwd")) return rc;
    GLF_REQUIRE(pstride_ok(p->lddy, p->ci) && pstride_ok(p->lddg, p->ci) && aligned16(dy), GLF_ERR_UNSUPPORTED,
                "s16_attn_pair_relu_bwd: dy must be 16-byte aligned, the row strides of dy / dg multiples of 8 elements and >= Ci");
    GLF_REQUIRE(workspace_bytes >= (int64_t)glf_s16_attn_pair_relu_workspace_bytes(p), GLF_ERR_WORKSPACE,
                "s16_attn_pair_relu_bwd: workspace of %lld bytes, glf_s16_attn_pair_relu_workspace_bytes() asks for %zu", (long long)workspace_bytes,
                glf_s16_attn_pair_relu_workspace_bytes(p));
    if (int rc = glf::ensure_init()) return rc;
    PairS16Args x = pair16_args(p, a, b, c, g);
    x.dy = static_cast<const u16*>(dy); x.lddy = p->lddy;
    x.out = static_cast<u16*>(dg); x.ldo = p->lddg;
    x.da = da; x.dbp = workspace;
    const unsigned grid = (unsigned)((long long)x.nob * p->frames);
    hipLaunchKernelGGL((attn_pair_s16_kernel<PS_DG>), dim3(grid), dim3(SA_NT), SMEM_PAIR_ACC, glf::S(stream), x);
    hipLaunchKernelGGL(attn_pair_s16_ds_kernel, dim3(grid), dim3(SA_NT), SMEM_PAIR_DS, glf::S(stream), x);
    const long long rows = (long long)p->frames * p->L;
    hipLaunchKernelGGL(attn_pair_s16_db_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, glf::S(stream), workspace, db, p->frames, p->L,
                       x.nob);
    hipLaunchKernelGGL(attn_pair_s16_total_kernel, dim3(1), dim3(256), 0, glf::S(stream), da, rows, dc);
    return glf::check_launch("s16_attn_pair_relu_bwd");
}

extern "C" size_t glf_s16_attn_pair_proj_workspace_bytes(int64_t rows, int ci) {
    if (rows <= 0 || ci <= 0) return 0;
    return (size_t)((rows + PPS_ROWS - 1) / PPS_ROWS) * 2 * (size_t)ci * sizeof(float);
}

extern "C" int glf_s16_attn_pair_proj_fwd(const void* theta, const void* phi, int64_t ld, const float* w, float* a, float* b, int64_t rows, int ci,
                                          glf_stream_t stream) {
    GLF_REQUIRE(theta && phi && w && a && b, GLF_ERR_NULL, "s16_attn_pair_proj_fwd: null argument");
    GLF_REQUIRE(rows > 0 && rows < (1LL << 33) && ci > 0 && ld >= ci, GLF_ERR_BAD_SHAPE, "s16_attn_pair_proj_fwd: bad shape");
    GLF_REQUIRE(ci % 8 == 0 && ld % 8 == 0 && aligned16(theta) && aligned16(phi) && aligned16(w), GLF_ERR_UNSUPPORTED,
                "s16_attn_pair_proj_fwd: Ci and ld must be multiples of 8, theta / phi / w 16-byte aligned");
    if (int rc = glf::ensure_init()) return rc;
    hipLaunchKernelGGL(pair_s16_proj_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, glf::S(stream), static_cast<const u16*>(theta),
                       static_cast<const u16*>(phi), (long long)ld, w, a, b, (long long)rows, ci);
    return glf::check_launch("s16_attn_pair_proj_fwd");
}

extern "C" int glf_s16_attn_pair_proj_bwd(const void* theta, const void* phi, int64_t ld, const float* w, const float* da, const float* db,
                                          void* dtheta, void* dphi, int64_t ldd, float* dw, float* workspace, int64_t workspace_bytes, int64_t rows,
                                          int ci, glf_stream_t stream) {
    GLF_REQUIRE(theta && phi && w && da && db && dtheta && dphi && dw && workspace, GLF_ERR_NULL, "s16_attn_pair_proj_bwd: null argument");
    GLF_REQUIRE(rows > 0 && ci > 0 && ld >= ci && ldd >= ci, GLF_ERR_BAD_SHAPE, "s16_attn_pair_proj_bwd: bad shape");
    const long long nslab = (rows + PPS_ROWS - 1) / PPS_ROWS;
    GLF_REQUIRE(nslab < 2147483647LL && (2 * ci + 255) / 256 <= 65535, GLF_ERR_BAD_SHAPE, "s16_attn_pair_proj_bwd: rows / Ci out of range");
    GLF_REQUIRE(workspace_bytes >= (int64_t)glf_s16_attn_pair_proj_workspace_bytes(rows, ci), GLF_ERR_WORKSPACE,
                "s16_attn_pair_proj_bwd: workspace of %lld bytes, glf_s16_attn_pair_proj_workspace_bytes() asks for %zu", (long long)workspace_bytes,
                glf_s16_attn_pair_proj_workspace_bytes(rows, ci));
    if (int rc = glf::ensure_init()) return rc;
    hipLaunchKernelGGL(pair_s16_proj_bwd_kernel, dim3((unsigned)nslab, (2 * ci + 255) / 256), dim3(256), 0, glf::S(stream),
                       static_cast<const u16*>(theta), static_cast<const u16*>(phi), (long long)ld, w, da, db, static_cast<u16*>(dtheta),
                       static_cast<u16*>(dphi), (long long)ldd, workspace, (long long)rows, ci);
    hipLaunchKernelGGL(pair_s16_proj_dw_kernel, dim3((2 * ci + 255) / 256), dim3(256), 0, glf::S(stream), workspace, dw, (int)nslab, 2 * ci);
    return glf::check_launch("s16_attn_pair_proj_bwd");
}

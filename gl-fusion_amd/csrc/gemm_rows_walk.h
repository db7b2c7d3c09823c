// What the NT ("rows") kernels share: which rows a workgroup owns (one tile enumeration for the launchers and the kernels), the
// order the tiles are walked in, the per-thread state of the A rows a thread stages, and the output epilogue of the two
// split-fp16 tile configurations (gemm_f16s.hip: 8 waves, 256 rows; gemm_f16s4.hip: 4 waves, 128 rows).  gemm_s16.hip takes the
// enumeration, the tile order and the row state.  The exact-fp32 rows kernel (gemm_f32.hip, 128 rows) and the bf16x6 rows kernel
// (gemm_bf16s.hip, 256 rows) take those three and the plain output epilogue at the end of this file; what stays with them is the
// staging of padding / overhang rows, a clamped load zeroed by a select instead of a load from the zero page (rows_next_tap).
//
// Every helper is __forceinline__ and takes scalars or a struct of scalars, never GemmArgs: a by-reference use of the by-value
// kernel argument made hipcc spill the whole struct (gemm_common.h, GeoS).
#pragma once
#include "gemm_common.h"

namespace {

struct RowsGeo { int gather, n_img, hs, ws, hd, wd, kw, stride, pad, dil; };

// One row tile.  In: tm = index of the tile in the launch's order, the other fields as for a plain launch (rows = M, the whole
// destination map, the caller's tap mask).  Out of rows_locate(): tm = index inside its region / tap rectangle, rows = rows of
// that part, (y0, x0, h, w) = its rectangle of destination pixels, mask = the taps it contracts.
struct RowTile { int tm, rows, y0, x0, h, w; unsigned mask; };

// The row tiles of a rect != 0 launch, part after part: the nine regions of region_of() (rect = 2) or one rectangle per kept tap
// (rect = 1, tap_rect()), each cut into BM_-row tiles of its own with a ragged last one.
// DROP_EMPTY: whether a region none of whose taps is kept by tap_mask gets tiles.  The split-fp16 launches drop it (true): they
// may accumulate onto C, and rows without a product must keep their old values.  The bf16-storage launch keeps it (false): it
// stores every output element exactly once, so those rows have to be written (zeros plus bias).
// LOCATE = false: returns the number of row tiles.  LOCATE = true: finds tile t.tm, returns 0 when there is no such tile.
template <int BM_, bool DROP_EMPTY, bool LOCATE>
__host__ __device__ __forceinline__ long long rows_walk(int rect, unsigned tap_mask, const RowsGeo& g, RowTile& t) {
    long long total = 0;
    if (rect == 2) {
        bool found = false;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            int y0, y1, x0, x1;
            unsigned rm;
            region_of(g.gather, r, g.dil, g.hd, g.wd, y0, y1, x0, x1, rm);
            const int mt = g.n_img * (y1 - y0) * (x1 - x0);
            const int tiles = (!DROP_EMPTY || (rm & tap_mask)) ? (mt + BM_ - 1) / BM_ : 0;
            total += tiles;
            if (LOCATE && !found) {
                if (t.tm < tiles) { found = true; t.mask = rm & tap_mask; t.rows = mt; t.y0 = y0; t.x0 = x0; t.h = y1 - y0; t.w = x1 - x0; }
                else t.tm -= tiles;
            }
        }
        return LOCATE ? (long long)found : total;
    }
    for (unsigned mm = tap_mask; mm; mm &= mm - 1) {
        const int tap = __builtin_ctz(mm);
        int y0, y1, x0, x1;
        tap_rect(g.gather, tap, g.kw, g.pad, g.dil, g.hs, g.ws, g.hd, g.wd, y0, y1, x0, x1);
        const int mt = g.n_img * (y1 - y0) * (x1 - x0);
        const int tiles = (mt + BM_ - 1) / BM_;
        total += tiles;
        if (LOCATE) {
            if (t.tm < tiles || (mm & (mm - 1)) == 0) { t.mask = 1u << tap; t.rows = mt; t.y0 = y0; t.x0 = x0; t.h = y1 - y0; t.w = x1 - x0; break; }
            t.tm -= tiles;
        }
    }
    return LOCATE ? 1 : total;
}

// launchers: row tiles of a launch (0 is possible: region mode with every region's tap set empty under the mask)
template <int BM_, bool DROP_EMPTY>
inline long long rows_tiles_m(int rect, int M, unsigned tap_mask, const Geo& g, int gather) {
    if (!rect) return (M + BM_ - 1) / BM_;
    const RowsGeo rg{gather, g.n_img, g.hs, g.ws, g.hd, g.wd, g.kw, g.stride, g.pad, g.dil};
    RowTile t{};
    return rows_walk<BM_, DROP_EMPTY, false>(rect, tap_mask, rg, t);
}

// kernels: rect != 0 only; false = this workgroup has no tile
template <int BM_, bool DROP_EMPTY>
__device__ __forceinline__ bool rows_locate(int rect, unsigned tap_mask, const RowsGeo& g, RowTile& t) {
    return rows_walk<BM_, DROP_EMPTY, true>(rect, tap_mask, g, t) != 0;
}

// rect mode (tap-parallel rectangles) of the BM-row kernels: validates and sizes the grid as the sum over taps of their tiles
inline int setup_rect(const glf_gemm_params* p, const float* bias, GemmArgs& a, dim3& grid, const char* who) {
    GLF_REQUIRE(p->gather == 1 || p->gather == 2, GLF_ERR_BAD_SHAPE, "%s: rect mode needs a conv gather", who);
    GLF_REQUIRE(p->stride == 1, GLF_ERR_UNSUPPORTED, "%s: rect mode needs stride 1", who);
    GLF_REQUIRE(bias == nullptr && !p->accumulate && p->batch == 1, GLF_ERR_UNSUPPORTED,
                "%s: rect mode takes no bias / accumulate / batch (C must be zero-filled by the caller)", who);
    const long long tiles = rows_tiles_m<BM, false>(1, p->M, p->tap_mask, a.g, p->gather);
    GLF_REQUIRE(tiles > 0 && tiles * a.tiles_n < 2147483647LL, GLF_ERR_BAD_SHAPE, "%s: rect mode grid out of range", who);
    a.rect = 1;
    grid = dim3((unsigned)(tiles * a.tiles_n), 1, 1);
    return GLF_OK;
}

// Tile order inside an XCD's contiguous range: groups of `gm` row tiles x all column tiles, walked down the rows first, so
// that the ~32 workgroups an XCD runs at a time form a gm x (32 / gm) block of tiles: each A row tile is shared by 32 / gm
// of them and each B column tile by gm of them through that XCD's L2 (gm = 0: the plain row-major order, every B tile
// fetched from the Infinity Cache once per row tile)
__device__ __forceinline__ void rows_tile_order(int gm, int tiles_n, int& tn, int& tm) {
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    if (gm > 1) {
        const int tiles_m_all = gridDim.x / tiles_n;
        const int per_group = gm * tiles_n;
        const int grp = bid / per_group, in_grp = bid - grp * per_group;
        const int first_m = grp * gm;
        const int gsz = min(tiles_m_all - first_m, gm);
        tn = in_grp / gsz;
        tm = first_m + (in_grp - tn * gsz);
    } else {
        tn = bid % tiles_n;
        tm = bid / tiles_n;
    }
}

// ---- row state: the R rows of the A tile a thread stages (rows m0 + STEP j of the part) -----------------------------------
// gather: (n, y, x) = the row's destination pixel, n = -1 past the part's end; after rows_to_fast(): n = source pixel index,
// (y, x) = source coordinates for tap offset (0, 0).  plain / SEG: off = element offset of the row in A, -1 = overhang.
template <int R> struct RowState { int n[R], y[R], x[R]; long long off[R]; };

// pixel coordinates of the thread's first row by division, of the others (STEP rows further each) by carrying.
// SEG (segmented region mode, 8-wave split-fp16 kernel only): the row's own pixel as an offset; a segment adds one uniform offset.
template <int R, int STEP, bool GATHER, bool SEG = false>
__device__ __forceinline__ void rows_init(RowState<R>& s, int m0, const RowTile& t, int lda, int hd, int wd) {
    int cn = 0, cy = 0, cx = 0;
    if (GATHER || SEG) {
        const int hw = t.h * t.w;
        cn = m0 / hw;
        const int rem = m0 - cn * hw;
        cy = rem / t.w; cx = rem - cy * t.w;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int m = m0 + STEP * j;
        if constexpr (SEG || GATHER) {
            if constexpr (SEG) {
                s.n[j] = 0; s.y[j] = 0; s.x[j] = 0;
                s.off[j] = (m < t.rows) ? (long long)((cn * hd + t.y0 + cy) * wd + t.x0 + cx) * lda : -1;
            } else {
                if (m < t.rows) { s.n[j] = cn; s.y[j] = t.y0 + cy; s.x[j] = t.x0 + cx; }
                else { s.n[j] = -1; s.y[j] = 0; s.x[j] = 0; }
                s.off[j] = -1;
            }
            if (j < R - 1 && m + STEP < t.rows) {
                cx += STEP;
                while (cx >= t.w) { cx -= t.w; ++cy; }
                while (cy >= t.h) { cy -= t.h; ++cn; }
            }
        } else {
            s.n[j] = 0; s.y[j] = 0; s.x[j] = 0;
            s.off[j] = (m < t.rows) ? (long long)m * lda : -1;
        }
    }
}

// Fast gather form (forward / wgrad-style gathers, and dgrad gathers of stride-1 convs -- everything but the dgrad of a
// strided conv): a row keeps (rb, y0, x0) = its source pixel index and coordinates for tap offset (0, 0); a tap then is
// one uniform offset pair (oy, ox): source = rb + oy * ws + ox, in range iff 0 <= y0 + oy < hs and 0 <= x0 + ox < ws.  The
// general map_src() (an integer division per call, two more for a strided dgrad, divergent branches around each) cost
// ~3.7 k cycles per tap change and ~20 k in the tap census below: 29 % of a 256 -> 256 3x3 conv's workgroup time
// (in-kernel stamps: prologue 26 k, 2 333 cycles per iteration against 1 869 for a plain GEMM).
__device__ __forceinline__ bool rows_fast_gather(const RowsGeo& g) { return g.gather == 1 || g.stride == 1; }

template <int R>
__device__ __forceinline__ void rows_to_fast(RowState<R>& s, const RowsGeo& g) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (s.n[j] >= 0) {
            const int y0 = (g.gather == 1) ? s.y[j] * g.stride - g.pad : s.y[j] + g.pad;
            const int x0 = (g.gather == 1) ? s.x[j] * g.stride - g.pad : s.x[j] + g.pad;
            s.n[j] = (s.n[j] * g.hs + y0) * g.ws + x0; s.y[j] = y0; s.x[j] = x0;
        } else { s.n[j] = 0; s.y[j] = -(1 << 30); s.x[j] = 0; }          // never in range
    }
}

// tap -> its uniform offsets (oy, ox) in source pixels
__device__ __forceinline__ void tap_offsets(int t, const RowsGeo& g, int& oy, int& ox) {
    int ky = 0, kx = __builtin_amdgcn_readfirstlane(t);
    while (kx >= g.kw) { kx -= g.kw; ++ky; }
    oy = (g.gather == 1 ? ky : -ky) * g.dil;
    ox = (g.gather == 1 ? kx : -kx) * g.dil;
}

// tap census: drop the taps that fall into the padding for EVERY row of this tile.  It can only find one when the tile
// covers fewer than dil + 1 full image rows (otherwise each tap has a row it reaches): skipped for the small dilations.
// `counts`: true in one thread per staged row.  Returns whether it ran (two barriers).
template <int BM_, int R, bool GATHER>
__device__ __forceinline__ bool rows_census(const RowState<R>& s, unsigned& mask, bool fastg, bool counts, int taps, int rect,
                                            const RowsGeo& g, unsigned* s_mask) {
    if (!(GATHER && taps > 1 && !rect && BM_ < g.wd * (g.dil + 1))) return false;
    if (threadIdx.x == 0) *s_mask = 0u;
    __syncthreads();
    if (counts) {
        unsigned local = 0;
        for (unsigned mm = mask; mm; mm &= mm - 1) {
            const int t = __ffs(mm) - 1;
            if (fastg) {
                int oy, ox;
                tap_offsets(t, g, oy, ox);
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if ((unsigned)(s.y[j] + oy) < (unsigned)g.hs && (unsigned)(s.x[j] + ox) < (unsigned)g.ws) local |= 1u << t;
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if (s.n[j] >= 0 && map_src(g.hs, g.ws, g.kw, g.stride, g.pad, g.dil, g.gather, s.n[j], s.y[j], s.x[j], t) >= 0) local |= 1u << t;
            }
        }
        if (local) atomicOr(s_mask, local);
    }
    __syncthreads();
    mask &= *s_mask;
    return true;
}

// tap change: takes the next tap off rem_mask and points the thread's R row pointers at its rows of A (element type T, col[j] =
// the thread's column offset in row j); padding / overhang rows read `zero`, the zero page.  Returns the tap.
// ok != nullptr (the exact-fp32 and bf16x6 kernels): bit j of *ok = row j is a real row.  Those kernels have no zero page --
// it would cap K at its size, and the exact kernel's slow path reads K tails and unaligned rows -- so they pass A itself for
// `zero` (row 0: an address every launch may read) and zero the other rows by a select when the registers go to LDS.
template <int R, bool GATHER, typename T>
__device__ __forceinline__ int rows_next_tap(const RowState<R>& s, unsigned& rem_mask, const T* (&pa)[R], const T* A, const T* zero,
                                             int lda, bool fastg, const RowsGeo& g, const int (&col)[R], unsigned* ok = nullptr) {
    const int tap = __ffs(rem_mask) - 1;
    rem_mask &= rem_mask - 1;
    unsigned real = 0;
    if (fastg) {
        int oy, ox;
        tap_offsets(tap, g, oy, ox);
        const int d = oy * g.ws + ox;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const bool in = (unsigned)(s.y[j] + oy) < (unsigned)g.hs && (unsigned)(s.x[j] + ox) < (unsigned)g.ws;
            pa[j] = (in ? A + (long long)(s.n[j] + d) * lda : zero) + col[j];
            real |= (in ? 1u : 0u) << j;
        }
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            long long off;
            if (GATHER) {
                const int sr = (s.n[j] >= 0) ? map_src(g.hs, g.ws, g.kw, g.stride, g.pad, g.dil, g.gather, s.n[j], s.y[j], s.x[j], tap) : -1;
                off = (sr >= 0) ? (long long)sr * lda : -1;
            } else {
                off = s.off[j];
            }
            pa[j] = (off >= 0 ? A + off : zero) + col[j];
            real |= (off >= 0 ? 1u : 0u) << j;
        }
    }
    if (ok) *ok = real;
    return tap;
}

// ---- the split-fp16 output epilogue ---------------------------------------------------------------------------------------
// Scalars of the epilogue: the output, what is added to it, what is reduced from it, and the tile (tm inside its part).
struct RowsOut {
    float* C; const float* bias; const float* res; double* colstats; float* colmax; float* amax_c;
    long long ld_res, bsc;
    int N, ldc, accumulate, rect, relu, tn, hd, wd;
    float alpha;
};

// BM_ x 128 tile of WR_ x 2 waves, each holding 64 x 64 results as 2 x 2 blocks of main (c) and mixed (m, x 2^11) products.
// EPI: the fused output epilogue of glf_gemm_nt_epilogue (residual with its own row stride, ReLU).
template <int BM_, int WR_, bool EPI>
__device__ __forceinline__ void rows_f16s_epilogue(const RowsOut& o, const RowTile& t, unsigned char* smem_s,
                                                   const f32x16& c00, const f32x16& c01, const f32x16& c10, const f32x16& c11,
                                                   const f32x16& m00, const f32x16& m01, const f32x16& m10, const f32x16& m11) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int pMe = t.rows, pN = o.N, p_ldc = o.ldc, p_accumulate = o.accumulate, p_rect = o.rect, tm = t.tm, tn = o.tn;
    const int r_y0 = t.y0, r_x0 = t.x0, r_h = t.h, r_w = t.w, g_hd = o.hd, g_wd = o.wd;
    const float p_alpha = o.alpha;
    float* __restrict__ C = o.C;
    const float* __restrict__ p_bias = o.bias;
    float cmax = 0.f;
    const bool p_colstats = o.colstats != nullptr;
    const float* __restrict__ p_res = EPI ? o.res : nullptr;
    const long long p_ldr = o.ld_res;
    const bool p_relu = EPI && o.relu != 0;
    const bool res_vec = (p_ldr % 4) == 0 && (reinterpret_cast<size_t>(p_res) % 16) == 0;
    // one result element -> C (plain / accumulate / region store, or the atomic of per-tap rectangles); cs / cq: the calling
    // lane's column sum and sum of squares over the elements it stores (colstats)
    auto put = [&](float a, int row, int col, float bv, double& cs, double& cq) __attribute__((always_inline)) {
        if (row >= pMe) return;
        long long orow = row;
        if (p_rect) {
            const int hw = r_h * r_w;
            const int n = row / hw, rem = row - n * hw;
            const int yy = rem / r_w;
            orow = ((long long)n * g_hd + r_y0 + yy) * g_wd + r_x0 + (rem - yy * r_w);
            if (p_rect == 1) { atomicAdd(C + orow * p_ldc + col, p_alpha * a); return; }
        }
        float* dst = C + orow * p_ldc + col;
        float v = p_alpha * a + bv;
        if constexpr (EPI) {
            if (p_res) v += p_res[orow * p_ldr + col];
            if (p_relu) v = fmaxf(v, 0.f);
        }
        if (p_accumulate) v += *dst;
        *dst = v;
        cmax = fmaxf(cmax, fabsf(v));
        if (p_colstats) { const double vd = (double)v; cs += vd; cq = fma(vd, vd, cq); }
    };
    // column statistics in double from the first product on: E[x^2] - E[x]^2 cancels badly when a channel's values are close
    // together (the ASPP pooled branch: N nearly equal frame averages), fp32 partial sums cost 4e-4 on its BatchNorm output
    // Fast epilogue (everything but the atomics of per-tap rectangles and unaligned outputs): every wave parks its 64 x 64
    // results in LDS (free once the main loop's last barrier is passed: 16 KB per wave) and stores them as whole 16-byte pieces
    // of rows -- 16 global_store_dwordx4 per lane instead of 64 one-dword stores.  The one-dword form took ~19 k cycles per
    // workgroup (in-kernel stamps, profiles/r02_stamps_*.txt): 13 % of a K = 2048 tile's time, 40 % of a K = 512 tile's,
    // with the matrix pipe idle (one 8-wave workgroup per CU: nothing else runs meanwhile).
    const bool wide_store = p_rect != 1 && (p_ldc % 4) == 0 && (pN % 4) == 0 && (reinterpret_cast<size_t>(C) % 16) == 0 &&
                            (o.bsc % 4) == 0;
    if (wide_store) {
        float* tile = reinterpret_cast<float*>(smem_s) + wave * (64 * 64);
        {
            const int col_l = lane & 31, row_l = 4 * (lane >> 5);
            auto park = [&](const f32x16& acc, int ti, int tj) __attribute__((always_inline)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) tile[(32 * ti + (r & 3) + 8 * (r >> 2) + row_l) * 64 + 32 * tj + col_l] = acc[r];
            };
            park(c00 + m00 * 0x1p-11f, 0, 0); park(c01 + m01 * 0x1p-11f, 0, 1);
            park(c10 + m10 * 0x1p-11f, 1, 0); park(c11 + m11 * 0x1p-11f, 1, 1);
        }
        __syncthreads();
        const int c4 = 4 * (lane & 15), r0 = lane >> 4;
        const int col = tn * BN + wn + c4;
        double cs[4] = {0.0, 0.0, 0.0, 0.0}, cq[4] = {0.0, 0.0, 0.0, 0.0};
        float cx[4] = {0.f, 0.f, 0.f, 0.f};          // column maxima of |C| (colmax)
        if (col < pN) {
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            if (p_bias) {
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = p_bias[col + j];
            }
            // region / rectangle stores: pixel coordinates of the lane's first row by division, of the next ones (4 rows on) by carrying
            int en = 0, ey = 0, ex = 0;
            if (p_rect) {
                const int row0 = tm * BM_ + wm + r0, hw = r_h * r_w;
                en = row0 / hw;
                const int rem = row0 - en * hw;
                ey = rem / r_w; ex = rem - ey * r_w;
            }
            if (p_accumulate && !p_rect && !p_colstats) {
                // C += result (the accumulate epilogue of glf_gemm): all 16 old values are requested before the first is
                // needed -- fetched inside the store loop, each of its 4-deep batches waited out a full memory round trip
                float4 prev[16];
                const int rowb = tm * BM_ + wm + r0;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    prev[i] = rowb + 4 * i < pMe ? *reinterpret_cast<const float4*>(C + (long long)(rowb + 4 * i) * p_ldc + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (rowb + 4 * i < pMe) {
                        const float4 a = *reinterpret_cast<const float4*>(tile + (r0 + 4 * i) * 64 + c4);
                        float4 v = make_float4(p_alpha * a.x + bv[0], p_alpha * a.y + bv[1], p_alpha * a.z + bv[2], p_alpha * a.w + bv[3]);
                        v.x += prev[i].x; v.y += prev[i].y; v.z += prev[i].z; v.w += prev[i].w;
                        *reinterpret_cast<float4*>(C + (long long)(rowb + 4 * i) * p_ldc + col) = v;
                        cmax = fmaxf(cmax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
                    }
                }
            } else
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const int rin = r0 + 4 * i;
                const int row = tm * BM_ + wm + rin;
                if (row >= pMe) break;
                long long orow = row;
                if (p_rect) {
                    orow = ((long long)en * g_hd + r_y0 + ey) * g_wd + r_x0 + ex;
                    ex += 4;
                    while (ex >= r_w) { ex -= r_w; ++ey; }
                    while (ey >= r_h) { ey -= r_h; ++en; }
                }
                const float4 a = *reinterpret_cast<const float4*>(tile + rin * 64 + c4);
                float* dst = C + orow * p_ldc + col;
                float v[4] = {p_alpha * a.x + bv[0], p_alpha * a.y + bv[1], p_alpha * a.z + bv[2], p_alpha * a.w + bv[3]};
                if constexpr (EPI) {
                    if (p_res) {
                        const float* rp = p_res + orow * p_ldr + col;
                        const float4 r = ld4(rp, 4, res_vec);
                        v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
                    }
                    if (p_relu) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                    }
                }
                if (p_accumulate) {
                    const float4 o4 = *reinterpret_cast<const float4*>(dst);
                    v[0] += o4.x; v[1] += o4.y; v[2] += o4.z; v[3] += o4.w;
                }
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                cmax = fmaxf(cmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
                if (p_colstats) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const double vd = (double)v[j]; cs[j] += vd; cq[j] = fma(vd, vd, cq[j]); cx[j] = fmaxf(cx[j], fabsf(v[j])); }
                }
            }
        }
        if (p_colstats) {
            // lanes l, l + 16, l + 32, l + 48 hold the four row groups of the same four columns; the wave rows of the workgroup
            // are then folded through LDS (each wave's own parking area is free once its stores are issued), so that ONE f64
            // atomic per column, statistic and WORKGROUP reaches memory.  Per wave it was M / 64 atomics on each of the N
            // addresses: 3 025 per address on a 193 600-row layer-1 conv output -- ~150 us of serialised atomics behind a 60 us
            // contraction (profiles/r03_colstats_atomics.txt).
            double* st = o.colstats;
            double* fold = reinterpret_cast<double*>(tile);              // [64 columns][3]: sum, sum of squares, maximum
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cs[j] += __shfl_xor(cs[j], 16, 64); cq[j] += __shfl_xor(cq[j], 16, 64);
                cs[j] += __shfl_xor(cs[j], 32, 64); cq[j] += __shfl_xor(cq[j], 32, 64);
                cx[j] = fmaxf(cx[j], __shfl_xor(cx[j], 16, 64)); cx[j] = fmaxf(cx[j], __shfl_xor(cx[j], 32, 64));
                if (lane < 16) { fold[3 * (c4 + j)] = cs[j]; fold[3 * (c4 + j) + 1] = cq[j]; fold[3 * (c4 + j) + 2] = (double)cx[j]; }
            }
            __syncthreads();
            if (wm == 0) {                                               // waves 0 / 1: the two column halves of the tile
                const int cl = lane;                                     // column within the wave's 64
                double s = 0.0, q = 0.0;
                float mx = 0.f;
#pragma unroll
                for (int w = 0; w < WR_; ++w) {
                    const double* f = reinterpret_cast<const double*>(reinterpret_cast<const float*>(smem_s) + (2 * w + (wave & 1)) * (64 * 64));
                    s += f[3 * cl]; q += f[3 * cl + 1]; mx = fmaxf(mx, (float)f[3 * cl + 2]);
                }
                const int cg = tn * BN + wn + cl;
                if (cg < pN) {
                    atomicAdd(st + cg, s); atomicAdd(st + pN + cg, q);
                    if (o.colmax && mx > 0.f) atomicMax(reinterpret_cast<unsigned*>(o.colmax + cg), __float_as_uint(mx));
                }
            }
        }
    } else {
        const int col_l = lane & 31, row_l = 4 * (lane >> 5);
        auto emit = [&](const f32x16& acc, int ti, int tj, double& cs, double& cq) {
            const int col = tn * BN + wn + 32 * tj + col_l;
            if (col >= pN) return;
            const float bv = p_bias ? p_bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) put(acc[r], tm * BM_ + wm + 32 * ti + (r & 3) + 8 * (r >> 2) + row_l, col, bv, cs, cq);
        };
        double cs0 = 0.0, cq0 = 0.0, cs1 = 0.0, cq1 = 0.0;
        emit(c00 + m00 * 0x1p-11f, 0, 0, cs0, cq0); emit(c01 + m01 * 0x1p-11f, 0, 1, cs1, cq1);
        emit(c10 + m10 * 0x1p-11f, 1, 0, cs0, cq0); emit(c11 + m11 * 0x1p-11f, 1, 1, cs1, cq1);
        if (o.colstats && p_rect != 1) {
            // lanes l and l + 32 hold the two row groups of the same column: fold them, then one f64 atomic per column
            // and statistic from this wave's 64 rows
            double* st = o.colstats;
            cs0 += __shfl_xor(cs0, 32, 64); cq0 += __shfl_xor(cq0, 32, 64);
            cs1 += __shfl_xor(cs1, 32, 64); cq1 += __shfl_xor(cq1, 32, 64);
            if (lane < 32) {
                const int col0 = tn * BN + wn + col_l, col1 = col0 + 32;
                if (col0 < pN) { atomicAdd(st + col0, cs0); atomicAdd(st + pN + col0, cq0); }
                if (col1 < pN) { atomicAdd(st + col1, cs1); atomicAdd(st + pN + col1, cq1); }
            }
        }
    }
    if (o.amax_c && p_rect != 1) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, off, 64));
        if (lane == 0 && cmax > *reinterpret_cast<volatile float*>(o.amax_c))      // thousands of waves, ONE address: only a wave that raises it
            atomicMax(reinterpret_cast<unsigned*>(o.amax_c), __float_as_uint(cmax));
    }
}

// ---- the plain output epilogue (exact-fp32 and bf16x6 kernels) ------------------------------------------------------------
// BM_ x 128 tile of waves holding 64 x 64 results as 2 x 2 blocks; a lane holds column (lane & 31), rows (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5) of a block.  One-dword stores of alpha * acc + bias (+ C); rect != 0 (per-tap rectangles): the tile's row -> its
// output pixel, and the taps meet in atomics.  Of RowsOut it reads C, bias, N, ldc, accumulate, rect, tn, hd, wd and alpha.
template <int BM_>
__device__ __forceinline__ void rows_plain_epilogue(const RowsOut& o, const RowTile& t, const f32x16& c00, const f32x16& c01,
                                                    const f32x16& c10, const f32x16& c11) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = t.tm * BM_ + (wave >> 1) * 64 + 4 * (lane >> 5), col0 = o.tn * BN + (wave & 1) * 64 + (lane & 31);
    const int pMe = t.rows, pN = o.N, p_ldc = o.ldc, p_accumulate = o.accumulate, p_rect = o.rect;
    const int r_y0 = t.y0, r_x0 = t.x0, r_h = t.h, r_w = t.w, g_hd = o.hd, g_wd = o.wd;
    const float p_alpha = o.alpha;
    float* __restrict__ C = o.C;
    const float* __restrict__ p_bias = o.bias;
    auto emit = [&](const f32x16& acc, int ti, int tj) {
        const int col = col0 + 32 * tj;
        if (col >= pN) return;
        const float bv = p_bias ? p_bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + 32 * ti + (r & 3) + 8 * (r >> 2);
            if (row >= pMe) continue;
            if (p_rect) {
                // unsigned divisions (nothing here is negative): the signed ones shared their magic numbers and signs with
                // the divisions of rows_init(), five scalars that then stayed live across the main loop and spilled SGPRs
                const unsigned hw = r_h * r_w;
                const int n = (unsigned)row / hw, rem = row - n * hw;
                const int yy = (unsigned)rem / (unsigned)r_w;
                const long long orow = ((long long)n * g_hd + r_y0 + yy) * g_wd + r_x0 + (rem - yy * r_w);
                atomicAdd(C + orow * p_ldc + col, p_alpha * acc[r]);
            } else {
                float* dst = C + (long long)row * p_ldc + col;
                float v = p_alpha * acc[r] + bv;
                if (p_accumulate) v += *dst;
                *dst = v;
            }
        }
    };
    emit(c00, 0, 0); emit(c01, 0, 1); emit(c10, 1, 0); emit(c11, 1, 1);
}

}  // namespace

// Contour distances of a prediction against its target, per (frame, class channel, direction): the numbers behind Hausdorff,
// percentile Hausdorff and average symmetric surface distance (no reference counterpart: main.py:800-815 counts overlap only).
//   contour of a mask  = its on pixels with a 4-neighbour that is off or outside the image (M ^ binary_erosion(M), cross element)
//   direction 0        = every contour pixel of the prediction -> nearest contour pixel of the target, squared, an exact integer
//   direction 1        = target -> prediction
// One workgroup owns one (frame, channel, direction).  Everything lives in LDS and is an integer until the final square roots:
//   1. both masks become bitmaps by wave ballots (coalesced reads, the predicates of mask_predicates.h), the contours follow by word
//      logic on the bitmaps (a pixel's four neighbours are two shifts and two rows);
//   2. separable exact distance transform: a ROW pass writes, for a strip of columns, g[y][x] = distance along row y to the nearest
//      destination-contour pixel (16 bits, kNone = none in this row; found by clz / ctz over at most kRowWords words), a COLUMN pass
//      takes min over y' of (y - y')^2 + g[y'][x]^2 for the source-contour pixels, walking outwards from y and stopping once
//      (y - y')^2 alone reaches the best so far: at most h steps per pixel whatever the masks are;
//   3. order statistics without a sort: the column pass fills a histogram of d2 >> kFineBits, one wave locates the bins of the two
//      ranks, a second column pass fills the two fine histograms of the low bits inside those bins.
// The sum of distances is taken in float64 in a fixed order (per thread over its pixels, a shuffle tree, then the waves in turn):
// bitwise reproducible.  Counts and the maximum use integer LDS atomics.
#include "glf_common.h"
#include "mask_predicates.h"
#include <cstdint>

namespace {

constexpr int kMaxDim = GLF_CONTOUR_MAX_DIM;        // h, w <= 256: d2 <= 2 * 255^2 < 2^17
constexpr int kRowWords = kMaxDim / 32;             // 32-bit words of one bitmap row (fixed stride)
constexpr int kMapWords = kMaxDim * kRowWords;      // one bitmap: 8 KB
constexpr int kGElems = 16384;                      // 16-bit row distances of one column strip: 32 KB (112 x 112 in one strip)
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kFineBits = 7;                        // fine histogram: the low 7 bits of d2
constexpr int kCoarseBins = 1024;                   // d2 >> 7 <= 130050 >> 7 = 1016
constexpr int kFineBins = 1 << kFineBits;
constexpr unsigned kNone = 0xffffu;
static_assert(2 * (kMaxDim - 1) * (kMaxDim - 1) < (kCoarseBins << kFineBits), "coarse histogram too short");
static_assert(kMaxDim * (kGElems / kMaxDim) <= kGElems && kGElems / kMaxDim >= 1, "strip");
static_assert(2 * kMapWords * 4 <= kGElems * 2, "the on-bitmaps borrow the strip buffer");

struct Shared {
    union {
        uint32_t on[2][kMapWords];                  // step 1 only
        uint16_t g[kGElems];                        // step 2
    } u;
    uint32_t contour[2][kMapWords];                 // [0] prediction, [1] target
    uint32_t coarse[kCoarseBins];
    uint32_t fine[2][kFineBins];
    double wave_sum[kWaves];
    int count[2];
    int max_d2;
    int bin[2], rest[2], low[2];        // per rank: coarse bin, rank inside it, low bits of the value
};

// wave 0, all 64 lanes: the bin holding ascending rank r of a histogram of 64 * per_lane bins, and r's rank inside that bin.
// True in the one lane that found it.
__device__ __forceinline__ bool find_rank(const uint32_t* hist, int per_lane, int r, int& bin, int& rest) {
    const int lane = threadIdx.x & 63;
    int mine = 0;
    for (int i = 0; i < per_lane; ++i) mine += (int)hist[lane * per_lane + i];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    int cum = incl - mine;
    if (!(cum <= r && r < incl)) return false;
    for (int i = 0; i < per_lane; ++i) {
        const int n = (int)hist[lane * per_lane + i];
        if (r < cum + n) { bin = lane * per_lane + i; rest = r - cum; break; }
        cum += n;
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void contour_distances_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                     long long* __restrict__ stats, double* __restrict__ sums, int h, int w,
                                                                     int pct) {
    __shared__ Shared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long item = blockIdx.x;              // (frame * c + channel) * 2 + direction
    const int dir = (int)(item & 1);
    const long long plane = (item >> 1) * (long long)h * w;
    const float* x = logits + plane;
    const float* t = target + plane;
    const int nw = (w + 31) >> 5, units = (w + 63) >> 6;

    for (int i = tid; i < kCoarseBins; i += kThreads) sh.coarse[i] = 0;
    for (int i = tid; i < 2 * kFineBins; i += kThreads) sh.fine[0][i] = 0;
    if (tid == 0) { sh.count[0] = sh.count[1] = 0; sh.max_d2 = 0; sh.bin[0] = sh.bin[1] = 0; sh.rest[0] = sh.rest[1] = 0; }

    // 1a. the masks as bitmaps: one wave ballot per 64 pixels of a row
    for (int u = wave; u < h * units; u += kWaves) {
        const int y = u / units, k = u - y * units, px = k * 64 + lane;
        bool p = false, q = false;
        if (px < w) { p = glf::channel_on(x[y * w + px]); q = glf::target_on(t[y * w + px]); }
        const unsigned long long bp = __ballot(p), bq = __ballot(q);
        if (lane < 2) {
            sh.u.on[0][y * kRowWords + 2 * k + lane] = (uint32_t)(bp >> (32 * lane));
            sh.u.on[1][y * kRowWords + 2 * k + lane] = (uint32_t)(bq >> (32 * lane));
        }
    }
    __syncthreads();
    // 1b. contours: on, and not all four neighbours on (bits past w and rows outside the image read as off)
    for (int i = tid; i < 2 * h * nw; i += kThreads) {
        const int m = i / (h * nw), r = i - m * (h * nw), y = r / nw, k = r - y * nw;
        const uint32_t* row = sh.u.on[m] + y * kRowWords;
        const uint32_t c = row[k];
        const uint32_t left = (c << 1) | (k > 0 ? row[k - 1] >> 31 : 0u);
        const uint32_t right = (c >> 1) | (k + 1 < nw ? row[k + 1] << 31 : 0u);
        const uint32_t up = y > 0 ? row[k - kRowWords] : 0u;
        const uint32_t down = y + 1 < h ? row[k + kRowWords] : 0u;
        const uint32_t edge = c & ~(left & right & up & down);
        sh.contour[m][y * kRowWords + k] = edge;
        if (edge) atomicAdd(&sh.count[m], __popc(edge));
    }
    __syncthreads();                                // the on-bitmaps are dead from here: u.g takes their place

    const int src = dir, dst = dir ^ 1;
    const int count = sh.count[src];
    if (count == 0 || sh.count[dst] == 0) {         // uniform over the workgroup
        if (tid == 0) {
            stats[item * 4 + 0] = count; stats[item * 4 + 1] = -1; stats[item * 4 + 2] = -1; stats[item * 4 + 3] = -1;
            sums[item] = 0.0;
        }
        return;
    }
    const int tq = pct * (count - 1);
    const int lo = tq / 100, hi = lo + (tq % 100 != 0);
    const uint32_t* sc = sh.contour[src];
    const uint32_t* dc = sh.contour[dst];
    const int sw = min(w, kGElems / h), strips = (w + sw - 1) / sw;

    double sum = 0.0;
    int best_max = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int s = 0; s < strips; ++s) {
            const int x0 = s * sw, cw = min(sw, w - x0);
            if (pass == 0 || strips > 1) {          // a plane of one strip keeps its row distances for the second pass
                __syncthreads();                    // the column pass of the strip before has finished reading g
                for (int i = tid; i < h * cw; i += kThreads) {
                    const int y = i / cw, xl = i - y * cw, px = x0 + xl, wi = px >> 5, b = px & 31;
                    const uint32_t* row = dc + y * kRowWords;
                    unsigned d = kNone;
                    uint32_t m = row[wi] & (0xffffffffu >> (31 - b));
                    int k = wi;
                    while (m == 0 && k > 0) m = row[--k];
                    if (m) d = (unsigned)(px - (k * 32 + 31 - __clz((int)m)));
                    m = row[wi] & (0xffffffffu << b);
                    k = wi;
                    while (m == 0 && k + 1 < nw) m = row[++k];
                    if (m) d = min(d, (unsigned)(k * 32 + __ffs((int)m) - 1 - px));
                    sh.u.g[y * cw + xl] = (uint16_t)d;
                }
                __syncthreads();
            }
            for (int i = tid; i < h * cw; i += kThreads) {
                const int y = i / cw, xl = i - y * cw, px = x0 + xl;
                if (!((sc[y * kRowWords + (px >> 5)] >> (px & 31)) & 1u)) continue;
                const uint16_t* col = sh.u.g + xl;
                int best = 0x7fffffff;
                for (int dy = 0; dy < h; ++dy) {
                    const int dy2 = dy * dy;
                    if (dy2 >= best) break;
                    if (y - dy >= 0) {
                        const int gv = col[(y - dy) * cw];
                        if (gv != (int)kNone) best = min(best, dy2 + gv * gv);
                    }
                    if (y + dy < h) {
                        const int gv = col[(y + dy) * cw];
                        if (gv != (int)kNone) best = min(best, dy2 + gv * gv);
                    }
                }
                if (pass == 0) {
                    sum += sqrt((double)best);
                    best_max = max(best_max, best);
                    atomicAdd(&sh.coarse[best >> kFineBits], 1u);
                } else {
                    if ((best >> kFineBits) == sh.bin[0]) atomicAdd(&sh.fine[0][best & (kFineBins - 1)], 1u);
                    if ((best >> kFineBits) == sh.bin[1]) atomicAdd(&sh.fine[1][best & (kFineBins - 1)], 1u);
                }
            }
        }
        __syncthreads();
        if (wave == 0) {                            // the two ranks: their coarse bins after the first pass, their low bits after the second
            for (int k = 0; k < 2; ++k) {
                int bin = 0, rest = 0;
                const bool found = pass == 0 ? find_rank(sh.coarse, kCoarseBins / 64, k == 0 ? lo : hi, bin, rest)
                                             : find_rank(sh.fine[k], kFineBins / 64, sh.rest[k], bin, rest);
                if (found) {
                    if (pass == 0) { sh.bin[k] = bin; sh.rest[k] = rest; }
                    else sh.low[k] = bin;
                }
            }
        }
        __syncthreads();
    }

    // the sum in a fixed order: shuffle tree inside a wave, then the waves in turn
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    atomicMax(&sh.max_d2, best_max);
    if (lane == 0) sh.wave_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < kWaves; ++i) total += sh.wave_sum[i];
        stats[item * 4 + 0] = count;
        stats[item * 4 + 1] = sh.max_d2;
        stats[item * 4 + 2] = ((long long)sh.bin[0] << kFineBits) | sh.low[0];
        stats[item * 4 + 3] = ((long long)sh.bin[1] << kFineBits) | sh.low[1];
        sums[item] = total;
    }
}

}  // namespace

extern "C" int glf_contour_distances(const float* logits, const float* target, int64_t* stats, double* sums, int n, int c, int h, int w,
                                     int pct, glf_stream_t s) {
    GLF_REQUIRE(logits && target && stats && sums, GLF_ERR_NULL, "contour_distances: null argument");
    GLF_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0, GLF_ERR_BAD_SHAPE, "contour_distances: n, c, h, w must be > 0 (got %d, %d, %d, %d)", n, c, h, w);
    GLF_REQUIRE(pct >= 0 && pct <= 100, GLF_ERR_BAD_SHAPE, "contour_distances: pct = %d is outside 0..100", pct);
    GLF_REQUIRE(2ll * n * c <= 0x7fffffffll, GLF_ERR_BAD_SHAPE, "contour_distances: %d x %d planes are more than one call takes", n, c);
    GLF_REQUIRE(h <= kMaxDim && w <= kMaxDim, GLF_ERR_UNSUPPORTED, "contour_distances: planes of %d x %d, at most %d x %d", h, w, kMaxDim, kMaxDim);
    hipLaunchKernelGGL(contour_distances_kernel, dim3((unsigned)(2ll * n * c)), dim3(kThreads), 0, glf::S(s), logits, target,
                       reinterpret_cast<long long*>(stats), sums, h, w, pct);
    return glf::check_launch("contour_distances");
}

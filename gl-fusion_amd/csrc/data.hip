// the GPU side of the reference's data path and evaluation harness.
//   * glf_prepare_frames: the per-sample transform chain of datasets/loader.py:460-498 (AddChannel -> Resized(144, 144,
//     mode='nearest') -> Center/RandSpatialCrop(112, 112) -> EnsureType) fused with the label handling of
//     loader.py:298-330, 358-414 (class id -> one of 5 part channels per view, images / 255), reading a raw
//     [H0][W0][T] volume and writing the model's layout directly: frames [T][1][112][112], masks [T][5][112][112].
//   * glf_overlap_counts_nchw: tp / fp / fn / tn of sigmoid(logit) > 0.5 against the mask PER CLASS CHANNEL
//     (main.py:537-543 slices the accumulated predictions per part), int64, one pass over [N][C][HW].
//   * glf_render_labels / glf_restore_labels: the visual mode (main.py:546-648).  Label map = argmax over [0.5, on_0 .. on_{C-1}]
//     (main.py:606-612), coloured through a palette (main.py:623-634) with an optional integer blend over the grey frame, and the
//     way back from the 112 x 112 crop to the source volume's geometry (the inverse of glf_prepare_frames), [H0][W0][T] uint8.
//   * glf_frame_label_sums / glf_prepare_batch: the training loaders (main.py:116-145, 185-218).  Per-frame sums of a resident label
//     volume (input_select's masks.sum(dim=(0, 1)), loader.py:429-458), and the frames of MANY (volume, frame window, crop) sources in
//     one call, from uint8 or float32 volumes, by glf_prepare_frames' arithmetic (one shared per-pixel body).
// HBM-bound byte / index work: one thread per output pixel, coalesced along x.
#include "glf_common.h"
#include "mask_predicates.h"
#include <cstdint>

namespace {

using glf::channel_on;                              // mask_predicates.h: the one binarisation of a logit
using glf::target_on;

// nearest-neighbour source index exactly as ATen's upsample_nearest (legacy 'nearest'): floor(dst * (in / out)) in
// fp32, clamped to in - 1
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

// One output pixel of the data path, the body glf_prepare_frames and glf_prepare_batch share: output pixel (y, x) of a frame reads
// voxel (ys, xs, t) of a [H0][W0][T] volume (T fastest) stored as TI / TL (float or uint8_t: a byte converts to float / int exactly,
// so both storages give the same bits).  o_img: this pixel of the frame's image plane or null; o_mask: this pixel of the frame's
// channel 0 plane or null, the 5 channel planes `plane` floats apart.
template <typename TI, typename TL>
__device__ __forceinline__ void prepare_pixel(const TI* __restrict__ img, const TL* __restrict__ lab, float* __restrict__ o_img,
                                              float* __restrict__ o_mask, long long plane, int y, int x, int t, int H0, int W0, int T,
                                              float sy, float sx, int oy, int ox, int4 chan, float img_div) {
    const int ys = nearest_src(y + oy, sy, H0), xs = nearest_src(x + ox, sx, W0);
    const long long src = ((long long)ys * W0 + xs) * T + t;
    if (o_img) *o_img = (float)img[src] / img_div;              // a true division: bit-identical to `images / 255.0` (loader.py:327)
    if (o_mask) {
        const int cls = (int)lab[src];                          // 0 = background, 1..4 = parts of this view
        const int ch = cls == 1 ? chan.x : cls == 2 ? chan.y : cls == 3 ? chan.z : cls == 4 ? chan.w : -1;
#pragma unroll
        for (int c = 0; c < 5; ++c) o_mask[(long long)c * plane] = (c == ch) ? 1.f : 0.f;
    }
}

// img / lab: [H0][W0][T] (T fastest, the NIfTI volume order nibabel hands over); out_img [T][1][oh][ow]; out_mask [T][5][oh][ow]
__global__ __launch_bounds__(256) void prepare_frames_kernel(const float* __restrict__ img, const float* __restrict__ lab,
                                                             float* __restrict__ out_img, float* __restrict__ out_mask, int H0, int W0, int T,
                                                             int rs, int oh, int ow, int oy, int ox, int4 chan_lo, int chan_4, float img_div) {
    const long long total = (long long)T * oh * ow, plane = (long long)oh * ow;
    const float sy = (float)H0 / (float)rs, sx = (float)W0 / (float)rs;
    (void)chan_4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % ow);
        const int y = (int)((i / ow) % oh);
        const int t = (int)(i / plane);
        prepare_pixel(img, lab, out_img ? out_img + i : nullptr, out_mask ? out_mask + (long long)t * 5 * plane + (long long)y * ow + x : nullptr,
                      plane, y, x, t, H0, W0, T, sy, sx, oy, ox, chan_lo, img_div);
    }
}

// ---- glf_prepare_batch: many sources, one launch per chunk -------------------------------------------------------------
constexpr int kBatchChunk = 32;                     // sources per launch: 32 x 64 B + 16 B of scalars = 2 064 B of kernel arguments
struct BatchSrc {                                   // what the kernel needs of a glf_frame_src, 64 bytes
    const void* img; const void* lab;               // img null: the source's frames are zeros (a patient without this view)
    int H0, W0, T, t0;
    int rs, oy, ox;
    float img_div;
    int first;                                      // first output frame of this source WITHIN the chunk
    int8_t chan[4];
    uint8_t img_u8, lab_u8, pad[2];
    int pad2;
};
static_assert(sizeof(BatchSrc) == 64, "BatchSrc is the by-value kernel argument: keep it 64 bytes");
struct BatchChunk { BatchSrc src[kBatchChunk]; };

// out_img [frames][1][oh][ow], out_mask [frames][5][oh][ow] (or null), both already advanced to the chunk's first frame.  A block
// belongs to ONE output frame (bpf blocks per frame), so the walk that finds the frame's source is uniform over the block and reads
// kernel arguments only: at most kBatchChunk compares, never more than this chunk.
__global__ __launch_bounds__(256) void prepare_batch_kernel(BatchChunk chunk, int n, float* __restrict__ out_img,
                                                            float* __restrict__ out_mask, int oh, int ow, int bpf) {
    const int f = blockIdx.x / bpf;
    const int p = (blockIdx.x - f * bpf) * 256 + threadIdx.x;
    const int plane = oh * ow;
    if (p >= plane) return;
    int k = 0;
    while (k + 1 < n && chunk.src[k + 1].first <= f) ++k;
    const BatchSrc& s = chunk.src[k];
    const int y = p / ow, x = p - y * ow;
    float* o_img = out_img + (long long)f * plane + p;
    float* o_mask = out_mask ? out_mask + (long long)f * 5 * plane + p : nullptr;
    if (o_mask && (s.img == nullptr || s.lab == nullptr)) {     // no view, or an image-only source in a batch with masks
#pragma unroll
        for (int c = 0; c < 5; ++c) o_mask[(long long)c * plane] = 0.f;
        o_mask = nullptr;
    }
    if (s.img == nullptr) {
        *o_img = 0.f;
        return;
    }
    const int t = s.t0 + (f - s.first);
    const float sy = (float)s.H0 / (float)s.rs, sx = (float)s.W0 / (float)s.rs;
    const int4 chan = make_int4(s.chan[0], s.chan[1], s.chan[2], s.chan[3]);
    const float* lf = static_cast<const float*>(s.lab); const uint8_t* lb = static_cast<const uint8_t*>(s.lab);
    if (s.img_u8) {
        const uint8_t* im = static_cast<const uint8_t*>(s.img);
        if (s.lab_u8) prepare_pixel(im, lb, o_img, o_mask, plane, y, x, t, s.H0, s.W0, s.T, sy, sx, s.oy, s.ox, chan, s.img_div);
        else          prepare_pixel(im, lf, o_img, o_mask, plane, y, x, t, s.H0, s.W0, s.T, sy, sx, s.oy, s.ox, chan, s.img_div);
    } else {
        const float* im = static_cast<const float*>(s.img);
        if (s.lab_u8) prepare_pixel(im, lb, o_img, o_mask, plane, y, x, t, s.H0, s.W0, s.T, sy, sx, s.oy, s.ox, chan, s.img_div);
        else          prepare_pixel(im, lf, o_img, o_mask, plane, y, x, t, s.H0, s.W0, s.T, sy, sx, s.oy, s.ox, chan, s.img_div);
    }
}

// ---- glf_frame_label_sums: column sums of the [H0 * W0][T] matrix a label volume is ---------------------------------------
// A block pass covers kSumRows(T) whole pixels x one tile of up to 256 frames: thread k reads frame c0 + k % tw of pixel
// r + k / tw, so with T <= 256 a pass is ONE contiguous run of rows * T elements, and beyond that 256 consecutive frames of a
// pixel.  The frame of a thread never changes, so it sums in a register (exact: int64 of (int)value, the conversion the mask
// kernel makes); the block folds its rows in LDS and adds ONE value per frame to the output.
template <typename TL>
__global__ __launch_bounds__(256) void frame_label_sums_kernel(const TL* __restrict__ lab, unsigned long long* __restrict__ sums,
                                                               long long pixels, int T, int tw, int rows) {
    __shared__ long long part[256];
    const int k = threadIdx.x, r_off = k / tw, c = blockIdx.y * tw + (k - r_off * tw);
    const bool active = r_off < rows && c < T;
    long long acc = 0;
    if (active) {
        const long long step = (long long)gridDim.x * rows;
        long long r = (long long)blockIdx.x * rows + r_off;
        for (; r + 3 * step < pixels; r += 4 * step) {          // four independent loads in flight
            const TL a = lab[r * T + c], b = lab[(r + step) * T + c], d = lab[(r + 2 * step) * T + c], e = lab[(r + 3 * step) * T + c];
            acc += (long long)(int)a + (long long)(int)b + (long long)(int)d + (long long)(int)e;
        }
        for (; r < pixels; r += step) acc += (long long)(int)lab[r * T + c];
    }
    part[k] = active ? acc : 0;
    __syncthreads();
    if (r_off == 0 && c < T) {
        long long total = 0;
        for (int j = 0; j < rows; ++j) total += part[j * tw + k];
        atomicAdd(sums + c, (unsigned long long)total);
    }
}

// counts[c][4] += (tp, fp, fn, tn) of channel c; x, t: [N][C][hw]
__global__ __launch_bounds__(256) void overlap_nchw_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                           unsigned long long* __restrict__ counts, int N, int C, long long hw) {
    const int c = blockIdx.y;
    unsigned long long tp = 0, fp = 0, fn = 0, tn = 0;
    const long long per = (long long)N * hw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / hw, p = i - n * hw;
        const long long o = (n * C + c) * hw + p;
        const bool pr = channel_on(x[o]);                     // main.py:250, 385
        const bool gt = target_on(t[o]);
        tp += pr && gt; fp += pr && !gt; fn += !pr && gt; tn += !pr && !gt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tp += __shfl_xor(tp, o, 64); fp += __shfl_xor(fp, o, 64); fn += __shfl_xor(fn, o, 64); tn += __shfl_xor(tn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* k = counts + 4 * c;
        atomicAdd(k + 0, tp); atomicAdd(k + 1, fp); atomicAdd(k + 2, fn); atomicAdd(k + 3, tn);
    }
}

constexpr int kMaxClasses = 8;                      // channels of a rendered / restored prediction (the model's C is 5)
struct Palette { uint32_t rgba[kMaxClasses + 1]; };  // r | g << 8 | b << 16 | a << 24 per label: the byte order of the store
struct ClassTable { uint8_t cls[kMaxClasses]; };     // channel -> class id, 0 = not shown by this view

// (alpha * colour + (255 - alpha) * grey + 127) / 255 on each of r, g, b; the alpha byte becomes 255
__device__ __forceinline__ uint32_t blend_rgba(uint32_t colour, int grey, int alpha) {
    uint32_t out = 0xff000000u;
#pragma unroll
    for (int k = 0; k < 24; k += 8) out |= (uint32_t)((alpha * (int)((colour >> k) & 0xffu) + (255 - alpha) * grey + 127) / 255) << k;
    return out;
}

// logits [N][C][hw]; frames [N][hw] or null; labels [N][hw] or null; rgba [N][hw] packed pixels or null.  One thread per pixel:
// the C plane reads, the byte store and the 32-bit store are all coalesced along x
__global__ __launch_bounds__(256) void render_labels_kernel(const float* __restrict__ logits, const float* __restrict__ frames,
                                                            uint8_t* __restrict__ labels, uint32_t* __restrict__ rgba, long long total,
                                                            int C, long long hw, Palette pal, int alpha) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / hw, p = i - n * hw;
        const float* x = logits + n * C * hw + p;
        int label = 0;
        for (int c = C - 1; c >= 0; --c)
            if (channel_on(x[c * hw])) label = c + 1;         // the first maximum of [0.5, on_0, ...]: the lowest channel that is on
        if (labels) labels[i] = (uint8_t)label;
        if (rgba) {
            uint32_t px = pal.rgba[label];
            if (frames) {
                // individually rounded (no fma): the grey level is the same on any host that restates it
                const float g = __fadd_rn(__fmul_rn(frames[i], 255.0f), 0.5f);
                const int grey = g >= 1.0f ? (g >= 255.0f ? 255 : (int)g) : 0;                  // NaN -> 0
                px = label ? blend_rgba(px, grey, alpha) : (0xff000000u | (uint32_t)grey * 0x010101u);
            }
            rgba[i] = px;
        }
    }
}

constexpr int kRestoreX = 64, kRestoreT = 64;       // one tile: 64 source pixels of one row x 64 frames

// logits [T][C][oh][ow] -> vol [H0][W0][T].  The reads run along x, the store along t, so a tile goes through LDS: a wave
// classifies 64 consecutive x0 of one frame (coalesced plane reads, up to the repeats / strides of the nearest mapping), then
// the block writes the tile's bytes in address order -- per x0 a run of up to 64 frames, the whole tile one run when T <= 64.
__global__ __launch_bounds__(256) void restore_labels_kernel(const float* __restrict__ logits, uint8_t* __restrict__ vol, int T, int C,
                                                             int oh, int ow, int H0, int W0, int rs, int oy, int ox, ClassTable tab,
                                                             long long tiles, int xtiles, int ttiles) {
    __shared__ uint8_t tile[kRestoreX][kRestoreT + 1];
    const float sy = (float)rs / (float)H0, sx = (float)rs / (float)W0;
    const long long plane = (long long)oh * ow;
    for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {
        const int tt = (int)(b % ttiles), xt = (int)((b / ttiles) % xtiles), y0 = (int)(b / ((long long)ttiles * xtiles));
        const int t0 = tt * kRestoreT, x00 = xt * kRestoreX;
        const int nt = T - t0 < kRestoreT ? T - t0 : kRestoreT, nx = W0 - x00 < kRestoreX ? W0 - x00 : kRestoreX;
        const int xl = threadIdx.x & (kRestoreX - 1);
        const int y = nearest_src(y0, sy, rs) - oy;
        const int x = xl < nx ? nearest_src(x00 + xl, sx, rs) - ox : -1;
        const bool inside = y >= 0 && y < oh && x >= 0 && x < ow;
        for (int tl = threadIdx.x / kRestoreX; tl < nt; tl += 256 / kRestoreX) {
            int cls = 0;
            if (inside) {
                const float* src = logits + (long long)(t0 + tl) * C * plane + (long long)y * ow + x;
                float best = 0.f;
                for (int c = 0; c < C; ++c) {
                    if (tab.cls[c] == 0) continue;               // uniform over the grid: a channel this view does not show is not read
                    const float v = src[c * plane];
                    if (channel_on(v) && (cls == 0 || v > best)) { cls = tab.cls[c]; best = v; }
                }
            }
            tile[xl][tl] = (uint8_t)cls;
        }
        __syncthreads();
        uint8_t* dst = vol + ((long long)y0 * W0 + x00) * T + t0;
        for (int j = threadIdx.x; j < nx * nt; j += 256) {
            const int xj = j / nt, tj = j - xj * nt;
            dst[(long long)xj * T + tj] = tile[xj][tj];
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int glf_prepare_frames(const float* img, const float* lab, float* out_img, float* out_mask, int H0, int W0, int T,
                                  int resize, int out_h, int out_w, int off_y, int off_x, const int* class_to_channel, float img_div,
                                  glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE((img && out_img) || (lab && out_mask), GLF_ERR_NULL, "prepare_frames: nothing to do (image and label both missing)");
    GLF_REQUIRE((img != nullptr) == (out_img != nullptr) && (lab != nullptr) == (out_mask != nullptr), GLF_ERR_NULL,
                "prepare_frames: an input needs its output and vice versa");
    GLF_REQUIRE(H0 > 0 && W0 > 0 && T > 0 && resize > 0 && out_h > 0 && out_w > 0, GLF_ERR_BAD_SHAPE, "prepare_frames: sizes must be > 0");
    GLF_REQUIRE(img_div != 0.f, GLF_ERR_BAD_SHAPE, "prepare_frames: img_div must not be 0");
    GLF_REQUIRE(off_y >= 0 && off_x >= 0 && off_y + out_h <= resize && off_x + out_w <= resize, GLF_ERR_BAD_SHAPE,
                "prepare_frames: crop window [%d+%d, %d+%d] leaves the %d x %d resized image", off_y, out_h, off_x, out_w, resize, resize);
    int4 lo = make_int4(-1, -1, -1, -1);
    if (lab) {
        GLF_REQUIRE(class_to_channel != nullptr, GLF_ERR_NULL, "prepare_frames: class_to_channel (4 ints: channel of class 1..4, -1 = none) missing");
        for (int i = 0; i < 4; ++i)
            GLF_REQUIRE(class_to_channel[i] >= -1 && class_to_channel[i] < 5, GLF_ERR_BAD_SHAPE, "prepare_frames: channel index out of range");
        lo = make_int4(class_to_channel[0], class_to_channel[1], class_to_channel[2], class_to_channel[3]);
    }
    const long long total = (long long)T * out_h * out_w;
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(prepare_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, glf::S(s), img, lab, out_img, out_mask, H0, W0, T, resize,
                       out_h, out_w, off_y, off_x, lo, 0, img_div);
    return glf::check_launch("prepare_frames");
}

extern "C" int glf_overlap_counts_nchw(const float* logits, const float* target, int64_t* counts, int n, int c, int64_t hw, glf_stream_t s) {
    if (int rc = glf::ensure_init()) return rc;
    GLF_REQUIRE(logits && target && counts, GLF_ERR_NULL, "overlap_counts_nchw: null argument");
    GLF_REQUIRE(n > 0 && c > 0 && c <= 65535 && hw > 0, GLF_ERR_BAD_SHAPE, "overlap_counts_nchw: bad extents");
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)c * 4 * sizeof(int64_t), glf::S(s));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "overlap_counts_nchw: memset: %s", hipGetErrorString(e));
    long long blocks = ((long long)n * hw + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(overlap_nchw_kernel, dim3((unsigned)blocks, c), dim3(256), 0, glf::S(s), logits, target,
                       reinterpret_cast<unsigned long long*>(counts), n, c, (long long)hw);
    return glf::check_launch("overlap_counts_nchw");
}

extern "C" int glf_render_labels(const float* logits, const float* frames, uint8_t* labels, uint8_t* rgba, int n, int c, int h, int w,
                                 const uint8_t* palette, int alpha, glf_stream_t s) {
    GLF_REQUIRE(logits != nullptr, GLF_ERR_NULL, "render_labels: null logits");
    GLF_REQUIRE(labels != nullptr || rgba != nullptr, GLF_ERR_NULL, "render_labels: nothing to do (labels and rgba both null)");
    GLF_REQUIRE(rgba == nullptr || palette != nullptr, GLF_ERR_NULL, "render_labels: null palette ((c + 1) x 4 host bytes)");
    GLF_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0, GLF_ERR_BAD_SHAPE, "render_labels: n, c, h, w must be > 0 (got %d, %d, %d, %d)", n, c, h, w);
    GLF_REQUIRE(c <= kMaxClasses, GLF_ERR_BAD_SHAPE, "render_labels: c = %d channels, at most %d", c, kMaxClasses);
    GLF_REQUIRE(alpha >= 0 && alpha <= 255, GLF_ERR_BAD_SHAPE, "render_labels: alpha = %d is outside 0..255", alpha);
    GLF_REQUIRE((reinterpret_cast<uintptr_t>(rgba) & 3u) == 0, GLF_ERR_BAD_SHAPE, "render_labels: rgba must be 4-byte aligned");
    Palette pal = {};
    if (rgba)
        for (int k = 0; k <= c; ++k)
            pal.rgba[k] = (uint32_t)palette[4 * k] | (uint32_t)palette[4 * k + 1] << 8 | (uint32_t)palette[4 * k + 2] << 16 |
                          (uint32_t)palette[4 * k + 3] << 24;
    if (int rc = glf::ensure_init()) return rc;
    const long long hw = (long long)h * w, total = hw * n;
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(render_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, glf::S(s), logits, frames, labels,
                       reinterpret_cast<uint32_t*>(rgba), total, c, hw, pal, alpha);
    return glf::check_launch("render_labels");
}

extern "C" int glf_restore_labels(const float* logits, uint8_t* volume, int T, int c, int out_h, int out_w, int H0, int W0, int resize,
                                  int off_y, int off_x, const int* channel_to_class, glf_stream_t s) {
    GLF_REQUIRE(logits != nullptr, GLF_ERR_NULL, "restore_labels: null logits");
    GLF_REQUIRE(volume != nullptr, GLF_ERR_NULL, "restore_labels: null volume");
    GLF_REQUIRE(channel_to_class != nullptr, GLF_ERR_NULL, "restore_labels: null channel_to_class (c host ints: class of each channel, 0 = none)");
    GLF_REQUIRE(T > 0 && c > 0 && out_h > 0 && out_w > 0 && H0 > 0 && W0 > 0 && resize > 0, GLF_ERR_BAD_SHAPE,
                "restore_labels: sizes must be > 0");
    GLF_REQUIRE(c <= kMaxClasses, GLF_ERR_BAD_SHAPE, "restore_labels: c = %d channels, at most %d", c, kMaxClasses);
    ClassTable tab = {};
    for (int k = 0; k < c; ++k) {
        GLF_REQUIRE(channel_to_class[k] >= 0 && channel_to_class[k] <= 255, GLF_ERR_BAD_SHAPE,
                    "restore_labels: channel_to_class[%d] = %d is outside 0..255", k, channel_to_class[k]);
        tab.cls[k] = (uint8_t)channel_to_class[k];
    }
    GLF_REQUIRE(off_y >= 0 && off_x >= 0 && off_y <= resize - out_h && off_x <= resize - out_w, GLF_ERR_BAD_SHAPE,
                "restore_labels: crop window [%d+%d, %d+%d] leaves the %d x %d resized image", off_y, out_h, off_x, out_w, resize, resize);
    if (int rc = glf::ensure_init()) return rc;
    const int xtiles = (W0 + kRestoreX - 1) / kRestoreX, ttiles = (T + kRestoreT - 1) / kRestoreT;
    const long long tiles = (long long)H0 * xtiles * ttiles;
    const long long blocks = tiles < 8192 ? tiles : 8192;
    hipLaunchKernelGGL(restore_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, glf::S(s), logits, volume, T, c, out_h, out_w, H0, W0,
                       resize, off_y, off_x, tab, tiles, xtiles, ttiles);
    return glf::check_launch("restore_labels");
}

extern "C" int glf_frame_label_sums(const void* lab, int dtype, int H0, int W0, int T, int64_t* sums, glf_stream_t s) {
    GLF_REQUIRE(lab != nullptr && sums != nullptr, GLF_ERR_NULL, "frame_label_sums: null argument");
    GLF_REQUIRE(H0 > 0 && W0 > 0 && T > 0, GLF_ERR_BAD_SHAPE, "frame_label_sums: H0, W0, T must be > 0 (got %d, %d, %d)", H0, W0, T);
    GLF_REQUIRE(dtype == GLF_SRC_F32 || dtype == GLF_SRC_U8, GLF_ERR_UNSUPPORTED, "frame_label_sums: dtype %d (0 = float32, 1 = uint8)", dtype);
    const int tw = T < 256 ? T : 256, rows = 256 / tw, ttiles = (T + tw - 1) / tw;
    GLF_REQUIRE(ttiles <= 65535, GLF_ERR_BAD_SHAPE, "frame_label_sums: T = %d frames, at most %d", T, 65535 * 256);
    if (int rc = glf::ensure_init()) return rc;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)T * sizeof(int64_t), glf::S(s));
    if (e != hipSuccess) return glf::fail(GLF_ERR_LAUNCH, "frame_label_sums: memset: %s", hipGetErrorString(e));
    const long long pixels = (long long)H0 * W0, passes = (pixels + rows - 1) / rows;
    long long bx = (passes + 7) / 8;                 // 8 passes or more per block: one atomic per frame pays for >= 2 048 loads
    const long long cap = 2048 / ttiles > 0 ? 2048 / ttiles : 1;
    if (bx > cap) bx = cap;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
    if (dtype == GLF_SRC_U8)
        hipLaunchKernelGGL(frame_label_sums_kernel<uint8_t>, dim3((unsigned)bx, ttiles), dim3(256), 0, glf::S(s),
                           static_cast<const uint8_t*>(lab), out, pixels, T, tw, rows);
    else
        hipLaunchKernelGGL(frame_label_sums_kernel<float>, dim3((unsigned)bx, ttiles), dim3(256), 0, glf::S(s),
                           static_cast<const float*>(lab), out, pixels, T, tw, rows);
    return glf::check_launch("frame_label_sums");
}

extern "C" int glf_prepare_batch(const glf_frame_src* srcs, int n, float* out_img, float* out_mask, int out_h, int out_w, glf_stream_t s) {
    GLF_REQUIRE(srcs != nullptr, GLF_ERR_NULL, "prepare_batch: null source descriptors");
    GLF_REQUIRE(out_img != nullptr, GLF_ERR_NULL, "prepare_batch: null out_img");
    GLF_REQUIRE(n > 0, GLF_ERR_BAD_SHAPE, "prepare_batch: n = %d sources, must be > 0", n);
    GLF_REQUIRE(out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1ll << 30), GLF_ERR_BAD_SHAPE, "prepare_batch: bad output extents %d x %d",
                out_h, out_w);
    long long frames = 0;
    for (int i = 0; i < n; ++i) {
        const glf_frame_src& d = srcs[i];
        GLF_REQUIRE(d.nt > 0, GLF_ERR_BAD_SHAPE, "prepare_batch: source %d: nt = %d frames, must be > 0", i, d.nt);
        frames += d.nt;
        if (d.img == nullptr) continue;                      // zeros: nothing else of the descriptor is read
        GLF_REQUIRE(d.img_dtype == GLF_SRC_F32 || d.img_dtype == GLF_SRC_U8, GLF_ERR_UNSUPPORTED,
                    "prepare_batch: source %d: image dtype %d (0 = float32, 1 = uint8)", i, d.img_dtype);
        GLF_REQUIRE(d.H0 > 0 && d.W0 > 0 && d.T > 0 && d.resize > 0, GLF_ERR_BAD_SHAPE, "prepare_batch: source %d: sizes must be > 0", i);
        GLF_REQUIRE(d.t0 >= 0 && (long long)d.t0 + d.nt <= d.T, GLF_ERR_BAD_SHAPE, "prepare_batch: source %d: frames [%d, %d + %d) leave the %d of the volume",
                    i, d.t0, d.t0, d.nt, d.T);
        GLF_REQUIRE(d.img_div != 0.f, GLF_ERR_BAD_SHAPE, "prepare_batch: source %d: img_div must not be 0", i);
        GLF_REQUIRE(d.off_y >= 0 && d.off_x >= 0 && d.off_y <= d.resize - out_h && d.off_x <= d.resize - out_w, GLF_ERR_BAD_SHAPE,
                    "prepare_batch: source %d: crop window [%d+%d, %d+%d] leaves the %d x %d resized image", i, d.off_y, out_h, d.off_x, out_w,
                    d.resize, d.resize);
        if (d.lab != nullptr) {
            GLF_REQUIRE(d.lab_dtype == GLF_SRC_F32 || d.lab_dtype == GLF_SRC_U8, GLF_ERR_UNSUPPORTED,
                        "prepare_batch: source %d: label dtype %d (0 = float32, 1 = uint8)", i, d.lab_dtype);
            for (int k = 0; k < 4; ++k)
                GLF_REQUIRE(d.class_to_channel[k] >= -1 && d.class_to_channel[k] < 5, GLF_ERR_BAD_SHAPE,
                            "prepare_batch: source %d: channel index out of range", i);
        }
    }
    const int plane = out_h * out_w, bpf = (plane + 255) / 256;
    GLF_REQUIRE(frames * bpf <= 0x7fffffffll, GLF_ERR_BAD_SHAPE, "prepare_batch: %lld output frames are more than one call takes", frames);
    if (int rc = glf::ensure_init()) return rc;
    // the descriptors travel as kernel arguments, kBatchChunk per launch: no device table, no copy, nothing to wait for
    long long done = 0;                                      // output frames of the chunks already launched
    for (int i0 = 0; i0 < n; i0 += kBatchChunk) {
        const int m = n - i0 < kBatchChunk ? n - i0 : kBatchChunk;
        BatchChunk chunk = {};
        int first = 0;
        for (int k = 0; k < m; ++k) {
            const glf_frame_src& d = srcs[i0 + k];
            BatchSrc& b = chunk.src[k];
            b.img = d.img; b.lab = d.img ? d.lab : nullptr;
            b.H0 = d.H0; b.W0 = d.W0; b.T = d.T; b.t0 = d.t0; b.rs = d.resize; b.oy = d.off_y; b.ox = d.off_x; b.img_div = d.img_div;
            b.first = first;
            for (int c = 0; c < 4; ++c) b.chan[c] = (int8_t)(b.lab ? d.class_to_channel[c] : -1);
            b.img_u8 = d.img_dtype == GLF_SRC_U8; b.lab_u8 = d.lab_dtype == GLF_SRC_U8;
            first += d.nt;
        }
        hipLaunchKernelGGL(prepare_batch_kernel, dim3((unsigned)((long long)first * bpf)), dim3(256), 0, glf::S(s), chunk, m,
                           out_img + done * plane, out_mask ? out_mask + done * 5 * plane : nullptr, out_h, out_w, bpf);
        if (int rc = glf::check_launch("prepare_batch")) return rc;
        done += first;
    }
    return GLF_OK;
}

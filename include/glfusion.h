/*
 * glfusion.h -- C ABI of libglfusion_hip.so: the MI355X (gfx950 / CDNA4) engine for the
 * GL-Fusion forward/backward hot path.
 *
 * The reference (xmed-lab/GL-Fusion) is pure PyTorch: it has no FFI of its own.  Each entry
 * point below replaces the ATen operator(s) the reference launches implicitly at the cited
 * call sites (file:line relative to GLfusion/ in the reference tree); the Python host side
 * (gl-fusion_amd/) binds them with ctypes from torch.autograd.Function wrappers.
 *
 * Conventions
 *   - plain pointers and sizes only; every tensor and workspace buffer is CALLER-OWNED (inputs,
 *     outputs, workspace, saved-for-backward) and no caller pointer is kept after return.  The
 *     library owns exactly three kinds of small device allocations, made lazily and kept until the
 *     process exits: a 1 MiB page of zeros per device (the split-fp16 kernels load conv-padding
 *     and tile-overhang rows from it), a 16 KiB ring of floats per (device, stream) that is
 *     used only when a precision-3 contraction is called with amax_a / amax_b == NULL (the
 *     library then measures the operand maxima itself, on that stream), and a 2 KiB plan table per
 *     distinct (device, geometry, segment list) of a segmented glf_gemm_nt launch (nseg > 0).
 *   - every function only ENQUEUES work on `stream` and returns; no host synchronisation (one
 *     exception: the FIRST segmented launch of a plan copies its table with a blocking hipMemcpy
 *     and therefore refuses to run on a capturing stream; later launches of that plan do neither).
 *   - return 0 on success, a negative glf_status otherwise; text via glf_last_error()
 *     (thread-local).  No exception crosses this boundary.
 *   - activations are channels-last: a tensor [N,H,W,C] is the row-major matrix
 *     [rows = N*H*W][C]; `ld*` arguments are row strides in elements.
 *   - arithmetic type: fp32 operands and results; contractions run on v_mfma_f32_32x32x2_f32 or on the
 *     split 16-bit MFMA schemes selected per call / per process (see glf_set_precision).
 */
#ifndef GLFUSION_H
#define GLFUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* glf_stream_t; /* hipStream_t */

typedef enum {
    GLF_OK = 0,
    GLF_ERR_BAD_SHAPE = -1,
    GLF_ERR_UNSUPPORTED = -2,
    GLF_ERR_WORKSPACE = -3,
    GLF_ERR_LAUNCH = -4,
    GLF_ERR_NULL = -5
} glf_status;

/* Element type tags of the typed ("_t") and 16-bit-storage ("glf_s16_") entry points. */
typedef enum { GLF_DT_F32 = 0, GLF_DT_BF16 = 1 } glf_dtype;

const char* glf_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int glf_abi_version(void);
/* Queries the current device once (CU count) and raises the dynamic-LDS limit of the MFMA
 * kernels.  Optional: every entry point calls it lazily. */
int glf_init(void);
/* DEFAULT contraction precision of glf_gemm_nt / glf_gemm_tn, used by calls whose glf_gemm_params.precision is 0:
 *   0 = exact fp32 on v_mfma_f32_32x32x2_f32 (default);
 *   1 = split-bf16 "bf16x6": each fp32 operand is split into three bf16 pieces and six
 *       v_mfma_f32_32x32x16_bf16 reproduce the fp32 product to 2^-23 (fp32 accumulate) -- fp32-equivalent
 *       results at 2.67x the fp32-MFMA roof.  Calls that miss the aligned fast path (and glf_gemm_nn) stay
 *       on the exact kernels;
 *   2 = split-fp16 "f16x3": each operand is scaled by a power of two taken from its max magnitude
 *       (glf_gemm_params.amax_a / amax_b) and split into two fp16 pieces; three
 *       v_mfma_f32_32x32x16_f16 reproduce the fp32 product to 2^-22 relative to the operand maxima
 *       (fp32 accumulate) at 5.3x the fp32-MFMA roof.  Elements more than 2^27 below their operand's
 *       maximum keep an absolute (not relative) error bound, 2^-49 of that maximum.  Same fast-path rule;
 *   3 = fp16 "f16": the same kernels keeping only the high fp16 half of each scaled operand -- ONE
 *       v_mfma_f32_32x32x16_f16 per product, fp32 accumulate, 11-bit operands (relative error ~2^-11 per
 *       element): the 16-bit-arithmetic configuration (BASELINE.json configs[2]), NOT fp32-equivalent. */
int glf_set_precision(int mode);
int glf_get_precision(void);
/* sizeof(glf_gemm_params) as compiled into the library (binding self-check). */
size_t glf_sizeof_gemm_params(void);

/* ---------------------------------------------------------------------------------------
 * Contractions (implicit GEMM, NHWC, im2col-free; v_mfma_f32_32x32x2_f32; 128x128x32 tiles
 * staged through LDS).  One parameter block serves conv forward / dgrad / wgrad and the
 * plain (batched) GEMMs of the fusion block.
 *
 *   C[b][m][n] (+)= alpha * sum_{tap} sum_{k} A_tap[b][m][k] * B_tap[b][k][n]  (+ bias[n])
 *
 * gather: 0 = A rows are taken as they are (plain GEMM / 1x1 stride-1 conv)
 *         1 = forward conv mapping : GEMM row m = output pixel (n,y,x) on the hd x wd grid reads
 *             source pixel (y*stride - pad + ky*dil, x*stride - pad + kx*dil) on the hs x ws grid
 *         2 = transposed mapping (dgrad): row m = input pixel (n,y,x) on hd x wd reads the
 *             output-gradient pixel ((y + pad - ky*dil)/stride, ...) on hs x ws when divisible
 * Out-of-range taps read zeros; taps invalid for a whole 128-row tile are skipped (or see `rect`).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t M, N, K;            /* per-tap GEMM extents (see each entry point)                   */
    int32_t lda, ldb, ldc;      /* row strides (elements)                                        */
    int32_t taps;               /* kh*kw (1 for plain GEMM)                                      */
    uint32_t tap_mask;          /* bit t set = tap t can be valid for some row (host-computed)   */
    int64_t tap_stride_b;       /* elements between consecutive taps of the weight operand       */
    int32_t gather;             /* 0 / 1 / 2 as above                                            */
    int32_t n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil;
    int32_t batch;              /* >= 1                                                          */
    int64_t batch_stride_a, batch_stride_b, batch_stride_c;
    float alpha;                /* scale applied to the accumulator                              */
    int32_t accumulate;         /* 1: C += result (fwd/dgrad: read-modify-write; wgrad: atomics) */
    int32_t split;              /* wgrad/TN only: number of reduction slices (>=1); >1 requires  */
                                /* C zero-filled (or holding the value to accumulate onto).  A   */
                                /* slice is ceil(K / split) rows (rounded up to 32) of EVERY      */
                                /* tap's reduction: in rect mode a tap whose rectangle is short   */
                                /* uses fewer slices, so all workgroups get reductions of equal   */
                                /* length whatever the rectangles' sizes.                        */
    int32_t rect;               /* 1: tap-parallel rectangle mode (stride-1 convs whose taps fall */
                                /* mostly into the padding, i.e. ASPP): each tap runs as its own  */
                                /* GEMM over exactly its in-range rectangle of pixels; nt/nn sum  */
                                /* the taps with float atomics into a ZERO-FILLED C (no bias); tn */
                                /* shortens each tap's reduction to its rectangle.                */
                                /* 2 (glf_gemm_nt, precision 2 only): region mode for 3x3 stride-1 */
                                /* convs with pad == dil on equal maps: the output map is cut into */
                                /* <= 9 rectangles inside each of which the set of in-range taps   */
                                /* is constant; each is a GEMM over exactly its taps, every output */
                                /* element is stored ONCE (no atomics, no zero fill, bias and      */
                                /* accumulate allowed, no padding work)                            */
    const float* amax_a;        /* precision 2 only: DEVICE scalars holding an upper bound of max|A| */
    const float* amax_b;        /* and max|B| over the elements the call reads (glf_amax, or the     */
                                /* kernel that produced the operand).  NULL: the library measures    */
                                /* the operand itself first (one extra read of it).                  */
    float* amax_c;              /* precision 2 only, may be NULL: device float that receives                 */
                                /* max(*amax_c, max|C|) over the elements this call stores -- the amax of    */
                                /* the NEXT contraction's operand for free.  Ignored (left untouched) by     */
                                /* calls that sum partial results with atomics (rect mode, split > 1).       */
    double* colstats;           /* glf_gemm_nt, precision 2 only, may be NULL: DEVICE doubles [2][N], zero-filled by   */
                                /* the caller; the epilogue adds the column sums of the stored C and of C^2 --   */
                                /* the BatchNorm batch statistics of a conv output without a pass over it        */
                                /* (finish with glf_bn_stats_from_sums).  A call that cannot honour it (exact    */
                                /* kernels, rect = 1) fails with GLF_ERR_UNSUPPORTED instead of ignoring it.     */
    float* workspace;           /* glf_gemm_tn with split > 1, may be NULL: caller-owned scratch of at least            */
    int64_t workspace_bytes;    /* glf_gemm_tn_workspace_bytes(p) bytes.  With it the reduction slices store partial     */
                                /* sums there and a second kernel adds them in a fixed order: no float atomics, C need   */
                                /* not be zero-filled, results are bitwise reproducible.  Without it (NULL) the slices   */
                                /* meet in float atomics and C must be zero-filled (or hold the value to add to).        */
    int32_t a_presplit;         /* precision 3 / 4 only: 1 = the A (B) pointer is not fp32 data but its packed pre-split   */
    int32_t b_presplit;         /* image written by glf_split_f16_packed with the SAME amax_a (amax_b): same byte size,     */
                                /* strides and addressing as the fp32 operand, every 16-byte group of four elements holding */
                                /* {h0..h3, l0..l3} (fp16).  The kernels then skip the split in their staging path: an       */
                                /* operand read by many tiles / launches (activations across column tiles, weights across   */
                                /* row tiles, a conv input again in its weight gradient) is split once.                     */
    int32_t precision;          /* contraction precision of THIS call: 0 = the process default (glf_set_precision), */
                                /* 1 = exact fp32, 2 = split-bf16 x6, 3 = split-fp16 x3, 4 = fp16 x1 (= 1 + the modes of */
                                /* glf_set_precision).  Two models with different precisions can share a process.   */
    float* colmax;              /* with colstats, may be NULL: DEVICE floats [N], zero-filled by the caller; the epilogue   */
                                /* raises colmax[n] to the largest |C[m][n]| it stores -- with the batch statistics it bounds */
                                /* the BatchNorm OUTPUT's maximum before that output exists (glf_bn_apply_from_sums         */
                                /* packed_y: the activation written once, as the packed image its consumer reads)           */
    int32_t c_dtype;            /* glf_s16_gemm_nt / _tn only: element type of C (GLF_DT_F32 or GLF_DT_BF16); the fp32-storage    */
    int32_t reserved0;          /* entry points ignore it (C is fp32).  reserved0: padding, leave 0.                              */
    int32_t c_oihw;             /* glf_gemm_tn only: 1 = C is the PARAMETER-SHAPED gradient [M][N][taps] (torch's OIHW), dense:   */
                                /* ldc / tap_stride_b are not used.  The slices always go through the workspace (required, also   */
                                /* with split == 1: glf_gemm_tn_workspace_bytes sizes it) and the second stage stores every tap   */
                                /* of an output element side by side: kept taps = the sum of their slices (the bits the tap-major */
                                /* store + glf_tap_major_to_oihw give), taps outside tap_mask = 0 -- no zero fill by the caller.  */
                                /* An EMPTY tap_mask is allowed here: no contraction runs, only the store (zeros and the foreign  */
                                /* tap).  accumulate adds to what C holds.  Needs batch == 1, N % 4 == 0, a 16-byte aligned C and */
                                /* taps <= GLF_TN_OIHW_MAX_TAPS; anything else is GLF_ERR_UNSUPPORTED.                            */
    int32_t foreign_tap;        /* with c_oihw and foreign_src: the tap (not in tap_mask) whose [M][N] values are copied from     */
    const float* foreign_src;   /* foreign_src (row stride foreign_ld floats, % 4 == 0, 16-byte aligned) -- a result another      */
    int64_t foreign_ld;         /* contraction produced (the ASPP centre taps, stacked).  NULL: no such tap.                      */
    int32_t nseg;               /* glf_gemm_nt only, segmented region mode (0 = off): a plain NT contraction (gather 0, taps 1,   */
    int32_t seg_kx;             /* rect 0) over the n_img x hd x wd pixel rows of A, extended by nseg <= GLF_SEG_MAX extra        */
    int32_t* seg;               /* segments.  seg is a HOST array [nseg][3] = (oy, ox, acol), only read; segment s adds to the    */
                                /* output row of pixel (n, y, x)   sum_{j < seg_kx} A[(n, y+oy, x+ox)][acol + j] * B[c][K + s*seg_kx + j] */
                                /* wherever (y+oy, x+ox) lies inside the map (ldb >= K + nseg*seg_kx, acol + seg_kx <= lda).  The  */
                                /* map is cut into the rectangles of glf_gemm_nt_seg_plan, inside each of which the set of        */
                                /* in-range segments is constant: a row tile walks the K columns, then its rectangle's segments   */
                                /* by ascending s, and every output element is stored ONCE (no accumulate, no zero fill, no       */
                                /* atomics; bitwise reproducible; amax_c reported).  Precision 3 / 4 with BOTH operands pre-split, */
                                /* K and seg_kx multiples of 32, acol a multiple of 4, batch 1; anything else is                  */
                                /* GLF_ERR_UNSUPPORTED.  The plan's small device table is made on the first launch of a given     */
                                /* (geometry, segment list) and kept: later launches allocate and copy nothing (graph-capturable). */
                                /* colstats / colmax are honoured: every stored element counts once, the overhang rows of a ragged */
                                /* rectangle tile do not.  Rows past a ragged tile's end read a zero page of 2^18 floats for the   */
                                /* whole chain: K plus the most segments any rectangle walks, times seg_kx, has to fit into it     */
                                /* (GLF_ERR_UNSUPPORTED otherwise).  Segments that belong to a group of output columns:            */
                                /* glf_gemm_nt_seg_cols.                                                                          */
} glf_gemm_params;
#define GLF_TN_OIHW_MAX_TAPS 9
#define GLF_SEG_MAX 28
#define GLF_SEG_MAX_REGIONS 49
#define GLF_SEG_ROW_TILE 256

/* Host-only plan of a segmented-region glf_gemm_nt launch (glf_gemm_params.nseg): the rectangles of the h x w map in DISPATCH
 * order (descending number of in-range segments).  seg = [nseg][3] (oy, ox, acol; acol is not used here).  Per axis the band
 * edges are the union of {min(d, H-d), max(d, H-d)} (clamped to [0, H]) over the distinct |offset| values d > 0 present; more
 * than 7 bands on an axis is GLF_ERR_UNSUPPORTED.  regions receives [*n_regions][6] = (y0, y1, x0, x1, segment mask, row tiles)
 * with room for GLF_SEG_MAX_REGIONS entries; a row tile is GLF_SEG_ROW_TILE of the n_img * (y1-y0) * (x1-x0) rows of its
 * rectangle (the last one ragged).  *row_tiles = their sum: the launch's grid is that times ceil(N / 128). */
int glf_gemm_nt_seg_plan(int32_t n_img, int32_t h, int32_t w, int32_t nseg, const int32_t* seg, int32_t* regions,
                         int32_t* n_regions, int64_t* row_tiles);

/* glf_gemm_nt in segmented region mode (p->nseg >= 1, no bias) whose segments belong to GROUPS OF OUTPUT COLUMNS -- the forward of
 * an ASPP head: the K columns are the 1x1 branch and every centre tap, a segment is an off-centre tap of ONE branch and adds to that
 * branch's columns only.  seg_cols is a HOST array [nseg][2] = (first column, column count) of whole 128-column tiles inside
 * [0, N) with N % 128 == 0 and at most 64 column tiles.  seg_boff, a HOST array [nseg] or NULL, is the offset in floats (>= 0,
 * % 4 == 0) from the start of the B row of one of the segment's columns to the segment's slice of seg_kx floats; NULL means
 * K + s * seg_kx.  With offsets the B image need not be [N][K + nseg * seg_kx]: each group keeps its segments behind its own rows,
 * or in row blocks of their own (ops.aspp_fwd_weights: offset = (block row - first column) * ldb); the caller vouches for the
 * buffer behind every offset.  A workgroup walks `rectangle mask & column-tile mask`; chains then differ across the column tiles of
 * one row tile, and the workgroups are dispatched longest chain first from a list kept with the plan's device table
 * (glf_gemm_nt_seg_plan_cols).  Everything else -- operands, precisions, amax_c, colstats / colmax, the zero-page bound, the first
 * launch of a plan allocating its table -- as documented for glf_gemm_params.nseg. */
int glf_gemm_nt_seg_cols(const float* A, const float* B, float* C, const glf_gemm_params* p, const int32_t* seg_cols,
                         const int64_t* seg_boff, glf_stream_t stream);
/* Host-only plan of a glf_gemm_nt_seg_cols launch: glf_gemm_nt_seg_plan's results, plus col_masks[ceil(N / 128)] = the segments
 * that contribute to each column tile, plus (order != NULL, room for order_cap >= *row_tiles * ceil(N / 128) entries) the dispatch
 * list [workgroups][3] = (rectangle, row tile inside it, column tile) in blockIdx order: non-increasing chain length
 * popcount(rectangle mask & column-tile mask) from one run of 16 entries to the next (inside a run, neighbouring pairs are dealt
 * to the eight XCDs that blockIdx % 8 selects, the heaviest pair to the XCD given the least work so far; a workgroup weighs
 * 1 + its chain length here, K / 32 + chain * seg_kx / 32 in the launcher: the same list when seg_kx == K).  A glf_gemm_nt launch
 * with nseg > 0 and no column groups is dispatched from the same kind of list (full column-tile masks, groups of four) when it
 * has at most 64 column tiles; results do not depend on the dispatch order. */
int glf_gemm_nt_seg_plan_cols(int32_t n_img, int32_t h, int32_t w, int32_t nseg, const int32_t* seg, const int32_t* seg_cols, int32_t N,
                              int32_t* regions, int32_t* n_regions, int64_t* row_tiles, uint32_t* col_masks, int32_t* order,
                              int64_t order_cap);

/* *out = max |x| over the [rows, cols] view with row stride ld (elements); out is a device float. */
int glf_amax(const float* x, int64_t rows, int cols, int64_t ld, float* out, glf_stream_t stream);
/* out = packed pre-split image of x [rows][cols] (row strides ld / ldo in floats; cols, ld, ldo % 4 == 0, 16-byte
 * aligned): every float4 {x0..x3} -> {h0..h3, l0..l3} fp16 with x * s = h + 2^-11 l, s the power of two the precision-3
 * kernels derive from *amax (a device float >= max|x|).  For glf_gemm_params.a_presplit / b_presplit. */
int glf_split_f16_packed(const float* x, int64_t rows, int cols, int64_t ld, const float* amax, float* out, int64_t ldo,
                         glf_stream_t stream);
/* glf_split_f16_packed that ALSO writes colsum[cols] = sum_r x[r][c] -- the bias gradient of a layer whose output gradient is
 * packed for its contractions anyway, read off the same pass instead of a second one over the tensor.  The image is
 * bit-identical to glf_split_f16_packed's.  The sums go through fixed-order two-stage partials (fp32 over at most 64 rows, then
 * double; no atomics: equal inputs give equal bits).  workspace: glf_bn_workspace(rows, cols) doubles.  out must not be x. */
int glf_split_f16_packed_colsum(const float* x, int rows, int cols, int64_t ld, const float* amax, float* out, int64_t ldo,
                                float* colsum, double* workspace, glf_stream_t stream);

/* A[m][k] (k contiguous, rows gathered per `gather`), B_tap[n][k] (k contiguous: torch's
 * [Cout][Cin] weight layout per tap), C[m][n].  Replaces F.conv2d / nn.Conv3d(1x1x1) forward:
 * models/_utils.py:192 (stem is separate), torchvision Bottleneck convs (ours.py:1797-1800),
 * deeplabv3.py:104-165, ours.py:866,878-879,908.  bias may be NULL. */
int glf_gemm_nt(const float* A, const float* B, const float* bias, float* C,
                const glf_gemm_params* p, glf_stream_t stream);
/* A[m][k] (rows gathered), B_tap[k][n] (n contiguous), C[m][n].  Conv dgrad (A = dY, B = the
 * same [tap][Cout][Cin] weights, gather = 2) and y = theta @ M of the re-associated dot
 * attention (ours.py:881-902). */
int glf_gemm_nn(const float* A, const float* B, const float* bias, float* C,
                const glf_gemm_params* p, glf_stream_t stream);
/* Reduction over ROWS: C_tap[m][n] (+)= alpha * sum_r A[r][m] * B[src(r,tap)][n], r < K.
 * Here p->K is the number of rows r, p->M / p->N the two channel extents, `gather` applies
 * to B's rows.  Conv wgrad (A = dY [rows][Cout], B = X [rows][Cin], C = dW [tap][Cout][Cin])
 * and M = phi^T g of the dot attention.  Output taps are p->tap_stride_b apart in C. */
int glf_gemm_tn(const float* A, const float* B, float* C,
                const glf_gemm_params* p, glf_stream_t stream);
/* bytes of glf_gemm_params.workspace the two-stage reduction of this call needs (0 when p->split <= 1). */
size_t glf_gemm_tn_workspace_bytes(const glf_gemm_params* p);

/* glf_gemm_nt with a fused output epilogue (split-fp16 kernels, precision 3 / 4 only):
 *     C[m][n] = act( alpha * sum_k A[m][k] B[n][k] + shift[n] (+ residual[m][n]) ),   act = identity or max(., 0)
 * -- a convolution followed by an eval-mode BatchNorm whose scale has been folded into the weights (glf_fold_bn), the
 * block's residual add and its ReLU, with the output written once.  residual rows are indexed like C's (row stride
 * ld_res floats).  p->amax_c receives the maximum of the value actually STORED (after the epilogue).  Works wherever
 * the kernels store every output element exactly once: plain and gathered contractions, rect = 0 or 2.  Arguments are
 * checked before any HIP runtime call: GLF_ERR_NULL (a null pointer wins over every other error), GLF_ERR_BAD_SHAPE
 * (extents, relu not 0 / 1, ld_res < N), GLF_ERR_UNSUPPORTED for what the epilogue cannot honour and therefore never
 * ignores: an effective precision other than 3 / 4, rect = 1, accumulate, split > 1, colstats / colmax, batch > 1,
 * operands off the aligned fast path (K % 32, 16-byte alignment, strides % 4). */
typedef struct {
    const float* shift;         /* [N], required                                                                 */
    const float* residual;      /* optional [M][ld_res]                                                          */
    int64_t ld_res;             /* row stride of residual in floats (>= N)                                       */
    int32_t relu;               /* 0 identity, 1 ReLU                                                            */
    int32_t reserved0;          /* leave 0                                                                       */
} glf_gemm_epilogue;
int glf_gemm_nt_epilogue(const float* A, const float* B, float* C, const glf_gemm_params* p, const glf_gemm_epilogue* e,
                         glf_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 16-bit storage ("S16": BASELINE.json configs[2] and [4] -- bf16 activations, saved tensors and
 * activation gradients in HBM, fp32 master weights, fp32 accumulate).  Same contraction
 * semantics and parameter block as glf_gemm_nt / glf_gemm_tn with these differences:
 *   - A and B hold bf16 (row / batch / tap strides multiples of 8 elements, 16-byte aligned);
 *     C holds p->c_dtype (activations: GLF_DT_BF16, weight gradients: GLF_DT_F32);
 *   - ONE v_mfma_f32_32x32x16_bf16 per product; operands go global -> LDS by LDS-DMA
 *     (global_load_lds_dwordx4), padding / overhang rows come from the library's zero page;
 *   - K % 64 == 0 (NT); M % 8 == 0 and N % 8 == 0 (TN); rect = 0 or 2 (NT region mode); no
 *     amax / presplit / precision fields (ignored); colstats is honoured by glf_s16_gemm_nt
 *     (sums of the fp32 results before they are rounded to bf16);
 *   - glf_s16_gemm_tn with split > 1 REQUIRES the workspace (glf_s16_gemm_tn_workspace_bytes):
 *     slices store partial slabs, a second kernel adds them in slice order (no atomics).
 * Replaces (reference call sites): the same convolutions / projections as glf_gemm_*, i.e.
 * torchvision Bottleneck convs (ours.py:1797-1800), ASPP / head convs (deeplabv3.py:102-166),
 * TPAVI theta/phi/g/W_z and the attention matmuls (ours.py:866-908), run under the bf16
 * configuration the reference itself never had.
 * ------------------------------------------------------------------------------------- */
int glf_s16_gemm_nt(const void* A, const void* B, const float* bias, void* C, const glf_gemm_params* p, glf_stream_t stream);
int glf_s16_gemm_tn(const void* A, const void* B, void* C, const glf_gemm_params* p, glf_stream_t stream);
size_t glf_s16_gemm_tn_workspace_bytes(const glf_gemm_params* p);
/* glf_s16_gemm_nt with a fused output epilogue (folded-BatchNorm inference under 16-bit storage):
 *     C[m][n] = bf16( act( alpha * acc[m][n] + shift[n] (+ float(residual[m][n])) ) ),   act = identity or max(., 0)
 * All arithmetic is fp32 on the fp32 accumulator; the value is rounded to bf16 ONCE, after the epilogue.  residual (bf16) rows
 * are indexed like C's rows (region mode included), ld_res elements apart.  Every output element is stored exactly once
 * (plain and forward-gathered contractions, rect = 0 or 2).  Checked before any HIP runtime call, in this order:
 * GLF_ERR_NULL (A, B, C, p, e, e->shift); GLF_ERR_BAD_SHAPE (the extents glf_s16_gemm_nt checks, ldc < N, relu not 0 / 1,
 * ld_res < N with a residual); GLF_ERR_UNSUPPORTED -- never ignored -- for c_dtype != GLF_DT_BF16, accumulate, colstats,
 * split > 1, batch != 1, gather == 2, a residual that is not 16-byte aligned or whose ld_res % 8 != 0, K % 64 != 0 and a
 * rect other than 0 / 2. */
typedef struct {
    const float* shift;         /* [N], required                                                                 */
    const void* residual;       /* optional bf16 [M][ld_res]                                                     */
    int64_t ld_res;             /* row stride of residual in elements (>= N, % 8 == 0)                           */
    int32_t relu;               /* 0 identity, 1 ReLU                                                            */
    int32_t reserved;           /* leave 0                                                                       */
} glf_s16_gemm_epilogue;
int glf_s16_gemm_nt_epilogue(const void* A, const void* B, void* C, const glf_gemm_params* p, const glf_s16_gemm_epilogue* e,
                             glf_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Convolution entry points (F.conv2d forward / backward: models/_utils.py:192 excluded -- glf_stem7x7_* --,
 * torchvision Bottleneck convs at ours.py:1797-1800, deeplabv3.py:104-165).  x [n][h][w][cin] and y / dy
 * [n][ho][wo][cout] channels-last, weights tap-major [kh*kw][cout][cin] (glf_oihw_to_tap_major), groups = 1, zero
 * padding.  They sit on top of glf_gemm_* and embed its launch policy (host-side tap mask of the taps that can touch
 * the map at all, per-tap rectangle / region modes when most tap work would be padding -- the ASPP rates on a 28 x 28
 * map --, split-K of the weight gradient, zero fills), so a C caller needs nothing but this block.
 * glf_conv2d_plan reports what a pass will do (GEMM extents, kept taps, mode, slices, workspace) without launching.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, h, w, cin, cout, kh, kw, stride, pad, dil;
    int32_t precision;          /* as glf_gemm_params.precision (0 = process default)                            */
    const float* amax_x;        /* precision 3 / 4, optional: device scalars bounding max|x|, max|w|, max|dy|     */
    const float* amax_w;        /* (NULL: measured by the library)                                               */
    const float* amax_dy;
    float* amax_out;            /* optional: receives max|output| of fwd / dgrad where the kernel stores directly */
    double* colstats;           /* fwd only, optional: [2][cout] zero-filled doubles, += column sums of y, y^2    */
} glf_conv_params;
typedef struct {
    int32_t ho, wo;             /* output map                                                                     */
    int32_t M, N, K;            /* per-tap GEMM extents of the pass                                               */
    int32_t taps, kept_taps;    /* kh*kw and how many of them can be in range                                     */
    uint32_t tap_mask;
    int32_t plain;              /* 1: a 1x1 stride-1 conv = plain GEMM                                            */
    int32_t rect;               /* 0 dense, 1 per-tap rectangles (atomics into a zero-filled output), 2 regions   */
    int32_t split;              /* wgrad: reduction slices                                                        */
    int32_t zero_fill;          /* the call zero-fills its output first                                           */
    int32_t colstats_ok;        /* fwd: glf_conv_params.colstats can be honoured                                  */
    int64_t workspace_bytes;    /* wgrad: scratch for the two-stage split-K reduction (0: none needed)            */
} glf_conv_plan;
/* pass 3 = the folded forward (glf_conv2d_fwd_folded): as pass 0, except that a 3x3 stride-1 conv with pad == dil on
 * equal maps and cin % 32 == 0 that pass 0 would run as per-tap rectangles runs in region mode (rect = 2: every output
 * element stored once, no zero fill); rect = 1 in a pass-3 plan means the folded entry point refuses the conv. */
int glf_conv2d_plan(const glf_conv_params* p, int pass /* 0 fwd, 1 dgrad, 2 wgrad, 3 folded fwd */, glf_conv_plan* plan);
int glf_conv2d_fwd(const float* x, const float* w_tap, const float* bias, float* y, const glf_conv_params* p, glf_stream_t s);
/* Inference forward with the BatchNorm folded in: y = act(conv(x, w_tap_folded) + shift[cout] (+ residual)), one launch,
 * y written once.  w_tap_folded / shift from glf_fold_bn; residual (optional) [n*ho*wo][ld_res] rows like y's; relu 0 / 1.
 * Precision 3 / 4 only.  Checked before any HIP runtime call: GLF_ERR_NULL, GLF_ERR_BAD_SHAPE, and GLF_ERR_UNSUPPORTED
 * for p->colstats, other precisions and a conv whose pass-3 plan is rect = 1 (run glf_conv2d_fwd + glf_bn_act for it). */
int glf_conv2d_fwd_folded(const float* x, const float* w_tap_folded, const float* shift, const float* residual, int64_t ld_res,
                          int relu, float* y, const glf_conv_params* p, glf_stream_t s);
/* w_tap_t: the same weights as [tap][cin][cout] (glf_oihw_to_tap_major_t); needed by the split-precision kernels,
 * may be NULL for exact fp32 (then w_tap is used). */
int glf_conv2d_dgrad(const float* dy, const float* w_tap, const float* w_tap_t, float* dx, const glf_conv_params* p, glf_stream_t s);
/* dw_tap [kh*kw][cout][cin].  workspace (>= plan.workspace_bytes, may be NULL: float atomics instead of the two-stage
 * reduction) is caller-owned scratch. */
int glf_conv2d_wgrad(const float* dy, const float* x, float* dw_tap, float* workspace, int64_t workspace_bytes,
                     const glf_conv_params* p, glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * Fused softmax attention of TPAVIModule's `embedded` mode (ours.py:881, 896-897, 902):
 *   y[n] = softmax(theta[n] phi[n]^T, dim = -1) g[n]      per frame n, theta / phi / g: [L][Ci] rows (row strides ld*).
 * One kernel per pass; the [L][L] score matrix is never written to memory (online row max / sum over 64-key tiles
 * staged through LDS, P g accumulated in MFMA accumulators; backward recomputes the tiles from theta, phi and the saved
 * row log-sum-exp).  Exact fp32 arithmetic (v_mfma_f32_32x32x2_f32).  Ci % 32 == 0, Ci <= 1024; frame n of every operand
 * starts L rows after frame n - 1 (frame stride = L * its row stride).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t frames, L, ci;
    int64_t ldq, ldk, ldv;      /* row strides of theta, phi, g (elements; column slices of one [rows][3 Ci] buffer: 3 Ci) */
    int64_t ldy;                /* row stride of y                                                                       */
    int64_t lddy;               /* backward: row stride of dy                                                            */
    int64_t ldd;                /* backward: common row stride of dtheta, dphi, dg                                        */
} glf_attn_params;
/* y [frames*L][Ci] and lse [frames*L] (row log-sum-exp, needed by the backward pass). */
int glf_attn_softmax_fwd(const float* theta, const float* phi, const float* g, float* y, float* lse,
                         const glf_attn_params* p, glf_stream_t stream);
/* dtheta, dphi, dg from dy (every output element is written exactly once: no zero fill, no atomics).
 * dsum_ws: caller-owned scratch of frames*L floats. */
int glf_attn_softmax_bwd(const float* theta, const float* phi, const float* g, const float* y, const float* dy, const float* lse,
                         float* dtheta, float* dphi, float* dg, float* dsum_ws, const glf_attn_params* p, glf_stream_t stream);
/* The same attention under 16-bit storage: theta, phi, g, y, dy and the three gradients are bf16 (void* = bf16 data), lse and
 * dsum_ws fp32 [frames*L].  S = theta phi^T on bf16 MFMA with fp32 accumulation; row max, row sum and rescaling in fp32; P is
 * rounded to bf16 only as the A operand of P g; y is accumulated and normalised in fp32 and stored as bf16 once.  Backward:
 * D = rowsum(dy o y) and dS = P (dP - D) in fp32, dS rounded to bf16 only as an MFMA operand; every output element is written
 * exactly once (no atomics, no zero fill: bitwise reproducible).  Ci % 64 == 0, Ci <= 1024, any L >= 1; every row stride
 * (ldq, ldk, ldv, ldy; backward also lddy, ldd) a multiple of 8 elements and >= Ci, theta / phi / g / y / dy 16-byte
 * aligned; frame stride = L * row stride.  dsum_ws is caller-owned; the calls allocate nothing and never wait on the host.
 * Arguments are checked before any HIP runtime call: GLF_ERR_NULL, GLF_ERR_BAD_SHAPE (frames or L < 1),
 * GLF_ERR_UNSUPPORTED (Ci, strides, alignment). */
int glf_s16_attn_softmax_fwd(const void* theta, const void* phi, const void* g, void* y, float* lse,
                             const glf_attn_params* p, glf_stream_t stream);
int glf_s16_attn_softmax_bwd(const void* theta, const void* phi, const void* g, const void* y, const void* dy,
                             const float* lse, void* dtheta, void* dphi, void* dg, float* dsum_ws,
                             const glf_attn_params* p, glf_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused pairwise-ReLU attention of TPAVIModule's `concatenate` mode (ours.py:883-894, 898-900, 902):
 *   s_ij = a[i] + b[j] + c ;  y[n][i] = (1 / L) sum_j relu(s_ij) g[n][j]      per frame n,
 * a = theta w_theta and b = phi w_phi being ONE scalar per position ([w_theta | w_phi] = the W_f.0.weight row, c = W_f.0.bias).
 * a, b: [frames*L] fp32; c: a DEVICE scalar (no host synchronisation); g: [L][Ci] rows per frame with row stride ldg (a
 * column slice of a wider buffer).  The 64 x 64 tiles of relu(s) are computed on the VALU, left in LDS and contracted with the
 * g rows into MFMA accumulators: nothing of size L x L is written.  Exact fp32 arithmetic (v_mfma_f32_32x32x2_f32) under
 * every precision setting.  Ci % 32 == 0, Ci <= 1024, any L >= 1; frame n of g / y / dy / dg starts L rows after frame n - 1.
 * Backward: dg (row stride lddg), da, db [frames*L] and dc [1] from dy (row stride lddy; g and dy 16-byte aligned, ldg and
 * lddy multiples of 4).  Every output element is written exactly once, no atomics, no zero fill; da, db and dc are summed in
 * a fixed order, so two runs are bitwise equal.  workspace: caller-owned, glf_attn_pair_relu_workspace_bytes() bytes
 * (one partial row of db per 64-query block: frames * ceil(L / 64) * L floats).
 * Arguments are checked before any HIP runtime call: GLF_ERR_NULL, GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED (Ci),
 * GLF_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t frames, L, ci;
    int32_t reserved0;
    int64_t ldg;                /* row stride of g (elements)   */
    int64_t ldy;                /* row stride of y              */
    int64_t lddy;               /* backward: row stride of dy   */
    int64_t lddg;               /* backward: row stride of dg   */
} glf_attn_pair_params;
size_t glf_sizeof_attn_pair_params(void);
size_t glf_attn_pair_relu_workspace_bytes(const glf_attn_pair_params* p);
int glf_attn_pair_relu_fwd(const float* a, const float* b, const float* c, const float* g, float* y,
                           const glf_attn_pair_params* p, glf_stream_t stream);
int glf_attn_pair_relu_bwd(const float* a, const float* b, const float* c, const float* g, const float* dy, float* dg,
                           float* da, float* db, float* dc, float* workspace, int64_t workspace_bytes,
                           const glf_attn_pair_params* p, glf_stream_t stream);
/* The skinny ends of the mode.  Forward: a[r] = theta[r] . w[0 .. Ci), b[r] = phi[r] . w[Ci .. 2 Ci) for rows of stride ld.
 * Backward: dtheta[r] = da[r] w[0 .. Ci), dphi[r] = db[r] w[Ci .. 2 Ci) (row stride ldd) and dw[2 Ci] = [theta^T da | phi^T db],
 * summed over slabs of 256 rows and then over the slabs in order, in double (bitwise reproducible).  workspace: caller-owned,
 * glf_attn_pair_proj_workspace_bytes(rows, Ci) bytes. */
size_t glf_attn_pair_proj_workspace_bytes(int64_t rows, int ci);
int glf_attn_pair_proj_fwd(const float* theta, const float* phi, int64_t ld, const float* w, float* a, float* b, int64_t rows, int ci,
                           glf_stream_t stream);
int glf_attn_pair_proj_bwd(const float* theta, const float* phi, int64_t ld, const float* w, const float* da, const float* db,
                           float* dtheta, float* dphi, int64_t ldd, float* dw, float* workspace, int64_t workspace_bytes, int64_t rows,
                           int ci, glf_stream_t stream);
/* The same mode under 16-bit storage (csrc/attn_pair_s16.hip): g, y, dy, dg (and theta, phi, dtheta, dphi of the skinny ends) are
 * bf16 (void* = bf16 data); a, b, da, db, dc, w, dw and the workspaces stay fp32, so all three kernels evaluate
 * s = (a_i + b_j) + c in fp32 and the backward mask is the forward's.  The relu(s) tile is computed in fp32 and rounded to bf16
 * only as the A operand of v_mfma_f32_32x32x16_bf16; y and dg are accumulated in fp32, scaled by 1 / L in fp32 and stored as bf16
 * once; t = dY g^T on the bf16 MFMA with fp32 accumulation, masked in fp32, summed to da / db / dc in a fixed order (dc: a fixed
 * tree in double).  Every output element is written exactly once (no atomics, no zero fill: bitwise reproducible); the calls
 * allocate nothing and never wait on the host.  Ci % 64 == 0, Ci <= 1024, any L >= 1; every row stride a multiple of 8 elements
 * and >= Ci, g / dy 16-byte aligned.  Workspaces as for the fp32 entry points (their own *_workspace_bytes functions).
 * Arguments are checked before any HIP runtime call, in this order: GLF_ERR_NULL, GLF_ERR_BAD_SHAPE (extents),
 * GLF_ERR_UNSUPPORTED (Ci, strides, alignment), GLF_ERR_WORKSPACE. */
size_t glf_s16_attn_pair_relu_workspace_bytes(const glf_attn_pair_params* p);
int glf_s16_attn_pair_relu_fwd(const float* a, const float* b, const float* c, const void* g, void* y,
                               const glf_attn_pair_params* p, glf_stream_t stream);
int glf_s16_attn_pair_relu_bwd(const float* a, const float* b, const float* c, const void* g, const void* dy, void* dg,
                               float* da, float* db, float* dc, float* workspace, int64_t workspace_bytes,
                               const glf_attn_pair_params* p, glf_stream_t stream);
/* a = theta w_theta, b = phi w_phi from bf16 rows and the fp32 W_f row (fp32 sums, one wavefront per row; Ci and ld multiples of
 * 8); dtheta = da w_theta^T, dphi = db w_phi^T stored as bf16 (row stride ldd), dw fp32 over 256-row slabs added in order in double. */
size_t glf_s16_attn_pair_proj_workspace_bytes(int64_t rows, int ci);
int glf_s16_attn_pair_proj_fwd(const void* theta, const void* phi, int64_t ld, const float* w, float* a, float* b, int64_t rows, int ci,
                               glf_stream_t stream);
int glf_s16_attn_pair_proj_bwd(const void* theta, const void* phi, int64_t ld, const float* w, const float* da, const float* db,
                               void* dtheta, void* dphi, int64_t ldd, float* dw, float* workspace, int64_t workspace_bytes, int64_t rows,
                               int ci, glf_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Weight layout: torch OIHW [Cout][Cin][kh][kw] <-> tap-major [kh*kw][Cout][Cin].
 * ------------------------------------------------------------------------------------- */
int glf_oihw_to_tap_major(const float* w, float* out, int cout, int cin, int taps, glf_stream_t s);
/* Eval-mode BatchNorm folded into tap-major conv weights, one launch per conv (fp32, scale computed in double):
 *     s_o = gamma_o / sqrt(var_o + eps),   w_out[t][o][i] = w_tap[t][o][i] * s_o,   shift_out[o] = beta_o + (bias_o - mean_o) * s_o
 * conv_bias may be NULL (0).  w_out may not alias w_tap.  GLF_ERR_NULL / GLF_ERR_BAD_SHAPE (taps, cout, cin < 1, eps < 0)
 * before any HIP runtime call. */
int glf_fold_bn(const float* w_tap, const float* conv_bias, const float* gamma, const float* beta, const float* mean, const float* var,
                float eps, float* w_out, float* shift_out, int taps, int cout, int cin, glf_stream_t s);
/* The same fold for 16-bit storage: w_folded_bf16[t][o][i] = bf16(w_tap[t][o][i] * s_o) with the product taken in double and
 * rounded ONCE, to nearest even (no fp32 W' in between); shift as glf_fold_bn (fp32).  cin % 8 == 0 (16-byte rows of bf16), else
 * GLF_ERR_UNSUPPORTED.  GLF_ERR_NULL, then GLF_ERR_BAD_SHAPE (taps, cout, cin < 1, eps < 0), before any HIP runtime call. */
int glf_s16_fold_bn(const float* w_tap, const float* bias /* may be NULL */, const float* gamma, const float* beta,
                    const float* mean, const float* var, float eps, void* w_folded_bf16, float* shift,
                    int taps, int cout, int cin, glf_stream_t s);
int glf_tap_major_to_oihw(const float* w, float* out, int cout, int cin, int taps, glf_stream_t s);
/* [kh*kw][Cin][Cout] (k = Cout contiguous): the dgrad weight operand when dgrad runs as an NT contraction. */
int glf_oihw_to_tap_major_t(const float* w, float* out, int cout, int cin, int taps, glf_stream_t s);
/* batched 2-D transpose dst[b][c][r] = src[b][r][c] (operand re-layout for NT contractions). */
int glf_transpose2d(const float* src, float* dst, int rows, int cols, int batch, glf_stream_t s);
/* The same with strides: src[b][r][c] = src[b * batch_stride_src + r * ld_src + c]; dst[b][c][r] (row stride ld_dst) for r < rows,
 * ZERO for rows <= r < rows_pad: a column slice of a wider matrix transposed into an operand whose reduction dimension is padded to
 * the contraction kernels' K granule (the g^T / phi^T operands of the per-frame softmax attention, fusion.py). */
int glf_transpose2d_strided(const float* src, int64_t ld_src, int64_t batch_stride_src, float* dst, int64_t ld_dst,
                            int64_t batch_stride_dst, int rows, int cols, int rows_pad, int batch, glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * Multi-tensor weight refresh.  Everything the contraction kernels derive from the parameters -- tap-major re-layouts
 * (forward / wgrad order and the transposed dgrad order), transposed copies of 1x1 / linear weights, the stacked
 * theta | phi | g operand of a fusion block (ours.py:866,878-879), each parameter's max magnitude (precision 3 / 4) and
 * the packed pre-split images of all of those -- has to be rebuilt after EVERY optimizer step (main.py:243).  Through the
 * per-tensor entry points above that is one launch per image, ~1 000 launches per update for the 3-view model; this block
 * does it in one launch per dependency level.  The caller describes every derived image once as a glf_weight_job (pointers
 * are caller-owned and must stay valid), sorts the jobs by `pass`, lets glf_weights_plan fill in the grid bookkeeping,
 * copies the table to the device, and calls glf_weights_refresh after each update.  Results are bit-identical to the
 * per-tensor entry points.
 * ------------------------------------------------------------------------------------- */
enum {
    GLF_WJ_COPY = 0,        /* dst[i] = src[i], d0 elements; with d1 > 0 a strided gather dst[i] = src[i * d1 + d2] (d1 = taps, d2 = taps / 2:
                               the centre tap of an OIHW weight as a dense [Cout][Cin] row block of the stacked centre-tap operand of an
                               ASPP head, whose maximum, transpose and packed forms are ordinary jobs on the stacked buffer)  (pass 0) */
    GLF_WJ_AMAX = 1,        /* *amax = max(*amax, max|src|), d0 elements; dst unused           (pass 1) */
    GLF_WJ_TAP_MAJOR = 2,   /* src OIHW [d0=Cout][d1=Cin][d2=taps] -> dst [taps][Cout][Cin]     (pass 2) */
    GLF_WJ_TAP_MAJOR_T = 3, /* ... -> dst [taps][Cin][Cout]                                     (pass 2) */
    GLF_WJ_TRANSPOSE = 4,   /* src [d0=rows][d1=cols] -> dst [cols][rows]                       (pass 2) */
    GLF_WJ_PACK = 5,        /* dst = packed pre-split image of src (d0 elements, % 4 == 0, both 16-byte aligned)
                               scaled by *amax, as glf_split_f16_packed                          (pass 3) */
    GLF_WJ_ZERO = 6,        /* dst[i] = 0, d0 elements (src unused): the amax slots of a table that covers only SOME of an
                               arena's parameters -- such a caller passes amax_arena = NULL to glf_weights_refresh      (pass 0) */
    GLF_WJ_CVT_BF16 = 7,    /* dst (bf16 elements behind the float* field) = round-to-nearest-even(src), d0 elements (% 4 == 0): the operand
                               images of the 16-bit-storage contractions, from fp32 master weights or their layouts   (pass 3) */
    GLF_WJ_PASSES = 4
};
typedef struct {
    const float* src;
    float* dst;
    float* amax;            /* AMAX: the slot to raise (inside the arena glf_weights_refresh zero-fills); PACK: the scale source */
    int32_t kind;           /* GLF_WJ_*                                                        */
    int32_t pass;           /* dependency level, 0 .. GLF_WJ_PASSES-1; the table is sorted by it */
    int32_t d0, d1, d2;     /* extents, see the kinds                                          */
    int32_t reserved;
    int64_t first_wg;       /* filled by glf_weights_plan: first workgroup of this job in its pass */
} glf_weight_job;
/* Validates a HOST table sorted by pass, fills first_wg of every job and, per pass p (arrays of GLF_WJ_PASSES entries),
 * the index of its first job, its job count and its workgroup count.  No device work. */
int glf_weights_plan(glf_weight_job* jobs_host, int n_jobs, int* pass_first, int* pass_count, int64_t* pass_wgs);
/* Zero-fills amax_arena[0 .. amax_floats) (may be NULL / 0) and runs the passes of a planned table that has been copied
 * to device memory (jobs_dev), in order, on `s`. */
int glf_weights_refresh(const glf_weight_job* jobs_dev, const int* pass_first, const int* pass_count, const int64_t* pass_wgs,
                        float* amax_arena, int64_t amax_floats, glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * 16-bit storage ("S16"), streaming kernels: the counterparts of the normalisation / pointwise
 * entry points above for bf16 tensors (`void*` = bf16 elements unless named float; channel
 * counts and row strides multiples of 8, 16-byte aligned tensors).  fp32 arithmetic, one
 * rounding at the store.  BatchNorm sums follow the glf_gemm_params.colstats contract: DEVICE
 * doubles [2][C], zero-filled by the caller, filled by glf_s16_gemm_nt's epilogue or by
 * glf_s16_colstats; the apply kernels finish the statistics themselves.
 * ------------------------------------------------------------------------------------- */
/* sums[c] += sum_r x[r][c]; sums[C + c] += sum_r x[r][c]^2 (f64 atomics, one per column and workgroup). */
int glf_s16_colstats(const void* x, int ldx, int rows, int c, double* sums, glf_stream_t s);
/* y = [relu]( BN(x) [+ residual] ).  sums != NULL (train): batch statistics from sums, written to mean / invstd, running
 * statistics updated (as glf_bn_apply_from_sums).  sums == NULL (eval): mean / invstd are inputs (glf_bn_eval_coeffs).
 * relu_mask (may be NULL): one byte per 8 channels, bit j = sign of the pre-ReLU value of channel 8 i + j. */
int glf_s16_bn_apply(const void* x, int ldx, const void* residual, int ldr, void* y, int ldy, const double* sums,
                     int rows, int c, float eps, float momentum, const float* gamma, const float* beta,
                     float* mean, float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     int relu, uint8_t* relu_mask, glf_stream_t s);
/* BatchNorm backward in two launches: column reduction (sum dy', sum dy' xhat; into `sums`, DEVICE doubles [2][C] zero-filled
 * by the caller) and apply (finishes the sums, writes dgamma / dbeta / dx / dres).  dy2 (may be NULL): second addend of the
 * incoming gradient; relu: relu_mask (bytes of glf_s16_bn_apply) or, without a residual, recomputed from x and beta. */
int glf_s16_bn_bwd(const void* dy, int lddy, const void* dy2, int lddy2, const void* x, int ldx,
                   const float* mean, const float* invstd, const float* gamma, const float* beta,
                   void* dx, int lddx, void* dres, int lddres, float* dgamma, float* dbeta,
                   int rows, int c, int relu, int training, double* sums, const uint8_t* relu_mask, glf_stream_t s);
/* db[c] = sum_r dy[r][c]; workspace: 2 C doubles (zero-filled by the call). */
int glf_s16_colsum(const void* dy, int lddy, float* db, int rows, int c, double* workspace, glf_stream_t s);
/* TPAVI tail (ours.py:908-915) on bf16 w, x, z, dz, du; statistics vectors fp32. */
int glf_s16_bn_res_ln_fwd(const void* w, const void* x, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                          const float* bn_beta, const float* ln_gamma, const float* ln_beta, float ln_eps, void* z,
                          float* row_mean, float* row_rstd, int rows, int c, glf_stream_t s);
size_t glf_s16_bn_res_ln_workspace(int rows, int c);   /* bytes */
int glf_s16_bn_res_ln_bwd(const void* dz, const void* w, const void* x, const float* bn_mean, const float* bn_invstd,
                          const float* bn_gamma, const float* bn_beta, const float* ln_gamma, const float* row_mean,
                          const float* row_rstd, void* du, float* dln_gamma, float* dln_beta, int rows, int c,
                          float* workspace, glf_stream_t s);
/* Stem with a bf16 conv output / output gradient (x, w, bias, dw, db fp32). */
int glf_s16_stem7x7_fwd(const float* x, const float* w, const float* bias, void* y,
                        int n, int h, int wdt, int cout, int pad, glf_stream_t s);
int glf_s16_stem7x7_wgrad(const float* x, const void* dy, float* dw, float* db, float* partial,
                          int n, int h, int wdt, int cout, int pad, glf_stream_t s);
int glf_s16_stem7x7_dgrad(const void* dy, const float* w, float* dx, int n, int h, int wdt, int cout, int pad, glf_stream_t s);
int glf_s16_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s);
int glf_s16_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, glf_stream_t s);
/* y[n][c] = scale * sum_p x[n][p][c] (x bf16, row stride ldx; y of y_dtype); y[n][p][c] (bf16, row stride ldy) = scale * x[n][c]
 * (x of x_dtype).  The ASPP pooled branch (deeplabv3.py:123-135) keeps its N per-frame vectors in fp32. */
int glf_s16_sum_rows(const void* x, int ldx, void* y, int y_dtype, float scale, int n, int p, int c, glf_stream_t s);
int glf_s16_bcast_rows(const void* x, int x_dtype, void* y, int ldy, float scale, int n, int p, int c, glf_stream_t s);
int glf_s16_dropout(const void* x, void* y, int64_t numel, float p, uint64_t seed, const uint64_t* step_counter, glf_stream_t s);
int glf_s16_relu_fwd(const void* x, void* y, int64_t numel, glf_stream_t s);
int glf_s16_relu_bwd(const void* dy, const void* y, void* dx, int64_t numel, glf_stream_t s);
int glf_s16_axpby(const void* x, const void* y, void* out, float a, float b, int64_t numel, glf_stream_t s);
/* Local gate (ours.py:1802-1816): cls / ctr logits, gate map, their gradients fp32; f, y, dy, df bf16. */
int glf_s16_gate_fwd(const float* cls, int ncls, const float* ctr, const void* f, void* y, float* a, int32_t* argmax, float weight,
                     int rows, int c, glf_stream_t s);
int glf_s16_gate_bwd(const void* dy, const void* f, const float* cls, int ncls, const float* ctr, const float* a, const int32_t* argmax,
                     float weight, void* df, float* dcls, float* dctr, int rows, int c, glf_stream_t s);
int glf_s16_add_frames(const void* a, int64_t a_fs, const void* b, int64_t b_fs, void* dst, int64_t dst_fs, int n, int64_t inner,
                       glf_stream_t s);
int glf_s16_add_n(const void* const* inputs, int k, void* out, int64_t numel, glf_stream_t s);
/* dst (dst_dtype) = src (src_dtype): GLF_DT_BF16 -> GLF_DT_F32 or GLF_DT_F32 -> GLF_DT_BF16; numel % 8 == 0. */
int glf_s16_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t numel, glf_stream_t s);
/* dst[b][c][r] = src[b][r][c] for 16-bit elements. */
int glf_s16_transpose2d(const void* src, void* dst, int rows, int cols, int batch, glf_stream_t s);
/* glf_transpose2d_strided for 16-bit elements: dst[b][c][r] (row stride ld_dst) = src[b][r][c] (row stride ld_src) for r < rows,
 * ZERO for rows <= r < rows_pad. */
int glf_s16_transpose2d_strided(const void* src, int64_t ld_src, int64_t batch_stride_src, void* dst, int64_t ld_dst,
                                int64_t batch_stride_dst, int rows, int cols, int rows_pad, int batch, glf_stream_t s);
/* Row softmax of fp32 scores into a bf16 contraction operand ('gaussian' under 16-bit storage):
 *   fwd: p[r][c] = softmax_c(s[r][0 .. cols));   bwd: ds[r][c] = P (dp - rowsum(P o dp)) with P recomputed from s in fp32.
 * Row max / sum / normalisation in fp32, one rounding to bf16 at the store; the pad columns [cols, ld_p) / [cols, ld_ds) are
 * written as ZERO (the operand's reduction extent is padded to the contraction kernels' K granule).  16-byte accesses, one row
 * per wavefront (cols <= 1024) or per workgroup, no atomics: bitwise reproducible.  fp32 row strides multiples of 4, the bf16
 * row stride a multiple of 8, all >= cols, every operand 16-byte aligned.  Checked before any HIP runtime call: GLF_ERR_NULL,
 * GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED. */
int glf_s16_softmax_rows_fwd(const float* s, void* p, int64_t rows, int cols, int64_t ld_s, int64_t ld_p, glf_stream_t stream);
int glf_s16_softmax_rows_bwd(const float* s, const float* dp, void* ds, int64_t rows, int cols, int64_t ld_s, int64_t ld_dp,
                             int64_t ld_ds, glf_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Single-call fusion block, 16-bit storage (SURVEY 8b rows tpavi_proj + tpavi_attn_dot +
 * tpavi_out_bn_res_ln; TPAVIModule.forward, ours.py:845-917, mode 'dot' -- the shipped model).
 * One call per direction enqueues the whole block on `stream`; the library allocates nothing:
 * results, the tensors kept for backward and the workspace are caller-owned device buffers.
 *   x, z, dz, dx   [n*L][C]    bf16   (n clips of L = V*h*w positions, channels-last)
 *   w_qkv          [3 Ci][C]   bf16   theta | phi | g weights stacked;  b_qkv [3 Ci] fp32
 *   w_z            [C][Ci]     bf16;  b_z [C] fp32
 *   w_qkv_t / w_z_t             bf16   their transposes [C][3 Ci] / [Ci][C] (glf_s16_transpose2d)
 *   qkv [n*L][3 Ci], att_t [n][Ci][Ci], y [n*L][Ci], wz [n*L][C]  bf16, bn_mean / bn_invstd [C],
 *   row_mean / row_rstd [n*L] fp32: written by the forward, read by the backward.
 *   dw_* / db_* / d*_gamma / d*_beta: fp32, torch parameter layouts.
 * C, Ci multiples of 64, C <= 2048.  Workspace: glf_s16_tpavi_workspace_bytes(p, pass) bytes (pass 0 = forward,
 * 1 = backward), 256-byte aligned, contents undefined on entry and exit.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, L, c, ci;
    int32_t training;            /* BatchNorm3d mode: batch statistics + running update (1) or running statistics (0) */
    float bn_eps, bn_momentum, ln_eps;
} glf_tpavi_params;
size_t glf_sizeof_tpavi_params(void);
size_t glf_s16_tpavi_workspace_bytes(const glf_tpavi_params* p, int pass);
int glf_s16_tpavi_fwd(const void* x, const void* w_qkv, const float* b_qkv, const void* w_z, const float* b_z,
                      const float* bn_gamma, const float* bn_beta, float* bn_running_mean, float* bn_running_var,
                      int64_t* num_batches_tracked, const float* ln_gamma, const float* ln_beta, void* z,
                      void* qkv, void* att_t, void* y, void* wz, float* bn_mean, float* bn_invstd, float* row_mean, float* row_rstd,
                      const glf_tpavi_params* p, void* workspace, size_t workspace_bytes, glf_stream_t stream);
int glf_s16_tpavi_bwd(const void* dz, const void* x, const void* qkv, const void* att_t, const void* y, const void* wz,
                      const float* bn_mean, const float* bn_invstd, const float* row_mean, const float* row_rstd,
                      const void* w_qkv_t, const void* w_z_t, const float* bn_gamma, const float* bn_beta, const float* ln_gamma,
                      void* dx, float* dw_qkv, float* db_qkv, float* dw_z, float* db_z, float* dbn_gamma, float* dbn_beta,
                      float* dln_gamma, float* dln_beta, const glf_tpavi_params* p, void* workspace, size_t workspace_bytes,
                      glf_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Stem (a2): Conv2d(1,64,7,stride 1,pad 2)+bias (models/_utils.py:192; used ours.py:1796).
 * x [N][H][W] (C=1), w [Cout][49], y [N][Ho][Wo][Cout] with Ho = H + 2*pad - 6.
 * ------------------------------------------------------------------------------------- */
int glf_stem7x7_fwd(const float* x, const float* w, const float* bias, float* y,
                    int n, int h, int wdt, int cout, int pad, glf_stream_t s);
/* Inference-mode stem in one launch (SURVEY 8b `stem7x7_bn_relu_pool`; ours.py:1725-1730, 1796: init_block = conv1, bn1, relu,
 * maxpool): y [N][Hp][Wp][Cout] = maxpool3x3s2p1(relu(bn(conv7x7(x) + bias))) with Hp = (Ho - 1) / 2 + 1 and the BatchNorm given by
 * mean / invstd (glf_bn_eval_coeffs of the running statistics), gamma, beta.  The conv output and its normalised copy are never
 * written.  Values equal the three-launch chain's bit for bit (same tap order, same BatchNorm expression).  amax_out (may be NULL):
 * as in glf_bn_apply.  Forward only: a train-mode step needs the batch statistics of the conv output before it can normalise, and
 * the conv output again in backward -- the three kernels stay. */
int glf_stem7x7_bn_relu_pool(const float* x, const float* w, const float* bias, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, float* y, int n, int h, int wdt, int cout, int pad,
                             float* amax_out, glf_stream_t s);
/* dW [Cout][49] and db [Cout]; partial must hold glf_stem7x7_wgrad_workspace() floats. */
size_t glf_stem7x7_wgrad_workspace(int n, int h, int wdt, int cout, int pad);
int glf_stem7x7_wgrad(const float* x, const float* dy, float* dw, float* db, float* partial,
                      int n, int h, int wdt, int cout, int pad, glf_stream_t s);
/* The stem's input gradient, for a stem whose image is itself computed (early_fusion mixes the views' images by a learned 1x1
 * convolution, ours.py:2299-2304): dx [N][H][W] fp32, dx[n][iy][ix] = sum_taps sum_co dy[n][iy - ky + pad][ix - kx + pad][co] *
 * w[co][ky][kx] over the taps that land inside dy [N][H + 2 pad - 6][W + 2 pad - 6][Cout] (16-byte aligned; bf16 for glf_s16_*).
 * Every element of dx is written once; no atomics. */
int glf_stem7x7_dgrad(const float* dy, const float* w, float* dx, int n, int h, int wdt, int cout, int pad, glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * BatchNorm (nn.BatchNorm2d / BatchNorm3d in train and eval mode), channels-last [rows][C].
 * ------------------------------------------------------------------------------------- */
/* number of doubles of workspace for bn_stats / bn_bwd_reduce */
size_t glf_bn_workspace(int rows, int c);
/* Batch statistics over `rows`: writes mean[c], invstd[c] (biased var, eps) and, when
 * running_mean != NULL, updates running_mean/var with `momentum` (unbiased var), as
 * nn.BatchNorm does in train(). */
int glf_bn_stats(const float* x, int ldx, int rows, int c, float eps, float momentum,
                 float* mean, float* invstd, float* running_mean, float* running_var,
                 int64_t* num_batches_tracked /* may be NULL; += 1 */,
                 double* workspace, glf_stream_t s);
/* The same outputs / running-statistics update as glf_bn_stats from per-channel sums[2][c] = (sum x, sum x^2) over
 * `rows` rows -- the colstats a contraction epilogue accumulated. */
int glf_bn_stats_from_sums(const double* sums, int rows, int c, float eps, float momentum, float* mean, float* invstd,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, glf_stream_t s);
/* Replays the running-statistics update of a train-mode BatchNorm from its saved batch statistics (mean, invstd over
 * `rows` samples): running_* <- (1 - momentum) running_* + momentum {mean, unbiased var}, num_batches_tracked += 1.
 * The engine shares the ASPP trunk between the two classifier calls on the same f4 (ours.py:1806, 1840); the second
 * call's three-fold effect on the buffers is reproduced with this. */
int glf_bn_replay_running(const float* mean, const float* invstd, int rows, int c, float eps, float momentum,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, glf_stream_t s);
/* y = [relu]( (x - mean)*invstd*gamma + beta [+ residual] ).  For eval() pass running_mean and
 * 1/sqrt(running_var+eps) (glf_bn_eval_coeffs).  In-place (y == x) allowed.
 * amax_out (may be NULL): device float that must hold 0 (or any lower bound) before the call and
 * receives max(*amax_out, max|y|) -- the operand maximum the f16x3 contractions need, for free. */
int glf_bn_eval_coeffs(const float* running_mean, const float* running_var, float eps,
                       float* mean, float* invstd, int c, glf_stream_t s);
/* relu_mask (may be NULL): receives the sign of the pre-ReLU value, one byte per four consecutive channels (bit j = element
 * 4 i + j is positive; [rows][c / 4] dense) -- what glf_bn_bwd needs of the forward output when a residual was added: the
 * backward passes then read 1 byte where they read 16 (y is the largest tensor class of the path: the block outputs). */
int glf_bn_apply(const float* x, int ldx, const float* residual, int ldr, float* y, int ldy,
                 const float* mean, const float* invstd, const float* gamma, const float* beta,
                 int rows, int c, int relu, float* amax_out, uint8_t* relu_mask, glf_stream_t s);
/* glf_bn_stats_from_sums + glf_bn_apply in ONE launch (train mode, statistics from a contraction's colstats): every
 * workgroup finishes mean / invstd for the channels of its own column block in LDS, the workgroups of the first row slice
 * write them to mean / invstd (for the backward pass) and update running_mean / running_var / num_batches_tracked (all
 * three may be NULL).  Bit-identical to the two calls.
 * C <= 4096.
 * colmax (may be NULL; precision 3 / 4 callers): the per-channel maxima of |x| the same contraction epilogue left
 * (glf_gemm_params.colmax).  With it y is NOT written as fp32 but once, directly, as the packed pre-split image of
 * glf_split_f16_packed -- the form the next convolution reads in its forward AND its weight gradient (a_presplit /
 * b_presplit) -- scaled with the bound  max_c |gamma_c| invstd_c (max|x_c| + |mean_c|) + |beta_c|  >=  max |y|, which is
 * known before a single element of y is; *amax_out receives that bound (plain store).  Needs amax_out, no residual, y != x.
 * The fp32 y is then never materialised: the activation inside a bottleneck costs 4 B / element once instead of
 * 4 B (write) + 4 B (re-read by the split pass) + 4 B (the image). */
int glf_bn_apply_from_sums(const float* x, int ldx, const float* residual, int ldr, float* y, int ldy, const double* sums,
                           int rows, int c, float eps, float momentum, const float* gamma, const float* beta,
                           float* mean, float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           int relu, float* amax_out, uint8_t* relu_mask, const float* colmax, glf_stream_t s);
/* Backward.  y is the forward output (ReLU mask = y > 0); it may be NULL when relu == 0, and also when
 * relu != 0 and there was NO residual: the mask is then recomputed from x with beta (one tensor read less
 * in both passes; with a residual the sign of y depends on it, so y is required).
 * training != 0: full batch-stat backward; training == 0: dx = dy*mask*gamma*invstd.
 * dres (may be NULL) receives dy*mask (gradient of the residual input).  amax_out: as in
 * glf_bn_apply, for dx.
 * packed_dx != 0 (precision 3 / 4 callers): dx is NOT written as fp32 but directly as the packed pre-split image of
 * glf_split_f16_packed -- what the producing convolution's dgrad and wgrad read (glf_gemm_params.a_presplit) -- so the
 * gradient of a conv output exists once, in the form its consumers want, and the separate split pass (one read + one write
 * of the tensor) is gone.  The image's power-of-two scale must be known before the first element is written: the reduction
 * pass also takes max|dy'| and max|xhat| per channel, and *amax_out (required, zeroed by the caller) receives the upper
 * bound of max|dx| derived from them (typically within 2x of the true maximum); pass the same scalar as amax_a.
 * packed_dx = 2 / 3 split that form in two for layers whose packed gradients are column slices of ONE image under ONE scale
 * (the conv branches of an ASPP head): 2 = reduction only (needs workspace, dgamma, dbeta, which are final afterwards; the
 * bound is raised into *amax_out by an atomic maximum), 3 = the apply pass only (same amax_out).  Run every layer's half 2
 * with the same amax_out before the first half 3.  In both halves fused_sums is required and means something else: 2 c floats
 * (no zero fill) that the caller keeps per layer from half 2, which stores the channel sums there as well, to half 3, which
 * reads them there and never touches dgamma / dbeta (which it takes as NULL) -- those may be reduced over ranks or accumulated into in between.
 * packed_dx = 4 is half 3 with dx written as plain fp32 (amax_out may be NULL; non-NULL it receives max|dx| as with packed_dx = 0).
 * dy2 (may be NULL; row stride lddy2): a second addend of the incoming gradient -- the node sees dy + dy2.  The input of a
 * residual block feeds its shortcut and its first conv (models/resnet.py:59-79), so the gradient that reaches the previous
 * block's last BatchNorm is a sum of two tensors: both passes add them while reading instead of a separate add kernel
 * writing the sum (3 tensor passes) that both passes then read (2 more).
 * Internal contract of the two-launch form (fused_sums) with BOTH dy2 and dres: the reduction pass stores the masked sum
 * (dy + dy2) * mask to dres while it holds it in registers, and the apply pass reads dres in place of dy, dy2 and the sign
 * source (28.25 instead of 32.5 bytes per element; dres and dx are bit-identical to the pass that re-added the pair).  dres is
 * therefore written while dy, dy2 and x are still being read: it must not alias dy, dy2 or x (refused where the pointers are
 * equal; overlapping views are the caller's to avoid). */
int glf_bn_bwd(const float* dy, int lddy, const float* x, int ldx, const float* y, int ldy,
               const float* mean, const float* invstd, const float* gamma, const float* beta /* may be NULL with y */,
               float* dx, int lddx, float* dres, int lddres, float* dgamma, float* dbeta,
               int rows, int c, int relu, int training, double* workspace, float* amax_out, int packed_dx,
               const uint8_t* relu_mask /* glf_bn_apply's sign bytes: replaces y */, const float* dy2, int lddy2,
               double* fused_sums /* may be NULL.  Non-NULL (C <= 4096): 2 C doubles followed by 2 C floats, ALL ZERO on entry -- the
                                     backward then takes TWO launches: the reduction meets in one f64 atomic per column and workgroup
                                     there, the apply kernel finishes the sums itself (no finalize launch; `workspace` may be NULL).
                                     dgamma / dbeta agree with the three-launch form to fp32 rounding, not bit for bit. */,
               glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * Pooling / resampling / pointwise pieces of the path.
 * ------------------------------------------------------------------------------------- */
/* nn.MaxPool2d(3, stride 2, pad 1) on [N][H][W][C] -> [N][Ho][Wo][C]; idx (uint8, same shape as
 * y) records the winning tap (first maximum in scan order, as ATen).  idx is accessed one pixel's channel group at a time: 4-byte
 * aligned here, 8-byte aligned for the glf_s16_* pair (forward and backward refuse anything else). */
int glf_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s);
int glf_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int w, int c, glf_stream_t s);
/* ---------------------------------------------------------------------------------------
 * The streaming pieces of the U-Net baselines (ours.py:2385-2625; unet_ops.hip).  Channels-last, 16-byte accesses: every tensor
 * 16-byte aligned, C % 4 == 0 (fp32) / C % 8 == 0 (the glf_s16_* forms, bf16 tensors).  fp32 arithmetic, bf16 rounded once at
 * the store.  No atomics: results are bit-identical from call to call.  Arguments are checked before any launch: GLF_ERR_NULL,
 * GLF_ERR_UNSUPPORTED (Cout), GLF_ERR_BAD_SHAPE (extents, channel counts, strides, alignment), GLF_ERR_WORKSPACE.
 *
 * Conv2d(1, 64, 3, stride 1, padding 1) + bias (conv_block(1, 64).conv[0], ours.py:2389): x [N][H][W] fp32, w [Cout][9],
 * bias [Cout] or NULL, y [N][H][W][Cout] (fp32, or bf16 for glf_s16_*: the entry into the 16-bit domain).  Cout must be 64.
 * wgrad: dW [Cout][9] and db [Cout] (db may be NULL) from dy [N][H][W][Cout]; `partial` is a workspace of partial_floats >=
 * glf_conv3x3_c1_wgrad_workspace() floats (one [10][Cout] block of partial sums per 1024 pixels, folded in a fixed order).
 * There is no dgrad: the gradient with respect to the image is not on the path. */
int glf_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wdt, int cout, glf_stream_t s);
int glf_s16_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, void* y, int n, int h, int wdt, int cout, glf_stream_t s);
size_t glf_conv3x3_c1_wgrad_workspace(int n, int h, int wdt, int cout);
int glf_conv3x3_c1_wgrad(const float* x, const float* dy, float* dw, float* db, float* partial, size_t partial_floats,
                         int n, int h, int wdt, int cout, glf_stream_t s);
int glf_s16_conv3x3_c1_wgrad(const float* x, const void* dy, float* dw, float* db, float* partial, size_t partial_floats,
                             int n, int h, int wdt, int cout, glf_stream_t s);
/* nn.MaxPool2d(2, 2), floor mode: x [N][H][W][C] -> y [N][H/2][W/2][C], H, W >= 2; a trailing odd row / column is not read.
 * idx (uint8, shape of y; 4-byte aligned, 8-byte for glf_s16_*) records the winner 2 * ky + kx: the first maximum in row-major
 * window order (ATen's choice on ties), a NaN wins.  Backward writes EVERY element of dx [N][H][W][C] exactly once -- the gradient
 * at the winner, zero elsewhere and in the trailing row / column: dx needs no clearing. */
int glf_maxpool2x2s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s);
int glf_maxpool2x2s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int w, int c, glf_stream_t s);
int glf_s16_maxpool2x2s2_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, glf_stream_t s);
int glf_s16_maxpool2x2s2_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, glf_stream_t s);
/* nn.Upsample(scale_factor=2) (nearest): y [N][2H][2W][C], y[n][2i+a][2j+b][c] = x[n][i][j][c]; n, h, w, c describe x / dx.
 * Backward: dx = (dy00 + dy01) + (dy10 + dy11) of each 2x2 block, in that order. */
int glf_upsample2x_fwd(const float* x, float* y, int n, int h, int w, int c, glf_stream_t s);
int glf_upsample2x_bwd(const float* dy, float* dx, int n, int h, int w, int c, glf_stream_t s);
int glf_s16_upsample2x_fwd(const void* x, void* y, int n, int h, int w, int c, glf_stream_t s);
int glf_s16_upsample2x_bwd(const void* dy, void* dx, int n, int h, int w, int c, glf_stream_t s);
/* torch.cat((a, b), dim=1) on channels-last rows: y [rows][ca + cb] (contiguous), y[r][0..ca) = a[r * lda + .],
 * y[r][ca..ca+cb) = b[r * ldb + .] (row strides in elements, multiples of the access width: a source may be a column slice of a
 * wider buffer).  Backward: the two column slices of dy into the contiguous da [rows][ca] and db [rows][cb], one launch. */
int glf_concat2_fwd(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t rows, int ca, int cb, glf_stream_t s);
int glf_concat2_bwd(const float* dy, float* da, float* db, int64_t rows, int ca, int cb, glf_stream_t s);
int glf_s16_concat2_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t rows, int ca, int cb, glf_stream_t s);
int glf_s16_concat2_bwd(const void* dy, void* da, void* db, int64_t rows, int ca, int cb, glf_stream_t s);

/* AdaptiveAvgPool2d(1) (deeplabv3.py:126): x [N][P][C] -> y [N][C], and its backward. */
int glf_avgpool_fwd(const float* x, float* y, int n, int p, int c, glf_stream_t s);
/* broadcast rows: y[n][p][0..c) (row stride ldy) = x[n][0..c) -- the "bilinear from 1x1"
 * upsample of ASPPPooling (deeplabv3.py:135). */
int glf_bcast_rows_fwd(const float* x, float* y, int ldy, int n, int p, int c, glf_stream_t s);
/* dx[n][c] = scale * sum_p dy[n][p][c] (row stride lddy): backward of the broadcast (scale=1)
 * and, with scale = 1/p on a dense dy, nothing else; avgpool backward is bcast with scale 1/p. */
int glf_sum_rows_fwd(const float* dy, int lddy, float* dx, float scale, int n, int p, int c, glf_stream_t s);
int glf_bcast_rows_scaled(const float* x, float* y, int ldy, float scale, int n, int p, int c, glf_stream_t s);
/* y[r][:] += scale * x[r / p][:] for the n p rows of y (c and ldy multiples of 4, 16-byte aligned): glf_bcast_rows_scaled adding
 * into y instead of overwriting it. */
int glf_bcast_rows_add(const float* x, float* y, int ldy, float scale, int n, int p, int c, glf_stream_t s);
/* Stand-alone nn.ReLU (the fused paths apply it inside glf_bn_apply). */
int glf_relu_fwd(const float* x, float* y, int64_t numel, glf_stream_t s);
int glf_relu_bwd(const float* dy, const float* y, float* dx, int64_t numel, glf_stream_t s);
/* Dropout with a counter-based generator: keep iff hash(seed', element) >= p.  y = x*keep/(1-p).
 * seed' = seed + *step_counter * odd constant when step_counter (a DEVICE uint64, may be NULL) is given: a launch recorded in
 * a hipGraph replays with the same `seed` argument, the counter -- advanced once per training step by glf_counter_add, itself
 * part of the graph -- gives every replay its own masks (deeplabv3.py:159 Dropout(0.5), a fresh mask per forward). */
int glf_dropout(const float* x, float* y, int64_t numel, float p, uint64_t seed, const uint64_t* step_counter, glf_stream_t s);
/* Operand-maximum bookkeeping for tensors whose maximum follows from their sources' (no pass over the data):
 * *out = max(*out, scale * (sum ? |*a| + |*b| : max(|*a|, |*b|))); b may be NULL.  A dropout output is bounded by its input's
 * maximum / (1 - p), a sum of two tensors by the sum of their maxima, a stack of tensors by the largest.  Upper bounds are
 * what glf_gemm_params.amax_a / amax_b ask for. */
int glf_amax_combine(const float* a, const float* b, float scale, int sum, float* out, glf_stream_t s);
/* *counter += inc (a device uint64), stream-ordered. */
int glf_counter_add(uint64_t* counter, uint64_t inc, glf_stream_t s);
/* Local gate (a5, ours.py:1802-1816): a[r] = sigmoid(w * max_c sigmoid(cls[r][c]) * sigmoid(ctr[r])),
 * y[r][:] = f[r][:] * a[r].  argmax (int32 per row) is saved for backward. */
int glf_gate_fwd(const float* cls, int ncls, const float* ctr, const float* f, float* y, float* a,
                 int32_t* argmax, float weight, int rows, int c, glf_stream_t s);
/* df[r][:] = dy[r][:]*a[r]; dcls/dctr from da[r] = sum_c dy[r][c]*f[r][c]. */
int glf_gate_bwd(const float* dy, const float* f, const float* cls, int ncls, const float* ctr,
                 const float* a, const int32_t* argmax, float weight,
                 float* df, float* dcls, float* dctr, int rows, int c, glf_stream_t s);
/* Stack / slice views for the fusion block (ours.py:1819-1834): frame-strided row copies.
 * dst[n][.] (frame stride dst_fs) = src[n][.] (frame stride src_fs), `inner` floats per frame. */
int glf_copy_frames(const float* src, int64_t src_fs, float* dst, int64_t dst_fs,
                    int n, int64_t inner, glf_stream_t s);
/* glf_copy_frames that ALSO writes the packed pre-split image (glf_split_f16_packed's format, same layout as dst) of what it
 * copies, scaled by *amax -- a device float that already holds an upper bound of max|src| (e.g. glf_amax_combine of the sources'
 * maxima).  ours.py:1819-1820: the stacked fusion-block input is read once, by the copy, instead of again by a split pass. */
int glf_copy_frames_split(const float* src, int64_t src_fs, float* dst, float* dst_packed, int64_t dst_fs, int n, int64_t inner,
                          const float* amax, glf_stream_t s);
/* dst = a + b with independent frame strides (f4_fusion = f4_global_fusion + f4_local_fusion). */
int glf_add_frames(const float* a, int64_t a_fs, const float* b, int64_t b_fs, float* dst, int64_t dst_fs,
                   int n, int64_t inner, glf_stream_t s);
/* out = sum of k (<= 8) same-sized tensors given as a HOST array of device pointers: the gradient fan-in of a
 * tensor that feeds several branches (f4 -> classifier / centerness / gate / fusion; ASPP input -> 5 branches). */
int glf_add_n(const float* const* inputs, int k, float* out, int64_t numel, glf_stream_t s);
/* ---------------------------------------------------------------------------------------
 * The view mix of the classical fusion baselines (early_fusion, late_fusion; ours.py:2251-2383; view_mix.hip): V per-view 1x1
 * convolutions over the channel concatenation of all V views, in one streaming pass that reads every view once and writes every
 * view's output once:
 *     y_v[r][o] = b_v[o] + sum_u sum_i W_v[o][u c + i] x_u[r][i]        (u c + i: the column order of torch.cat(dim=1))
 * xs / ys / dys / dxs are HOST arrays of V device pointers (as glf_add_n's inputs), each a contiguous, 16-byte aligned fp32
 * [rows][c] tensor; w is the V weights [c][V c] stacked by rows into one [V c][V c] matrix, bias the V biases stacked into [V c]
 * (NULL: none).  All data is fp32 under every precision.  Limits: c <= 8, V <= 8, V c <= 40; anything else is
 * GLF_ERR_UNSUPPORTED.  A null pointer, a misaligned tensor or a non-positive extent is GLF_ERR_BAD_SHAPE.  A thread moves the
 * smallest run of rows whose bytes are a multiple of 16 (4 / gcd(c, 4) rows) with 16-byte accesses; the rows left over take a
 * scalar path; every output element is written exactly once.
 * dgrad: dx_u[r][i] = sum_v sum_o W_v[o][u c + i] dy_v[r][o] -- the same kernel on the transposed matrix, without the bias.
 * wgrad: dW[v c + o][u c + i] = sum_r dy_v[r][o] x_u[r][i] (dw [V c][V c]) and db[v c + o] = sum_r dy_v[r][o] (db [V c], may be
 * NULL).  No atomics: each workgroup reduces 1024 consecutive rows into a block of V c (V c + 1) partial sums in `workspace`
 * (caller-owned, uninitialised, 16-byte aligned, `bytes` >= glf_view_mix_wgrad_workspace() BYTES; a smaller one is
 * GLF_ERR_WORKSPACE), and a finalize folds the blocks in float64 in a fixed order: bit-identical from call to call. */
int glf_view_mix_fwd(const float* const* xs, const float* w, const float* bias, float* const* ys, int64_t rows, int v, int c, glf_stream_t s);
int glf_view_mix_dgrad(const float* const* dys, const float* w, float* const* dxs, int64_t rows, int v, int c, glf_stream_t s);
size_t glf_view_mix_wgrad_workspace(int64_t rows, int v, int c);
int glf_view_mix_wgrad(const float* const* xs, const float* const* dys, float* dw, float* db, void* workspace, size_t bytes,
                       int64_t rows, int v, int c, glf_stream_t s);
/* W_z tail of TPAVIModule (ours.py:908-915): z = LayerNorm_C( BN(w) + x ) with the BN already
 * folded into per-channel (bn_mean, bn_invstd, gamma, beta).  Saves row mean / rstd.  amax_out (may be NULL): as in
 * glf_bn_apply, receives max(*amax_out, max|z|). */
int glf_bn_res_ln_fwd(const float* w, const float* x, const float* bn_mean, const float* bn_invstd,
                      const float* bn_gamma, const float* bn_beta, const float* ln_gamma,
                      const float* ln_beta, float ln_eps, float* z, float* row_mean, float* row_rstd,
                      int rows, int c, float* amax_out, glf_stream_t s);
/* LayerNorm backward: du (gradient w.r.t. u = BN(w)+x), dgamma/dbeta of the LayerNorm.
 * workspace: glf_bn_workspace(rows, c) doubles. */
int glf_bn_res_ln_bwd(const float* dz, const float* w, const float* x, const float* bn_mean,
                      const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                      const float* ln_gamma, const float* row_mean, const float* row_rstd,
                      float* du, float* dln_gamma, float* dln_beta, int rows, int c,
                      double* workspace, glf_stream_t s);
/* glf_bn_res_ln_bwd and the reduction half of the BatchNorm backward that follows it (glf_bn_bwd on dy = du, x = w, no ReLU)
 * in ONE walk over dz, w and x: du (bit-identical to glf_bn_res_ln_bwd's), dln_gamma / dln_beta, and from du while it is in
 * registers dbn_beta = sum_r du, dbn_gamma = sum_r du what (what = (w - mean) invstd), both also kept as floats in bn_sums
 * [2 c] for the apply half, and -- amax_out non-NULL: a zeroed device float -- the upper bound of max |dx| of that BatchNorm
 * backward (training as in glf_bn_bwd) raised into *amax_out, as glf_bn_bwd's packed_dx = 2 does.  Finish with
 * glf_bn_bwd(du, ..., packed_dx = 3 (packed dx, same amax_out) or 4 (fp32 dx), fused_sums = bn_sums).
 * Two launches (the walk, one finalize); fixed-order sums, no atomics on them: equal inputs give equal bits.
 * C <= 2048 as glf_bn_res_ln_bwd; du must not alias dz, w or x.  workspace: glf_bn_workspace(rows, c) doubles. */
int glf_bn_res_ln_bwd_sums(const float* dz, const float* w, const float* x, const float* bn_mean,
                           const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                           const float* ln_gamma, const float* row_mean, const float* row_rstd,
                           float* du, float* dln_gamma, float* dln_beta, float* dbn_gamma, float* dbn_beta,
                           float* bn_sums, float* amax_out /* may be NULL */, int rows, int c, int training,
                           double* workspace, glf_stream_t s);
/* Row softmax in place over `cols` (TPAVI 'embedded' mode, ours.py:896-897) and its backward
 * ds = p * (dp - sum(dp*p)). */
int glf_softmax_rows(float* x, int64_t rows, int cols, glf_stream_t s);
int glf_softmax_rows_bwd(const float* p, float* dp_inout, int64_t rows, int cols, glf_stream_t s);
/* The same over rows of stride ld >= cols; the padding columns [cols, ld) are written as zeros (zero probabilities / zero score
 * gradients: the matrices then serve as contraction operands with K = ld). */
int glf_softmax_rows_ld(float* x, int64_t rows, int cols, int ld, glf_stream_t s);
int glf_softmax_rows_bwd_ld(const float* p, float* dp_inout, int64_t rows, int cols, int ld, glf_stream_t s);
/* F.interpolate(mode='bilinear', align_corners=False) (ours.py:1838,1841): x [N][h][w][C]
 * channels-last -> y [N][C][H][W] (NCHW, what the caller's loss consumes), and its adjoint. */
int glf_bilinear_up_fwd(const float* x, float* y, int n, int h, int w, int c, int ho, int wo, glf_stream_t s);
int glf_bilinear_up_bwd(const float* dy, float* dx, int n, int h, int w, int c, int ho, int wo, glf_stream_t s);
/* nn.BCEWithLogitsLoss(reduction='sum') (main.py:87,209-211): loss_out (double[1], zeroed by the
 * call) and, when dx != NULL, dx = (sigmoid(x) - t) * grad_scale * (*grad_scale_dev), the latter a
 * device scalar (autograd's upstream gradient) that may be NULL. */
int glf_bce_logits_sum(const float* x, const float* t, double* loss_out, float* dx, float grad_scale,
                       const float* grad_scale_dev, int64_t numel, glf_stream_t s);
/* Trainer._calculate_overlap_metrics (main.py:800-815) on pred = sigmoid(x) > 0.5:
 * counts[4] = {tp, fp, fn, tn} as int64 (zeroed by the call). */
int glf_overlap_counts(const float* logits, const float* target, int64_t* counts, int64_t numel, glf_stream_t s);
/* Cross pseudo supervision between two logit maps (the loss of Global_and_Local_CPS, no reference counterpart): with
 * on(x) = sigmoid(x) > 0.5 by the predicate glf_overlap_counts counts with,
 * loss_out[0] = sum_i bce(a_i, on(b_i)) + sum_i bce(b_i, on(a_i)) (double[1], zeroed by the call; bce as glf_bce_logits_sum).
 * stats (may be NULL): int64[4], zeroed by the call, counts of (on(a), on(b)) = {11, 10, 01, 00} -- what
 * glf_overlap_counts(a, on(b)) returns.  da and db: both NULL (forward) or both given; da = (sigmoid(a) - on(b)) * g,
 * db = (sigmoid(b) - on(a)) * g with g = grad_scale * (*grad_scale_dev), the latter a device scalar that may be NULL (the labels
 * are constants).  One launch; every input element is read once.  da / db must not alias a, b or each other. */
int glf_cps_bce_sum(const float* a, const float* b, double* loss_out, int64_t* stats, float* da, float* db, float grad_scale,
                    const float* grad_scale_dev, int64_t numel, glf_stream_t s);
/* bias gradient: db[c] = sum_r dy[r][c]; workspace glf_bn_workspace(rows, c) doubles. */
int glf_colsum(const float* dy, int lddy, float* db, int rows, int c, double* workspace, glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam as main.py:162-165 builds it (L2 weight decay folded into the
 * gradient, no amsgrad), every parameter of one step count in ONE launch.  `table` is a DEVICE array of
 * n_rows x 5 int64 { param ptr, grad ptr, exp_avg ptr, exp_avg_sq ptr, n elements }, one row per chunk of a
 * parameter; `step` = the parameters' step count t, counted from 1 (torch keeps one per parameter; parameters
 * with different counts go into separate calls).  The bias corrections, 1 - beta and lr / (1 - beta1^t) are
 * formed in double on the host as torch does.
 * Updates param, exp_avg and exp_avg_sq in place with the operation order of torch.optim._functional.adam.
 * ------------------------------------------------------------------------------------- */
int glf_adam_step(const int64_t* table, int n_rows, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int64_t step, glf_stream_t s);
/* torch.optim.SGD (main.py:159-161; momentum, dampening and nesterov as torch defines them) over a table of the same
 * n_rows x 5 int64 format, ONE launch: column 2 is the momentum buffer, column 3 is ignored (may be 0).  In torch's
 * operation order, every operation individually rounded:
 *   d = grad;  if weight_decay != 0: d += weight_decay * param
 *   if momentum != 0: buf = first ? d : buf * momentum + (1 - dampening) * d;  d = nesterov ? d + momentum * buf : buf
 *   param += (-lr) * d
 * first != 0: the parameters of this call have no momentum buffer yet (the buffer is written, never read); parameters
 * with and without one go into separate calls.  With momentum == 0 the buffer column is neither read nor written and
 * may be 0 -- then and only then.  1 - dampening and -lr are formed in double on the host as torch does.
 * Checked before any HIP runtime call: GLF_ERR_NULL (table), GLF_ERR_BAD_SHAPE (n_rows < 1, table not 8-byte aligned,
 * momentum < 0, nesterov with momentum <= 0 or dampening != 0). */
int glf_sgd_step(const int64_t* table, int n_rows, double lr, double momentum, double dampening, double weight_decay,
                 int nesterov, int first, glf_stream_t s);
/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) with a non-finite guard, on the device
 * throughout: nothing here reads a value back or blocks the host.  All tables have the format above, the gradient in column 1.
 * glf_grad_sumsq: partials[row] (DEVICE double[n_rows]) = sum of grad^2 over the row, accumulated in double in a fixed order,
 * no atomics: the same bits on every run.  Only column 1 and column 4 (n) of the table are read.
 * glf_grad_clip_coef: adds partials[0..n) in index order in double and writes record (DEVICE float[4]):
 *   record[0] = norm = (float)sqrt(sum)
 *   record[1] = coef = min(1.0f, (float)max_norm / (norm + 1e-6f)) in float, every operation individually rounded (what
 *               clip_grad_norm_ evaluates on a float32 norm); 0.0f when the sum is not finite
 *   record[2] = ok = 1.0f when the sum is finite, 0.0f otherwise;  record[3] = 0.0f
 * and adds 1 to *skipped (DEVICE int64) when the sum is not finite.  max_norm = +inf is legal: coef is then 1 and only the
 * guard is active.  Partials of several glf_grad_sumsq calls may be laid end to end into one glf_grad_clip_coef.
 * glf_adam_step_clipped / glf_sgd_step_clipped: their unclipped twins with every gradient element replaced by
 * grad * record[1] (individually rounded, before the weight decay; the stored gradient is NOT rewritten); with
 * record[2] == 0 nothing is read or written beyond the record -- not param, exp_avg, exp_avg_sq or the momentum buffer, the
 * `first` call that was to write a new buffer included.  Because the host cannot know that such a call was skipped,
 * glf_sgd_step_clipped also takes a row whose momentum buffer still begins with the bit pattern 0x7fc0dead (a quiet NaN no
 * arithmetic produces; the caller fills a new buffer with it) as `first`, whatever the argument says.
 * glf_grad_scale: grad *= record[1] in place over the table; writes nothing when record[2] == 0 or record[1] == 1.
 * Checked before any HIP runtime call: GLF_ERR_NULL (any pointer), then GLF_ERR_BAD_SHAPE (n_rows < 1, n < 1, table or
 * partials not 8-byte aligned, max_norm negative or NaN, and what the unclipped twin refuses). */
int glf_grad_sumsq(const int64_t* table, int n_rows, double* partials, glf_stream_t s);
int glf_grad_clip_coef(const double* partials, int n, double max_norm, float* record, int64_t* skipped, glf_stream_t s);
int glf_adam_step_clipped(const int64_t* table, int n_rows, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int64_t step, const float* record, glf_stream_t s);
int glf_sgd_step_clipped(const int64_t* table, int n_rows, double lr, double momentum, double dampening, double weight_decay,
                         int nesterov, int first, const float* record, glf_stream_t s);
int glf_grad_scale(const int64_t* table, int n_rows, const float* record, glf_stream_t s);

/* ---------------------------------------------------------------------------------------
 * Temporal cycle-consistency loss: Trainer.seg_cycle and Trainer.dense_seg_cycle
 * (main.py:650-718, 720-798) on the pooled fusion features feat [T][F] (main.py:226-231: T = 40,
 * target_region 16, cyc_off 2, chunk_size 3, temperature 10).  *loss_out = weight * sum over the start frames
 * start0, start0 + stride, ... (n_starts of them) of the mean BCE-with-logits; dfeat [T][F] (may be NULL)
 * receives d loss / d feat.  seg_cycle: n_starts = 1, weight = 1, start0 = the frame the reference draws with
 * np.random.choice (an explicit input here).  dense_seg_cycle: start0 = 0, stride = 1 (is_overlap) or
 * chunk_size, weight = 1 / (target_region - chunk_size - cyc_off + 1); soft_label as main.py:790-791.
 * ------------------------------------------------------------------------------------- */
int glf_seg_cycle(const float* feat, int T, int F, int target_region, int cyc_off, int chunk_size, float temperature,
                  int start0, int n_starts, int stride, float weight, int soft_label, float* loss_out, float* dfeat,
                  glf_stream_t s);
/* out = a*x + b*y (out may alias x or y): the background branch f4 * (1 - gate) = f4 - f4 * gate of
 * Foreground_and_Background (ours.py:2966) and its gradient. */
int glf_axpby(const float* x, const float* y, float* out, float a, float b, int64_t numel, glf_stream_t s);
/* y = x * scale * (*scale_dev) (scale_dev: device scalar, may be NULL): a saved gradient times autograd's
 * upstream gradient. */
int glf_scale(const float* x, float* y, int64_t numel, float scale, const float* scale_dev, glf_stream_t s);
/* ---------------------------------------------------------------------------------------
 * Data path and evaluation harness.
 * glf_prepare_frames: one raw volume [H0][W0][T] (T fastest; img = grey levels, lab = class ids 0..4, either may be
 * NULL with its output) -> frames out_img [T][1][out_h][out_w] = img / img_div (255 for labelled, 1 for unlabelled clips,
 * loader.py:325-327) and part masks out_mask [T][5][out_h][out_w]: nearest-neighbour resize to resize x resize
 * (Resized(mode='nearest'), loader.py:478, 488), crop window at (off_y, off_x) (RandSpatialCropd / CenterSpatialCropd,
 * loader.py:480, 489: centre = (resize - out) / 2), class id k = 1..4 -> channel class_to_channel[k-1] (HOST array of 4
 * ints, -1 = dropped; the per-view tables of loader.py:298-316 + mask_to_allclass, loader.py:358-414).
 * glf_overlap_counts_nchw: counts[c][4] = (tp, fp, fn, tn) of sigmoid(logits) > 0.5 vs target per class channel of
 * [n][c][hw] tensors (the per-part Dice of main.py:537-543); counts is zeroed by the call.
 * ------------------------------------------------------------------------------------- */
int glf_prepare_frames(const float* img, const float* lab, float* out_img, float* out_mask, int H0, int W0, int T,
                       int resize, int out_h, int out_w, int off_y, int off_x, const int* class_to_channel, float img_div,
                       glf_stream_t s);
int glf_overlap_counts_nchw(const float* logits, const float* target, int64_t* counts, int n, int c, int64_t hw, glf_stream_t s);
/* ---------------------------------------------------------------------------------------
 * Visual mode (Trainer.test_visualize, main.py:546-648): predictions as label maps, pictures and volumes.
 * A channel is ON when sigmoid(logit) > 0.5, by the device predicate glf_overlap_counts_nchw counts with: logit 0.0, -0.0,
 * -inf and NaN are off, +inf is on.
 * glf_render_labels: logits [n][c][h][w] (c = 1..8) -> labels [n][h][w] (uint8) = argmax over [0.5, on_0, .., on_{c-1}], the
 * first maximum winning (main.py:606-612): 0 when no channel is on, else 1 + the lowest channel that is on; and
 * rgba [n][h][w][4] (uint8, 4-byte aligned, one 32-bit store per pixel) = palette[label], palette = (c + 1) x 4 HOST bytes
 * (r, g, b, a per label).  Either output may be NULL, not both; palette may be NULL when rgba is.
 * frames [n][1][h][w] (fp32 in [0, 1], may be NULL) adds the overlay, which the reference does not have: with the grey level
 * G = clamp((int)(v * 255.0f + 0.5f), 0, 255) (product and sum individually rounded; NaN -> 0) every colour byte becomes
 * (alpha * colour + (255 - alpha) * G + 127) / 255 in integer arithmetic where label != 0 and G where label == 0; the alpha
 * byte becomes 255.  alpha = 0..255 (checked with or without frames).
 * glf_restore_labels: the inverse geometry of glf_prepare_frames.  logits [T][c][out_h][out_w] -> volume [H0][W0][T] (uint8,
 * T fastest: the order of the NIfTI volume the clip was cut from).  Source pixel (y0, x0) looks up the resized pixel
 * yr = min(floor(y0 * ((float)resize / (float)H0)), resize - 1), xr likewise (ATen's legacy 'nearest' from resize x resize up
 * or down to H0 x W0); outside the crop window [off_y, off_y + out_h) x [off_x, off_x + out_w) the voxel is 0; inside it is
 * channel_to_class[ch] of the channel ch with the largest logit among those that are on AND have channel_to_class[ch] != 0
 * (ties: the lowest channel), 0 when there is none.  channel_to_class: c HOST ints 0..255, 0 = this view does not show that
 * channel.
 * Both check their arguments before any HIP runtime call, in this order: GLF_ERR_NULL (logits, both outputs / volume, palette /
 * table; a null pointer wins over every other error), then GLF_ERR_BAD_SHAPE (n, c, h, w, T, H0, W0, resize < 1, c > 8, alpha or a
 * table entry outside 0..255, a crop window that leaves the resized image, rgba not 4-byte aligned).
 * ------------------------------------------------------------------------------------- */
int glf_render_labels(const float* logits, const float* frames, uint8_t* labels, uint8_t* rgba, int n, int c, int h, int w,
                      const uint8_t* palette, int alpha, glf_stream_t s);
int glf_restore_labels(const float* logits, uint8_t* volume, int T, int c, int out_h, int out_w, int H0, int W0, int resize,
                       int off_y, int off_x, const int* channel_to_class, glf_stream_t s);
/* ---------------------------------------------------------------------------------------
 * Training data path: label-frame sums of a resident volume, and one batch of frames from many volumes in one call.
 * Volumes are [H0][W0][T] (T fastest) stored as float32 (GLF_SRC_F32) or uint8 (GLF_SRC_U8); a byte converts exactly, so
 * both storages give the same output bits.
 * glf_frame_label_sums: sums[t] = sum over (y, x) of (int)lab[y][x][t], T int64 on the device: the quantity input_select
 * compares with 100 (loader.py:429-458, masks.sum(dim=(0, 1))), exact for class-id volumes.  Any T >= 1.  The call writes
 * all of sums (no pre-zeroing by the caller).  Reads run along the volume's memory order; a block sums its share of each
 * frame in registers and LDS and adds one value per frame.  GLF_ERR_NULL, GLF_ERR_BAD_SHAPE (H0, W0, T < 1),
 * GLF_ERR_UNSUPPORTED (dtype), all before any HIP runtime call.
 * glf_prepare_batch: srcs = n HOST descriptors; descriptor i yields nt consecutive output frames, frames t0 .. t0 + nt - 1 of
 * its volume, by exactly glf_prepare_frames' arithmetic (fp32 nearest scale, true division by img_div, (int)lab -> channel):
 * out_img [sum nt][1][out_h][out_w], out_mask [sum nt][5][out_h][out_w] (NULL for image-only batches).  img == NULL: the
 * source's frames are zeros in both outputs (a patient without this view, loader.py:267-282) and only nt is read; lab == NULL:
 * its mask frames are zeros.  resize == H0 == W0 == out_h == out_w, offsets 0, img_div 1 is the identity (raw video clips).
 * The descriptors reach the device as kernel arguments, 32 per launch: no allocation, copy or synchronisation per call.
 * Checked before any HIP runtime call: GLF_ERR_NULL (srcs, out_img), then per source GLF_ERR_BAD_SHAPE (n < 1, nt < 1,
 * sizes < 1, t0 < 0, t0 + nt > T, img_div 0, a crop window that leaves the resized image, a label pointer with a
 * class_to_channel entry outside [-1, 4]) and GLF_ERR_UNSUPPORTED (a dtype that is neither GLF_SRC_F32 nor GLF_SRC_U8).
 * ------------------------------------------------------------------------------------- */
enum { GLF_SRC_F32 = 0, GLF_SRC_U8 = 1 };
typedef struct {
    const void* img;              /* device volume, or NULL: zeros */
    const void* lab;              /* device volume of class ids, or NULL: no masks from this source */
    int32_t img_dtype, lab_dtype; /* GLF_SRC_F32 / GLF_SRC_U8 */
    int32_t H0, W0, T;
    int32_t t0, nt;               /* first frame and frame count */
    int32_t resize, off_y, off_x;
    int32_t class_to_channel[4];  /* channel of class 1..4, -1 = dropped (read only with lab) */
    float img_div;
    int32_t reserved;
} glf_frame_src;
int glf_frame_label_sums(const void* lab, int dtype, int H0, int W0, int T, int64_t* sums, glf_stream_t s);
int glf_prepare_batch(const glf_frame_src* srcs, int n, float* out_img, float* out_mask, int out_h, int out_w, glf_stream_t s);
/* ---------------------------------------------------------------------------------------
 * Contour metrics (no reference counterpart; main.py:800-815 counts overlap only): what Hausdorff distance, its percentile
 * form and the average symmetric surface distance are made of, per (frame, class channel, direction), in pixels.
 * logits, target: [n][c][h][w] fp32.  A prediction pixel is ON by glf_overlap_counts_nchw's device predicate
 * (sigmoid(logit) > 0.5: logit 0.0, -0.0, -inf and NaN are off, +inf is on), a target pixel when target != 0.
 * The CONTOUR of a mask is its on pixels with at least one 4-neighbour (up, down, left, right) that is off or outside the
 * image (= M xor binary_erosion(M) with the cross element and border value 0).  Direction 0 gives every contour pixel p of the
 * prediction d2(p) = min over contour pixels q of the target of (py - qy)^2 + (px - qx)^2; direction 1 is target -> prediction.
 * stats [n][c][2][4] int64 = (count, max_d2, d2_lo, d2_hi): count = contour pixels of the direction's source mask; d2_lo, d2_hi =
 * the ascending-sorted d2 at ranks lo = (pct * (count - 1)) / 100 and hi = lo + ((pct * (count - 1)) % 100 != 0).  All exact.
 * sums [n][c][2] double = sum of sqrt((double)d2) over the source contour, added in a fixed order: bitwise reproducible.
 * When either contour of a pair is empty both directions report their own count, max_d2 = d2_lo = d2_hi = -1 and sum 0.0.
 * Every element of stats and sums is written by the call (no pre-zeroing by the caller).
 * One launch, one workgroup per (frame, channel, direction), all intermediate state in LDS (bitmaps, a separable integer
 * distance transform by column strips, two histogram passes for the ranks): no workspace, allocation, synchronisation or state.
 * h, w <= GLF_CONTOUR_MAX_DIM (so that d2 < 2^17 and a plane's bitmaps fit LDS); the work per plane is O(h * w * h) at most,
 * whatever the masks are.
 * Checked before any HIP runtime call, in this order: GLF_ERR_NULL (any of the four pointers; wins over everything), then
 * GLF_ERR_BAD_SHAPE (n, c, h, w < 1, pct outside 0..100, 2 * n * c > 2^31 - 1), then GLF_ERR_UNSUPPORTED (h or w above
 * GLF_CONTOUR_MAX_DIM).
 * ------------------------------------------------------------------------------------- */
#define GLF_CONTOUR_MAX_DIM 256
int glf_contour_distances(const float* logits, const float* target, int64_t* stats, double* sums, int n, int c, int h, int w,
                          int pct, glf_stream_t s);
/* Zero `bytes` bytes at p on the stream (accumulation targets: atomically summed gradients, column statistics, maxima). */
int glf_zero(void* p, int64_t bytes, glf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* GLFUSION_H */

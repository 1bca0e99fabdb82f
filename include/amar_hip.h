/*
 * amar_hip.h — C-ABI of the MI355X (gfx950) GNN-propagation + hybrid-scoring hot path.
 *
 * The reference (swapUniba/Deep_CBRS_Amar_Renaissance) is pure Python on TensorFlow/Keras/
 * Spektral and has no FFI of its own; each entry point below replaces the framework call the
 * reference makes at the cited file:line (paths relative to the reference root).  A maintainer
 * binds these with ctypes — see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; nothing here allocates, frees or
 *     synchronises; work is enqueued on `stream` (a hipStream_t passed as void*, NULL = default)
 *   - matrices are row-major fp32 with an explicit leading dimension (in elements), so a layer
 *     can write straight into its column slice of the [N, d(L+1)] concatenation buffer
 *     (ReductionLayer 'concatenation', src/layers/reduction.py:15-16)
 *   - CSR is canonical: int32 rowptr[n_rows+1], int32 colidx[nnz] ascending within a row
 *   - return value: 0 = ok, <0 = AMAR_E* below; never throws, never aborts
 *   - re-entrant for distinct streams; no global mutable state
 */
#ifndef AMAR_HIP_H
#define AMAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMAR_OK            0
#define AMAR_EINVAL       -1   /* bad argument (null pointer, negative size, misaligned ld)   */
#define AMAR_EUNSUPPORTED -2   /* shape outside what the kernels are built for                */
#define AMAR_ELAUNCH      -3   /* HIP reported an error at launch (see amar_last_hip_error)   */

#define AMAR_ACT_NONE     0
#define AMAR_ACT_RELU     1
#define AMAR_ACT_SIGMOID  2
#define AMAR_DENSE_WT 0x100    /* amar_dense_f32, OR-ed into `act`: W is given transposed ([N, K] row-major), for dX = dZ . W^T */

/* flags of amar_spmm_csr_f32 */
#define AMAR_SPMM_BIAS      1u   /* y += bias[F]                                              */
#define AMAR_SPMM_RELU      2u   /* y = max(y, 0) after bias                                  */
#define AMAR_SPMM_ACCUM     4u   /* acc_out = acc_in + y (LightGCN running layer sum)         */
#define AMAR_SPMM_ACCUM_DIV 8u   /* ... and acc_out /= acc_div (ReductionLayer 'mean')        */
#define AMAR_SPMM_SCALE_NEXT 16u /* amar_spmm_xs_f32, value-free image: Hnext[i] *= row_scale[i] */
#define AMAR_SPMM_SAGE_TAIL 32u  /* amar_spmm_lt_f32 on GraphSAGE's mean-aggregate image (diag = self loop, row_scale = 1/count, X un-scaled):
                                    Y[i] = relu(l2_normalize([X_i || mean_i] . Wnext + bias)), Wnext [2F, F] (Cn = F), the tail of
                                    spektral GraphSageConv (src/models/gnn.py:354-361) in the same launch; Hnext (optional, ld ldhn) receives
                                    a second copy of Y: a dense table for the next layer's gathers when Y is a concat slice */
#define AMAR_SPMM_LT_NOPAIRS 64u /* amar_spmm_lt_f32: the image holds no implicit pairs — every repeat of a virtual row inside a step is
                                    flagged (utilities/lds_tiled.py, pairs=False: the default for F >= 16) — so the kernel may skip
                                    the pair logic of a step; an image WITH implicit pairs must not carry this flag */

typedef void *amar_stream_t;

int amar_version(void);
const char *amar_error_string(int code);
int amar_last_hip_error(void);          /* last hipError_t seen by this thread, 0 if none */

/* ---- propagation --------------------------------------------------------------------------
 * Y[n_rows, F] = A . X   (+ bias, ReLU, running sum)        fp32, CSR, F in {4, 8, 16, 32, 64};
 * any other multiple of 4 runs as column chunks of those widths (24 = 16 + 8), same results column by column
 * Replaces spektral.layers.ops.modal_dot -> tf.sparse.sparse_dense_matmul at
 * src/layers/lightgcn_conv.py:51-54 and inside GCNConv.call (built at src/models/gnn.py:289-295,
 * invoked at src/models/gnn.py:78).  vals == NULL means an all-ones (binary) matrix.
 * ldx, ldy (and ld_acc) must be multiples of 4 and the bases 16-byte aligned.
 * Y may be NULL when only the running sum is wanted (last LightGCN layer).
 */
int amar_spmm_csr_f32(const int32_t *rowptr, const int32_t *colidx, const float *vals,
                      const float *X, int64_t ldx, float *Y, int64_t ldy,
                      int32_t n_rows, int32_t F, uint32_t flags, const float *bias,
                      const float *acc_in, int64_t ld_acc_in, float *acc_out, int64_t ld_acc_out,
                      float acc_div, amar_stream_t stream);

/* The same product on the sliced-jagged (SJ) image of A, for graphs whose node table exceeds the
 * per-XCD L2 (built by utilities/math.py:SlicedJagged.from_csr; any producer may build it):
 *   rows are taken 64 at a time (wave w = rows [64w, 64w+64), lane = row & 63);
 *   columns are cut into n_slices slices of 2^cbits columns (slice of col = col >> cbits);
 *   for w = 0.., for slice = 0..n_slices-1, for j = 0,1,..: the j-th non-zero (ascending column) of
 *   every row of w that has more than j non-zeros in that slice, in ascending lane order, is the
 *   next entry:  entries[e] = (int32 global column, fp32 value bits)               8 bytes per non-zero
 *   counts[(w * n_slices + slice) * 64 + lane] = non-zeros of that row in that slice (int16)
 *   wave_start[w] = index of wave w's first entry; wave_start[n_waves] = nnz.
 * flags / bias / acc_* as amar_spmm_csr_f32 (AMAR_SPMM_RELU with AMAR_SPMM_BIAS gives the GCN
 * epilogue); Wnext != NULL additionally writes Hnext[i, 0:Cn] = Y[i, :] . Wnext (Cn <= 64) like
 * amar_gcn_layer_f32.  Each row is summed in ascending column order by a single lane.
 */
int amar_spmm_sj_f32(const int32_t *entries, const int16_t *counts, const int32_t *wave_start, int32_t n_slices,
                     const float *X, int64_t ldx, float *Y, int64_t ldy,
                     int32_t n_rows, int32_t F, uint32_t flags, const float *bias,
                     const float *acc_in, int64_t ld_acc_in, float *acc_out, int64_t ld_acc_out, float acc_div,
                     const float *Wnext, int32_t Cn, float *Hnext, int64_t ldhn, amar_stream_t stream);

/* The same product on the XCD-sliced (XS) image of a square A — the form used when the node table does
 * not fit one 4 MB per-XCD L2 (utilities/math.py:XcdSliced.from_csr builds it; any producer may):
 *   diag[n]                  the diagonal of A (duplicates summed)
 *   the off-diagonal non-zeros sorted by (slice, row, column), columns cut into n_slices contiguous slices of
 *   equal non-zero count:  colidx (= (row & 63) << 26 | column; n <= 2^26) / vals, and
 *   rowptr[k * n + r] = first entry of (slice k, row r)  (int32 [n_slices*n + 1])
 * Two launches: per-slice partial rows -> partials[n_slices, n, F] (caller-provided scratch), workgroup b touching
 * slice b % n_slices only (XCD <-> L2 affinity under round-robin dispatch); then
 *   Y[i] = epilogue( diag[i] . X[i] + sum_k partials[k][i] )   in slice order, epilogue as amar_spmm_sj_f32.
 * X has n_cols rows (the columns of A).  Xself[i] is row i's own feature row for the diag term: NULL means X (square A,
 * the rows index the same table); a row block of a larger matrix (multi-GPU node-range partition) passes X + offset.
 *
 * Value-free form (vals == NULL, row_scale != NULL) for A = S (C) S with S = diag(row_scale) and C a matrix of small
 * non-negative integers — exactly gcn_filter's D^-1/2 (A + I) D^-1/2 (Spektral, called at src/models/gnn.py:283,381):
 * every entry weighs 1 (an entry of C equal to c is stored c times), diag[i] = C_ii, X must already hold S . X
 * (row i scaled by row_scale[i]) and Y[i] = epilogue( row_scale[i] * (diag[i] . X[i] + sum_k partials[k][i]) ).
 * This halves the read-once index stream.  AMAR_SPMM_SCALE_NEXT also scales Hnext[i] by row_scale[i], so that a
 * chain of GCN layers stays in the pre-scaled form.  With vals != NULL row_scale must be NULL.
 */
int amar_spmm_xs_f32(const float *diag, const int32_t *rowptr, const int32_t *colidx, const float *vals, const float *row_scale,
                     int32_t n_slices, const float *X, int64_t ldx, int32_t n_cols, const float *Xself, float *partials, float *Y, int64_t ldy,
                     int32_t n_rows, int32_t F, uint32_t flags, const float *bias,
                     const float *acc_in, int64_t ld_acc_in, float *acc_out, int64_t ld_acc_out, float acc_div,
                     const float *Wnext, int32_t Cn, float *Hnext, int64_t ldhn, amar_stream_t stream);

/* The same value-free product on the LDS-tiled (LT) image (utilities/lds_tiled.py:LdsTiled builds it; any producer
 * may) — the form the 2-layer basic-gnn propagation (src/models/gnn.py:74-84 with GCNConv / LightGCNConv layers,
 * gnn.py:289-295, src/layers/lightgcn_conv.py:51-54) runs on when the node table exceeds the per-XCD L2s:
 * ONE launch, one 1024-thread workgroup per tile of consecutive rows, the tile's fp32 sums in 128 KB of LDS, the
 * tile's entries walked in column order so that neighbouring entries share L1 lines.  W = 16 waves,
 * RW = 128 KB / (4.F.W) LDS rows per wave, cbits = 31 - log2(RW) (n_cols <= 2^cbits, else AMAR_EUNSUPPORTED).
 *   tile_row0[n_tiles+1]   row range of every tile
 *   vstart[n_rows+1], vcount[n_tiles]   a row owns the virtual rows [vstart[i], vstart[i+1]) of its tile (the last row of
 *                          tile t up to vcount[t]); a tile has at most W.(RW-1) virtual rows.  Virtual row v belongs to
 *                          wave v % W and accumulates in LDS row (v/W).W + (v%W + v/W) % W.
 *   words                  one int32 per unit entry: flag << 31 | (v / W) << cbits | column; every (tile, wave) stream is
 *                          contiguous, 256-entry aligned and padded with (RW-1) << cbits.  Within a step (64/(F/4)
 *                          consecutive entries) a virtual row is read-modified-written once: a repeat in the next slot
 *                          (same 16-lane DPP row, flag 0) is folded into its neighbour in registers; any other repeat
 *                          carries flag = 1 and is added with an LDS atomic after the step.
 *   stream_start[n_tiles*W], wsteps[n_tiles][W][maxwin1], n_win[n_tiles]: see utilities/lds_tiled.py
 *   pace_every             the tile's waves meet at a barrier after every pace_every-th window (a power of two >= 1)
 * X (n_cols rows) must hold S.X; Y[i] = epilogue( row_scale[i] . (diag[i] . Xself[i] + sum of the row's entries) ),
 * flags / bias / acc_* / Wnext / AMAR_SPMM_SCALE_NEXT as amar_spmm_xs_f32.  The summation order of a row is fixed by
 * the image, so results are bitwise reproducible run to run (they differ from the XS / CSR forms in the last bits).
 */
int amar_spmm_lt_f32(const int32_t *words, const int32_t *stream_start, const int32_t *wsteps, const int32_t *tile_row0,
                     const int32_t *n_win, const int32_t *vstart, const int32_t *vcount, int32_t n_tiles, int32_t maxwin1, int32_t pace_every,
                     const float *diag, const float *row_scale,
                     const float *X, int64_t ldx, int32_t n_cols, const float *Xself,
                     float *Y, int64_t ldy, int32_t n_rows, int32_t F, uint32_t flags, const float *bias,
                     const float *acc_in, int64_t ld_acc_in, float *acc_out, int64_t ld_acc_out, float acc_div,
                     const float *Wnext, int32_t Cn, float *Hnext, int64_t ldhn, amar_stream_t stream);

/* Which gather-address form a tiled propagation launch takes (host only: launches nothing, reads no device memory).  The four
 * kernel families that gather rows of a node table pick their address arithmetic from the table's SPAN, n_cols * ld * 4 bytes
 * (the packed table of amar_gat_xs_f32: n_cols * 2C * 4, whatever ldh), in one host function that the launchers and this
 * query share — so a test can assert the form a call runs before it launches it.
 *   kind      AMAR_PROPAGATE_LT      amar_spmm_lt_f32   (n_cols, ldx, F, flags)
 *             AMAR_PROPAGATE_GAT_LT  amar_gat_lt_f32    (n_cols, ldh, C; flags ignored)
 *             AMAR_PROPAGATE_XS      amar_spmm_xs_f32   (n_cols, ldx, F; flags ignored)
 *             AMAR_PROPAGATE_GAT_XS  amar_gat_xs_f32    (n_cols, ldh, C; flags ignored)
 *   form      AMAR_ADDR_64        span >= 2^32: X + (int64) column * ld
 *             AMAR_ADDR_32        span <  2^32: one 32-bit byte offset (column * ld + 4 q) * 4 from a scalar base
 *             AMAR_ADDR_32_DENSE  span <  2^32 and a compile-time row width (LT kinds: ld == width, a shift; GAT_XS: the packed
 *                                 table).  AMAR_PROPAGATE_XS has no dense form: its 32-bit form is AMAR_ADDR_32 at every ld.
 *             -1 when an argument was refused before the form was decided
 *   kernel    AMAR_PROPAGATE_LT only (0 otherwise): AMAR_LT_KERNEL_PAIRS (the step with the implicit-pair logic),
 *             AMAR_LT_KERNEL_NOPAIRS (AMAR_SPMM_LT_NOPAIRS, F >= 8, a 32-bit form; on the 64-bit form and at F = 4 an image
 *             without pairs runs the PAIRS kernel, which is right for it: every repeat is flagged), AMAR_LT_KERNEL_SAGE_TAIL
 *             (AMAR_SPMM_SAGE_TAIL, F >= 8, a 32-bit form), AMAR_LT_KERNEL_UNSUPPORTED (AMAR_SPMM_SAGE_TAIL otherwise: the call
 *             returns AMAR_EUNSUPPORTED and the caller takes the aggregate + amar_sage_tail_f32).  The AMAR_LT_VARIANT
 *             development kernels are not reported.
 *   col_bits, max_cols = 2^col_bits   columns the packed entry word holds: 31 - ceil(log2(RW)) for the LT kinds (22 / 23 / 24 /
 *             25 at F = 4 / 8 / 16 / 32; GAT: 23 / 24 / 25 at C = 8 / 16 / 32), 26 for the XS kinds.  n_cols == max_cols is
 *             accepted, one more returns AMAR_EUNSUPPORTED (from the query and from all four launchers).
 *   span_bytes  the span compared against 2^32
 * Returns what the launcher returns for these arguments where it looks at nothing else: AMAR_EINVAL (n_cols < 0, an unknown kind,
 * ld < width or, except GAT_XS, ld % 4 != 0, info == NULL), AMAR_EUNSUPPORTED (a width without a kernel, n_cols > max_cols, the
 * GraphSAGE tail without a kernel), in the launcher's order of checks. */
#define AMAR_PROPAGATE_LT 0
#define AMAR_PROPAGATE_GAT_LT 1
#define AMAR_PROPAGATE_XS 2
#define AMAR_PROPAGATE_GAT_XS 3
#define AMAR_ADDR_64 0
#define AMAR_ADDR_32 1
#define AMAR_ADDR_32_DENSE 2
#define AMAR_LT_KERNEL_PAIRS 0
#define AMAR_LT_KERNEL_NOPAIRS 1
#define AMAR_LT_KERNEL_SAGE_TAIL 2
#define AMAR_LT_KERNEL_UNSUPPORTED 3
typedef struct amar_propagate_route_info {
    int32_t form, kernel, col_bits, reserved;
    int64_t max_cols, span_bytes;
} amar_propagate_route_info;
int amar_propagate_route(int32_t kind, int64_t n_cols, int64_t ld, int32_t width, uint32_t flags, amar_propagate_route_info *info);

/* One fused GCN layer (src/models/gnn.py:289-295 + gnn.py:78, Spektral GCNConv.call):
 *     Y[i, 0:C]      = ReLU( sum_j A_hat[i,j] . H[j, 0:C] + bias )      H = X_prev . W  (pre-multiplied)
 *     Hnext[i, 0:Cn] = Y[i, :] . Wnext[C, Cn]                            (only if Wnext != NULL)
 * so that layer l's epilogue performs layer l+1's dense product and each layer is ONE kernel.
 * C in {4,8,16,32,64}; Cn <= 64.  Other multiples of 4 run as column chunks, without the fused next product
 * (Wnext must be NULL for them: AMAR_EUNSUPPORTED otherwise).
 */
int amar_gcn_layer_f32(const int32_t *rowptr, const int32_t *colidx, const float *vals,
                       const float *H, int64_t ldh, int32_t C, const float *bias,
                       float *Y, int64_t ldy,
                       const float *Wnext, int32_t Cn, float *Hnext, int64_t ldhn,
                       int32_t n_rows, amar_stream_t stream);

/* Row-wise small dense product used as the GNN prologue (Keras `K.dot(x, kernel)` inside
 * GCNConv / GATConv; reference call site src/models/gnn.py:78):
 *     H[i, 0:C] = X[i, 0:F] . W[F, C]                     F, C <= 64
 *     copy_to != NULL:  copy_to[i, 0:F] = X[i, 0:F]       (X_0 slice of the concat buffer)
 *     a_self/a_neigh != NULL (GAT):  s_self[i] = H[i,:].a_self,  s_neigh[i] = H[i,:].a_neigh
  * row_scale != NULL (not together with the attention scalars): H[i] is multiplied by row_scale[i] — the pre-scaled table
 * the value-free form of amar_spmm_xs_f32 gathers from.
 */
int amar_rowwise_xw_f32(const float *X, int64_t ldx, int32_t F, const float *W, int32_t C,
                        float *H, int64_t ldh, float *copy_to, int64_t ld_copy,
                        const float *a_self, const float *a_neigh, float *s_self, float *s_neigh,
                        const float *row_scale, int32_t n_rows, amar_stream_t stream);

/* The same product with a row gather:  H[p, 0:C] = row_scale[p] . ( X[row_ids[p], 0:F] . W[F, C] ),  p < n_rows
 * (row_scale NULL: 1; row_ids[p] < 0: a zero row).  The X_0 . W_1 prologue of the SAME call site (src/models/gnn.py:78) when
 * the gathered table is kept in the rank-major block layout of a node-range partition (parallel.py:TypedPartition): X is the
 * trainable node table in the reference's id order (users | items [| properties], src/data/loaders.py:43-68), row_ids maps
 * every row of the block layout to its node (-1 for the padding rows at the end of a type's last block). */
int amar_rowwise_xw_gather_f32(const float *X, int64_t ldx, int32_t F, const int32_t *row_ids, const float *W, int32_t C,
                               float *H, int64_t ldh, const float *row_scale, int32_t n_rows, amar_stream_t stream);

/* Which kernel the two entry points above (and the product of amar_rowwise_xw_heads_f32, asked with C = heads * C) run for a call,
 * and how its capped grid walks the rows (host only: launches nothing, the pointers are looked at for NULL and alignment only).  The
 * launcher calls the same function, AMAR_XW_FORM read at every call included, so a test can assert the form before it launches it.
 *   kernel   AMAR_XW_KERNEL_PIECES8  F == C == 8, no attention scalars, no row ids, AMAR_XW_FORM != "rows"; ldx, ldh (and ld_copy)
 *                                    multiples of 4; X, H, W (and copy_to) 16-byte aligned: 16-byte pieces, two lanes per row
 *            AMAR_XW_KERNEL_VEC8     the same alignment of X, H, copy_to and the leading dimensions, with attention scalars, row ids,
 *                                    a W that is not 16-byte aligned or AMAR_XW_FORM=rows: one thread per row, two rows per thread
 *            AMAR_XW_KERNEL_VEC16    F == C == 16 under the same alignment rules (W's alignment is not looked at): one row per thread
 *            AMAR_XW_KERNEL_GENERIC  everything else: cp lanes per row, cp = C rounded up to a power of two
 *   cp              C rounded up to a power of two (every kernel)
 *   rows_per_block  rows one workgroup of 256 threads takes per trip: 256 / cp (generic), 512 (pieces, vec 8), 256 (vec 16)
 *   blocks          min(ceil(n_rows / rows_per_block), 8192) workgroups; 0 for n_rows == 0 (nothing is launched)
 *   trips           iterations of the grid-stride loop of the thread that makes most: ceil(n_rows / (blocks * rows_per_block)).  The
 *                   second trip starts at n_rows = 8192 * rows_per_block + 1: 4 194 305 (pieces, vec 8), 2 097 153 (vec 16),
 *                   32 768 * (64 / cp) + 1 (generic).
 * has_attn: any of a_self / a_neigh / s_self / s_neigh is given; has_row_ids: the call is amar_rowwise_xw_gather_f32's.
 * Returns the launcher's first refusals in its order: AMAR_EINVAL (n_rows < 0, X, W or H NULL, F or C < 1, ldx < F, ldh < C,
 * info == NULL), AMAR_EUNSUPPORTED (F or C > 64), AMAR_EINVAL (copy_to with ld_copy < F).  What the launcher refuses after these (an
 * incomplete set of attention operands; attention scalars together with row_scale) is not asked here. */
#define AMAR_XW_KERNEL_GENERIC 0
#define AMAR_XW_KERNEL_VEC8 1
#define AMAR_XW_KERNEL_VEC16 2
#define AMAR_XW_KERNEL_PIECES8 3
typedef struct amar_xw_route_info {
    int32_t kernel, cp, rows_per_block, blocks;
    int64_t trips;
} amar_xw_route_info;
int amar_rowwise_xw_route(const float *X, int64_t ldx, int32_t F, const float *W, int32_t C,
                          const float *H, int64_t ldh, const float *copy_to, int64_t ld_copy,
                          int32_t has_attn, int32_t has_row_ids, int32_t n_rows, amar_xw_route_info *info);

/* One GraphSAGE-mean layer (Spektral 1.x GraphSageConv, built at src/models/gnn.py:354-361):
 *     agg_i = ( [self_loop] X_i + sum_{j in N(i)} X_j ) / ( [self_loop] 1 + |N(i)| )
 *     Y_i   = ReLU( l2_normalize( [X_i || agg_i] . W[2F, C] + bias ) )
 * rowptr/colidx hold the raw symmetric adjacency with duplicate edges kept and no diagonal;
 * edge values are ignored, as in the reference.  F in {4,8,16,32}; C <= 64.
 */
int amar_sage_layer_f32(const int32_t *rowptr, const int32_t *colidx,
                        const float *X, int64_t ldx, int32_t F,
                        const float *W, const float *bias, int32_t C,
                        float *Y, int64_t ldy, int32_t self_loop,
                        int32_t n_rows, amar_stream_t stream);

/* The tail of the same layer when the mean aggregate AGG[n_rows, F] was produced by an SpMM (amar_spmm_xs_f32 on the
 * XCD-sliced mean image for large graphs; amar_spmm_csr_f32 + amar_row_affine_f32 for widths the fused kernel is not
 * instantiated for):  Y = relu(l2_normalize([X || AGG] . W + bias)), W [2F, C] row-major.  F, C multiples of 4, <= 64. */
int amar_sage_tail_f32(const float *X, int64_t ldx, const float *AGG, int64_t lda, int32_t F,
                       const float *W, const float *bias, int32_t C, float *Y, int64_t ldy,
                       int64_t n_rows, amar_stream_t stream);

/* The instantiation and the grid of amar_sage_tail_f32 (host only; the launcher takes both from the same function):
 *   cp      accumulators per thread: the smallest of 4, 8, 16, 32, 64 that holds C (C = 12, 20, 36 .. leave cp - C of them guarded off)
 *   blocks  min(ceil(n_rows / 256), 8192) workgroups of 256 threads, one row per thread; 0 for n_rows == 0
 *   trips   ceil(n_rows / (blocks * 256)): the second trip starts at n_rows = 2 097 153
 * Returns the launcher's shape refusals: AMAR_EINVAL (n_rows < 0, F or C < 4 or not a multiple of 4, info == NULL), AMAR_EUNSUPPORTED
 * (F or C > 64).  The launcher looks at its pointers and leading dimensions between the two. */
typedef struct amar_sage_tail_route_info {
    int32_t cp, blocks;
    int64_t trips;
} amar_sage_tail_route_info;
int amar_sage_tail_route(int32_t F, int32_t C, int64_t n_rows, amar_sage_tail_route_info *info);

/* GraphSAGE's other aggregators (config.yaml:17-18 `model.aggregate`, handed to Spektral's GraphSageConv at
 * src/models/gnn.py:331-361; Spektral 1.x resolves the name to a segment reduction).  The entries of row i are its CSR row
 * (duplicates kept, values ignored) plus i itself when self_loop:
 *     agg_i[f] = OP over entries j of X[j, f]          OP = sum | max | min;  a row without entries gives 0
 * (a stated deviation from tf.math.unsorted_segment_max, which fills such a row with the lowest float).  Inputs are finite;
 * max / min compare with IEEE ==, so +0 and -0 are one value. */
#define AMAR_AGG_SUM 0
#define AMAR_AGG_MAX 1
#define AMAR_AGG_MIN 2

/* One GraphSAGE layer with aggregator `op`, fused like amar_sage_layer_f32 (one wavefront per row):
 *     Y_i = ReLU( l2_normalize( [X_i || agg_i] . W[2F, C] + bias ) )
 * F in {4,8,16,32}; C <= 64; other shapes AMAR_EUNSUPPORTED (amar_sage_aggregate_f32 + amar_sage_tail_f32). */
int amar_sage_layer_agg_f32(const int32_t *rowptr, const int32_t *colidx,
                            const float *X, int64_t ldx, int32_t F,
                            const float *W, const float *bias, int32_t C,
                            float *Y, int64_t ldy, int32_t self_loop, int32_t op,
                            int32_t n_rows, amar_stream_t stream);

/* The max / min aggregate alone: AGG[n_rows, F] (leading dimension lda) and, when CNT is not NULL, the training tape's
 *     CNT[i, f] = number of entries j of row i with X[j, f] == AGG[i, f]      (exact small integers stored as float; ldc)
 * F % 4 == 0, F <= 64 (else AMAR_EUNSUPPORTED); op = AMAR_AGG_MAX | AMAR_AGG_MIN (AMAR_AGG_SUM: AMAR_EUNSUPPORTED — the sum is
 * amar_spmm_csr_f32 without values, plus the own row).  Both results are exact, hence bitwise reproducible. */
int amar_sage_aggregate_f32(const int32_t *rowptr, const int32_t *colidx,
                            const float *X, int64_t ldx, int32_t F,
                            float *AGG, int64_t lda, float *CNT, int64_t ldc,
                            int32_t self_loop, int32_t op, int32_t n_rows, amar_stream_t stream);

/* Reverse pass of the max / min aggregate (TensorFlow's _UnsortedSegmentMinOrMaxGrad: every entry that attains the
 * extremum, duplicates included, takes an equal share):
 *     DX[j, f] += sum over entries (i <- j) of  [X[j, f] == AGG[i, f]] * DAGG[i, f] / CNT[i, f]
 * rowptr / colidx here are the structure whose row j lists the entries INTO j — the TRANSPOSE of the one the forward pass walked
 * (the stable transpose of the csr-transpose entry point; the same arrays where the edge multiset is symmetric): row j walks that row
 * (+ itself when self_loop) and adds in a fixed order — no atomics, bitwise reproducible.
 * pack: scratch of n_rows * 2F floats; a first launch writes [AGG_i | DAGG_i / CNT_i] there (0 where CNT is 0) so that a
 * neighbour is one contiguous read.  F % 4 == 0, F <= 64.  DX is accumulated into. */
int amar_sage_aggregate_bwd_f32(const int32_t *rowptr, const int32_t *colidx,
                                const float *X, int64_t ldx, const float *AGG, int64_t lda,
                                const float *CNT, int64_t ldc, const float *DAGG, int64_t ldg, int32_t F,
                                float *pack, float *DX, int64_t lddx,
                                int32_t self_loop, int32_t n_rows, amar_stream_t stream);

/* One GAT layer, 1 head (Spektral 1.x GATConv._call_single, built at src/models/gnn.py:321-328):
 *     e_ij  = LeakyReLU_0.2( s_self[i] + s_neigh[j] ),  j in N(i) (+ i itself if self_loop)
 *     alpha = exp(e_ij - max_j e_ij) / ( sum_j exp(e_ij - max_j e_ij) + 1e-9 )
 *     Y_i   = ReLU( sum_j alpha_ij H_j + bias )
 * H, s_self, s_neigh come from amar_rowwise_xw_f32.  C in {4,8,16,32,64}; other multiples of 4 run as column chunks
 * (the attention coefficients only depend on the per-node scalars).
 */
int amar_gat_layer_f32(const int32_t *rowptr, const int32_t *colidx,
                       const float *H, int64_t ldh, int32_t C,
                       const float *s_self, const float *s_neigh, const float *bias,
                       float *Y, int64_t ldy, int32_t self_loop,
                       int32_t n_rows, amar_stream_t stream);

/* Multi-head GAT (Spektral 1.x GATConv._call_single + call with attn_heads = heads, heads x C output channels).  The prologue:
 *     Hd[i, h*C + c] = X[i, 0:F] . W[0:F, h, c]            W [F, heads, C] in Keras's order = row-major [F, heads*C]
 *     S[i, h]         = Hd[i, h, :] . a_self[:, h]          a_self, a_neigh [C, heads, 1]: element (c, h) at c*heads + h
 *     S[i, heads + h] = Hd[i, h, :] . a_neigh[:, h]
 * S is [n_rows, 2*heads] contiguous: one row holds the node's `heads` self scalars, then its `heads` neighbour scalars, so that a
 * neighbour's scalars for every head are ONE contiguous read of heads floats.  The product is amar_rowwise_xw_f32's (same kernels,
 * same bits for Hd); the scalars are one thread per (row, head), c ascending.  C % 4 == 0 and heads*C <= 64, F <= 64; other shapes
 * AMAR_EUNSUPPORTED. */
int amar_rowwise_xw_heads_f32(const float *X, int64_t ldx, int32_t F, const float *W, int32_t heads, int32_t C,
                              float *Hd, int64_t ldh, const float *a_self, const float *a_neigh, float *S,
                              int32_t n_rows, amar_stream_t stream);

/* One multi-head GAT layer on Hd / S of amar_rowwise_xw_heads_f32, one wavefront per row, every head in the same walk:
 *     e_ijh     = LeakyReLU_0.2( S[i, h] + S[j, heads + h] ),   j over the entries of row i (duplicates kept) (+ i itself if self_loop)
 *     alpha_ijh = exp(e_ijh - max_j e_ijh) / ( sum_j exp(e_ijh - max_j e_ijh) + 1e-9 )         per target i AND head h
 *     out[i, h, :] = sum_j alpha_ijh Hd[j, h, :]
 *     concat != 0:  Y[i, 0:heads*C] = ReLU( out[i, :, :] flattened + bias[0:heads*C] )
 *     concat == 0:  Y[i, 0:C]       = ReLU( (1/heads) sum_h out[i, h, :] + bias[0:C] )       (h ascending)
 * A row without entries and without self loop gives ReLU(bias).  out_tape (may be NULL; [n_rows, heads*C] contiguous) receives
 * out[i, :, :] before the bias: what amar_gat_heads_bwd_f32 needs under concat == 0, where Y no longer holds the heads apart.
 * Y and Hd are strided (ldy, ldh; multiples of 4, 16-byte aligned bases).  C % 4 == 0 and heads*C <= 64; other shapes
 * AMAR_EUNSUPPORTED. */
int amar_gat_heads_f32(const int32_t *rowptr, const int32_t *colidx,
                       const float *Hd, int64_t ldh, int32_t heads, int32_t C,
                       const float *S, const float *bias, float *Y, int64_t ldy, float *out_tape,
                       int32_t concat, int32_t self_loop, int32_t n_rows, amar_stream_t stream);

/* ---- scoring head -------------------------------------------------------------------------
 * Y[M, N] = act( X[M, K] . W[K, N] + bias[N] )   fp32 MFMA GEMM (Keras Dense; src/models/dense.py:4-17)
 * ids != NULL gathers the input rows first: row m of the product reads X[ids[m], :]
 * (tf.nn.embedding_lookup at src/models/basic.py:73-74, src/models/hybrid.py:138-139).
 * Y is written at column offset 0 of a matrix with leading dimension ldy, so two calls with
 * Y and Y + N realise `Concatenate` (src/models/basic.py:35, src/layers/fusion.py:51-53).
 */
int amar_dense_f32(const float *X, int64_t ldx, const int32_t *ids,
                   const float *W, const float *bias, float *Y, int64_t ldy,
                   int64_t M, int32_t K, int32_t N, int32_t act, amar_stream_t stream);
/* Which kernel an amar_dense_f32 call with these arguments takes (host only: nothing is launched, the pointers are looked at for NULL and
 * for their alignment; `act` may carry AMAR_DENSE_WT).  The launcher asks the same function, so the two cannot disagree.  Returns what the
 * launcher's argument checks return (AMAR_EINVAL, AMAR_EUNSUPPORTED for a grid past 2^31 - 1; info == NULL: AMAR_EINVAL).
 *   kernel        first match wins; "aligned" = vec_x and vec_w and no AMAR_DENSE_WT
 *                 AMAR_DENSE_KERNEL_SMALL    64 x 64 tiles, two k-tiles of 32 in flight: aligned, K % 32 == 0, N % 64 == 0, M <= 4 096
 *                 AMAR_DENSE_KERNEL_TILE128  128 x 128 tiles, guard-free: aligned, K % 16 == 0, N % 128 == 0 and
 *                                            ceil8(ceil(M / 128)) * N / 128 >= 256 workgroups
 *                 AMAR_DENSE_KERNEL_FULL     128 x 64 tiles, guard-free: aligned, K % 16 == 0, N % 64 == 0
 *                 AMAR_DENSE_KERNEL_GUARDED  128 x 64 tiles with guarded staging, in the (vec_x, vec_w) variant: everything else
 *                 -1 when an argument was refused
 *   vec_x         X is read by 16-byte loads where the kernel can: ldx % 4 == 0 and X 16-byte aligned
 *   vec_w         the same for W: N % 4 == 0 and W 16-byte aligned (a transposed W is read by single floats whatever vec_w says; it still
 *                 selects the variant).  Y and bias are written / read by single floats: their alignment is not looked at.
 *   w_trans       AMAR_DENSE_WT was given
 *   grid_x, grid_y  the launched grid.  SMALL: ceil(M / 64) x N / 64.  The others: ceil8(ceil(M / 128)) * n_col_blocks x 1 (workgroup L
 *                 runs on XCD L % 8; row tiles past M return at once)
 *   n_col_blocks  column blocks: N / 64 (SMALL), N / 128 (TILE128), ceil(N / 64) (FULL, GUARDED)
 *   launches      1, or 0 for M == 0 (AMAR_OK, nothing to do: kernel is -1, vec_x, vec_w, the grid and n_col_blocks are 0) */
#define AMAR_DENSE_KERNEL_SMALL 0
#define AMAR_DENSE_KERNEL_TILE128 1
#define AMAR_DENSE_KERNEL_FULL 2
#define AMAR_DENSE_KERNEL_GUARDED 3
typedef struct amar_dense_route_info {
    int32_t kernel, vec_x, vec_w, w_trans, grid_x, grid_y, n_col_blocks, launches;
} amar_dense_route_info;
int amar_dense_route(const float *X, int64_t ldx, const int32_t *ids, const float *W, const float *bias, float *Y, int64_t ldy,
                     int64_t M, int32_t K, int32_t N, int32_t act, amar_dense_route_info *info);

/* The same layer with its products on the bf16 matrix instruction and BOTH operands split three ways (x = hi + mid + lo
 * exactly, six part products accumulated in f32: as accurate as the f32 instruction, 2.7 times fewer matrix-pipe cycles) for
 * the wide layers of the content towers (768 -> 256 of src/models/hybrid.py:52-58).  K % 32 == 0, N % 128 == 0, ldx % 4 == 0,
 * 16-byte aligned X; other shapes return AMAR_EUNSUPPORTED (use amar_dense_f32).  Wq is the layer's kernel pre-split by
 * amar_dense_split_pack_f32 (HOST in, HOST out of amar_dense_split_bytes(K, N) bytes — once per weight update), copied to
 * the device by the caller.
 * PRECONDITION: finite inputs.  The split x = hi + mid + lo is exact for finite x only; an infinite activation or weight gives
 * mid = Inf - Inf = NaN, so a product that the f32 instruction would return as +-Inf (or saturate) comes back NaN here.  NaN
 * inputs propagate as NaN in both forms.  The same holds for the split-product forms of amar_chain_f32 / amar_dual_chain_f32
 * (the default of the pair stages; AMAR_PAIR_MFMA=f32 / AMAR_DENSE_SPLIT=0 select the f32 instruction). */
int64_t amar_dense_split_bytes(int32_t K, int32_t N);
int amar_dense_split_pack_f32(const float *W, int32_t K, int32_t N, void *out);
int amar_dense_split_f32(const float *X, int64_t ldx, const int32_t *ids, const void *Wq, const float *bias,
                         float *Y, int64_t ldy, int64_t M, int32_t K, int32_t N, int32_t act, amar_stream_t stream);

/* Fused gather + Concatenate + Dense stack (BasicRS / HybridCBRS towers and classifiers:
 * src/models/basic.py:31-37,72-75, src/models/hybrid.py:72-89, src/models/dense.py:4-17).
 * For every row p < P:
 *     x = [ A[ida(p), 0:Da] || B[idb(p), 0:Db] ],  ida(p) = ids_a ? ids_a[p] - base_a : p   (same for B)
 *         or, with sum_inputs != 0 (Da == Db):  x = in_act( A[ida(p)] + B[idb(p)] ) — the form a Dense layer over a
 *         concatenation takes once its two halves have been applied per entity (x.W = u.W[:d] + i.W[d:])
 *     x = act_l( x . W_l + b_l )  for l = 0 .. n_layers-1      dims[0] = Da + Db (Da if sum_inputs), dims[l+1] = units of layer l
 * out[p, 0:dims[n_layers]] = x.  A trailing 1-unit layer (the sigmoid scorer) is evaluated as a
 * dot product and written to out[p * ldo].  Activations stay in registers between layers
 * (fp32 MFMA 16x16x4); weights come pre-packed in fragment order from amar_chain_pack_f32 and
 * stay in LDS.  Limits: every width <= 128, Da and Db multiples of 4, <= 8 layers; shapes
 * outside them return AMAR_EUNSUPPORTED (use amar_dense_f32 layer by layer instead).
 * amar_chain_pack_floats / amar_chain_pack_f32 run on the HOST (host pointers): kernels[l] is the
 * row-major [dims[l], dims[l+1]] Keras kernel, biases[l] its bias; the blob is then copied to
 * the device by the caller.
 * Arithmetic: f32 values and f32 sums throughout.  The pair-stage form (sum_inputs with both id lists, ReLU, equal
 * layer widths of 48 or 64, with or without a trailing 1-unit layer) and amar_dual_chain_f32's 64-wide form take their PRODUCTS on
 * the bf16 matrix instruction with both operands split into three bf16 parts (x = hi + mid + lo exactly; six part
 * products accumulated in f32): a term x.w is off by at most 3 * 2^-24 |x.w| — as close to a float64 evaluation as the
 * f32 instruction, not bit-identical to it.  Environment AMAR_PAIR_MFMA=f32 keeps v_mfma_f32_16x16x4_f32 everywhere.
 * The pair-stage form does NOT need the trailing 1-unit layer: a [P, 48] or [P, 64] block out of square ReLU layers runs it too.
 * It also keeps the f32 instruction, without being asked, when the packed weights plus their bf16 fragments (3 KB per pair of
 * 16 x 16 tiles) exceed 64 KB of LDS: two or more square layers at 64, three or more at 48 (amar_chain_route reports `split`).
 */
int64_t amar_chain_pack_floats(const int32_t *dims, int32_t n_layers);
int amar_chain_pack_f32(const float *const *kernels, const float *const *biases, const int32_t *dims,
                        int32_t n_layers, float *out);
int amar_chain_f32(const float *A, int64_t lda, int32_t Da, const int32_t *ids_a, int32_t base_a,
                   const float *B, int64_t ldb, int32_t Db, const int32_t *ids_b, int32_t base_b,
                   int32_t sum_inputs, int32_t in_act,
                   const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers,
                   float *out, int64_t ldo, int64_t P, amar_stream_t stream);

/* The same with an output index: row p of the chain is written to out row out_index[p] (int32 [P], a permutation of
 * 0..P-1, or NULL = amar_chain_f32).  For a pair list the caller keeps in another order than the one the scores are
 * wanted in — the pair stage of a predict pass (src/experiment.py:197, the test Sequence's order, datasets.py:199-203)
 * bucketed ONCE per dataset by item range so that the workgroups of one XCD (pairs p with (p >> 7) % 8 equal, under
 * round-robin dispatch) gather item-tower rows of one eighth of the items and find them in that XCD's L2: the list is
 * constant across steps and epochs, the scores still land in the Sequence's order.
 * Every shape amar_chain_f32 takes is taken with an index too, except the segment form.  The pair-stage kernel scatters scores
 * only: a pair-stage-shaped call with out_index and NO trailing 1-unit layer (a [P, N] block) runs the generic kernel, and its
 * rows are, bit for bit, those of the same call without out_index, scattered.
 */
int amar_chain_indexed_f32(const float *A, int64_t lda, int32_t Da, const int32_t *ids_a, int32_t base_a,
                           const float *B, int64_t ldb, int32_t Db, const int32_t *ids_b, int32_t base_b,
                           int32_t sum_inputs, int32_t in_act,
                           const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers,
                           float *out, int64_t ldo, const int32_t *out_index, int64_t P, amar_stream_t stream);

/* The per-entity tower form of the chain (one input table, no second table, no trailing 1-unit layer) reading the
 * `Concatenate` of ReductionLayer('concatenation') (src/layers/reduction.py:15-17; src/models/gnn.py:84) IN PLACE:
 *     x = [ seg[0][r, 0:w_0] || seg[1][r, 0:w_1] || ... ],   r = ids ? ids[p] - base : p       (HOST arrays of n_seg entries)
 * so that the [N, d(L+1)] table never has to be assembled — each X_l stays where its layer (or the all-gather of a
 * node-range partition) left it.  Widths are multiples of 4, their sum <= 128, n_seg <= 8.  Only stacks with a
 * compile-time tower shape run this way (ReLU layers with an optionally linear last one, every width <= 64, at most three
 * layers: the towers of every econfig of the reference); other shapes return AMAR_EUNSUPPORTED — the caller then copies the
 * columns together (amar_copy_columns_f32) and calls amar_chain_f32.  Same arithmetic as amar_chain_f32 on the assembled
 * table, bit for bit. */
int amar_chain_segments_f32(const float *const *seg, const int64_t *seg_ld, const int32_t *seg_width, int32_t n_seg,
                            const int32_t *ids, int32_t base,
                            const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers,
                            float *out, int64_t ldo, int64_t P, amar_stream_t stream);

/* What an amar_chain_indexed_f32 / amar_chain_segments_f32 call with these arguments does (host only: nothing is launched, the device
 * pointers are looked at for NULL and alignment, dims and acts are read).  The launchers start from the same function, so the two
 * cannot disagree.  Returns what the launcher's argument checks return (AMAR_OK, AMAR_EINVAL, AMAR_EUNSUPPORTED; info == NULL:
 * AMAR_EINVAL); `info` is meaningful after AMAR_OK only.
 *   kernel     AMAR_CHAIN_KERNEL_GENERIC  chain_kernel<maxt, 2, full, am>: any shape
 *              AMAR_CHAIN_KERNEL_PIPE     chain_pipe_kernel<maxt, 2, scatter, split>: the pair stage — sum_inputs with in_act = relu, both
 *                                         id lists, every width (Da, every layer) 16 maxt with maxt <= 4, ReLU layers, a trailing
 *                                         1-unit layer or none (none: without out_index only), lda / ldb < 2^30, P < 2^30 - 2^22
 *              AMAR_CHAIN_KERNEL_ROWS     chain_rows_kernel<shape, 2, lastlin, seg>: one table (Db = 0), no 1-unit layer, no
 *                                         out_index, two or three ReLU layers with an optionally linear last one, in one of six shapes
 *   maxt       tiles of 16 the widest width needs, rounded up to 3, 4 or 8 (widths <= 48, <= 64, <= 128)
 *   full       every width (dims[0], every layer, the 1-unit layer's input) has exactly maxt tiles
 *   am         1: ReLU on every layer (and on the summed input, with sum_inputs); 2: the same with a linear LAST layer and no 1-unit
 *              layer; 0: anything else (activations are run-time values).  The 1-unit layer's activation never counts.
 *   split      (pipe) products on the bf16 instruction with split operands: packed floats (rounded up to 4) * 4 +
 *              layers * maxt * ceil(maxt / 2) * 3 072 bytes <= 65 536 and AMAR_PAIR_MFMA != f32 (read once per process)
 *   scatter    (pipe) out_index given
 *   shape      (rows) layers | tiles(dims[0]) << 3 | tiles(dims[1]) << 6 | tiles(dims[2]) << 9 | tiles(dims[3]) << 12; the six:
 *              24-24-24-48, 48-48-48-64, 24-24-24, 8-24-24-48, 16-48-48-64, 48-48-48 (any widths with the same tile counts); else 0
 *   lastlin    (rows) am == 2;  seg: (rows) called through amar_chain_segments_*
 *   has_dot    the stack ends in a 1-unit layer evaluated as a dot product;  layers: the layers before it
 *   blocks     workgroups launched: ceil(P / 128), at most 4 096 (generic), 1 536 (pipe), 1 024 (rows); 0: no launch
 *   threads    256
 *   lds_bytes  dynamic LDS asked for: amar_chain_pack_floats * 4, plus the fragments (see split) for the split pair stage */
#define AMAR_CHAIN_KERNEL_GENERIC 0
#define AMAR_CHAIN_KERNEL_PIPE 1
#define AMAR_CHAIN_KERNEL_ROWS 2
typedef struct amar_chain_route_info {
    int32_t kernel, maxt, full, am, split, scatter, shape, lastlin, seg, has_dot, layers, threads;
    int64_t blocks, lds_bytes;
} amar_chain_route_info;
int amar_chain_route(const float *A, int64_t lda, int32_t Da, const int32_t *ids_a, int32_t base_a,
                     const float *B, int64_t ldb, int32_t Db, const int32_t *ids_b, int32_t base_b,
                     int32_t sum_inputs, int32_t in_act,
                     const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers,
                     float *out, int64_t ldo, const int32_t *out_index, int64_t P, amar_chain_route_info *info);
int amar_chain_segments_route(const float *const *seg, const int64_t *seg_ld, const int32_t *seg_width, int32_t n_seg,
                              const int32_t *ids, int32_t base,
                              const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers,
                              float *out, int64_t ldo, int64_t P, amar_chain_route_info *info);

/* Both entity towers in ONE launch: two one-table row-chain problems (rows themselves, no ids; each with its own table, packed
 * weights, widths and output) whose stacks run the same compile-time tower kernel (amar_chain_route_info.kernel ==
 * AMAR_CHAIN_KERNEL_ROWS with equal `shape`, `lastlin` and `lds_bytes`), both with at least one row.  The workgroups of one grid are
 * dealt to the two problems in proportion to their rows; per row the arithmetic is that of amar_chain_f32, bit for bit.
 * A, lda, wpack, dims, acts, out, ldo, P are HOST arrays of two entries.  amar_chain_rows2_route (host only, no launch) reports
 * whether the launch is taken (one_launch) and the workgroups of each part; amar_chain_rows2_f32 returns AMAR_EUNSUPPORTED where
 * it is not: call amar_chain_f32 once per problem instead.  Argument errors of either problem are those of amar_chain_f32. */
typedef struct amar_chain_rows2_route_info {
    int32_t one_launch, shape, lastlin, threads;
    int64_t blocks[2], lds_bytes;
} amar_chain_rows2_route_info;
int amar_chain_rows2_route(const float *const *A, const int64_t *lda, const float *const *wpack, const int32_t *const *dims,
                           const int32_t *const *acts, int32_t n_layers, float *const *out, const int64_t *ldo, const int64_t *P,
                           amar_chain_rows2_route_info *info);
int amar_chain_rows2_f32(const float *const *A, const int64_t *lda, const float *const *wpack, const int32_t *const *dims,
                         const int32_t *const *acts, int32_t n_layers, float *const *out, const int64_t *ldo, const int64_t *P,
                         amar_stream_t stream);

/* Fused two-branch scorer for the hybrid head (src/models/hybrid.py:72-89) once the first Dense layers of
 * dense3a / dense3b have been folded into the per-entity tables:
 *     x_b  = in_act( A[b][ida_b(p)] + B[b][idb_b(p)] )            b = 0, 1;  [P, D]
 *     x_b  = act_l( x_b . W_bl + b_bl )                            n_branch layers D -> D per branch
 *     out  = trunk( [x_0 || x_1] )                                 Dense stack trunk_dims[0] = 2D, equal hidden widths, last = 1 unit
 * A, lda, ida, base_a (and B, ...) are HOST arrays of two entries (device pointers inside).  wpack = the
 * amar_chain_pack_f32 blobs of branch 0 (dims [D, D, ..]), branch 1 and the trunk, concatenated on the device.
 * D % 16 == 0, D <= 64, trunk hidden widths <= 64; other shapes return AMAR_EUNSUPPORTED (use amar_chain_f32).
 */
int amar_dual_chain_f32(const float *const *A, const int64_t *lda, const int32_t *const *ida, const int32_t *base_a,
                        const float *const *B, const int64_t *ldb, const int32_t *const *idb, const int32_t *base_b,
                        int32_t D, int32_t in_act, int32_t n_branch, const int32_t *branch_acts,
                        const int32_t *trunk_dims, const int32_t *trunk_acts, int32_t n_trunk,
                        const float *wpack, float *out, int64_t ldo, int64_t P, amar_stream_t stream);
/* The same on a pair list kept in another order (pair p is written to out[out_index[p] * ldo]; out_index == NULL: in place),
 * like amar_chain_indexed_f32. */
int amar_dual_chain_indexed_f32(const float *const *A, const int64_t *lda, const int32_t *const *ida, const int32_t *base_a,
                                const float *const *B, const int64_t *ldb, const int32_t *const *idb, const int32_t *base_b,
                                int32_t D, int32_t in_act, int32_t n_branch, const int32_t *branch_acts,
                                const int32_t *trunk_dims, const int32_t *trunk_acts, int32_t n_trunk,
                                const float *wpack, float *out, int64_t ldo, const int32_t *out_index, int64_t P,
                                amar_stream_t stream);

/* Concatenate / ReductionLayer as layout operations (src/layers/reduction.py:15-33,
 * src/layers/fusion.py:51-53): copy a [n_rows, width] block between two strided matrices
 * (row r of dst reads row ids[r] - base of src when ids != NULL: tf.nn.embedding_lookup), and
 * out = X_0 + X_1 + ... (+ division by n_layers for 'mean') over the n_layers equal-width column
 * blocks of a concatenation buffer, added in layer order like tf.add_n.
 */
int amar_copy_columns_f32(const float *src, int64_t lds, const int32_t *ids, int32_t base,
                          float *dst, int64_t ldd, int64_t n_rows, int32_t width, amar_stream_t stream);
int amar_reduce_layers_f32(const float *cat, int64_t ld, int32_t n_layers, int32_t width, float *out, int64_t ldo,
                           int64_t n_rows, int32_t mean, amar_stream_t stream);

/* dst[index[t] * ldd] = src[t] for t in [0, n): Keras `predict` returns the scores in the order of the Sequence's pairs
 * (src/data/datasets.py:199-213 — the test Sequence is not shuffled, its order is the file's), while the pair stage walks
 * a list prepared for its gathers; this is the second half of the way back.  The positions are visited window by window
 * (window w = [window_off[w], window_off[w + 1]), device array of n_windows + 1 entries; NULL: n_windows equal slices),
 * all workgroups of one XCD in the same window: prepared so that a window's destinations are a narrow range of dst, its
 * lines are completed in that XCD's L2 and leave it whole.  index must be a partial permutation (no two t with the same
 * destination); n < 2^31. */
int amar_scatter_f32(const float *src, const int32_t *index, float *dst, int64_t ldd, int64_t n,
                     const int32_t *window_off, int32_t n_windows, amar_stream_t stream);

/* The same permutation for a caller that can PROMISE more (models/basic.py:PairPlan does, by construction):
 *   - every window is CLOSED: the values index[t] of t in [window_off[w], window_off[w + 1]) are a bijection onto that same
 *     range (sources and destinations of a window are one contiguous range; window_off[0] = 0, window_off[n_windows] = n);
 *   - dst is dense (one float per position: ldd == 1);
 *   - no window is longer than max_window, and max_window <= AMAR_SCATTER_CLOSED_MAX_WINDOW.
 * A window is then finished in LDS — its values placed at their final offset on chip — and written to dst in whole 16-byte
 * stores (a scalar head and tail where dst + window_off[w] is not 16-byte aligned) instead of one store transaction per
 * score; windows longer than half the capacity are cut into two destination pieces, one workgroup each.  Same bits as
 * amar_scatter_f32: the values are moved, never recomputed.  max_window is the host's knowledge of the table (nothing is
 * read back from the device): AMAR_EINVAL for a null pointer (window_off included), n < 0, n >= 2^31, n_windows < 1,
 * max_window < 0 or > AMAR_SCATTER_CLOSED_MAX_WINDOW, or n_windows windows of max_window that cannot cover n; AMAR_OK and
 * nothing written for n == 0.  A table that breaks the promise gives wrong values inside [0, n), never a store outside a
 * window's own range. */
#define AMAR_SCATTER_CLOSED_MAX_WINDOW 65536
int amar_scatter_closed_f32(const float *src, const int32_t *index, float *dst, int64_t n, const int32_t *window_off,
                            int32_t n_windows, int32_t max_window, amar_stream_t stream);

/* ReductionLayer('w-sum') = WeightedSum (src/layers/reduction.py:36-55): out = sum over the n_layers column blocks of
 * (w[l] * w[l]) * X_l with a learnable device vector w [n_layers] (initialised to ones); products rounded, then added in layer order.
 * n_layers <= 8.  The reverse pass writes d_cat[:, block l] = w[l]^2 d_out and dw[l] = 2 w[l] sum(d_out . X_l), the sums formed per
 * workgroup of a fixed grid and added in workgroup order (no float atomics); `scratch` holds amar_reduce_layers_wsum_bwd_scratch()
 * floats.
 */
int amar_reduce_layers_wsum_f32(const float *cat, int64_t ld, int32_t n_layers, int32_t width, const float *w, float *out, int64_t ldo,
                                int64_t n_rows, amar_stream_t stream);
int64_t amar_reduce_layers_wsum_bwd_scratch(void);
int amar_reduce_layers_wsum_bwd_f32(const float *cat, int64_t ld, int32_t n_layers, int32_t width, const float *w,
                                    const float *d_out, int64_t ldd, float *d_cat, int64_t ld_dcat, float *dw, float *scratch,
                                    int64_t n_rows, amar_stream_t stream);

/* The same GAT layer on the XCD-sliced image of the (square) edge-list adjacency, for graphs whose node table exceeds the
 * per-XCD L2s: rowptr / colidx as in amar_spmm_xs_f32 (values unused).  `packed` is scratch [n, 2C] floats that the call
 * fills with [ H | s_neigh | 0 .. ] rows (one L2 request then serves the neighbour's features and its scalar), `partials`
 * scratch [n_slices, n, 2C].  The segment softmax stays exact through (max, sum, weighted sum) triples merged per
 * (row, slice) and across slices.  C = 8.  H, s_self, s_neigh and `packed` have n_cols rows (the columns of the image);
 * a row block of a larger graph (multi-GPU partition) has n_rows < n_cols and its row i is node row_offset + i.
 */
int amar_gat_xs_f32(const int32_t *rowptr, const int32_t *colidx, int32_t n_slices,
                    const float *H, int64_t ldh, int32_t C, const float *s_self, const float *s_neigh, const float *bias,
                    float *packed, float *partials, float *Y, int64_t ldy, int32_t self_loop, int32_t n_rows,
                    int32_t n_cols, int32_t row_offset, amar_stream_t stream);

/* The same GAT layer (Spektral GATConv as instantiated at src/models/gnn.py:321-328) on the LDS-tiled image of the
 * edge-list adjacency (layout as amar_spmm_lt_f32; every edge a unit entry, duplicates repeated), C = 8, 16 or 32.
 * The LDS row of a virtual row holds (sum w.h [C], sum w, s_self of its row): RW = amar_gat_lt_rows_per_wave(C) rows per
 * wave (216 / 124 / 64), cbits = 31 - ceil(log2(RW)); `rows_per_wave` states the RW the image was cut for and must equal that
 * value (AMAR_EINVAL otherwise: a taller tile would index past the workgroup's LDS).  An entry (i, j) weighs
 *     w_ij = exp( LeakyReLU_0.2(s_self[i] + s_neigh[j]) - M_i ),   M_i = LeakyReLU_0.2(s_self[i] + *s_neigh_max)
 * with *s_neigh_max >= every s_neigh (amar_colmax_f32 writes it): M_i bounds the row's maximum, so no running maximum is
 * needed and the weights add up like the plain sum's entries; out_i = ReLU( (sum_j w_ij H_j) / (sum_j w_ij) + bias ) is
 * Spektral's max-subtracted softmax up to rounding (its +1e-9 in the denominator, >= 1 there, is below fp32 resolution).
 * A row whose weight sum stays below e^-60 (its own maximum lies more than 60 under the bound), and every empty row, is
 * recomputed in the same launch from rowptr / colidx (the CSR of the same rows and columns, duplicates kept) with the row's true
 * maximum and the 1e-9, exactly as amar_gat_layer_f32 does.  diag[i] = number of (i, i) edges in the list (they, and the added
 * self loop when self_loop != 0, enter as the row's self term).  H, s_self, s_neigh cover the n_cols columns; row i of a row
 * block (multi-GPU partition) is node row_offset + i.
 */
int amar_gat_lt_f32(const int32_t *words, const int32_t *stream_start, const int32_t *wsteps, const int32_t *tile_row0,
                    const int32_t *n_win, const int32_t *vstart, const int32_t *vcount, int32_t n_tiles, int32_t maxwin1, int32_t pace_every,
                    int32_t rows_per_wave, const float *diag, const int32_t *rowptr, const int32_t *colidx,
                    const float *H, int64_t ldh, int32_t C, const float *s_self, const float *s_neigh, const float *s_neigh_max,
                    const float *bias, float *Y, int64_t ldy, int32_t self_loop, int32_t n_rows, int32_t n_cols, int32_t row_offset,
                    amar_stream_t stream);
int amar_gat_lt_rows_per_wave(int32_t C);
/* out[0] = max(x[0..n)) (-inf for n = 0), reset and folded in-stream: the bound amar_gat_lt_f32 takes. */
int amar_colmax_f32(const float *x, int64_t n, float *out, amar_stream_t stream);

/* ---- hybrid-head variants of econfigs/hybrid-gnn-tweaks*.yaml -----------------------
 * amar_attention_mix_f32      FusionLayer('attention') (src/layers/fusion.py:54-68) after the two products
 *                             TA = A . att_weight, TB = B . att_weight (amar_dense_f32, no bias): the softmax over the two
 *                             stacked sources is per feature wa = sigmoid(tanh(TA) - tanh(TB)); out = wa*A + (1-wa)*B
 * amar_attention_mix_bwd_f32  its reverse: dA, dB = the direct paths, dTA, dTB = gradients of the two products
 *                             (all four contiguous [M, D])
 * amar_add3_act_f32           out = act(A + B + C): the residual head, activation(residual(x) + x1 + x2)
 *                             (src/models/hybrid.py:86-89)
 * amar_locality_scale_f32     DGCFConv's LocalityAdaptive (src/layers/dgcf_conv.py:83-102): out = X * sigmoid(w[row]);
 *                             the layer is then amar_spmm_* on the DGCF adjacency (dgcf_conv.py:32-36)
 * amar_locality_scale_bwd_f32 dX (+)= dOut * sigmoid(w), dw[row] = sigmoid'(w[row]) * (dOut[row] . X[row])
 */
int amar_attention_mix_f32(const float *A, int64_t lda, const float *B, int64_t ldb, const float *TA, int64_t ldta,
                           const float *TB, int64_t ldtb, float *out, int64_t ldo, int64_t M, int32_t D, amar_stream_t stream);
int amar_attention_mix_bwd_f32(const float *dOut, int64_t ldd, const float *A, int64_t lda, const float *B, int64_t ldb,
                               const float *TA, int64_t ldta, const float *TB, int64_t ldtb,
                               float *dA, float *dB, float *dTA, float *dTB, int64_t M, int32_t D, amar_stream_t stream);
int amar_add3_act_f32(const float *A, int64_t lda, const float *B, int64_t ldb, const float *C, int64_t ldc, float *out, int64_t ldo,
                      int64_t M, int32_t W, int32_t act, amar_stream_t stream);
int amar_locality_scale_f32(const float *X, int64_t ldx, const float *w, float *out, int64_t ldo, int64_t M, int32_t W,
                            amar_stream_t stream);
int amar_locality_scale_bwd_f32(const float *dOut, int64_t ldd, const float *X, int64_t ldx, const float *w, float *dX, int64_t lddx,
                                float *dw, int64_t M, int32_t W, int32_t accumulate, amar_stream_t stream);

/* ---- training step -------------------------------------------------------
 * What Keras' fit() adds around the forward path for one batch (src/experiment.py:155-188, config.yaml:50-58):
 * reverse-mode derivatives of Dense / GCNConv / LightGCNConv / embedding_lookup, binary cross-entropy,
 * L2 regularisers (src/models/gnn.py:45,293-294) and the Adam update.  The forward kernels above are reused
 * (the SpMM on the transposed image of A_hat — A_hat itself where it is symmetric; dX = dZ . W^T is amar_dense_f32 on the
 * transposed kernel).
 *
 * amar_act_bwd_f32          dZ = dY * act'(Y)        (Y = the layer's OUTPUT; relu / sigmoid / none)
 * amar_wgrad_f32            dW[K,N] = X^T . dZ and/or db[N] = column sums of dZ, reduced in two stages in a fixed
 *                           order (no float atomics); scratch must hold amar_wgrad_scratch_floats(M, K, N) floats
 * amar_bce_grad_f32         Keras backend binary_crossentropy on probabilities (epsilon 1e-7, mean over B):
 *                           loss_terms[i] and dz[i] = dL/dlogit_i through the final sigmoid
 * amar_scatter_add_rows_f32 dst[ids[m] - base, :] += src[m, :]   (gradient of embedding_lookup).  Up to 8 192 ids: without atomics —
 *                           the first position of an id adds the rows of all its positions in position order (one writer per row,
 *                           reproducible bit for bit); longer lists: global float atomics (order-dependent last bits)
 * amar_add_inplace_f32      dst += scale * src on strided [M, W] blocks
 * amar_row_affine_f32       out = (A + B) * scale[row], B optional: GraphSAGE's mean aggregate (sum + self) / count
 *                           (Spektral GraphSageConv, built at src/models/gnn.py:354-361) and its reverse
 * amar_l2norm_fwd_f32       tf.nn.l2_normalize(axis=-1) + activation as GraphSageConv applies them: inv[r] =
 *                           rsqrt(max(sum z^2, 1e-12)), Nrm = z * inv (kept for the reverse pass), Y = act(Nrm)
 * amar_l2norm_bwd_f32       dZ = inv * (dn - Nrm * (Nrm . dn)) with dn = dY * act'(Nrm); dZ = inv * dn where the norm
 *                           was clamped
 * amar_gat_bwd_f32          reverse of amar_gat_layer_f32 (Spektral GATConv, src/models/gnn.py:321-328) given dY = dL/dY:
 *                           dout = dY * [Y > 0] ([n, C] contiguous, also the source of the bias gradient), ds / dt = the
 *                           gradients of the two attention scalars per node, dH = dL/dH including their ds (x) a_self +
 *                           dt (x) a_neigh terms.  row_scratch: 3 * n_rows floats.  Row-wise sums only (no float atomics):
 *                           relies on the edge multiset being symmetric, as build_adjacency_matrix + symmetrize_matrix
 *                           produce it (src/data/preprocess.py:44-170, src/utilities/math.py:6-21).  C in {4,8,16,32,64}.
 * amar_gat_bwd_directed_f32 the same for ANY edge multiset (dataset.symmetric_adjacency: False): the target walk (softmax statistics,
 *                           ds) reads rowptr / colidx, the source walk (dt, dH) reads t_rowptr / t_colidx = the stable transpose
 *                           of that structure.  Passing one structure twice gives amar_gat_bwd_f32 bit for bit.
 * amar_transpose_f32        dst[N,K] = src[K,N]^T
 * amar_adam_f32             keras.optimizers.Adam on a flat parameter: g' = g + 2*l2*w; m, v moments; lr_t = the
 *                           bias-corrected step lr * sqrt(1 - b2^t) / (1 - b1^t);  w -= lr_t * m / (sqrt(v) + epsilon)
 * amar_adam_advance_f32     state[0] = t + 1, state[1] = lr_t for that t (device memory, 2 floats): the step counter of
 *                           keras.optimizers.Adam (`iterations`) kept on the device ...
 * amar_adam_dev_f32         ... and the same update as amar_adam_f32 reading lr_t from state[1], so that a whole batch
 *                           (forward, reverse pass, optimizer) can be captured once as a hipGraph and replayed
 */
int amar_act_bwd_f32(const float *dY, int64_t ldd, const float *Y, int64_t ldy, float *dZ, int64_t ldz,
                     int64_t M, int32_t N, int32_t act, amar_stream_t stream);
int64_t amar_wgrad_scratch_floats(int64_t M, int32_t K, int32_t N);
/* A whole Dense stack forward in ONE launch with every layer's output kept (what model.fit's forward pass needs of a tower / classifier:
 * src/models/dense.py:4-17 called from src/models/basic.py:31-37): y_0 = X[ids] (ids == NULL: X), y_{l+1} = act_l(y_l . W_l + b_l) written to
 * Y[l] (leading dimension ldy[l]: a column slice of a wider buffer realises `Concatenate`), l < n_layers <= 4, every width <= 128
 * (else AMAR_EUNSUPPORTED: layer by layer with amar_dense_f32).  W, bias, Y, ldy, dims (n_layers + 1 widths), acts: HOST arrays of device
 * pointers / values.  Xcopy != NULL: the gathered input rows are also written there (the reverse pass multiplies by them).
 * bias[l] == NULL: layer l has no bias (a zero bias: the same bits as a bias vector of zeros); the `bias` array itself must be given.
 * M = 0: AMAR_OK, nothing is launched.  Workgroups of 16 rows up to M = 4 096, of 64 rows above. */
int amar_dense_stack_f32(const float *X, int64_t ldx, const int32_t *ids, float *Xcopy, int64_t ldxc, int32_t n_layers,
                         const float *const *W, const float *const *bias, const int32_t *dims, const int32_t *acts,
                         float *const *Y, const int64_t *ldy, int64_t M, amar_stream_t stream);
/* Two INDEPENDENT stacks in one launch — the user and the item tower of src/models/basic.py:31-35 inside model.fit: each is 16 workgroups
 * of a 1 024-pair batch and ~18 us as a launch of its own, and a training batch at ML-1M size is a chain of such latencies.  A descriptor
 * holds the arguments of amar_dense_stack_f32 (same meaning, same limits, same error codes); the results are those of two separate calls,
 * bit for bit.  Row form of the pair: 16-row workgroups if BOTH stacks have M <= 4 096, else 64-row workgroups for both (a stack's sums
 * run in ascending k whatever the row form, so a stack that alone would run 16-row workgroups keeps its bits); the first stack's
 * workgroups come first; a stack with M = 0 has none, and nothing is launched if both have none. */
typedef struct amar_dense_stack_desc {
    const float *X; int64_t ldx; const int32_t *ids; float *Xcopy; int64_t ldxc; int32_t n_layers;
    const float *const *W; const float *const *bias; const int32_t *dims; const int32_t *acts; float *const *Y; const int64_t *ldy; int64_t M;
} amar_dense_stack_desc;
int amar_dense_stack_pair_f32(const amar_dense_stack_desc *s0, const amar_dense_stack_desc *s1, amar_stream_t stream);
/* What an amar_dense_stack_f32 call with these arguments does (host only: nothing is launched, the device pointers are looked at for their
 * alignment and for NULL; the host arrays are read).  The launcher calls the same functions, so the two cannot disagree.  Returns what the
 * launcher's argument checks return.
 *   rows       rows per workgroup: 16 (M <= 4 096) or 64
 *   vec_x      X (and Xcopy, if given) moved by 16 bytes: dims[0] and ldx (and ldxc) multiples of 4 floats, 16-byte aligned bases
 *   vec_w[l]   W[l] staged by 16-byte loads: dims[l + 1] a multiple of 4, a 16-byte aligned base (0 for l >= n_layers)
 *   groups     workgroups launched = ceil(M / rows) (0: no launch)
 *   lds_bytes  dynamic LDS asked for: (2 * 64 * (D + 2) + max_l Kp_l * (Np_l + 2)) floats, D = the widest width rounded up to 16,
 *              Kp / Np = dims[l] / dims[l + 1] rounded up to 16 (the same for both row forms) */
typedef struct amar_dense_stack_route_info {
    int32_t rows, vec_x, vec_w[4];
    int64_t groups, lds_bytes;
} amar_dense_stack_route_info;
int amar_dense_stack_route(const float *X, int64_t ldx, const int32_t *ids, float *Xcopy, int64_t ldxc, int32_t n_layers,
                           const float *const *W, const float *const *bias, const int32_t *dims, const int32_t *acts,
                           float *const *Y, const int64_t *ldy, int64_t M, amar_dense_stack_route_info *out);
/* The reverse pass of a whole Dense stack (a tower / the classifier of src/models/basic.py:11-37 inside model.fit) in ONE launch: from
 * dYtop = d(loss)/d(last output) (Ytop = that output; Ytop == NULL: dYtop is already the last pre-activation's gradient) down to
 * dX0 = d(loss)/d(stack input) (or NULL), leaving every layer's dW[l] [K_l, N_l] and db[l] [N_l].  X[l] = layer l's input (X[l+1] is layer
 * l's output), W, dims (n_layers + 1 widths), acts as in amar_dense_stack_f32; n_layers <= 4, widths <= 128, M <= 4 096 rows (else
 * AMAR_EUNSUPPORTED: layer by layer).  workspace: amar_dense_stack_bwd_workspace_floats(M, n_layers, dims) floats of scratch.
 * flags & AMAR_DENSE_BWD_DEFER: dW / db are not written; layer l's partials stay at  workspace + 4 + sum_{j<l} G (K_j N_j + N_j):
 * [G][K_l N_l] then [G][N_l],  G = amar_dense_stack_bwd_groups(M)  (amar_adam_multi_f32 with g_groups = G adds them). */
int64_t amar_dense_stack_bwd_groups(int64_t M);      /* G: the partials per layer a deferred call leaves (one per workgroup: 16 rows each up to M = 1 024, else 64) */
int64_t amar_dense_stack_bwd_workspace_floats(int64_t M, int32_t n_layers, const int32_t *dims);
int amar_dense_stack_bwd_f32(const float *dYtop, int64_t lddy, const float *Ytop, int64_t ldytop, int32_t n_layers,
                             const float *const *X, const int64_t *ldx, const float *const *W, const int32_t *dims, const int32_t *acts,
                             float *dX0, int64_t lddx0, float *const *dW, float *const *db, float *workspace, int32_t flags,
                             int64_t M, amar_stream_t stream);
/* ... and the reverse passes of two independent stacks in one launch (descriptor = the arguments of amar_dense_stack_bwd_f32; each stack
 * with its own workspace; the partial sums of a stack without AMAR_DENSE_BWD_DEFER in `flags` are added by launches behind the shared one).
 * The results are those of two separate calls, bit for bit.  Row form of the pair: both stacks must select the same one (both M <= 1 024:
 * 16-row workgroups; both 1 025 .. 4 096: 64-row workgroups), because a stack's partials are per workgroup; a pair that mixes the two
 * returns AMAR_EUNSUPPORTED before anything is launched. */
typedef struct amar_dense_stack_bwd_desc {
    const float *dYtop; int64_t lddy; const float *Ytop; int64_t ldytop; int32_t n_layers;
    const float *const *X; const int64_t *ldx; const float *const *W; const int32_t *dims; const int32_t *acts;
    float *dX0; int64_t lddx0; float *const *dW; float *const *db; float *workspace; int32_t flags; int64_t M;
} amar_dense_stack_bwd_desc;
int amar_dense_stack_bwd_pair_f32(const amar_dense_stack_bwd_desc *s0, const amar_dense_stack_bwd_desc *s1, amar_stream_t stream);
/* What an amar_dense_stack_bwd_f32 call with these arguments does (host only, as amar_dense_stack_route; `flags` does not change it).
 *   rows       rows per workgroup = rows per partial: 16 (M <= 1 024) or 64 (M <= 4 096; beyond: AMAR_EUNSUPPORTED)
 *   vec_top    dYtop (and Ytop, if given) read by 16-byte loads: dims[n_layers], lddy (and ldytop) multiples of 4, aligned bases
 *   vec_x[l]   X[l] read by 16-byte loads: dims[l] and ldx[l] multiples of 4, an aligned base
 *   vec_w[l]   W[l] read by 16-byte loads: dims[l + 1] a multiple of 4, an aligned base
 *   groups     workgroups launched = amar_dense_stack_bwd_groups(M)
 *   lds_bytes  dynamic LDS asked for (the formula of amar_dense_stack_route_info) */
typedef struct amar_dense_stack_bwd_route_info {
    int32_t rows, vec_top, vec_x[4], vec_w[4];
    int64_t groups, lds_bytes;
} amar_dense_stack_bwd_route_info;
int amar_dense_stack_bwd_route(const float *dYtop, int64_t lddy, const float *Ytop, int64_t ldytop, int32_t n_layers,
                               const float *const *X, const int64_t *ldx, const float *const *W, const int32_t *dims, const int32_t *acts,
                               float *dX0, int64_t lddx0, float *const *dW, float *const *db, float *workspace, int32_t flags,
                               int64_t M, amar_dense_stack_bwd_route_info *out);
/* The reverse pass of ONE Dense layer (Keras Dense inside model.fit: src/models/dense.py:4-17, src/experiment.py:183-188) in two launches
 * instead of four:
 *     dZ = dY * act'(Y)   (Y = the layer's OUTPUT; act == AMAR_ACT_NONE or Y == NULL: dY already is dZ)
 *     dX[M, K] = dZ . W^T (dX == NULL: skipped)      dW[K, N] = X^T . dZ (dW == NULL: skipped)      db[N] = column sums of dZ (or NULL)
 * Both products on the f32 matrix instruction; the workgroups (one per 64 rows) leave partial weight / bias gradients in the workspace, which
 * the second launch adds in workgroup order (a FIXED order: no float atomics, results reproducible bit for bit).  Past 64 workgroups (M >
 * 4 096: the reverse pass of a convolution layer runs over every node of the graph) operands of at most 32 columns take a row-walking
 * kernel instead of the tile kernel, and a launch in between folds the raw partials, in workgroup order, into at most 64 (G below).
 * K, N <= 128 (wider layers: AMAR_EUNSUPPORTED — use amar_act_bwd_f32 + amar_wgrad_f32 + amar_dense_f32 with AMAR_DENSE_WT).
 * workspace: amar_dense_bwd_workspace_floats(M, K, N) floats owned by the caller (scratch: any contents); two calls in flight on
 * different streams must not share one.
 * act | AMAR_DENSE_BWD_DEFER: the second launch is left out — dW / db (still non-NULL to request them) are NOT written; the partials stay
 * in the workspace as  workspace + 4: [G][K * N] (if dW)  then [G][N] (if db),  G = amar_dense_bwd_groups(M), for a consumer that adds them
 * itself (amar_adam_multi_f32 with g_groups = G). */
#define AMAR_DENSE_BWD_DEFER 0x100
/* act | AMAR_DENSE_BWD_ACCUM_DX: dX += dZ . W^T instead of dX = (a layer whose input already carries a gradient: the concat slices of a
 * convolution stack).  dZ != NULL: the pre-activation gradient dZ itself is also written ([M, N], leading dimension lddz) — a GCN layer
 * multiplies it by A_hat before the weight gradient — so that act', its bias gradient and dZ are one launch (X, W, dX, dW all NULL). */
#define AMAR_DENSE_BWD_ACCUM_DX 0x200
int64_t amar_dense_bwd_groups(int64_t M);
int64_t amar_dense_bwd_workspace_floats(int64_t M, int32_t K, int32_t N);
/* Which kernel an amar_dense_bwd_f32 call with these arguments takes (host only: nothing is launched, the pointers are looked at for
 * their alignment and for NULL; `act` may carry the flags above).  The launcher asks the same function, so the two cannot disagree.
 * Returns what the launcher's argument checks return (a workspace is taken as given).
 *   kernel           AMAR_DENSE_BWD_KERNEL_TILE (64-row tiles, matrix instructions) or _ROWS (the row-walking kernel: M > 4 096, K, N <= 32,
 *                    dY / Y / W / dX / dZ 16-byte aligned with leading dimensions that are multiples of 4 floats)
 *   mt               tile kernel: 16 x 16 tiles of dW per wave, 4 or 16 (0 for the row-walking kernel)
 *   kp, np           row-walking kernel: its compile-time widths, each 8, 16 or 32 (0 for the tile kernel)
 *   vec              operands read by 16-byte loads (tile kernel: all of them or none; row-walking kernel: always 1)
 *   x_scalar         row-walking kernel: X read by single floats (K not a multiple of 4, or X unaligned)
 *   subtiles         tile kernel: 64-row tiles per workgroup (0 for the row-walking kernel)
 *   launched_groups  workgroups of the main launch = raw partials
 *   fold             raw partials added per partial the caller sees (1: the workgroups write the visible partials themselves)
 *   fold_launch      1 if a launch that folds the raw partials follows (only where dW or db is asked for)
 *   out_groups       amar_dense_bwd_groups(M) */
#define AMAR_DENSE_BWD_KERNEL_TILE 0
#define AMAR_DENSE_BWD_KERNEL_ROWS 1
typedef struct amar_dense_bwd_route_info {
    int32_t kernel, mt, kp, np, vec, x_scalar, subtiles, fold, fold_launch;
    int64_t launched_groups, out_groups;
} amar_dense_bwd_route_info;
int amar_dense_bwd_route(const float *X, int64_t ldx, const float *Y, int64_t ldy, const float *dY, int64_t lddy, const float *W, int32_t act,
                         float *dX, int64_t lddx, float *dW, float *db, float *dZ, int64_t lddz, int64_t M, int32_t K, int32_t N,
                         amar_dense_bwd_route_info *out);
int amar_dense_bwd_f32(const float *X, int64_t ldx, const float *Y, int64_t ldy, const float *dY, int64_t lddy, const float *W,
                       int32_t act, float *dX, int64_t lddx, float *dW, float *db, float *dZ, int64_t lddz, float *workspace,
                       int64_t M, int32_t K, int32_t N, amar_stream_t stream);
/* Which kernel an amar_wgrad_f32 call with these arguments takes (host only: nothing is launched, the pointers are looked at for NULL
 * and for their alignment).  The launcher asks the same function.  Returns what the launcher's argument checks return (a scratch
 * buffer is taken as given).
 *   kernel          AMAR_WGRAD_KERNEL_MFMA (one workgroup per 32 x 32 tile of dW walks all rows on the matrix instruction: dW asked for,
 *                   M <= 16 384, K, N, ldx, ldz multiples of 4, X and dZ 16-byte aligned, at least 16 tiles) or _PARTIAL (16 x 16 tiles
 *                   over row chunks, then a reduction launch in chunk order)
 *   wg_rows         partial: rows per chunk, 128 ... 512 in steps of 64 (max(128, min(512, ceil(floor(M / 64) / 64) * 64))); mfma: 0
 *   grid_k, grid_n  tiles of dW along K and N (partial: 16 wide, grid_k = 1 without dW; mfma: 32 wide)
 *   chunks          partial: row chunks = partial sums per element; mfma: 1
 *   scratch_floats  floats of `scratch` the call writes: chunks * (K N + N) with K taken as 0 without dW; mfma: 0 */
#define AMAR_WGRAD_KERNEL_PARTIAL 0
#define AMAR_WGRAD_KERNEL_MFMA 1
typedef struct amar_wgrad_route_info {
    int32_t kernel, wg_rows, grid_k, grid_n;
    int64_t chunks, scratch_floats;
} amar_wgrad_route_info;
int amar_wgrad_route(const float *X, int64_t ldx, const float *dZ, int64_t ldz, int64_t M, int32_t K, int32_t N, float *dW, float *db,
                     amar_wgrad_route_info *out);
int amar_wgrad_f32(const float *X, int64_t ldx, const float *dZ, int64_t ldz, int64_t M, int32_t K, int32_t N,
                   float *dW, float *db, float *scratch, amar_stream_t stream);
int amar_bce_grad_f32(const float *p, int64_t ldp, const float *y, float *dz, float *loss_terms, int64_t B, amar_stream_t stream);
/* Which kernel an amar_scatter_add_rows_f32 call over M ids of W columns takes (host only; the launcher asks the same function).
 *   kernel              AMAR_SCATTER_KERNEL_OWNER (M <= 8 192: no atomics, fixed order) or _ATOMIC
 *   blocks              workgroups launched (owner: min(ceil(M / 4), 1 024) of four wavefronts; 0 for M = 0: nothing is launched)
 *   lds_bytes           owner: the id list, 4 M bytes; atomic: 0
 *   positions_per_wave  owner: positions the first wavefront walks (2 from M = 4 097 on); atomic: 0 */
#define AMAR_SCATTER_KERNEL_OWNER 0
#define AMAR_SCATTER_KERNEL_ATOMIC 1
typedef struct amar_scatter_add_rows_route_info {
    int32_t kernel, blocks, lds_bytes, positions_per_wave;
} amar_scatter_add_rows_route_info;
int amar_scatter_add_rows_route(int64_t M, int32_t W, amar_scatter_add_rows_route_info *out);
int amar_scatter_add_rows_f32(const float *src, int64_t lds, const int32_t *ids, int32_t base, float *dst, int64_t ldd,
                              int64_t M, int32_t W, amar_stream_t stream);
int amar_add_inplace_f32(float *dst, int64_t ldd, const float *src, int64_t lds, int64_t M, int32_t W, float scale, amar_stream_t stream);
int amar_row_affine_f32(const float *A, int64_t lda, const float *B, int64_t ldb, const float *scale, float *out, int64_t ldo,
                        int64_t M, int32_t W, amar_stream_t stream);
int amar_l2norm_fwd_f32(const float *Z, int64_t ldz, float *Nrm, int64_t ldn, float *inv, float *Y, int64_t ldy,
                        int64_t M, int32_t C, int32_t act, amar_stream_t stream);
int amar_l2norm_bwd_f32(const float *dY, int64_t ldd, const float *Nrm, int64_t ldn, const float *inv, float *dZ, int64_t ldz,
                        int64_t M, int32_t C, int32_t act, amar_stream_t stream);
int amar_gat_bwd_f32(const int32_t *rowptr, const int32_t *colidx, const float *H, int64_t ldh, int32_t C,
                     const float *s_self, const float *s_neigh, const float *Y, int64_t ldy, const float *dY, int64_t ldd,
                     const float *bias, const float *a_self, const float *a_neigh,
                     float *dout, float *row_scratch, float *ds, float *dt, float *dH, int64_t lddh,
                     int32_t self_loop, int32_t n_rows, amar_stream_t stream);
int amar_gat_bwd_directed_f32(const int32_t *rowptr, const int32_t *colidx, const int32_t *t_rowptr, const int32_t *t_colidx,
                              const float *H, int64_t ldh, int32_t C,
                              const float *s_self, const float *s_neigh, const float *Y, int64_t ldy, const float *dY, int64_t ldd,
                              const float *bias, const float *a_self, const float *a_neigh,
                              float *dout, float *row_scratch, float *ds, float *dt, float *dH, int64_t lddh,
                              int32_t self_loop, int32_t n_rows, amar_stream_t stream);
/* Reverse of amar_gat_heads_f32 given dY = dL/dY, with the structure of amar_gat_bwd_directed_f32: a target walk on rowptr / colidx
 * (softmax statistics per (row, head), ds), then a source walk on t_rowptr / t_colidx = the stable transpose (dt, dHd); a symmetric
 * edge multiset passes the one structure twice.  With g_i = dY_i * [Y_i > 0]:
 *     concat != 0:  g_ih = g_i[h*C : (h+1)*C],  out[i,h,:] = Y[i, h*C : (h+1)*C] - bias   (only read where Y > 0)
 *     concat == 0:  g_ih = g_i / heads,         out[i,h,:] = out_tape[i, h, :]            (the forward's tape; required)
 *     c_ih = g_ih . out[i,h,:],   d e_ijh = alpha_ijh (g_ih . Hd[j,h,:] - c_ih),   d pre_ijh = d e_ijh * LeakyReLU'(S[i,h] + S[j,heads+h])
 *     dS[i, h] = sum_j d pre_ijh,   dS[j, heads + h] = sum_i d pre_ijh                      ([n_rows, 2*heads], the layout of S)
 *     dHd[j,h,:] = sum_i alpha_ijh g_ih + dS[j,h] a_self[:,h] + dS[j,heads+h] a_neigh[:,h]
 * dout = g_i in Y's own width ([n_rows, heads*C] or [n_rows, C], contiguous): the source of the bias gradient.  row_scratch:
 * 3 * heads * n_rows floats.  Row-wise sums in a fixed order, no float atomics: two runs give the same bits.  C % 4 == 0 and
 * heads*C <= 64; other shapes AMAR_EUNSUPPORTED. */
int amar_gat_heads_bwd_f32(const int32_t *rowptr, const int32_t *colidx, const int32_t *t_rowptr, const int32_t *t_colidx,
                           const float *Hd, int64_t ldh, int32_t heads, int32_t C, const float *S,
                           const float *Y, int64_t ldy, const float *dY, int64_t ldd, const float *bias,
                           const float *a_self, const float *a_neigh, const float *out_tape,
                           float *dout, float *row_scratch, float *dS, float *dHd, int64_t lddh,
                           int32_t concat, int32_t self_loop, int32_t n_rows, amar_stream_t stream);
int amar_transpose_f32(const float *src, int32_t K, int32_t N, float *dst, amar_stream_t stream);
int amar_adam_f32(float *w, const float *g, float *m, float *v, int64_t n, float lr_t, float beta_1, float beta_2,
                  float epsilon, float l2, amar_stream_t stream);
int amar_adam_advance_f32(float *state, float learning_rate, float beta_1, float beta_2, amar_stream_t stream);
/* All parameters of a model in one launch (a table of slots in device memory; slot k owns blocks [first_block_k,
 * first_block_{k+1}) of 1024 elements each, first_block_0 = 0, total_blocks = sum of ceil(n / 1024)); the update of
 * amar_adam_dev_f32.  If loss_acc != NULL, reg_scale * l2 * sum(w^2) of the pre-update weights is added to *loss_acc (the
 * regularisation part of the loss Keras reports).  amar_sum_into_f32: *acc += scale * sum(x) (the data part). */
typedef struct amar_adam_slot { float *w; const float *g; float *m; float *v; int64_t n; int64_t first_block; float l2; int32_t g_groups; } amar_adam_slot;
/* g_groups == 0: g[n] is the gradient.  g_groups = G > 0: g holds G partial gradients [G][n] (what amar_dense_bwd_f32 leaves in its
 * workspace with AMAR_DENSE_BWD_DEFER) and the gradient is their sum in the order 0 .. G-1 — the reduction launch of every layer folded
 * into the one Adam launch (same order of additions as the explicit reduction: the same bits). */
int amar_adam_multi_f32(const amar_adam_slot *slots, int32_t n_slots, int64_t total_blocks, const float *state, float beta_1,
                        float beta_2, float epsilon, float reg_scale, float *loss_acc, amar_stream_t stream);
int amar_sum_into_f32(const float *x, int64_t n, float scale, float *acc, amar_stream_t stream);
int amar_adam_dev_f32(float *w, const float *g, float *m, float *v, int64_t n, const float *state, float beta_1, float beta_2,
                      float epsilon, float l2, amar_stream_t stream);

/* ---- the optimizers of tf.keras.optimizers as rules (src/experiment.py:111,130-134: `parameters.optimizer.name` is a free choice) -------
 * Adam, SGD, RMSprop, Adagrad, Adamax, Nadam and Adam(amsgrad=True): a step counter and the step-dependent scalars in device memory, one
 * launch for every parameter of a model, a single-tensor form reading the same state.  The Adam entry points above are the AMAR_OPT_ADAM
 * instantiations of the same kernels, over their own slot struct and two floats of state: the same bits either way.  The formulas below are the contract; they restate Keras 2's optimizer_v2 classes.  Common to all rules: g' = g + 2 l2 w
 * first (the L2 regulariser's gradient), t = 1 for the first step, `step` = state[1] of this step.  s0, s1, s2 are the rule's state arrays
 * in the order given; a rule neither reads nor writes the arrays it does not have (their pointers may be NULL).
 *
 * AMAR_OPT_SGD      momentum == 0 (no array):       w -= lr g'
 *                   momentum > 0 (s0 = a):          a = momentum a - lr g';  w += a
 *                   ... with AMAR_OPT_NESTEROV:     a as above;  w += momentum a - lr g'  (the new a; without momentum the flag does nothing)
 * AMAR_OPT_RMSPROP  s0 = rms:                       rms = rho rms + (1 - rho) g'^2;  d = rms
 *                   AMAR_OPT_CENTERED (s1 = mg):    mg = rho mg + (1 - rho) g';  d = max(rms - mg^2, 0)  (the max is a stated deviation: it
 *                                                   differs from TensorFlow only where TensorFlow returns NaN)
 *                   momentum == 0:                  w -= lr g' / (sqrt(d) + epsilon)
 *                   momentum > 0 (next array = mom): mom = momentum mom + lr g' / sqrt(d + epsilon);  w -= mom   (TensorFlow's fused op
 *                                                   puts epsilon inside the root)
 * AMAR_OPT_ADAGRAD  s0 = acc (the caller fills it with initial_accumulator_value):   acc += g'^2;  w -= lr g' / (sqrt(acc) + epsilon)
 * AMAR_OPT_ADAMAX   s0 = m, s1 = u:                 m = b1 m + (1 - b1) g';  u = max(b2 u, |g'|);  w -= step m / (u + epsilon),
 *                                                   step = lr / (1 - b1^t)
 * AMAR_OPT_NADAM    s0 = m, s1 = v:                 mu_t = b1 (1 - 0.5 0.96^(0.004 t));  P_t = P_{t-1} mu_t, P_0 = 1;
 *                                                   m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
 *                                                   w -= lr ((1 - mu_t) g' / (1 - P_t) + mu_{t+1} m / (1 - P_t mu_{t+1})) / (sqrt(v / (1 - b2^t)) + epsilon)
 * AMAR_OPT_AMSGRAD  s0 = m, s1 = v, s2 = vhat:      Adam's m and v;  vhat = max(vhat, v);  w -= step m / (sqrt(vhat) + epsilon),
 *                                                   step = Adam's lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
 * AMAR_OPT_ADAM     s0 = m, s1 = v:                 m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  w -= step m / (sqrt(v) + epsilon),
 *                                                   step = lr_t as above (amar_adam_dev_f32 / amar_adam_multi_f32)
 *
 * The device state is AMAR_OPTIM_STATE_FLOATS floats, zero before the first step:
 *   [0] t   [1] step (lr; Adamax, AMSGrad, Adam: as above)   and for Nadam   [2] mu_t   [3] mu_{t+1}   [4] P_t (the running product: read back
 *   at the next step)   [5] 1 - b2^t   [6] lr (1 - mu_t) / (1 - P_t)   [7] lr mu_{t+1} / (1 - P_t mu_{t+1})   (0 for the other rules).
 * amar_optim_advance_f32 (one thread, ordinary stores) sets [0] = t + 1 and the scalars of that step, computed in double from the float32
 * hyper-parameters.  The update kernels read lr from [1], Nadam's also [3], [5], [6] and [7]: nothing that changes from step to
 * step is an argument, so a captured training batch replays as it is.  AMAR_OPT_ADAM reads and writes [0] and [1] alone (the state of
 * the amar_adam_* entry points, which is those two floats) and leaves [2] .. [7] as they are.
 * The single-tensor and the multi-slot form share one element function per rule (fused products written out, nothing else fused): they
 * give the same bits on the same element.  Unknown rule, flags the rule does not have, momentum < 0, null pointers (of arrays the rule
 * has), negative sizes: AMAR_EINVAL. */
#define AMAR_OPT_SGD      1
#define AMAR_OPT_RMSPROP  2
#define AMAR_OPT_ADAGRAD  3
#define AMAR_OPT_ADAMAX   4
#define AMAR_OPT_NADAM    5
#define AMAR_OPT_AMSGRAD  6
#define AMAR_OPT_ADAM     7
#define AMAR_OPT_NESTEROV 0x100   /* flag of AMAR_OPT_SGD     */
#define AMAR_OPT_CENTERED 0x200   /* flag of AMAR_OPT_RMSPROP */
#define AMAR_OPTIM_STATE_FLOATS 8
/* HOST struct, read when the call is made; a rule ignores the members it does not use */
typedef struct amar_optim_hyper { float learning_rate, momentum, rho, beta_1, beta_2, epsilon; } amar_optim_hyper;
/* how many state arrays (0 .. 3) a slot of this rule needs */
int amar_optim_state_arrays(int32_t rule, int32_t flags, float momentum);
int amar_optim_advance_f32(float *state, int32_t rule, int32_t flags, const amar_optim_hyper *hyper, amar_stream_t stream);
int amar_optim_f32(int32_t rule, int32_t flags, const amar_optim_hyper *hyper, float *w, const float *g, float *s0, float *s1, float *s2,
                   int64_t n, const float *state, float l2, amar_stream_t stream);
/* All parameters of a model in one launch: the slot table (device memory), blocks of 1024 elements, first_block, g_groups (partials [G][n]
 * added in the order 0 .. G-1: the bits of an explicit reduction), reg_scale and loss_acc mean what they mean for amar_adam_multi_f32. */
typedef struct amar_optim_slot { float *w; const float *g; float *s0; float *s1; float *s2; int64_t n; int64_t first_block; float l2; int32_t g_groups; } amar_optim_slot;
int amar_optim_multi_f32(int32_t rule, int32_t flags, const amar_optim_hyper *hyper, const amar_optim_slot *slots, int32_t n_slots,
                         int64_t total_blocks, const float *state, float reg_scale, float *loss_acc, amar_stream_t stream);

/* ---- learning-rate schedules: tf.keras.optimizers.schedules, Keras 2's optimizer argument `decay`, and a rate the host sets --------------
 * The learning rate of the two advance entry points above is an argument, so a captured training batch has it baked in.  Their siblings
 * below take it from device memory instead and evaluate a schedule inside the same one-thread launch: a captured batch then replays
 * under a rate that follows the step counter, or that the host rewrites between replays, without being captured again.
 *
 * lr_state: AMAR_LR_STATE_FLOATS floats in device memory.
 *   [0] the base rate: what AMAR_LR_CONSTANT returns.  The host writes it; no kernel does.
 *   [1] the rate the last step used: written by the advance kernels, for the host to read.
 * The rate of the ZERO-BASED step s (the first step has s = 0, as Keras' `iterations`), computed in double from the float32 members
 * and rounded once to float32 (Keras holds the rate as float32), without fused products.  lr0 = initial_learning_rate, d = decay_steps:
 *   AMAR_LR_CONSTANT      lr_state[0]
 *   AMAR_LR_EXPONENTIAL   lr0 * decay_rate^p,  p = s / d;  AMAR_LR_STAIRCASE: p = floor(s / d)                  (ExponentialDecay)
 *   AMAR_LR_INVERSE_TIME  lr0 / (1 + decay_rate * p),  p as above                                                (InverseTimeDecay;
 *                         Keras 2's optimizer argument `decay` is this with d = 1 and decay_rate = decay)
 *   AMAR_LR_POLYNOMIAL    (lr0 - end_learning_rate) * (1 - p)^power + end_learning_rate,  p = min(s, d) / d;     (PolynomialDecay)
 *                         AMAR_LR_CYCLE: p = s / (d * (s == 0 ? 1 : ceil(s / d))), without the min
 *   AMAR_LR_COSINE        lr0 * ((1 - alpha) * 0.5 * (1 + cos(pi * (min(s, d) / d))) + alpha)                    (CosineDecay)
 *   AMAR_LR_PIECEWISE     values[i] for the first i < n_boundaries with s <= boundaries[i], values[n_boundaries] if there is none
 *                         (PiecewiseConstantDecay): 1 <= n_boundaries <= AMAR_LR_MAX_BOUNDARIES, one value more than boundaries
 * A kind ignores the members it does not use.  The step counter is state[0] of the optimizer state, a float: it counts exactly up to
 * 2^24 = AMAR_LR_MAX_STEP steps, and so do the boundaries; a run longer than that is outside this contract.
 * Unknown kind, a flag the kind does not have, decay_steps <= 0 (or NaN) where the kind divides by it, n_boundaries outside
 * 1 .. 16, null pointers: AMAR_EINVAL. */
#define AMAR_LR_CONSTANT     0
#define AMAR_LR_EXPONENTIAL  1
#define AMAR_LR_INVERSE_TIME 2
#define AMAR_LR_POLYNOMIAL   3
#define AMAR_LR_COSINE       4
#define AMAR_LR_PIECEWISE    5
#define AMAR_LR_STAIRCASE 0x1     /* flag of AMAR_LR_EXPONENTIAL and AMAR_LR_INVERSE_TIME */
#define AMAR_LR_CYCLE     0x2     /* flag of AMAR_LR_POLYNOMIAL */
#define AMAR_LR_MAX_BOUNDARIES 16
#define AMAR_LR_STATE_FLOATS 2
#define AMAR_LR_MAX_STEP 16777216
/* HOST struct, read when the call is made (the kernels receive it by value) */
typedef struct amar_lr_schedule {
    int32_t kind, flags;
    float initial_learning_rate, decay_steps, decay_rate, end_learning_rate, power, alpha;
    int32_t n_boundaries;
    float boundaries[AMAR_LR_MAX_BOUNDARIES], values[AMAR_LR_MAX_BOUNDARIES + 1];
} amar_lr_schedule;
/* out[i] = the rate of step first_step + i, i < n (one thread each; first_step >= 0, first_step + n <= AMAR_LR_MAX_STEP; n = 0: AMAR_OK,
 * nothing is launched).  The advance entry points below call the same device function: the same bits. */
int amar_lr_rates_f32(const amar_lr_schedule *sched, const float *lr_state, int64_t first_step, int64_t n, float *out, amar_stream_t stream);
/* amar_adam_advance_f32 / amar_optim_advance_f32 with the rate of step s = state[0] in place of the learning-rate argument (one thread,
 * one launch, ordinary stores): lr_state[1] = that rate, then state[0] = s + 1 and the step-dependent scalars exactly as those entry
 * points form them from a float32 rate.  hyper->learning_rate is not read.  Under AMAR_LR_CONSTANT with lr_state[0] = lr every float of
 * `state` equals, bit for bit, what the entry point with the argument lr writes. */
int amar_adam_advance_lr_f32(float *state, const amar_lr_schedule *sched, float *lr_state, float beta_1, float beta_2, amar_stream_t stream);
int amar_optim_advance_lr_f32(float *state, int32_t rule, int32_t flags, const amar_optim_hyper *hyper, const amar_lr_schedule *sched,
                              float *lr_state, amar_stream_t stream);

/* ---- gradient clipping: clipvalue, clipnorm, global_clipnorm of every tf.keras optimizer (Keras 2.7 / 2.8 OptimizerV2, restated) ---------
 * The clipped quantity is the finished gradient of (data loss + regularisation losses), per parameter tensor (slot):
 *   gi = fmaf(2 l2, w, g[0] + g[1] + ... + g[G-1])     the partials added in the order 0 .. G-1, as the optimizer launches add them
 * AMAR_CLIP_VALUE        gi <- min(max(gi, -clip), clip)
 * AMAR_CLIP_NORM         gi <- gi * s,  s = clip / max(||gi||_2, clip)                      one s per slot
 * AMAR_CLIP_GLOBAL_NORM  gi <- gi * s,  s = clip / max(sqrt(sum over slots ||gi||_2^2), clip)   one s for all slots
 * s is formed in float32 from a float32 sum of squares, as (norm > clip ? clip / norm : 1).  This differs from TensorFlow's
 * (g * clip) / max(norm, clip) and clip * min(1 / norm, 1 / clip) by rounding only, and where the clip does not bind s == 1.0f exactly:
 * no bit of a gradient changes.  A zero gradient has norm 0 and s = 1 (no NaN is made); non-finite gradients propagate, nothing special
 * is done for them.
 * The slot table (device memory) is partitioned as the optimizer slot tables are: slot k owns blocks [first_block_k, first_block_{k+1}) of
 * 1024 elements, first_block_0 = 0, total_blocks = sum of ceil(n / 1024); g_groups == 0: g[n] is the gradient, g_groups = G > 0: g
 * holds G partials [G][n].  After the call g[0 .. n) of every slot holds the clipped finished gradient and the groups 1 .. G-1 are as
 * they were; if loss_acc != NULL, reg_scale * l2 * sum(w^2) has been added to *loss_acc (the expression of the optimizer launches).
 * The optimizer launch that follows runs on a table whose slots have g_groups = 0 and l2 = 0: fmaf(0, w, g) == g, so it applies the
 * clipped gradient as it is, and it is not given loss_acc a second time.
 * Three launches: finish (gi into group 0; VALUE clamps and is done; per block the sum of squares into the workspace), scales (one
 * workgroup per slot, or one in all, adds the block sums in ascending block order with a fixed tree and writes s), apply (g *= s).
 * No float atomic takes part in a norm: the same inputs give the same bits on every run, eagerly or replayed from a captured graph,
 * and every value that depends on the step lives in device memory (only mode and clip are arguments).
 * workspace: the number of floats the _workspace_floats function returns (total_blocks + n_slots; VALUE does not use it, NULL allowed).
 * norms: NULL, or [n_slots] (NORM) / [1] (GLOBAL_NORM) floats that receive the measured norms (before scaling); VALUE ignores it.
 * Unknown mode, clip not > 0 (NaN included), NULL tables, n_slots < 1, total_blocks < 1 or > 2^31 - 1: AMAR_EINVAL. */
#define AMAR_CLIP_VALUE       1
#define AMAR_CLIP_NORM        2
#define AMAR_CLIP_GLOBAL_NORM 3
typedef struct amar_clip_slot { const float *w; float *g; int64_t n; int64_t first_block; float l2; int32_t g_groups; } amar_clip_slot;
int64_t amar_grad_clip_workspace_floats(int32_t n_slots, int64_t total_blocks);
int amar_grad_clip_f32(int32_t mode, float clip, const amar_clip_slot *slots, int32_t n_slots, int64_t total_blocks,
                       float *workspace, float *norms, float reg_scale, float *loss_acc, amar_stream_t stream);

/* ---- BPR training (utilities/losses.py:BPRLoss, data/datasets.py:UserItemGraphPosNegSample) ----------------------------------
 * amar_bpr_grad_f32    the pairwise loss of src/utilities/losses.py:15-25 on the probability column p ([B], or a strided [B, 1] with
 *                      leading dimension ldp): h = B / 2 (an odd B drops its last element), s_j = sigmoid(p[j] - p[h + j]),
 *                      loss = -mean_{j<h} log s_j.  loss_terms[j] = (B / h) * (-log s_j), every other term 0 (so sum = B * loss, as
 *                      amar_bce_grad_f32's terms); dz = d(loss)/d(logit) through the final sigmoid: dz[j] = -(1 - s_j) p_j (1 - p_j) / h,
 *                      dz[h + j] = (1 - s_j) p_{h+j} (1 - p_{h+j}) / h, 0 for the dropped element.  B = 1: zero loss and gradient.
 *                      One lane per pair, no atomics: reproducible bit for bit.  dz and loss_terms are contiguous [B].
 * amar_bpr_sample_i32  one BPR batch of h draws into u[2h], items[2h] and (y != NULL) y[2h] = [1]*h + [0]*h, the layout of the
 *                      reference's __getitem__ (datasets.py:286-306): u[2j] = u[2j+1] = user_j, items[j] = pos_j, items[h+j] = neg_j.
 *                      Draw j: Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (j, s & 0xffffffff, s >> 32, 0),
 *                      s = *step read from DEVICE memory; word 0 -> user_j = (uint64(w0) * n_users) >> 32, word 1 -> pos_j =
 *                      pos_ids[pos_ptr[user_j] + ((uint64(w1) * n_pos) >> 32)], word 2 -> neg_j likewise from the negative-candidate CSR.
 *                      advance != 0: *step = s + 1 after the batch (a replayed graph draws new ids every step).  CSR row pointers
 *                      [n_users + 1] and int32 node ids; every user row of both lists must be non-empty (the caller checks: the
 *                      kernel reads without bounds checks).  One workgroup of 256 lanes. */
int amar_bpr_grad_f32(const float *p, int64_t ldp, float *dz, float *loss_terms, int64_t B, amar_stream_t stream);
int amar_bpr_sample_i32(const int32_t *pos_ptr, const int32_t *pos_ids, const int32_t *neg_ptr, const int32_t *neg_ids,
                        int32_t n_users, uint64_t seed, uint64_t *step, int32_t advance, int32_t h,
                        int32_t *u, int32_t *items, float *y, amar_stream_t stream);

/* ---- BPR triples (data/datasets.py:UserItemGraphTriplets): both items of a pair scored against the user they were drawn for --------
 * amar_bpr_sample_triplets_i32  one batch of h triples (user, pos, neg) into u[2h], items[2h] and (y != NULL) y[2h] = [1]*h + [0]*h:
 *                      u[t] = u[h + t] = user_t, items[t] = pos_t, items[h + t] = neg_t, so amar_bpr_grad_f32's pair (t, h + t) is one
 *                      user's positive against its own negative.  K = n_negatives triples share a draw: P = h / K draws, triple
 *                      t = j * K + k belongs to draw j.  Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), s = *step read from
 *                      DEVICE memory, pick(w, n) = (uint64(w) * n) >> 32.
 *                        draw j, counter (j, s & 0xffffffff, s >> 32, 0):
 *                          mode 0 (by user)         user = pick(w0, n_users), pos = pos_ids[pos_ptr[user] + pick(w1, n_pos(user))]
 *                          mode 1 (by interaction)  e = pick(w0, pos_ptr[n_users]), user = the largest r with pos_ptr[r] <= e (binary
 *                                                   search), pos = pos_ids[e]
 *                        triple t, counter (t, s & 0xffffffff, s >> 32, 1): with d the length of the user's exclusion row and
 *                          e_q = excl_ids[excl_ptr[user] + q] - item_base:  r = pick(w0, n_items - d), m = #{q : e_q - q <= r} (e_q - q
 *                          never decreases: one binary search), neg = item_base + r + m — the r-th item outside the row, exactly uniform
 *                          over the complement, no rejection loop.
 *                      advance != 0: *step = s + 1 after the batch.  CSR row pointers [n_users + 1], int32 node ids; exclusion rows
 *                      strictly ascending, inside [item_base, item_base + n_items) and shorter than n_items, positive rows non-empty
 *                      (the caller checks: the kernel reads without bounds checks).  One workgroup of 256 lanes.
 *                      NULL pointer (y excepted), n_users / n_items / h / n_negatives < 1, h % n_negatives != 0, mode not 0 or 1:
 *                      AMAR_EINVAL. */
int amar_bpr_sample_triplets_i32(const int32_t *pos_ptr, const int32_t *pos_ids, const int32_t *excl_ptr, const int32_t *excl_ids,
                                 int32_t n_users, int32_t n_items, int32_t item_base, int32_t n_negatives, int32_t mode, uint64_t seed,
                                 uint64_t *step, int32_t advance, int32_t h, int32_t *u, int32_t *items, float *y,
                                 amar_stream_t stream);

/* ---- listwise ranking losses on the triplet sampler's groups (utilities/losses.py: SampledSoftmaxLoss, HardestNegativeBPRLoss,
 *      MarginRankingLoss) ---------------------------------------------------------------------------------------------------------
 * amar_group_loss_grad_f32  in amar_bpr_grad_f32's place and conventions, on amar_bpr_sample_triplets_i32's layout: h = B / 2 (an odd B
 *                      drops its last element), G = h / K groups; group g has the positive a = p[g K] and the negatives
 *                      b_k = p[h + g K + k], k < K (rows g K + 1 .. g K + K - 1 repeat the positive's pair and carry nothing).
 *                        AMAR_GROUP_SOFTMAX  l_g = -a / t + log(exp(a / t) + sum_k exp(b_k / t)), t = hyper > 0, evaluated with
 *                                            the group's maximum M subtracted: s = sum_k exp((b_k - M) / t), S = exp((a - M) / t) + s,
 *                                            l_g = log1p(s) where a = M, else (M - a) / t + log S; dl/da = -(s / S) / t,
 *                                            dl/db_k = (exp((b_k - M) / t) / S) / t
 *                        AMAR_GROUP_HARDEST  l_g = -log sigmoid(a - max_k b_k); the negative side's gradient goes to the LOWEST k
 *                                            that attains the maximum, every other negative gets 0 (hyper is not read)
 *                        AMAR_GROUP_MARGIN   l_g = (1 / K) sum_k max(0, (m - a) + b_k), m = hyper >= 0; a hinge that is not strictly
 *                                            positive contributes no gradient
 *                      loss = mean_g l_g.  loss_terms[g K] = (B / G) l_g and every other term 0 (sum = B x loss);
 *                      dz[i] = (1 / G) dl_g/dp_i . p_i (1 - p_i): the positive's whole gradient on row g K, exactly 0 on its copies and
 *                      on the dropped trailing element.  dz and loss_terms contiguous [B]; p [B] or a strided column (ldp).
 *                      B = 1: zeros.  AMAR_EINVAL: K < 1, h % K != 0, an unknown kind, t <= 0, m < 0 (or either not a number).
 *                      One launch, float32, no atomics.  K <= 32: a group takes a segment of the next power of two >= K lanes, several
 *                      groups per wavefront; K > 32: one wavefront per group, lane l takes k = l, l + 64, ... in ascending order.
 *                      Every reduction is a lane-local ascending sum followed by an xor butterfly inside the segment, so a group's
 *                      bits depend on its own floats, K and hyper only — not on the grid, the wavefront or the group's place in the
 *                      batch. */
#define AMAR_GROUP_SOFTMAX 0
#define AMAR_GROUP_HARDEST 1
#define AMAR_GROUP_MARGIN  2
int amar_group_loss_grad_f32(int32_t kind, float hyper, const float *p, int64_t ldp, float *dz, float *loss_terms, int64_t B, int32_t K,
                             amar_stream_t stream);

/* ---- the compiled loss and the compiled metrics (Model.compile(loss=..., metrics=...)) -------------------------------------------
 * amar_loss_grad_f32   Keras 2's pointwise losses on ONE sigmoid output, in amar_bce_grad_f32's place and conventions: p is [B] or a
 *                      strided [B, 1] column (leading dimension ldp), y the 0/1 labels, loss_terms[i] the pair's term (their sum =
 *                      B x batch loss), dz[i] = d(mean loss)/d(logit) = dL_i/dp . p (1 - p) / B; dz and loss_terms contiguous [B].
 *                      With e = p - y and s = 2y - 1:
 *                        AMAR_LOSS_BCE            amar_bce_grad_f32's term on y <- y (1 - ls) + ls / 2; ls = 0 gives its very bits
 *                        AMAR_LOSS_MSE            e^2
 *                        AMAR_LOSS_MAE            |e|, gradient 0 at e = 0
 *                        AMAR_LOSS_HINGE          max(1 - s p, 0)
 *                        AMAR_LOSS_SQUARED_HINGE  max(1 - s p, 0)^2
 *                        AMAR_LOSS_HUBER          e^2 / 2 where |e| <= delta, else delta |e| - delta^2 / 2
 *                        AMAR_LOSS_LOG_COSH       e + softplus(-2e) - log 2, evaluated as log1p(2 sinh^2(e / 2))
 *                        AMAR_LOSS_POISSON        p - y log(p + 1e-7)
 *                        AMAR_LOSS_FOCAL          [alpha y + (1 - alpha)(1 - y) if balance] (1 - p_t)^gamma bce(p, y), p_t = y p + (1 - y)(1 - p),
 *                                                 y smoothed first as above, bce the clipped term of AMAR_LOSS_BCE
 *                      hyper: AMAR_LOSS_HYPER_FLOATS host floats read at the call — [0] label_smoothing in [0, 1] (BCE, FOCAL),
 *                      [1] delta (HUBER) or gamma (FOCAL), >= 0, [2] alpha, [3] apply_class_balancing as 0 / 1; NULL = Keras' defaults
 *                      (0, 1 or 2, 0.25, 0).  Where a loss is flat or clipped (hinge beyond the margin, cross-entropy outside
 *                      [1e-7, 1 - 1e-7]) and where p is exactly 0 or 1, dz is exactly 0.  float32, one lane per pair, no float atomics.
 *                      counters (nullable): AMAR_LOSS_COUNTERS 64-bit integers in DEVICE memory that the launch ADDS this batch to
 *                      (the host clears them): [0..3] = tp, fp, tn, fn with predicted positive <=> p > 0.5 and actual positive <=>
 *                      y > 0.5 (binary accuracy, Precision, Recall at 0.5); [4 + label * AMAR_AUC_BUCKETS + b] = the pairs of that label
 *                      whose p exceeds exactly b of the 198 interior thresholds float32(k / 199.0), k = 1..198, of Keras'
 *                      AUC(num_thresholds=200) — b agrees with the float comparison p > threshold for every p.  Integer sums
 *                      (per wavefront, LDS, one global atomic per non-zero cell and workgroup): the same bits on every run.
 *                      NULL: nothing is counted and nothing is written.
 * amar_loss_counters   AMAR_LOSS_COUNTERS, for a caller that sizes the block at run time.
 * amar_loss_grad_weighted_f32  amar_loss_grad_f32 under Keras' fit(class_weight=..., sample_weight=...): the pair's weight is
 *                      w_i = (sample_w ? sample_w[i] : 1) * (class_w ? class_w[y[i] > 0.5] : 1), the class taken from the 0/1 label
 *                      itself (before label smoothing).  sample_w: [B] floats, class_w: TWO floats (class 0, class 1), both in DEVICE
 *                      memory and read by the kernel (a captured graph follows new weights without a new capture); either may be
 *                      NULL, both NULL: AMAR_EINVAL (that call is amar_loss_grad_f32's).  The kernel computes exactly what the
 *                      unweighted instance computes and multiplies as the LAST float32 operation: loss_terms[i] = w_i * term_i,
 *                      dz[i] = w_i * dz_i — so every output is float32(w_i x amar_loss_grad_f32's output), w_i = 1 gives its bits and
 *                      w_i = 0 gives 0.  The divisor of dz stays B (Keras' SUM_OVER_BATCH_SIZE), not sum(w).  The counters, if
 *                      given, count every pair once as before: compiled metrics are unweighted.  Other arguments and refusals as
 *                      amar_loss_grad_f32. */
#define AMAR_LOSS_BCE           0
#define AMAR_LOSS_MSE           1
#define AMAR_LOSS_MAE           2
#define AMAR_LOSS_HINGE         3
#define AMAR_LOSS_SQUARED_HINGE 4
#define AMAR_LOSS_HUBER         5
#define AMAR_LOSS_LOG_COSH      6
#define AMAR_LOSS_POISSON       7
#define AMAR_LOSS_FOCAL         8
#define AMAR_LOSS_HYPER_FLOATS  4
#define AMAR_AUC_BUCKETS        199
#define AMAR_LOSS_COUNTERS      (4 + 2 * AMAR_AUC_BUCKETS)
int32_t amar_loss_counters(void);
int amar_loss_grad_f32(int32_t loss, const float *hyper, const float *p, int64_t ldp, const float *y, float *dz, float *loss_terms,
                       int64_t B, int64_t *counters, amar_stream_t stream);
int amar_loss_grad_weighted_f32(int32_t loss, const float *hyper, const float *p, int64_t ldp, const float *y, const float *sample_w,
                                const float *class_w, float *dz, float *loss_terms, int64_t B, int64_t *counters, amar_stream_t stream);

/* ---- training-time dropout (the `dropout` key of the GNN stacks, `dropout_rate` of GAT) ------------------------------------------
 * No mask is stored: a keep bit is a function of (seed, step, site, element) through Philox4x32-10 and the reverse pass regenerates
 * it.  key = (seed & 0xffffffff, seed >> 32); counter = (c0, s & 0xffffffff, s >> 32, (site << 24) | c3) with s = *step read from
 * DEVICE memory (a replayed graph drops other elements every step) and site in 1..255 (which dropout of the model).  A value is
 * kept iff its 32-bit word >= threshold (= min(2^32 - 1, round(rate * 2^32))) and then multiplied by scale (= float32(1 / (1 - rate)));
 * a dropped value becomes +0.  None of these entries advances *step.
 * amar_dropout_f32            Y[r, c] = X[r, c] * keep * scale on an [n_rows, C] slice (Y == X: in place); applied to a gradient slice
 *                             it is its own reverse.  Element: c0 = r * ceil(C / 4) + c / 4, c3 = 0, word c % 4 of the call (one call
 *                             per 16 bytes; a width that is no multiple of 4 leaves the surplus words of a row's last call unused and
 *                             takes scalar accesses, as do slices that are not 16-byte aligned).  n_rows * ceil(C / 4) < 2^31.
 * amar_dropout_advance        *step += 1, once per training step after the last reader.
 * amar_gat_layer_dropout_f32  amar_gat_layer_f32 with the attention coefficients dropped AFTER the softmax (Spektral):
 *                             Y_i = ReLU(sum_j alpha_ij keep_ij scale H_j + bias); maximum, denominator and the 1e-9 are those of the
 *                             undropped logits.  Element of the stored entry (target i, source j) that is the o-th of its row's equal
 *                             columns (colidx sorted per row): c0 = min(i, j) | ((o % 255) << 24), c3 = max(i, j), word 0; the added self
 *                             loop is the entry (i, i) with ordinal slot 255.  (i, j, o) and (j, i, o) draw one bit: on a symmetric
 *                             edge multiset the reverse pass may therefore visit an entry from either end; on a directed one a
 *                             reciprocal pair shares its bit.  n_rows <= 2^24.  threshold 0, scale 1: the bits of amar_gat_layer_f32.
 * amar_gat_bwd_dropout_f32    amar_gat_bwd_f32 for that forward with the same bits: d alpha_ij = keep_ij scale (dout_i . H_j) into the
 *                             unchanged softmax reverse, dH_j accumulates alpha_ij keep_ij scale dout_i; no float atomics.
 *                             Symmetric edge multiset, as amar_gat_bwd_f32.
 * amar_gat_bwd_directed_dropout_f32   the same with the source walk on the stable transpose (t_rowptr / t_colidx), for any edge
 *                             multiset: entry (i, j, o) of A is entry (j, i, o) of A^T — the stable transpose keeps the order of
 *                             parallel entries — so both walks regenerate the same bit. */
int amar_dropout_f32(const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t n_rows, int32_t C,
                     uint64_t seed, const uint64_t *step, uint32_t site, uint32_t threshold, float scale, amar_stream_t stream);
int amar_dropout_advance(uint64_t *step, amar_stream_t stream);
int amar_gat_layer_dropout_f32(const int32_t *rowptr, const int32_t *colidx,
                               const float *H, int64_t ldh, int32_t C,
                               const float *s_self, const float *s_neigh, const float *bias,
                               float *Y, int64_t ldy, int32_t self_loop, int32_t n_rows,
                               uint64_t seed, const uint64_t *step, uint32_t site, uint32_t threshold, float scale,
                               amar_stream_t stream);
int amar_gat_bwd_dropout_f32(const int32_t *rowptr, const int32_t *colidx, const float *H, int64_t ldh, int32_t C,
                             const float *s_self, const float *s_neigh, const float *Y, int64_t ldy, const float *dY, int64_t ldd,
                             const float *bias, const float *a_self, const float *a_neigh,
                             float *dout, float *row_scratch, float *ds, float *dt, float *dH, int64_t lddh,
                             int32_t self_loop, int32_t n_rows,
                             uint64_t seed, const uint64_t *step, uint32_t site, uint32_t threshold, float scale, amar_stream_t stream);
int amar_gat_bwd_directed_dropout_f32(const int32_t *rowptr, const int32_t *colidx, const int32_t *t_rowptr, const int32_t *t_colidx,
                                      const float *H, int64_t ldh, int32_t C,
                                      const float *s_self, const float *s_neigh, const float *Y, int64_t ldy, const float *dY, int64_t ldd,
                                      const float *bias, const float *a_self, const float *a_neigh,
                                      float *dout, float *row_scratch, float *ds, float *dt, float *dH, int64_t lddh,
                                      int32_t self_loop, int32_t n_rows,
                                      uint64_t seed, const uint64_t *step, uint32_t site, uint32_t threshold, float scale, amar_stream_t stream);

/* ---- transposed image of a graph (training on directed graphs, dataset.symmetric_adjacency: False) --------------------------------
 * The STABLE transpose of an int32 CSR structure [n_rows, n_cols] with nnz = rowptr[n_rows] entries:
 *     t_rowptr[n_cols + 1], t_colidx[nnz]   the CSR structure of A^T
 *     perm[nnz]                             perm[q] = the input position of the entry that stands at output position q
 * Inside output row j the entries stand in the order of their input positions — by source row, parallel (duplicate) entries in
 * their input order — which is scipy's csr -> csc conversion without summing duplicates; perm is strictly increasing inside every
 * output row.  Hence: input rows with sorted columns give output rows with sorted columns, and an entry is the o-th of its equals
 * in row i of A exactly when it is the o-th of its equals in row j of A^T.  Whatever else an entry carries (value, multiplicity)
 * follows by a gather through perm.
 * The result is the same bits on every run: integer counting (vector atomics on int32), a scan, a fill through atomic cursors and
 * then a sort of every output row's positions, which removes the arrival order (long rows — hub columns — included).  No float or
 * scalar atomics.  cursor: n_cols int32 of scratch.  Column indices must lie in [0, n_cols) (entries outside are skipped, never
 * written out of bounds; the result is then unspecified).  nnz == 0: t_rowptr is zeroed, the other outputs may be NULL.
 * Not meant for a captured graph's body: it runs once per graph. */
int amar_csr_transpose_i32(const int32_t *rowptr, const int32_t *colidx, int32_t n_rows, int32_t n_cols, int32_t nnz,
                           int32_t *t_rowptr, int32_t *t_colidx, int32_t *perm, int32_t *cursor, amar_stream_t stream);

/* ---- ranking ------------------------------------------------------------------------------
 * Per-user top-k over that user's own test pairs (src/utilities/metrics.py:11-34):
 * pairs are grouped by user (seg_ptr[n_users+1] into item_ids/scores); for each user the k
 * best (score desc, item id asc on ties) are written to out_items/out_scores [n_users, k],
 * padded with -1 / -inf when the user has fewer than k pairs.  k <= 64.
 */
int amar_topk_segmented_f32(const int32_t *seg_ptr, const int32_t *item_ids, const float *scores,
                            int32_t n_users, int32_t k, int32_t *out_items, float *out_scores,
                            amar_stream_t stream);

/* The same from a cursor ("the next page" of the pair route): user u's list holds the k best pairs that come STRICTLY AFTER the
 * position (after_scores[u], after_items[u]) in the order above, i.e. score < after_scores[u], or score == after_scores[u] and
 * item id > after_items[u]; after_scores / after_items [n_users] go together and are required when n_users > 0 (AMAR_EINVAL).
 * The cursor values are those of amar_recommend_after_f32 below: (+inf, -1) is the start (amar_topk_segmented_f32's output, bit for
 * bit), (-inf, -1) and a NaN score admit nothing, the cursor's item need not be one of the user's pairs.  The scores are read, never
 * recomputed: a caller pages through one scored chunk with one call per page.  k <= 64; the other checks, in
 * amar_topk_segmented_f32's order, are that entry point's. */
int amar_topk_segmented_after_f32(const int32_t *seg_ptr, const int32_t *item_ids, const float *scores,
                                  int32_t n_users, int32_t k, const float *after_scores, const int32_t *after_items,
                                  int32_t *out_items, float *out_scores, amar_stream_t stream);

/* Full-catalogue top-k of the split scoring head (models/basic.py:_split_plan: the classifier's first Dense layer folded
 * into the towers), fused: for every listed user j (users[j], or j itself when users == NULL, m == n_users) and EVERY item
 * i in 0..n_items-1 that is not in the user's exclusion list,
 *     score(u, i) = rest( in_act( Tu[u, 0:c1] + Ti[i, 0:c1] ) )
 * rest = the Dense stack packed by amar_chain_pack_f32 (dims[0] = c1, dims[n_layers] = 1: at least one Dense layer, then the
 * 1-unit scorer), and the k best (score descending, item ascending on ties) are written to out_items / out_scores [m, k],
 * padded with -1 / -inf when fewer than k items remain.  Nothing of size m x n_items is written.  Item ids are Ti rows.
 * Exclusion CSR (optional, both NULL = rank every item): excl_ptr[n_users+1], excl_items sorted and de-duplicated per user,
 * values in 0..n_items-1.  PRECONDITION: every users[j] < n_users (not checked on the device).  The CSR holds fewer than 2^30
 * entries (the selector's binary search adds two int32 positions); the host caller knows its length, the library does not.
 * A score is bit-identical to amar_chain_f32's f32 generic kernel on the same pair (its loop order, fragments and dot stage).
 * Limits: c1 and every width <= 128, c1 % 4 == 0, <= 8 Dense layers before the scorer, k <= 64; else AMAR_EUNSUPPORTED.
 * Tu, Ti, wpack 16-byte aligned, ldu / ldi multiples of 4.
 * n_slices: item slices per user block (<= 0: automatic).  amar_recommend_slices returns the count a call will launch; with
 * more than one, workspace_items / workspace_scores hold m * slices * k entries each (any contents) and a second launch
 * merges the slices.  The result does not depend on the slicing, the other users of the call or the grid. */
int32_t amar_recommend_slices(int64_t m, int32_t n_items, const int32_t *dims, int32_t n_layers, int32_t n_slices);
int amar_recommend_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                       const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                       const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                       int32_t k, int32_t n_slices, int32_t *workspace_items, float *workspace_scores,
                       int32_t *out_items, float *out_scores, amar_stream_t stream);

/* Group recommendation over the same split head, fused: the members' scores of every item are combined by a social-choice rule
 * and each group's k best items are selected on chip ("what should WE watch?").  Tables, packed rest stack, limits, alignment
 * rules and slicing contract are those of amar_recommend_f32.
 * Group j of n_groups has the members grp_users[grp_ptr[j] .. grp_ptr[j+1]): rows of Tu, ascending and distinct inside a group
 * (a PRECONDITION, like every member < n_users: not checked on the device); n_members = grp_ptr[n_groups], which the host caller
 * knows.  Exclusion CSR (optional, both NULL = rank every item) over the GROUPS: excl_ptr[n_groups+1], segment j sorted and
 * de-duplicated, values in 0..n_items-1; it belongs to group j, not to a user.
 * All in float32, for item i not in the group's segment: s_t = score(member_t, i), exactly the value amar_recommend_f32 computes
 * for that pair (one score routine: the same fragments, loop order and dot stage), and
 *     AMAR_GROUP_MEAN:  acc = s_0, then acc = acc + s_t for t = 1..n-1 in member order; the aggregate is acc / (float)n, correctly
 *                       rounded (IEEE division, no reciprocal, nothing contracted)
 *     AMAR_GROUP_MIN:   the smallest s_t (least misery)          AMAR_GROUP_MAX:  the largest s_t (most pleasure)
 * Veto: the item is dropped for the group when any s_t < min_score; min_score = -INFINITY turns it off.
 * The k best (aggregate descending, item ascending on ties) go to out_items / out_scores [n_groups, k], padded with -1 / -inf; an
 * empty group, or one with nothing left, gives an all-padding row.  A group of one member returns, under every strategy, the bits
 * amar_recommend_f32 returns for that user with the same exclusion list.  Nothing of size members x n_items or
 * n_groups x n_items is written; selection runs once per item per group.  A group's result depends on its own members, Ti, the
 * weights, the strategy, min_score and its segment only: not on the other groups of the call, the grid or the slicing; no atomics,
 * the same bits on every run.
 * n_slices: item slices per block of 16 groups (<= 0: automatic, sized from n_groups AND n_members: a workgroup's work is its
 * members' walks over its tiles).  amar_recommend_group_slices returns the count a call will launch (a call that passes
 * n_slices > 0 must pass that count); with more than one, workspace_items / workspace_scores hold n_groups * slices * k entries
 * each (any contents) and a second launch merges the slices.
 * NULL tables, negative sizes, k < 1, an unknown strategy, a NaN min_score, grp_ptr == NULL with n_groups > 0, grp_users == NULL
 * with n_members > 0, excl_ptr without excl_items, a missing workspace: AMAR_EINVAL; the shape limits: AMAR_EUNSUPPORTED; all
 * checked before any device call.  n_groups == 0: AMAR_OK, nothing is launched. */
#define AMAR_GROUP_MEAN 0   /* additive / average */
#define AMAR_GROUP_MIN  1   /* least misery */
#define AMAR_GROUP_MAX  2   /* most pleasure */
int32_t amar_recommend_group_slices(int64_t n_groups, int64_t n_members, int32_t n_items, const int32_t *dims, int32_t n_layers,
                                    int32_t n_slices);
int amar_recommend_group_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *grp_ptr, const int32_t *grp_users, int64_t n_groups, int64_t n_members,
                             const int32_t *excl_ptr, const int32_t *excl_items, int32_t strategy, float min_score,
                             int32_t k, int32_t n_slices, int32_t *workspace_items, float *workspace_scores,
                             int32_t *out_items, float *out_scores, amar_stream_t stream);

/* Top-k among a candidate slice of the catalogue ("the best k among THESE items": one genre, what is in stock, a shelf, the
 * output of a retrieval stage), fused: amar_recommend_f32 with the tile loop running over a candidate list instead of the rows
 * 0..n_items-1.  Tables, packed rest stack, limits, alignment rules, users[m] and the exclusion CSR over USERS are exactly those of
 * amar_recommend_f32.
 * Candidates: cand_items[n_cand], device item rows.  PRECONDITION: strictly ascending (so distinct) and each in [0, n_items); the
 * library cannot check device memory, a list that breaks this is read out of bounds or walks the exclusion rows wrongly.  Host
 * callers check the list before they upload it (capi.recommend_among does).
 * For every listed user and every candidate that is not in the user's exclusion row the score is the one amar_recommend_f32
 * computes for the pair, bit for bit (one score routine), and the k best (score descending, item row ascending on ties) go to
 * out_items / out_scores [m, k] as item ROWS, padded with -1 / -inf: the lists amar_recommend_f32 returns with the complement of
 * the candidates merged into every exclusion row.  m x n_cand pairs are scored, not m x n_items; nothing of either size is written.
 * n_cand == 0 is a valid call: every list is padding and cand_items is not read (it may be NULL).
 * How: the workgroup gathers the candidates' Ti rows into the item tile and keeps the tile's item rows beside it in LDS
 * (4 * tile_items bytes more than amar_recommend_f32: amar_rank_route with AMAR_RANK_AMONG); selection and the exclusion walk
 * stay in item-row space, which ascending candidates keep valid.  A user's result depends on its own Tu row, the candidates' Ti
 * rows, the weights and its exclusion row only: not on the other users, the grid or the slicing; the same bits on every run.
 * n_slices: slices of candidate POSITIONS per user block (<= 0: automatic).  amar_recommend_slices(m, n_cand, ...) returns the
 * count a call will launch (a call that passes n_slices > 0 must pass that count); with more than one, workspace_items /
 * workspace_scores hold m * slices * k entries each (any contents) and a second launch merges the slices.
 * NULL tables, negative sizes, k < 1, n_cand > n_items, cand_items == NULL with n_cand > 0, users == NULL with m != n_users,
 * excl_ptr without excl_items, a missing workspace or output: AMAR_EINVAL; k > 64, the shape limits, a head whose LDS sum does not
 * fit (amar_rank_route: fits == 0): AMAR_EUNSUPPORTED; all checked before any device call.  m == 0: AMAR_OK, nothing is launched. */
int amar_recommend_among_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                             const int32_t *cand_items, int32_t n_cand, int32_t k, int32_t n_slices,
                             int32_t *workspace_items, float *workspace_scores, int32_t *out_items, float *out_scores,
                             amar_stream_t stream);

/* Top-k over PER-USER candidate lists ("the best k of THIS user's candidates": a retrieval stage's output to re-rank, per-user
 * availability, the 1 + N sampled-negatives protocol), fused.  Tables, packed rest stack, limits, alignment rules, users[m] and
 * the exclusion CSR over USERS are exactly those of amar_recommend_f32.
 * Candidates: a CSR over the m LISTED rows, cand_ptr[m + 1] (int32, so the lists hold fewer than 2^31 entries together) and
 * cand_items (device item rows).  PRECONDITION: inside every listed row j, cand_items[cand_ptr[j] .. cand_ptr[j + 1]) is strictly
 * ascending (so distinct) and lies in [0, n_items) — the contract amar_recommend_among_f32 puts on its one list.  Nothing on the
 * device checks it; host callers check a host list before they upload it (capi.recommend_lists does).  The same user may be
 * listed twice with two lists; a list may be empty (the row is all padding).
 * For every listed row and every candidate of its list that is not in the user's exclusion row the score is the one
 * amar_recommend_f32 computes for the pair, bit for bit (one score routine, the same user fragments), and the k best (score
 * descending, item row ascending on ties) go to out_items / out_scores [m, k] as item ROWS, padded with -1 / -inf: the lists
 * amar_recommend_f32 returns with the complement of the row's candidates merged into its exclusion row.  sum_j |C_j| pairs are
 * scored; nothing of size m x n_items is built, read or written, and there is no workspace.
 * How: ceil(m / 4) workgroups of 4 waves, one listed row and one selector per wave.  The packed stack is staged once per
 * workgroup, followed by the kernel's only workgroup barrier; from there a wave walks its own list 16 pt candidates a step —
 * it gathers their Ti rows into its own tile-shaped LDS buffer, scores them, offers them to its selector — and synchronises at
 * wave scope only: the four lists of a workgroup may have any lengths.  A wave walks its whole list: there are no slices and no
 * merge launch, so a call whose lists are all the same long set is amar_recommend_among_f32's, not this one's.  LDS: the stack +
 * 4 gather buffers + 4 selectors and no item tile (amar_rank_route with AMAR_RANK_LISTS), so a head may fit here that
 * amar_recommend_f32 refuses.  A row's result depends on its own Tu row, its candidates' Ti rows, the weights and its exclusion row
 * only; the same bits on every run.
 * NULL tables, negative sizes, k < 1, users == NULL with m != n_users, excl_ptr without excl_items, cand_ptr == NULL with m > 0,
 * cand_ptr without cand_items, a missing output with m > 0: AMAR_EINVAL; k > 64, the shape limits, a head whose LDS sum does not
 * fit (amar_rank_route: fits == 0): AMAR_EUNSUPPORTED; all checked before any device call.  m == 0: AMAR_OK, nothing is launched. */
int amar_recommend_lists_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                             const int32_t *cand_ptr, const int32_t *cand_items, int32_t k,
                             int32_t *out_items, float *out_scores, amar_stream_t stream);

/* Top-k AFTER a position of the user's ranking ("the next page"; chained, lists longer than 64), fused: amar_recommend_f32 with a
 * cursor per selector row.  Tables, packed rest stack, limits, alignment rules, users[m], the exclusion CSR, the slicing contract
 * (amar_recommend_slices, the workspaces, the merge launch), the LDS sum (amar_rank_route with AMAR_RANK_RECOMMEND) and the
 * -1 / -inf padding are exactly those of amar_recommend_f32.
 * Cursor: after_scores[m], after_items[m], device arrays indexed by the selector row j of the call, NOT by the user row users[j]:
 * the same user may stand twice in a call with two cursors.  The order of the rankers (score descending, item row ascending) is a
 * strict total order, so (score, item row) is a position in a user's ranking; a pair (z, item) is offered to the selector only if
 * it comes strictly after the cursor: z < after_scores[j], or z == after_scores[j] and item > after_items[j].  For every pair that
 * passes the score is the one amar_recommend_f32 computes, bit for bit (one score routine), and the list is that user's ranking
 * with everything up to and including the cursor struck out: the list amar_recommend_f32 returns with the earlier pages merged
 * into the user's exclusion row.  Cursor values:
 *     the start         (+inf, -1)  admits every pair: the call returns amar_recommend_f32's output, bit for bit
 *     the end           (-inf, -1)  admits nothing: no sigmoid, ReLU or linear score is below -inf.  It is the padding of an
 *                                   exhausted list, so a page chained onto an exhausted list is all padding
 *     the cursor's item need not be a real row (it may be >= n_items) and may be an excluded row: it is only a position
 *     a NaN score admits nothing (every comparison with it is false); host callers refuse it
 * The typical cursor is the last column of the previous page: (out_scores[j, k-1], out_items[j, k-1]).
 * NULL tables, negative sizes, k < 1, users == NULL with m != n_users, excl_ptr without excl_items, one of after_scores /
 * after_items without the other, either missing with m > 0, a missing workspace or output: AMAR_EINVAL; k > 64, the shape limits,
 * a head whose LDS sum does not fit: AMAR_EUNSUPPORTED; amar_recommend_f32's checks in its order, then the cursor's, all before any
 * device call.  m == 0: AMAR_OK, nothing is launched. */
#define AMAR_AFTER_NO_ITEM (-1)   /* the item of both constant cursors: with +INFINITY the start, with -INFINITY the end */
int amar_recommend_after_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                             const float *after_scores, const int32_t *after_items, int32_t k, int32_t n_slices,
                             int32_t *workspace_items, float *workspace_scores, int32_t *out_items, float *out_scores,
                             amar_stream_t stream);

/* Nearest rows of a table under dot or cosine similarity, fused score-and-select ("which items are like this one?").
 * Listed query j is row Q[query_rows[j]] (row j itself when query_rows == NULL, m == n_queries).  For every listed query and EVERY
 * row i of T[n_rows, d] that is not in the query's exclusion segment,
 *     AMAR_NEAREST_DOT:     score(j, i) = sum_c Q[q, c] * T[i, c]
 *     AMAR_NEAREST_COSINE:  score(j, i) = (dot * inv_norm(Q[q])) * inv_norm(T[i]),  inv_norm(x) = 1/sqrt(sum x^2), 0 when the sum is 0
 * (a zero row scores 0 against everything, never NaN), and the k best (score descending, table row ascending on ties) are written
 * to out_rows / out_scores [m, k], padded with -1 / -inf when fewer than k rows remain.  Nothing of size m x n_rows is written.
 * Exclusion CSR (optional, both NULL = rank every row) over the LISTED queries: excl_ptr[m+1], segment j belongs to listed query j
 * (not to its row in Q); each segment sorted ascending and de-duplicated, values in 0..n_rows-1.  Self-exclusion, profile items
 * and filters are all expressed through it.  PRECONDITION: every query_rows[j] < n_queries (not checked on the device).
 * Products run on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: one fmaf chain per score, features in the fragment order
 * 16t + 4g + r of amar_recommend_f32: t ascending, r ascending inside t); the inverse norms are computed once per table row and
 * once per listed query in a pre-pass.  A query's result depends on its own row, T, the metric and its exclusion segment only:
 * not on the other queries of the call, the grid or the slicing; a call returns the same bits on every run (no float atomics).
 * Limits: d % 4 == 0, 4 <= d <= 512, k <= 64, ldq / ldt multiples of 4 (they may exceed d), Q and T 16-byte aligned; else
 * AMAR_EUNSUPPORTED.  NULL Q / T, negative sizes, k < 1, an unknown metric, ldq or ldt < d, excl_ptr without excl_rows, a missing
 * workspace: AMAR_EINVAL.  All of these are checked before any device call.
 * n_slices: table slices per query block (<= 0: automatic).  amar_nearest_slices returns the count a call will launch (a call that
 * passes n_slices > 0 must pass that count).  workspace_scores holds amar_nearest_workspace_floats(m, n_rows, k, metric, slices)
 * floats, 16-byte aligned (the inverse norms for cosine, then the per-slice scores; may be NULL when that is 0), workspace_rows
 * m * slices * k entries when slices > 1 (else it may be NULL); any contents.  With slices a second launch merges them. */
#define AMAR_NEAREST_DOT    0
#define AMAR_NEAREST_COSINE 1
int32_t amar_nearest_slices(int64_t m, int32_t n_rows, int32_t d, int32_t n_slices);
int64_t amar_nearest_workspace_floats(int64_t m, int32_t n_rows, int32_t k, int32_t metric, int32_t slices);
int amar_nearest_f32(const float *Q, int64_t ldq, int32_t n_queries, const float *T, int64_t ldt, int32_t n_rows, int32_t d,
                     int32_t metric, const int32_t *query_rows, int64_t m, const int32_t *excl_ptr, const int32_t *excl_rows,
                     int32_t k, int32_t n_slices, int32_t *workspace_rows, float *workspace_scores,
                     int32_t *out_rows, float *out_scores, amar_stream_t stream);

/* Full-ranking metrics of top-K lists that are already on the device (utilities/metrics.py:full_ranking_metrics, restated):
 * lists [m, K] holds item ROWS best first, padded with -1 (what amar_recommend_f32 / amar_topk_segmented_f32 write); row j
 * belongs to user users[j] (j itself when users == NULL, m == n_users).  The relevant items are a CSR over users:
 * rel_ptr[n_users+1], rel_items sorted ascending and de-duplicated per user.  A user with an empty relevant segment (or an id
 * outside 0..n_users-1) is skipped and counted; a padded rank is a miss.  For every other user and every cutoff k = ks[q], with
 * hits = relevant items among the first k ranks:
 *     precision = hits / k,  recall = hits / |rel|,  hit = [hits > 0],
 *     ndcg = sum_{hit at rank r <= k} 1 / log2(r + 1)  /  cum_disc[min(|rel|, k)]
 * in float64.  out_sums [nk, 4] (device) receives the SUMS over the evaluated users in the order precision, recall, ndcg, hit;
 * out_counts [2] (device, int64) receives (evaluated, skipped): the caller divides.
 * ks (nk cutoffs) and cum_disc (K + 1 entries: cum_disc[0] = 0, cum_disc[j] = sum_{r <= j} 1 / log2(r + 1)) are HOST arrays.
 * workspace: AMAR_RANK_METRICS_MAX_BLOCKS * AMAR_RANK_METRICS_CELLS doubles of device scratch (any contents).
 * Two launches, no atomics: users are summed in an order fixed by m alone, so a call returns the same bits on every run.
 * K > 64 or nk > AMAR_RANK_METRICS_MAX_KS: AMAR_EUNSUPPORTED; K < 1, nk < 1, a k outside [1, K], a NULL pointer (lists may be
 * NULL when m == 0), users == NULL with m != n_users, negative sizes: AMAR_EINVAL. */
#define AMAR_RANK_METRICS_MAX_KS     8
#define AMAR_RANK_METRICS_MAX_BLOCKS 1024
#define AMAR_RANK_METRICS_CELLS      (4 * AMAR_RANK_METRICS_MAX_KS + 2)
int amar_rank_metrics_f64(const int32_t *lists, int64_t m, int32_t K, const int32_t *users, const int32_t *rel_ptr,
                          const int32_t *rel_items, int32_t n_users, const int32_t *ks, int32_t nk, const double *cum_disc,
                          double *workspace, double *out_sums, int64_t *out_counts, amar_stream_t stream);

/* Where does THIS item stand?  Exact positions of chosen (user, item) pairs in the full catalogue of the split scoring head, by
 * counting: the third consumer of the score routine of amar_recommend_f32 / amar_recommend_group_f32 (one text, the same bits per
 * pair wherever it is staged).  Tables, packed rest stack, limits, alignment rules, users[m] and the exclusion CSR over USERS are
 * exactly those of amar_recommend_f32.
 * Targets: a CSR over the m LISTED entries, tgt_ptr[m+1] and tgt_items (item rows in 0..n_items-1, ascending and de-duplicated per
 * entry; n_targets = tgt_ptr[m], which the host caller knows).  The same user may be listed in several entries; an entry holds at
 * most AMAR_RANK_OF_MAX_TARGETS targets (the host caller passes max_targets, the longest entry it built; more: AMAR_EUNSUPPORTED).
 * For entry j with user u, C(u) = {items} \ excl(u) and target t at position e of tgt_items, in float32:
 *     out_scores[e]    = s_t = score(u, t)
 *     out_greater[e]   = #{ i in C(u), i != t : score(u, i) >  s_t }
 *     out_eq_before[e] = #{ i in C(u), i != t : score(u, i) == s_t, i < t }
 *     out_eq_after[e]  = #{ i in C(u), i != t : score(u, i) == s_t, i > t }
 * so 1 + greater + eq_before is the position at which amar_recommend_f32 with an unbounded k would list t.  A target that is
 * itself in excl(u) is scored and counted against C(u) like any other (the host decides what that means); other targets of the
 * same user are ordinary candidates.  Counts are int32.  Nothing of size m x n_items is written.
 * How: blocks of 16 entries x item slices, as amar_recommend_f32.  Per entry the targets' Ti rows are gathered into a tile-shaped
 * LDS buffer and scored, then sorted by (score, item); every catalogue pair costs one binary search among them and one integer LDS
 * add; the user's excluded items of the slice are scored as gathered tiles and subtracted (exact: a pair's bits do not depend on
 * where it is staged); the slices add their integer partials to the outputs with integer atomics.  No float atomics: an entry's
 * result depends on its own user row, Ti, the weights, its exclusion row and its targets only, not on the other entries, the grid
 * or the slicing, and a call returns the same bits on every run.
 * AMAR_RANK_OF_MAX_TARGETS = 64: one lane per target in the sort and the final prefix sums, and 16 entries' sorted targets and
 * counters (6 x 64 + 2 words each, 25 KB) fit beside the largest stack the rankers take (128 -> 128 -> 1: 67 KB of weights, a 25 KB
 * tile, 34 KB of gather buffers: 151 of the 160 KB).
 * n_slices: item slices per entry block (<= 0: automatic).  amar_rank_of_slices returns the count a call will launch (a call that
 * passes n_slices > 0 must pass that count).  PRECONDITION: every users[j] < n_users (not checked on the device); a target or
 * excluded row outside 0..n_items-1 is scored as a row of zeros, never read.
 * NULL tables or outputs, negative sizes, tgt_ptr == NULL with m > 0, tgt_items == NULL with n_targets > 0, excl_ptr without
 * excl_items, users == NULL with m != n_users: AMAR_EINVAL; the shape limits: AMAR_EUNSUPPORTED; all checked before any device
 * call.  m == 0 or n_targets == 0: AMAR_OK, nothing is launched. */
#define AMAR_RANK_OF_MAX_TARGETS 64
int32_t amar_rank_of_slices(int64_t m, int32_t n_items, const int32_t *dims, int32_t n_layers, int32_t n_slices);
int amar_rank_of_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                     const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                     const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                     const int32_t *tgt_ptr, const int32_t *tgt_items, int64_t n_targets, int32_t max_targets, int32_t n_slices,
                     float *out_scores, int32_t *out_greater, int32_t *out_eq_before, int32_t *out_eq_after, amar_stream_t stream);

/* Cut-off-free ranking metrics from amar_rank_of_f32's flat outputs: AUC, reciprocal rank and average precision per evaluated
 * user, in float64.  Evaluated user v of n_eval owns the targets rel_ptr[v] .. rel_ptr[v+1] of the flat order (a CSR over USERS,
 * independent of how the entries were chunked): R' = relevant(u) \ excl(u), the user's held-out items; n_cand[v] = |C(u)|.
 * With r_t = 1 + greater_t + eq_before_t, h_t = #{t' in R' : r_t' <= r_t}, R = |R'| and N_neg = n_cand - R:
 *     rr  = 1 / min_t r_t
 *     ap  = (1 / R) sum_t h_t / r_t                                     (terms added in target order)
 *     auc = 1 - [ sum_t ( neg_greater_t + neg_equal_t / 2 ) ] / ( R N_neg )
 * neg_greater_t = greater_t - #{t' != t : s_t' > s_t}, neg_equal_t = eq_before_t + eq_after_t - #{t' != t : s_t' == s_t}: the
 * candidates that are not targets, the target-target corrections from comparing `scores` pairwise.  This is the Mann-Whitney
 * statistic with ties at 1/2; it does not depend on the numbering of the items (the sum is an exact integer count of halves).
 * out [n_eval, 3] = (auc, rr, ap); valid [n_eval] (int32) = 0 for R = 0 or N_neg <= 0 (the row is then 0, 0, 0: the caller skips
 * and counts it), else 1.  One wavefront per user, no atomics, the same bits on every run; the caller means the valid rows.
 * NULL rel_ptr / n_cand / out / valid with n_eval > 0, NULL flat arrays with n_targets > 0, negative sizes: AMAR_EINVAL.
 * n_eval == 0: AMAR_OK, nothing is launched. */
int amar_rank_of_metrics_f64(const float *scores, const int32_t *greater, const int32_t *eq_before, const int32_t *eq_after,
                             int64_t n_targets, const int32_t *rel_ptr, const int32_t *n_cand, int64_t n_eval,
                             double *out, int32_t *valid, amar_stream_t stream);

/* What the three fused rankers above do with a rest stack of these widths, without a device call: the launch geometry, the LDS a
 * launch asks for, and whether the kernel takes the head at all.  dims[0] = c1, dims[n_layers] = 1, as for amar_recommend_f32.
 * amar_recommend_f32, amar_recommend_group_f32 and amar_rank_of_f32 take their geometry and their capacity refusal from the function
 * behind this query, so what it reports is what a launch with these dims does.
 *     maxt         16-wide tiles of the widest layer (hidden layers included), rounded up to 1, 2, 4 or 8: the kernel form
 *     pt           16-item pair tiles a wave scores per step: 4, 4, 2, 1 for maxt 1, 2, 4, 8 (a step is 16 pt items)
 *     tile_items   items of a staged tile: a multiple of 16 pt, at most 256, within a 32 KB budget (at least one step)
 *     tile_stride  floats between staged rows: 16 ceil(c1 / 16) + 4
 *     wpack_floats floats of the packed stack (amar_chain_pack_floats of the same dims)
 *     lds_bytes    dynamic LDS of a launch: the stack (rounded up to 16 bytes) + tile_items * tile_stride * 4 + per kind:
 *                  RECOMMEND, GROUP: 16 640 (sixteen selectors);  RANK_OF: 4 * 16 pt * tile_stride * 4 (a gather buffer per wave)
 *                  + 16 * (6 * AMAR_RANK_OF_MAX_TARGETS + 2) * 4 = 24 704 (sixteen entries' sorted targets and counters)
 *                  LISTS is the one kind without the tile term: the stack + 4 * 16 pt * tile_stride * 4 (a gather buffer per wave)
 *                  + 4 160 (four selectors)
 *     fits        lds_bytes <= 160 KB.  0: the entry point returns AMAR_EUNSUPPORTED for this head, before any device call
 *     large_lds    lds_bytes > 64 KB: the launch first asks for the large dynamic LDS attribute
 * The capacity rule in short: recommend / group take a stack of up to 121 856 B next to a 128-wide c1 (128 -> 128 -> 64 -> 1 fits,
 * 128 -> 128 -> 128 -> 1 does not); rank_of takes up to 80 000 B there (128 -> 128 -> 1 fits, 128 -> 128 -> 64 -> 1 does not).
 * Returns AMAR_OK with `fits` 0 or 1 for every head the argument checks of the launchers pass; AMAR_EINVAL for dims or info == NULL,
 * an unknown kind, c1 < 4 or c1 % 4 != 0, a width < 1; AMAR_EUNSUPPORTED for n_layers outside [2, 9], dims[n_layers] != 1, a 1-unit
 * layer before the last, a width above 128: the code the launchers return for these dims. */
#define AMAR_RANK_RECOMMEND 0
#define AMAR_RANK_GROUP     1
#define AMAR_RANK_RANK_OF   2
#define AMAR_RANK_AMONG     4   /* amar_recommend_among_f32: RECOMMEND's sum + 4 * tile_items (the tile's item rows); 3 stays unknown */
#define AMAR_RANK_LISTS     5   /* amar_recommend_lists_f32: the stack + 4 * 16 pt * tile_stride * 4 (a gather buffer per wave)
                                 * + 4 160 (four selectors); no item tile */
typedef struct amar_rank_route_info {
    int32_t maxt, pt, tile_items, tile_stride;
    int32_t wpack_floats, fits, large_lds, reserved;
    int64_t lds_bytes;
} amar_rank_route_info;
int amar_rank_route(int32_t kind, const int32_t *dims, int32_t n_layers, amar_rank_route_info *info);

/* Diversified re-ranking of candidate pools that are already on the device: greedy Maximal Marginal Relevance (MMR), and the
 * intra-list diversity (ILD) of finished lists.  Both work on the P x P Gram matrix of a list's item vectors, kept on chip.
 *
 * T [n_rows, d] (leading dimension ldt) is the item table.  sim(a, b) is amar_nearest_f32's score of row a against row b:
 *     AMAR_NEAREST_DOT:     sim(a, b) = sum_c T[a, c] * T[b, c]
 *     AMAR_NEAREST_COSINE:  sim(a, b) = (dot * inv_norm(T[a])) * inv_norm(T[b]),  inv_norm(x) = 1/sqrt(sum x^2), 0 when the sum is 0
 * (a zero row is similar to nothing, never NaN), products and sums in float32 (v_mfma_f32_16x16x4_f32, one fmaf chain per pair,
 * features in the fragment order 16t + 4g + r of amar_nearest_f32; the inverse norms come from the Gram matrix's diagonal).
 *
 * amar_rerank_mmr_f32: list j of m has the candidates pool_items[j, 0:P] (int32 rows of T, the valid entries as a prefix, the
 * rest -1; no duplicates among the valid entries: a precondition) with the model's scores pool_scores[j, 0:P] (finite on valid
 * entries; the pool need not be sorted).
 *   - relevance, min-max normalised over the list's valid entries: rel_t = (r_t - r_min) / (r_max - r_min); every rel_t is 1 when
 *     r_max == r_min (one valid entry included).
 *   - step 0 picks argmax rel_t.  Step s >= 1 picks, among the valid unselected positions t,
 *         argmax v_t,   v_t = trade_off * rel_t - (1 - trade_off) * max_{u selected} sim(t, u)
 *     (the maximum runs over the selected set only: no implicit 0).  Ties go to the smaller pool position.  Step 0, and every
 *     step when 1 - trade_off is 0, compare the scores r_t themselves: the same order, without the rounding of rel.
 *   - steps beyond the number of valid entries write -1 / -inf.
 *   - out_items [m, k]: the chosen rows of T in selection order; out_scores [m, k]: their pool_scores, unmodified bits;
 *     out_mmr [m, k] (optional, may be NULL): the v values, v_0 = trade_off * rel; out_ild [m] (optional, double): the ILD of the
 *     chosen list as amar_list_diversity_f64 defines it at cutoff k (0 with fewer than 2 items), bit for bit.
 *   - trade_off = 1: the first k of the pool in (score descending, position ascending) order.
 * A list's result depends on its own row of the inputs, T, the metric, trade_off and k only: not on m, the other lists or the
 * grid; a call returns the same bits on every run (no atomics).  One launch, one wavefront per list, no workspace: nothing of size
 * m x P x P or m x P x d reaches memory.
 * Limits: 1 <= k <= P <= 64, d % 4 == 0, 4 <= d <= 512, ldt a multiple of 4, T 16-byte aligned; else AMAR_EUNSUPPORTED.  NULL
 * pointers (out_mmr / out_ild excepted; all but T may be NULL when m == 0), negative sizes, k < 1, P < 1, an unknown metric,
 * ldt < d, trade_off outside [0, 1] (NaN included): AMAR_EINVAL.  All of these are checked before any device call.
 * PRECONDITION: every valid item < n_rows; an entry outside 0..n_rows-1 is treated as padding, not read.
 *
 * amar_list_diversity_f64: lists [m, K] (int32 rows of T, -1 padded, K <= 64), HOST cutoffs ks[nk] (1 <= ks[q] <= K,
 * nk <= AMAR_RANK_METRICS_MAX_KS).  out_count [m, nk] (int32): the valid items among the first ks[q] ranks; out_ild [m, nk]
 * (double): the mean over the pairs a < b of those items of 1 - sim(a, b), 0 where the count is below 2.  The similarities are the
 * float32 values above; the pairs are summed in float64 in a fixed order (b ascending, a ascending inside b).  Limits and refusals
 * as above (K in place of P; nk < 1 or a cutoff outside [1, K]: AMAR_EINVAL; nk > AMAR_RANK_METRICS_MAX_KS: AMAR_EUNSUPPORTED). */
#define AMAR_DIVERSIFY_MAX_P 64
int amar_rerank_mmr_f32(const int32_t *pool_items, const float *pool_scores, int64_t m, int32_t P, const float *T, int64_t ldt,
                        int32_t n_rows, int32_t d, int32_t metric, float trade_off, int32_t k, int32_t *out_items,
                        float *out_scores, float *out_mmr, double *out_ild, amar_stream_t stream);
int amar_list_diversity_f64(const int32_t *lists, int64_t m, int32_t K, const float *T, int64_t ldt, int32_t n_rows, int32_t d,
                            int32_t metric, const int32_t *ks, int32_t nk, double *out_ild, int32_t *out_count,
                            amar_stream_t stream);

/* Explanations of recommended pairs: for every target of device lists, the liked items of the list's user that are most similar to
 * it, and the properties it shares with other liked items ("why this item for this user?").
 *
 * lists [m, K] (int32 rows of T, -1 padded: what amar_recommend_f32 writes); row j belongs to user users[j] (j itself when
 * users == NULL, m == n_users).  The liked items are a CSR over users: liked_ptr[n_users+1], liked_items sorted ascending and
 * de-duplicated per user.  T [n_items, d] (leading dimension ldt) is the item table; sim(a, b) is amar_nearest_f32's score of row
 * a against row b:
 *     AMAR_NEAREST_DOT:     sim(a, b) = sum_c T[a, c] * T[b, c]
 *     AMAR_NEAREST_COSINE:  sim(a, b) = (dot * inv_norm(T[a])) * inv_norm(T[b]),  inv_norm(x) = 1/sqrt(sum x^2), 0 when the sum is 0
 * (a zero row is similar to nothing, never NaN), products and sums in float32 (v_mfma_f32_16x16x4_f32, one fmaf chain per pair,
 * features in the fragment order 16t + 4g + r of amar_nearest_f32; the squared norms are fmaf chains over the columns, ascending).
 * The item-property links are an optional CSR over items: prop_ptr[n_items+1], prop_ids sorted ascending and de-duplicated per
 * item, values in 0..n_props-1, with the weights prop_weight[n_props]; all three NULL = no property part (the property outputs
 * are then padding).  For target i = lists[j, t] of user u:
 *   - out_evidence / out_evidence_sim [m, K, n_evidence]: the n_evidence items of liked(u) other than i with the largest
 *     sim(i, .), similarity descending, item row ascending on ties; padded with -1 / -inf.
 *   - for every property p of i:  support(p) = |{j in liked(u), j != i, p in props(j)}|  and
 *         score(p) = prop_weight[p] * sum over those j, item row ascending, of max(sim(i, j), 0).
 *     out_props / out_prop_score / out_prop_support [m, K, n_properties]: the n_properties properties of support > 0 with the
 *     largest scores, score descending, property index ascending on ties; padded with -1 / -inf / 0.  They may be NULL when
 *     n_properties == 0.
 * A padded list entry (or a row outside 0..n_items-1) writes padding only; a user id outside 0..n_users-1 writes padding for the
 * whole list.  A list's result depends on its own row of lists, its user's segment, the touched rows of T, the property rows and
 * weights, the metric, n_evidence and n_properties only: not on m, the other lists or the grid; a call returns the same bits on
 * every run (no atomics, in LDS either: every sum runs in liked-row order).  One launch, one wavefront per list, no workspace:
 * nothing of size m x L, m x K x L or m x L x d (L a liked-list length) reaches memory.  The user's liked rows are gathered once
 * per list while the property rows of the list's targets together hold at most AMAR_EXPLAIN_MAX_PROP_ROW entries, and once per
 * group of targets that does beyond.
 * max_prop_row: the longest row of the property CSR (a precondition; ignored without one).  PRECONDITIONS, not checked on the
 * device: max_prop_row is not understated (a target's row longer than AMAR_EXPLAIN_MAX_PROP_ROW that slips through that way is read
 * up to the cap only, so that LDS is never overrun: the result is then undefined, not an error); T and prop_weight are finite (a
 * similarity that is NaN counts as -inf in the evidence order, and a property whose score is NaN or -inf is not reported even with
 * support > 0).
 * Limits: K <= AMAR_EXPLAIN_MAX_K, 1 <= n_evidence <= AMAR_EXPLAIN_MAX_E, 0 <= n_properties <= AMAR_EXPLAIN_MAX_E, d % 4 == 0,
 * 4 <= d <= 512, ldt a multiple of 4, T 16-byte aligned, max_prop_row <= AMAR_EXPLAIN_MAX_PROP_ROW; else AMAR_EUNSUPPORTED (a longer
 * row is never truncated).  Liked lists and the property rows of liked items may have any length.  NULL T / liked_ptr, NULL lists
 * / liked_items / outputs with m > 0, negative sizes, K < 1, n_evidence < 1, n_properties < 0, an unknown metric, ldt < d,
 * users == NULL with m != n_users, some but not all of prop_ptr / prop_ids / prop_weight: AMAR_EINVAL.  All of these are checked
 * before any device call. */
#define AMAR_EXPLAIN_MAX_K        64
#define AMAR_EXPLAIN_MAX_E        16
#define AMAR_EXPLAIN_MAX_PROP_ROW 2048
int amar_explain_f32(const int32_t *lists, int64_t m, int32_t K, const int32_t *users, const int32_t *liked_ptr,
                     const int32_t *liked_items, int32_t n_users, const float *T, int64_t ldt, int32_t n_items, int32_t d,
                     int32_t metric, const int32_t *prop_ptr, const int32_t *prop_ids, const float *prop_weight, int32_t n_props,
                     int32_t max_prop_row, int32_t n_evidence, int32_t n_properties, int32_t *out_evidence,
                     float *out_evidence_sim, int32_t *out_props, float *out_prop_score, int32_t *out_prop_support,
                     amar_stream_t stream);

/* Calibrated re-ranking (Steck, "Calibrated recommendations", RecSys 2018): keep a list in proportion to the categories of what its
 * user liked, and measure how far a finished list is from that proportion.
 *
 * Categories: a CSR over item rows, cat_ptr[n_items+1] and cat_ids, every row sorted ascending and de-duplicated, values in 0..G-1,
 * 1 <= G <= AMAR_CALIBRATE_MAX_G.  len_i is the length of row i and p(g|i) = 1/len_i for g in row i; an item with an empty row is
 * NEUTRAL: it has no distribution.
 * User target: L(u) is the liked segment of u (the liked CSR of amar_explain_f32: liked_ptr[n_users+1], liked_items sorted ascending
 * and de-duplicated per user), L+(u) its items with a non-empty row, support(u) = |L+(u)|,
 *     psum(g) = sum over i in L+(u), item row ascending, of 1/len_i        p(g) = psum(g) / support(u);
 * a user with support 0 has no target.
 * List distribution: for the chosen items S in selection order, S+ the non-neutral ones,
 *     n(g) = sum over i in S+, selection order, of 1/len_i                  q(g) = n(g) / |S+|, 0 everywhere when S+ is empty.
 * Miscalibration, with the smoothing a (0 < a < 1):
 *     C(p, S) = sum over the g with p(g) > 0, g ascending, of  p(g) log( p(g) / ((1 - a) q(g) + a p(g)) ),
 * 0 <= C <= log(1/a), and C = log(1/a) when S+ is empty.
 *
 * amar_rerank_calibrated_f32: list j of m has the candidates pool_items[j, 0:P] (int32 item rows, -1 = padding, no duplicates among
 * the valid entries: a precondition) with the model's scores pool_scores[j, 0:P] (finite on valid entries; the pool need not be
 * sorted) and belongs to user users[j] (j itself when users == NULL, m == n_users).
 *   - rel_t is the min-max normalised score of amar_rerank_mmr_f32: (r_t - r_min) / (r_max - r_min) over the valid entries, 1
 *     everywhere when r_max == r_min.
 *   - every step s >= 0, step 0 included, picks among the valid unselected positions t
 *         argmax v_t,   v_t = trade_off * rel_t - (1 - trade_off) * C(p, S + {t}),
 *     ties to the smaller pool position.  When 1 - trade_off is 0, or the user has no target (C then counts as 0), the steps compare
 *     the scores r_t themselves: the score order, position ascending on ties.
 *   - steps beyond the number of valid entries write -1 / -inf; a user id outside 0..n_users-1 writes padding for the whole list
 *     (and a target of zeros).
 *   - out_items [m, k]: the chosen item rows in selection order; out_scores [m, k]: their pool_scores, unmodified bits;
 *     out_value [m, k] (optional, may be NULL): the v values; out_kl [m, k] (optional): C after each step; out_target [m, G]
 *     (optional): p, zeros for a user without a target.
 * Arithmetic, part of the contract: float32 throughout.  1/len_i is the correctly rounded quotient; psum and n are sequential
 * additions in the orders above; p = psum / support is one division; a is the float32 argument and 1 - a one float32 subtraction;
 * a cell's term is p * logf(p / fmaf(1 - a, x / N, a * p)) with x = n(g) and N = |S+| (x / N = 0 when N is 0), logf the accurate one
 * (no fast-math).  Per step the terms of all g are added once for N = |S+| and once for N = |S+| + 1 (lane l adds g = l, l + 64, ...
 * in that order, then a 6-level xor butterfly over the 64 lanes); a non-neutral candidate adds to the second sum, for the cells of
 * its row with p > 0 in row order, term(x + 1/len_t) - term(x); a neutral candidate takes the first sum.  out_target therefore has
 * the bits of a float32 loop on the host.
 * A list's result depends on its own row of the inputs, its user's liked segment, the touched category rows, trade_off, smoothing
 * and k only: not on m, the other lists or the grid; a call returns the same bits on every run (no atomics, in LDS either).  One
 * launch, one wavefront per list, no workspace: nothing of size m x P x G reaches memory.  p and n live in LDS; the pool's category
 * rows are staged there, position after position, while they fit AMAR_CALIBRATE_POOL_BUDGET entries together, and the positions past
 * that read their rows from memory: nothing is truncated.
 * max_cat_row: the longest row of the category CSR.  The host refuses a value that no valid CSR can have (negative; above G, since
 * a row is de-duplicated) and the kernel does not otherwise use it: whatever the caller states, a pool row is read up to G entries
 * only and an id outside 0..G-1 is skipped, so that LDS is never overrun; a CSR that breaks the rules above gives an undefined
 * result, not an error.  Pool or liked items outside 0..n_items-1 are padding and are never read.
 * Limits: 1 <= k <= P <= AMAR_CALIBRATE_MAX_P, G <= AMAR_CALIBRATE_MAX_G, max_cat_row <= G; else AMAR_EUNSUPPORTED.  NULL pointers
 * (out_value / out_kl / out_target and users excepted; the pools and outputs may be NULL when m == 0), negative sizes, P < 1, k < 1, G < 1, trade_off outside [0, 1] or smoothing
 * outside (0, 1) (NaN included), users == NULL with m != n_users: AMAR_EINVAL.  All of these are checked before any device call.
 *
 * amar_list_calibration_f64: lists [m, K] (int32 item rows, -1 padded, K <= 64) of users[j] (NULL as above), HOST cutoffs ks[nk]
 * (1 <= ks[q] <= K, nk <= AMAR_RANK_METRICS_MAX_KS).  out_kl [m, nk] (double) = C(p, the first ks[q] ranks) entirely in float64:
 * 1.0/len, the sums in the orders above, p = psum / support, a = (double)smoothing, the accurate log, g ascending; 0 for a user
 * without a target.  out_count [m, nk] (int32): the non-neutral valid items in those ranks; out_support [m] (int32): |L+(u)|, 0 for
 * a user id outside 0..n_users-1 (whose row is otherwise zeros).  Limits and refusals as above (K in place of P; nk < 1 or a cutoff
 * outside [1, K]: AMAR_EINVAL; nk > AMAR_RANK_METRICS_MAX_KS: AMAR_EUNSUPPORTED).  One wavefront per list, the same bits on every
 * run. */
#define AMAR_CALIBRATE_MAX_P       64
#define AMAR_CALIBRATE_MAX_G       1024
#define AMAR_CALIBRATE_POOL_BUDGET 4096
int amar_rerank_calibrated_f32(const int32_t *pool_items, const float *pool_scores, int64_t m, int32_t P, const int32_t *users,
                               const int32_t *liked_ptr, const int32_t *liked_items, int32_t n_users, const int32_t *cat_ptr,
                               const int32_t *cat_ids, int32_t n_items, int32_t G, int32_t max_cat_row, float trade_off,
                               float smoothing, int32_t k, int32_t *out_items, float *out_scores, float *out_value, float *out_kl,
                               float *out_target, amar_stream_t stream);
int amar_list_calibration_f64(const int32_t *lists, int64_t m, int32_t K, const int32_t *users, const int32_t *liked_ptr,
                              const int32_t *liked_items, int32_t n_users, const int32_t *cat_ptr, const int32_t *cat_ids,
                              int32_t n_items, int32_t G, float smoothing, const int32_t *ks, int32_t nk, double *out_kl,
                              int32_t *out_count, int32_t *out_support, amar_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AMAR_HIP_H */

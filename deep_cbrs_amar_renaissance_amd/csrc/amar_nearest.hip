// Nearest rows of a table: fused dot / cosine score-and-select (gfx950).  "Which items are like this one?" over the vectors the
// models learn (the propagated node table, the first-stage towers), without the m x n_rows score matrix ever reaching memory.
//
//     dot:     score(j, i) = sum_c Q[q_j, c] * T[i, c]
//     cosine:  score(j, i) = (dot * inv_norm(Q[q_j])) * inv_norm(T[i])        inv_norm(x) = 1/sqrt(sum x^2), 0 for a zero row
//
// Decomposition:
//   * cosine only: nearest_norm_kernel writes inv_norm once per table row and once per listed query into a workspace vector
//     (16 lanes per row, a fixed summation order that depends on d alone).
//   * nearest_kernel, grid (query blocks of 16, table slices), 4 waves.  The block's 16 query rows are staged in LDS once; per
//     table tile the workgroup stages TR rows of T, then
//       - product: the tile's 16-row units are dealt to the waves; a unit is one 16 x 16 accumulator of v_mfma_f32_16x16x4_f32
//         (A = the 16 queries, B = 16 table rows, both read from LDS as float4 at features 16t + 4g + r, the fragment order of
//         rank_topk_kernel / chain_kernel: t ascending, r ascending inside t, one fmaf chain per score).  The scaled scores go to
//         a [16][TR] LDS window: the matrix layout holds 4 queries x 16 rows per register, the selection wants 64 rows of one query.
//       - selection: the RankSlot of amar_rank_select.h, one per query (the selector rank_topk_kernel uses); each wave owns 4
//         queries and hands its slots the window's scores 64 rows at a time.
//   * with several table slices each workgroup leaves its slice's list in a workspace and rank_merge_slices (amar_rank.hip)
//     merges them in slice order; the order is a strict total order, so the result does not depend on the slicing.
// A score depends on its query row, its table row, d and the metric only: not on the block, the tile, the slice or the call.
#include "amar_common.h"
#include "amar_rank_select.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NEAR_WAVES = 4, NEAR_QPW = 4, NEAR_QB = NEAR_WAVES * NEAR_QPW;     // queries per wave, per workgroup
constexpr int NEAR_TILE_BYTES = 48 * 1024;
constexpr int NEAR_MAX_D = 512;

struct NearArgs {
    const float *Q; int64_t ldq; const float *T; int64_t ldt; int d, n_rows, cosine;
    const int32_t *query_rows; int64_t m;
    const int32_t *excl_ptr, *excl_rows;
    const float *t_inv, *q_inv;                // cosine: inverse norms per table row / per listed query
    int kt, tile_rows, stride, sstride, slice_rows;
    RankOut out;
};

// inv_norm of n rows of X (rows[j] or j itself), 16 lanes per row: lane s squares the float4s s, s + 16, ... in that order,
// then the 16 partial sums meet in a fixed xor tree.
__global__ __launch_bounds__(256) void nearest_norm_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows,
                                                           int64_t n, float *__restrict__ out) {
    const int sub = threadIdx.x & 15;
    const int64_t j = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    float s = 0.f;
    if (j < n) {
        const float *x = X + (int64_t)(rows ? rows[j] : j) * ld;
        for (int f = 4 * sub; f < d; f += 64) {
            const float4 v = *reinterpret_cast<const float4 *>(x + f);
            s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
        }
    }
    s += __shfl_xor(s, 8, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    if (j < n && sub == 0) out[j] = s > 0.f ? 1.f / sqrtf(s) : 0.f;
}

__global__ __launch_bounds__(256) void nearest_kernel(const NearArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *q_lds = lds;                                              // [16][stride]
    float *tile = q_lds + NEAR_QB * a.stride;                        // [tile_rows][stride]
    float *sc = tile + a.tile_rows * a.stride;                       // [16][sstride]: the tile's scores
    float *t_inv = sc + NEAR_QB * a.sstride;                         // [tile_rows]
    float *q_inv = t_inv + a.tile_rows;                              // [16]
    float *select = q_inv + NEAR_QB;                                 // NEAR_QB selector slots (amar_rank_select.h)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * NEAR_QB;
    const int slice = blockIdx.y;
    const int s0 = slice * a.slice_rows, s1 = min(a.n_rows, s0 + a.slice_rows);
    const int f4_per_row = 4 * a.kt;                             // float4s of a staged row (16 kt features, zero past d)

    for (int idx = threadIdx.x; idx < NEAR_QB * f4_per_row; idx += blockDim.x) {
        const int r = idx / f4_per_row, f = 4 * (idx - r * f4_per_row);
        const int64_t j = j0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < a.m && f < a.d) v = *reinterpret_cast<const float4 *>(a.Q + (int64_t)(a.query_rows ? a.query_rows[j] : j) * a.ldq + f);
        *reinterpret_cast<float4 *>(&q_lds[r * a.stride + f]) = v;
    }
    if (threadIdx.x < NEAR_QB) {
        const int64_t j = j0 + threadIdx.x;
        q_inv[threadIdx.x] = (a.cosine && j < a.m) ? a.q_inv[j] : 1.f;
    }
    for (int qw = 0; qw < NEAR_QPW; ++qw) {
        const int slot = wave * NEAR_QPW + qw;
        const int64_t j = j0 + slot;
        int eb = 0, ee = 0;                                      // the query's excluded rows
        if (lane == 0 && j < a.m && a.excl_ptr) { eb = a.excl_ptr[j]; ee = a.excl_ptr[j + 1]; }
        RankSlot<NEAR_QB>(select, slot).init(lane, a.excl_rows, eb, ee, s0);
    }

    for (int t0 = s0; t0 < s1; t0 += a.tile_rows) {
        const int rows = min(a.tile_rows, s1 - t0);
        __syncthreads();                                         // the previous tile and its scores are no longer read
        for (int idx = threadIdx.x; idx < a.tile_rows * f4_per_row; idx += blockDim.x) {
            const int r = idx / f4_per_row, f = 4 * (idx - r * f4_per_row);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && f < a.d) v = *reinterpret_cast<const float4 *>(a.T + (int64_t)(t0 + r) * a.ldt + f);
            *reinterpret_cast<float4 *>(&tile[r * a.stride + f]) = v;
        }
        for (int r = threadIdx.x; r < a.tile_rows; r += blockDim.x) t_inv[r] = (a.cosine && r < rows) ? a.t_inv[t0 + r] : 1.f;
        __syncthreads();

        // product: units wave, wave + 4 (two accumulator chains in flight), then wave + 8, wave + 12, ...
        const int units = (rows + 15) >> 4;
        for (int u = wave; u < units; u += 2 * NEAR_WAVES) {
            const bool two = u + NEAR_WAVES < units;
            const float *qa = q_lds + col * a.stride + 4 * g;
            const float *b0 = tile + (16 * u + col) * a.stride + 4 * g;
            const float *b1 = two ? b0 + 16 * NEAR_WAVES * a.stride : b0;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < a.kt; ++t) {
                const f32x4 q4 = *reinterpret_cast<const f32x4 *>(qa + 16 * t);
                const f32x4 x0 = *reinterpret_cast<const f32x4 *>(b0 + 16 * t);
                const f32x4 x1 = *reinterpret_cast<const f32x4 *>(b1 + 16 * t);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[r], x0[r], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[r], x1[r], acc1, 0, 0, 0);
                }
            }
            // lane (g, col), register r: query 4g + r of the block against table row 16u + col of the tile
            const float ti0 = t_inv[16 * u + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = a.cosine ? (acc0[r] * q_inv[4 * g + r]) * ti0 : acc0[r];
                sc[(4 * g + r) * a.sstride + 16 * u + col] = z;
            }
            if (two) {
                const float ti1 = t_inv[16 * (u + NEAR_WAVES) + col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = a.cosine ? (acc1[r] * q_inv[4 * g + r]) * ti1 : acc1[r];
                    sc[(4 * g + r) * a.sstride + 16 * (u + NEAR_WAVES) + col] = z;
                }
            }
        }
        __syncthreads();

        for (int qw = 0; qw < NEAR_QPW; ++qw) {
            const int slot = wave * NEAR_QPW + qw;
            const int64_t j = j0 + slot;
            if (j >= a.m) break;
            RankSlot<NEAR_QB> top(select, slot);
            top.load();
            const int ee = a.excl_ptr ? a.excl_ptr[j + 1] : 0;
            const float *srow = sc + slot * a.sstride;

            for (int grp = 0; grp < rows; grp += 64) {
                const bool in = grp + lane < rows;
                const float z = in ? srow[grp + lane] : -INFINITY;
                top.offer(z, t0 + grp + lane, in, a.excl_rows, ee, a.out.k, lane);
            }
            top.advance(a.excl_rows, ee, t0 + rows);
            top.store(lane);
        }
    }
    __syncthreads();                                             // n_rows == 0: the lists and states above are written
    for (int qw = 0; qw < NEAR_QPW; ++qw) {
        const int slot = wave * NEAR_QPW + qw;
        const int64_t j = j0 + slot;
        if (j >= a.m) break;
        RankSlot<NEAR_QB>(select, slot).finish(j, slice, a.out, lane);
    }
}

// Launch geometry of a width: staged row stride (features padded to 16, +4 floats so neighbouring rows start on different
// banks) and the rows of a tile (a power of two in 32..256 whose rows fit NEAR_TILE_BYTES; 32 at the widest).
struct NearShape { int kt, stride, tile_rows, sstride; };

int near_shape(int d, NearShape &s) {
    if (d < 4 || (d & 3) || d > NEAR_MAX_D) return AMAR_EUNSUPPORTED;
    s.kt = (d + 15) / 16;
    s.stride = 16 * s.kt + 4;
    const int fit = NEAR_TILE_BYTES / (4 * s.stride);
    int tr = 256;
    while (tr > 32 && tr > fit) tr >>= 1;
    s.tile_rows = tr;
    s.sstride = tr + 4;
    return AMAR_OK;
}

inline int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

}  // namespace

extern "C" {

int32_t amar_nearest_slices(int64_t m, int32_t n_rows, int32_t d, int32_t n_slices) {
    if (m < 0 || n_rows < 0 || d < 0) return AMAR_EINVAL;
    NearShape s;
    const int rc = near_shape(d, s);
    if (rc != AMAR_OK) return rc;
    return rank_slices(m, n_rows, s.tile_rows, NEAR_QB, n_slices);
}

int64_t amar_nearest_workspace_floats(int64_t m, int32_t n_rows, int32_t k, int32_t metric, int32_t slices) {
    if (m < 0 || n_rows < 0 || k < 1 || slices < 1 || (metric != AMAR_NEAREST_DOT && metric != AMAR_NEAREST_COSINE)) return AMAR_EINVAL;
    const int64_t norms = metric == AMAR_NEAREST_COSINE ? round4(n_rows) + round4(m) : 0;
    return norms + (slices > 1 ? m * slices * k : 0);
}

int amar_nearest_f32(const float *Q, int64_t ldq, int32_t n_queries, const float *T, int64_t ldt, int32_t n_rows, int32_t d,
                     int32_t metric, const int32_t *query_rows, int64_t m, const int32_t *excl_ptr, const int32_t *excl_rows,
                     int32_t k, int32_t n_slices, int32_t *workspace_rows, float *workspace_scores,
                     int32_t *out_rows, float *out_scores, amar_stream_t stream) {
    if (!Q || !T || m < 0 || n_queries < 0 || n_rows < 0 || d < 0 || k < 1) return AMAR_EINVAL;
    if (metric != AMAR_NEAREST_DOT && metric != AMAR_NEAREST_COSINE) return AMAR_EINVAL;
    if (!query_rows && m != n_queries) return AMAR_EINVAL;
    if (excl_ptr && !excl_rows) return AMAR_EINVAL;
    if (ldq < d || ldt < d) return AMAR_EINVAL;
    if (k > RANK_LIST) return AMAR_EUNSUPPORTED;
    NearShape sh;
    const int rc = near_shape(d, sh);
    if (rc != AMAR_OK) return rc;
    if ((ldq & 3) || (ldt & 3) || !amar_aligned16(Q) || !amar_aligned16(T)) return AMAR_EUNSUPPORTED;
    const int32_t slices = amar_nearest_slices(m, n_rows, d, n_slices);
    if (slices < 1) return slices < 0 ? slices : AMAR_EINVAL;
    if (n_slices > 0 && slices != n_slices) return AMAR_EINVAL;       // the caller sizes the workspace from amar_nearest_slices
    const bool cosine = metric == AMAR_NEAREST_COSINE;
    if (slices > 1 && !workspace_rows) return AMAR_EINVAL;
    if ((slices > 1 || cosine) && (!workspace_scores || !amar_aligned16(workspace_scores))) return AMAR_EINVAL;
    if (m == 0) return AMAR_OK;
    if (!out_rows || !out_scores) return AMAR_EINVAL;
    const int64_t blocks = (m + NEAR_QB - 1) / NEAR_QB;
    if (blocks >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);

    // workspace_scores: [inv_norm of the table rows | inv_norm of the listed queries] (cosine), then the per-slice scores
    float *t_inv = workspace_scores, *q_inv = workspace_scores + (cosine ? round4(n_rows) : 0);
    float *part_scores = workspace_scores + (cosine ? round4(n_rows) + round4(m) : 0);
    if (cosine) {
        if (n_rows > 0) {
            hipLaunchKernelGGL(nearest_norm_kernel, dim3((unsigned)((n_rows + 15) / 16)), dim3(256), 0, st, T, ldt, d,
                               (const int32_t *)nullptr, (int64_t)n_rows, t_inv);
            const int e = amar_check_launch();
            if (e != AMAR_OK) return e;
        }
        hipLaunchKernelGGL(nearest_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, st, Q, ldq, d, query_rows, m, q_inv);
        const int e = amar_check_launch();
        if (e != AMAR_OK) return e;
    }

    NearArgs a{};
    a.Q = Q; a.ldq = ldq; a.T = T; a.ldt = ldt; a.d = d; a.n_rows = n_rows; a.cosine = cosine ? 1 : 0;
    a.query_rows = query_rows; a.m = m; a.excl_ptr = excl_ptr; a.excl_rows = excl_rows;
    a.t_inv = t_inv; a.q_inv = q_inv;
    a.out.k = k; a.kt = sh.kt; a.tile_rows = sh.tile_rows; a.stride = sh.stride; a.sstride = sh.sstride;
    a.slice_rows = (int)rank_slice_rows(n_rows, sh.tile_rows, slices);
    a.out.n_slices = slices;
    a.out.rows = slices > 1 ? workspace_rows : out_rows;
    a.out.scores = slices > 1 ? part_scores : out_scores;
    const size_t lds_bytes = ((size_t)(NEAR_QB + sh.tile_rows) * sh.stride + (size_t)NEAR_QB * sh.sstride + sh.tile_rows + NEAR_QB +
                              (size_t)rank_select_state_floats(NEAR_QB)) * 4;
    if (lds_bytes > 160 * 1024) return AMAR_EUNSUPPORTED;
    if (lds_bytes > 64 * 1024) {
        static bool done[AMAR_MAX_DEVICES];
        const int e = amar_allow_lds(reinterpret_cast<const void *>(nearest_kernel), 160 * 1024, done);
        if (e != AMAR_OK) return e;
    }
    hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)blocks, (unsigned)slices), dim3(256), lds_bytes, st, a);
    const int e = amar_check_launch();
    if (e != AMAR_OK || slices == 1) return e;
    return rank_merge_slices(workspace_rows, part_scores, m, slices, k, out_rows, out_scores, st);
}

}  // extern "C"

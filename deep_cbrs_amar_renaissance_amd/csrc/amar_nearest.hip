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
//         recommend_kernel / chain_kernel: t ascending, r ascending inside t, one fmaf chain per score).  The scaled scores go to
//         a [16][TR] LDS window: the matrix layout holds 4 queries x 16 rows per register, the selection wants 64 rows of one query.
//       - selection (amar_rank_select.h, the scheme of recommend_kernel): each wave owns 4 queries; per query a threshold = the
//         current k-th best (score, row), a forward-walking exclusion pointer with a binary search in the remaining window, a
//         64-entry candidate buffer merged into the sorted list by rank counting.
//   * with several table slices each workgroup leaves its slice's list in a workspace and recommend_merge_kernel merges them in
//     slice order; the order is a strict total order, so the result does not depend on the slicing.
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
    int k, kt, tile_rows, stride, sstride, slice_rows, n_slices;
    int32_t *out_rows; float *out_scores;      // n_slices == 1: the result [m, k]; else the per-slice lists [m][n_slices][k]
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
    float *list_s = q_inv + NEAR_QB;
    int *list_i = reinterpret_cast<int *>(list_s + NEAR_QB * RANK_LIST);
    float *cand_s = reinterpret_cast<float *>(list_i + NEAR_QB * RANK_LIST);
    int *cand_i = reinterpret_cast<int *>(cand_s + NEAR_QB * RANK_CAND);
    int *st_cnt = cand_i + NEAR_QB * RANK_CAND;          // per query: candidates buffered, exclusion pointer, threshold
    int *st_ep = st_cnt + NEAR_QB;
    float *st_ts = reinterpret_cast<float *>(st_ep + NEAR_QB);
    int *st_ti = reinterpret_cast<int *>(st_ts + NEAR_QB);

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
        list_s[slot * RANK_LIST + lane] = -INFINITY;
        list_i[slot * RANK_LIST + lane] = RANK_EMPTY;
        if (lane == 0) {
            const int64_t j = j0 + slot;
            int ep = 0;
            if (j < a.m && a.excl_ptr) ep = rank_lower_bound(a.excl_rows, a.excl_ptr[j], a.excl_ptr[j + 1], s0);
            st_cnt[slot] = 0; st_ep[slot] = ep; st_ts[slot] = -INFINITY; st_ti[slot] = RANK_EMPTY;
        }
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
            int cnt = st_cnt[slot], ep = st_ep[slot];
            float ts = st_ts[slot];
            int ti = st_ti[slot];
            const int ee = a.excl_ptr ? a.excl_ptr[j + 1] : 0;
            float *ls = list_s + slot * RANK_LIST, *cs = cand_s + slot * RANK_CAND;
            int *li = list_i + slot * RANK_LIST, *ci = cand_i + slot * RANK_CAND;
            const float *srow = sc + slot * a.sstride;

            for (int grp = 0; grp < rows; grp += 64) {
                const bool in = grp + lane < rows;
                const float z = in ? srow[grp + lane] : -INFINITY;
                const int item = t0 + grp + lane;
                bool pred = in && rank_better(z, item, ts, ti);
                if (__ballot(pred) == 0) continue;
                if (pred && ep < ee) {                               // excluded for this query?
                    const int pos = rank_lower_bound(a.excl_rows, ep, ee, item);
                    pred = !(pos < ee && a.excl_rows[pos] == item);
                }
                const uint64_t mask = __ballot(pred);
                if (mask == 0) continue;
                const int n = __popcll(mask);
                if (cnt + n > RANK_CAND) {
                    rank_merge(ls, li, cs, ci, cnt, a.k, lane);
                    cnt = 0;
                    ts = ls[a.k - 1]; ti = li[a.k - 1];
                    pred = pred && rank_better(z, item, ts, ti);
                }
                const uint64_t mask2 = __ballot(pred);
                if (pred) {
                    const int pos = cnt + __popcll(mask2 & ((1ull << lane) - 1ull));
                    cs[pos] = z; ci[pos] = item;
                }
                cnt += __popcll(mask2);
            }
            // the exclusion pointer moves past this tile
            if (a.excl_ptr && ep < ee) ep = rank_lower_bound(a.excl_rows, ep, ee, t0 + rows);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) { st_cnt[slot] = cnt; st_ep[slot] = ep; st_ts[slot] = ts; st_ti[slot] = ti; }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();                                             // n_rows == 0: the lists and states above are written
    // slice done: last merge, then the list goes out (final result or this slice's partial list)
    for (int qw = 0; qw < NEAR_QPW; ++qw) {
        const int slot = wave * NEAR_QPW + qw;
        const int64_t j = j0 + slot;
        if (j >= a.m) break;
        float *ls = list_s + slot * RANK_LIST;
        int *li = list_i + slot * RANK_LIST;
        const int cnt = st_cnt[slot];
        if (cnt > 0) rank_merge(ls, li, cand_s + slot * RANK_CAND, cand_i + slot * RANK_CAND, cnt, a.k, lane);
        if (lane < a.k) {
            const float s = ls[lane];
            const int i = li[lane];
            if (a.n_slices == 1) {
                a.out_rows[j * a.k + lane] = i == RANK_EMPTY ? -1 : i;
                a.out_scores[j * a.k + lane] = i == RANK_EMPTY ? -INFINITY : s;
            } else {
                const int64_t o = (j * a.n_slices + slice) * a.k + lane;
                a.out_rows[o] = i;
                a.out_scores[o] = s;
            }
        }
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
    const int64_t tiles = ((int64_t)n_rows + s.tile_rows - 1) / s.tile_rows;
    const int64_t blocks = (m + NEAR_QB - 1) / NEAR_QB;
    int64_t want = n_slices;
    if (want <= 0) {
        // automatic: about four resident workgroups per CU of the 256 (a slice covers at least four tiles)
        want = blocks > 0 ? (1024 + blocks - 1) / blocks : 1;
        const int64_t cap = tiles / 4 > 0 ? tiles / 4 : 1;
        want = want > cap ? cap : want;
        want = want > 16 ? 16 : want;
    }
    if (want < 1) want = 1;
    if (want > tiles) want = tiles > 0 ? tiles : 1;
    if (want > 64) want = 64;
    // slices cover whole tiles: the count actually launched
    const int64_t per = ((tiles + want - 1) / want) * s.tile_rows;
    const int64_t eff = per > 0 ? (n_rows + per - 1) / per : 1;
    return (int32_t)(eff > 0 ? eff : 1);
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

    const int64_t tiles = ((int64_t)n_rows + sh.tile_rows - 1) / sh.tile_rows;
    const int64_t per_tiles = (tiles + slices - 1) / slices;
    NearArgs a{};
    a.Q = Q; a.ldq = ldq; a.T = T; a.ldt = ldt; a.d = d; a.n_rows = n_rows; a.cosine = cosine ? 1 : 0;
    a.query_rows = query_rows; a.m = m; a.excl_ptr = excl_ptr; a.excl_rows = excl_rows;
    a.t_inv = t_inv; a.q_inv = q_inv;
    a.k = k; a.kt = sh.kt; a.tile_rows = sh.tile_rows; a.stride = sh.stride; a.sstride = sh.sstride;
    a.slice_rows = (int)(per_tiles * sh.tile_rows > 0 ? per_tiles * sh.tile_rows : sh.tile_rows);
    a.n_slices = slices;
    a.out_rows = slices > 1 ? workspace_rows : out_rows;
    a.out_scores = slices > 1 ? part_scores : out_scores;
    const size_t lds_bytes = ((size_t)(NEAR_QB + sh.tile_rows) * sh.stride + (size_t)NEAR_QB * sh.sstride + sh.tile_rows + NEAR_QB +
                              (size_t)NEAR_QB * (2 * RANK_LIST + 2 * RANK_CAND + 4)) * 4;
    if (lds_bytes > 160 * 1024) return AMAR_EUNSUPPORTED;
    if (lds_bytes > 64 * 1024) {
        static bool done[AMAR_MAX_DEVICES];
        const int e = amar_allow_lds(reinterpret_cast<const void *>(nearest_kernel), 160 * 1024, done);
        if (e != AMAR_OK) return e;
    }
    hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)blocks, (unsigned)slices), dim3(256), lds_bytes, st, a);
    const int e = amar_check_launch();
    if (e != AMAR_OK || slices == 1) return e;
    hipLaunchKernelGGL(recommend_merge_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, workspace_rows, part_scores, m, slices,
                       k, out_rows, out_scores);
    return amar_check_launch();
}

}  // extern "C"

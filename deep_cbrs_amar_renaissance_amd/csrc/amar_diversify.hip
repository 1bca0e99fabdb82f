// Diversified re-ranking: greedy MMR over a pool of at most 64 candidates, and the intra-list diversity of finished lists (gfx950).
//
// One wavefront (one 64-thread workgroup) per list; lane t owns position t of the list.
//   * Gram stage (shared by both kernels): the list's rows of T are gathered through LDS in chunks of 64 columns ([64][68] floats:
//     the pad puts neighbouring rows four banks apart); per 16 columns every 16-row unit is read once as float4 fragments (features
//     16t + 4g + r, the fragment order of nearest_kernel) and the NT x NT accumulators of v_mfma_f32_16x16x4_f32 (NT = ceil(P / 16),
//     a template parameter so that they stay in registers) take 4 k-steps each.  Rows past the list and columns past d are staged as
//     zeros.  After the last chunk the accumulators are written over the staging area: G[64][68], 17 KB.  G is bitwise symmetric
//     (the two products of a k-step commute) and an entry depends on its two rows of T and d only, not on where the rows stand.
//   * inverse norms: 1 / sqrt(G[t][t]), 0 for a zero row.
//   * MMR: rel, the running penalty and the selected flag live in one register each per lane; a step is a 6-level xor butterfly
//     over (key, position), four broadcasts of the winner and one read of the row G[t*][.] (consecutive addresses).
//   * ILD: lane b sums 1 - sim(a, b) over a < b in float64 (rows G[a][.], consecutive addresses), then the row sums are added in
//     lane order; lane b keeps the prefix, which is the pair sum of the first b + 1 ranks.
// No atomics, no scratch, no workspace in memory.
#include "amar_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DIV_P = AMAR_DIVERSIFY_MAX_P;      // list positions = lanes
constexpr int DIV_STRIDE = DIV_P + 4;            // floats per LDS row, of the staged chunk and of G
constexpr int DIV_CHUNK = 64;                    // columns staged at a time
constexpr int DIV_MAX_D = 512;

// G[a][b] = sum_c T[item_a, c] T[item_b, c] for the 16 NT positions of the list; `item` is the lane's row of T or -1.
template <int NT>
__device__ __forceinline__ void gram_stage(const float *__restrict__ T, int64_t ldt, int d, int item, float *lds, int lane) {
    const int g = lane >> 4, col = lane & 15;
    f32x4 acc[NT][NT];
#pragma unroll
    for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = 0; bj < NT; ++bj) acc[bi][bj] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < d; c0 += DIV_CHUNK) {
        __syncthreads();                                         // the previous chunk is no longer read
#pragma unroll
        for (int i = 0; i < 4 * NT; ++i) {                       // 16 NT rows x 16 float4s, 16 lanes per row
            const int idx = lane + 64 * i, r = idx >> 4, f = 4 * (idx & 15);
            const int it = __shfl(item, r, 64);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (it >= 0 && c0 + f < d) v = *reinterpret_cast<const float4 *>(T + (int64_t)it * ldt + c0 + f);
            *reinterpret_cast<float4 *>(&lds[r * DIV_STRIDE + f]) = v;
        }
        __syncthreads();
        const int steps = min(DIV_CHUNK / 16, (d - c0 + 15) >> 4);
        for (int t = 0; t < steps; ++t) {
            f32x4 x[NT];
#pragma unroll
            for (int b = 0; b < NT; ++b) x[b] = *reinterpret_cast<const f32x4 *>(&lds[(16 * b + col) * DIV_STRIDE + 16 * t + 4 * g]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int bi = 0; bi < NT; ++bi)
#pragma unroll
                    for (int bj = 0; bj < NT; ++bj)
                        acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[bi][r], x[bj][r], acc[bi][bj], 0, 0, 0);
        }
    }
    __syncthreads();
    // lane (g, col), register r of unit (bi, bj): position 16 bi + 4 g + r against position 16 bj + col
#pragma unroll
    for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = 0; bj < NT; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[(16 * bi + 4 * g + r) * DIV_STRIDE + 16 * bj + col] = acc[bi][bj][r];
    __syncthreads();
}

// Lanes past the 16 NT positions that gram_stage wrote hold no entry of G: they read nothing and get 1.
__device__ __forceinline__ float inv_norm_of(const float *G, int lane, int cosine, int written) {
    if (!cosine || lane >= written) return 1.f;
    const float s = G[lane * DIV_STRIDE + lane];
    return s > 0.f ? 1.f / sqrtf(s) : 0.f;
}

// sim of positions a and b of G, a the first factor: the association both kernels use, so that their ILDs agree bit for bit.
__device__ __forceinline__ float sim_of(float g, float inv_a, float inv_b, int cosine) { return cosine ? (g * inv_a) * inv_b : g; }

// Rank b = this lane holds position `pos` of G (any position in 0..63 where the rank is not in `ranks`) with inverse norm `inv`.
// Returns the sum over the ranks b' <= b and a < b', both in `ranks`, of 1 - sim(a, b'): b' ascending, a ascending inside b'.
__device__ __forceinline__ double ild_prefix(const float *G, int pos, float inv, uint64_t ranks, int n, int cosine, int lane) {
    const bool mine = (ranks >> lane) & 1ull;
    double row = 0.0;
    for (int a = 0; a < n; ++a) {
        const int pa = __shfl(pos, a, 64);
        const float ia = __shfl(inv, a, 64);
        if (mine && a < lane && ((ranks >> a) & 1ull)) row += 1.0 - (double)sim_of(G[pa * DIV_STRIDE + pos], ia, inv, cosine);
    }
    double run = 0.0, prefix = 0.0;
    for (int b = 0; b < n; ++b) {
        run += __shfl(row, b, 64);
        if (lane == b) prefix = run;
    }
    return prefix;
}

__device__ __forceinline__ double ild_mean(double pair_sum, int count) {
    return count < 2 ? 0.0 : pair_sum / (0.5 * (double)count * (double)(count - 1));
}

struct MmrArgs {
    const int32_t *pool_items; const float *pool_scores; int P;
    const float *T; int64_t ldt; int n_rows, d, cosine;
    float lambda; int k;
    int32_t *out_items; float *out_scores, *out_mmr; double *out_ild;
};

template <int NT>
__global__ __launch_bounds__(64) void rerank_mmr_kernel(const MmrArgs a) {
    __shared__ __attribute__((aligned(16))) float G[DIV_P * DIV_STRIDE];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    int item = -1;
    float score = 0.f;
    if (lane < a.P) {
        item = a.pool_items[j * a.P + lane];
        score = a.pool_scores[j * a.P + lane];
    }
    if (item < 0 || item >= a.n_rows) item = -1;
    gram_stage<NT>(a.T, a.ldt, a.d, item, G, lane);

    const bool valid = item >= 0;
    const int n_valid = __popcll(__ballot(valid));
    const float inv = inv_norm_of(G, lane, a.cosine, 16 * NT);
    float r_min = valid ? score : INFINITY, r_max = valid ? score : -INFINITY;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        r_min = fminf(r_min, __shfl_xor(r_min, off, 64));
        r_max = fmaxf(r_max, __shfl_xor(r_max, off, 64));
    }
    const float rel = r_max > r_min ? (score - r_min) / (r_max - r_min) : 1.f;
    const float lrel = a.lambda * rel, oml = 1.f - a.lambda;

    float pen = -INFINITY;
    bool selected = false;
    int o_item = -1, o_pos = 0, n_sel = 0;
    float o_score = -INFINITY, o_mmr = -INFINITY;
    const int steps = min(a.k, n_valid);
    for (int s = 0; s < steps; ++s) {
        const float v = s == 0 ? lrel : lrel - oml * pen;
        float key = (s == 0 || oml == 0.f) ? score : v;
        if (!(key == key)) key = -INFINITY;                      // a NaN (non-finite input) must not break the order's totality
        const bool cand = valid && !selected;
        float bk = cand ? key : -INFINITY;
        int bp = cand ? lane : 64 + lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ok = __shfl_xor(bk, off, 64);
            const int op = __shfl_xor(bp, off, 64);
            if (ok > bk || (ok == bk && op < bp)) { bk = ok; bp = op; }
        }
        const int t = __builtin_amdgcn_readfirstlane(bp);
        if (t >= DIV_P) break;
        const int t_item = __shfl(item, t, 64);
        const float t_score = __shfl(score, t, 64), t_v = __shfl(v, t, 64), t_inv = __shfl(inv, t, 64);
        if (lane == s) { o_item = t_item; o_score = t_score; o_mmr = t_v; o_pos = t; }
        if (lane == t) selected = true;
        if (lane < 16 * NT) pen = fmaxf(pen, sim_of(G[t * DIV_STRIDE + lane], t_inv, inv, a.cosine));   // columns past 16 NT are not G
        n_sel = s + 1;
    }
    if (lane < a.k) {
        a.out_items[j * a.k + lane] = o_item;
        a.out_scores[j * a.k + lane] = o_score;
        if (a.out_mmr) a.out_mmr[j * a.k + lane] = o_mmr;
    }
    if (a.out_ild) {
        const uint64_t ranks = n_sel >= 64 ? ~0ull : (1ull << n_sel) - 1ull;
        const float o_inv = __shfl(inv, o_pos, 64);
        const double prefix = ild_prefix(G, o_pos, o_inv, ranks, n_sel, a.cosine, lane);
        const double total = __shfl(prefix, n_sel > 0 ? n_sel - 1 : 0, 64);
        if (lane == 0) a.out_ild[j] = ild_mean(total, n_sel);
    }
}

struct DivArgs {
    const int32_t *lists; int K;
    const float *T; int64_t ldt; int n_rows, d, cosine;
    int nk, ks[AMAR_RANK_METRICS_MAX_KS];
    double *out_ild; int32_t *out_count;
};

template <int NT>
__global__ __launch_bounds__(64) void list_diversity_kernel(const DivArgs a) {
    __shared__ __attribute__((aligned(16))) float G[DIV_P * DIV_STRIDE];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    int item = -1;
    if (lane < a.K) item = a.lists[j * a.K + lane];
    if (item < 0 || item >= a.n_rows) item = -1;
    gram_stage<NT>(a.T, a.ldt, a.d, item, G, lane);
    const uint64_t ranks = __ballot(item >= 0);
    const float inv = inv_norm_of(G, lane, a.cosine, 16 * NT);
    const double prefix = ild_prefix(G, lane, inv, ranks, a.K, a.cosine, lane);
#pragma unroll
    for (int q = 0; q < AMAR_RANK_METRICS_MAX_KS; ++q) {
        if (q >= a.nk) break;
        const int kq = a.ks[q];
        const int count = __popcll(ranks & (kq >= 64 ? ~0ull : (1ull << kq) - 1ull));
        const double total = __shfl(prefix, kq - 1, 64);
        if (lane == 0) {
            a.out_ild[j * a.nk + q] = ild_mean(total, count);
            a.out_count[j * a.nk + q] = count;
        }
    }
}

// What both entries refuse before any device call.
int diversify_check(int64_t m, int32_t P, const float *T, int64_t ldt, int32_t n_rows, int32_t d, int32_t metric) {
    if (!T || m < 0 || P < 1 || n_rows < 0 || d < 0) return AMAR_EINVAL;
    if (metric != AMAR_NEAREST_DOT && metric != AMAR_NEAREST_COSINE) return AMAR_EINVAL;
    if (ldt < d) return AMAR_EINVAL;
    if (P > DIV_P || d < 4 || (d & 3) || d > DIV_MAX_D) return AMAR_EUNSUPPORTED;
    if ((ldt & 3) || !amar_aligned16(T)) return AMAR_EUNSUPPORTED;
    if (m >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    return AMAR_OK;
}

}  // namespace

extern "C" {

int amar_rerank_mmr_f32(const int32_t *pool_items, const float *pool_scores, int64_t m, int32_t P, const float *T, int64_t ldt,
                        int32_t n_rows, int32_t d, int32_t metric, float trade_off, int32_t k, int32_t *out_items,
                        float *out_scores, float *out_mmr, double *out_ild, amar_stream_t stream) {
    const int rc = diversify_check(m, P, T, ldt, n_rows, d, metric);
    if (rc == AMAR_EINVAL) return rc;
    if (k < 1 || !(trade_off >= 0.f && trade_off <= 1.f)) return AMAR_EINVAL;
    if (rc != AMAR_OK) return rc;
    if (k > P) return AMAR_EUNSUPPORTED;
    if (m == 0) return AMAR_OK;
    if (!pool_items || !pool_scores || !out_items || !out_scores) return AMAR_EINVAL;
    MmrArgs a{};
    a.pool_items = pool_items; a.pool_scores = pool_scores; a.P = P;
    a.T = T; a.ldt = ldt; a.n_rows = n_rows; a.d = d; a.cosine = metric == AMAR_NEAREST_COSINE ? 1 : 0;
    a.lambda = trade_off; a.k = k;
    a.out_items = out_items; a.out_scores = out_scores; a.out_mmr = out_mmr; a.out_ild = out_ild;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)m), block(64);
    switch ((P + 15) / 16) {
        case 1: hipLaunchKernelGGL(rerank_mmr_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(rerank_mmr_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(rerank_mmr_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(rerank_mmr_kernel<4>, grid, block, 0, st, a); break;
    }
    return amar_check_launch();
}

int amar_list_diversity_f64(const int32_t *lists, int64_t m, int32_t K, const float *T, int64_t ldt, int32_t n_rows, int32_t d,
                            int32_t metric, const int32_t *ks, int32_t nk, double *out_ild, int32_t *out_count,
                            amar_stream_t stream) {
    const int rc = diversify_check(m, K, T, ldt, n_rows, d, metric);
    if (rc == AMAR_EINVAL) return rc;
    if (!ks || nk < 1) return AMAR_EINVAL;
    if (rc != AMAR_OK) return rc;
    if (nk > AMAR_RANK_METRICS_MAX_KS) return AMAR_EUNSUPPORTED;
    for (int q = 0; q < nk; ++q)
        if (ks[q] < 1 || ks[q] > K) return AMAR_EINVAL;
    if (m == 0) return AMAR_OK;
    if (!lists || !out_ild || !out_count) return AMAR_EINVAL;
    DivArgs a{};
    a.lists = lists; a.K = K;
    a.T = T; a.ldt = ldt; a.n_rows = n_rows; a.d = d; a.cosine = metric == AMAR_NEAREST_COSINE ? 1 : 0;
    a.nk = nk;
    for (int q = 0; q < nk; ++q) a.ks[q] = ks[q];
    a.out_ild = out_ild; a.out_count = out_count;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)m), block(64);
    switch ((K + 15) / 16) {
        case 1: hipLaunchKernelGGL(list_diversity_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(list_diversity_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(list_diversity_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(list_diversity_kernel<4>, grid, block, 0, st, a); break;
    }
    return amar_check_launch();
}

}  // extern "C"

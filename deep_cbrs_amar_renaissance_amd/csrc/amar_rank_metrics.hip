// Full-ranking metrics of top-K lists on the device (gfx950): Precision / Recall / NDCG / HitRate @k, summed over users in float64.
//
// What utilities/metrics.py:full_ranking_metrics computes on the host in a Python loop over users, for lists that are already on the
// device (amar_recommend_f32 / amar_topk_segmented_f32 leave item ROWS best first, -1 padded).  Decomposition:
//   * stage 1, one wavefront per user and one lane per rank: lane r looks its item up in the user's sorted relevant segment (binary
//     search in global memory), the 64 outcomes are balloted into one mask, and lane q < nk derives cutoff ks[q] from the mask:
//     hits = popcount(mask below k), DCG = the discounts of the set bits added in rank order.  A workgroup (4 waves) owns a
//     contiguous range of users; wave w walks users w, w + 4, ... of the range and keeps its sums in registers, then the four waves'
//     sums are added in wave order and written as the workgroup's partial.
//   * stage 2, one wavefront: lane (q, metric) adds the partials in workgroup order.
// No atomics; the user -> (workgroup, wave, turn) assignment and both summation orders depend on m alone, so a call returns the same
// bits on every run.  All arithmetic is float64; the discount of rank r is 1 / log2(r + 1) evaluated here, the ideal DCG comes from
// the caller's cum_disc table.
#include "amar_common.h"

namespace {

constexpr int RM_WAVES = 4;
constexpr int RM_MAX_BLOCKS = AMAR_RANK_METRICS_MAX_BLOCKS;
constexpr int RM_MAX_KS = AMAR_RANK_METRICS_MAX_KS;
constexpr int RM_CELLS = AMAR_RANK_METRICS_CELLS;            // doubles per partial: nk x 4 sums, then (evaluated, skipped) as int64

struct RankMetricsArgs {
    const int32_t *lists; int64_t m; int K;
    const int32_t *users; const int32_t *rel_ptr, *rel_items; int n_users;
    int nk; int ks[RM_MAX_KS];
    double cum_disc[65];
    int users_per_block;
    double *partials;
};

__global__ __launch_bounds__(256) void rank_metrics_kernel(const RankMetricsArgs a) {
    __shared__ double disc[64];
    __shared__ double wave_sums[RM_WAVES][RM_MAX_KS][4];
    __shared__ long long wave_counts[RM_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) disc[lane] = 1.0 / log2((double)(lane + 2));
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.x * a.users_per_block;
    const int64_t j1 = j0 + a.users_per_block < a.m ? j0 + a.users_per_block : a.m;
    const int k = lane < a.nk ? a.ks[lane] : 1;
    const unsigned long long below = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
    double s_p = 0.0, s_r = 0.0, s_n = 0.0, s_h = 0.0;
    long long evaluated = 0, skipped = 0;
    for (int64_t j = j0 + wave; j < j1; j += RM_WAVES) {
        const int u = a.users ? a.users[j] : (int)j;
        int lo = 0, hi = 0;
        if (u >= 0 && u < a.n_users) { lo = a.rel_ptr[u]; hi = a.rel_ptr[u + 1]; }
        const int n_rel = hi - lo;
        if (n_rel <= 0) { ++skipped; continue; }               // (wave-uniform: u is the same in every lane)
        ++evaluated;
        const int item = lane < a.K ? a.lists[j * a.K + lane] : -1;
        bool hit = false;
        if (item >= 0) {
            int b = lo, e = hi;
            while (b < e) {
                const int mid = (b + e) >> 1;
                if (a.rel_items[mid] < item) b = mid + 1; else e = mid;
            }
            hit = b < hi && a.rel_items[b] == item;
        }
        const unsigned long long mask = __ballot(hit) & below;
        if (lane < a.nk) {
            const int hits = __popcll(mask);
            double dcg = 0.0;
            for (unsigned long long rest = mask; rest; rest &= rest - 1) dcg += disc[__ffsll((long long)rest) - 1];
            s_p += (double)hits / (double)k;
            s_r += (double)hits / (double)n_rel;
            s_n += dcg / a.cum_disc[n_rel < k ? n_rel : k];
            s_h += hits > 0 ? 1.0 : 0.0;
        }
    }
    if (lane < a.nk) {
        wave_sums[wave][lane][0] = s_p; wave_sums[wave][lane][1] = s_r;
        wave_sums[wave][lane][2] = s_n; wave_sums[wave][lane][3] = s_h;
    }
    if (lane == 0) { wave_counts[wave][0] = evaluated; wave_counts[wave][1] = skipped; }
    __syncthreads();
    double *out = a.partials + (int64_t)blockIdx.x * RM_CELLS;
    if (threadIdx.x < a.nk * 4) {
        const int q = threadIdx.x >> 2, c = threadIdx.x & 3;
        double s = wave_sums[0][q][c];
        for (int w = 1; w < RM_WAVES; ++w) s += wave_sums[w][q][c];
        out[threadIdx.x] = s;
    } else if (threadIdx.x >= 64 && threadIdx.x < 66) {
        const int c = threadIdx.x - 64;
        long long s = 0;
        for (int w = 0; w < RM_WAVES; ++w) s += wave_counts[w][c];
        reinterpret_cast<long long *>(out)[4 * RM_MAX_KS + c] = s;
    }
}

__global__ __launch_bounds__(64) void rank_metrics_reduce_kernel(const double *__restrict__ partials, int blocks, int nk,
                                                                 double *__restrict__ out_sums, long long *__restrict__ out_counts) {
    const int t = threadIdx.x;
    if (t < nk * 4) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += partials[(int64_t)b * RM_CELLS + t];
        out_sums[t] = s;
    } else if (t >= 4 * RM_MAX_KS && t < 4 * RM_MAX_KS + 2) {
        long long s = 0;
        for (int b = 0; b < blocks; ++b) s += reinterpret_cast<const long long *>(partials)[(int64_t)b * RM_CELLS + t];
        out_counts[t - 4 * RM_MAX_KS] = s;
    }
}

}  // namespace

extern "C" {

int amar_rank_metrics_f64(const int32_t *lists, int64_t m, int32_t K, const int32_t *users, const int32_t *rel_ptr,
                          const int32_t *rel_items, int32_t n_users, const int32_t *ks, int32_t nk, const double *cum_disc,
                          double *workspace, double *out_sums, int64_t *out_counts, amar_stream_t stream) {
    if (m < 0 || n_users < 0 || K < 1 || nk < 1 || !ks || !cum_disc || !rel_ptr || !rel_items || !workspace || !out_sums || !out_counts)
        return AMAR_EINVAL;
    if (m > 0 && !lists) return AMAR_EINVAL;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (K > 64 || nk > RM_MAX_KS) return AMAR_EUNSUPPORTED;
    RankMetricsArgs a{};
    for (int q = 0; q < nk; ++q) {
        if (ks[q] < 1 || ks[q] > K) return AMAR_EINVAL;
        a.ks[q] = ks[q];
    }
    for (int r = 0; r <= K; ++r) a.cum_disc[r] = cum_disc[r];
    int64_t blocks = (m + 63) / 64;                                  // about 16 users per wave, at most RM_MAX_BLOCKS workgroups
    if (blocks > RM_MAX_BLOCKS) blocks = RM_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    const int64_t per = (m + blocks - 1) / blocks;
    if (per >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    blocks = per > 0 ? (m + per - 1) / per : 1;                      // (no workgroup without a user, except for m == 0)
    a.lists = lists; a.m = m; a.K = K; a.users = users; a.rel_ptr = rel_ptr; a.rel_items = rel_items; a.n_users = n_users;
    a.nk = nk; a.users_per_block = (int)(per > 0 ? per : 1); a.partials = workspace;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(rank_metrics_kernel, dim3((unsigned)blocks), dim3(64 * RM_WAVES), 0, st, a);
    int e = amar_check_launch();
    if (e != AMAR_OK) return e;
    hipLaunchKernelGGL(rank_metrics_reduce_kernel, dim3(1), dim3(64), 0, st, workspace, (int)blocks, (int)nk, out_sums,
                       reinterpret_cast<long long *>(out_counts));
    return amar_check_launch();
}

}  // extern "C"

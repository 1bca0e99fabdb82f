// On-chip top-k selection shared by the fused rankers (amar_rank.hip: user -> item scores of the split head; amar_nearest.hip:
// dot / cosine neighbours): the order, the rank-counting merge of a candidate buffer into a sorted list, the lower bound of the
// exclusion walk, and the second launch that merges the per-slice lists of a sliced call.
#pragma once
#include "amar_common.h"

namespace {

constexpr int RANK_CAND = 64;                                                    // candidate buffer entries per user
constexpr int RANK_LIST = 64;                                                    // top-k list slots per user (k <= 64)
constexpr int RANK_EMPTY = 0x7fffffff;                                           // item of an empty slot (loses every tie)

__device__ __forceinline__ bool rank_better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// Merge n candidates (cs, ci) into the sorted list (ls, li) of k slots; one wave, every lane calls it.  Each entry's rank is the
// number of entries that beat it (items are distinct inside a user, empty slots never reach a written rank).
__device__ void rank_merge(float *ls, int *li, const float *cs, const int *ci, int n, int k, int lane) {
    const float s0 = lane < k ? ls[lane] : -INFINITY;
    const int i0 = lane < k ? li[lane] : RANK_EMPTY;
    const float s1 = lane < n ? cs[lane] : -INFINITY;
    const int i1 = lane < n ? ci[lane] : RANK_EMPTY;
    int r0 = 0, r1 = 0;
    for (int e = 0; e < k; ++e) {
        const float s = ls[e];
        const int i = li[e];
        r0 += rank_better(s, i, s0, i0);
        r1 += rank_better(s, i, s1, i1);
    }
    for (int e = 0; e < n; ++e) {
        const float s = cs[e];
        const int i = ci[e];
        r0 += rank_better(s, i, s0, i0);
        r1 += rank_better(s, i, s1, i1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < k) { ls[lane] = -INFINITY; li[lane] = RANK_EMPTY; }
    if (i0 != RANK_EMPTY && r0 < k) { ls[r0] = s0; li[r0] = i0; }
    if (i1 != RANK_EMPTY && r1 < k) { ls[r1] = s1; li[r1] = i1; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// First position in [lo, hi) of the sorted list whose value is >= x.
__device__ __forceinline__ int rank_lower_bound(const int32_t *v, int lo, int hi, int x) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Second launch with item slices: one wave per user merges its n_slices partial lists, slice by slice, into the final top-k.
__global__ __launch_bounds__(256) void recommend_merge_kernel(const int32_t *__restrict__ part_items, const float *__restrict__ part_scores,
                                                              int64_t m, int n_slices, int k, int32_t *__restrict__ out_items,
                                                              float *__restrict__ out_scores) {
    __shared__ float ls_all[4][RANK_LIST], cs_all[4][RANK_CAND];
    __shared__ int li_all[4][RANK_LIST], ci_all[4][RANK_CAND];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= m) return;
    float *ls = ls_all[wave], *cs = cs_all[wave];
    int *li = li_all[wave], *ci = ci_all[wave];
    ls[lane] = -INFINITY; li[lane] = RANK_EMPTY;
    for (int s = 0; s < n_slices; ++s) {
        const int64_t o = (j * n_slices + s) * k;
        cs[lane] = lane < k ? part_scores[o + lane] : -INFINITY;
        ci[lane] = lane < k ? part_items[o + lane] : RANK_EMPTY;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        rank_merge(ls, li, cs, ci, k, k, lane);
    }
    if (lane < k) {
        const int i = li[lane];
        out_items[j * k + lane] = i == RANK_EMPTY ? -1 : i;
        out_scores[j * k + lane] = i == RANK_EMPTY ? -INFINITY : ls[lane];
    }
}

}  // namespace

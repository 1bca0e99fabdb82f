// Full-catalogue top-k: fused score-and-select over every (user, item) pair of the split scoring head (gfx950).
//
// With the classifier's first Dense layer folded into the towers (models/basic.py:_split_plan), a pair's score is
//     score(u, i) = rest( in_act( Tu[u] + Ti[i] ) )          rest = Dense stack ending in Dense(1, sigmoid)
// This file evaluates that for a block of users against every item and keeps each user's k best on chip: nothing of size
// |U| x |I| is written.  Decomposition:
//   * grid (user blocks of 16, item slices); 4 waves per workgroup, each owning 4 users of the block.
//   * per item tile: the workgroup stages TI rows of Ti in LDS once; every wave then walks the tile for each of its users with
//     that user's Tu row in registers.  The first product's B fragment (pair on the MFMA column, features 16t + 4g + r on rows,
//     the layout of chain_kernel in amar_chain.hip) is formed in registers as in_act(Tu[u] + Ti[i]): no per-pair gathers.
//   * the rest stack runs on v_mfma_f32_16x16x4_f32 with chain_kernel's loop order, fragment blob and dot stage, so a score is
//     bit-identical to what amar_chain_f32's generic kernel returns for the same pair (the pair stage of predict() for heads
//     whose widths it takes).  These two steps are amar_rank_score.inc, the fragment every ranker's body includes.
//   * selection: the RankSlot of amar_rank_select.h, one per user (threshold, exclusion walk over the user's training items,
//     candidate buffer, rank-counting merge); the kernel hands it 16 PT scores at a time, lane group g holding pair tile g.
//   * with several item slices each workgroup leaves its slice's top-k in a workspace and a second launch (recommend_merge_kernel
//     below, also amar_nearest.hip's second launch) merges the slices of a user in slice order (the order is a strict total
//     order, so the result does not depend on the slicing).
// The result of a user depends on its own Tu row, Ti and the weights only: not on the other users of the block or the call.
// The kernel is rank_topk_kernel (amar_rank_score.h), the body the top-k rankers share, with the variant that changes
// nothing: RankPlain below.
// The pair route's ranker (amar_topk_segmented_f32: scores already in memory, one wave per user; amar_topk_segmented_after_f32: the
// same from a cursor) is at the end of the file.
#include "amar_rank_score.h"
#include <stdlib.h>

namespace {

typedef RankVariant<RankArgs> RankPlain;         // one user per selector row, every row of Ti, nothing to add

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

// The pair route's ranker: one wave per user over scores already in memory.  Round t picks the best pair that comes strictly
// after round t-1's winner in the order of rank_better; items are distinct within a user.  AFTER (amar_topk_segmented_after_f32):
// round 0 starts from the user's cursor (after_scores[u], after_items[u]) instead of (+inf, -1), the position before every pair.
template <bool AFTER>
__global__ __launch_bounds__(256) void topk_segmented_kernel(const int32_t *__restrict__ seg_ptr,
                                                              const int32_t *__restrict__ item_ids,
                                                              const float *__restrict__ scores, int n_users, int k,
                                                              const float *__restrict__ after_scores,
                                                              const int32_t *__restrict__ after_items,
                                                              int32_t *__restrict__ out_items,
                                                              float *__restrict__ out_scores) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    const int beg = seg_ptr[u], end = seg_ptr[u + 1];
    float prev_s = AFTER ? after_scores[u] : INFINITY;
    int prev_i = AFTER ? after_items[u] : -1;
    for (int t = 0; t < k; ++t) {
        float best_s = -INFINITY;
        int best_i = RANK_EMPTY;
        for (int p = beg + lane; p < end; p += 64) {
            const float s = scores[p];
            const int it = item_ids[p];
            if (rank_better(prev_s, prev_i, s, it) && rank_better(s, it, best_s, best_i)) { best_s = s; best_i = it; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(best_s, off, 64);
            const int oi = __shfl_xor(best_i, off, 64);
            if (rank_better(os, oi, best_s, best_i)) { best_s = os; best_i = oi; }
        }
        const bool found = best_i != RANK_EMPTY;
        if (lane == 0) {
            out_items[(int64_t)u * k + t] = found ? best_i : -1;
            out_scores[(int64_t)u * k + t] = found ? best_s : -INFINITY;
        }
        if (!found) {
            if (lane == 0)
                for (int r = t + 1; r < k; ++r) { out_items[(int64_t)u * k + r] = -1; out_scores[(int64_t)u * k + r] = -INFINITY; }
            break;
        }
        prev_s = best_s; prev_i = best_i;
    }
}

}  // namespace

int rank_merge_slices(const int32_t *part_rows, const float *part_scores, int64_t m, int slices, int k, int32_t *out_rows,
                      float *out_scores, hipStream_t stream) {
    hipLaunchKernelGGL(recommend_merge_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, part_rows, part_scores, m, slices, k,
                       out_rows, out_scores);
    return amar_check_launch();
}

extern "C" {

int32_t amar_recommend_slices(int64_t m, int32_t n_items, const int32_t *dims, int32_t n_layers, int32_t n_slices) {
    RankShape s;
    const int rc = rank_slices_tile(m, 0, n_items, dims, n_layers, s);
    return rc != AMAR_OK ? rc : rank_slices(m, n_items, s.tile_items, RANK_UB, n_slices);
}

int amar_recommend_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                       const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                       const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                       int32_t k, int32_t n_slices, int32_t *workspace_items, float *workspace_scores,
                       int32_t *out_items, float *out_scores, amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || m < 0 || n_users < 0 || n_items < 0 || k < 1) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    const RankHead head = {Tu, ldu, Ti, ldi, n_items, c1, wpack, dims, acts, n_layers, in_act, users, excl_ptr, excl_items};
    RankArgs a{};
    static RankForms<RankArgs> forms = AMAR_RANK_TOPK_FORMS(RankPlain);
    return rank_topk(forms, AMAR_RANK_RECOMMEND, head, a, m, n_items, amar_recommend_slices(m, n_items, dims, n_layers, n_slices), n_slices, k,
                     workspace_items, workspace_scores, out_items, out_scores, stream);
}

int amar_rank_route(int32_t kind, const int32_t *dims, int32_t n_layers, amar_rank_route_info *info) {
    if (!dims || !info) return AMAR_EINVAL;
    *info = amar_rank_route_info{};
    if (!rank_kind_known(kind)) return AMAR_EINVAL;
    if (n_layers < 2 || n_layers > RANK_MAX_LAYERS + 1) return AMAR_EUNSUPPORTED;
    const int32_t c1 = dims[0];                                          // the head's part of rank_check_tables, in its order
    if (c1 < 4 || (c1 & 3)) return AMAR_EINVAL;
    if (c1 > 128 || dims[n_layers] != 1) return AMAR_EUNSUPPORTED;
    RankArgs a{};
    RankShape sh;
    return rank_route(kind, dims, nullptr, n_layers, a, sh, *info);
}

int amar_topk_segmented_f32(const int32_t *seg_ptr, const int32_t *item_ids, const float *scores,
                            int32_t n_users, int32_t k, int32_t *out_items, float *out_scores,
                            amar_stream_t stream) {
    if (n_users < 0 || k < 1 || !seg_ptr) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (n_users == 0) return AMAR_OK;                                    // nothing to rank: the outputs may be empty (NULL)
    if (!item_ids || !scores || !out_items || !out_scores) return AMAR_EINVAL;
    hipLaunchKernelGGL(topk_segmented_kernel<false>, dim3((n_users + 3) / 4), dim3(256), 0,
                       static_cast<hipStream_t>(stream), seg_ptr, item_ids, scores, n_users, k, nullptr, nullptr, out_items, out_scores);
    return amar_check_launch();
}

int amar_topk_segmented_after_f32(const int32_t *seg_ptr, const int32_t *item_ids, const float *scores,
                                  int32_t n_users, int32_t k, const float *after_scores, const int32_t *after_items,
                                  int32_t *out_items, float *out_scores, amar_stream_t stream) {
    if (n_users < 0 || k < 1 || !seg_ptr) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (!after_scores != !after_items || (n_users > 0 && !after_scores)) return AMAR_EINVAL;
    if (n_users == 0) return AMAR_OK;                                    // nothing to rank: the outputs may be empty (NULL)
    if (!item_ids || !scores || !out_items || !out_scores) return AMAR_EINVAL;
    hipLaunchKernelGGL(topk_segmented_kernel<true>, dim3((n_users + 3) / 4), dim3(256), 0,
                       static_cast<hipStream_t>(stream), seg_ptr, item_ids, scores, n_users, k, after_scores, after_items, out_items,
                       out_scores);
    return amar_check_launch();
}

}  // extern "C"

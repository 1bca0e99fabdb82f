// Group recommendation: fused aggregate-and-select over the members' scores of the split scoring head (gfx950).
//
// "What should WE watch?": for a group of users and every item, the members' scores score(u, i) (amar_rank_score.inc: the value
// amar_recommend_f32 computes for the pair, bit for bit) are combined by a social-choice rule — the mean, the minimum (least
// misery) or the maximum (most pleasure), optionally with a veto on any member's score below a floor — and the group's k best
// items are kept on chip.  Nothing of size members x |I| or groups x |I| is written.  Decomposition:
//   * the kernel is rank_topk_kernel (amar_rank_score.h) with the variant RankGroup below.
//   * grid (group blocks of 16, item slices); 4 waves per workgroup, each owning 4 groups of the block, one RankSlot per group.
//   * per item tile: the workgroup stages the tile in LDS as every ranker does; a wave then walks the tile for each of its
//     groups.  For every step of 16 PT items it loops over the group's members in member order: the member's Tu row comes from
//     global memory (c1 floats, L2-resident), the score stage (amar_rank_score.inc) gives the lane its score, and the lane folds it into one aggregate
//     register and one running-minimum register.  After the last member the selector is offered the aggregate once, with
//     in_range && minimum >= min_score: selection runs once per item per group, not once per member.
//   * a group is walked by one wave from its first member to its last, so its result depends on its own members, Ti, the weights
//     and its exclusion segment only: not on the wave, the other groups, the grid or the slicing.  No atomics.
//   * item slices and their merge are those of amar_recommend_f32 (rank_merge_slices).  The automatic slice count looks at the
//     members as well as the groups (group_slices below).
#include "amar_rank_score.h"

namespace {

struct GroupArgs {
    RankArgs r;                                  // r.users = grp_users, r.m = n_groups, r.excl_ptr = the CSR over groups
    const int32_t *grp_ptr;
    int strategy;
    float min_score;
};

// A group per selector row: the exclusion CSR runs over groups, an empty group is skipped, and what the selector is offered is the
// fold of the members' scores in member order, admitted where no member scores below the floor.
struct RankGroup : RankVariant<GroupArgs> {
    static constexpr bool MEMBERS = true;
    static __device__ __forceinline__ int64_t excl_row(const RankArgs &, int64_t j) { return j; }
    static __device__ __forceinline__ void fold(const GroupArgs &ga, bool first, float z, float &acc, float &low) {
        const float both = ga.strategy == AMAR_GROUP_MEAN ? acc + z : (ga.strategy == AMAR_GROUP_MIN ? fminf(acc, z) : fmaxf(acc, z));
        acc = first ? z : both;
        low = first ? z : fminf(low, z);
    }
    static __device__ __forceinline__ float close(const GroupArgs &ga, float acc, float n) {
        return ga.strategy == AMAR_GROUP_MEAN ? __fdiv_rn(acc, n) : acc;
    }

    template <int MAXT>
    struct Sel {
        int mb, me;                              // the group's members: a.users[mb .. me)
        float n;
        __device__ __forceinline__ bool begin(const RankArgs &, const GroupArgs &ga, int64_t j, int64_t, int) {
            mb = ga.grp_ptr[j]; me = ga.grp_ptr[j + 1];
            n = (float)(me - mb);
            return mb < me;                      // an empty group: its list stays empty
        }
        __device__ __forceinline__ bool admit(const GroupArgs &ga, float, int, float low) const { return low >= ga.min_score; }
    };
};

// Item slices of a call.  Requested (n_slices > 0): clamped as rank_slices clamps.  Automatic: enough slices for about four
// resident workgroups per CU, as for amar_recommend_f32, but a workgroup's work is its members' walks over its tiles, not its
// groups': a slice keeps at least 64 member-tile walks per workgroup (what four tiles of sixteen users are there), so blocks of
// large groups are cut down to single tiles and blocks of small ones are not cut below what pays for staging the stack.
int32_t group_slices(int64_t n_groups, int64_t n_members, int64_t n_items, int tile_items, int32_t n_slices) {
    int64_t want = n_slices;
    if (want <= 0) {
        const int64_t tiles = (n_items + tile_items - 1) / tile_items;
        const int64_t blocks = (n_groups + RANK_UB - 1) / RANK_UB;
        want = blocks > 0 ? (1024 + blocks - 1) / blocks : 1;
        const int64_t per_block = blocks > 0 ? (n_members + blocks - 1) / blocks : 0;          // members a workgroup walks, on average
        const int64_t min_tiles = per_block >= 64 ? 1 : (per_block > 0 ? (64 + per_block - 1) / per_block : 4);
        const int64_t cap = tiles / min_tiles > 0 ? tiles / min_tiles : 1;
        want = want > cap ? cap : want;
        want = want > 16 ? 16 : want;
    }
    return rank_slices(n_groups, n_items, tile_items, RANK_UB, (int32_t)want);
}

}  // namespace

extern "C" {

int32_t amar_recommend_group_slices(int64_t n_groups, int64_t n_members, int32_t n_items, const int32_t *dims, int32_t n_layers,
                                    int32_t n_slices) {
    RankShape s;
    const int rc = rank_slices_tile(n_groups, n_members, n_items, dims, n_layers, s);
    return rc != AMAR_OK ? rc : group_slices(n_groups, n_members, n_items, s.tile_items, n_slices);
}

int amar_recommend_group_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *grp_ptr, const int32_t *grp_users, int64_t n_groups, int64_t n_members,
                             const int32_t *excl_ptr, const int32_t *excl_items, int32_t strategy, float min_score,
                             int32_t k, int32_t n_slices, int32_t *workspace_items, float *workspace_scores,
                             int32_t *out_items, float *out_scores, amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || n_groups < 0 || n_members < 0 || n_users < 0 || n_items < 0 || k < 1) return AMAR_EINVAL;
    if (strategy != AMAR_GROUP_MEAN && strategy != AMAR_GROUP_MIN && strategy != AMAR_GROUP_MAX) return AMAR_EINVAL;
    if (min_score != min_score) return AMAR_EINVAL;                    // NaN
    if ((n_groups > 0 && !grp_ptr) || (n_members > 0 && !grp_users)) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    const RankHead head = {Tu, ldu, Ti, ldi, n_items, c1, wpack, dims, acts, n_layers, in_act, grp_users, excl_ptr, excl_items};
    GroupArgs ga{};
    ga.grp_ptr = grp_ptr; ga.strategy = strategy; ga.min_score = min_score;
    static RankForms<GroupArgs> forms = AMAR_RANK_TOPK_FORMS(RankGroup);
    return rank_topk(forms, AMAR_RANK_GROUP, head, ga, n_groups, n_items,
                     amar_recommend_group_slices(n_groups, n_members, n_items, dims, n_layers, n_slices), n_slices, k,
                     workspace_items, workspace_scores, out_items, out_scores, stream);
}

}  // extern "C"

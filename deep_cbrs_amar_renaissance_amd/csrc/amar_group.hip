// Group recommendation: fused aggregate-and-select over the members' scores of the split scoring head (gfx950).
//
// "What should WE watch?": for a group of users and every item, the members' scores score(u, i) (amar_rank_score.inc: the value
// amar_recommend_f32 computes for the pair, bit for bit) are combined by a social-choice rule — the mean, the minimum (least
// misery) or the maximum (most pleasure), optionally with a veto on any member's score below a floor — and the group's k best
// items are kept on chip.  Nothing of size members x |I| or groups x |I| is written.  Decomposition:
//   * grid (group blocks of 16, item slices); 4 waves per workgroup, each owning 4 groups of the block, one RankSlot per group.
//   * per item tile: the workgroup stages the tile in LDS as recommend_kernel does; a wave then walks the tile for each of its
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

template <int MAXT, int PT>
__global__ __launch_bounds__(256) void recommend_group_kernel(const GroupArgs ga) {
    const RankArgs &a = ga.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *tile = lds + ((a.wpack_floats + 3) & ~3);
    float *select = tile + a.tile_items * a.tile_stride;         // RANK_UB selector slots (amar_rank_select.h)

    rank_stage_weights(a, w_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * RANK_UB;
    const int slice = blockIdx.y;
    const int s0 = slice * a.slice_items, s1 = min(a.n_items, s0 + a.slice_items);
    const int KT0 = a.kt[0];
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        int eb = 0, ee = 0;                                      // the group's excluded items
        if (lane == 0 && j < a.m && a.excl_ptr) { eb = a.excl_ptr[j]; ee = a.excl_ptr[j + 1]; }
        RankSlot<RANK_UB>(select, slot).init(lane, a.excl_items, eb, ee, s0);
    }

    for (int t0 = s0; t0 < s1; t0 += a.tile_items) {
        const int rows = min(a.tile_items, s1 - t0);
        __syncthreads();                                         // the previous tile is no longer read
        rank_stage_tile(a, tile, t0, rows);
        __syncthreads();
        for (int uw = 0; uw < RANK_UPW; ++uw) {
            const int slot = wave * RANK_UPW + uw;
            const int64_t j = j0 + slot;
            if (j >= a.m) break;
            const int mb = ga.grp_ptr[j], me = ga.grp_ptr[j + 1];
            if (mb >= me) continue;                              // an empty group: its list stays empty
            const float n = (float)(me - mb);
            RankSlot<RANK_UB> top(select, slot);
            top.load();
            const int ee = a.excl_ptr ? a.excl_ptr[j + 1] : 0;

            for (int grp = 0; grp < rows; grp += 16 * PT) {
                float acc = 0.f, low = 0.f;                      // the aggregate so far, the smallest member score so far
                for (int t = mb; t < me; ++t) {
                    f32x4 tu[MAXT];
                    rank_load_user<MAXT>(a, a.users[t], g, tu);
#include "amar_rank_score.inc"
                    const float both = ga.strategy == AMAR_GROUP_MEAN ? acc + z : (ga.strategy == AMAR_GROUP_MIN ? fminf(acc, z) : fmaxf(acc, z));
                    acc = t == mb ? z : both;
                    low = t == mb ? z : fminf(low, z);
                }
                if (ga.strategy == AMAR_GROUP_MEAN) acc = __fdiv_rn(acc, n);
                const int item = t0 + grp + 16 * g + col;
                top.offer(acc, item, g < PT && grp + 16 * g + col < rows && low >= ga.min_score, a.excl_items, ee, a.out.k, lane);
            }
            top.advance(a.excl_items, ee, t0 + rows);
            top.store(lane);
        }
    }
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        if (j >= a.m) break;
        RankSlot<RANK_UB>(select, slot).finish(j, slice, a.out, lane);
    }
}

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
    static RankForms<GroupArgs> forms = AMAR_RANK_FORMS(recommend_group_kernel);
    return rank_topk(forms, AMAR_RANK_GROUP, head, ga, n_groups, n_items,
                     amar_recommend_group_slices(n_groups, n_members, n_items, dims, n_layers, n_slices), n_slices, k,
                     workspace_items, workspace_scores, out_items, out_scores, stream);
}

}  // extern "C"

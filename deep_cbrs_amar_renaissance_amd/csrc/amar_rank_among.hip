// Top-k among a candidate slice of the catalogue: fused score-and-select over (user, candidate) pairs of the split head (gfx950).
//
// "The best k among THESE items": amar_recommend_f32 with the tile loop running over the positions of a candidate list instead of
// the rows 0..n_items-1 of Ti.  cand_items holds item rows, strictly ascending, each in [0, n_items); a launch scores
// m x n_cand pairs, not m x n_items.  Decomposition:
//   * the kernel is rank_topk_kernel (amar_rank_score.h) with the variant RankAmong below, which says LISTED and nothing else.
//   * grid (user blocks of 16, slices of candidate POSITIONS); 4 waves per workgroup, each owning 4 users, one RankSlot per user:
//     amar_recommend_f32's geometry with n_cand in the place of n_items (rank_slices / rank_slice_rows / amar_recommend_slices).
//   * per tile: the workgroup gathers the rows Ti[cand_items[t0 + r]] into the LDS tile (rank_stage_tile<true>: the float4 pieces
//     and zero fill of every ranker's staging) and leaves the tile's item rows in tile_rows, an int array of tile_items entries
//     behind the selectors (RANK_EMPTY past the tile's last candidate; such an entry is never used as a row of Ti).  The array
//     sits after everything the other variants place, so the stack, the tile with its +4 float stagger and the selectors keep
//     their offsets and alignment; a step reads 16 PT consecutive words of it, one bank each.
//   * the score stage is amar_rank_score.inc: a pair has the bits amar_recommend_f32 gives it, wherever its row is staged.
//   * selection: RankSlot, unchanged.  It is offered item ROWS (from tile_rows), so lists, ties and the exclusion walk stay in
//     item-row space; the walk needs ascending rows only, which the candidate list gives it: init() starts the exclusion pointer
//     at the slice's first candidate row, advance() moves it to the row of the next candidate position (INT_MAX at the end).
//   * sliced calls finish with rank_merge_slices, as amar_recommend_f32's.
// A user's result depends on its own Tu row, the candidates' Ti rows, the weights and its exclusion row only.
#include "amar_rank_score.h"

namespace {

struct AmongArgs {
    RankArgs r;                                  // r.n_items = rows of Ti; the tile loop runs over candidate positions
    const int32_t *cand_items;
    int n_cand;
};

struct RankAmong : RankVariant<AmongArgs> {
    static constexpr bool LISTED = true;         // the tile loop runs over cand_items[0 .. n_cand)
};

}  // namespace

extern "C" {

int amar_recommend_among_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                             const int32_t *cand_items, int32_t n_cand, int32_t k, int32_t n_slices,
                             int32_t *workspace_items, float *workspace_scores, int32_t *out_items, float *out_scores,
                             amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || m < 0 || n_users < 0 || n_items < 0 || k < 1) return AMAR_EINVAL;
    if (n_cand < 0 || n_cand > n_items || (n_cand > 0 && !cand_items)) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    const RankHead head = {Tu, ldu, Ti, ldi, n_items, c1, wpack, dims, acts, n_layers, in_act, users, excl_ptr, excl_items};
    AmongArgs aa{};
    aa.cand_items = cand_items; aa.n_cand = n_cand;
    static RankForms<AmongArgs> forms = AMAR_RANK_TOPK_FORMS(RankAmong);
    return rank_topk(forms, AMAR_RANK_AMONG, head, aa, m, n_cand, amar_recommend_slices(m, n_cand, dims, n_layers, n_slices), n_slices, k,
                     workspace_items, workspace_scores, out_items, out_scores, stream);
}

}  // extern "C"

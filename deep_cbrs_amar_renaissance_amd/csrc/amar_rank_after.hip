// Top-k AFTER a position of the user's ranking: fused score-and-select over every (user, item) pair of the split head (gfx950).
//
// "The next page": amar_recommend_f32 with a cursor per selector row.  The order of the rankers (rank_better: score descending, item
// row ascending) is a strict total order, so a position in a user's ranking is a pair (score, item row) and "strictly after it" is
// one comparison per scored pair.  Decomposition:
//   * grid, waves, item tiles, the staged stack and the selectors are amar_recommend_f32's: the LDS sum, the slicing and the
//     capacity rule are AMAR_RANK_RECOMMEND's, amar_recommend_slices counts the slices, rank_merge_slices merges them.
//   * the kernel below is still its own copy of the walk that rank_topk_kernel (amar_rank_score.h) holds for the other three
//     top-k rankers.  As a variant of that body (a Sel with the cursor, admit = rank_better(cursor, pair)) it returned the same
//     bits but measured 0.3 % slower than this kernel at ml1m(s=8), just past the run-to-run band of two builds of one source
//     (DESIGN.md, 8a10), so it stays until that is gone.  A fix to the walk has to be made here too.
//   * the cursor of selector row j, (after_scores[j], after_items[j]), is indexed by the ROW of the call, not by users[j]: the same
//     user may stand twice in a call with two cursors.  It lives in two lane-uniform registers, loaded where the user's exclusion end
//     is loaded; rank_better(cursor, pair) is ANDed into the in_range predicate of RankSlot::offer.
//   * the score stage is amar_rank_score.inc: a pair has the bits amar_recommend_f32 gives it.
//   * selection: RankSlot, unchanged.  A pair the cursor keeps out never reaches the threshold test, the exclusion walk or the
//     candidate buffer, so the list is the user's ranking with everything up to the cursor struck out.
// (+inf, -1) admits every pair (amar_recommend_f32's output, bit for bit); (-inf, -1), the padding of an exhausted list, and a NaN
// score admit nothing.  A user's result depends on its own Tu row, Ti, the weights, its exclusion row and its cursor only.
#include "amar_rank_score.h"

namespace {

struct AfterArgs {
    RankArgs r;
    const float *after_scores;                   // [m]: the cursor of selector row j
    const int32_t *after_items;
};

template <int MAXT, int PT>
__global__ __launch_bounds__(256) void recommend_after_kernel(const AfterArgs aa) {
    const RankArgs &a = aa.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *tile = lds + ((a.wpack_floats + 3) & ~3);
    float *select = tile + a.tile_items * a.tile_stride;         // RANK_UB selector slots (amar_rank_select.h)

    rank_stage_weights(a, w_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * RANK_UB;
    const int slice = blockIdx.y;
    const int s0 = slice * a.slice_items, s1 = min(a.n_items, s0 + a.slice_items);
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        int eb = 0, ee = 0;                                      // the user's training items
        if (lane == 0 && j < a.m && a.excl_ptr) {
            const int u = a.users ? a.users[j] : (int)j;
            eb = a.excl_ptr[u]; ee = a.excl_ptr[u + 1];
        }
        RankSlot<RANK_UB>(select, slot).init(lane, a.excl_items, eb, ee, s0);
    }
    const int KT0 = a.kt[0];

    for (int t0 = s0; t0 < s1; t0 += a.tile_items) {
        const int rows = min(a.tile_items, s1 - t0);
        __syncthreads();                                         // the previous tile is no longer read
        rank_stage_tile(a, tile, t0, rows);
        __syncthreads();
        for (int uw = 0; uw < RANK_UPW; ++uw) {
            const int slot = wave * RANK_UPW + uw;
            const int64_t j = j0 + slot;
            if (j >= a.m) break;
            const int u = a.users ? a.users[j] : (int)j;
            f32x4 tu[MAXT];
            rank_load_user<MAXT>(a, u, g, tu);
            RankSlot<RANK_UB> top(select, slot);
            top.load();
            const int ee = a.excl_ptr ? a.excl_ptr[u + 1] : 0;
            const float after_s = aa.after_scores[j];            // the cursor: lane-uniform, in registers
            const int after_i = aa.after_items[j];

            for (int grp = 0; grp < rows; grp += 16 * PT) {
#include "amar_rank_score.inc"
                const int item = t0 + grp + 16 * g + col;
                const bool in_range = g < PT && grp + 16 * g + col < rows;
                top.offer(z, item, in_range && rank_better(after_s, after_i, z, item), a.excl_items, ee, a.out.k, lane);
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

}  // namespace

extern "C" {

int amar_recommend_after_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                             const float *after_scores, const int32_t *after_items, int32_t k, int32_t n_slices,
                             int32_t *workspace_items, float *workspace_scores, int32_t *out_items, float *out_scores,
                             amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || m < 0 || n_users < 0 || n_items < 0 || k < 1) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    if (!after_scores != !after_items || (m > 0 && !after_scores)) return AMAR_EINVAL;
    const RankHead head = {Tu, ldu, Ti, ldi, n_items, c1, wpack, dims, acts, n_layers, in_act, users, excl_ptr, excl_items};
    AfterArgs aa{};
    aa.after_scores = after_scores; aa.after_items = after_items;
    static RankForms<AfterArgs> forms = AMAR_RANK_FORMS(recommend_after_kernel);
    return rank_topk(forms, AMAR_RANK_RECOMMEND, head, aa, m, n_items, amar_recommend_slices(m, n_items, dims, n_layers, n_slices), n_slices, k,
                     workspace_items, workspace_scores, out_items, out_scores, stream);
}

}  // extern "C"

// Top-k among a candidate slice of the catalogue: fused score-and-select over (user, candidate) pairs of the split head (gfx950).
//
// "The best k among THESE items": amar_recommend_f32 with the tile loop running over the positions of a candidate list instead of
// the rows 0..n_items-1 of Ti.  cand_items holds item rows, strictly ascending, each in [0, n_items); a launch scores
// m x n_cand pairs, not m x n_items.  Decomposition:
//   * grid (user blocks of 16, slices of candidate POSITIONS); 4 waves per workgroup, each owning 4 users, one RankSlot per user:
//     recommend_kernel's geometry with n_cand in the place of n_items (rank_slices / rank_slice_rows / amar_recommend_slices).
//   * per tile: the workgroup gathers the rows Ti[cand_items[t0 + r]] into the LDS tile (the float4 pieces and zero fill of
//     recommend_kernel's staging) and leaves the tile's item rows in tile_rows, an int array of tile_items entries behind the
//     selectors (RANK_EMPTY past the tile's last candidate; such an entry is never used as a row of Ti).  The array sits after
//     everything recommend_kernel places, so the stack, the tile with its +4 float stagger and the selectors keep their offsets
//     and alignment; a step reads 16 PT consecutive words of it, one bank each.
//   * the score stage is amar_rank_score.inc: a pair has the bits amar_recommend_f32 gives it, wherever its row is staged.
//   * selection: RankSlot, unchanged.  It is offered item ROWS (from tile_rows), so lists, ties and the exclusion walk stay in
//     item-row space; the walk needs ascending rows only, which the candidate list gives it: init() starts the exclusion pointer
//     at the slice's first candidate row, advance() moves it to the row of the next candidate position (INT_MAX at the end).
//   * sliced calls finish with rank_merge_slices, as amar_recommend_f32's.
// A user's result depends on its own Tu row, the candidates' Ti rows, the weights and its exclusion row only.
#include "amar_rank_score.h"
#include <limits.h>

namespace {

struct AmongArgs {
    RankArgs r;                                  // r.n_items = rows of Ti; the tile loop runs over candidate positions
    const int32_t *cand_items;
    int n_cand;
};

template <int MAXT, int PT>
__global__ __launch_bounds__(256) void recommend_among_kernel(const AmongArgs aa) {
    const RankArgs &a = aa.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *tile = lds + ((a.wpack_floats + 3) & ~3);
    float *select = tile + a.tile_items * a.tile_stride;         // RANK_UB selector slots (amar_rank_select.h)
    int *tile_rows = reinterpret_cast<int *>(select + rank_select_state_floats(RANK_UB));      // item row of every tile row

    rank_stage_weights(a, w_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * RANK_UB;
    const int slice = blockIdx.y;
    const int s0 = slice * a.slice_items, s1 = min(aa.n_cand, s0 + a.slice_items);           // candidate positions
    const int first_row = s0 < aa.n_cand ? aa.cand_items[s0] : 0;
    const int KT0 = a.kt[0];
    const int f4_per_row = 4 * KT0;                              // float4s of a staged row (16 KT0 features, zero past c1)
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        int eb = 0, ee = 0;                                      // the user's training items
        if (lane == 0 && j < a.m && a.excl_ptr) {
            const int u = a.users ? a.users[j] : (int)j;
            eb = a.excl_ptr[u]; ee = a.excl_ptr[u + 1];
        }
        RankSlot<RANK_UB>(select, slot).init(lane, a.excl_items, eb, ee, first_row);
    }

    for (int t0 = s0; t0 < s1; t0 += a.tile_items) {
        const int rows = min(a.tile_items, s1 - t0);
        const int next_row = t0 + rows < aa.n_cand ? aa.cand_items[t0 + rows] : INT_MAX;
        __syncthreads();                                         // the previous tile is no longer read
        for (int idx = threadIdx.x; idx < a.tile_items * f4_per_row; idx += blockDim.x) {
            const int r = idx / f4_per_row, f = 4 * (idx - r * f4_per_row);
            const int row = r < rows ? aa.cand_items[t0 + r] : RANK_EMPTY;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && f < a.c1) v = *reinterpret_cast<const float4 *>(a.Ti + (int64_t)row * a.ldi + f);
            *reinterpret_cast<float4 *>(&tile[r * a.tile_stride + f]) = v;
            if (f == 0) tile_rows[r] = row;
        }
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

            for (int grp = 0; grp < rows; grp += 16 * PT) {
#include "amar_rank_score.inc"
                const bool in_range = g < PT && grp + 16 * g + col < rows;
                const int item = in_range ? tile_rows[grp + 16 * g + col] : RANK_EMPTY;
                top.offer(z, item, in_range, a.excl_items, ee, a.out.k, lane);
            }
            top.advance(a.excl_items, ee, next_row);
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
    static RankForms<AmongArgs> forms = AMAR_RANK_FORMS(recommend_among_kernel);
    return rank_topk(forms, AMAR_RANK_AMONG, head, aa, m, n_cand, amar_recommend_slices(m, n_cand, dims, n_layers, n_slices), n_slices, k,
                     workspace_items, workspace_scores, out_items, out_scores, stream);
}

}  // extern "C"

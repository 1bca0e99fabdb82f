// Top-k over per-user candidate lists: fused score-and-select over the (user, candidate) pairs of a CSR of lists, split head (gfx950).
//
// "The best k of THIS user's candidates": where amar_recommend_among_f32 takes one candidate list for every user, every listed row
// j has its own, cand_items[cand_ptr[j] .. cand_ptr[j + 1]) (item rows, strictly ascending, each in [0, n_items): the contract of
// amar_recommend_among_f32's list, per row; nothing on the device checks it).  A launch scores sum_j |C_j| pairs.  It puts together
// what amar_rank_of.hip does with an entry's targets (a wave gathers its own rows into a tile-shaped buffer of its own and scores
// them with the shared fragment: rank_gather, amar_rank_score.inc) and what rank_topk_kernel does with a score (RankSlot).
// Decomposition:
//   * grid ceil(m / 4) workgroups of 256 threads; a wave owns ONE listed row and one RankSlot (RANK_WAVES slots, not RANK_UB).
//   * LDS: the packed stack, staged once per workgroup and followed by the one __syncthreads() of the kernel; RANK_WAVES gather
//     buffers of rank_of_gather_floats(sh) floats (16 PT rows of tile_stride, the +4 float stagger of every ranker's tile);
//     RANK_WAVES selectors.  No shared item tile: rank_lists_lds_bytes is smaller than rank_lds_bytes by most of a tile, so heads
//     that amar_recommend_f32 refuses for capacity fit here.
//   * per step a wave gathers the Ti rows of its next 16 PT candidates into its buffer (float4 pieces, zero past c1 and past the
//     list's end), includes the score stage with tile = the buffer and grp = 0, and offers z with the item row read from
//     cand_items.  The selector works in item-row space: init() starts the exclusion walk at the row's first candidate, advance()
//     moves it to the first candidate of the next step (INT_MAX after the last).
//   * NO BARRIER IN THE LOOP.  The four waves of a workgroup have different trip counts (one list may be empty, its neighbour the
//     whole catalogue), so after the staging barrier nothing waits for another wave: the loop synchronises at wave scope only
//     (rank_wave_sync), there is no __syncthreads() behind the first one and no return in front of it (a wave past m skips its
//     work, it does not leave early).
//   * no slices, no workspace, no merge launch: a wave walks its whole list.  A call whose lists are all the same long set wants
//     amar_recommend_among_f32, which stages each candidate once per 16 users and slices the list over workgroups.
// A pair has the bits amar_recommend_f32 gives it (the same fragment, the same rank_load_user); ties and order are rank_better's.
// A row's result depends on its own Tu row, its candidates' Ti rows, the weights and its exclusion row only.
#include "amar_rank_score.h"

namespace {

struct ListsArgs {
    RankArgs r;                                  // r.n_items = rows of Ti; tile_items / slice_items are not used
    const int32_t *cand_ptr, *cand_items;
    int gather_floats;                           // floats of a wave's gather buffer: 16 PT rows of tile_stride
};

template <int MAXT, int PT>
__global__ __launch_bounds__(256) void rank_lists_kernel(const ListsArgs la) {
    const RankArgs &a = la.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *gather = lds + ((a.wpack_floats + 3) & ~3);           // RANK_WAVES buffers of 16 PT rows
    float *select = gather + RANK_WAVES * la.gather_floats;      // RANK_WAVES selector slots (amar_rank_select.h)

    rank_stage_weights(a, w_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j = (int64_t)blockIdx.x * RANK_WAVES + wave;
    const int KT0 = a.kt[0];
    float *tile = gather + wave * la.gather_floats;
    __syncthreads();                                             // the stack is staged: the only workgroup barrier
    if (j < a.m) {                                               // wave-uniform; from here on the wave waits for itself alone
        const int u = a.users ? a.users[j] : (int)j;
        const int cb = la.cand_ptr[j], ce = la.cand_ptr[j + 1];
        const int eb = a.excl_ptr ? a.excl_ptr[u] : 0, ee = a.excl_ptr ? a.excl_ptr[u + 1] : 0;
        RankSlot<RANK_WAVES> top(select, wave);
        top.init(lane, a.excl_items, eb, ee, cb < ce ? la.cand_items[cb] : 0);
        rank_wave_sync();
        top.load();
        f32x4 tu[MAXT];
        rank_load_user<MAXT>(a, u, g, tu);
        for (int t0 = cb; t0 < ce; t0 += 16 * PT) {
            const int rows = min(16 * PT, ce - t0);
            rank_gather<PT>(a, tile, la.cand_items + t0, rows, lane);
            rank_wave_sync();
            const int grp = 0;
#include "amar_rank_score.inc"
            const int r = 16 * g + col;
            const bool in_range = g < PT && r < rows;
            const int item = in_range ? la.cand_items[t0 + r] : RANK_EMPTY;
            top.offer(z, item, in_range, a.excl_items, ee, a.out.k, lane);
            top.advance(a.excl_items, ee, t0 + rows < ce ? la.cand_items[t0 + rows] : INT_MAX);
            rank_wave_sync();                                    // the buffer is no longer read
        }
        top.store(lane);
        top.finish(j, 0, a.out, lane);
    }
}

}  // namespace

extern "C" {

int amar_recommend_lists_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                             const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                             const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                             const int32_t *cand_ptr, const int32_t *cand_items, int32_t k,
                             int32_t *out_items, float *out_scores, amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || m < 0 || n_users < 0 || n_items < 0 || k < 1) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    if ((m > 0 && !cand_ptr) || (cand_ptr && !cand_items)) return AMAR_EINVAL;
    const RankHead head = {Tu, ldu, Ti, ldi, n_items, c1, wpack, dims, acts, n_layers, in_act, users, excl_ptr, excl_items};
    ListsArgs la{};
    RankArgs &a = la.r;
    RankShape sh;
    amar_rank_route_info route;
    const int rc = rank_prepare(AMAR_RANK_LISTS, head, m, a, sh, route);
    if (rc != AMAR_OK) return rc;
    if (m == 0) return AMAR_OK;
    if (!out_items || !out_scores) return AMAR_EINVAL;
    la.cand_ptr = cand_ptr; la.cand_items = cand_items; la.gather_floats = rank_of_gather_floats(sh);
    a.out.k = k; a.out.n_slices = 1; a.out.rows = out_items; a.out.scores = out_scores;
    if (!route.fits) return AMAR_EUNSUPPORTED;
    const int64_t blocks = (m + RANK_WAVES - 1) / RANK_WAVES;
    if (blocks >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    static RankForms<ListsArgs> forms = AMAR_RANK_FORMS(rank_lists_kernel);
    return rank_launch_form(forms, route, dim3((unsigned)blocks), static_cast<hipStream_t>(stream), la);
}

}  // extern "C"

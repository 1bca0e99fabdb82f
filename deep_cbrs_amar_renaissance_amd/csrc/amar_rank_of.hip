// Where does THIS item stand?  Exact full-catalogue positions of chosen (user, item) pairs of the split scoring head, by counting
// (gfx950), and the cut-off-free metrics (AUC, reciprocal rank, average precision) that follow from the counts.
//
// The third consumer of the score stage (amar_rank_score.inc: the value amar_recommend_f32 computes for the pair, bit for bit): where
// rank_topk_kernel (amar_rank_score.h) selects, this file counts.  For entry j (a user u and up to AMAR_RANK_OF_MAX_TARGETS target items)
// and every target t it returns s_t = score(u, t) and, over the candidates C(u) = {items} \ excl(u) other than t, how many score
// higher, how many score the same with a smaller item row, and how many the same with a larger one.  Nothing of size m x |I| is
// written.  Decomposition:
//   * grid (entry blocks of 16, item slices); 4 waves per workgroup, each owning 4 entries of the block: rank_topk_kernel's grid.
//   * prologue, per entry: the targets' Ti rows are gathered into the wave's own tile-shaped LDS buffer (16 PT rows) and scored by
//     the same fragment; the (score, item) pairs are sorted ascending by rank counting, one lane per target.  Then the user's
//     excluded items that fall into the slice are gathered and scored the same way and counted with weight -1.
//   * per item tile: the workgroup stages the tile as rank_topk_kernel does; a wave walks it for each of its entries.  Per pair: a
//     binary search of z among the entry's sorted target scores (p = targets scoring below z) and one integer LDS add into cnt[p];
//     a lane whose z equals a target's score also walks that run of equal targets and adds to their before / after counters by
//     item row.  cnt[p] of an equal pair lands on the first target of its run, so for the target at sorted position q
//         greater = sum of cnt[p] over p > q
//     holds for pairs between two target scores and for pairs equal to a higher target alike.  The walk counts every item; the
//     prologue has already taken the excluded ones out (a pair's bits do not depend on where it is staged, so this is exact).
//   * epilogue: lane q adds its suffix sum and its two tie counters to the outputs with integer atomics: the slices add up.
// An entry is walked by one wave and all its counters are integers: its result depends on its own user row, Ti, the weights, its
// exclusion row and its targets only, not on the other entries, the grid or the slicing, and is the same on every run.
// A user whose scores saturate (many pairs equal to a target) pays the length of the equal run per such pair.
#include "amar_rank_score.h"

namespace {

constexpr int RO_T = AMAR_RANK_OF_MAX_TARGETS;
constexpr int RO_WORDS = RANK_OF_WORDS;         // per entry: ts, ti, tp [T], cnt [T + 1, padded to T + 2], bf, af [T] (6 T + 2)
static_assert(RO_T == AMAR_WAVE, "one lane per target");

struct RankOfArgs {
    RankArgs r;                                  // r.out is not used
    const int32_t *tgt_ptr, *tgt_items;
    int gather_floats;                           // floats of a wave's gather buffer: 16 PT rows of tile_stride
    float *out_scores;
    int32_t *out_greater, *out_before, *out_after;
};

// The score stage on the 16 PT rows that start at row `grp` of `tile`: the score of the user against row grp + 16 g + col.
template <int MAXT, int PT>
__device__ __forceinline__ float ro_score(const RankArgs &a, const float *w_lds, const float *tile, int grp, const f32x4 (&tu)[MAXT],
                                          int lane, int g, int col, int KT0) {
#include "amar_rank_score.inc"
    return z;
}

// One entry's sorted targets and counters in LDS; a wave owns its entries.
struct RankOfSlot {
    float *ts;                                   // target scores, ascending (ties by item row ascending)
    int *ti, *tp;                                // their item rows, their positions in the entry's segment of tgt_items
    int *cnt, *bf, *af;                          // pairs by targets below them; per target: equal pairs before / after it

    __device__ __forceinline__ RankOfSlot(int *base, int slot) {
        int *p = base + slot * RO_WORDS;
        ts = reinterpret_cast<float *>(p); ti = p + RO_T; tp = p + 2 * RO_T;
        cnt = p + 3 * RO_T; bf = cnt + RO_T + 2; af = bf + RO_T;
    }

    // One pair (score z, item row `item`) enters (sign = 1) or leaves (sign = -1) the counts of the entry's n targets.
    __device__ __forceinline__ void count(float z, int item, int n, int sign) const {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ts[mid] < z) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&cnt[lo], sign);
        for (int r = lo; r < n && ts[r] == z; ++r) {                 // rare: the run of targets that score exactly z
            const int t = ti[r];
            if (item < t) atomicAdd(&bf[r], sign);
            else if (item > t) atomicAdd(&af[r], sign);
        }
    }
};

template <int MAXT, int PT>
__global__ __launch_bounds__(256) void rank_of_kernel(const RankOfArgs ra) {
    const RankArgs &a = ra.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *tile = lds + ((a.wpack_floats + 3) & ~3);
    float *gather = tile + a.tile_items * a.tile_stride;         // RANK_WAVES buffers of 16 PT rows
    int *state = reinterpret_cast<int *>(gather + RANK_WAVES * ra.gather_floats);

    rank_stage_weights(a, w_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * RANK_UB;
    const int slice = blockIdx.y;
    const int s0 = slice * a.slice_items, s1 = min(a.n_items, s0 + a.slice_items);
    const int KT0 = a.kt[0];
    float *buf = gather + wave * ra.gather_floats;
    __syncthreads();                                             // the stack is staged

    // prologue: score and sort every entry's targets, take the slice's excluded items out of the counts
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        if (j >= a.m) break;
        const int tb = ra.tgt_ptr[j], n = min(ra.tgt_ptr[j + 1] - tb, RO_T);
        if (n <= 0) continue;
        const int u = a.users ? a.users[j] : (int)j;
        f32x4 tu[MAXT];
        rank_load_user<MAXT>(a, u, g, tu);
        RankOfSlot st(state, slot);
        for (int b = 0; b < n; b += 16 * PT) {
            rank_gather<PT>(a, buf, ra.tgt_items + tb + b, min(16 * PT, n - b), lane);
            rank_wave_sync();
            const float z = ro_score<MAXT, PT>(a, w_lds, buf, 0, tu, lane, g, col, KT0);
            const int e = b + 16 * g + col;
            if (g < PT && e < n) { st.bf[e] = __float_as_int(z); st.af[e] = ra.tgt_items[tb + e]; }      // in segment order, for the sort
            rank_wave_sync();
        }
        const float s = lane < n ? __int_as_float(st.bf[lane]) : 0.f;
        const int it = lane < n ? st.af[lane] : 0;
        int rank = 0;
        for (int e = 0; e < n; ++e) {
            const float se = __int_as_float(st.bf[e]);
            rank += (se < s || (se == s && st.af[e] < it)) ? 1 : 0;
        }
        rank_wave_sync();
        if (lane < n) { st.ts[rank] = s; st.ti[rank] = it; st.tp[rank] = lane; }
        st.bf[lane] = 0; st.af[lane] = 0; st.cnt[lane] = 0;
        if (lane < 2) st.cnt[RO_T + lane] = 0;
        if (slice == 0 && lane < n) ra.out_scores[tb + lane] = s;
        rank_wave_sync();
        if (a.excl_ptr) {
            const int ee = a.excl_ptr[u + 1];
            const int xb = rank_lower_bound(a.excl_items, a.excl_ptr[u], ee, s0);
            const int xe = rank_lower_bound(a.excl_items, xb, ee, s1);
            for (int b = xb; b < xe; b += 16 * PT) {
                const int rows = min(16 * PT, xe - b);
                rank_gather<PT>(a, buf, a.excl_items + b, rows, lane);
                rank_wave_sync();
                const float z = ro_score<MAXT, PT>(a, w_lds, buf, 0, tu, lane, g, col, KT0);
                const int r = 16 * g + col;
                if (g < PT && r < rows) {
                    const int item = a.excl_items[b + r];
                    if (item >= s0 && item < s1) st.count(z, item, n, -1);
                }
                rank_wave_sync();
            }
        }
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
            const int n = min(ra.tgt_ptr[j + 1] - ra.tgt_ptr[j], RO_T);
            if (n <= 0) continue;
            const int u = a.users ? a.users[j] : (int)j;
            f32x4 tu[MAXT];
            rank_load_user<MAXT>(a, u, g, tu);
            const RankOfSlot st(state, slot);
            for (int grp = 0; grp < rows; grp += 16 * PT) {
                const float z = ro_score<MAXT, PT>(a, w_lds, tile, grp, tu, lane, g, col, KT0);
                if (g < PT && grp + 16 * g + col < rows) st.count(z, t0 + grp + 16 * g + col, n, 1);
            }
        }
    }

    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        if (j >= a.m) break;
        const int tb = ra.tgt_ptr[j], n = min(ra.tgt_ptr[j + 1] - tb, RO_T);
        if (n <= 0) continue;
        const RankOfSlot st(state, slot);
        rank_wave_sync();
        if (lane < n) {
            int greater = 0;
            for (int p = lane + 1; p <= n; ++p) greater += st.cnt[p];
            const int e = st.tp[lane];
            if ((unsigned)e < (unsigned)n) {
                atomicAdd(ra.out_greater + tb + e, greater);
                atomicAdd(ra.out_before + tb + e, st.bf[lane]);
                atomicAdd(ra.out_after + tb + e, st.af[lane]);
            }
        }
    }
}

// AUC, reciprocal rank and average precision of one evaluated user per wavefront, from the flat counts (include/amar_hip.h).
__global__ __launch_bounds__(256) void rank_of_metrics_kernel(const float *__restrict__ scores, const int32_t *__restrict__ greater,
                                                               const int32_t *__restrict__ before, const int32_t *__restrict__ after,
                                                               const int32_t *__restrict__ rel_ptr, const int32_t *__restrict__ n_cand,
                                                               int64_t n_eval, int64_t n_targets, double *__restrict__ out,
                                                               int32_t *__restrict__ valid) {
    __shared__ double terms_all[4][AMAR_WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t v = (int64_t)blockIdx.x * 4 + wave;
    if (v >= n_eval) return;
    double *terms = terms_all[wave];
    const int lo = rel_ptr[v], hi = rel_ptr[v + 1];
    const long long R = (long long)hi - lo, n_neg = (long long)n_cand[v] - R;
    if (R <= 0 || n_neg <= 0 || lo < 0 || hi > n_targets) {            // (a segment outside the flat arrays is never read)
        if (lane == 0) { out[3 * v] = 0.0; out[3 * v + 1] = 0.0; out[3 * v + 2] = 0.0; valid[v] = 0; }
        return;
    }
    long long halves = 0;                                        // sum over targets of 2 neg_greater + neg_equal (this lane's)
    int r_min = 0x7fffffff;
    double ap = 0.0;                                             // (lane 0: the terms h_t / r_t added in target order)
    for (int base = lo; base < hi; base += AMAR_WAVE) {
        const int t = base + lane;
        const bool active = t < hi;
        const float s_t = active ? scores[t] : 0.f;
        const int g_t = active ? greater[t] : 0, b_t = active ? before[t] : 0, a_t = active ? after[t] : 0;
        const int r_t = 1 + g_t + b_t;
        int h = 0, above = 0, same = 0;
        for (int t2 = lo; t2 < hi; ++t2) {
            const float s2 = scores[t2];
            h += (1 + greater[t2] + before[t2] <= r_t) ? 1 : 0;
            above += s2 > s_t ? 1 : 0;
            same += (t2 != t && s2 == s_t) ? 1 : 0;
        }
        if (active) {
            halves += 2ll * (g_t - above) + (long long)(b_t + a_t - same);
            r_min = min(r_min, r_t);
        }
        terms[lane] = active ? (double)h / (double)r_t : 0.0;
        rank_wave_sync();
        if (lane == 0)
            for (int i = 0; i < AMAR_WAVE; ++i) ap += terms[i];
        rank_wave_sync();
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        halves += __shfl_xor(halves, off, 64);
        r_min = min(r_min, __shfl_xor(r_min, off, 64));
    }
    if (lane == 0) {
        out[3 * v] = 1.0 - (0.5 * (double)halves) / ((double)R * (double)n_neg);
        out[3 * v + 1] = 1.0 / (double)r_min;
        out[3 * v + 2] = ap / (double)R;
        valid[v] = 1;
    }
}

}  // namespace

extern "C" {

int32_t amar_rank_of_slices(int64_t m, int32_t n_items, const int32_t *dims, int32_t n_layers, int32_t n_slices) {
    RankShape s;
    const int rc = rank_slices_tile(m, 0, n_items, dims, n_layers, s);
    return rc != AMAR_OK ? rc : rank_slices(m, n_items, s.tile_items, RANK_UB, n_slices);
}

int amar_rank_of_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                     const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                     const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                     const int32_t *tgt_ptr, const int32_t *tgt_items, int64_t n_targets, int32_t max_targets, int32_t n_slices,
                     float *out_scores, int32_t *out_greater, int32_t *out_eq_before, int32_t *out_eq_after, amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || m < 0 || n_users < 0 || n_items < 0 || n_targets < 0 || max_targets < 0) return AMAR_EINVAL;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    if ((m > 0 && !tgt_ptr) || (n_targets > 0 && !tgt_items)) return AMAR_EINVAL;
    if (n_targets > 0 && (!out_scores || !out_greater || !out_eq_before || !out_eq_after)) return AMAR_EINVAL;
    const RankHead head = {Tu, ldu, Ti, ldi, n_items, c1, wpack, dims, acts, n_layers, in_act, users, excl_ptr, excl_items};
    RankOfArgs ra{};
    RankArgs &a = ra.r;
    RankShape sh;
    amar_rank_route_info route;
    const int rc = rank_prepare(AMAR_RANK_RANK_OF, head, m, a, sh, route);
    if (rc != AMAR_OK) return rc;
    if (max_targets > AMAR_RANK_OF_MAX_TARGETS || n_targets >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    const int32_t slices = amar_rank_of_slices(m, n_items, dims, n_layers, n_slices);
    if (slices < 1) return slices < 0 ? slices : AMAR_EINVAL;
    if (n_slices > 0 && slices != n_slices) return AMAR_EINVAL;
    a.slice_items = (int)rank_slice_rows(n_items, sh.tile_items, slices);
    ra.tgt_ptr = tgt_ptr; ra.tgt_items = tgt_items; ra.gather_floats = rank_of_gather_floats(sh);
    ra.out_scores = out_scores; ra.out_greater = out_greater; ra.out_before = out_eq_before; ra.out_after = out_eq_after;
    if (!route.fits) return AMAR_EUNSUPPORTED;
    const int64_t blocks = (m + RANK_UB - 1) / RANK_UB;
    if (blocks >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    if (m == 0 || n_targets == 0) return AMAR_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *counts[3] = {out_greater, out_eq_before, out_eq_after};         // the slices add their partials to zero
    for (int c = 0; c < 3; ++c) {
        const hipError_t e = hipMemsetAsync(counts[c], 0, (size_t)n_targets * sizeof(int32_t), st);
        if (e != hipSuccess) { amar_tls_hip_error = (int)e; return AMAR_ELAUNCH; }
    }
    static RankForms<RankOfArgs> forms = AMAR_RANK_FORMS(rank_of_kernel);
    return rank_launch_form(forms, route, dim3((unsigned)blocks, (unsigned)slices), st, ra);
}

int amar_rank_of_metrics_f64(const float *scores, const int32_t *greater, const int32_t *eq_before, const int32_t *eq_after,
                             int64_t n_targets, const int32_t *rel_ptr, const int32_t *n_cand, int64_t n_eval,
                             double *out, int32_t *valid, amar_stream_t stream) {
    if (n_targets < 0 || n_eval < 0) return AMAR_EINVAL;
    if (n_eval > 0 && (!rel_ptr || !n_cand || !out || !valid)) return AMAR_EINVAL;
    if (n_targets > 0 && (!scores || !greater || !eq_before || !eq_after)) return AMAR_EINVAL;
    if (n_targets >= (1ll << 31) || (n_eval + 3) / 4 >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    if (n_eval == 0) return AMAR_OK;
    hipLaunchKernelGGL(rank_of_metrics_kernel, dim3((unsigned)((n_eval + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), scores,
                       greater, eq_before, eq_after, rel_ptr, n_cand, n_eval, n_targets, out, valid);
    return amar_check_launch();
}

}  // extern "C"

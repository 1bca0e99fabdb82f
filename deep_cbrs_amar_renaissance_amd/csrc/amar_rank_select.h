// On-chip top-k selection of the fused rankers (amar_rank.hip: user -> item scores of the split head; amar_nearest.hip: dot /
// cosine neighbours).  The whole scheme lives here; a kernel computes a score per lane and calls it:
//   * the order (rank_better: score descending, row ascending: a strict total order) and RANK_EMPTY, the row of an empty slot;
//   * RankSlot, one query's selector in LDS: a sorted list of k <= 64 (score, row), a 64-entry candidate buffer and four state
//     words (candidates buffered, exclusion pointer, threshold = the current k-th best).  A wave owns its slots.  Per 64 scores
//     offer() tests the threshold, then the query's sorted exclusion list (binary search in the window the pointer has not
//     passed), merges a buffer that would overflow by rank counting, re-tests against the new threshold and appends by ballot;
//     advance() walks the exclusion pointer past a tile; finish() merges what is left and writes the list: the result with
//     -1 / -inf padding, or the slice's partial list.  Expected inserts ~ k ln(rows / k): per score the selection is one compare;
//   * rank_select_state_floats, the LDS a kernel reserves for its slots (the carve-up and the launch's byte count both use it);
//   * host side: how a call is cut into table slices (rank_slices, rank_slice_rows) and rank_merge_slices, the second launch
//     that merges a query's per-slice lists in slice order (the kernel is defined once, in amar_rank.hip).
#pragma once
#include "amar_common.h"

namespace {

constexpr int RANK_CAND = 64;                                                    // candidate buffer entries per query
constexpr int RANK_LIST = 64;                                                    // top-k list slots per query (k <= 64)
constexpr int RANK_EMPTY = 0x7fffffff;                                           // row of an empty slot (loses every tie)

__device__ __forceinline__ bool rank_better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// Merge n candidates (cs, ci) into the sorted list (ls, li) of k slots; one wave, every lane calls it.  Each entry's rank is the
// number of entries that beat it (rows are distinct inside a query, empty slots never reach a written rank).
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

// Floats of LDS the selector needs for `slots` queries: lists, candidate buffers, four state words each.
__host__ __device__ constexpr int rank_select_state_floats(int slots) { return slots * (2 * RANK_LIST + 2 * RANK_CAND + 4); }

// Where a kernel's lists go: n_slices == 1: the result [m, k]; else the per-slice lists [m][n_slices][k].
struct RankOut { int32_t *rows; float *scores; int k, n_slices; };

// Slot `slot` of the SLOTS selectors that start at `base`: [SLOTS] list scores, list rows, candidate scores, candidate rows, then
// [SLOTS] of each state word.  The state words live in LDS between tiles (init / store) and in registers while the wave walks a
// tile (load ... offer ... advance ... store).
template <int SLOTS>
struct RankSlot {
    float *ls, *cs;                              // sorted list / candidate buffer: scores
    int *li, *ci;                                //                                 rows
    int *state;                                  // the SLOTS selectors' state words: word w of this slot is st(w)
    int slot;
    int cnt, ep, ti;                             // state in registers: candidates buffered, exclusion pointer, threshold (ts, ti)
    float ts;

    __device__ __forceinline__ RankSlot(float *base, int slot_) : slot(slot_) {
        ls = base + slot * RANK_LIST;
        li = reinterpret_cast<int *>(base + SLOTS * RANK_LIST) + slot * RANK_LIST;
        cs = base + 2 * SLOTS * RANK_LIST + slot * RANK_CAND;
        ci = reinterpret_cast<int *>(base + 2 * SLOTS * RANK_LIST + SLOTS * RANK_CAND) + slot * RANK_CAND;
        state = reinterpret_cast<int *>(base + 2 * SLOTS * RANK_LIST + 2 * SLOTS * RANK_CAND);
    }
    __device__ __forceinline__ int &st(int w) const { return state[w * SLOTS + slot]; }

    // Empty list, empty buffer; the exclusion pointer starts at the first excluded row >= slice_start.  Lane 0 alone looks at
    // the exclusion window [excl_begin, excl_end) (an empty window: nothing is excluded).
    __device__ __forceinline__ void init(int lane, const int32_t *excl_rows, int excl_begin, int excl_end, int slice_start) {
        ls[lane] = -INFINITY;
        li[lane] = RANK_EMPTY;
        if (lane == 0) {
            st(0) = 0; st(1) = rank_lower_bound(excl_rows, excl_begin, excl_end, slice_start);
            st(2) = __float_as_int(-INFINITY); st(3) = RANK_EMPTY;
        }
    }

    __device__ __forceinline__ void load() { cnt = st(0); ep = st(1); ts = __int_as_float(st(2)); ti = st(3); }

    __device__ __forceinline__ void store(int lane) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) { st(0) = cnt; st(1) = ep; st(2) = __float_as_int(ts); st(3) = ti; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // One score per lane: z of row `item`, in_range false on lanes that hold none.  ee = end of the query's exclusion list.
    __device__ __forceinline__ void offer(float z, int item, bool in_range, const int32_t *excl_rows, int ee, int k, int lane) {
        bool pred = in_range && rank_better(z, item, ts, ti);
        if (__ballot(pred) == 0) return;
        if (pred && ep < ee) {                                   // excluded for this query?
            const int pos = rank_lower_bound(excl_rows, ep, ee, item);
            pred = !(pos < ee && excl_rows[pos] == item);
        }
        const uint64_t mask = __ballot(pred);
        if (mask == 0) return;
        const int n = __popcll(mask);
        if (cnt + n > RANK_CAND) {
            rank_merge(ls, li, cs, ci, cnt, k, lane);
            cnt = 0;
            ts = ls[k - 1]; ti = li[k - 1];
            pred = pred && rank_better(z, item, ts, ti);
        }
        const uint64_t mask2 = __ballot(pred);
        if (pred) {
            const int pos = cnt + __popcll(mask2 & ((1ull << lane) - 1ull));
            cs[pos] = z; ci[pos] = item;
        }
        cnt += __popcll(mask2);
    }

    // The exclusion pointer moves past a tile that ends before next_row.
    __device__ __forceinline__ void advance(const int32_t *excl_rows, int ee, int next_row) {
        if (ep < ee) ep = rank_lower_bound(excl_rows, ep, ee, next_row);
    }

    // Slice done: last merge, then the list of query j goes out (the final result, or this slice's partial list in
    // [m][n_slices][k] for rank_merge_slices).
    __device__ __forceinline__ void finish(int64_t j, int slice, const RankOut &o, int lane) {
        const int n = st(0);
        if (n > 0) rank_merge(ls, li, cs, ci, n, o.k, lane);
        if (lane < o.k) {
            const float s = ls[lane];
            const int i = li[lane];
            if (o.n_slices == 1) {
                o.rows[j * o.k + lane] = i == RANK_EMPTY ? -1 : i;
                o.scores[j * o.k + lane] = i == RANK_EMPTY ? -INFINITY : s;
            } else {
                const int64_t at = (j * o.n_slices + slice) * o.k + lane;
                o.rows[at] = i;
                o.scores[at] = s;
            }
        }
    }
};

// ---- host side --------------------------------------------------------------------------------------------------------------
// Rows of a slice when n_rows are cut into `slices` runs of whole tiles.
inline int64_t rank_slice_rows(int64_t n_rows, int tile_rows, int64_t slices) {
    const int64_t tiles = (n_rows + tile_rows - 1) / tile_rows;
    const int64_t rows = ((tiles + slices - 1) / slices) * tile_rows;
    return rows > 0 ? rows : tile_rows;
}

// Table slices of a call with m queries in blocks of block_queries: n_slices as requested (<= 0: automatic), clamped to what the
// table can give, and then the count actually launched, since slices cover whole tiles.
inline int32_t rank_slices(int64_t m, int64_t n_rows, int tile_rows, int block_queries, int32_t n_slices) {
    const int64_t tiles = (n_rows + tile_rows - 1) / tile_rows;
    const int64_t blocks = (m + block_queries - 1) / block_queries;
    int64_t want = n_slices;
    if (want <= 0) {
        // automatic: about four resident workgroups per CU of the 256 (a slice covers at least four tiles)
        want = blocks > 0 ? (1024 + blocks - 1) / blocks : 1;
        const int64_t cap = tiles / 4 > 0 ? tiles / 4 : 1;
        want = want > cap ? cap : want;
        want = want > 16 ? 16 : want;
    }
    if (want < 1) want = 1;
    if (want > tiles) want = tiles > 0 ? tiles : 1;
    if (want > 64) want = 64;
    const int64_t per = rank_slice_rows(n_rows, tile_rows, want);
    const int64_t eff = (n_rows + per - 1) / per;
    return (int32_t)(eff > 0 ? eff : 1);
}

}  // namespace

// Second launch of a sliced call: merges the `slices` partial lists [m][slices][k] of every query into out_rows / out_scores
// [m, k].  Returns an AMAR_* status.
int rank_merge_slices(const int32_t *part_rows, const float *part_scores, int64_t m, int slices, int k, int32_t *out_rows,
                      float *out_scores, hipStream_t stream);

// Explanations of recommended (user, item) pairs: the liked items most similar to the target, and the properties the target shares
// with other liked items (gfx950).
//
// One wavefront (one 64-thread workgroup) per list; the K targets of a list share one user.
//   * The user's liked rows are walked in chunks of 64.  Per chunk, targets and liked rows are staged through LDS in pieces of 32
//     columns ([64][36] floats each) and the 16 NT x 64 similarity tile is accumulated on v_mfma_f32_16x16x4_f32 (NT = ceil(K / 16),
//     a template parameter so that the accumulators stay in registers; features in the fragment order 16t + 4g + r of
//     amar_nearest_f32).  Squared norms are summed from the staged pieces, column ascending.  The finished tile is written over
//     the staging area as S[liked][target] ([64][68] floats), already scaled for cosine.
//   * Evidence: lane t owns target t and keeps its E best (similarity, item) pairs as a column of an LDS list [16][64]; liked
//     rows arrive ascending, so a stable insertion gives the item-ascending tie order.
//   * Properties: the property rows of a group of targets are copied to LDS (EXPLAIN_BUDGET entries, rows back to back) with one
//     float sum and one integer count per entry.  Liked item after liked item, the lanes take the (entry of the liked item's row,
//     target) pairs, look the property up in the target's row by bisection and add max(sim, 0) and 1 to its cells.  The pairs of
//     one liked item are distinct cells, and liked items follow each other in program order: every cell is summed in liked-row
//     order by plain LDS read-modify-writes.  Lists whose targets' rows exceed the budget take further passes over the liked rows
//     (a pass recomputes the tile; evidence belongs to the first pass).  Lane t then picks target t's Q best cells.
// No atomics, no scratch, no workspace in memory.
#include "amar_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int EXP_K = AMAR_EXPLAIN_MAX_K;          // targets per list = lanes
constexpr int EXP_SLOTS = AMAR_EXPLAIN_MAX_E;      // list slots per target (E, Q <= 16)
constexpr int EXP_BUDGET = AMAR_EXPLAIN_MAX_PROP_ROW;   // property cells in LDS per pass; one target row always fits
constexpr int EXP_COLS = 32;                       // columns staged at a time
constexpr int EXP_STAGE = EXP_COLS + 4;            // floats per staged row
constexpr int EXP_SROW = EXP_K + 4;                // floats per row of S
constexpr int EXP_MAX_D = 512;

struct ExplainArgs {
    const int32_t *lists; int K;
    const int32_t *users, *liked_ptr, *liked_items; int n_users;
    const float *T; int64_t ldt; int n_items, d, cosine;
    const int32_t *prop_ptr, *prop_ids; const float *prop_weight; int n_props;
    int E, Q;
    int32_t *out_ev; float *out_ev_sim;
    int32_t *out_props; float *out_prop_score; int32_t *out_prop_support;
};

// Stable insertion of (s, i) into column `lane` of a list sorted best first: an equal entry that is already there stays ahead.
__device__ __forceinline__ void column_insert(float *ls, int *li, int slots, float s, int i, int lane) {
    if (!(s > ls[(slots - 1) * 64 + lane])) return;
    int p = slots - 1;
    while (p > 0 && ls[(p - 1) * 64 + lane] < s) {
        ls[p * 64 + lane] = ls[(p - 1) * 64 + lane];
        li[p * 64 + lane] = li[(p - 1) * 64 + lane];
        --p;
    }
    ls[p * 64 + lane] = s;
    li[p * 64 + lane] = i;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int NT>
__global__ __launch_bounds__(64) void explain_kernel(const ExplainArgs a) {
    __shared__ __attribute__((aligned(16))) float stage[2 * 64 * EXP_STAGE];   // targets, liked rows; then S[liked][target]
    __shared__ float ls[EXP_SLOTS * 64];
    __shared__ int li[EXP_SLOTS * 64];
    __shared__ int lk_item[64], t_item[64], t_len[64], t_off[64];
    __shared__ int pid[EXP_BUDGET], pcnt[EXP_BUDGET];
    __shared__ float pacc[EXP_BUDGET];
    float *tg = stage, *lkrows = stage + 64 * EXP_STAGE, *S = stage;

    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15;
    const int64_t j = blockIdx.x;
    const int K = a.K, E = a.E, Q = a.Q;
    const int64_t u = a.users ? (int64_t)a.users[j] : j;
    const bool user_ok = u >= 0 && u < a.n_users;
    int item = -1;
    if (user_ok && lane < K) item = a.lists[j * K + lane];
    if (item < 0 || item >= a.n_items) item = -1;
    int lo = 0, L = 0;
    if (user_ok) { lo = a.liked_ptr[u]; L = a.liked_ptr[u + 1] - lo; }
    int pbase = 0, plen = 0;
    if (Q > 0 && a.prop_ptr && item >= 0) {
        pbase = a.prop_ptr[item];
        plen = min(a.prop_ptr[item + 1] - pbase, EXP_BUDGET);
    }
    t_item[lane] = item;
    t_len[lane] = plen;
#pragma unroll
    for (int e = 0; e < EXP_SLOTS; ++e) { ls[e * 64 + lane] = -INFINITY; li[e * 64 + lane] = -1; }

    int k0 = 0;
    for (int pass = 0; k0 < K; ++pass) {
        // the targets of this pass: as many consecutive ones as the cell budget holds, at least one
        int k1 = k0, total = 0, off = 0;
        while (k1 < K) {
            const int l = __shfl(plen, k1, 64);
            if (k1 > k0 && total + l > EXP_BUDGET) break;
            if (lane == k1) off = total;
            total += l;
            ++k1;
        }
        const int G = k1 - k0;
        t_off[lane] = off;
        for (int k = k0; k < k1; ++k) {
            const int base = __shfl(pbase, k, 64), l = __shfl(plen, k, 64), o = __shfl(off, k, 64);
            for (int s = lane; s < l; s += 64) { pid[o + s] = a.prop_ids[base + s]; pacc[o + s] = 0.f; pcnt[o + s] = 0; }
        }
        __syncthreads();

        for (int c0 = 0; c0 < L; c0 += 64) {
            const int nc = min(64, L - c0);
            int lk = lane < nc ? a.liked_items[lo + c0 + lane] : -1;
            if (lk < 0 || lk >= a.n_items) lk = -1;
            int rbase = 0, rlen = 0;
            if (total > 0 && lk >= 0) { rbase = a.prop_ptr[lk]; rlen = a.prop_ptr[lk + 1] - rbase; }

            f32x4 acc[NT][4];
#pragma unroll
            for (int bi = 0; bi < NT; ++bi)
#pragma unroll
                for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = f32x4{0.f, 0.f, 0.f, 0.f};
            float ss_t = 0.f, ss_l = 0.f;
            for (int d0 = 0; d0 < a.d; d0 += EXP_COLS) {
                __syncthreads();                                 // the previous piece, or S, is no longer read
#pragma unroll
                for (int i = 0; i < 2 * NT; ++i) {               // 16 NT target rows x 8 float4s, 8 lanes per row
                    const int idx = lane + 64 * i, r = idx >> 3, f = 4 * (idx & 7);
                    const int it = __shfl(item, r, 64);
                    float4 v = f4_zero();
                    if (it >= 0 && d0 + f < a.d) v = *reinterpret_cast<const float4 *>(a.T + (int64_t)it * a.ldt + d0 + f);
                    *reinterpret_cast<float4 *>(&tg[r * EXP_STAGE + f]) = v;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {                    // 64 liked rows
                    const int idx = lane + 64 * i, r = idx >> 3, f = 4 * (idx & 7);
                    const int it = __shfl(lk, r, 64);
                    float4 v = f4_zero();
                    if (it >= 0 && d0 + f < a.d) v = *reinterpret_cast<const float4 *>(a.T + (int64_t)it * a.ldt + d0 + f);
                    *reinterpret_cast<float4 *>(&lkrows[r * EXP_STAGE + f]) = v;
                }
                __syncthreads();
                if (a.cosine) {
#pragma unroll
                    for (int f = 0; f < EXP_COLS; f += 4) {
                        const float4 v = *reinterpret_cast<const float4 *>(&lkrows[lane * EXP_STAGE + f]);
                        ss_l = fmaf(v.x, v.x, ss_l); ss_l = fmaf(v.y, v.y, ss_l);
                        ss_l = fmaf(v.z, v.z, ss_l); ss_l = fmaf(v.w, v.w, ss_l);
                    }
                    if (lane < 16 * NT) {
#pragma unroll
                        for (int f = 0; f < EXP_COLS; f += 4) {
                            const float4 v = *reinterpret_cast<const float4 *>(&tg[lane * EXP_STAGE + f]);
                            ss_t = fmaf(v.x, v.x, ss_t); ss_t = fmaf(v.y, v.y, ss_t);
                            ss_t = fmaf(v.z, v.z, ss_t); ss_t = fmaf(v.w, v.w, ss_t);
                        }
                    }
                }
                const int steps = min(EXP_COLS / 16, (a.d - d0 + 15) >> 4);
                for (int t = 0; t < steps; ++t) {
                    f32x4 xa[NT], xb[4];
#pragma unroll
                    for (int b = 0; b < NT; ++b) xa[b] = *reinterpret_cast<const f32x4 *>(&tg[(16 * b + col) * EXP_STAGE + 16 * t + 4 * g]);
#pragma unroll
                    for (int b = 0; b < 4; ++b) xb[b] = *reinterpret_cast<const f32x4 *>(&lkrows[(16 * b + col) * EXP_STAGE + 16 * t + 4 * g]);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int bi = 0; bi < NT; ++bi)
#pragma unroll
                            for (int bj = 0; bj < 4; ++bj)
                                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[bi][r], xb[bj][r], acc[bi][bj], 0, 0, 0);
                }
            }
            __syncthreads();
            // lane (g, col), register r of unit (bi, bj): target 16 bi + 4 g + r against liked row 16 bj + col
            const float inv_t = ss_t > 0.f ? 1.f / sqrtf(ss_t) : 0.f, inv_l = ss_l > 0.f ? 1.f / sqrtf(ss_l) : 0.f;
#pragma unroll
            for (int bi = 0; bi < NT; ++bi) {
                float it4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) it4[r] = __shfl(inv_t, 16 * bi + 4 * g + r, 64);
#pragma unroll
                for (int bj = 0; bj < 4; ++bj) {
                    const float il = __shfl(inv_l, 16 * bj + col, 64);
                    f32x4 v = acc[bi][bj];
                    if (a.cosine) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = (v[r] * it4[r]) * il;
                    }
                    *reinterpret_cast<f32x4 *>(&S[(16 * bj + col) * EXP_SROW + 16 * bi + 4 * g]) = v;
                }
            }
            lk_item[lane] = lk;
            __syncthreads();

            if (pass == 0 && item >= 0) {
                for (int c = 0; c < nc; ++c) {
                    const int it = lk_item[c];
                    if (it < 0 || it == item) continue;
                    float s = S[c * EXP_SROW + lane];
                    if (!(s == s)) s = -INFINITY;                // a NaN (non-finite input) must not break the order's totality
                    column_insert(ls, li, E, s, it, lane);
                }
            }
            if (total > 0) {
                for (int c = 0; c < nc; ++c) {
                    const int jt = __shfl(lk, c, 64), base = __shfl(rbase, c, 64), pairs = __shfl(rlen, c, 64) * G;
                    for (int q = lane; q < pairs; q += 64) {
                        const int e = q / G, kk = k0 + (q - e * G);
                        const int ik = t_item[kk], len = t_len[kk];
                        if (ik < 0 || ik == jt || len == 0) continue;
                        const int p = a.prop_ids[base + e];
                        const int o = t_off[kk];
                        int b0 = o, b1 = o + len;
                        while (b0 < b1) {
                            const int mid = (b0 + b1) >> 1;
                            if (pid[mid] < p) b0 = mid + 1; else b1 = mid;
                        }
                        if (b0 < o + len && pid[b0] == p) {
                            pcnt[b0] += 1;
                            pacc[b0] += fmaxf(S[c * EXP_SROW + kk], 0.f);
                        }
                    }
                    wave_sync();                                 // the next liked item may touch the same cells
                }
            }
        }

        if (pass == 0) {
            __syncthreads();
            if (lane < K) {
                for (int e = 0; e < E; ++e) {
                    a.out_ev[(j * K + lane) * E + e] = li[e * 64 + lane];
                    a.out_ev_sim[(j * K + lane) * E + e] = ls[e * 64 + lane];
                }
            }
        }
        if (Q == 0) break;                                       // no property part: one pass covers every target
        __syncthreads();
        for (int s = lane; s < total; s += 64) {
            const int p = pid[s];
            pacc[s] = (p >= 0 && p < a.n_props) ? a.prop_weight[p] * pacc[s] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < EXP_SLOTS; ++e) { ls[e * 64 + lane] = -INFINITY; li[e * 64 + lane] = -1; }
        __syncthreads();
        if (lane >= k0 && lane < k1) {
            for (int s = 0; s < plen; ++s) {
                if (pcnt[off + s] == 0) continue;
                float sc = pacc[off + s];
                if (!(sc == sc)) sc = -INFINITY;
                column_insert(ls, li, Q, sc, off + s, lane);
            }
            for (int q = 0; q < Q; ++q) {
                const int cell = li[q * 64 + lane];
                const int64_t o = (j * K + lane) * Q + q;
                a.out_props[o] = cell >= 0 ? pid[cell] : -1;
                a.out_prop_score[o] = cell >= 0 ? ls[q * 64 + lane] : -INFINITY;
                a.out_prop_support[o] = cell >= 0 ? pcnt[cell] : 0;
            }
        }
        __syncthreads();
        k0 = k1;
    }
}

}  // namespace

extern "C" {

int amar_explain_f32(const int32_t *lists, int64_t m, int32_t K, const int32_t *users, const int32_t *liked_ptr,
                     const int32_t *liked_items, int32_t n_users, const float *T, int64_t ldt, int32_t n_items, int32_t d,
                     int32_t metric, const int32_t *prop_ptr, const int32_t *prop_ids, const float *prop_weight, int32_t n_props,
                     int32_t max_prop_row, int32_t n_evidence, int32_t n_properties, int32_t *out_evidence,
                     float *out_evidence_sim, int32_t *out_props, float *out_prop_score, int32_t *out_prop_support,
                     amar_stream_t stream) {
    if (!T || !liked_ptr || m < 0 || K < 1 || n_users < 0 || n_items < 0 || d < 0 || n_props < 0 || max_prop_row < 0) return AMAR_EINVAL;
    if (metric != AMAR_NEAREST_DOT && metric != AMAR_NEAREST_COSINE) return AMAR_EINVAL;
    if (ldt < d || n_evidence < 1 || n_properties < 0) return AMAR_EINVAL;
    if (!users && m != n_users) return AMAR_EINVAL;
    const bool any_prop = prop_ptr || prop_ids || prop_weight;
    if (any_prop && !(prop_ptr && prop_ids && prop_weight)) return AMAR_EINVAL;
    if (K > EXP_K || n_evidence > EXP_SLOTS || n_properties > EXP_SLOTS) return AMAR_EUNSUPPORTED;
    if (d < 4 || (d & 3) || d > EXP_MAX_D) return AMAR_EUNSUPPORTED;
    if ((ldt & 3) || !amar_aligned16(T)) return AMAR_EUNSUPPORTED;
    if (any_prop && max_prop_row > EXP_BUDGET) return AMAR_EUNSUPPORTED;
    if (m >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    if (m == 0) return AMAR_OK;
    if (!lists || !liked_items || !out_evidence || !out_evidence_sim) return AMAR_EINVAL;
    if (n_properties > 0 && (!out_props || !out_prop_score || !out_prop_support)) return AMAR_EINVAL;
    ExplainArgs a{};
    a.lists = lists; a.K = K;
    a.users = users; a.liked_ptr = liked_ptr; a.liked_items = liked_items; a.n_users = n_users;
    a.T = T; a.ldt = ldt; a.n_items = n_items; a.d = d; a.cosine = metric == AMAR_NEAREST_COSINE ? 1 : 0;
    a.prop_ptr = prop_ptr; a.prop_ids = prop_ids; a.prop_weight = prop_weight; a.n_props = n_props;
    a.E = n_evidence; a.Q = n_properties;
    a.out_ev = out_evidence; a.out_ev_sim = out_evidence_sim;
    a.out_props = out_props; a.out_prop_score = out_prop_score; a.out_prop_support = out_prop_support;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)m), block(64);
    switch ((K + 15) / 16) {
        case 1: hipLaunchKernelGGL(explain_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(explain_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(explain_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(explain_kernel<4>, grid, block, 0, st, a); break;
    }
    return amar_check_launch();
}

}  // extern "C"

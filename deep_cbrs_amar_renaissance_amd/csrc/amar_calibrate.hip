// Calibrated re-ranking (Steck 2018): greedy selection from a pool of at most 64 candidates against the Kullback-Leibler distance
// between the user's category distribution and the list's, and that distance of finished lists on float64 (gfx950).
//
// One wavefront (one 64-thread workgroup) per list; lane t owns position t of the pool / rank t of the list.
//   * Target: p[G] lives in LDS.  The user's liked rows are walked once in item-row order; the lanes take the entries of one liked
//     item's category row (the next item's first 64 entries are already on their way).  The cells of one row are distinct and the
//     liked items follow each other in program order, so plain LDS read-modify-writes sum every cell in liked-row order.
//   * Pool rows: the candidates' category rows are copied to LDS, position after position, while they fit CAL_BUDGET entries; the
//     rows past that are read from memory every time they are needed.  An id outside 0..G-1 is staged as -1 and skipped.
//   * A step: the list's sums n[G] (LDS) give, for the normalisers |S+| and |S+| + 1, the G-wide sum of the terms
//     p log(p / ((1 - a) n / N + a p)): the lanes take g = lane, lane + 64, ... and a 6-level xor butterfly adds the 64 partial sums
//     (a + b commutes, so every lane holds the same bits).  Lane t then walks its own row and exchanges the terms of its cells for
//     the ones with n + 1/len_t; a neutral candidate keeps the sum at |S+|.  The winner comes from the (key, position) butterfly of
//     amar_rerank_mmr_f32, and its row is added to n by all lanes (distinct cells again).
//   * The float64 metric keeps p, n and the terms of one cutoff in LDS as doubles and adds the terms g ascending.
// No atomics, no scratch, no workspace in memory.
#include "amar_common.h"

namespace {

constexpr int CAL_P = AMAR_CALIBRATE_MAX_P;          // pool positions = lanes
constexpr int CAL_G = AMAR_CALIBRATE_MAX_G;          // categories: floats of p and of n in LDS
constexpr int CAL_BUDGET = AMAR_CALIBRATE_POOL_BUDGET;   // staged category ids of the pool's rows

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One cell's share of C: p log(p / ((1 - a) q + a p)), q = x / N (0 when N is 0); p > 0.
__device__ __forceinline__ float cal_term(float p, float x, float N, float oma, float alpha) {
    const float q = N > 0.f ? x / N : 0.f;
    const float den = fmaf(oma, q, alpha * p);
    return p * logf(p / den);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over g = lane, lane + 64, ... of the terms at normaliser N, then over the lanes
__device__ __forceinline__ float cal_base(const float *p, const float *n, int G, float N, float oma, float alpha, int lane) {
    float s = 0.f;
    for (int g = lane; g < G; g += 64) {
        const float pg = p[g];
        if (pg > 0.f) s += cal_term(pg, n[g], N, oma, alpha);
    }
    return wave_sum(s);
}

struct CalUser {
    const int32_t *users, *liked_ptr, *liked_items; int n_users;
    const int32_t *cat_ptr, *cat_ids; int n_items, G;
};

// Adds 1/len of every liked item with a non-empty row to the cells of its categories (acc[0:G], zeroed here), liked items in
// segment order; returns the number of such items.  T = float for the re-ranking, double for the metric.
template <typename T>
__device__ __forceinline__ int cal_liked_sums(const CalUser &a, int64_t u, T *acc, int lane) {
    for (int g = lane; g < a.G; g += 64) acc[g] = (T)0;
    wave_sync();
    const int64_t lo = a.liked_ptr[u];
    const int L = (int)(a.liked_ptr[u + 1] - lo);
    int support = 0;
    for (int c0 = 0; c0 < L; c0 += 64) {
        const int nc = min(64, L - c0);
        int lk = lane < nc ? a.liked_items[lo + c0 + lane] : -1;
        if (lk < 0 || lk >= a.n_items) lk = -1;
        int rbase = 0, rlen = 0;
        if (lk >= 0) { rbase = a.cat_ptr[lk]; rlen = a.cat_ptr[lk + 1] - rbase; }
        int base = __shfl(rbase, 0, 64);
        int len = __shfl(rlen, 0, 64);
        int g_cur = lane < len ? a.cat_ids[(int64_t)base + lane] : -1;
        for (int c = 0; c < nc; ++c) {
            const int base_next = __shfl(rbase, (c + 1) & 63, 64);
            const int len_next = c + 1 < nc ? __shfl(rlen, (c + 1) & 63, 64) : 0;
            const int g_next = lane < len_next ? a.cat_ids[(int64_t)base_next + lane] : -1;
            if (len > 0) {
                const T w = (T)1 / (T)len;
                if (g_cur >= 0 && g_cur < a.G) acc[g_cur] += w;
                for (int e = 64 + lane; e < len; e += 64) {
                    const int g = a.cat_ids[(int64_t)base + e];
                    if (g >= 0 && g < a.G) acc[g] += w;
                }
                ++support;
                wave_sync();                                 // the next liked item may touch the same cells
            }
            base = base_next; len = len_next; g_cur = g_next;
        }
    }
    return support;
}

struct CalArgs {
    const int32_t *pool_items; const float *pool_scores; int P;
    CalUser u;
    float lambda, alpha; int k;
    int32_t *out_items; float *out_scores, *out_value, *out_kl, *out_target;
};

__global__ __launch_bounds__(64) void rerank_calibrated_kernel(const CalArgs a) {
    __shared__ float p[CAL_G], n[CAL_G];
    __shared__ int staged[CAL_BUDGET];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int G = a.u.G, k = a.k;
    const int64_t u = a.u.users ? (int64_t)a.u.users[j] : j;
    const bool user_ok = u >= 0 && u < a.u.n_users;

    int item = -1;
    float score = 0.f;
    if (user_ok && lane < a.P) {
        item = a.pool_items[j * a.P + lane];
        score = a.pool_scores[j * a.P + lane];
    }
    if (item < 0 || item >= a.u.n_items) item = -1;
    const bool valid = item >= 0;
    const int n_valid = __popcll(__ballot(valid));

    // the target
    const int support = user_ok ? cal_liked_sums<float>(a.u, u, p, lane) : 0;
    const bool has_target = support > 0;
    for (int g = lane; g < G; g += 64) {
        const float pg = has_target ? p[g] / (float)support : 0.f;
        p[g] = pg;
        n[g] = 0.f;
        if (a.out_target) a.out_target[j * G + g] = pg;
    }

    // the pool's rows: lengths, 1/len, and the staged prefix
    int rbase = 0, rlen = 0;
    if (valid && has_target) { rbase = a.u.cat_ptr[item]; rlen = min(a.u.cat_ptr[item + 1] - rbase, G); }
    if (rlen < 0) rlen = 0;
    const float w = rlen > 0 ? 1.f / (float)rlen : 0.f;
    int off = rlen;                                              // inclusive prefix sum of the lengths, lane order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(off, d, 64);
        if (lane >= d) off += o;
    }
    off -= rlen;
    const bool in_lds = off + rlen <= CAL_BUDGET;               // a prefix of the positions: the offsets only grow
    for (int t = 0; t < a.P; ++t) {
        const int b = __shfl(rbase, t, 64), l = __shfl(rlen, t, 64), o = __shfl(off, t, 64);
        if (o + l > CAL_BUDGET) break;
        for (int e = lane; e < l; e += 64) {
            const int g = a.u.cat_ids[(int64_t)b + e];
            staged[o + e] = (g >= 0 && g < G) ? g : -1;
        }
    }
    __syncthreads();

    float r_min = valid ? score : INFINITY, r_max = valid ? score : -INFINITY;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        r_min = fminf(r_min, __shfl_xor(r_min, d, 64));
        r_max = fmaxf(r_max, __shfl_xor(r_max, d, 64));
    }
    const float rel = r_max > r_min ? (score - r_min) / (r_max - r_min) : 1.f;
    const float lrel = a.lambda * rel, oml = 1.f - a.lambda, alpha = a.alpha, oma = 1.f - a.alpha;
    const bool by_score = oml == 0.f || !has_target;

    bool selected = false;
    int cnt = 0;                                                 // |S+|
    int o_item = -1;
    float o_score = -INFINITY, o_v = -INFINITY, o_kl = -INFINITY;
    const int steps = min(k, n_valid);
    for (int s = 0; s < steps; ++s) {
        float C = 0.f;
        if (has_target) {
            const float N0 = (float)cnt, N1 = (float)(cnt + 1);
            const float base0 = cal_base(p, n, G, N0, oma, alpha, lane);
            const float base1 = cal_base(p, n, G, N1, oma, alpha, lane);
            C = base0;
            if (valid && !selected && rlen > 0) {
                float delta = 0.f;
                for (int e = 0; e < rlen; ++e) {
                    const int g = in_lds ? staged[off + e] : a.u.cat_ids[(int64_t)rbase + e];
                    if (g < 0 || g >= G) continue;
                    const float pg = p[g];
                    if (!(pg > 0.f)) continue;
                    const float x = n[g];
                    delta += cal_term(pg, x + w, N1, oma, alpha) - cal_term(pg, x, N1, oma, alpha);
                }
                C = base1 + delta;
            }
        }
        const float v = lrel - oml * C;
        float key = by_score ? score : v;
        if (!(key == key)) key = -INFINITY;                      // a NaN (non-finite input) must not break the order's totality
        const bool cand = valid && !selected;
        float bk = cand ? key : -INFINITY;
        int bp = cand ? lane : 64 + lane;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float ok = __shfl_xor(bk, d, 64);
            const int op = __shfl_xor(bp, d, 64);
            if (ok > bk || (ok == bk && op < bp)) { bk = ok; bp = op; }
        }
        const int t = __builtin_amdgcn_readfirstlane(bp);
        if (t >= CAL_P) break;
        const int t_item = __shfl(item, t, 64);
        const float t_score = __shfl(score, t, 64), t_v = __shfl(v, t, 64), t_C = __shfl(C, t, 64), t_w = __shfl(w, t, 64);
        const int t_base = __shfl(rbase, t, 64), t_len = __shfl(rlen, t, 64), t_off = __shfl(off, t, 64);
        const bool t_lds = t_off + t_len <= CAL_BUDGET;
        if (lane == s) { o_item = t_item; o_score = t_score; o_v = t_v; o_kl = t_C; }
        if (lane == t) selected = true;
        if (t_len > 0) {
            wave_sync();                                         // every lane has read n for this step
            for (int e = lane; e < t_len; e += 64) {
                const int g = t_lds ? staged[t_off + e] : a.u.cat_ids[(int64_t)t_base + e];
                if (g >= 0 && g < G) n[g] += t_w;
            }
            ++cnt;
            wave_sync();
        }
    }
    if (lane < k) {
        a.out_items[j * k + lane] = o_item;
        a.out_scores[j * k + lane] = o_score;
        if (a.out_value) a.out_value[j * k + lane] = o_v;
        if (a.out_kl) a.out_kl[j * k + lane] = o_kl;
    }
}

struct CalMetricArgs {
    const int32_t *lists; int K;
    CalUser u;
    double alpha;
    int nk, ks[AMAR_RANK_METRICS_MAX_KS];
    double *out_kl; int32_t *out_count, *out_support;
};

__global__ __launch_bounds__(64) void list_calibration_kernel(const CalMetricArgs a) {
    __shared__ double p[CAL_G], n[CAL_G], term[CAL_G];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int G = a.u.G;
    const int64_t u = a.u.users ? (int64_t)a.u.users[j] : j;
    const bool user_ok = u >= 0 && u < a.u.n_users;
    int item = -1;
    if (user_ok && lane < a.K) item = a.lists[j * a.K + lane];
    if (item < 0 || item >= a.u.n_items) item = -1;
    int rbase = 0, rlen = 0;
    if (item >= 0) { rbase = a.u.cat_ptr[item]; rlen = max(a.u.cat_ptr[item + 1] - rbase, 0); }
    const uint64_t full = __ballot(rlen > 0);                    // the non-neutral ranks

    const int support = user_ok ? cal_liked_sums<double>(a.u, u, p, lane) : 0;
    for (int g = lane; g < G; g += 64) {
        if (support > 0) p[g] = p[g] / (double)support;
        n[g] = 0.0;
    }
    wave_sync();
    if (lane == 0) a.out_support[j] = support;

    const double alpha = a.alpha, oma = 1.0 - a.alpha;
    int r = 0;                                                   // ranks already added to n
    for (int q = 0; q < a.nk; ++q) {
        // cutoffs in the caller's order: start again when one is smaller than its predecessor
        const int kq = a.ks[q];
        if (kq < r) {
            for (int g = lane; g < G; g += 64) n[g] = 0.0;
            wave_sync();
            r = 0;
        }
        for (; r < kq; ++r) {
            const int l = __shfl(rlen, r, 64);
            if (l == 0) continue;
            const int b = __shfl(rbase, r, 64);
            const double w = 1.0 / (double)l;
            for (int e = lane; e < l; e += 64) {
                const int g = a.u.cat_ids[(int64_t)b + e];
                if (g >= 0 && g < G) n[g] += w;
            }
            wave_sync();                                         // the next rank may touch the same cells
        }
        const int count = __popcll(full & (kq >= 64 ? ~0ull : (1ull << kq) - 1ull));
        double C = 0.0;
        if (support > 0) {
            for (int g = lane; g < G; g += 64) {
                const double pg = p[g];
                double t = 0.0;
                if (pg > 0.0) {
                    const double qg = count > 0 ? n[g] / (double)count : 0.0;
                    t = pg * log(pg / (oma * qg + alpha * pg));
                }
                term[g] = t;
            }
            wave_sync();
            for (int g = 0; g < G; ++g) C += term[g];            // g ascending, the same address for every lane
            wave_sync();
        }
        if (lane == 0) {
            a.out_kl[j * a.nk + q] = C;
            a.out_count[j * a.nk + q] = count;
        }
    }
}

// What both entries refuse before any device call.
int calibrate_check(int64_t m, int32_t P, const int32_t *liked_ptr, const int32_t *liked_items, int32_t n_users, const int32_t *users,
                    const int32_t *cat_ptr, const int32_t *cat_ids, int32_t n_items, int32_t G, float smoothing) {
    if (!liked_ptr || !liked_items || !cat_ptr || !cat_ids) return AMAR_EINVAL;
    if (m < 0 || P < 1 || n_users < 0 || n_items < 0 || G < 1) return AMAR_EINVAL;
    if (!(smoothing > 0.f && smoothing < 1.f)) return AMAR_EINVAL;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (P > CAL_P || G > CAL_G || m >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    return AMAR_OK;
}

}  // namespace

extern "C" {

int amar_rerank_calibrated_f32(const int32_t *pool_items, const float *pool_scores, int64_t m, int32_t P, const int32_t *users,
                               const int32_t *liked_ptr, const int32_t *liked_items, int32_t n_users, const int32_t *cat_ptr,
                               const int32_t *cat_ids, int32_t n_items, int32_t G, int32_t max_cat_row, float trade_off,
                               float smoothing, int32_t k, int32_t *out_items, float *out_scores, float *out_value, float *out_kl,
                               float *out_target, amar_stream_t stream) {
    const int rc = calibrate_check(m, P, liked_ptr, liked_items, n_users, users, cat_ptr, cat_ids, n_items, G, smoothing);
    if (rc == AMAR_EINVAL) return rc;
    if (k < 1 || max_cat_row < 0 || !(trade_off >= 0.f && trade_off <= 1.f)) return AMAR_EINVAL;
    if (rc != AMAR_OK) return rc;
    if (k > P || max_cat_row > G) return AMAR_EUNSUPPORTED;
    if (m == 0) return AMAR_OK;
    if (!pool_items || !pool_scores || !out_items || !out_scores) return AMAR_EINVAL;
    CalArgs a{};
    a.pool_items = pool_items; a.pool_scores = pool_scores; a.P = P;
    a.u.users = users; a.u.liked_ptr = liked_ptr; a.u.liked_items = liked_items; a.u.n_users = n_users;
    a.u.cat_ptr = cat_ptr; a.u.cat_ids = cat_ids; a.u.n_items = n_items; a.u.G = G;
    a.lambda = trade_off; a.alpha = smoothing; a.k = k;
    a.out_items = out_items; a.out_scores = out_scores; a.out_value = out_value; a.out_kl = out_kl; a.out_target = out_target;
    hipLaunchKernelGGL(rerank_calibrated_kernel, dim3((unsigned)m), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return amar_check_launch();
}

int amar_list_calibration_f64(const int32_t *lists, int64_t m, int32_t K, const int32_t *users, const int32_t *liked_ptr,
                              const int32_t *liked_items, int32_t n_users, const int32_t *cat_ptr, const int32_t *cat_ids,
                              int32_t n_items, int32_t G, float smoothing, const int32_t *ks, int32_t nk, double *out_kl,
                              int32_t *out_count, int32_t *out_support, amar_stream_t stream) {
    const int rc = calibrate_check(m, K, liked_ptr, liked_items, n_users, users, cat_ptr, cat_ids, n_items, G, smoothing);
    if (rc == AMAR_EINVAL) return rc;
    if (!ks || nk < 1) return AMAR_EINVAL;
    if (rc != AMAR_OK) return rc;
    if (nk > AMAR_RANK_METRICS_MAX_KS) return AMAR_EUNSUPPORTED;
    for (int q = 0; q < nk; ++q)
        if (ks[q] < 1 || ks[q] > K) return AMAR_EINVAL;
    if (m == 0) return AMAR_OK;
    if (!lists || !out_kl || !out_count || !out_support) return AMAR_EINVAL;
    CalMetricArgs a{};
    a.lists = lists; a.K = K;
    a.u.users = users; a.u.liked_ptr = liked_ptr; a.u.liked_items = liked_items; a.u.n_users = n_users;
    a.u.cat_ptr = cat_ptr; a.u.cat_ids = cat_ids; a.u.n_items = n_items; a.u.G = G;
    a.alpha = (double)smoothing;
    a.nk = nk;
    for (int q = 0; q < nk; ++q) a.ks[q] = ks[q];
    a.out_kl = out_kl; a.out_count = out_count; a.out_support = out_support;
    hipLaunchKernelGGL(list_calibration_kernel, dim3((unsigned)m), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return amar_check_launch();
}

}  // extern "C"

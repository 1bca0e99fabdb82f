// BPR training (gfx950): the pairwise loss's gradient and the on-device positive / negative sampler.
//
// amar_bpr_grad_f32 is the counterpart of amar_bce_grad_f32 (amar_train.hip) for utilities/losses.py:BPRLoss: one lane per pair
// (j, h + j), no float atomics, so a training step stays reproducible bit for bit.
// amar_bpr_sample_i32 draws one batch of data/datasets.py:UserItemGraphPosNegSample in the reference's layout from a counter-based
// RNG (Philox4x32-10): the draws depend on (seed, step, j) only, so data/datasets.py:bpr_device_batch restates every id, and a step
// index read from device memory lets a captured training graph draw new ids on every replay.
// amar_bpr_sample_triplets_i32 draws (user, positive, negative) triples of data/datasets.py:UserItemGraphTriplets the same way: both
// items of a pair belong to one user and the negative is uniform over the items outside that user's exclusion row
// (data/datasets.py:bpr_triplet_device_batch restates it).
#include "amar_common.h"
#include "amar_philox.h"

namespace {

// -log sigmoid(p[j] - p[h + j]) for j < h.  terms[j] = (B / h) * that, terms[h + j] = 0 (and the dropped trailing element of an odd
// batch: 0), so that sum(terms) = B * loss like amar_bce_grad_f32's terms.  dz = d(loss)/d(logit) through the final sigmoid.
__global__ __launch_bounds__(256) void bpr_grad_kernel(const float *__restrict__ p, int64_t ldp, float *__restrict__ dz,
                                                       float *__restrict__ terms, int64_t B, int64_t h) {
    const float scale = h ? (float)B / (float)h : 0.f, inv_h = h ? 1.f / (float)h : 0.f;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < h; j += (int64_t)gridDim.x * blockDim.x) {
        const float a = p[j * ldp], b = p[(h + j) * ldp];
        const float x = a - b;                                        // in (-1, 1): probabilities, so exp cannot overflow
        const float e = expf(-x);
        const float one_minus_s = e / (1.f + e);                      // 1 - sigmoid(x)
        terms[j] = scale * log1pf(e);                                 // -log sigmoid(x)
        terms[h + j] = 0.f;
        const float g = one_minus_s * inv_h;
        dz[j] = -g * (a * (1.f - a));
        dz[h + j] = g * (b * (1.f - b));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && 2 * h < B) {
        dz[B - 1] = 0.f;
        terms[B - 1] = 0.f;
    }
}

// Listwise losses on the triplet layout (include/amar_hip.h: amar_group_loss_grad_f32).  A group occupies a segment of W lanes of
// one wavefront (W = the next power of two >= K for K <= 32: 64 / W groups per wavefront; W = 64 above: lane l takes the negatives
// k = l, l + 64, ... in ascending order).  Every reduction is that lane-local ascending pass followed by an xor butterfly inside the
// segment: both partners of a step add the same two floats, so all W lanes hold the same bits and those bits depend on the group's
// own floats only.  All 64 lanes stay active through the butterflies (a lane without a group carries neutral values and stores
// nothing); the loop over groups is uniform over the workgroup.  The launch moves a few thousand floats: a group's negatives beyond
// the first 64 are read again from L1 in the later passes, nothing is staged.
template <int W>
__device__ __forceinline__ float seg_sum(float x) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <int W>
__global__ __launch_bounds__(256) void group_loss_kernel(int32_t kind, float hyper, const float *__restrict__ p, int64_t ldp,
                                                         float *__restrict__ dz, float *__restrict__ terms, int64_t B, int64_t h,
                                                         int32_t K, int64_t G) {
    constexpr int GW = 64 / W;                                        // groups per wavefront
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & (W - 1);
    const float scale = G ? (float)B / (float)G : 0.f, inv_g = G ? 1.f / (float)G : 0.f, fk = (float)K;
    const int64_t per_block = 4 * GW;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < G; base += (int64_t)gridDim.x * per_block) {
        const int64_t g = base + wave * GW + lane / W;
        const bool live = g < G;
        const int64_t row0 = live ? g * K : 0, nrow = h + row0;       // the positive's row, the first negative's row
        const float a = live ? p[row0 * ldp] : 0.f;
        const bool first = live && j < K;
        const float b0 = first ? p[(nrow + j) * ldp] : 0.f;
        // f(k, b_k) over this lane's negatives, k ascending
        auto each = [&](auto f) {
            if (first) f((int64_t)j, b0);
            if constexpr (W == 64) {
                if (live)
                    for (int64_t k = (int64_t)j + 64; k < K; k += 64) f(k, p[(nrow + k) * ldp]);
            }
        };
        float mx = -INFINITY;                                          // the largest negative and the lowest k that attains it
        int32_t arg = INT32_MAX;
        each([&](int64_t k, float b) { if (b > mx) { mx = b; arg = (int32_t)k; } });
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) {
            const float om = __shfl_xor(mx, o, 64);
            const int32_t oa = __shfl_xor(arg, o, 64);
            if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
        }
        float loss, ga;                                               // l_g and dl_g/da; gk(k, b) = dl_g/db_k
        if (kind == AMAR_GROUP_SOFTMAX) {
            const float M = fmaxf(a, mx);
            float s = 0.f;
            each([&](int64_t, float b) { s += expf((b - M) / hyper); });
            s = seg_sum<W>(s);
            const float S = expf((a - M) / hyper) + s;
            loss = a >= mx ? log1pf(s) : (M - a) / hyper + logf(S);
            ga = -(s / S) / hyper;
            each([&](int64_t k, float b) {
                dz[nrow + k] = (inv_g * ((expf((b - M) / hyper) / S) / hyper)) * (b * (1.f - b));
            });
        } else if (kind == AMAR_GROUP_HARDEST) {
            const float e = expf(mx - a);                             // in (-1, 1): probabilities, so exp cannot overflow
            const float gs = e / (1.f + e);                           // 1 - sigmoid(a - mx)
            loss = log1pf(e);
            ga = -gs;
            each([&](int64_t k, float b) { dz[nrow + k] = (int32_t)k == arg ? (inv_g * gs) * (b * (1.f - b)) : 0.f; });
        } else {
            const float d = hyper - a;
            float s = 0.f, c = 0.f;
            each([&](int64_t, float b) { const float v = d + b; s += fmaxf(v, 0.f); c += v > 0.f ? 1.f : 0.f; });
            s = seg_sum<W>(s);
            c = seg_sum<W>(c);                                        // (a count below 2^24: exact)
            loss = s / fk;
            ga = -(c / fk);
            each([&](int64_t k, float b) { dz[nrow + k] = d + b > 0.f ? (inv_g * (1.f / fk)) * (b * (1.f - b)) : 0.f; });
        }
        each([&](int64_t k, float) {
            terms[nrow + k] = 0.f;
            if (k > 0) { dz[row0 + k] = 0.f; terms[row0 + k] = 0.f; }  // the copies of the positive's pair
        });
        if (live && j == 0) {
            dz[row0] = (inv_g * ga) * (a * (1.f - a));
            terms[row0] = scale * loss;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && 2 * h < B) {
        dz[B - 1] = 0.f;
        terms[B - 1] = 0.f;
    }
}

template <int W>
int launch_group_loss(int32_t kind, float hyper, const float *p, int64_t ldp, float *dz, float *terms, int64_t B, int64_t h, int32_t K,
                      hipStream_t st) {
    const int64_t G = h / K, per_block = 4 * (64 / W);
    int64_t grid = (G + per_block - 1) / per_block;
    grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
    hipLaunchKernelGGL(group_loss_kernel<W>, dim3((unsigned)grid), dim3(256), 0, st, kind, hyper, p, ldp, dz, terms, B, h, K, G);
    return amar_check_launch();
}

__device__ __forceinline__ int32_t pick(uint32_t word, int32_t n) { return (int32_t)(((uint64_t)word * (uint32_t)n) >> 32); }

// ONE workgroup: every lane reads *step before the barrier, one lane advances it after, so the batch sees one step value.
__global__ __launch_bounds__(256) void bpr_sample_kernel(const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_ids,
                                                         const int32_t *__restrict__ neg_ptr, const int32_t *__restrict__ neg_ids,
                                                         int32_t n_users, uint32_t key0, uint32_t key1, uint64_t *step, int32_t advance,
                                                         int32_t h, int32_t *__restrict__ u, int32_t *__restrict__ items,
                                                         float *__restrict__ y) {
    const uint64_t s = *step;
    for (int32_t j = threadIdx.x; j < h; j += blockDim.x) {
        uint32_t c[4] = {(uint32_t)j, (uint32_t)s, (uint32_t)(s >> 32), 0u};
        philox4x32_10(c, key0, key1);
        const int32_t user = pick(c[0], n_users);
        const int32_t p0 = pos_ptr[user], n_pos = pos_ptr[user + 1] - p0;
        const int32_t q0 = neg_ptr[user], n_neg = neg_ptr[user + 1] - q0;
        u[2 * j] = user;                                               // users = repeat(batch_users, 2)
        u[2 * j + 1] = user;
        items[j] = pos_ids[p0 + pick(c[1], n_pos)];                    // items = [pos ; neg]
        items[h + j] = neg_ids[q0 + pick(c[2], n_neg)];
        if (y) { y[j] = 1.f; y[h + j] = 0.f; }
    }
    __syncthreads();
    if (advance && threadIdx.x == 0) *step = s + 1;
}

// Triples (user, pos, neg): draw j < h / K picks the user and its positive, triple t = j * K + k its k-th negative — the r-th item
// outside the user's ascending exclusion row, r uniform in [0, n_items - d).  With e_q the q-th excluded item (0-based in the item
// range), e_q - q counts the free items below e_q and never decreases, so m = #{q : e_q - q <= r} is one binary search and the
// r-th free item is r + m.  ONE workgroup, as above: every lane reads *step before the barrier, one lane advances it after.
__global__ __launch_bounds__(256) void bpr_sample_triplets_kernel(const int32_t *__restrict__ pos_ptr, const int32_t *__restrict__ pos_ids,
                                                                  const int32_t *__restrict__ excl_ptr, const int32_t *__restrict__ excl_ids,
                                                                  int32_t n_users, int32_t n_items, int32_t item_base, int32_t K, int32_t mode,
                                                                  uint32_t key0, uint32_t key1, uint64_t *step, int32_t advance, int32_t h,
                                                                  int32_t *__restrict__ u, int32_t *__restrict__ items, float *__restrict__ y) {
    const uint64_t s = *step;
    for (int32_t t = threadIdx.x; t < h; t += blockDim.x) {
        uint32_t c[4] = {(uint32_t)(t / K), (uint32_t)s, (uint32_t)(s >> 32), 0u};
        philox4x32_10(c, key0, key1);
        int32_t user, pos;
        if (mode == 0) {                                               // users uniform
            user = pick(c[0], n_users);
            const int32_t p0 = pos_ptr[user];
            pos = pos_ids[p0 + pick(c[1], pos_ptr[user + 1] - p0)];
        } else {                                                       // interactions uniform: the row that holds entry e
            const int32_t e = pick(c[0], pos_ptr[n_users]);
            int32_t lo = 0, hi = n_users - 1;                          // largest r with pos_ptr[r] <= e
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo + 1) / 2;
                if (pos_ptr[mid] <= e) lo = mid; else hi = mid - 1;
            }
            user = lo;
            pos = pos_ids[e];
        }
        uint32_t w[4] = {(uint32_t)t, (uint32_t)s, (uint32_t)(s >> 32), 1u};
        philox4x32_10(w, key0, key1);
        const int32_t x0 = excl_ptr[user], d = excl_ptr[user + 1] - x0;
        const int32_t r = pick(w[0], n_items - d);
        int32_t lo = 0, hi = d;                                        // m = #{q < d : e_q - q <= r}
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (excl_ids[x0 + mid] - item_base - mid <= r) lo = mid + 1; else hi = mid;
        }
        u[t] = user;
        u[h + t] = user;
        items[t] = pos;
        items[h + t] = item_base + r + lo;
        if (y) { y[t] = 1.f; y[h + t] = 0.f; }
    }
    __syncthreads();
    if (advance && threadIdx.x == 0) *step = s + 1;
}

}  // namespace

int amar_bpr_grad_f32(const float *p, int64_t ldp, float *dz, float *loss_terms, int64_t B, amar_stream_t stream) {
    if (B < 1 || !p || !dz || !loss_terms || ldp < 1) return AMAR_EINVAL;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t h = B / 2;
    if (h == 0) {                                                      // no pair: zero loss and gradient
        hipLaunchKernelGGL(bpr_grad_kernel, dim3(1), dim3(64), 0, st, p, ldp, dz, loss_terms, B, (int64_t)0);
        return amar_check_launch();
    }
    int64_t grid = (h + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(bpr_grad_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, ldp, dz, loss_terms, B, h);
    return amar_check_launch();
}

int amar_group_loss_grad_f32(int32_t kind, float hyper, const float *p, int64_t ldp, float *dz, float *loss_terms, int64_t B, int32_t K,
                             amar_stream_t stream) {
    if (B < 1 || !p || !dz || !loss_terms || ldp < 1 || K < 1) return AMAR_EINVAL;
    if (kind != AMAR_GROUP_SOFTMAX && kind != AMAR_GROUP_HARDEST && kind != AMAR_GROUP_MARGIN) return AMAR_EINVAL;
    if ((kind == AMAR_GROUP_SOFTMAX && !(hyper > 0.f)) || (kind == AMAR_GROUP_MARGIN && !(hyper >= 0.f))) return AMAR_EINVAL;
    const int64_t h = B / 2;
    if (h % K != 0) return AMAR_EINVAL;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (K > 32) return launch_group_loss<64>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
    if (K > 16) return launch_group_loss<32>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
    if (K > 8) return launch_group_loss<16>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
    if (K > 4) return launch_group_loss<8>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
    if (K > 2) return launch_group_loss<4>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
    if (K > 1) return launch_group_loss<2>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
    return launch_group_loss<1>(kind, hyper, p, ldp, dz, loss_terms, B, h, K, st);
}

int amar_bpr_sample_i32(const int32_t *pos_ptr, const int32_t *pos_ids, const int32_t *neg_ptr, const int32_t *neg_ids,
                        int32_t n_users, uint64_t seed, uint64_t *step, int32_t advance, int32_t h,
                        int32_t *u, int32_t *items, float *y, amar_stream_t stream) {
    if (n_users < 1 || h < 1 || !pos_ptr || !pos_ids || !neg_ptr || !neg_ids || !step || !u || !items) return AMAR_EINVAL;
    hipLaunchKernelGGL(bpr_sample_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), pos_ptr, pos_ids, neg_ptr, neg_ids,
                       n_users, (uint32_t)seed, (uint32_t)(seed >> 32), step, advance, h, u, items, y);
    return amar_check_launch();
}

int amar_bpr_sample_triplets_i32(const int32_t *pos_ptr, const int32_t *pos_ids, const int32_t *excl_ptr, const int32_t *excl_ids,
                                 int32_t n_users, int32_t n_items, int32_t item_base, int32_t n_negatives, int32_t mode, uint64_t seed,
                                 uint64_t *step, int32_t advance, int32_t h, int32_t *u, int32_t *items, float *y,
                                 amar_stream_t stream) {
    if (n_users < 1 || n_items < 1 || h < 1 || n_negatives < 1 || h % n_negatives != 0 || (mode != 0 && mode != 1) || !pos_ptr ||
        !pos_ids || !excl_ptr || !excl_ids || !step || !u || !items)
        return AMAR_EINVAL;
    hipLaunchKernelGGL(bpr_sample_triplets_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), pos_ptr, pos_ids, excl_ptr,
                       excl_ids, n_users, n_items, item_base, n_negatives, mode, (uint32_t)seed, (uint32_t)(seed >> 32), step, advance, h,
                       u, items, y);
    return amar_check_launch();
}

// Full-catalogue top-k: fused score-and-select over every (user, item) pair of the split scoring head (gfx950).
//
// With the classifier's first Dense layer folded into the towers (models/basic.py:_split_plan), a pair's score is
//     score(u, i) = rest( in_act( Tu[u] + Ti[i] ) )          rest = Dense stack ending in Dense(1, sigmoid)
// This file evaluates that for a block of users against every item and keeps each user's k best on chip: nothing of size
// |U| x |I| is written.  Decomposition:
//   * grid (user blocks of 16, item slices); 4 waves per workgroup, each owning 4 users of the block.
//   * per item tile: the workgroup stages TI rows of Ti in LDS once; every wave then walks the tile for each of its users with
//     that user's Tu row in registers.  The first product's B fragment (pair on the MFMA column, features 16t + 4g + r on rows,
//     the layout of chain_kernel in amar_chain.hip) is formed in registers as in_act(Tu[u] + Ti[i]): no per-pair gathers.
//   * the rest stack runs on v_mfma_f32_16x16x4_f32 with chain_kernel's loop order, fragment blob and dot stage, so a score is
//     bit-identical to what amar_chain_f32's generic kernel returns for the same pair (the pair stage of predict() for heads
//     whose widths it takes).
//   * selection: per user a threshold = the current k-th best (score, item); a pair beating it is checked against the user's
//     sorted exclusion list (a pointer walked forward tile by tile, binary search inside the remaining window) and appended to a
//     64-entry LDS candidate buffer; a full buffer (and the end of the slice) is merged into the sorted top-k list by rank
//     counting.  Expected inserts ~ k ln(|I| / k): per pair the selection is one compare.
//   * with several item slices each workgroup leaves its slice's top-k in a workspace and a second launch merges the slices
//     of a user in slice order (the order is a strict total order, so the result does not depend on the slicing).
// The result of a user depends on its own Tu row, Ti and the weights only: not on the other users of the block or the call.
#include "amar_common.h"
#include "amar_rank_select.h"
#include <stdlib.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RANK_MAX_LAYERS = 8;
constexpr int RANK_WAVES = 4, RANK_UPW = 4, RANK_UB = RANK_WAVES * RANK_UPW;     // users per wave, per workgroup
constexpr int RANK_TILE_BYTES = 32 * 1024;

struct RankArgs {
    const float *Tu; int64_t ldu; const float *Ti; int64_t ldi; int c1; int n_items;
    const int32_t *users; int64_t m;
    const int32_t *excl_ptr, *excl_items;
    const float *wpack; int wpack_floats;
    int in_act, n_layers;
    int kt[RANK_MAX_LAYERS], nt[RANK_MAX_LAYERS], act[RANK_MAX_LAYERS], w_off[RANK_MAX_LAYERS], b_off[RANK_MAX_LAYERS];
    int dot_off, dot_bias_off, dot_kt, dot_act;
    int k, tile_items, tile_stride, slice_items, n_slices;
    int32_t *out_items; float *out_scores;     // n_slices == 1: the result [m, k]; else the per-slice lists [m][n_slices][k]
};

__device__ __forceinline__ float rank_act(float v, int act) {       // chain_act of amar_chain.hip: the same expressions
    if (act == AMAR_ACT_RELU) return fmaxf(v, 0.f);
    if (act == AMAR_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
    return v;
}

template <int MAXT, int PT>
__global__ __launch_bounds__(256) void recommend_kernel(const RankArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *tile = lds + ((a.wpack_floats + 3) & ~3);
    float *list_s = tile + a.tile_items * a.tile_stride;
    int *list_i = reinterpret_cast<int *>(list_s + RANK_UB * RANK_LIST);
    float *cand_s = reinterpret_cast<float *>(list_i + RANK_UB * RANK_LIST);
    int *cand_i = reinterpret_cast<int *>(cand_s + RANK_UB * RANK_CAND);
    int *st_cnt = cand_i + RANK_UB * RANK_CAND;          // per user: candidates buffered, exclusion pointer, threshold
    int *st_ep = st_cnt + RANK_UB;
    float *st_ts = reinterpret_cast<float *>(st_ep + RANK_UB);
    int *st_ti = reinterpret_cast<int *>(st_ts + RANK_UB);

    for (int i = threadIdx.x * 4; i < a.wpack_floats; i += blockDim.x * 4)
        *reinterpret_cast<float4 *>(&w_lds[i]) = *reinterpret_cast<const float4 *>(a.wpack + i);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * RANK_UB;
    const int slice = blockIdx.y;
    const int s0 = slice * a.slice_items, s1 = min(a.n_items, s0 + a.slice_items);
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        list_s[slot * RANK_LIST + lane] = -INFINITY;
        list_i[slot * RANK_LIST + lane] = RANK_EMPTY;
        if (lane == 0) {
            const int64_t j = j0 + slot;
            int ep = 0;
            if (j < a.m && a.excl_ptr) {
                const int u = a.users ? a.users[j] : (int)j;
                ep = rank_lower_bound(a.excl_items, a.excl_ptr[u], a.excl_ptr[u + 1], s0);
            }
            st_cnt[slot] = 0; st_ep[slot] = ep; st_ts[slot] = -INFINITY; st_ti[slot] = RANK_EMPTY;
        }
    }
    const int KT0 = a.kt[0];
    const int f4_per_row = 4 * KT0;                              // float4s of a staged row (16 KT0 features, zero past c1)

    for (int t0 = s0; t0 < s1; t0 += a.tile_items) {
        const int rows = min(a.tile_items, s1 - t0);
        __syncthreads();                                         // the previous tile is no longer read
        for (int idx = threadIdx.x; idx < a.tile_items * f4_per_row; idx += blockDim.x) {
            const int r = idx / f4_per_row, f = 4 * (idx - r * f4_per_row);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && f < a.c1) v = *reinterpret_cast<const float4 *>(a.Ti + (int64_t)(t0 + r) * a.ldi + f);
            *reinterpret_cast<float4 *>(&tile[r * a.tile_stride + f]) = v;
        }
        __syncthreads();
        for (int uw = 0; uw < RANK_UPW; ++uw) {
            const int slot = wave * RANK_UPW + uw;
            const int64_t j = j0 + slot;
            if (j >= a.m) break;
            const int u = a.users ? a.users[j] : (int)j;
            f32x4 tu[MAXT];
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                const int f = 16 * t + 4 * g;
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                tu[t] = (t < KT0 && f < a.c1) ? *reinterpret_cast<const f32x4 *>(a.Tu + (int64_t)u * a.ldu + f) : zero;
            }
            int cnt = st_cnt[slot], ep = st_ep[slot];
            float ts = st_ts[slot];
            int ti = st_ti[slot];
            const int ee = a.excl_ptr ? a.excl_ptr[u + 1] : 0;
            float *ls = list_s + slot * RANK_LIST, *cs = cand_s + slot * RANK_CAND;
            int *li = list_i + slot * RANK_LIST, *ci = cand_i + slot * RANK_CAND;

            for (int grp = 0; grp < rows; grp += 16 * PT) {
                f32x4 x[MAXT][PT];
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) {
                    const float *row = tile + (grp + 16 * pt + col) * a.tile_stride;
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) {
                        const int f = 16 * t + 4 * g;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (t < KT0 && f < a.c1) {
                            v = tu[t] + *reinterpret_cast<const f32x4 *>(row + f);
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = rank_act(v[r], a.in_act);
                        }
                        x[t][pt] = v;
                    }
                }
                for (int l = 0; l < a.n_layers; ++l) {
                    const int KT = a.kt[l], NT = a.nt[l];
                    const float *wl = w_lds + a.w_off[l];
                    const float *bl = w_lds + a.b_off[l];
                    f32x4 y[MAXT][PT];
#pragma unroll
                    for (int mm = 0; mm < MAXT; ++mm) {
                        if (mm < NT) {
                            const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bl + 16 * mm + 4 * g);
#pragma unroll
                            for (int pt = 0; pt < PT; ++pt) y[mm][pt] = b4;
#pragma unroll
                            for (int t = 0; t < MAXT; ++t) {
                                if (t < KT) {
                                    const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wl + ((mm * KT + t) * 64 + lane) * 4);
#pragma unroll
                                    for (int r = 0; r < 4; ++r)
#pragma unroll
                                        for (int pt = 0; pt < PT; ++pt)
                                            y[mm][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[r], x[t][pt][r], y[mm][pt], 0, 0, 0);
                                }
                            }
                        }
                    }
                    const int act = a.act[l];
#pragma unroll
                    for (int mm = 0; mm < MAXT; ++mm)
#pragma unroll
                        for (int pt = 0; pt < PT; ++pt) {
                            f32x4 v = {0.f, 0.f, 0.f, 0.f};
                            if (mm < NT) {
                                v = y[mm][pt];
#pragma unroll
                                for (int r = 0; r < 4; ++r) v[r] = rank_act(v[r], act);
                            }
                            x[mm][pt] = v;
                        }
                }
                // the 1-unit layer: chain_kernel's dot, then lane group g keeps pair tile g
                const float *wd = w_lds + a.dot_off;
                float sel = 0.f;
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) {
                    float s = 0.f;
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) {
                        if (t < a.dot_kt) {
                            const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wd + 16 * t + 4 * g);
#pragma unroll
                            for (int r = 0; r < 4; ++r) s = fmaf(x[t][pt][r], w4[r], s);
                        }
                    }
                    s += __shfl_xor(s, 16, 64);
                    s += __shfl_xor(s, 32, 64);
                    sel = g == pt ? s : sel;
                }
                const float z = rank_act(sel + w_lds[a.dot_bias_off], a.dot_act);
                const int item = t0 + grp + 16 * g + col;
                bool pred = g < PT && grp + 16 * g + col < rows && rank_better(z, item, ts, ti);
                if (__ballot(pred) == 0) continue;
                if (pred && ep < ee) {                               // training item of this user?
                    const int pos = rank_lower_bound(a.excl_items, ep, ee, item);
                    pred = !(pos < ee && a.excl_items[pos] == item);
                }
                const uint64_t mask = __ballot(pred);
                if (mask == 0) continue;
                const int n = __popcll(mask);
                if (cnt + n > RANK_CAND) {
                    rank_merge(ls, li, cs, ci, cnt, a.k, lane);
                    cnt = 0;
                    ts = ls[a.k - 1]; ti = li[a.k - 1];
                    pred = pred && rank_better(z, item, ts, ti);
                }
                const uint64_t mask2 = __ballot(pred);
                if (pred) {
                    const int pos = cnt + __popcll(mask2 & ((1ull << lane) - 1ull));
                    cs[pos] = z; ci[pos] = item;
                }
                cnt += __popcll(mask2);
            }
            // the exclusion pointer moves past this tile
            if (a.excl_ptr && ep < ee) ep = rank_lower_bound(a.excl_items, ep, ee, t0 + rows);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) { st_cnt[slot] = cnt; st_ep[slot] = ep; st_ts[slot] = ts; st_ti[slot] = ti; }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    // slice done: last merge, then the list goes out (final result or this slice's partial list)
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        if (j >= a.m) break;
        float *ls = list_s + slot * RANK_LIST;
        int *li = list_i + slot * RANK_LIST;
        const int cnt = st_cnt[slot];
        if (cnt > 0) rank_merge(ls, li, cand_s + slot * RANK_CAND, cand_i + slot * RANK_CAND, cnt, a.k, lane);
        if (lane < a.k) {
            const float s = ls[lane];
            const int i = li[lane];
            if (a.n_slices == 1) {
                a.out_items[j * a.k + lane] = i == RANK_EMPTY ? -1 : i;
                a.out_scores[j * a.k + lane] = i == RANK_EMPTY ? -INFINITY : s;
            } else {
                const int64_t o = (j * a.n_slices + slice) * a.k + lane;
                a.out_items[o] = i;
                a.out_scores[o] = s;
            }
        }
    }
}

inline int tiles16(int n) { return (n + 15) / 16; }

// Launch geometry of a rest stack: tile budget MAXT (widest layer / 16, rounded up to a power of two), pair tiles per wave PT.
struct RankShape { int maxt, pt, tile_items, tile_stride; };

int rank_shape(const int32_t *dims, int32_t n_layers, RankShape &s) {
    int maxw = 0;
    for (int l = 0; l < n_layers; ++l) maxw = dims[l] > maxw ? dims[l] : maxw;   // dims[n_layers] == 1 (the dot)
    if (maxw > 128) return AMAR_EUNSUPPORTED;
    s.maxt = maxw <= 16 ? 1 : (maxw <= 32 ? 2 : (maxw <= 64 ? 4 : 8));
    s.pt = s.maxt <= 2 ? 4 : (s.maxt == 4 ? 2 : 1);
    s.tile_stride = 16 * tiles16(dims[0]) + 4;                     // +4 floats: neighbouring items start on different banks
    const int group = 16 * s.pt;
    int ti = RANK_TILE_BYTES / (4 * s.tile_stride);
    ti = ti > 256 ? 256 : ti;
    ti = (ti / group) * group;
    s.tile_items = ti < group ? group : ti;
    return AMAR_OK;
}

}  // namespace

extern "C" {

int32_t amar_recommend_slices(int64_t m, int32_t n_items, const int32_t *dims, int32_t n_layers, int32_t n_slices) {
    if (m < 0 || n_items < 0 || !dims || n_layers < 2 || n_layers > RANK_MAX_LAYERS + 1) return AMAR_EINVAL;
    RankShape s;
    const int rc = rank_shape(dims, n_layers, s);
    if (rc != AMAR_OK) return rc;
    const int64_t tiles = (n_items + s.tile_items - 1) / s.tile_items;
    const int64_t blocks = (m + RANK_UB - 1) / RANK_UB;
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
    // slices cover whole tiles: the count actually launched
    const int64_t per = ((tiles + want - 1) / want) * s.tile_items;
    const int64_t eff = per > 0 ? (n_items + per - 1) / per : 1;
    return (int32_t)(eff > 0 ? eff : 1);
}

int amar_recommend_f32(const float *Tu, int64_t ldu, int32_t n_users, const float *Ti, int64_t ldi, int32_t n_items, int32_t c1,
                       const float *wpack, const int32_t *dims, const int32_t *acts, int32_t n_layers, int32_t in_act,
                       const int32_t *users, int64_t m, const int32_t *excl_ptr, const int32_t *excl_items,
                       int32_t k, int32_t n_slices, int32_t *workspace_items, float *workspace_scores,
                       int32_t *out_items, float *out_scores, amar_stream_t stream) {
    if (!Tu || !Ti || !wpack || !dims || !acts || m < 0 || n_users < 0 || n_items < 0 || k < 1) return AMAR_EINVAL;
    if (k > 64) return AMAR_EUNSUPPORTED;
    if (!users && m != n_users) return AMAR_EINVAL;
    if (excl_ptr && !excl_items) return AMAR_EINVAL;
    if (c1 < 4 || (c1 & 3) || (ldu & 3) || (ldi & 3) || ldu < c1 || ldi < c1 || !amar_aligned16(Tu) || !amar_aligned16(Ti) ||
        !amar_aligned16(wpack))
        return AMAR_EINVAL;
    if (c1 > 128) return AMAR_EUNSUPPORTED;
    if (in_act != AMAR_ACT_NONE && in_act != AMAR_ACT_RELU && in_act != AMAR_ACT_SIGMOID) return AMAR_EINVAL;
    // the rest stack: >= 1 MFMA layer, then Dense(1) as the dot stage
    if (n_layers < 2 || n_layers > RANK_MAX_LAYERS + 1 || dims[0] != c1 || dims[n_layers] != 1) return AMAR_EUNSUPPORTED;
    RankArgs a{};
    int off = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int K = dims[l], N = dims[l + 1], act = acts[l];
        if (K < 1 || N < 1 || (act != AMAR_ACT_NONE && act != AMAR_ACT_RELU && act != AMAR_ACT_SIGMOID)) return AMAR_EINVAL;
        if (l == n_layers - 1) {
            a.dot_off = off; a.dot_kt = tiles16(K); a.dot_act = act;
            off += 16 * tiles16(K);
            a.dot_bias_off = off;
            off += 4;
        } else {
            if (N == 1) return AMAR_EUNSUPPORTED;
            a.kt[l] = tiles16(K); a.nt[l] = tiles16(N); a.act[l] = act;
            a.w_off[l] = off;
            off += tiles16(N) * tiles16(K) * 256;
            a.b_off[l] = off;
            off += 16 * tiles16(N);
        }
    }
    a.n_layers = n_layers - 1;
    a.wpack_floats = off;
    RankShape sh;
    const int rc = rank_shape(dims, n_layers, sh);
    if (rc != AMAR_OK) return rc;
    const int32_t slices = amar_recommend_slices(m, n_items, dims, n_layers, n_slices);
    if (slices < 1) return slices < 0 ? slices : AMAR_EINVAL;
    if (n_slices > 0 && slices != n_slices) return AMAR_EINVAL;       // the caller sizes the workspace from amar_recommend_slices
    if (slices > 1 && (!workspace_items || !workspace_scores)) return AMAR_EINVAL;
    if (m == 0) return AMAR_OK;
    if (!out_items || !out_scores) return AMAR_EINVAL;
    const int64_t tiles = (n_items + sh.tile_items - 1) / sh.tile_items;
    const int64_t per_tiles = (tiles + slices - 1) / slices;
    a.Tu = Tu; a.ldu = ldu; a.Ti = Ti; a.ldi = ldi; a.c1 = c1; a.n_items = n_items;
    a.users = users; a.m = m; a.excl_ptr = excl_ptr; a.excl_items = excl_items;
    a.wpack = wpack; a.in_act = in_act; a.k = k;
    a.tile_items = sh.tile_items; a.tile_stride = sh.tile_stride;
    a.slice_items = (int)(per_tiles * sh.tile_items > 0 ? per_tiles * sh.tile_items : sh.tile_items);
    a.n_slices = slices;
    a.out_items = slices > 1 ? workspace_items : out_items;
    a.out_scores = slices > 1 ? workspace_scores : out_scores;
    const size_t lds_bytes = (size_t)((a.wpack_floats + 3) & ~3) * 4 + (size_t)sh.tile_items * sh.tile_stride * 4 +
                             (size_t)RANK_UB * (2 * RANK_LIST + 2 * RANK_CAND + 4) * 4;
    if (lds_bytes > 160 * 1024) return AMAR_EUNSUPPORTED;
    const int64_t blocks = (m + RANK_UB - 1) / RANK_UB;
    if (blocks >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)slices), block(256);
    static bool done[4][AMAR_MAX_DEVICES];
#define AMAR_RANK_LAUNCH(MT, PTT, D)                                                                                    \
    do {                                                                                                                \
        auto kern = recommend_kernel<MT, PTT>;                                                                          \
        if (lds_bytes > 64 * 1024) {                                                                                    \
            const int e = amar_allow_lds(reinterpret_cast<const void *>(kern), 160 * 1024, done[D]);                   \
            if (e != AMAR_OK) return e;                                                                                 \
        }                                                                                                               \
        hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, a);                                                        \
    } while (0)
    switch (sh.maxt) {
    case 1: AMAR_RANK_LAUNCH(1, 4, 0); break;
    case 2: AMAR_RANK_LAUNCH(2, 4, 1); break;
    case 4: AMAR_RANK_LAUNCH(4, 2, 2); break;
    default: AMAR_RANK_LAUNCH(8, 1, 3); break;
    }
#undef AMAR_RANK_LAUNCH
    const int e = amar_check_launch();
    if (e != AMAR_OK || slices == 1) return e;
    hipLaunchKernelGGL(recommend_merge_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, workspace_items, workspace_scores, m, slices,
                       k, out_items, out_scores);
    return amar_check_launch();
}

}  // extern "C"

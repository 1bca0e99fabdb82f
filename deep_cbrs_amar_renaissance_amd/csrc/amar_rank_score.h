// What the fused rankers of the split head share besides the selector of amar_rank_select.h:
//   * RankArgs, the kernels' argument block, and the constants of their decomposition;
//   * device helpers: the packed rest stack and an item tile go to LDS (rank_stage_weights, rank_stage_tile), a user's Tu row
//     becomes MFMA fragments (rank_load_user); a wave gathers listed Ti rows into a tile-shaped buffer of its own (rank_gather,
//     rank_wave_sync: amar_rank_of.hip's targets and excluded rows, amar_rank_lists.hip's candidates);
//   * the score stage itself is amar_rank_score.inc, a fragment of a kernel body (one text, the same bits per pair):
//     rank_topk_kernel includes it, and amar_rank_of.hip wraps it in a function of its own;
//   * rank_topk_kernel<MAXT, PT, V>, the one body of three of the four top-k kernels, and RankVariant, what a variant V says by default.
//     The variants: RankPlain (amar_rank.hip, amar_recommend_f32: one user per selector), RankAmong (amar_rank_among.hip: the
//     same over a candidate list), RankGroup (amar_group.hip: a group of users per selector).  amar_rank_after.hip (the same
//     from a cursor) still has its own copy of the walk, and amar_rank_of.hip counts instead of selecting: its kernel has its
//     own walk; both call the helpers and include the fragment;
//   * host: the argument checks the entry points share (rank_check_tables), the walk over the packed stack (rank_pack_args), the
//     launch geometry of a stack (rank_shape), the LDS a launch needs (rank_lds_bytes, rank_of_lds_bytes, rank_lists_lds_bytes),
//     rank_route — the one
//     function the launchers and the query amar_rank_route take all of that and the capacity refusal from — and the launch
//     path itself: rank_prepare (tables, route, the argument fields every ranker sets alike), rank_launch_form (the MAXT / PT
//     dispatch over a kernel's four forms), rank_topk (everything the top-k launchers do after their own leading checks)
//     and rank_slices_tile (what the *_slices queries check before they count).
#pragma once
#include "amar_common.h"
#include "amar_rank_select.h"
#include <limits.h>
#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RANK_MAX_LAYERS = 8;
constexpr int RANK_WAVES = 4, RANK_UPW = 4, RANK_UB = RANK_WAVES * RANK_UPW;     // selectors per wave, per workgroup
constexpr int RANK_TILE_BYTES = 32 * 1024;

struct RankArgs {
    const float *Tu; int64_t ldu; const float *Ti; int64_t ldi; int c1; int n_items;
    const int32_t *users; int64_t m;
    const int32_t *excl_ptr, *excl_items;
    const float *wpack; int wpack_floats;
    int in_act, n_layers;
    int kt[RANK_MAX_LAYERS], nt[RANK_MAX_LAYERS], act[RANK_MAX_LAYERS], w_off[RANK_MAX_LAYERS], b_off[RANK_MAX_LAYERS];
    int dot_off, dot_bias_off, dot_kt, dot_act;
    int tile_items, tile_stride, slice_items;
    RankOut out;
};

// The packed rest stack goes to LDS once per workgroup.
__device__ __forceinline__ void rank_stage_weights(const RankArgs &a, float *w_lds) {
    for (int i = threadIdx.x * 4; i < a.wpack_floats; i += blockDim.x * 4)
        *reinterpret_cast<float4 *>(&w_lds[i]) = *reinterpret_cast<const float4 *>(a.wpack + i);
}

// Rows t0 .. t0 + rows - 1 of Ti go to the tile (16 KT0 features a row, zero past c1 and past `rows`); the caller's barriers
// stand on either side.  LISTED: the rows are cand[t0 .. t0 + rows - 1] instead, and tile_rows keeps the item row of every tile
// row (RANK_EMPTY past `rows`; such an entry is never used as a row of Ti).
template <bool LISTED = false>
__device__ __forceinline__ void rank_stage_tile(const RankArgs &a, float *tile, int t0, int rows, const int32_t *cand = nullptr,
                                                int *tile_rows = nullptr) {
    const int f4_per_row = 4 * a.kt[0];
    for (int idx = threadIdx.x; idx < a.tile_items * f4_per_row; idx += blockDim.x) {
        const int r = idx / f4_per_row, f = 4 * (idx - r * f4_per_row);
        int row = t0 + r;
        if constexpr (LISTED) row = r < rows ? cand[t0 + r] : RANK_EMPTY;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows && f < a.c1) v = *reinterpret_cast<const float4 *>(a.Ti + (int64_t)row * a.ldi + f);
        *reinterpret_cast<float4 *>(&tile[r * a.tile_stride + f]) = v;
        if constexpr (LISTED)
            if (f == 0) tile_rows[r] = row;
    }
}

// Row u of Tu as this lane's fragments: features 16t + 4g .. + 3 of k-step t.
template <int MAXT>
__device__ __forceinline__ void rank_load_user(const RankArgs &a, int u, int g, f32x4 (&tu)[MAXT]) {
    const int KT0 = a.kt[0];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int f = 16 * t + 4 * g;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        tu[t] = (t < KT0 && f < a.c1) ? *reinterpret_cast<const f32x4 *>(a.Tu + (int64_t)u * a.ldu + f) : zero;
    }
}

// What orders a wave's own LDS writes before its own LDS reads of other lanes' words: no other wave is waited for.
__device__ __forceinline__ void rank_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Rows ids[0 .. count) of Ti go to the wave's buffer (16 PT rows of 16 KT0 features, zero past c1, past `count` and for an id
// outside the table); the caller's wave syncs stand on either side.
template <int PT>
__device__ __forceinline__ void rank_gather(const RankArgs &a, float *buf, const int32_t *ids, int count, int lane) {
    const int f4_per_row = 4 * a.kt[0];
    for (int idx = lane; idx < 16 * PT * f4_per_row; idx += AMAR_WAVE) {
        const int r = idx / f4_per_row, f = 4 * (idx - r * f4_per_row);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < count && f < a.c1) {
            const int it = ids[r];
            if ((unsigned)it < (unsigned)a.n_items) v = *reinterpret_cast<const float4 *>(a.Ti + (int64_t)it * a.ldi + f);
        }
        *reinterpret_cast<float4 *>(&buf[r * a.tile_stride + f]) = v;
    }
}

// ---- the top-k walk -----------------------------------------------------------------------------------------------------------
// What a variant V tells rank_topk_kernel, all of it resolved at compile time; RankVariant<Args> is amar_recommend_f32's answer
// and the base the others change one thing of:
//   * Args: the kernel's argument block, RankArgs or a struct whose first member r is one;
//   * LISTED: the rows of a tile are va.cand_items[t0 + r], positions t0 + r < va.n_cand (false: the rows t0 + r of Ti);
//   * excl_row(a, j): the row of the exclusion CSR that belongs to selector row j;
//   * Sel<MAXT>: what a wave holds for one selector row while it walks a tile.  begin() loads it (false: the row is skipped,
//     its list stays empty): the user's Tu row `tu`, or — MEMBERS — the range [mb, me) of a.users the row folds over and its
//     length n.  admit(va, z, item, low) is the variant's own condition beside "the row is inside the tile";
//   * MEMBERS only: fold(va, first, z, acc, low) takes one member's score into the aggregate and the running minimum,
//     close(va, acc, n) turns the aggregate into what the selector is offered.
// The score itself is amar_rank_score.inc, the fragment the body includes: one text, the same bits per pair.
template <class A>
struct RankVariant {
    typedef A Args;
    static constexpr bool LISTED = false, MEMBERS = false;
    static __device__ __forceinline__ int64_t excl_row(const RankArgs &a, int64_t j) { return a.users ? a.users[j] : (int)j; }

    template <int MAXT>
    struct Sel {                                 // one user (row u of Tu: excl_row's), scored once, nothing to add
        f32x4 tu[MAXT];
        __device__ __forceinline__ bool begin(const RankArgs &a, const A &, int64_t, int64_t u, int g) {
            rank_load_user<MAXT>(a, (int)u, g, tu);
            return true;
        }
        __device__ __forceinline__ bool admit(const A &, float, int, float) const { return true; }
    };
};

// The RankArgs of a kernel's argument block: the block itself, or its first member `r`.
template <class Args>
__host__ __device__ inline auto &rank_args_of(Args &args) {
    if constexpr (std::is_same_v<std::remove_const_t<Args>, RankArgs>) return args;
    else return args.r;
}

// The one body of amar_recommend_f32, amar_recommend_among_f32 and amar_recommend_group_f32:
//   * grid (blocks of RANK_UB selector rows, slices of the tile loop's rows); 4 waves per workgroup, each owning RANK_UPW
//     selector rows of the block, one RankSlot each;
//   * LDS: the packed stack, one item tile, the selectors and — LISTED only, behind everything else, so that the other offsets
//     are every variant's — the item row of every tile row (rank_lds_bytes, rank_among_lds_bytes);
//   * per tile: the workgroup stages it once between two barriers; every wave then walks it for each of its selector rows, 16 PT
//     rows a step: the score stage (MEMBERS: once per member, folded), the selector's offer; then the exclusion pointer moves to the next tile's first row;
//   * with several slices each workgroup leaves its slice's top-k in a workspace (RankSlot::finish) for rank_merge_slices.
template <int MAXT, int PT, class V>
__global__ __launch_bounds__(256) void rank_topk_kernel(const typename V::Args va) {
    const RankArgs &a = rank_args_of(va);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w_lds = lds;
    float *tile = lds + ((a.wpack_floats + 3) & ~3);
    float *select = tile + a.tile_items * a.tile_stride;         // RANK_UB selector slots (amar_rank_select.h)
    int *tile_rows = nullptr;                                    // LISTED: the item row of every tile row
    if constexpr (V::LISTED) tile_rows = reinterpret_cast<int *>(select + rank_select_state_floats(RANK_UB));

    rank_stage_weights(a, w_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * RANK_UB;
    const int slice = blockIdx.y;
    int n_rows = a.n_items;
    if constexpr (V::LISTED) n_rows = va.n_cand;
    const int s0 = slice * a.slice_items, s1 = min(n_rows, s0 + a.slice_items);
    int first_row = s0;                                          // where the exclusion walk starts
    if constexpr (V::LISTED) first_row = s0 < n_rows ? va.cand_items[s0] : 0;
    const int KT0 = a.kt[0];
    for (int uw = 0; uw < RANK_UPW; ++uw) {
        const int slot = wave * RANK_UPW + uw;
        const int64_t j = j0 + slot;
        int eb = 0, ee = 0;                                      // the selector row's excluded items
        if (lane == 0 && j < a.m && a.excl_ptr) {
            const int64_t e = V::excl_row(a, j);
            eb = a.excl_ptr[e]; ee = a.excl_ptr[e + 1];
        }
        RankSlot<RANK_UB>(select, slot).init(lane, a.excl_items, eb, ee, first_row);
    }

    for (int t0 = s0; t0 < s1; t0 += a.tile_items) {
        const int rows = min(a.tile_items, s1 - t0);
        int next_row = t0 + rows;                                // the row the next tile starts at (LISTED: INT_MAX at the end)
        if constexpr (V::LISTED) next_row = t0 + rows < n_rows ? va.cand_items[t0 + rows] : INT_MAX;
        __syncthreads();                                         // the previous tile is no longer read
        if constexpr (V::LISTED) rank_stage_tile<true>(a, tile, t0, rows, va.cand_items, tile_rows);
        else rank_stage_tile(a, tile, t0, rows);
        __syncthreads();
        for (int uw = 0; uw < RANK_UPW; ++uw) {
            const int slot = wave * RANK_UPW + uw;
            const int64_t j = j0 + slot;
            if (j >= a.m) break;
            const int64_t e = V::excl_row(a, j);
            typename V::template Sel<MAXT> cur;
            if (!cur.begin(a, va, j, e, g)) continue;
            RankSlot<RANK_UB> top(select, slot);
            top.load();
            const int ee = a.excl_ptr ? a.excl_ptr[e + 1] : 0;

            for (int grp = 0; grp < rows; grp += 16 * PT) {
                float offered, low = 0.f;                        // MEMBERS: the smallest member score of the step
                if constexpr (V::MEMBERS) {                      // the members' scores, folded in member order
                    float acc = 0.f;
                    for (int t = cur.mb; t < cur.me; ++t) {
                        f32x4 tu[MAXT];
                        rank_load_user<MAXT>(a, a.users[t], g, tu);
#include "amar_rank_score.inc"
                        V::fold(va, t == cur.mb, z, acc, low);
                    }
                    offered = V::close(va, acc, cur.n);
                } else {
                    const f32x4 (&tu)[MAXT] = cur.tu;
#include "amar_rank_score.inc"
                    offered = z;
                }
                const bool in_range = g < PT && grp + 16 * g + col < rows;
                int item = t0 + grp + 16 * g + col;
                if constexpr (V::LISTED) item = in_range ? tile_rows[grp + 16 * g + col] : RANK_EMPTY;
                top.offer(offered, item, in_range && cur.admit(va, offered, item, low), a.excl_items, ee, a.out.k, lane);
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

// ---- host side --------------------------------------------------------------------------------------------------------------
inline int tiles16(int n) { return (n + 15) / 16; }

// Launch geometry of a rest stack: tile budget MAXT (widest layer / 16, rounded up to a power of two), pair tiles per wave PT.
struct RankShape { int maxt, pt, tile_items, tile_stride; };

inline int rank_shape(const int32_t *dims, int32_t n_layers, RankShape &s) {
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

// The tables, the input activation and the outline of the rest stack (>= 1 MFMA layer, then Dense(1) as the dot stage).
inline int rank_check_tables(const float *Tu, int64_t ldu, const float *Ti, int64_t ldi, int32_t c1, const float *wpack,
                             const int32_t *dims, int32_t n_layers, int32_t in_act) {
    if (c1 < 4 || (c1 & 3) || (ldu & 3) || (ldi & 3) || ldu < c1 || ldi < c1 || !amar_aligned16(Tu) || !amar_aligned16(Ti) ||
        !amar_aligned16(wpack))
        return AMAR_EINVAL;
    if (c1 > 128) return AMAR_EUNSUPPORTED;
    if (in_act != AMAR_ACT_NONE && in_act != AMAR_ACT_RELU && in_act != AMAR_ACT_SIGMOID) return AMAR_EINVAL;
    if (n_layers < 2 || n_layers > RANK_MAX_LAYERS + 1 || dims[0] != c1 || dims[n_layers] != 1) return AMAR_EUNSUPPORTED;
    return AMAR_OK;
}

// Where every layer of the blob packed by amar_chain_pack_f32 sits: a's layer fields, n_layers (the MFMA layers) and wpack_floats.
inline int rank_pack_args(const int32_t *dims, const int32_t *acts, int32_t n_layers, RankArgs &a) {
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
    return AMAR_OK;
}

// Dynamic LDS of a launch: the stack, one item tile, RANK_UB selectors.
inline size_t rank_lds_bytes(const RankArgs &a, const RankShape &sh) {
    return (size_t)((a.wpack_floats + 3) & ~3) * 4 + (size_t)sh.tile_items * sh.tile_stride * 4 +
           (size_t)rank_select_state_floats(RANK_UB) * 4;
}

// amar_rank_among.hip: the same, and behind it the item row of every tile row (rank_topk_kernel's tile_rows, LISTED).
inline size_t rank_among_lds_bytes(const RankArgs &a, const RankShape &sh) { return rank_lds_bytes(a, sh) + (size_t)sh.tile_items * 4; }

// amar_rank_of.hip's share of the LDS: per entry RANK_OF_WORDS words of sorted targets and counters (its RankOfSlot), per wave a
// gather buffer of one step's rows; rank_of_kernel's carve-up reads the same two numbers.
constexpr int RANK_OF_WORDS = 6 * AMAR_RANK_OF_MAX_TARGETS + 2;
inline int rank_of_gather_floats(const RankShape &sh) { return 16 * sh.pt * sh.tile_stride; }
inline size_t rank_of_lds_bytes(const RankArgs &a, const RankShape &sh) {
    return (size_t)((a.wpack_floats + 3) & ~3) * 4 + (size_t)sh.tile_items * sh.tile_stride * 4 +
           (size_t)RANK_WAVES * rank_of_gather_floats(sh) * 4 + (size_t)RANK_UB * RANK_OF_WORDS * 4;
}

// amar_rank_lists.hip: the stack, a gather buffer per wave and one selector per wave; no item tile.
inline size_t rank_lists_lds_bytes(const RankArgs &a, const RankShape &sh) {
    return (size_t)((a.wpack_floats + 3) & ~3) * 4 + (size_t)RANK_WAVES * rank_of_gather_floats(sh) * 4 +
           (size_t)rank_select_state_floats(RANK_WAVES) * 4;
}

constexpr size_t RANK_LDS_LIMIT = 160 * 1024, RANK_LDS_PLAIN = 64 * 1024;

// The kinds amar_rank_route answers for (include/amar_hip.h; 3 is none of them).
inline bool rank_kind_known(int kind) {
    return kind == AMAR_RANK_RECOMMEND || kind == AMAR_RANK_GROUP || kind == AMAR_RANK_RANK_OF || kind == AMAR_RANK_AMONG ||
           kind == AMAR_RANK_LISTS;
}

// The one decision about a rest stack that amar_recommend_f32, amar_recommend_group_f32, amar_rank_of_f32, amar_recommend_among_f32,
// amar_recommend_lists_f32 and the query amar_rank_route share: where its layers sit in the packed blob (a's layer fields, rank_pack_args), the launch geometry (sh,
// rank_shape; a.tile_items / a.tile_stride), the LDS the kind's kernel asks for and whether that fits.  The launchers refuse on
// !r.fits, size the launch by r.lds_bytes and dispatch on r.maxt, so the query cannot say anything else.  No HIP call.
// acts == NULL (the query): every layer counts as linear, which the layout does not depend on.
inline int rank_route(int kind, const int32_t *dims, const int32_t *acts, int32_t n_layers, RankArgs &a, RankShape &sh,
                      amar_rank_route_info &r) {
    r = amar_rank_route_info{};
    if (!rank_kind_known(kind)) return AMAR_EINVAL;
    int32_t linear[RANK_MAX_LAYERS + 1] = {};
    int rc = rank_pack_args(dims, acts ? acts : linear, n_layers, a);
    if (rc != AMAR_OK) return rc;
    rc = rank_shape(dims, n_layers, sh);
    if (rc != AMAR_OK) return rc;
    a.tile_items = sh.tile_items; a.tile_stride = sh.tile_stride;
    const size_t bytes = kind == AMAR_RANK_RANK_OF ? rank_of_lds_bytes(a, sh)
                         : (kind == AMAR_RANK_AMONG ? rank_among_lds_bytes(a, sh)
                            : (kind == AMAR_RANK_LISTS ? rank_lists_lds_bytes(a, sh) : rank_lds_bytes(a, sh)));
    r.maxt = sh.maxt; r.pt = sh.pt; r.tile_items = sh.tile_items; r.tile_stride = sh.tile_stride;
    r.wpack_floats = a.wpack_floats;
    r.lds_bytes = (int64_t)bytes;
    r.fits = bytes <= RANK_LDS_LIMIT ? 1 : 0;
    r.large_lds = bytes > RANK_LDS_PLAIN ? 1 : 0;
    return AMAR_OK;
}

// ---- the launch path ------------------------------------------------------------------------------------------------------------
// The head arguments the four entry points take alike (`users`: the user row of a selector; amar_group.hip: the members).
struct RankHead {
    const float *Tu; int64_t ldu; const float *Ti; int64_t ldi; int32_t n_items, c1;
    const float *wpack; const int32_t *dims, *acts; int32_t n_layers, in_act;
    const int32_t *users, *excl_ptr, *excl_items;
};

// The first half of every launcher once its own leading checks have passed: the table check, the route, and the fields of `a`
// that all four set alike (`m`: the selector rows).  slice_items and out stay with the caller.
inline int rank_prepare(int kind, const RankHead &h, int64_t m, RankArgs &a, RankShape &sh, amar_rank_route_info &route) {
    int rc = rank_check_tables(h.Tu, h.ldu, h.Ti, h.ldi, h.c1, h.wpack, h.dims, h.n_layers, h.in_act);
    if (rc != AMAR_OK) return rc;
    rc = rank_route(kind, h.dims, h.acts, h.n_layers, a, sh, route);
    if (rc != AMAR_OK) return rc;
    a.Tu = h.Tu; a.ldu = h.ldu; a.Ti = h.Ti; a.ldi = h.ldi; a.c1 = h.c1; a.n_items = h.n_items;
    a.users = h.users; a.m = m; a.excl_ptr = h.excl_ptr; a.excl_items = h.excl_items;
    a.wpack = h.wpack; a.in_act = h.in_act;
    return AMAR_OK;
}

// The four instantiated forms of a ranking kernel, KERN<MAXT, PT> = <1, 4> <2, 4> <4, 2> <8, 1> in this order, and which of them
// has been allowed the large LDS on which device.  One static object per call site (AMAR_RANK_FORMS names the instantiations).
template <class Args>
struct RankForms {
    void (*kern[4])(Args);
    bool done[4][AMAR_MAX_DEVICES];
};
#define AMAR_RANK_FORMS(KERN) {{KERN<1, 4>, KERN<2, 4>, KERN<4, 2>, KERN<8, 1>}, {}}
#define AMAR_RANK_TOPK_FORMS(V) \
    {{rank_topk_kernel<1, 4, V>, rank_topk_kernel<2, 4, V>, rank_topk_kernel<4, 2, V>, rank_topk_kernel<8, 1, V>}, {}}

// Launches the form of the stack's shape (route.maxt) on 256 threads, allowing it the large LDS where the launch needs more than
// 64 KB (once per device and form), and checks the launch.
template <class Args>
inline int rank_launch_form(RankForms<Args> &forms, const amar_rank_route_info &route, dim3 grid, hipStream_t st, const Args &args) {
    const int f = route.maxt == 1 ? 0 : (route.maxt == 2 ? 1 : (route.maxt == 4 ? 2 : 3));
    const size_t lds_bytes = (size_t)route.lds_bytes;
    if (lds_bytes > RANK_LDS_PLAIN) {
        const int e = amar_allow_lds(reinterpret_cast<const void *>(forms.kern[f]), RANK_LDS_LIMIT, forms.done[f]);
        if (e != AMAR_OK) return e;
    }
    hipLaunchKernelGGL(forms.kern[f], grid, dim3(256), lds_bytes, st, args);
    return amar_check_launch();
}

// Everything amar_recommend_f32, amar_recommend_among_f32 and amar_recommend_group_f32 do after their own leading checks, in the
// order their callers rely on: tables, route; the slice count (`slices`: what the entry point's own *_slices rule gave for
// `n_slices`, negative = its refusal), its cross-check with the count the caller sized the workspaces from, the workspaces; the
// empty call; the outputs; the fit, the grid limit; the launch and, with several slices, their merge.  `m`: the selector rows
// (users or groups); `n_rows`: the length the tile loop runs over (items or candidates); `args`: zeroed but for the entry
// point's own fields.
template <class Args>
inline int rank_topk(RankForms<Args> &forms, int kind, const RankHead &h, Args &args, int64_t m, int64_t n_rows, int32_t slices,
                     int32_t n_slices, int32_t k, int32_t *workspace_items, float *workspace_scores, int32_t *out_items,
                     float *out_scores, amar_stream_t stream) {
    RankArgs &a = rank_args_of(args);
    RankShape sh;
    amar_rank_route_info route;
    const int rc = rank_prepare(kind, h, m, a, sh, route);
    if (rc != AMAR_OK) return rc;
    if (slices < 1) return slices < 0 ? slices : AMAR_EINVAL;
    if (n_slices > 0 && slices != n_slices) return AMAR_EINVAL;       // the caller sizes the workspace from the *_slices query
    if (slices > 1 && (!workspace_items || !workspace_scores)) return AMAR_EINVAL;
    if (m == 0) return AMAR_OK;
    if (!out_items || !out_scores) return AMAR_EINVAL;
    a.out.k = k;
    a.slice_items = (int)rank_slice_rows(n_rows, sh.tile_items, slices);
    a.out.n_slices = slices;
    a.out.rows = slices > 1 ? workspace_items : out_items;
    a.out.scores = slices > 1 ? workspace_scores : out_scores;
    if (!route.fits) return AMAR_EUNSUPPORTED;
    const int64_t blocks = (m + RANK_UB - 1) / RANK_UB;
    if (blocks >= (1ll << 31)) return AMAR_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int e = rank_launch_form(forms, route, dim3((unsigned)blocks, (unsigned)slices), st, args);
    if (e != AMAR_OK || slices == 1) return e;
    return rank_merge_slices(workspace_items, workspace_scores, m, slices, k, out_items, out_scores, st);
}

// What amar_recommend_slices, amar_rank_of_slices and amar_recommend_group_slices check before they count, and the tile a
// stack's launches walk (s.tile_items).  `members`: 0 where the query has none.
inline int rank_slices_tile(int64_t rows, int64_t members, int32_t n_items, const int32_t *dims, int32_t n_layers, RankShape &s) {
    if (rows < 0 || members < 0 || n_items < 0 || !dims || n_layers < 2 || n_layers > RANK_MAX_LAYERS + 1) return AMAR_EINVAL;
    return rank_shape(dims, n_layers, s);
}

}  // namespace

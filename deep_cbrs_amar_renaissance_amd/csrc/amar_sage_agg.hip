// GraphSAGE's sum / max / min aggregators for gfx950 (the mean aggregator lives in amar_propagate.hip).
//
// Same work decomposition as the mean row kernel: one 64-lane wavefront per CSR row, LPN = F/4 lanes per entry (one coalesced
// 4F-byte read of the neighbour's row), NS = 64/LPN entries in flight per wave-instruction.  What differs is the merge: a
// maximum is not an addition, so nothing of the sum kernels' machinery (DPP adds, value-free images that count duplicates by
// repetition, "the reverse pass is the same SpMM") carries over.
//
//   sage_agg_row_kernel   the fused inference layer: gather-reduce, then [x || agg] . W + b, l2-normalise, ReLU in registers
//   sage_agg_kernel       the aggregate alone for any F % 4 == 0, F <= 64, with the tie count the reverse pass divides by
//   sage_agg_pack_kernel  [agg_i | d_agg_i / cnt_i] as one row of 2F floats
//   sage_agg_bwd_kernel   row j walks the targets that list it — row j of the TRANSPOSED structure (its own row where the edge
//                         multiset is symmetric) — and adds the shares it attained
//
// max / min / counts are exact and the reverse pass adds in a fixed order: every result is bitwise reproducible.  No atomics.
// Reference semantics: see include/amar_hip.h.
#include "amar_common.h"
#include <math.h>

namespace {

constexpr int WAVES_PER_BLOCK = 4;

bool ld_ok(int64_t ld, int F) { return ld >= F && (ld & 3) == 0; }

template <int OP>
__device__ __forceinline__ float agg_identity() {
    return OP == AMAR_AGG_MAX ? -INFINITY : (OP == AMAR_AGG_MIN ? INFINITY : 0.f);
}
template <int OP>
__device__ __forceinline__ float agg_op(float a, float b) {
    return OP == AMAR_AGG_MAX ? fmaxf(a, b) : (OP == AMAR_AGG_MIN ? fminf(a, b) : a + b);
}
template <int OP>
__device__ __forceinline__ float4 f4_agg(float4 a, float4 b) {
    return make_float4(agg_op<OP>(a.x, b.x), agg_op<OP>(a.y, b.y), agg_op<OP>(a.z, b.z), agg_op<OP>(a.w, b.w));
}

// OP over all lanes l' with l' % STRIDE == l % STRIDE; every lane receives the result (wave_sum_stride with another operator).
template <int STRIDE, int OP>
__device__ __forceinline__ float wave_agg_stride(float v) {
    if (STRIDE <= 8) v = agg_op<OP>(v, dpp_mov<0x128>(v));          // row_ror:8
    if (STRIDE <= 4) v = agg_op<OP>(v, dpp_mov<0x124>(v));          // row_ror:4
    if (STRIDE <= 2) v = agg_op<OP>(v, dpp_mov<0x122>(v));          // row_ror:2
    if (STRIDE <= 1) v = agg_op<OP>(v, dpp_mov<0x121>(v));          // row_ror:1
    float a, b;
    b = swap16_other(v, a); v = agg_op<OP>(a, b);                    // lane offset 16
    b = swap32_other(v, a); v = agg_op<OP>(a, b);                    // lane offset 32
    return v;
}

// ---- fused inference layer -------------------------------------------------------------------------------------------
struct SageAggArgs {
    const int32_t *rowptr; const int32_t *colidx; const float *X; int64_t ldx;
    const float *W; const float *bias; int C; float *Y; int64_t ldy; int self_loop; int n_rows;
};

template <int F, int OP>
__global__ __launch_bounds__(WAVES_PER_BLOCK * AMAR_WAVE) void sage_agg_row_kernel(const SageAggArgs a) {
    constexpr int LPN = F / 4, NS = AMAR_WAVE / LPN;
    const int lane = threadIdx.x & (AMAR_WAVE - 1);
    const int row = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int q = lane % LPN, slot = lane / LPN;

    float wx[F], wa[F];                                // column `lane` of W[0:F] (self) and W[F:2F] (aggregate)
#pragma unroll
    for (int k = 0; k < F; ++k) {
        wx[k] = lane < a.C ? a.W[k * a.C + lane] : 0.f;
        wa[k] = lane < a.C ? a.W[(F + k) * a.C + lane] : 0.f;
    }
    const int beg = a.rowptr[row], end = a.rowptr[row + 1];
    const float id = agg_identity<OP>();
    float4 agg = make_float4(id, id, id, id);
    int p = beg + slot;
    // two entries per lane in flight: both index loads are issued before either gather
    for (; p + NS < end; p += 2 * NS) {
        const int c0 = a.colidx[p], c1 = a.colidx[p + NS];
        const float4 x0 = *reinterpret_cast<const float4 *>(a.X + (int64_t)c0 * a.ldx + 4 * q);
        const float4 x1 = *reinterpret_cast<const float4 *>(a.X + (int64_t)c1 * a.ldx + 4 * q);
        agg = f4_agg<OP>(f4_agg<OP>(agg, x0), x1);
    }
    if (p < end) {
        const int c0 = a.colidx[p];
        agg = f4_agg<OP>(agg, *reinterpret_cast<const float4 *>(a.X + (int64_t)c0 * a.ldx + 4 * q));
    }
    agg = make_float4(wave_agg_stride<LPN, OP>(agg.x), wave_agg_stride<LPN, OP>(agg.y),
                      wave_agg_stride<LPN, OP>(agg.z), wave_agg_stride<LPN, OP>(agg.w));
    const float4 xs = *reinterpret_cast<const float4 *>(a.X + (int64_t)row * a.ldx + 4 * q);
    if (a.self_loop) agg = f4_agg<OP>(agg, xs);
    else if (end == beg) agg = f4_zero();              // a row without entries aggregates to 0 (amar_hip.h)

    float fx[F], fa[F];
    broadcast_row<F>(xs, fx);
    broadcast_row<F>(agg, fa);
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < F; ++k) o = fmaf(fx[k], wx[k], o);
#pragma unroll
    for (int k = 0; k < F; ++k) o = fmaf(fa[k], wa[k], o);
    o = lane < a.C ? o + a.bias[lane] : 0.f;
    float ss = o * o;
    ss = wave_sum_stride<1>(ss);
    o *= rsqrtf(fmaxf(ss, 1e-12f));                    // tf.nn.l2_normalize(axis=-1), before the activation
    o = fmaxf(o, 0.f);
    if (lane < a.C) a.Y[(int64_t)row * a.ldy + lane] = o;
}

// ---- aggregate + tie count -------------------------------------------------------------------------------------------
// (m, c) = (extremum so far, how many entries attain it).  Merging two pairs is associative and commutative and every
// intermediate is exact, so the order the lanes meet in does not matter.
template <bool MIN>
__device__ __forceinline__ void ext_merge(float &m, float &c, float pm, float pc) {
    if (MIN ? pm < m : pm > m) { m = pm; c = pc; }
    else if (pm == m) c += pc;
}
template <bool MIN>
__device__ __forceinline__ void f4_ext_merge(float4 &m, float4 &c, const float4 &pm, const float4 &pc) {
    ext_merge<MIN>(m.x, c.x, pm.x, pc.x); ext_merge<MIN>(m.y, c.y, pm.y, pc.y);
    ext_merge<MIN>(m.z, c.z, pm.z, pc.z); ext_merge<MIN>(m.w, c.w, pm.w, pc.w);
}

struct AggArgs {
    const int32_t *rowptr; const int32_t *colidx; const float *X; int64_t ldx; int F;
    float *AGG; int64_t lda; float *CNT; int64_t ldc; int self_loop; int n_rows;
};

// F is a run-time value here (24 and 48 give LPN = 6 and 12, which no DPP butterfly spans): slot s of NS = 64 / LPN takes the
// entries s, s + NS, ...; the slots are then folded onto slot 0 by halving distances with wavefront shuffles.  After the step at
// distance d the slots below d hold everything of the slots below 2d, so each slot is merged exactly once.
template <bool MIN>
__global__ __launch_bounds__(WAVES_PER_BLOCK * AMAR_WAVE) void sage_agg_kernel(const AggArgs a) {
    const int lane = threadIdx.x & (AMAR_WAVE - 1);
    const int row = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int LPN = a.F >> 2, NS = AMAR_WAVE / LPN;
    const int slot = lane / LPN, q = lane - slot * LPN;
    const bool active = slot < NS;                     // 64 % LPN lanes at the top of the wave have no entry slot
    const int beg = a.rowptr[row], end = a.rowptr[row + 1];
    const float id = MIN ? INFINITY : -INFINITY;
    const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
    float4 m = make_float4(id, id, id, id), c = f4_zero();
    if (active) {
        if (a.self_loop && slot == 0) { m = *reinterpret_cast<const float4 *>(a.X + (int64_t)row * a.ldx + 4 * q); c = one; }
        int p = beg + slot;
        for (; p + NS < end; p += 2 * NS) {
            const int c0 = a.colidx[p], c1 = a.colidx[p + NS];
            const float4 x0 = *reinterpret_cast<const float4 *>(a.X + (int64_t)c0 * a.ldx + 4 * q);
            const float4 x1 = *reinterpret_cast<const float4 *>(a.X + (int64_t)c1 * a.ldx + 4 * q);
            f4_ext_merge<MIN>(m, c, x0, one);
            f4_ext_merge<MIN>(m, c, x1, one);
        }
        if (p < end) {
            const int c0 = a.colidx[p];
            f4_ext_merge<MIN>(m, c, *reinterpret_cast<const float4 *>(a.X + (int64_t)c0 * a.ldx + 4 * q), one);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        if (d >= NS) continue;                         // wave-uniform
        const int src = (lane + d * LPN) & (AMAR_WAVE - 1);
        const float4 pm = f4_shfl(m, src), pc = f4_shfl(c, src);
        if (active && slot + d < NS) f4_ext_merge<MIN>(m, c, pm, pc);
    }
    if (slot == 0) {
        if (end == beg && !a.self_loop) m = f4_zero();   // a row without entries aggregates to 0; its count stays 0
        *reinterpret_cast<float4 *>(a.AGG + (int64_t)row * a.lda + 4 * q) = m;
        if (a.CNT) *reinterpret_cast<float4 *>(a.CNT + (int64_t)row * a.ldc + 4 * q) = c;
    }
}

// ---- reverse pass ----------------------------------------------------------------------------------------------------
struct AggBwdArgs {
    const int32_t *rowptr; const int32_t *colidx; const float *X; int64_t ldx;
    const float *AGG; int64_t lda; const float *CNT; int64_t ldc; const float *DAGG; int64_t ldg; int F;
    float *pack; float *DX; int64_t lddx; int self_loop; int n_rows;
};

__global__ __launch_bounds__(256) void sage_agg_pack_kernel(const AggBwdArgs a) {
    const int LPN = a.F >> 2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)a.n_rows * LPN) return;
    const int64_t i = idx / LPN;
    const int q = (int)(idx - i * LPN);
    const float4 g = *reinterpret_cast<const float4 *>(a.DAGG + i * a.ldg + 4 * q);
    const float4 c = *reinterpret_cast<const float4 *>(a.CNT + i * a.ldc + 4 * q);
    float *dst = a.pack + i * (2 * a.F) + 4 * q;
    *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(a.AGG + i * a.lda + 4 * q);
    *reinterpret_cast<float4 *>(dst + a.F) = make_float4(c.x > 0.f ? g.x / c.x : 0.f, c.y > 0.f ? g.y / c.y : 0.f,
                                                         c.z > 0.f ? g.z / c.z : 0.f, c.w > 0.f ? g.w / c.w : 0.f);
}

__device__ __forceinline__ void take_share(float4 &acc, const float4 &xs, const float *__restrict__ prow, int F) {
    const float4 m = *reinterpret_cast<const float4 *>(prow);
    const float4 g = *reinterpret_cast<const float4 *>(prow + F);
    acc.x += xs.x == m.x ? g.x : 0.f; acc.y += xs.y == m.y ? g.y : 0.f;
    acc.z += xs.z == m.z ? g.z : 0.f; acc.w += xs.w == m.w ? g.w : 0.f;
}

__global__ __launch_bounds__(WAVES_PER_BLOCK * AMAR_WAVE) void sage_agg_bwd_kernel(const AggBwdArgs a) {
    const int lane = threadIdx.x & (AMAR_WAVE - 1);
    const int row = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int LPN = a.F >> 2, NS = AMAR_WAVE / LPN;
    const int slot = lane / LPN, q = lane - slot * LPN;
    const bool active = slot < NS;
    const int beg = a.rowptr[row], end = a.rowptr[row + 1];
    const int64_t ldp = 2 * a.F;
    float4 acc = f4_zero();
    if (active) {
        const float4 xs = *reinterpret_cast<const float4 *>(a.X + (int64_t)row * a.ldx + 4 * q);
        if (a.self_loop && slot == 0) take_share(acc, xs, a.pack + row * ldp + 4 * q, a.F);
        int p = beg + slot;
        for (; p + NS < end; p += 2 * NS) {
            const int c0 = a.colidx[p], c1 = a.colidx[p + NS];
            take_share(acc, xs, a.pack + c0 * ldp + 4 * q, a.F);
            take_share(acc, xs, a.pack + c1 * ldp + 4 * q, a.F);
        }
        if (p < end) take_share(acc, xs, a.pack + a.colidx[p] * ldp + 4 * q, a.F);
    }
    for (int d = 32; d >= 1; d >>= 1) {                // the fold of sage_agg_kernel with +: a fixed order, so reproducible
        if (d >= NS) continue;
        const float4 pa = f4_shfl(acc, (lane + d * LPN) & (AMAR_WAVE - 1));
        if (active && slot + d < NS) acc = f4_add(acc, pa);
    }
    if (slot == 0) {
        float4 *dx = reinterpret_cast<float4 *>(a.DX + (int64_t)row * a.lddx + 4 * q);
        *dx = f4_add(*dx, acc);
    }
}

}  // namespace

extern "C" {

int amar_sage_layer_agg_f32(const int32_t *rowptr, const int32_t *colidx,
                            const float *X, int64_t ldx, int32_t F,
                            const float *W, const float *bias, int32_t C,
                            float *Y, int64_t ldy, int32_t self_loop, int32_t op,
                            int32_t n_rows, amar_stream_t stream) {
    if (n_rows < 0 || !rowptr || !X || !W || !bias || !Y || C < 1 || ldy < C) return AMAR_EINVAL;
    if (op != AMAR_AGG_SUM && op != AMAR_AGG_MAX && op != AMAR_AGG_MIN) return AMAR_EINVAL;
    if (F < 1 || !ld_ok(ldx, F) || !amar_aligned16(X)) return AMAR_EINVAL;
    if (C > 64 || (F != 4 && F != 8 && F != 16 && F != 32)) return AMAR_EUNSUPPORTED;
    if (n_rows == 0) return AMAR_OK;
    if (!colidx) return AMAR_EINVAL;
    SageAggArgs a{rowptr, colidx, X, ldx, W, bias, C, Y, ldy, self_loop ? 1 : 0, n_rows};
    const dim3 grid((n_rows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), block(WAVES_PER_BLOCK * AMAR_WAVE);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define AMAR_SAGE_AGG_F(FF)                                                                               \
    case FF:                                                                                              \
        if (op == AMAR_AGG_MAX) hipLaunchKernelGGL((sage_agg_row_kernel<FF, AMAR_AGG_MAX>), grid, block, 0, st, a);      \
        else if (op == AMAR_AGG_MIN) hipLaunchKernelGGL((sage_agg_row_kernel<FF, AMAR_AGG_MIN>), grid, block, 0, st, a); \
        else hipLaunchKernelGGL((sage_agg_row_kernel<FF, AMAR_AGG_SUM>), grid, block, 0, st, a);                         \
        break;
    switch (F) {
    AMAR_SAGE_AGG_F(4)
    AMAR_SAGE_AGG_F(8)
    AMAR_SAGE_AGG_F(16)
    AMAR_SAGE_AGG_F(32)
    default: return AMAR_EUNSUPPORTED;
    }
#undef AMAR_SAGE_AGG_F
    return amar_check_launch();
}

int amar_sage_aggregate_f32(const int32_t *rowptr, const int32_t *colidx,
                            const float *X, int64_t ldx, int32_t F,
                            float *AGG, int64_t lda, float *CNT, int64_t ldc,
                            int32_t self_loop, int32_t op, int32_t n_rows, amar_stream_t stream) {
    if (n_rows < 0 || !rowptr || !X || !AGG || F < 4 || (F & 3)) return AMAR_EINVAL;
    if (op != AMAR_AGG_SUM && op != AMAR_AGG_MAX && op != AMAR_AGG_MIN) return AMAR_EINVAL;
    if (!ld_ok(ldx, F) || !ld_ok(lda, F) || !amar_aligned16(X) || !amar_aligned16(AGG)) return AMAR_EINVAL;
    if (CNT && (!ld_ok(ldc, F) || !amar_aligned16(CNT))) return AMAR_EINVAL;
    if (F > 64 || op == AMAR_AGG_SUM) return AMAR_EUNSUPPORTED;
    if (n_rows == 0) return AMAR_OK;
    if (!colidx) return AMAR_EINVAL;
    AggArgs a{rowptr, colidx, X, ldx, F, AGG, lda, CNT, ldc, self_loop ? 1 : 0, n_rows};
    const dim3 grid((n_rows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), block(WAVES_PER_BLOCK * AMAR_WAVE);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (op == AMAR_AGG_MIN) hipLaunchKernelGGL(sage_agg_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(sage_agg_kernel<false>, grid, block, 0, st, a);
    return amar_check_launch();
}

int amar_sage_aggregate_bwd_f32(const int32_t *rowptr, const int32_t *colidx,
                                const float *X, int64_t ldx, const float *AGG, int64_t lda,
                                const float *CNT, int64_t ldc, const float *DAGG, int64_t ldg, int32_t F,
                                float *pack, float *DX, int64_t lddx,
                                int32_t self_loop, int32_t n_rows, amar_stream_t stream) {
    if (n_rows < 0 || !rowptr || !X || !AGG || !CNT || !DAGG || !pack || !DX || F < 4 || (F & 3)) return AMAR_EINVAL;
    if (!ld_ok(ldx, F) || !ld_ok(lda, F) || !ld_ok(ldc, F) || !ld_ok(ldg, F) || !ld_ok(lddx, F)) return AMAR_EINVAL;
    if (!amar_aligned16(X) || !amar_aligned16(AGG) || !amar_aligned16(CNT) || !amar_aligned16(DAGG) || !amar_aligned16(pack) ||
        !amar_aligned16(DX))
        return AMAR_EINVAL;
    if (F > 64) return AMAR_EUNSUPPORTED;
    if (n_rows == 0) return AMAR_OK;
    if (!colidx) return AMAR_EINVAL;
    AggBwdArgs a{rowptr, colidx, X, ldx, AGG, lda, CNT, ldc, DAGG, ldg, F, pack, DX, lddx, self_loop ? 1 : 0, n_rows};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t quads = (int64_t)n_rows * (F >> 2);
    hipLaunchKernelGGL(sage_agg_pack_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, a);
    const dim3 grid((n_rows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), block(WAVES_PER_BLOCK * AMAR_WAVE);
    hipLaunchKernelGGL(sage_agg_bwd_kernel, grid, block, 0, st, a);
    return amar_check_launch();
}

}  // extern "C"

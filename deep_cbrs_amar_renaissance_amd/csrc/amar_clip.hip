// Gradient clipping of tf.keras optimizers (gfx950): clipvalue, clipnorm and global_clipnorm, as include/amar_hip.h states them.  The
// clipped quantity is the FINISHED gradient gi = fmaf(2 l2, w, sum of the deferred partials in group order) — what optim_multi_kernel
// forms in registers and never stores — so the pass finishes the gradients itself, into group 0 of every slot, and the
// optimizer launch that follows runs on a table with g_groups = 0 and l2 = 0 (fmaf(0, w, g) == g: the update kernels stay as they are).
// Three small launches over the block partition of the optimizer slot tables (1024 elements per block):
//   finish   gi into group 0 (clipvalue: clamped, and done); per block the sum of gi^2 into workspace[block]; the L2 part of the loss
//   scales   one workgroup per slot (global norm: one in all) adds the block sums in ascending block order with a fixed tree and
//            writes s = norm > clip ? clip / norm : 1 into workspace[total_blocks + slot]
//   apply    g *= s
// No float atomic takes part in a norm: the same inputs give the same bits on every run, eagerly and replayed.  The scales live in
// device memory; only `mode` and `clip` are baked into a captured batch.  Plain vector stores only.
#include "amar_common.h"

namespace {

__device__ __forceinline__ void f4_to(float (&dst)[4], const float4 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
__device__ __forceinline__ float4 f4_from(const float (&src)[4]) { return make_float4(src[0], src[1], src[2], src[3]); }

__device__ __forceinline__ int slot_of_block(const amar_clip_slot *__restrict__ slots, int n_slots) {
    int sidx = 0;
    while (sidx + 1 < n_slots && (int64_t)blockIdx.x >= slots[sidx + 1].first_block) ++sidx;
    return sidx;
}

// The sum of the workgroup's 256 values, in every thread: the wavefront's tree, then the four wave sums in fixed order.
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum_stride<1>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// optim_multi_kernel's loads (16 bytes per lane where n % 4 == 0 and w, g are aligned, else the scalar layout; the partials' loads
// before their adds, the adds in group order) without an update behind them: the finished gradient goes back to group 0.
template <int MODE>
__global__ __launch_bounds__(256) void clip_finish_kernel(const amar_clip_slot *__restrict__ slots, int n_slots, float clip,
                                                          float *__restrict__ workspace, float reg_scale, float *__restrict__ loss_acc) {
#pragma clang fp contract(off)
    __shared__ float red[8];
    const amar_clip_slot sl = slots[slot_of_block(slots, n_slots)];
    const float l2x2 = 2.f * sl.l2;
    const int64_t base = ((int64_t)blockIdx.x - sl.first_block) * 1024;
    const bool vec = (sl.n & 3) == 0 && ((reinterpret_cast<uintptr_t>(sl.w) | reinterpret_cast<uintptr_t>(sl.g)) & 15u) == 0;
    float wi[4], gs[4];
    int64_t idx[4];
    if (vec) {
        const int64_t i0 = base + 4 * threadIdx.x;
        const bool ok = i0 < sl.n;
#pragma unroll
        for (int r = 0; r < 4; ++r) idx[r] = ok ? i0 + r : sl.n;
        f4_to(wi, ok ? *reinterpret_cast<const float4 *>(sl.w + i0) : f4_zero());
        f4_to(gs, ok ? *reinterpret_cast<const float4 *>(sl.g + i0) : f4_zero());
        for (int c = 1; c < sl.g_groups; c += 16) {                  // sixteen groups in flight
            float4 part[16];
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                part[cc] = (c + cc < sl.g_groups && ok) ? *reinterpret_cast<const float4 *>(sl.g + (int64_t)(c + cc) * sl.n + i0) : f4_zero();
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                if (c + cc < sl.g_groups) { gs[0] += part[cc].x; gs[1] += part[cc].y; gs[2] += part[cc].z; gs[3] += part[cc].w; }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            idx[r] = base + r * 256 + threadIdx.x;
            const bool ok = idx[r] < sl.n;
            wi[r] = ok ? sl.w[idx[r]] : 0.f;
            gs[r] = ok ? sl.g[idx[r]] : 0.f;
        }
        for (int c = 1; c < sl.g_groups; c += 4) {
            float part[4][4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    part[cc][r] = (c + cc < sl.g_groups && idx[r] < sl.n) ? sl.g[(int64_t)(c + cc) * sl.n + idx[r]] : 0.f;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                if (c + cc < sl.g_groups) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) gs[r] += part[cc][r];
                }
        }
    }
    float gsq = 0.f, wsq = 0.f;
    float gi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        gi[r] = fmaf(l2x2, wi[r], gs[r]);
        if (MODE == AMAR_CLIP_VALUE) gi[r] = gi[r] < -clip ? -clip : (gi[r] > clip ? clip : gi[r]);   // (a NaN stays a NaN)
        if (idx[r] < sl.n) { gsq = fmaf(gi[r], gi[r], gsq); wsq = fmaf(wi[r], wi[r], wsq); }
    }
    if (vec) {
        if (idx[0] < sl.n) *reinterpret_cast<float4 *>(sl.g + idx[0]) = f4_from(gi);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (idx[r] < sl.n) sl.g[idx[r]] = gi[r];
    }
    if (MODE != AMAR_CLIP_VALUE) {
        gsq = block_sum(gsq, red);
        if (threadIdx.x == 0) workspace[blockIdx.x] = gsq;
    }
    if (loss_acc && sl.l2 != 0.f) {                                  // as the optimizer launches: block sum, one atomic per block
        wsq = block_sum(wsq, red + 4);
        if (threadIdx.x == 0) atomicAdd(loss_acc, reg_scale * sl.l2 * wsq);
    }
}

// Workgroup s (global norm: the only one) owns the block sums [b0, b1): thread t adds those at b0 + t, b0 + t + 256, ... in ascending
// order, block_sum adds the 256 results.  s = 1 exactly where the clip does not bind, so the apply launch then changes no bit.
template <int MODE>
__global__ __launch_bounds__(256) void clip_scales_kernel(const amar_clip_slot *__restrict__ slots, int64_t total_blocks, float clip,
                                                          float *__restrict__ workspace, float *__restrict__ norms) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    int64_t b0 = 0, b1 = total_blocks;
    if (MODE == AMAR_CLIP_NORM) {
        const amar_clip_slot sl = slots[blockIdx.x];
        b0 = sl.first_block;
        b1 = b0 + (sl.n + 1023) / 1024;
        if (b1 > total_blocks) b1 = total_blocks;
    }
    float acc = 0.f;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += 256) acc += workspace[b];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(acc);
        workspace[total_blocks + blockIdx.x] = norm > clip ? clip / norm : 1.f;
        if (norms) norms[blockIdx.x] = norm;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void clip_apply_kernel(const amar_clip_slot *__restrict__ slots, int n_slots, int64_t total_blocks,
                                                         const float *__restrict__ workspace) {
    const int sidx = slot_of_block(slots, n_slots);
    const float s = workspace[total_blocks + (MODE == AMAR_CLIP_NORM ? sidx : 0)];
    if (s == 1.f) return;                                            // (uniform over the workgroup)
    const amar_clip_slot sl = slots[sidx];
    const int64_t base = ((int64_t)blockIdx.x - sl.first_block) * 1024;
    if ((sl.n & 3) == 0 && (reinterpret_cast<uintptr_t>(sl.g) & 15u) == 0) {
        const int64_t i0 = base + 4 * threadIdx.x;
        if (i0 < sl.n) {
            float4 v = *reinterpret_cast<const float4 *>(sl.g + i0);
            v.x *= s; v.y *= s; v.z *= s; v.w *= s;
            *reinterpret_cast<float4 *>(sl.g + i0) = v;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = base + r * 256 + threadIdx.x;
            if (i < sl.n) sl.g[i] *= s;
        }
    }
}

template <int MODE>
void launch_clip(float clip, const amar_clip_slot *slots, int32_t n_slots, int64_t total_blocks, float *workspace, float *norms,
                 float reg_scale, float *loss_acc, hipStream_t st) {
    hipLaunchKernelGGL(clip_finish_kernel<MODE>, dim3((unsigned)total_blocks), dim3(256), 0, st, slots, n_slots, clip, workspace,
                       reg_scale, loss_acc);
    if (MODE == AMAR_CLIP_VALUE) return;
    hipLaunchKernelGGL(clip_scales_kernel<MODE>, dim3(MODE == AMAR_CLIP_NORM ? (unsigned)n_slots : 1u), dim3(256), 0, st, slots,
                       total_blocks, clip, workspace, norms);
    hipLaunchKernelGGL(clip_apply_kernel<MODE>, dim3((unsigned)total_blocks), dim3(256), 0, st, slots, n_slots, total_blocks, workspace);
}

}  // namespace

extern "C" {

int64_t amar_grad_clip_workspace_floats(int32_t n_slots, int64_t total_blocks) {
    if (n_slots < 1 || total_blocks < 1 || total_blocks > 0x7fffffff) return AMAR_EINVAL;
    return total_blocks + n_slots;
}

int amar_grad_clip_f32(int32_t mode, float clip, const amar_clip_slot *slots, int32_t n_slots, int64_t total_blocks, float *workspace,
                       float *norms, float reg_scale, float *loss_acc, amar_stream_t stream) {
    if (mode != AMAR_CLIP_VALUE && mode != AMAR_CLIP_NORM && mode != AMAR_CLIP_GLOBAL_NORM) return AMAR_EINVAL;
    if (!(clip > 0.f) || !slots || n_slots < 1 || total_blocks < 1 || total_blocks > 0x7fffffff) return AMAR_EINVAL;
    if (mode != AMAR_CLIP_VALUE && !workspace) return AMAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == AMAR_CLIP_VALUE) launch_clip<AMAR_CLIP_VALUE>(clip, slots, n_slots, total_blocks, workspace, norms, reg_scale, loss_acc, st);
    else if (mode == AMAR_CLIP_NORM) launch_clip<AMAR_CLIP_NORM>(clip, slots, n_slots, total_blocks, workspace, norms, reg_scale, loss_acc, st);
    else launch_clip<AMAR_CLIP_GLOBAL_NORM>(clip, slots, n_slots, total_blocks, workspace, norms, reg_scale, loss_acc, st);
    return amar_check_launch();
}

}  // extern "C"

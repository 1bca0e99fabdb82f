// The optimizers of tf.keras.optimizers (gfx950): Adam, SGD (momentum, Nesterov), RMSprop (momentum, centered), Adagrad, Adamax, Nadam and
// Adam(amsgrad=True), as include/amar_hip.h states them.  A one-thread kernel advances the step counter and the step-dependent scalars in
// device memory (nothing that changes from step to step is baked into a captured training graph), ONE launch updates every parameter of
// a model from a slot table (adding the deferred weight-gradient partials in group order and the L2 part of the reported loss), and a
// single-tensor form reads the same device state.  The rule is a template parameter: a rule loads and stores only the arrays it uses and
// nothing inside the element loop branches on it.  The amar_adam_* entry points are Adam's instantiations of the same kernels.
#include "amar_optim.h"

namespace {

// What an element update reads besides its own element: the hyper-parameters and the device state of this step (wave-uniform).
struct OptK { float step, momentum, rho, b1, b2, eps, mu_next, omb2, cg, cm; };

__device__ __forceinline__ OptK hyper_k(const amar_optim_hyper h, float step) {
    OptK k = {};
    k.step = step; k.momentum = h.momentum; k.rho = h.rho; k.b1 = h.beta_1; k.b2 = h.beta_2; k.eps = h.epsilon;
    return k;
}

// Every rule reads state[1]; Nadam alone reads above it (Adam's state ends there).
template <int V>
__device__ __forceinline__ OptK load_k(const float *__restrict__ state, const amar_optim_hyper h) {
    OptK k = hyper_k(h, state[1]);
    if constexpr (V == V_NADAM) { k.mu_next = state[3]; k.omb2 = state[5]; k.cg = state[6]; k.cm = state[7]; }
    return k;
}

// One update of one element, shared by every update kernel: they give the same bits on the same element (the header's promise).  The
// fused products are written out and nothing else may be fused, so the bits do not depend on the kernel around it.  s0..s2 are the
// rule's state arrays in the header's order; the ones a rule does not have are neither read nor written.
template <int V>
__device__ __forceinline__ void optim_step(float &w, float g, float &s0, float &s1, float &s2, const OptK &k, float l2x2) {
#pragma clang fp contract(off)
    const float gi = fmaf(l2x2, w, g);
    if constexpr (V == V_SGD) {
        w = fmaf(-k.step, gi, w);
    } else if constexpr (V == V_SGD_MOM) {
        s0 = fmaf(k.momentum, s0, -(k.step * gi));
        w = w + s0;
    } else if constexpr (V == V_SGD_NESTEROV) {
        const float lg = k.step * gi;
        s0 = fmaf(k.momentum, s0, -lg);
        w = w + fmaf(k.momentum, s0, -lg);
    } else if constexpr (V == V_RMS || V == V_RMS_MOM || V == V_RMS_CENTERED || V == V_RMS_CENTERED_MOM) {
        constexpr bool centered = V == V_RMS_CENTERED || V == V_RMS_CENTERED_MOM;
        const float omr = 1.f - k.rho;
        s0 = fmaf(k.rho, s0, (omr * gi) * gi);
        float d = s0;
        if constexpr (centered) {
            s1 = fmaf(k.rho, s1, omr * gi);
            d = fmaxf(fmaf(-s1, s1, s0), 0.f);                        // (rounding can take rms - mg^2 below 0 where the true value is 0)
        }
        if constexpr (V == V_RMS || V == V_RMS_CENTERED) {
            w = w - (k.step * gi) / (sqrtf(d) + k.eps);
        } else {
            float &mom = centered ? s2 : s1;
            mom = fmaf(k.momentum, mom, (k.step * gi) / sqrtf(d + k.eps));
            w = w - mom;
        }
    } else if constexpr (V == V_ADAGRAD) {
        s0 = fmaf(gi, gi, s0);
        w = w - (k.step * gi) / (sqrtf(s0) + k.eps);
    } else if constexpr (V == V_ADAMAX) {
        s0 = fmaf(k.b1, s0, (1.f - k.b1) * gi);
        s1 = fmaxf(k.b2 * s1, fabsf(gi));
        w = w - (k.step * s0) / (s1 + k.eps);
    } else if constexpr (V == V_NADAM) {
        s0 = fmaf(k.b1, s0, (1.f - k.b1) * gi);
        s1 = fmaf(k.b2, s1, ((1.f - k.b2) * gi) * gi);
        w = w - fmaf(k.cg, gi, k.cm * s0) / (sqrtf(s1 / k.omb2) + k.eps);
    } else {                                                          // V_ADAM, V_AMSGRAD: step carries the bias correction
        s0 = fmaf(k.b1, s0, (1.f - k.b1) * gi);
        s1 = fmaf(k.b2, s1, ((1.f - k.b2) * gi) * gi);
        float d = s1;
        if constexpr (V == V_AMSGRAD) d = s2 = fmaxf(s2, s1);
        w = w - (k.step * s0) / (sqrtf(d) + k.eps);
    }
}

__global__ void optim_advance_kernel(float *__restrict__ state, int rule, const amar_optim_hyper h) {
    optim_advance_state(state, rule, h.learning_rate, h);
}

// The single-tensor form.  The step scalars come from the device state, or (amar_adam_f32 alone: a step size formed on the host) from
// the argument.
template <int V>
__device__ __forceinline__ void optim_elements(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ s0,
                                               float *__restrict__ s1, float *__restrict__ s2, int64_t n, const OptK k, float l2x2) {
    constexpr int NS = state_arrays_of(V);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float wi = w[i], a = 0.f, b = 0.f, c = 0.f;
        if constexpr (NS > 0) a = s0[i];
        if constexpr (NS > 1) b = s1[i];
        if constexpr (NS > 2) c = s2[i];
        optim_step<V>(wi, g[i], a, b, c, k, l2x2);
        if constexpr (NS > 0) s0[i] = a;
        if constexpr (NS > 1) s1[i] = b;
        if constexpr (NS > 2) s2[i] = c;
        w[i] = wi;
    }
}

template <int V>
__global__ __launch_bounds__(256) void optim_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ s0,
                                                    float *__restrict__ s1, float *__restrict__ s2, int64_t n,
                                                    const float *__restrict__ state, const amar_optim_hyper h, float l2x2) {
    optim_elements<V>(w, g, s0, s1, s2, n, load_k<V>(state, h), l2x2);
}

__global__ __launch_bounds__(256) void adam_host_step_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m,
                                                             float *__restrict__ v, int64_t n, float lr_t, const amar_optim_hyper h,
                                                             float l2x2) {
    optim_elements<V_ADAM>(w, g, m, v, nullptr, n, hyper_k(h, lr_t), l2x2);
}

// State array a of a slot, for both slot layouts of the header.
__device__ __forceinline__ float *slot_array(const amar_optim_slot &sl, int a) { return a == 0 ? sl.s0 : (a == 1 ? sl.s1 : sl.s2); }
__device__ __forceinline__ float *slot_array(const amar_adam_slot &sl, int a) { return a == 0 ? sl.m : sl.v; }

__device__ __forceinline__ void f4_to(float (&dst)[4], const float4 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
__device__ __forceinline__ float4 f4_from(const float (&src)[4]) { return make_float4(src[0], src[1], src[2], src[3]); }

// Every parameter of a model in ONE launch: block b works on 1024 elements of the slot that owns it (slots carry their first block).
// All loads of a thread's four elements first, then the deferred partial gradients sixteen (scalar path: four) groups at a time, loads
// before adds, the adds in group order: written as one load -> add chain per element, the 16 partials of a Dense kernel's gradient were
// 16 dependent memory round trips — 30 us of every training batch, whatever the model's size.  Slots whose arrays allow it (16-byte
// aligned, n a multiple of 4: every table and kernel of the models here) move 16 bytes per lane — a thread then owns four NEIGHBOURING
// elements instead of four 256 apart; each element's arithmetic is the same either way.  Also adds reg_scale * l2 * sum(w^2) of the
// PRE-update weights to *loss_acc (the regularisation part of the batch loss Keras reports), one atomic per block, so no separate
// reduction launches are needed.  Slot: amar_optim_slot, or amar_adam_slot (V_ADAM) read where it lies.
template <int V, typename Slot>
__global__ __launch_bounds__(256) void optim_multi_kernel(const Slot *__restrict__ slots, int n_slots,
                                                          const float *__restrict__ state, const amar_optim_hyper h,
                                                          float reg_scale, float *__restrict__ loss_acc) {
    constexpr int NS = state_arrays_of(V);
    int sidx = 0;
    while (sidx + 1 < n_slots && (int64_t)blockIdx.x >= slots[sidx + 1].first_block) ++sidx;
    const Slot sl = slots[sidx];
    const OptK k = load_k<V>(state, h);
    const float l2x2 = 2.f * sl.l2;
    const int64_t base = ((int64_t)blockIdx.x - sl.first_block) * 1024;
    float *sp[3] = {nullptr, nullptr, nullptr};                      // (the arrays the rule has: the others are never looked at)
#pragma unroll
    for (int a = 0; a < NS; ++a) sp[a] = slot_array(sl, a);
    uintptr_t bits = reinterpret_cast<uintptr_t>(sl.w) | reinterpret_cast<uintptr_t>(sl.g);
#pragma unroll
    for (int a = 0; a < NS; ++a) bits |= reinterpret_cast<uintptr_t>(sp[a]);
    const bool vec = (sl.n & 3) == 0 && (bits & 15u) == 0;
    float wi[4], gs[4], si[3][4];
    int64_t idx[4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) si[a][r] = 0.f;
    if (vec) {
        const int64_t i0 = base + 4 * threadIdx.x;
        const bool ok = i0 < sl.n;
#pragma unroll
        for (int r = 0; r < 4; ++r) idx[r] = ok ? i0 + r : sl.n;
        f4_to(wi, ok ? *reinterpret_cast<const float4 *>(sl.w + i0) : f4_zero());
        f4_to(gs, ok ? *reinterpret_cast<const float4 *>(sl.g + i0) : f4_zero());
#pragma unroll
        for (int a = 0; a < NS; ++a) f4_to(si[a], ok ? *reinterpret_cast<const float4 *>(sp[a] + i0) : f4_zero());
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
#pragma unroll
            for (int a = 0; a < NS; ++a) si[a][r] = ok ? sp[a][idx[r]] : 0.f;
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
    float sq = 0.f;
    float wo[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        wo[r] = wi[r];
        optim_step<V>(wo[r], gs[r], si[0][r], si[1][r], si[2][r], k, l2x2);
        if (idx[r] < sl.n) sq = fmaf(wi[r], wi[r], sq);
    }
    if (vec) {
        if (idx[0] < sl.n) {
#pragma unroll
            for (int a = 0; a < NS; ++a) *reinterpret_cast<float4 *>(sp[a] + idx[0]) = f4_from(si[a]);
            *reinterpret_cast<float4 *>(sl.w + idx[0]) = f4_from(wo);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (idx[r] < sl.n) {
#pragma unroll
                for (int a = 0; a < NS; ++a) sp[a][idx[r]] = si[a][r];
                sl.w[idx[r]] = wo[r];
            }
    }
    if (loss_acc && sl.l2 != 0.f) {                                  // block sum, one atomic per block
        __shared__ float red[4];
        sq = wave_sum_stride<1>(sq);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(loss_acc, reg_scale * sl.l2 * (red[0] + red[1] + red[2] + red[3]));
    }
}

unsigned grid_of(int64_t total) {
    const int64_t b = (total + 255) / 256;
    return (unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

template <int V>
void launch_single(float *w, const float *g, float *s0, float *s1, float *s2, int64_t n, const float *state, const amar_optim_hyper &h,
                   float l2, hipStream_t st) {
    hipLaunchKernelGGL(optim_kernel<V>, dim3(grid_of(n)), dim3(256), 0, st, w, g, s0, s1, s2, n, state, h, 2.f * l2);
}

template <int V, typename Slot>
void launch_multi(const Slot *slots, int32_t n_slots, int64_t total_blocks, const float *state, const amar_optim_hyper &h,
                  float reg_scale, float *loss_acc, hipStream_t st) {
    hipLaunchKernelGGL((optim_multi_kernel<V, Slot>), dim3((unsigned)total_blocks), dim3(256), 0, st, slots, n_slots, state, h, reg_scale, loss_acc);
}

#define AMAR_FOR_EACH_VARIANT(CALL)                                                                                                      \
    switch (v) {                                                                                                                         \
    case V_SGD: CALL(V_SGD); break;                     case V_SGD_MOM: CALL(V_SGD_MOM); break;                                          \
    case V_SGD_NESTEROV: CALL(V_SGD_NESTEROV); break;   case V_RMS: CALL(V_RMS); break;                                                  \
    case V_RMS_MOM: CALL(V_RMS_MOM); break;             case V_RMS_CENTERED: CALL(V_RMS_CENTERED); break;                                \
    case V_RMS_CENTERED_MOM: CALL(V_RMS_CENTERED_MOM); break;                                                                            \
    case V_ADAGRAD: CALL(V_ADAGRAD); break;             case V_ADAMAX: CALL(V_ADAMAX); break;                                            \
    case V_NADAM: CALL(V_NADAM); break;                 case V_AMSGRAD: CALL(V_AMSGRAD); break;                                          \
    default: CALL(V_ADAM); break;                                                                                                        \
    }

}  // namespace

extern "C" {

int amar_optim_state_arrays(int32_t rule, int32_t flags, float momentum) {
    const int v = resolve_variant(rule, flags, momentum);
    return v < 0 ? AMAR_EINVAL : state_arrays_of(v);
}

int amar_optim_advance_f32(float *state, int32_t rule, int32_t flags, const amar_optim_hyper *hyper, amar_stream_t stream) {
    if (!state || !hyper || resolve_variant(rule, flags, hyper->momentum) < 0) return AMAR_EINVAL;
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, (int)rule, *hyper);
    return amar_check_launch();
}

int amar_optim_f32(int32_t rule, int32_t flags, const amar_optim_hyper *hyper, float *w, const float *g, float *s0, float *s1, float *s2,
                   int64_t n, const float *state, float l2, amar_stream_t stream) {
    if (!hyper) return AMAR_EINVAL;
    const int v = resolve_variant(rule, flags, hyper->momentum);
    if (v < 0 || n < 0 || !w || !g || !state) return AMAR_EINVAL;
    const int ns = state_arrays_of(v);
    if ((ns > 0 && !s0) || (ns > 1 && !s1) || (ns > 2 && !s2)) return AMAR_EINVAL;
    if (n == 0) return AMAR_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define AMAR_CALL(V) launch_single<V>(w, g, s0, s1, s2, n, state, *hyper, l2, st)
    AMAR_FOR_EACH_VARIANT(AMAR_CALL)
#undef AMAR_CALL
    return amar_check_launch();
}

int amar_optim_multi_f32(int32_t rule, int32_t flags, const amar_optim_hyper *hyper, const amar_optim_slot *slots, int32_t n_slots,
                         int64_t total_blocks, const float *state, float reg_scale, float *loss_acc, amar_stream_t stream) {
    if (!hyper) return AMAR_EINVAL;
    const int v = resolve_variant(rule, flags, hyper->momentum);
    if (v < 0 || !slots || n_slots < 1 || total_blocks < 1 || total_blocks > 0x7fffffff || !state) return AMAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define AMAR_CALL(V) launch_multi<V>(slots, n_slots, total_blocks, state, *hyper, reg_scale, loss_acc, st)
    AMAR_FOR_EACH_VARIANT(AMAR_CALL)
#undef AMAR_CALL
    return amar_check_launch();
}

// ---- Adam by its own entry points: the V_ADAM instantiations over two floats of state and amar_adam_slot ------------------------------
int amar_adam_f32(float *w, const float *g, float *m, float *v, int64_t n, float lr_t, float beta_1, float beta_2,
                  float epsilon, float l2, amar_stream_t stream) {
    if (n < 0 || !w || !g || !m || !v) return AMAR_EINVAL;
    if (n == 0) return AMAR_OK;
    hipLaunchKernelGGL(adam_host_step_kernel, dim3(grid_of(n)), dim3(256), 0, static_cast<hipStream_t>(stream), w, g, m, v, n, lr_t,
                       adam_hyper(0.f, beta_1, beta_2, epsilon), 2.f * l2);
    return amar_check_launch();
}

int amar_adam_advance_f32(float *state, float learning_rate, float beta_1, float beta_2, amar_stream_t stream) {
    if (!state) return AMAR_EINVAL;
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, AMAR_OPT_ADAM,
                       adam_hyper(learning_rate, beta_1, beta_2, 0.f));
    return amar_check_launch();
}

int amar_adam_dev_f32(float *w, const float *g, float *m, float *v, int64_t n, const float *state, float beta_1, float beta_2,
                      float epsilon, float l2, amar_stream_t stream) {
    if (n < 0 || !w || !g || !m || !v || !state) return AMAR_EINVAL;
    if (n == 0) return AMAR_OK;
    launch_single<V_ADAM>(w, g, m, v, nullptr, n, state, adam_hyper(0.f, beta_1, beta_2, epsilon), l2, static_cast<hipStream_t>(stream));
    return amar_check_launch();
}

int amar_adam_multi_f32(const amar_adam_slot *slots, int32_t n_slots, int64_t total_blocks, const float *state, float beta_1,
                        float beta_2, float epsilon, float reg_scale, float *loss_acc, amar_stream_t stream) {
    if (!slots || n_slots < 1 || total_blocks < 1 || total_blocks > 0x7fffffff || !state) return AMAR_EINVAL;
    launch_multi<V_ADAM>(slots, n_slots, total_blocks, state, adam_hyper(0.f, beta_1, beta_2, epsilon), reg_scale, loss_acc,
                         static_cast<hipStream_t>(stream));
    return amar_check_launch();
}

}  // extern "C"

// The optimizers of tf.keras.optimizers besides Adam (gfx950): SGD (momentum, Nesterov), RMSprop (momentum, centered), Adagrad, Adamax,
// Nadam and Adam(amsgrad=True), as include/amar_hip.h states them.  Same build as the Adam kernels of amar_train.hip, which stay as they
// are: a one-thread kernel advances the step counter and the step-dependent scalars in device memory (nothing that changes from step to
// step is baked into a captured training graph), ONE launch updates every parameter of a model from a slot table (adding the deferred
// weight-gradient partials in group order and the L2 part of the reported loss), and a single-tensor form reads the same device state.
// The rule is a template parameter: a rule loads and stores only the arrays it uses and nothing inside the element loop branches on it.
#include "amar_common.h"

namespace {

// A rule with its flags resolved: what the kernels are instantiated for.
enum Variant {
    V_SGD, V_SGD_MOM, V_SGD_NESTEROV, V_RMS, V_RMS_MOM, V_RMS_CENTERED, V_RMS_CENTERED_MOM, V_ADAGRAD, V_ADAMAX, V_NADAM, V_AMSGRAD, V_COUNT
};

__host__ __device__ constexpr int state_arrays_of(int v) {
    return v == V_SGD ? 0
         : (v == V_SGD_MOM || v == V_SGD_NESTEROV || v == V_RMS || v == V_ADAGRAD) ? 1
         : (v == V_RMS_MOM || v == V_RMS_CENTERED || v == V_ADAMAX || v == V_NADAM) ? 2 : 3;
}

// -1: not a rule, flags the rule does not have, or a momentum that is negative or NaN
int resolve_variant(int32_t rule, int32_t flags, float momentum) {
    if (!(momentum >= 0.f)) return -1;
    const bool mom = momentum > 0.f;
    switch (rule) {
    case AMAR_OPT_SGD:
        if (flags & ~AMAR_OPT_NESTEROV) return -1;
        return !mom ? V_SGD : ((flags & AMAR_OPT_NESTEROV) ? V_SGD_NESTEROV : V_SGD_MOM);     // (Keras: nesterov without momentum is plain SGD)
    case AMAR_OPT_RMSPROP:
        if (flags & ~AMAR_OPT_CENTERED) return -1;
        return (flags & AMAR_OPT_CENTERED) ? (mom ? V_RMS_CENTERED_MOM : V_RMS_CENTERED) : (mom ? V_RMS_MOM : V_RMS);
    case AMAR_OPT_ADAGRAD: return flags ? -1 : V_ADAGRAD;
    case AMAR_OPT_ADAMAX:  return flags ? -1 : V_ADAMAX;
    case AMAR_OPT_NADAM:   return flags ? -1 : V_NADAM;
    case AMAR_OPT_AMSGRAD: return flags ? -1 : V_AMSGRAD;
    default: return -1;
    }
}

// What an element update reads besides its own element: the hyper-parameters and the device state of this step (wave-uniform).
struct OptK { float step, momentum, rho, b1, b2, eps, mu_next, omb2, cg, cm; };

__device__ __forceinline__ OptK load_k(const float *__restrict__ state, const amar_optim_hyper h) {
    OptK k;
    k.step = state[1]; k.momentum = h.momentum; k.rho = h.rho; k.b1 = h.beta_1; k.b2 = h.beta_2; k.eps = h.epsilon;
    k.mu_next = state[3]; k.omb2 = state[5]; k.cg = state[6]; k.cm = state[7];
    return k;
}

// One update of one element, shared by optim_kernel and optim_multi_kernel: the two give the same bits on the same element (the header's
// promise).  As adam_step: the fused products are written out and nothing else may be fused, so the bits do not depend on the kernel
// around it.  s0..s2 are the rule's state arrays in the header's order; the ones a rule does not have are neither read nor written.
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
    } else {                                                          // V_AMSGRAD
        s0 = fmaf(k.b1, s0, (1.f - k.b1) * gi);
        s1 = fmaf(k.b2, s1, ((1.f - k.b2) * gi) * gi);
        s2 = fmaxf(s2, s1);
        w = w - (k.step * s0) / (sqrtf(s2) + k.eps);
    }
}

// state[0] = t + 1 and the scalars of that step, computed in double from the float32 hyper-parameters (as adam_advance_kernel); plain
// vector stores from the one thread.  Nadam's running product P_t lives in state[4]: P_t = P_{t-1} * mu_t with P_0 = 1 (t == 1 starts it).
__global__ void optim_advance_kernel(float *__restrict__ state, int rule, const amar_optim_hyper h) {
    const double t = (double)state[0] + 1.0;
    const double lr = (double)h.learning_rate, b1 = (double)h.beta_1, b2 = (double)h.beta_2;
    const double p_prev = t == 1.0 ? 1.0 : (double)state[4];
    double out[AMAR_OPTIM_STATE_FLOATS] = {t, lr, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (rule == AMAR_OPT_ADAMAX) {
        out[1] = lr / (1.0 - pow(b1, t));
    } else if (rule == AMAR_OPT_AMSGRAD) {
        out[1] = lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t));
    } else if (rule == AMAR_OPT_NADAM) {
        const double mu = b1 * (1.0 - 0.5 * pow(0.96, 0.004 * t)), mu_next = b1 * (1.0 - 0.5 * pow(0.96, 0.004 * (t + 1.0)));
        const double p = p_prev * mu;
        out[2] = mu; out[3] = mu_next; out[4] = p; out[5] = 1.0 - pow(b2, t);
        out[6] = lr * (1.0 - mu) / (1.0 - p);
        out[7] = lr * mu_next / (1.0 - p * mu_next);
    }
    for (int k = 0; k < AMAR_OPTIM_STATE_FLOATS; ++k) state[k] = (float)out[k];
}

template <int V>
__global__ __launch_bounds__(256) void optim_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ s0,
                                                    float *__restrict__ s1, float *__restrict__ s2, int64_t n,
                                                    const float *__restrict__ state, const amar_optim_hyper h, float l2x2) {
    constexpr int NS = state_arrays_of(V);
    const OptK k = load_k(state, h);
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

__device__ __forceinline__ void f4_to(float (&dst)[4], const float4 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
__device__ __forceinline__ float4 f4_from(const float (&src)[4]) { return make_float4(src[0], src[1], src[2], src[3]); }

// Every parameter of a model in ONE launch — adam_multi_kernel's build for the other rules: block b works on 1024 elements of the slot
// that owns it, all loads of a thread's four elements first, then the deferred partial gradients (loads before adds, the adds in group
// order), 16 bytes per lane where the slot's arrays allow it, one atomic per block into *loss_acc for the L2 part of the loss.
template <int V>
__global__ __launch_bounds__(256) void optim_multi_kernel(const amar_optim_slot *__restrict__ slots, int n_slots,
                                                          const float *__restrict__ state, const amar_optim_hyper h,
                                                          float reg_scale, float *__restrict__ loss_acc) {
    constexpr int NS = state_arrays_of(V);
    int sidx = 0;
    while (sidx + 1 < n_slots && (int64_t)blockIdx.x >= slots[sidx + 1].first_block) ++sidx;
    const amar_optim_slot sl = slots[sidx];
    const OptK k = load_k(state, h);
    const float l2x2 = 2.f * sl.l2;
    const int64_t base = ((int64_t)blockIdx.x - sl.first_block) * 1024;
    float *const sp[3] = {sl.s0, sl.s1, sl.s2};
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

template <int V>
void launch_multi(const amar_optim_slot *slots, int32_t n_slots, int64_t total_blocks, const float *state, const amar_optim_hyper &h,
                  float reg_scale, float *loss_acc, hipStream_t st) {
    hipLaunchKernelGGL(optim_multi_kernel<V>, dim3((unsigned)total_blocks), dim3(256), 0, st, slots, n_slots, state, h, reg_scale, loss_acc);
}

#define AMAR_FOR_EACH_VARIANT(CALL)                                                                                                      \
    switch (v) {                                                                                                                         \
    case V_SGD: CALL(V_SGD); break;                     case V_SGD_MOM: CALL(V_SGD_MOM); break;                                          \
    case V_SGD_NESTEROV: CALL(V_SGD_NESTEROV); break;   case V_RMS: CALL(V_RMS); break;                                                  \
    case V_RMS_MOM: CALL(V_RMS_MOM); break;             case V_RMS_CENTERED: CALL(V_RMS_CENTERED); break;                                \
    case V_RMS_CENTERED_MOM: CALL(V_RMS_CENTERED_MOM); break;                                                                            \
    case V_ADAGRAD: CALL(V_ADAGRAD); break;             case V_ADAMAX: CALL(V_ADAMAX); break;                                            \
    case V_NADAM: CALL(V_NADAM); break;                 default: CALL(V_AMSGRAD); break;                                                 \
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

}  // extern "C"

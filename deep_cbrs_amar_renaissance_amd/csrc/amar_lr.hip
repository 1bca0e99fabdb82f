// Learning-rate schedules on the device (gfx950), as include/amar_hip.h states them: the rate of a step is a function of the step counter
// that already lives in device memory, evaluated by the ONE thread that advances the optimizer state, inside that launch.  The rate is
// therefore no kernel argument: a captured training batch replays under a rate that follows the step count (a schedule) or that the host
// rewrites between replays (lr_state[0]: LearningRateScheduler, ReduceLROnPlateau) without being captured again.  The scalars of the
// step come from the function amar_adam_advance_f32 and amar_optim_advance_f32 call (amar_optim.h): a constant schedule gives their bits.
#include "amar_optim.h"

namespace {

// The rate of the zero-based step s: in double from the float32 parameters, rounded once to float32 (Keras holds the rate as float32).
// Contraction is off (as in optim_step): a host restatement without fused products follows it operation for operation.
__device__ __forceinline__ float lr_rate(const amar_lr_schedule &sc, const float *__restrict__ lr_state, double s) {
#pragma clang fp contract(off)
    const double lr0 = (double)sc.initial_learning_rate, d = (double)sc.decay_steps;
    switch (sc.kind) {
    case AMAR_LR_EXPONENTIAL: {
        double p = s / d;
        if (sc.flags & AMAR_LR_STAIRCASE) p = floor(p);
        return (float)(lr0 * pow((double)sc.decay_rate, p));
    }
    case AMAR_LR_INVERSE_TIME: {
        double p = s / d;
        if (sc.flags & AMAR_LR_STAIRCASE) p = floor(p);
        return (float)(lr0 / (1.0 + (double)sc.decay_rate * p));
    }
    case AMAR_LR_POLYNOMIAL: {
        const double end = (double)sc.end_learning_rate;
        double p;
        if (sc.flags & AMAR_LR_CYCLE) p = s / (d * (s == 0.0 ? 1.0 : ceil(s / d)));
        else p = fmin(s, d) / d;
        return (float)((lr0 - end) * pow(1.0 - p, (double)sc.power) + end);
    }
    case AMAR_LR_COSINE: {
        const double alpha = (double)sc.alpha;
        const double c = 0.5 * (1.0 + cos(3.14159265358979323846 * (fmin(s, d) / d)));
        return (float)(lr0 * ((1.0 - alpha) * c + alpha));
    }
    case AMAR_LR_PIECEWISE: {
        int i = 0;
        while (i < sc.n_boundaries && s > (double)sc.boundaries[i]) ++i;
        return sc.values[i];
    }
    default:                                                          // AMAR_LR_CONSTANT: the base rate, which the host writes
        return lr_state[0];
    }
}

__global__ __launch_bounds__(256) void lr_rates_kernel(const amar_lr_schedule sc, const float *__restrict__ lr_state, int64_t first_step,
                                                       int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = lr_rate(sc, lr_state, (double)(first_step + i));
}

// optim_advance_kernel (amar_optim.hip) with the rate of step s = state[0] in place of h.learning_rate, which is not read.
__global__ void optim_advance_lr_kernel(float *__restrict__ state, int rule, const amar_optim_hyper h, const amar_lr_schedule sc,
                                        float *__restrict__ lr_state) {
    const float rate = lr_rate(sc, lr_state, (double)state[0]);
    lr_state[1] = rate;
    optim_advance_state(state, rule, rate, h);
}

// what the header asks of a schedule (NaN parameters fail the comparisons and are refused with them)
bool schedule_ok(const amar_lr_schedule *sc) {
    if (!sc) return false;
    switch (sc->kind) {
    case AMAR_LR_CONSTANT:     return sc->flags == 0;
    case AMAR_LR_EXPONENTIAL:
    case AMAR_LR_INVERSE_TIME: return !(sc->flags & ~AMAR_LR_STAIRCASE) && sc->decay_steps > 0.f;
    case AMAR_LR_POLYNOMIAL:   return !(sc->flags & ~AMAR_LR_CYCLE) && sc->decay_steps > 0.f;
    case AMAR_LR_COSINE:       return sc->flags == 0 && sc->decay_steps > 0.f;
    case AMAR_LR_PIECEWISE:    return sc->flags == 0 && sc->n_boundaries >= 1 && sc->n_boundaries <= AMAR_LR_MAX_BOUNDARIES;
    default:                   return false;
    }
}

}  // namespace

extern "C" {

int amar_lr_rates_f32(const amar_lr_schedule *sched, const float *lr_state, int64_t first_step, int64_t n, float *out, amar_stream_t stream) {
    if (!schedule_ok(sched) || !lr_state || first_step < 0 || n < 0 || first_step + n > AMAR_LR_MAX_STEP || (n > 0 && !out)) return AMAR_EINVAL;
    if (n == 0) return AMAR_OK;
    hipLaunchKernelGGL(lr_rates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), *sched, lr_state,
                       first_step, n, out);
    return amar_check_launch();
}

int amar_adam_advance_lr_f32(float *state, const amar_lr_schedule *sched, float *lr_state, float beta_1, float beta_2, amar_stream_t stream) {
    if (!state || !schedule_ok(sched) || !lr_state) return AMAR_EINVAL;
    hipLaunchKernelGGL(optim_advance_lr_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, AMAR_OPT_ADAM,
                       adam_hyper(0.f, beta_1, beta_2, 0.f), *sched, lr_state);
    return amar_check_launch();
}

int amar_optim_advance_lr_f32(float *state, int32_t rule, int32_t flags, const amar_optim_hyper *hyper, const amar_lr_schedule *sched,
                              float *lr_state, amar_stream_t stream) {
    if (!state || !hyper || resolve_variant(rule, flags, hyper->momentum) < 0 || !schedule_ok(sched) || !lr_state) return AMAR_EINVAL;
    hipLaunchKernelGGL(optim_advance_lr_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, (int)rule, *hyper, *sched,
                       lr_state);
    return amar_check_launch();
}

}  // extern "C"

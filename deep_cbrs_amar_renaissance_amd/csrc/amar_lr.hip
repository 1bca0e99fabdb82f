// Learning-rate schedules on the device (gfx950), as include/amar_hip.h states them: the rate of a step is a function of the step counter
// that already lives in device memory, evaluated by the ONE thread that advances the optimizer state, inside that launch.  The rate is
// therefore no kernel argument: a captured training batch replays under a rate that follows the step count (a schedule) or that the host
// rewrites between replays (lr_state[0]: LearningRateScheduler, ReduceLROnPlateau) without being captured again.  amar_adam_advance_f32 and
// amar_optim_advance_f32 stay as they are; their step-dependent scalars are restated here expression for expression, under the same build
// flags, so that a constant schedule gives their bits.
#include "amar_common.h"

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

// adam_advance_kernel (amar_train.hip) with the rate of step s = state[0] in place of its argument; plain vector stores from the one thread.
__global__ void adam_advance_lr_kernel(float *__restrict__ state, const amar_lr_schedule sc, float *__restrict__ lr_state, float b1, float b2) {
    const float lr = lr_rate(sc, lr_state, (double)state[0]);
    lr_state[1] = lr;
    const double t = (double)state[0] + 1.0;
    state[0] = (float)t;
    state[1] = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
}

// optim_advance_kernel (amar_optim.hip) in the same way; h.learning_rate is not read.
__global__ void optim_advance_lr_kernel(float *__restrict__ state, int rule, const amar_optim_hyper h, const amar_lr_schedule sc,
                                        float *__restrict__ lr_state) {
    const float rate = lr_rate(sc, lr_state, (double)state[0]);
    lr_state[1] = rate;
    const double t = (double)state[0] + 1.0;
    const double lr = (double)rate, b1 = (double)h.beta_1, b2 = (double)h.beta_2;
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

// the argument checks of amar_optim_advance_f32 (resolve_variant of amar_optim.hip, restated: that file stays as it is)
bool rule_ok(int32_t rule, int32_t flags, float momentum) {
    if (!(momentum >= 0.f)) return false;
    switch (rule) {
    case AMAR_OPT_SGD:     return !(flags & ~AMAR_OPT_NESTEROV);
    case AMAR_OPT_RMSPROP: return !(flags & ~AMAR_OPT_CENTERED);
    case AMAR_OPT_ADAGRAD: case AMAR_OPT_ADAMAX: case AMAR_OPT_NADAM: case AMAR_OPT_AMSGRAD: return flags == 0;
    default: return false;
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
    hipLaunchKernelGGL(adam_advance_lr_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, *sched, lr_state, beta_1, beta_2);
    return amar_check_launch();
}

int amar_optim_advance_lr_f32(float *state, int32_t rule, int32_t flags, const amar_optim_hyper *hyper, const amar_lr_schedule *sched,
                              float *lr_state, amar_stream_t stream) {
    if (!state || !hyper || !rule_ok(rule, flags, hyper->momentum) || !schedule_ok(sched) || !lr_state) return AMAR_EINVAL;
    hipLaunchKernelGGL(optim_advance_lr_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, (int)rule, *hyper, *sched,
                       lr_state);
    return amar_check_launch();
}

}  // extern "C"

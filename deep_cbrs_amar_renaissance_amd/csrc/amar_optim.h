// What the optimizer files share (amar_optim.hip: the update kernels and the advance entry points that take the rate as an argument;
// amar_lr.hip: the advance entry points that evaluate a schedule): the rules with their flags resolved, the one check of a rule and its
// flags, and the one function that computes the scalars of a step.
#pragma once
#include "amar_common.h"

namespace {

// A rule with its flags resolved: what the kernels are instantiated for.
enum Variant {
    V_SGD, V_SGD_MOM, V_SGD_NESTEROV, V_RMS, V_RMS_MOM, V_RMS_CENTERED, V_RMS_CENTERED_MOM, V_ADAGRAD, V_ADAMAX, V_NADAM, V_AMSGRAD, V_ADAM,
    V_COUNT
};

__host__ __device__ constexpr int state_arrays_of(int v) {
    return v == V_SGD ? 0
         : (v == V_SGD_MOM || v == V_SGD_NESTEROV || v == V_RMS || v == V_ADAGRAD) ? 1
         : (v == V_RMS_MOM || v == V_RMS_CENTERED || v == V_ADAMAX || v == V_NADAM || v == V_ADAM) ? 2 : 3;
}

// -1: not a rule, flags the rule does not have, or a momentum that is negative or NaN
inline int resolve_variant(int32_t rule, int32_t flags, float momentum) {
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
    case AMAR_OPT_ADAM:    return flags ? -1 : V_ADAM;
    default: return -1;
    }
}

// The hyper-parameters of the amar_adam_* entry points as the shared kernels take them (Adam reads beta_1, beta_2 and epsilon).
inline amar_optim_hyper adam_hyper(float learning_rate, float beta_1, float beta_2, float epsilon) {
    return amar_optim_hyper{learning_rate, 0.f, 0.f, beta_1, beta_2, epsilon};
}

// One thread opens step t = state[0] + 1 under the rate `rate`: state[0] = t and the scalars of that step, computed in double from the
// float32 rate and hyper-parameters; plain vector stores.  Nadam's running product P_t lives in state[4]: P_t = P_{t-1} * mu_t with
// P_0 = 1 (t == 1 starts it); no other rule reads it.  Adam's state is the two floats the amar_adam_* entry points document: it writes
// [0] and [1] and touches nothing above them; every other rule writes all AMAR_OPTIM_STATE_FLOATS.
__device__ __forceinline__ void optim_advance_state(float *__restrict__ state, int rule, float rate, const amar_optim_hyper &h) {
    const double t = (double)state[0] + 1.0;
    const double lr = (double)rate, b1 = (double)h.beta_1, b2 = (double)h.beta_2;
    double out[AMAR_OPTIM_STATE_FLOATS] = {t, lr, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (rule == AMAR_OPT_ADAMAX) {
        out[1] = lr / (1.0 - pow(b1, t));
    } else if (rule == AMAR_OPT_AMSGRAD || rule == AMAR_OPT_ADAM) {
        out[1] = lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t));
    } else if (rule == AMAR_OPT_NADAM) {
        const double p_prev = t == 1.0 ? 1.0 : (double)state[4];
        const double mu = b1 * (1.0 - 0.5 * pow(0.96, 0.004 * t)), mu_next = b1 * (1.0 - 0.5 * pow(0.96, 0.004 * (t + 1.0)));
        const double p = p_prev * mu;
        out[2] = mu; out[3] = mu_next; out[4] = p; out[5] = 1.0 - pow(b2, t);
        out[6] = lr * (1.0 - mu) / (1.0 - p);
        out[7] = lr * mu_next / (1.0 - p * mu_next);
    }
    state[0] = (float)out[0]; state[1] = (float)out[1];
    if (rule != AMAR_OPT_ADAM)
        for (int k = 2; k < AMAR_OPTIM_STATE_FLOATS; ++k) state[k] = (float)out[k];
}

}  // namespace

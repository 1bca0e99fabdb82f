// The compiled loss and the compiled metrics of a training batch (gfx950): Model.compile(loss=..., metrics=...).
//
// amar_loss_grad_f32 stands where amar_bce_grad_f32 (amar_train.hip) and amar_bpr_grad_f32 (amar_bpr.hip) stand: one lane per pair,
// loss_terms[i] = the pair's term (sum = B x batch loss), dz[i] = d(mean loss)/d(logit) through the final sigmoid.  The loss is a
// template argument, so every instance is the straight-line code of its own formula; AMAR_LOSS_BCE without smoothing is
// bce_grad_kernel's expressions letter for letter and gives its bits.  With a counter block the same launch also counts the batch
// for accuracy / Precision / Recall (a confusion matrix at 0.5) and AUC (a 2 x 199 histogram over Keras' 200 thresholds): integer
// sums only — per-wavefront, LDS, then one global pass per workgroup — so the counters are the same bits whatever order workgroups
// arrive in.  No float atomics anywhere.
#include "amar_common.h"

namespace {

struct LossHyper { float label_smoothing, shape, alpha, balance; };   // shape = delta (Huber) or gamma (focal)

constexpr int LOSS_BCE_SMOOTH = AMAR_LOSS_FOCAL + 1;                   // AMAR_LOSS_BCE with label_smoothing != 0 (host-side choice)

// AUC(num_thresholds=200): the interior thresholds are float32(k / 199.0), k = 1..198, the division in double as Python does it
// (keras/metrics: (i + 1) * 1.0 / (num_thresholds - 1)); entry 0 is not a threshold.
struct AucThresholds { float v[AMAR_AUC_BUCKETS]; };
constexpr AucThresholds make_auc_thresholds() {
    AucThresholds t{};
    for (int k = 1; k < AMAR_AUC_BUCKETS; ++k) t.v[k] = (float)((double)k / (double)AMAR_AUC_BUCKETS);
    return t;
}
__constant__ AucThresholds auc_thr = make_auc_thresholds();

// How many interior thresholds p exceeds (0..198): an arithmetic candidate, corrected against the table so that the result agrees
// with the comparison p > float32(k / 199) for every float p (a NaN exceeds none).
__device__ __forceinline__ int auc_bucket(float p) {
    int b = (int)(fminf(fmaxf(p, 0.f), 1.f) * (float)AMAR_AUC_BUCKETS);   // (fmaxf drops a NaN: the conversion always has a value)
    b = b > AMAR_AUC_BUCKETS - 1 ? AMAR_AUC_BUCKETS - 1 : b;
    while (b < AMAR_AUC_BUCKETS - 1 && p > auc_thr.v[b + 1]) ++b;
    while (b > 0 && !(p > auc_thr.v[b])) --b;
    return b;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int off = AMAR_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, AMAR_WAVE);
    return v;                                                          // lane 0 holds the wavefront's sum
}

// Keras' binary_crossentropy on probabilities for the (possibly smoothed) label yi: bce_grad_kernel's expressions.
__device__ __forceinline__ void bce_pair(float pi, float yi, float &term, float &dp) {
    const float eps = 1e-7f;
    const float pc = fminf(fmaxf(pi, eps), 1.f - eps);
    term = -(yi * logf(pc + eps) + (1.f - yi) * logf(1.f - pc + eps));
    const bool inside = pi >= eps && pi <= 1.f - eps;
    dp = inside ? -(yi / (pc + eps) - (1.f - yi) / (1.f - pc + eps)) : 0.f;
}

// term = the pair's loss, dp = d(term)/dp.  e = p - y, s = 2y - 1 (Keras' hinge losses move 0/1 labels to -1/+1).
template <int CODE>
__device__ __forceinline__ void loss_pair(const LossHyper &hp, float pi, float yi, float &term, float &dp) {
    const float e = pi - yi;
    if (CODE == AMAR_LOSS_MSE) {
        term = e * e;
        dp = 2.f * e;
    } else if (CODE == AMAR_LOSS_MAE) {
        term = fabsf(e);
        dp = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
    } else if (CODE == AMAR_LOSS_HINGE || CODE == AMAR_LOSS_SQUARED_HINGE) {
        const float s = 2.f * yi - 1.f;
        const float m = fmaxf(1.f - s * pi, 0.f);
        if (CODE == AMAR_LOSS_HINGE) {
            term = m;
            dp = m > 0.f ? -s : 0.f;
        } else {
            term = m * m;
            dp = -2.f * s * m;
        }
    } else if (CODE == AMAR_LOSS_HUBER) {
        const float d = hp.shape, a = fabsf(e);
        const bool quad = a <= d;
        term = quad ? 0.5f * e * e : d * a - 0.5f * d * d;
        dp = quad ? e : (e > 0.f ? d : -d);
    } else if (CODE == AMAR_LOSS_LOG_COSH) {
        // e + softplus(-2e) - log 2 = log cosh e = log1p(2 sinh^2(e / 2)): the form that keeps its digits where e is small
        const float sh = sinhf(0.5f * e);
        term = log1pf(2.f * sh * sh);
        dp = tanhf(e);
    } else if (CODE == AMAR_LOSS_POISSON) {
        const float q = pi + 1e-7f;
        term = pi - yi * logf(q);
        dp = 1.f - yi / q;
    } else if (CODE == AMAR_LOSS_FOCAL) {
        const float ls = hp.label_smoothing, g = hp.shape;
        const float ys = yi * (1.f - ls) + 0.5f * ls;
        float bce, dbce;
        bce_pair(pi, ys, bce, dbce);
        // 1 - p_t = ys (1 - p) + (1 - ys) p: the same number without the cancellation of 1 - (ys p + (1 - ys)(1 - p)) at small p
        const float q = fmaxf(ys * (1.f - pi) + (1.f - ys) * pi, 0.f);
        const float w = hp.balance != 0.f ? ys * hp.alpha + (1.f - ys) * (1.f - hp.alpha) : 1.f;
        const float ff = powf(q, g);
        // d(1 - p_t)/dp = 1 - 2 ys;  q^(g - 1) at q = 0 is taken as 0 for g > 1 and 1 for g = 1 (powf), never a division
        const float dff = g == 0.f ? 0.f : g * powf(q, g - 1.f) * (1.f - 2.f * ys);
        term = w * ff * bce;
        dp = w * (dff * bce + ff * dbce);
    }
}

// WEIGHTED: the pair's weight w = sample_w[i] * class_w[y[i] > 0.5] (a missing factor is 1) multiplies the finished term and the
// finished dz as the LAST float32 operation, so a weighted output is float32(w x the unweighted output) and w = 1 gives its bits.
// The class is read from the 0/1 label itself, before any smoothing; the counters do not see the weights.
template <int CODE, bool COUNT, bool WEIGHTED>
__global__ __launch_bounds__(256) void loss_grad_kernel(LossHyper hp, const float *__restrict__ p, int64_t ldp, const float *__restrict__ y,
                                                        float *__restrict__ dz, float *__restrict__ loss_terms, int64_t B,
                                                        unsigned long long *__restrict__ counters, const float *__restrict__ sample_w,
                                                        const float *__restrict__ class_w) {
    __shared__ unsigned cells[COUNT ? AMAR_LOSS_COUNTERS : 1];
    unsigned tp = 0, fp = 0, tn = 0, fn = 0;
    if (COUNT) {
        for (int c = threadIdx.x; c < AMAR_LOSS_COUNTERS; c += blockDim.x) cells[c] = 0u;
        __syncthreads();
    }
    const float eps = 1e-7f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const float pi = p[i * ldp], yi = y[i];
        float wi = 1.f;
        if constexpr (WEIGHTED) wi = (sample_w ? sample_w[i] : 1.f) * (class_w ? class_w[yi > 0.5f ? 1 : 0] : 1.f);
        if constexpr (CODE == AMAR_LOSS_BCE) {
            const float pc = fminf(fmaxf(pi, eps), 1.f - eps);
            const float term = -(yi * logf(pc + eps) + (1.f - yi) * logf(1.f - pc + eps));
            loss_terms[i] = WEIGHTED ? wi * term : term;
            const bool inside = pi >= eps && pi <= 1.f - eps;
            const float dp = inside ? -(yi / (pc + eps) - (1.f - yi) / (1.f - pc + eps)) / (float)B : 0.f;
            const float g = dp * pi * (1.f - pi);                        // through the sigmoid of the last Dense layer
            dz[i] = WEIGHTED ? wi * g : g;
        } else {
            float term, dp;
            if constexpr (CODE == LOSS_BCE_SMOOTH) bce_pair(pi, yi * (1.f - hp.label_smoothing) + 0.5f * hp.label_smoothing, term, dp);
            else loss_pair<CODE>(hp, pi, yi, term, dp);
            loss_terms[i] = WEIGHTED ? wi * term : term;
            const float through = pi * (1.f - pi);                       // a probability of exactly 0 or 1 passes nothing back
            const float g = through == 0.f ? 0.f : dp / (float)B * through;
            dz[i] = WEIGHTED ? wi * g : g;
        }
        if (COUNT) {
            const bool actual = yi > 0.5f, predicted = pi > 0.5f;
            tp += actual && predicted;
            fp += !actual && predicted;
            tn += !actual && !predicted;
            fn += actual && !predicted;
            atomicAdd(&cells[4 + (actual ? AMAR_AUC_BUCKETS : 0) + auc_bucket(pi)], 1u);
        }
    }
    if (COUNT) {
        tp = wave_sum_u32(tp); fp = wave_sum_u32(fp); tn = wave_sum_u32(tn); fn = wave_sum_u32(fn);
        if ((threadIdx.x & (AMAR_WAVE - 1)) == 0) {
            if (tp) atomicAdd(&cells[0], tp);
            if (fp) atomicAdd(&cells[1], fp);
            if (tn) atomicAdd(&cells[2], tn);
            if (fn) atomicAdd(&cells[3], fn);
        }
        __syncthreads();
        for (int c = threadIdx.x; c < AMAR_LOSS_COUNTERS; c += blockDim.x) {
            const unsigned v = cells[c];
            if (v) atomicAdd(&counters[c], (unsigned long long)v);
        }
    }
}

template <int CODE, bool WEIGHTED>
void launch_counted(bool count, unsigned grid, hipStream_t st, const LossHyper &hp, const float *p, int64_t ldp, const float *y,
                    const float *sw, const float *cw, float *dz, float *terms, int64_t B, unsigned long long *counters) {
    if (count) hipLaunchKernelGGL((loss_grad_kernel<CODE, true, WEIGHTED>), dim3(grid), dim3(256), 0, st, hp, p, ldp, y, dz, terms, B, counters, sw, cw);
    else hipLaunchKernelGGL((loss_grad_kernel<CODE, false, WEIGHTED>), dim3(grid), dim3(256), 0, st, hp, p, ldp, y, dz, terms, B, counters, sw, cw);
}

template <int CODE>
void launch(bool count, unsigned grid, hipStream_t st, const LossHyper &hp, const float *p, int64_t ldp, const float *y, const float *sw,
            const float *cw, float *dz, float *terms, int64_t B, unsigned long long *counters) {
    if (sw || cw) launch_counted<CODE, true>(count, grid, st, hp, p, ldp, y, sw, cw, dz, terms, B, counters);
    else launch_counted<CODE, false>(count, grid, st, hp, p, ldp, y, nullptr, nullptr, dz, terms, B, counters);
}

// The body of both entry points: sw = cw = NULL launches the unweighted instances.
int loss_grad(int32_t loss, const float *hyper, const float *p, int64_t ldp, const float *y, const float *sw, const float *cw, float *dz,
              float *loss_terms, int64_t B, int64_t *counters, amar_stream_t stream) {
    if (B < 1 || !p || !y || !dz || !loss_terms || ldp < 1 || loss < AMAR_LOSS_BCE || loss > AMAR_LOSS_FOCAL) return AMAR_EINVAL;
    LossHyper hp = {0.f, loss == AMAR_LOSS_FOCAL ? 2.f : 1.f, 0.25f, 0.f};
    if (hyper) hp = {hyper[0], hyper[1], hyper[2], hyper[3]};
    if (!(hp.label_smoothing >= 0.f && hp.label_smoothing <= 1.f)) return AMAR_EINVAL;
    if ((loss == AMAR_LOSS_HUBER || loss == AMAR_LOSS_FOCAL) && !(hp.shape >= 0.f)) return AMAR_EINVAL;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t blocks = (B + 255) / 256;                                  // (bce_grad_kernel's grid)
    const unsigned grid = (unsigned)(blocks > 8192 ? 8192 : blocks);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counters);
    const bool count = counters != nullptr;
    switch (loss) {
    case AMAR_LOSS_BCE:
        if (hp.label_smoothing != 0.f) launch<LOSS_BCE_SMOOTH>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt);
        else launch<AMAR_LOSS_BCE>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt);
        break;
    case AMAR_LOSS_MSE: launch<AMAR_LOSS_MSE>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    case AMAR_LOSS_MAE: launch<AMAR_LOSS_MAE>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    case AMAR_LOSS_HINGE: launch<AMAR_LOSS_HINGE>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    case AMAR_LOSS_SQUARED_HINGE: launch<AMAR_LOSS_SQUARED_HINGE>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    case AMAR_LOSS_HUBER: launch<AMAR_LOSS_HUBER>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    case AMAR_LOSS_LOG_COSH: launch<AMAR_LOSS_LOG_COSH>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    case AMAR_LOSS_POISSON: launch<AMAR_LOSS_POISSON>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    default: launch<AMAR_LOSS_FOCAL>(count, grid, st, hp, p, ldp, y, sw, cw, dz, loss_terms, B, cnt); break;
    }
    return amar_check_launch();
}

}  // namespace

int32_t amar_loss_counters(void) { return AMAR_LOSS_COUNTERS; }

int amar_loss_grad_f32(int32_t loss, const float *hyper, const float *p, int64_t ldp, const float *y, float *dz, float *loss_terms,
                       int64_t B, int64_t *counters, amar_stream_t stream) {
    return loss_grad(loss, hyper, p, ldp, y, nullptr, nullptr, dz, loss_terms, B, counters, stream);
}

int amar_loss_grad_weighted_f32(int32_t loss, const float *hyper, const float *p, int64_t ldp, const float *y, const float *sample_w,
                                const float *class_w, float *dz, float *loss_terms, int64_t B, int64_t *counters, amar_stream_t stream) {
    if (!sample_w && !class_w) return AMAR_EINVAL;
    return loss_grad(loss, hyper, p, ldp, y, sample_w, class_w, dz, loss_terms, B, counters, stream);
}

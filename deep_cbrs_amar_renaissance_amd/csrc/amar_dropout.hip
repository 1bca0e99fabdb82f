// Training-time dropout on node tables (gfx950).  No mask is stored: the keep bits are a function of (seed, step, site, element)
// through Philox4x32-10 (amar_philox.h states the draw), so the reverse pass applies the same entry to the gradient slice and
// regenerates them.  `step` lives in device memory: a captured training graph drops other elements at every replay.
#include "amar_common.h"
#include "amar_philox.h"

namespace {

// One Philox call per four consecutive columns of a row (16 bytes).  VEC: both slices are 16-byte aligned with leading dimensions
// and a width that are multiples of 4, so a quad is one float4 access; otherwise element by element (the words of the last call of
// a row past its width are not used).
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float *X, int64_t ldx, float *Y, int64_t ldy,        // (X == Y: in place)
                                                      uint32_t n_quads, uint32_t qpr, int32_t C, const AmarDropout d) {
    const uint64_t s = *d.step;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < n_quads; e += gridDim.x * 256u) {
        const uint32_t r = e / qpr, c0 = 4u * (e - r * qpr);
        uint32_t w[4] = {e, (uint32_t)s, (uint32_t)(s >> 32), d.site << 24};
        philox4x32_10(w, d.key0, d.key1);
        const float *x = X + (int64_t)r * ldx + c0;
        float *y = Y + (int64_t)r * ldy + c0;
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4 *>(x);
            *reinterpret_cast<float4 *>(y) = make_float4(w[0] >= d.threshold ? v.x * d.scale : 0.f, w[1] >= d.threshold ? v.y * d.scale : 0.f,
                                                         w[2] >= d.threshold ? v.z * d.scale : 0.f, w[3] >= d.threshold ? v.w * d.scale : 0.f);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((int32_t)c0 + k < C) y[k] = w[k] >= d.threshold ? x[k] * d.scale : 0.f;
        }
    }
}

__global__ void dropout_advance_kernel(uint64_t *step) { *step += 1; }

}  // namespace

int amar_dropout_f32(const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t n_rows, int32_t C,
                     uint64_t seed, const uint64_t *step, uint32_t site, uint32_t threshold, float scale, amar_stream_t stream) {
    if (n_rows < 0 || C < 1 || !X || !Y || !step || ldx < C || ldy < C || site < 1 || site > 255 || !(scale >= 1.f) || scale > 3.0e38f)
        return AMAR_EINVAL;
    if (n_rows == 0) return AMAR_OK;
    const int64_t qpr = (C + 3) / 4, n_quads = n_rows * qpr;
    if (n_quads >= ((int64_t)1 << 31)) return AMAR_EUNSUPPORTED;      // the element index is one counter word (and e + stride must not wrap)
    const AmarDropout d{(uint32_t)seed, (uint32_t)(seed >> 32), step, site, threshold, scale};
    const bool vec = !(C & 3) && !(ldx & 3) && !(ldy & 3) && amar_aligned16(X) && amar_aligned16(Y);
    const dim3 grid((unsigned)((n_quads + 255) / 256 < 65536 ? (n_quads + 255) / 256 : 65536)), block(256);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(dropout_kernel<true>, grid, block, 0, st, X, ldx, Y, ldy, (uint32_t)n_quads, (uint32_t)qpr, C, d);
    else hipLaunchKernelGGL(dropout_kernel<false>, grid, block, 0, st, X, ldx, Y, ldy, (uint32_t)n_quads, (uint32_t)qpr, C, d);
    return amar_check_launch();
}

int amar_dropout_advance(uint64_t *step, amar_stream_t stream) {
    if (!step) return AMAR_EINVAL;
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), step);
    return amar_check_launch();
}

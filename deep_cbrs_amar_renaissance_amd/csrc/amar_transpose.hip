// Stable transpose of an int32 CSR structure on the device (amar_csr_transpose_i32, see include/amar_hip.h).
//
// The result is defined exactly — inside output row j the entries stand in the order of their input positions — so it must not
// depend on the order the hardware schedules waves in.  Five launches:
//
//   csrt_count_kernel    t_rowptr[c + 1] += 1 per entry of column c.  Integer adds commute: the counts are exact in any order.
//   csrt_scan_kernel     inclusive scan of the counts in place (one workgroup, a contiguous chunk per lane), and a copy of every
//                        row start into the fill cursors
//   csrt_scatter_kernel  perm[cursor[c]++] = p.  After it every output row holds the right SET of input positions in the order
//                        the adds arrived ...
//   csrt_sort_kernel     ... which this launch removes: the positions of a row are unique, so sorting them ascending IS the stable
//                        order.  One workgroup per output row: a bitonic network in LDS for rows of up to 8 192 entries, the same
//                        network in place in global memory for a longer row (a hub column of 100 000 entries and more)
//   csrt_rows_kernel     t_colidx[q] = the input row that holds position perm[q] (binary search in rowptr)
//
// It runs once per graph, outside any captured hipGraph, and is not tuned further than that: a typical output row (an item's few
// hundred raters) is one LDS sort.  Only vector atomics (global_atomic_add on int32), no float atomics.
#include "amar_common.h"
#include <limits.h>

namespace {

constexpr int CSRT_BLOCK = 256;
constexpr int CSRT_SCAN_BLOCK = 1024;
constexpr int CSRT_LDS_ROW = 8192;                     // entries of an output row sorted in LDS (32 KB)

int csrt_grid(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// A column outside [0, n_cols) is skipped here and in the scatter (nothing is ever written out of bounds); the result is then
// unspecified, and the Python wrapper refuses such input before the call.
__global__ __launch_bounds__(CSRT_BLOCK) void csrt_count_kernel(const int32_t *__restrict__ colidx, int64_t nnz, int32_t n_cols,
                                                                int32_t *__restrict__ t_rowptr) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = colidx[p];
        if (c >= 0 && c < n_cols) atomicAdd(t_rowptr + c + 1, 1);
    }
}

// counts[0] = 0, counts[1 .. n] = per-column counts  ->  counts[k] = sum of the first k counts; cursor[c] = counts[c].
__global__ __launch_bounds__(CSRT_SCAN_BLOCK) void csrt_scan_kernel(int32_t *__restrict__ counts, int32_t n, int32_t *__restrict__ cursor) {
    __shared__ int32_t part[CSRT_SCAN_BLOCK];
    const int t = threadIdx.x;
    const int64_t chunk = ((int64_t)n + CSRT_SCAN_BLOCK - 1) / CSRT_SCAN_BLOCK;
    const int64_t lo = 1 + (int64_t)t * chunk;
    const int64_t hi = lo + chunk < (int64_t)n + 1 ? lo + chunk : (int64_t)n + 1;
    int32_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += counts[k];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < CSRT_SCAN_BLOCK; d <<= 1) {    // Hillis-Steele over the 1 024 chunk sums
        const int32_t add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int32_t run = part[t] - sum;                       // everything before this lane's chunk
    for (int64_t k = lo; k < hi; ++k) {
        cursor[k - 1] = run;                           // start of output row k - 1
        run += counts[k];
        counts[k] = run;
    }
}

__global__ __launch_bounds__(CSRT_BLOCK) void csrt_scatter_kernel(const int32_t *__restrict__ colidx, int64_t nnz, int32_t n_cols,
                                                                  int32_t *__restrict__ cursor, int32_t *__restrict__ perm) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = colidx[p];
        if (c >= 0 && c < n_cols) perm[atomicAdd(cursor + c, 1)] = (int32_t)p;
    }
}

// Ascending bitonic network in its "flip" form: the first step of a merge of width k pairs i with i ^ (2k - 1), the others i
// with i ^ j — every compare-exchange leaves the smaller value at the lower index.  Indices >= len stand for +infinity: such a
// slot never wins a comparison against a real one, so pairs that reach past the end are skipped and no padding is stored.
__device__ __forceinline__ void csrt_bitonic(int32_t *v, unsigned len) {
    unsigned pow2 = 1;
    while (pow2 < len) pow2 <<= 1;                     // len < 2^31: no overflow
    const unsigned half = pow2 >> 1;
    for (unsigned k = 1; k < pow2; k <<= 1) {
        for (unsigned j = k; j >= 1; j >>= 1) {
            for (unsigned t = threadIdx.x; t < half; t += CSRT_BLOCK) {
                const unsigned lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // bit j of the pair's lower index is clear
                const unsigned hi = j == k ? lo ^ (2 * k - 1) : lo | j;
                if (hi < len) {
                    const int32_t a = v[lo], b = v[hi];
                    if (a > b) { v[lo] = b; v[hi] = a; }
                }
            }
            __syncthreads();                           // (workgroup scope: orders the LDS and the global form alike)
        }
    }
}

__global__ __launch_bounds__(CSRT_BLOCK) void csrt_sort_kernel(const int32_t *__restrict__ t_rowptr, int32_t n_cols, int32_t *perm) {
    __shared__ int32_t tile[CSRT_LDS_ROW];
    for (int row = blockIdx.x; row < n_cols; row += gridDim.x) {     // uniform over the workgroup
        const int beg = t_rowptr[row], len = t_rowptr[row + 1] - beg;
        if (len < 2) continue;
        if (len > CSRT_LDS_ROW) {
            csrt_bitonic(perm + beg, (unsigned)len);
            continue;
        }
        for (int t = threadIdx.x; t < len; t += CSRT_BLOCK) tile[t] = perm[beg + t];
        __syncthreads();
        csrt_bitonic(tile, (unsigned)len);
        for (int t = threadIdx.x; t < len; t += CSRT_BLOCK) perm[beg + t] = tile[t];
        __syncthreads();                               // the tile is reused by the next row
    }
}

__global__ __launch_bounds__(CSRT_BLOCK) void csrt_rows_kernel(const int32_t *__restrict__ rowptr, int32_t n_rows,
                                                               const int32_t *__restrict__ perm, int64_t nnz,
                                                               int32_t *__restrict__ t_colidx) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = perm[q];
        int lo = 0, hi = n_rows - 1;                   // the last row with rowptr[row] <= p (empty rows share a start: the last one holds it)
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (rowptr[mid] <= p) lo = mid; else hi = mid - 1;
        }
        t_colidx[q] = lo;
    }
}

}  // namespace

extern "C" {

int amar_csr_transpose_i32(const int32_t *rowptr, const int32_t *colidx, int32_t n_rows, int32_t n_cols, int32_t nnz,
                           int32_t *t_rowptr, int32_t *t_colidx, int32_t *perm, int32_t *cursor, amar_stream_t stream) {
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || !rowptr || !t_rowptr) return AMAR_EINVAL;
    if (nnz > 0 && (n_rows < 1 || n_cols < 1 || !colidx || !t_colidx || !perm || !cursor)) return AMAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(t_rowptr, 0, ((size_t)n_cols + 1) * sizeof(int32_t), st) != hipSuccess) return amar_check_launch();
    if (nnz == 0) return amar_check_launch();
    const int grid = csrt_grid(nnz, CSRT_BLOCK);
    hipLaunchKernelGGL(csrt_count_kernel, dim3(grid), dim3(CSRT_BLOCK), 0, st, colidx, (int64_t)nnz, n_cols, t_rowptr);
    hipLaunchKernelGGL(csrt_scan_kernel, dim3(1), dim3(CSRT_SCAN_BLOCK), 0, st, t_rowptr, n_cols, cursor);
    hipLaunchKernelGGL(csrt_scatter_kernel, dim3(grid), dim3(CSRT_BLOCK), 0, st, colidx, (int64_t)nnz, n_cols, cursor, perm);
    hipLaunchKernelGGL(csrt_sort_kernel, dim3(n_cols < 65536 ? n_cols : 65536), dim3(CSRT_BLOCK), 0, st, t_rowptr, n_cols, perm);
    hipLaunchKernelGGL(csrt_rows_kernel, dim3(grid), dim3(CSRT_BLOCK), 0, st, rowptr, n_rows, perm, (int64_t)nnz, t_colidx);
    return amar_check_launch();
}

}  // extern "C"

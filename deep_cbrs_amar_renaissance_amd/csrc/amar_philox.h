// Philox4x32-10 (Salmon et al., SC'11) and the dropout draws built on it, shared by the BPR sampler (amar_bpr.hip), the node
// dropout (amar_dropout.hip) and the GAT attention dropout (amar_propagate.hip forward, amar_train.hip reverse).
//
// One definition of a dropout draw (restated in numpy by data/datasets.py:dropout_node_mask / dropout_edge_mask):
//   key     = (seed_lo, seed_hi)
//   counter = (c0, step_lo, step_hi, (site << 24) | c3) with step read from device memory and site in 1 .. 255, where
//     node mask:  c0 = r * ceil(C / 4) + c / 4 (< 2^31), c3 = 0; word (c % 4) of the call belongs to column c of row r
//     edge mask:  entry (target i, source j, ordinal o among the row's equal columns): c0 = min(i, j) | ((o % 255) << 24),
//                 c3 = max(i, j) (node ids < 2^24); the self loop a layer adds itself is the entry with ordinal slot 255.
//                 Word 0 of the call is the entry's word: (i, j, o) and its mirror (j, i, o) draw the same one.
//   keep iff word >= threshold; kept values are multiplied by scale, dropped ones become +0.
// The BPR sampler's counters end in a zero word, site >= 1 keeps every dropout counter apart from them under one key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    }
}

// What a kernel needs to regenerate a dropout mask (passed by value; `step` is one 64-bit counter in device memory).
struct AmarDropout {
    uint32_t key0, key1; const uint64_t *step; uint32_t site; uint32_t threshold; float scale;
};

#define AMAR_DROPOUT_MAX_NODES (1 << 24)

// keep * scale of the entry (i, j, ordinal) of a symmetric edge multiset; ordinal 255 = the added self loop
__device__ __forceinline__ float dropout_edge_factor(const AmarDropout &d, uint64_t step, int i, int j, int ordinal) {
    const uint32_t lo = (uint32_t)(i < j ? i : j), hi = (uint32_t)(i < j ? j : i);
    uint32_t c[4] = {lo | ((uint32_t)ordinal << 24), (uint32_t)step, (uint32_t)(step >> 32), (d.site << 24) | hi};
    philox4x32_10(c, d.key0, d.key1);
    return c[0] >= d.threshold ? d.scale : 0.f;
}

// ordinal of entry p (column c) among the equal columns of its row [beg, end): columns are sorted, so its equals precede it
__device__ __forceinline__ int edge_ordinal(const int32_t *__restrict__ colidx, int beg, int p, int c) {
    int o = 0;
    while (p - o > beg && colidx[p - o - 1] == c) ++o;
    return o % 255;
}

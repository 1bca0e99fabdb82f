// The score stage of the fused rankers of the split head, as a fragment of a kernel body: rank_topk_kernel (amar_rank_score.h)
// includes it inside its loop over the 16 PT-item steps of a staged tile — once for a selector row that is one user, once inside
// the member loop of a row that folds over several — amar_rank_after.hip's kernel includes it, and amar_rank_of.hip wraps it in ro_score, so that a pair has the same bits
// everywhere.  It is text, not a function: as an always-inline function the same lines made hipcc allocate the top-k kernels'
// registers differently, and the <1, 4> form measurably slower (DESIGN.md, 8a10).
// In scope where it is included: MAXT, PT; a (RankArgs); w_lds, tile (LDS); grp (tile row of the step); tu[MAXT] (the user's Tu
// row as fragments: rank_load_user); lane, g = lane / 16, col = lane % 16; KT0 = a.kt[0].  It defines z: the score of the user
// against item 16 g + col of the step (lane group g holds pair tile g).
//     score(u, i) = rest( in_act( Tu[u] + Ti[i] ) )
// The first product's B fragment (pair on the MFMA column, features 16t + 4g + r on rows, the layout of chain_kernel in
// amar_chain.hip) is formed in registers; the rest stack runs on v_mfma_f32_16x16x4_f32 with chain_kernel's loop order, fragment
// blob and dot stage.
                f32x4 x[MAXT][PT];
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) {
                    const float *row = tile + (grp + 16 * pt + col) * a.tile_stride;
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) {
                        const int f = 16 * t + 4 * g;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (t < KT0 && f < a.c1) {
                            v = tu[t] + *reinterpret_cast<const f32x4 *>(row + f);
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = amar_act(v[r], a.in_act);
                        }
                        x[t][pt] = v;
                    }
                }
                for (int l = 0; l < a.n_layers; ++l) {
                    const int KT = a.kt[l], NT = a.nt[l];
                    const float *wl = w_lds + a.w_off[l];
                    const float *bl = w_lds + a.b_off[l];
                    f32x4 y[MAXT][PT];
#pragma unroll
                    for (int mm = 0; mm < MAXT; ++mm) {
                        if (mm < NT) {
                            const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bl + 16 * mm + 4 * g);
#pragma unroll
                            for (int pt = 0; pt < PT; ++pt) y[mm][pt] = b4;
#pragma unroll
                            for (int t = 0; t < MAXT; ++t) {
                                if (t < KT) {
                                    const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wl + ((mm * KT + t) * 64 + lane) * 4);
#pragma unroll
                                    for (int r = 0; r < 4; ++r)
#pragma unroll
                                        for (int pt = 0; pt < PT; ++pt)
                                            y[mm][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[r], x[t][pt][r], y[mm][pt], 0, 0, 0);
                                }
                            }
                        }
                    }
                    const int act = a.act[l];
#pragma unroll
                    for (int mm = 0; mm < MAXT; ++mm)
#pragma unroll
                        for (int pt = 0; pt < PT; ++pt) {
                            f32x4 v = {0.f, 0.f, 0.f, 0.f};
                            if (mm < NT) {
                                v = y[mm][pt];
#pragma unroll
                                for (int r = 0; r < 4; ++r) v[r] = amar_act(v[r], act);
                            }
                            x[mm][pt] = v;
                        }
                }
                // the 1-unit layer: chain_kernel's dot, then lane group g keeps pair tile g
                const float *wd = w_lds + a.dot_off;
                float sel = 0.f;
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) {
                    float s = 0.f;
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) {
                        if (t < a.dot_kt) {
                            const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wd + 16 * t + 4 * g);
#pragma unroll
                            for (int r = 0; r < 4; ++r) s = fmaf(x[t][pt][r], w4[r], s);
                        }
                    }
                    s += __shfl_xor(s, 16, 64);
                    s += __shfl_xor(s, 32, 64);
                    sel = g == pt ? s : sel;
                }
                const float z = amar_act(sel + w_lds[a.dot_bias_off], a.dot_act);

"""Full-catalogue top-k (recommend(), k = 10, every user, training pairs excluded): the fused route (amar_recommend_f32) against the
pair route (pair list built on the device + hoisted pair scoring + amar_topk_segmented_f32) at ml1m(s=1) and ml1m(s=8).

Heads: BasicGCN with the default head (towers 32 -> 16, clf 16 -> 16 -> 1: rest = 16 -> 16 -> 1) and BasicRS on KGE rows with the
basic-kge head (towers 512 -> 256 -> 128, clf 64 -> 64 -> 1: rest = 64 -> 64 -> 1).  Reported per case: ms per recommend() call
(median of the timed calls), the fused ranking launch alone on cached towers, pairs ranked per second, and the launch against its
MFMA floor = the products' flops (sum over the rest stack of 2 K N per pair) at the f32 matrix peak (157.3 TFLOP/s).

Usage: python tools/exp_recommend.py [--scales 1 8] [--reps 5] [--skip-pairs-above 8]  (one JSON line per case on stdout)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK = 157.3e12


class _Train:
    def __init__(self, ratings, n_users, n_items, embeddings=None):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)
        if embeddings is not None:
            self.embeddings = embeddings


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), out


def _flops_per_pair(dims):
    return sum(2 * k * n for k, n in zip(dims[:-1], dims[1:]))


def run_case(label, model, train, rs, reps, pairs_too):
    from deep_cbrs_amar_renaissance_amd import capi
    nu, ni = len(train.users), len(train.items)
    n_pairs = nu * ni
    res = {'case': label, 'users': nu, 'items': ni, 'pairs': n_pairs, 'k': 10, 'route': model._recommend_route(train)}
    ms, all_ms = _time(lambda: model.recommend(train, k=10), reps)
    res.update({'fused_ms': ms, 'fused_ms_all': [round(x, 3) for x in all_ms], 'fused_pairs_per_s': n_pairs / (ms * 1e-3)})
    # the ranking launch alone, on the towers of one call
    towers = rs._recommend_split(*model._recommend_tables(train))
    plan = towers[2]
    blob, dims, acts = plan['rest']
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    excl = rec._exclusion_device(train, nu, ni, True)
    kms, _ = _time(lambda: capi.recommend(towers[0], towers[1], blob, dims, acts, plan['in_act'], 10, excl_ptr=excl[0], excl_items=excl[1]), reps)
    slices = capi.load().amar_recommend_slices(nu, ni, (__import__('ctypes').c_int32 * len(dims))(*dims), len(dims) - 1, 0)
    flops = n_pairs * _flops_per_pair(dims)
    res.update({'kernel_ms': kms, 'kernel_pairs_per_s': n_pairs / (kms * 1e-3), 'rest_dims': dims, 'gflop': flops / 1e9,
                'mfma_floor_ms': flops / F32_MFMA_PEAK * 1e3, 'fraction_of_mfma_floor': (flops / F32_MFMA_PEAK * 1e3) / kms,
                'item_slices': int(slices)})
    s1_ms, _ = _time(lambda: capi.recommend(towers[0], towers[1], blob, dims, acts, plan['in_act'], 10, excl_ptr=excl[0], excl_items=excl[1],
                                            n_slices=1), reps)
    res['kernel_ms_one_slice'] = s1_ms
    if pairs_too:
        pms, pall = _time(lambda: model._recommend_pairs(train, k=10), max(1, reps // 2))
        res.update({'pairs_ms': pms, 'pairs_ms_all': [round(x, 3) for x in pall], 'pairs_pairs_per_s': n_pairs / (pms * 1e-3),
                    'speedup_fused_over_pairs': pms / ms})
        a, b = model.recommend(train, k=10), model._recommend_pairs(train, k=10)
        res['lists_equal_to_pair_route'] = bool(np.array_equal(a[1], b[1]))
        res['max_score_diff_to_pair_route'] = float(np.abs(np.where(np.isfinite(a[2]), a[2] - np.where(np.isfinite(b[2]), b[2], 0), 0)).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-pairs-above', type=int, default=8, help='pair route only at scales up to this one')
    ap.add_argument('--cases', nargs='+', default=['gcn', 'kge'])
    args = ap.parse_args()
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    capi.load()
    torch.cuda.set_device(0)
    for s in args.scales:
        d = helpers.ml1m_indexed(s)
        nu, ni = len(d['users']), len(d['items'])
        for case in args.cases:
            engine.set_seed(1)
            if case == 'gcn':
                model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
                helpers.spread_scores(model)
                train, rs = _Train(d['train'], nu, ni), model.rs
                label = 'BasicGCN default head ml1m(s={})'.format(s)
            else:
                table = np.random.default_rng(2).normal(0, 1, size=(nu + ni, 100)).astype(np.float32)
                model = basic.BasicRS(dense_units=[512, 256, 128], clf_units=[64, 64])
                model.build_head(100, 100)
                train, rs = _Train(d['train'], nu, ni, table), model
                label = 'BasicRS basic-kge head ml1m(s={})'.format(s)
            res = run_case(label, model, train, rs, args.reps, s <= args.skip_pairs_above)
            print(json.dumps(res), flush=True)
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

"""Exact full-catalogue positions (amar_rank_of_f32) for BasicGCN with the default head at ml1m(s=1) and ml1m(s=8): every user, the
targets = a held-out split of the training ratings (datasets.holdout_split, 10 %; the kept rows are the exclusion rows).  Timed on
the towers of one call, alternating inside every repetition:

  (a) rank_of:   the new launch alone (capi.rank_of: the entries are on the device before the clock starts only as far as the
                 binding allows — its host split and three small uploads are inside, as they are in every call);
  (b) recommend: amar_recommend_f32 at k = 10 over the same users — the same score work with a selection instead of a count;
  (c) pairs:     rank_of_pairs on the same inputs (the pair stage's kernel over explicit pair lists and torch comparisons), with its
                 peak workspace;
and, once per case, a whole evaluate_ranking(ks=[10], rank_metrics=(auc, mrr, map)) call against the same call without rank_metrics.

A sample is the host clock around `inner` back-to-back calls that end in a device synchronise, divided by `inner`; reported are the
median over 5 samples and the spread (min, max).  (a) is also checked against (c): the integer counts must be equal.  One JSON line
per case goes to stdout and to --out.

Usage: python tools/exp_rank_of.py [--scales 1 8] [--reps 5] [--out profiles/exp_rank_of.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 10


class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def _sample(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def _stats(samples):
    return {'median_ms': float(np.median(samples)), 'min_ms': float(min(samples)), 'max_ms': float(max(samples)),
            'samples_ms': [round(x, 4) for x in samples]}


def run_case(scale, model, train, held, reps):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = len(train.users), len(train.items)
    test = np.concatenate([held[:, :2], np.ones((len(held), 1), dtype=held.dtype)], axis=1)      # every held-out row is a target
    ptr, items, _ = rec.heldout_targets(train, test, True)
    users = np.arange(nu)
    towers = model.rs._recommend_split(*model._recommend_tables(train))
    plan = towers[2]
    blob, dims, acts = plan['rest']
    tu, ti = towers[0], towers[1]
    pair_towers = model.rs.towers(*model._recommend_tables(train))
    excl = rec._exclusion_device(train, nu, ni, True)
    score_fn = lambda u, i: model.rs.score_towers(pair_towers, u, i)

    def rank_of():
        return capi.rank_of(tu, ti, blob, dims, acts, plan['in_act'], users, ptr, items, excl_ptr=excl[0], excl_items=excl[1])

    def recommend():
        return capi.recommend(tu, ti, blob, dims, acts, plan['in_act'], K, excl_ptr=excl[0], excl_items=excl[1])

    def pairs():
        return rec.rank_of_pairs(score_fn, train, users, (ptr, items), True, device=tu.device)

    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    lib = capi.load()
    entries = len(capi.rank_of_entries(users, ptr)[0])
    res = {'case': 'BasicGCN default head ml1m(s={})'.format(scale), 'scale': scale, 'users': nu, 'items': ni, 'targets': int(len(items)),
           'entries': entries, 'longest_row': int(np.diff(ptr).max()), 'catalogue_pairs': nu * ni, 'k': K, 'rest_dims': list(dims),
           'rank_of_slices': int(lib.amar_rank_of_slices(entries, ni, dims_c, len(dims) - 1, 0)),
           'recommend_slices': int(lib.amar_recommend_slices(nu, ni, dims_c, len(dims) - 1, 0))}
    for fn in (rank_of, recommend, pairs):                               # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pairs()
    torch.cuda.synchronize()
    res['pairs_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    torch.cuda.reset_peak_memory_stats()
    rank_of()
    torch.cuda.synchronize()
    res['rank_of_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    a, b, c = [], [], []
    for _ in range(reps):                                                # alternating: drift hits all three alike
        a.append(_sample(rank_of, 10))
        b.append(_sample(recommend, 10))
        c.append(_sample(pairs, 1))
    res.update({'rank_of': _stats(a), 'recommend': _stats(b), 'pairs': _stats(c)})
    res['rank_of_over_recommend'] = res['rank_of']['median_ms'] / res['recommend']['median_ms']
    res['pairs_over_rank_of'] = res['pairs']['median_ms'] / res['rank_of']['median_ms']
    plain = [_sample(lambda: model.evaluate_ranking(train, test, [K]), 1) for _ in range(reps)]
    both = [_sample(lambda: model.evaluate_ranking(train, test, [K], rank_metrics=('auc', 'mrr', 'map')), 1) for _ in range(reps)]
    res['evaluate_ranking_ms'] = _stats(plain)                           # propagation, towers, lists, metrics
    res['evaluate_ranking_with_rank_metrics_ms'] = _stats(both)
    res['metrics'] = {k: v for k, v in model.evaluate_ranking(train, test, [K], rank_metrics=('auc', 'mrr', 'map')).items()}
    fused, slow = [t.cpu().numpy() for t in rank_of()], [t.cpu().numpy() for t in pairs()]
    res['counts_equal_to_pairs'] = bool(all(np.array_equal(x, y) for x, y in zip(fused[1:], slow[1:])))
    res['max_score_diff_to_pairs'] = float(np.abs(fused[0] - slow[0]).max()) if len(items) else 0.0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_rank_of.jsonl'))
    args = ap.parse_args()
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import holdout_split
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    capi.load()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        for s in args.scales:
            d = helpers.ml1m_indexed(s)
            nu, ni = len(d['users']), len(d['items'])
            kept, held = holdout_split(d['train'], 0.1, seed=7)
            engine.set_seed(1)
            model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
            helpers.spread_scores(model)
            line = json.dumps(run_case(s, model, _Train(kept, nu, ni), held, args.reps))
            print(line, flush=True)
            out.write(line + '\n')
            out.flush()
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

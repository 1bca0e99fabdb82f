"""The fused rankers through a library built from the parent commit and through this tree's: the same bits, the same time.

For BasicGCN with the default head at ml1m(s=1) and ml1m(s=8), every user, training items excluded, each of these calls goes through
three libraries — `parent` (--parent-lib), `this` (the tree's own) and `parent_again` (--parent-lib-again: a second, separate build
of the same parent commit) — with the same arguments:

    recommend_k10, recommend_k64    amar_recommend_f32
    after_k64                       amar_recommend_after_f32 with second-page cursors (the last column of recommend_k64)
    among_10pct, among_100pct       amar_recommend_among_f32 at k = 10 over every tenth item row / every item row
    group_mean_4                    amar_recommend_group_f32 at k = 10, `mean`, groups of 4 consecutive users, the members' union excluded
    rank_of_8                       amar_rank_of_f32 for every user and the first 8 items of its recommend_k10 list

Bits first: the three outputs of a call must be EQUAL (item rows / counts, and score bits) before any time is recorded.  Then time:
a sample is the host clock around `inner` back-to-back calls that end in a device synchronise, divided by `inner`; the three libraries
alternate inside every repetition.  Reported per call and library: median, min, max.  The yardstick is `parent`; the margin is
measured, not assumed: `band` is [min, max] over the samples of `parent` and `parent_again` together, two builds of one source, and
`this_in_band` says whether this tree's median lies inside it and `this_slower` whether it lies above it (a median below the band
is faster than both parent builds ever were).  The band is wider than the distance of the two parent medians on purpose: it is what
one source gives from sample to sample and from build to build.  `this_over_parent` and `again_over_parent` are ratios of medians.
One JSON line per scale goes to stdout and to --out.

Usage: python tools/exp_rank_one_body.py --parent-lib A/libamar_hip.so --parent-lib-again B/libamar_hip.so [--scales 1 8] [--reps 7]
           [--out profiles/exp_rank_one_body.jsonl]
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


ORDER = ('parent', 'this', 'parent_again')


def _load(capi, path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def _equal(a, b):
    """Tuples of device tensors: the same integers, the same float bits."""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def run_scale(scale, model, train, reps, libs):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = len(train.users), len(train.items)
    towers = model.rs._recommend_split(*model._recommend_tables(train))
    plan = towers[2]
    blob, dims, acts = plan['rest']
    head = (towers[0], towers[1], blob, dims, acts, plan['in_act'])
    dev = towers[0].device
    excl = rec._exclusion_device(train, nu, ni, True)
    kw = dict(excl_ptr=excl[0], excl_items=excl[1])

    def through(lib, fn, *a, **k):                                     # the binding's own marshalling, on the library `lib`
        capi._lib = libs[lib]
        try:
            return fn(*a, **k)
        finally:
            capi._lib = libs['this']

    page = through('parent', capi.recommend, *head, 64, **kw)
    cursor = (page[0][:, -1].contiguous(), page[1][:, -1].contiguous())
    top10 = through('parent', capi.recommend, *head, 10, **kw)[0].cpu().numpy()
    g_ptr, g_users = rec.group_csr([list(range(u, min(u + 4, nu))) for u in range(0, nu, 4)], nu)
    ge_ptr, ge_items = rec.group_exclusion_csr(train.ratings, g_ptr, g_users, nu, ni)
    g_dev = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev) for x in (g_ptr, g_users, ge_ptr, ge_items)]
    targets = np.sort(top10[:, :8], axis=1)
    assert (targets >= 0).all()
    t_ptr = np.arange(nu + 1) * 8
    calls = {
        'recommend_k10': lambda: capi.recommend(*head, 10, **kw),
        'recommend_k64': lambda: capi.recommend(*head, 64, **kw),
        'after_k64': lambda: capi.recommend_after(*head, 64, *cursor, **kw),
        'among_10pct': lambda: capi.recommend_among(*head, 10, np.arange(0, ni, 10), **kw),
        'among_100pct': lambda: capi.recommend_among(*head, 10, np.arange(ni), **kw),
        'group_mean_4': lambda: capi.recommend_group(*head, 10, g_dev[0], g_dev[1], strategy='mean', excl_ptr=g_dev[2], excl_items=g_dev[3]),
        'rank_of_8': lambda: capi.rank_of(*head, np.arange(nu), t_ptr, targets.reshape(-1), **kw),
    }
    res = {'case': 'BasicGCN default head ml1m(s={})'.format(scale), 'scale': scale, 'users': nu, 'items': ni, 'rest_dims': list(dims),
           'route': capi.rank_route('recommend', dims), 'groups': len(g_ptr) - 1, 'reps': reps, 'calls': {}}
    for name, call in calls.items():                                   # bits before time
        outs = {lib: through(lib, call) for lib in ORDER}
        torch.cuda.synchronize()
        same = {lib: _equal(outs[lib], outs['parent']) for lib in ('this', 'parent_again')}
        res['calls'][name] = {'this_equals_parent': same['this'], 'again_equals_parent': same['parent_again']}
        assert same['this'] and same['parent_again'], (res['case'], name, same)
    inner = 10 if scale == 1 else 3
    for name, call in calls.items():
        samples = {lib: [] for lib in ORDER}
        for _ in range(reps):                                          # alternating: drift hits all alike
            for lib in ORDER:
                samples[lib].append(through(lib, lambda: _sample(call, inner)))
        entry = res['calls'][name]
        entry.update({lib: _stats(samples[lib]) for lib in ORDER})
        both = samples['parent'] + samples['parent_again']
        entry['band_ms'] = [float(min(both)), float(max(both))]
        entry['this_in_band'] = bool(min(both) <= entry['this']['median_ms'] <= max(both))
        entry['this_slower'] = bool(entry['this']['median_ms'] > max(both))
        entry['this_over_parent'] = entry['this']['median_ms'] / entry['parent']['median_ms']
        entry['again_over_parent'] = entry['parent_again']['median_ms'] / entry['parent']['median_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--parent-lib', required=True, help="libamar_hip.so built from the parent commit: the yardstick")
    ap.add_argument('--parent-lib-again', required=True, help="a second, separate build of the same commit: the margin")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_rank_one_body.jsonl'))
    args = ap.parse_args()
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    libs = {'this': capi.load(), 'parent': _load(capi, args.parent_lib), 'parent_again': _load(capi, args.parent_lib_again)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        for s in args.scales:
            d = helpers.ml1m_indexed(s)
            nu, ni = len(d['users']), len(d['items'])
            engine.set_seed(1)
            model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
            helpers.spread_scores(model)
            line = json.dumps(run_scale(s, model, _Train(d['train'], nu, ni), args.reps, libs))
            print(line, flush=True)
            out.write(line + '\n')
            out.flush()
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

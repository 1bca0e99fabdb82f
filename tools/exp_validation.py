#!/usr/bin/env python
"""What validating during fit() costs: BasicGCN at ml1m(s), Adam, batch 1 024.
    metrics    amar_rank_metrics_f64 (capi.rank_metrics, result read back) against the host full_ranking_metrics on the same top-10
               lists of recommend(), ks = [5, 10]
    epochs     the wall time of one fit() epoch: plain (no new argument), with validation_data (the test pairs), with
               validation_ranking (ks = [10]); the variants alternate inside every round
usage: python tools/exp_validation.py <scale> [<rounds> [<out.jsonl> [<parts> [<label>]]]]
       <parts>: comma-separated subset of metrics,epochs (default: both).  `epochs` also runs on a tree without the feature, where only
       the plain variant exists: that run, labelled e.g. `parent`, is the reference point of the plain epoch.
Every timing is the host clock around a device synchronise, one warm-up first, then <rounds> rounds; reported: the median over the rounds
and the rounds' smallest and largest value (the run-to-run spread)."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def _spread(values, digits=4):
    v = sorted(values)
    return {'median': round(v[len(v) // 2], digits), 'min': round(v[0], digits), 'max': round(v[-1], digits)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    scale = int(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    out = sys.argv[3] if len(sys.argv) > 3 else None
    parts = sys.argv[4].split(',') if len(sys.argv) > 4 else ['metrics', 'epochs']
    label = sys.argv[5] if len(sys.argv) > 5 else 'feature'
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.data import loaders, preprocess, synthetic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    capi.load()
    ds = synthetic.ml1m(scale, with_props=False)
    (train, test), (users, items) = loaders.index_ratings(ds.train, ds.test)
    adj = preprocess.build_adjacency_matrix(train, users, items)
    trainset = UserItemGraph(train, users, items, adj, batch_size=1024, shuffle=True)
    testset = UserItemGraph(test, users, items, adj, batch_size=1024)

    def build():
        engine.set_seed(42)
        model = basic.BasicGCN(adj, embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
        model.n_users, model.n_items = len(users), len(items)
        model.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=1e-3), metrics=['accuracy'])
        model(trainset[0][0])
        return model

    records = []
    base = {'tree': label, 'scale': scale, 'users': len(users), 'items': len(items), 'rounds': rounds}
    if 'metrics' in parts:
        from deep_cbrs_amar_renaissance_amd import recommend as rec
        from deep_cbrs_amar_renaissance_amd.utilities import metrics as um
        model, ks = build(), [5, 10]
        with rec.device_lists():
            _, lists, _ = model.recommend(trainset, k=10)
        host_users, host_items, _ = model.recommend(trainset, k=10)
        rel_ptr, rel_items = um._relevant_device(test, len(users), len(items))
        kernel = lambda: capi.rank_metrics(lists, rel_ptr, rel_items, ks)
        kernel()
        dev_ms = [_timed(kernel) for _ in range(rounds)]
        host_ms = []
        for _ in range(max(3, rounds // 2)):
            t0 = time.perf_counter()
            want = um.full_ranking_metrics(host_users, host_items, test, ks)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        got = um.full_ranking_metrics_device(None, lists, test, ks, len(users), len(items))
        err = max(abs(got[key] - want[key]) for key in want)
        records.append(dict(base, part='metrics', ks=ks, lists=int(lists.shape[0]), kernel_ms=_spread(dev_ms), host_ms=_spread(host_ms, 1),
                            host_over_kernel=round(sorted(host_ms)[len(host_ms) // 2] / sorted(dev_ms)[len(dev_ms) // 2], 1),
                            max_abs_difference=err))
    if 'epochs' in parts:
        variants = {'plain': {}}
        if label == 'feature':
            variants['validation_data'] = {'validation_data': testset}
            variants['validation_ranking'] = {'validation_ranking': {'trainset': trainset, 'ratings': test, 'ks': [10], 'users': None}}
        models = {name: build() for name in variants}
        for name, kwargs in variants.items():                                         # warm-up: eager batch, capture, first validation
            models[name].fit(trainset, epochs=2, verbose=False, **kwargs)
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, kwargs in variants.items():
                times[name].append(_timed(lambda: models[name].fit(trainset, epochs=1, verbose=False, **kwargs)))
        first = sorted(times['plain'])[rounds // 2]
        for name in variants:
            records.append(dict(base, part='epochs', variant=name, batches=len(trainset), epoch_ms=_spread(times[name], 2),
                                vs_plain=round(sorted(times[name])[rounds // 2] / first, 4)))
    for record in records:
        print(json.dumps(record))
        if out:
            with open(out, 'a') as fp:
                fp.write(json.dumps(record) + '\n')


if __name__ == '__main__':
    main()

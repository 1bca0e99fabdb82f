#!/usr/bin/env python
"""What training-time dropout costs: fit() with and without it, ml1m(s=1) and ml1m(s=8), batch 1 024, replayed graphs.

One JSON line per (dataset, model, leg) appended to profiles/exp_dropout.jsonl (--out), seconds per epoch after one warm-up epoch:
  rate0      no dropout key at all: the path every config took before (the leg that also runs on an older checkout, --root)
  stack0.2   dropout=0.2: every layer's output dropped (GCN leaves the fused multi-layer propagation, one mask launch per layer
             forward and one reverse)
  attn0.2    BasicGAT only, dropout_rate=0.2: the attention coefficients dropped inside the three GAT walks (one Philox call per entry)
  both0.2    BasicGAT only, both keys
Models: BasicGCN / BasicGAT 16 x 2, dense [48, 48], clf [64, 64] (the dimensions of tools/exp_bpr.py).

    python tools/exp_dropout.py [--epochs N] [--scales 1 8] [--models BasicGCN BasicGAT] [--legs rate0 stack0.2 ...] [--tag T]
                                [--root DIR]    import the package from another checkout (its own built library), rate0 only
    python tools/exp_dropout.py profile MODEL LEG    one epoch of that leg at s=1 after a warm-up epoch (under rocprofv3)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = dict(embedding_dim=16, n_hiddens=[16, 16], dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4)
LEGS = {'rate0': {}, 'stack0.2': {'dropout': 0.2}, 'attn0.2': {'dropout_rate': 0.2}, 'both0.2': {'dropout': 0.2, 'dropout_rate': 0.2}}


def dataset(scale):
    from deep_cbrs_amar_renaissance_amd.data import loaders, preprocess, synthetic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    ds = synthetic.ml1m(scale, with_props=False)
    (train, _), (users, items) = loaders.index_ratings(ds.train, ds.test)
    adj = preprocess.build_adjacency_matrix(train, users, items)
    return UserItemGraph(train, users, items, adj, batch_size=1024, shuffle=True), adj


def model_for(name, adj, extra):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(42)
    m = getattr(basic, name)(adj, **dict(CFG, **extra))
    m.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=1e-3), metrics=['accuracy'])
    return m


def timed_fit(model, seq, epochs):
    import torch
    model.fit(seq, epochs=1, verbose=False)                          # warm-up: capture, allocator, packing caches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = model.fit(seq, epochs=epochs, verbose=False)['loss']
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='*')
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--models', nargs='+', default=['BasicGCN', 'BasicGAT'])
    ap.add_argument('--legs', nargs='+', default=None)
    ap.add_argument('--tag', default='this')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_dropout.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    if args.mode and args.mode[0] == 'profile':
        name, leg = args.mode[1], args.mode[2]
        seq, adj = dataset(1)
        s, _ = timed_fit(model_for(name, adj, LEGS[leg]), seq, 1)
        print('profile: one replayed {} epoch ({}) of {} batches: {:.3f} s'.format(name, leg, len(seq), s), flush=True)
        return
    with open(args.out, 'a') as fp:
        for scale in args.scales:
            seq, adj = dataset(scale)
            for name in args.models:
                legs = args.legs or [leg for leg in LEGS if name == 'BasicGAT' or leg in ('rate0', 'stack0.2')]
                for leg in legs:
                    s, hist = timed_fit(model_for(name, adj, LEGS[leg]), seq, args.epochs)
                    rec = {'dataset': 'ml1m(s={})'.format(scale), 'model': name + ' 16x2 dense [48,48] clf [64,64]', 'leg': leg,
                           'code': args.tag, 'batch': 1024, 'epochs_timed': args.epochs, 'batches_per_epoch': len(seq),
                           'nodes': int(adj.shape[0]), 's_per_epoch': round(s, 4), 'ms_per_batch': round(1e3 * s / len(seq), 4),
                           'loss': [round(float(v), 5) for v in hist]}
                    print(json.dumps(rec), flush=True)
                    fp.write(json.dumps(rec) + '\n')
                    fp.flush()


if __name__ == '__main__':
    main()

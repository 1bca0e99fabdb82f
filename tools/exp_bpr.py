#!/usr/bin/env python
"""BPR fit() against BCE fit() on the same model, ml1m(s=1) and ml1m(s=8), batch 1 024.

Per scale, one JSON line in profiles/exp_bpr.jsonl:
  bpr_s_per_epoch          fit() on UserItemGraphPosNegSample with BPRLoss: every batch drawn on the device inside the replayed graph
  bce_s_per_epoch          fit() on the shuffled UserItemGraph with binary cross-entropy, replayed (the path every other config takes)
  host_getitem_s_per_epoch HOST number: the Sequence's own __getitem__ (the reference's sampler restated, numpy RandomState) timed over
                           a few batches and scaled to len(sequence) batches — what a host-fed BPR epoch would spend before any GPU work
Model: BasicGCN 16 x 2, dense [48, 48], clf [64, 64] (the doc.pdf Table 5 config of tools/exp_train.py).  One warm-up epoch each.

    python tools/exp_bpr.py [epochs] [scales...]        (repo root, GPU box; writes profiles/exp_bpr.jsonl)
    python tools/exp_bpr.py profile                     one BPR epoch at s=1 after a warm-up epoch (under rocprofv3)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

CFG = dict(embedding_dim=16, n_hiddens=[16, 16], dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4)


def datasets(scale):
    from deep_cbrs_amar_renaissance_amd.data import loaders, preprocess, synthetic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph, UserItemGraphPosNegSample
    ds = synthetic.ml1m(scale, with_props=False)
    (train, _), (users, items) = loaders.index_ratings(ds.train, ds.test)
    t0 = time.perf_counter()
    sample = UserItemGraphPosNegSample(train, users, items, preprocess.build_adjacency_matrix(train, users, items, type_adjacency='binary'),
                                       batch_size=1024)
    build_s = time.perf_counter() - t0
    adj = preprocess.build_adjacency_matrix(train, users, items)
    return sample, UserItemGraph(train, users, items, adj, batch_size=1024, shuffle=True), adj, build_s


def model_for(adj, loss):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(42)
    m = basic.BasicGCN(adj, **CFG)
    m.compile(loss=loss, optimizer=Adam(learning_rate=1e-3), metrics=['accuracy'])
    return m


def timed_fit(model, seq, epochs):
    model.fit(seq, epochs=1, verbose=False)                          # warm-up: capture, allocator, packing caches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = model.fit(seq, epochs=epochs, verbose=False)['loss']
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs, hist


def main():
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    capi.load()
    if len(sys.argv) > 1 and sys.argv[1] == 'profile':
        sample, _, _, _ = datasets(1)
        model = model_for(sample.adj_matrix, BPRLoss())
        s, _ = timed_fit(model, sample, 1)
        print('profile: one replayed BPR epoch of {} batches: {:.3f} s'.format(len(sample), s), flush=True)
        return
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    scales = [int(a) for a in sys.argv[2:]] or [1, 8]
    out = os.path.join(ROOT, 'profiles', 'exp_bpr.jsonl')
    lines = []
    for scale in scales:
        sample, ui, adj, build_s = datasets(scale)
        bpr_s, bpr_hist = timed_fit(model_for(sample.adj_matrix, BPRLoss()), sample, epochs)
        bce_s, bce_hist = timed_fit(model_for(adj, 'binary_crossentropy'), ui, epochs)
        n = 20
        t0 = time.perf_counter()
        for b in range(n):
            sample[b]
        host = (time.perf_counter() - t0) / n * len(sample)
        rec = {'dataset': 'ml1m(s={})'.format(scale), 'model': 'BasicGCN 16x2 dense [48,48] clf [64,64]', 'batch': 1024,
               'epochs_timed': epochs, 'batches_per_epoch': len(sample), 'train_ratings': int(len(sample.ratings)),
               'bpr_s_per_epoch': round(bpr_s, 4), 'bce_s_per_epoch': round(bce_s, 4), 'bpr_over_bce': round(bpr_s / bce_s, 3),
               'host_getitem_s_per_epoch': round(host, 3), 'host_getitem_note': 'host CPU, __getitem__ over {} batches scaled to an epoch'.format(n),
               'sequence_build_s_host': round(build_s, 3),
               'bpr_loss': [round(float(v), 5) for v in bpr_hist], 'bce_loss': [round(float(v), 5) for v in bce_hist]}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    with open(out, 'w') as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""A replayed BPR epoch on per-user triples (UserItemGraphTriplets) against the reference-layout BPR epoch (UserItemGraphPosNegSample)
on the same models, ml1m(s=1), batch 1 024, and the two samplers' launches by themselves.

One JSON line per (model, sequence) in profiles/exp_bpr_triplets.jsonl:
  s_per_epoch_median / _min / _max   fit() epochs timed one by one (host clock around a device synchronise), the variants ALTERNATING
                                     inside every repeat so that drift of the shared host hits them alike
  ms_per_batch_median                the median over the batches of an epoch
and one line for the samplers: a hipGraph of 200 launches of amar_bpr_sample_i32 / amar_bpr_sample_triplets_i32 (h = 512) replayed and
timed with device events -> us per launch, launch gaps of a serial stream included (median and range over the repeats).
Models: BasicGCN 16 x 2 and BasicLightGCN 16, 2 layers; dense [48, 48], clf [64, 64].  An epoch of the triplet Sequence has
ceil(#positives / (512 // K)) batches, the reference-layout one ceil(#ratings / 1024): compare per batch.

    python tools/exp_bpr_triplets.py [repeats]        (repo root, GPU box; writes profiles/exp_bpr_triplets.jsonl)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

CFG = {'BasicGCN': dict(embedding_dim=16, n_hiddens=[16, 16], dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4),
       'BasicLightGCN': dict(embedding_dim=16, n_layers=2, dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4)}


def sequences():
    from deep_cbrs_amar_renaissance_amd.data import loaders, preprocess, synthetic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphPosNegSample, UserItemGraphTriplets
    ds = synthetic.ml1m(1, with_props=False)
    (train, _), (users, items) = loaders.index_ratings(ds.train, ds.test)
    keep = np.isin(train[:, 0], train[train[:, 2] == 1, 0])          # every user needs a positive to be sampled
    train = train[keep]
    adj = preprocess.build_adjacency_matrix(train, users, items)
    seqs = {'reference layout': UserItemGraphPosNegSample(
        train, users, items, preprocess.build_adjacency_matrix(train, users, items, type_adjacency='binary'), batch_size=1024)}
    for K in (1, 4):
        seqs['triplets K={}'.format(K)] = UserItemGraphTriplets(train, users, items, adj, batch_size=1024, n_negatives=K)
    return seqs


def model_for(cls, adj):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    engine.set_seed(42)
    m = getattr(basic, cls)(adj, **CFG[cls])
    m.compile(loss=BPRLoss(), optimizer=Adam(learning_rate=1e-3))
    return m


def one_epoch(model, seq):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(seq, epochs=1, verbose=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sampler_launches(seqs, repeats, n=200):
    """us per launch of either sampler: n launches captured into one graph, replayed 10 times between two device events."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.engine import capture_graph
    dev, out = torch.device('cuda'), {}
    for name, seq in seqs.items():
        cls = training.DeviceSampler if name == 'reference layout' else training.TripletSampler
        s = cls(seq, dev)
        u, i = (torch.zeros(2 * s.h, dtype=torch.int32, device=dev) for _ in range(2))
        y = torch.zeros(2 * s.h, device=dev)

        def body():
            for _ in range(n):
                s.sample(u, i, y)
        body()
        graph, _ = capture_graph(body)
        graph.replay()
        times = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / (10 * n))
        out[name] = {'us_per_launch_median': round(float(np.median(times)), 3), 'us_per_launch_min': round(min(times), 3),
                     'us_per_launch_max': round(max(times), 3)}
    return out


def main():
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    seqs = sequences()
    lines = []
    for cls in CFG:
        models = {name: model_for(cls, seq.adj_matrix) for name, seq in seqs.items()}
        for name, seq in seqs.items():
            one_epoch(models[name], seq)                             # warm-up: capture, allocator, packing caches
        times = {name: [] for name in seqs}
        for _ in range(repeats):
            for name, seq in seqs.items():                           # alternating
                times[name].append(one_epoch(models[name], seq))
        for name, seq in seqs.items():
            t = times[name]
            rec = {'dataset': 'ml1m(s=1)', 'model': cls, 'sequence': name, 'batch': 1024, 'batches_per_epoch': len(seq),
                   'epochs_timed': repeats, 's_per_epoch_median': round(float(np.median(t)), 4), 's_per_epoch_min': round(min(t), 4),
                   's_per_epoch_max': round(max(t), 4), 'ms_per_batch_median': round(1e3 * float(np.median(t)) / len(seq), 4),
                   'ms_per_batch_min': round(1e3 * min(t) / len(seq), 4), 'ms_per_batch_max': round(1e3 * max(t) / len(seq), 4)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    rec = {'samplers': sampler_launches(seqs, repeats), 'h': 512, 'launches_per_graph': 200,
           'note': 'device events around 10 replays of a 200-launch graph: per launch, gaps of a serial stream included'}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    with open(os.path.join(ROOT, 'profiles', 'exp_bpr_triplets.jsonl'), 'w') as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

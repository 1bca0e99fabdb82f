#!/usr/bin/env python
"""What GraphSAGE's max aggregator costs next to mean: one process, one device, JSON lines appended to
profiles/exp_sage_aggregate.jsonl (--out).

  layer   ml1m(s=64), F = C = 8, one layer, the legs interleaved round by round (warm-up rounds first, then --rounds timed
          rounds of --iters launches each between two events; median, min and the relative spread (max - min) / median of
          the rounds are reported):
            max_fused    amar_sage_layer_agg_f32, op = max                       (the new kernel, every graph size)
            mean_row     amar_sage_layer_f32, the mean row kernel                (unchanged by the aggregator work: same gathers)
            mean_tiled   mean on its shipped large-graph route                   (LDS-tiled image, fused tail)
            sum_tiled    sum on the same route                                   (row scale 1)
  train   ml1m(s=1), BasicGraphSage 8 x 2, batch 1 024, aggregate mean and max: ms per batch of fit() on replayed graphs after a
          warm-up epoch, and the C-ABI calls of one eager batch (every call is one kernel launch except
          amar_sage_aggregate_bwd_f32, which is two: its pack prologue and the row walk — `launches` adds that one).

    python tools/exp_sage_aggregate.py [layer] [train] [--rounds N] [--iters N] [--epochs N] [--tag T]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)


def edge_csr(scale, dev):
    import torch
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR, gcn_filter_device
    data = synthetic.ml1m_device(scale, device=dev)
    n = data['n_users'] + data['n_items']
    a = gcn_filter_device(data['train_pos'][:, 0], data['train_pos'][:, 1], n)
    rp = a.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1])
    keep = rows != a.colidx.long()
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=n), 0)
    return DeviceCSR(rowptr.to(torch.int32), a.colidx[keep].contiguous(), None, (n, n))


def layer_legs(out, rounds, iters, tag):
    import torch
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd.layers.graphsage_conv import GraphSageConv
    from deep_cbrs_amar_renaissance_amd.utilities.lds_tiled import LdsTiled
    dev = torch.device('cuda')
    e = edge_csr(64, dev)
    n, F = e.shape[0], 8
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.randn((n, F), device=dev, generator=g)
    layers = {}
    for agg in ('mean', 'sum'):
        layers[agg] = GraphSageConv(F, aggregate=agg, activation='relu')
        layers[agg].build([(n, F), None])
    w, b = layers['mean'].kernel, layers['mean'].bias
    y = torch.empty((n, F), device=dev)
    assert isinstance(e.tiled_mean_image(F, True), LdsTiled) and isinstance(e.tiled_sum_image(F, True), LdsTiled)
    legs = {
        'max_fused': lambda: capi.sage_layer_agg(e.rowptr, e.colidx, x, w, b, y, 'max'),
        'mean_row': lambda: capi.sage_layer(e.rowptr, e.colidx, x, w, b, y),
        'mean_tiled': lambda: layers['mean']([x, e], out=y),
        'sum_tiled': lambda: layers['sum']([x, e], out=y),
    }
    times = {k: [] for k in legs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds + 2):                                       # two warm-up rounds: images, clocks, caches
        for name, fn in legs.items():
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append(start.elapsed_time(stop) / iters)
    for name, t in times.items():
        med = statistics.median(t)
        rec = {'what': 'layer', 'graph': 'ml1m(s=64)', 'nodes': n, 'entries': int(e.nnz), 'F': F, 'C': F, 'leg': name, 'rounds': rounds,
               'iters_per_round': iters, 'ms_median': round(med, 5), 'ms_min': round(min(t), 5), 'ms_max': round(max(t), 5),
               'spread': round((max(t) - min(t)) / med, 4), 'tag': tag}
        print(json.dumps(rec))
        out.write(json.dumps(rec) + '\n')
    out.flush()


def count_calls(fn):
    """C-ABI calls made while fn() runs, by symbol."""
    from deep_cbrs_amar_renaissance_amd import capi
    lib, seen = capi.load(), {}
    originals = {name: getattr(lib, name) for name in capi.SIGNATURES if name.endswith(('_f32', '_i32'))}

    def wrap(name, f):
        def counted(*a):
            seen[name] = seen.get(name, 0) + 1
            return f(*a)
        return counted
    for name, f in originals.items():
        setattr(lib, name, wrap(name, f))
    try:
        fn()
    finally:
        for name, f in originals.items():
            setattr(lib, name, f)
    return seen


def train_legs(out, epochs, tag):
    import torch
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.data import loaders, preprocess, synthetic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    ds = synthetic.ml1m(1, with_props=False)
    (train, _), (users, items) = loaders.index_ratings(ds.train, ds.test)
    adj = preprocess.build_adjacency_matrix(train, users, items)
    seq = UserItemGraph(train, users, items, adj, batch_size=1024, shuffle=True)
    for agg in ('mean', 'max', 'mean', 'max'):
        engine.set_seed(42)
        m = basic.BasicGraphSage(adj, aggregate=agg, **CFG)
        m.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=1e-3), metrics=['accuracy'])
        m.fit(seq, epochs=1, verbose=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist = m.fit(seq, epochs=epochs, verbose=False)['loss']
        torch.cuda.synchronize()
        s = (time.perf_counter() - t0) / epochs
        (u, i), yb = seq[0][0][:2], seq[0][1]
        calls = count_calls(lambda: training.Trainer(m).train_batch(u, i, yb))
        n_calls = sum(calls.values())
        rec = {'what': 'train', 'dataset': 'ml1m(s=1)', 'model': 'BasicGraphSage 8x2 dense [24,24] clf [48,48]', 'aggregate': agg, 'batch': 1024,
               'epochs_timed': epochs, 'batches_per_epoch': len(seq), 's_per_epoch': round(s, 4), 'ms_per_batch': round(1e3 * s / len(seq), 4),
               'abi_calls_per_eager_batch': n_calls, 'launches': n_calls + calls.get('amar_sage_aggregate_bwd_f32', 0),
               'loss': [round(float(v), 5) for v in hist], 'tag': tag}
        print(json.dumps(rec))
        out.write(json.dumps(rec) + '\n')
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='*', default=['layer', 'train'])
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_sage_aggregate.jsonl'))
    args = ap.parse_args()
    modes = args.mode or ['layer', 'train']
    with open(args.out, 'a') as out:
        if 'layer' in modes:
            layer_legs(out, args.rounds, args.iters, args.tag)
        if 'train' in modes:
            train_legs(out, args.epochs, args.tag)


if __name__ == '__main__':
    main()

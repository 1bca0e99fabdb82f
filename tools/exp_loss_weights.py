#!/usr/bin/env python
"""What the weights of the training loss cost a replayed training batch: Adam on BasicGCN and HybridBertGCN at ml1m(s),
without weights, with class_weight alone, and with per-pair sample weights.
usage: python tools/exp_loss_weights.py <scale> [<rounds> [<batches> [<out.jsonl> [<variants> [<tree label>]]]]]
       (BasicGCN 8 x 2, dense [24, 24], clf [48, 48]; HybridBertGCN grid1 with a resident 768-d table; batch 1 024)
       <variants>: comma-separated subset of none,class_weight,sample_weight (default: all three).  `none` alone runs on a tree without
       the feature too: copy this file into the parent commit's tree, run it there with the label `parent`, and run it here with the label
       `this` — in ONE session, the two commands alternating, so that a drift of the machine meets both trees.
Per model every variant gets its own trainer, four batches (eager, capture, two replays), then <rounds> rounds; in a round every variant
replays <batches> batches, timed with the host clock around a device synchronise; the variants alternate inside a round.  Reported: the
median over the rounds of the ms per batch, the rounds' smallest and largest value (the run-to-run spread), and the launch list of one
batch: the C-ABI entry points the batch's body calls, in order, recorded once while the same body runs eagerly on a trainer of its own
(`entry_points`, and `launch_list` = the first 12 hex digits of the SHA-1 of their names joined by commas)."""
import hashlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

HYBRID_GRID1 = dict(embedding_dim=8, n_hiddens=[8, 8], dense_units=[[24, 24], [256, 64], [64, 64]], clf_units=[64, 64], feature_based=True)
VARIANTS = ('none', 'class_weight', 'sample_weight')


def recorded_entry_points(capi, run):
    """Names of the library's entry points `run()` calls, in order (host-only queries such as *_route or *_floats included)."""
    lib, names, calls = capi.load(), list(capi.SIGNATURES), []
    originals = {name: getattr(lib, name) for name in names}

    def proxy(name, fn):
        def call(*args):
            calls.append(name)
            return fn(*args)
        return call
    for name, fn in originals.items():
        setattr(lib, name, proxy(name, fn))
    try:
        run()
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)
    return [name for name in calls if name not in ('amar_error_string', 'amar_last_hip_error')]


def main():
    scale = int(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    batches = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    out = sys.argv[4] if len(sys.argv) > 4 else None
    names = sys.argv[5].split(',') if len(sys.argv) > 5 else list(VARIANTS)
    tree = sys.argv[6] if len(sys.argv) > 6 else 'this'
    for name in names:
        if name not in VARIANTS:
            raise SystemExit("no variant '{}': {}".format(name, ', '.join(VARIANTS)))
    from deep_cbrs_amar_renaissance_amd import capi, engine, training
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    from deep_cbrs_amar_renaissance_amd.utilities.math import gcn_filter_device
    capi.load()
    dev = torch.device('cuda')
    data = synthetic.ml1m_device(scale, device=dev)
    n = data['n_users'] + data['n_items']
    a = gcn_filter_device(data['train_pos'][:, 0], data['train_pos'][:, 1], n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    pairs, bs = data['train_pos'], 1024
    prepared, weights = [], []
    for _ in range(8):
        idx = torch.randint(0, pairs.shape[0], (bs,), device=dev, generator=gen)
        prepared.append((pairs[idx, 0].to(torch.int32), pairs[idx, 1].to(torch.int32),
                         (torch.rand(bs, device=dev, generator=gen) < 0.57).to(torch.float32)))
        weights.append(torch.rand(bs, device=dev, generator=gen) * 2.0 + 0.25)
    bert = torch.randn((n, 768), device=dev, generator=gen) * 0.5

    def build(kind):
        engine.set_seed(42)
        if kind == 'BasicGCN':
            return basic.BasicGCN(a, embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
        model = hybrid.HybridBertGCN(a, **HYBRID_GRID1)
        model.set_bert_table(bert)
        return model

    def trainer_of(kind, variant):
        tr = training.Trainer(build(kind), rule='Adam', learning_rate=1e-3)
        if variant == 'class_weight':
            tr.set_class_weight({0: 1.0, 1: 3.0})
        return tr

    def batch_args(variant, k):
        return {'sample_weight': weights[k % 8]} if variant == 'sample_weight' else {}

    for kind in ('BasicGCN', 'HybridBertGCN'):
        runs = []
        for variant in names:
            probe = trainer_of(kind, variant)
            probe.train_batch_graphed(*prepared[0], graph=False, **batch_args(variant, 0))       # (the eager first batch of the shape)
            points = recorded_entry_points(capi, lambda: probe.train_batch_graphed(*prepared[1], graph=False, **batch_args(variant, 1)))
            torch.cuda.synchronize()
            del probe
            tr = trainer_of(kind, variant)
            for k in range(4):
                tr.train_batch_graphed(*prepared[k % 8], **batch_args(variant, k))
            torch.cuda.synchronize()
            assert tr._graphs
            runs.append({'variant': variant, 'trainer': tr, 'ms': [], 'points': points})
        for _ in range(rounds):
            for run in runs:
                tr, variant = run['trainer'], run['variant']
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(batches):
                    tr.train_batch_graphed(*prepared[k % 8], **batch_args(variant, k))
                torch.cuda.synchronize()
                run['ms'].append(1e3 * (time.perf_counter() - t0) / batches)
        for run in runs:
            ms = sorted(run['ms'])
            tr = run['trainer']
            rec = {'tree': tree, 'scale': scale, 'model': kind, 'variant': run['variant'], 'batch_ms_median': round(ms[len(ms) // 2], 4),
                   'batch_ms_min': round(ms[0], 4), 'batch_ms_max': round(ms[-1], 4), 'rounds': rounds, 'batches_per_round': batches,
                   'captures': int(getattr(tr, 'capture_count', len(tr._graphs))), 'steps': tr.t,
                   'loss_sum_finite': bool(abs(tr.pop_loss_sum()) < float('inf')), 'entry_points': len(run['points']),
                   'launch_list': hashlib.sha1(','.join(run['points']).encode()).hexdigest()[:12],
                   'loss_entry': [p for p in run['points'] if p.startswith('amar_loss_grad') or p.startswith('amar_bce_grad')]}
            print(json.dumps(rec), flush=True)
            if out:
                os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                with open(out, 'a') as fp:
                    fp.write(json.dumps(rec) + '\n')
        del runs


if __name__ == '__main__':
    main()

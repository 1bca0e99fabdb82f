#!/usr/bin/env python
"""What the compiled loss kernel and its metric counters cost a replayed training batch: Adam on BasicGCN and
HybridBertGCN at ml1m(s), batch 1 024, under three compiles:
    bce_none       loss='binary_crossentropy', no metrics
    bce_accuracy   loss='binary_crossentropy', metrics=['accuracy']              (what bench.py compiles: counters on)
    mse_all        loss='mean_squared_error', metrics=['accuracy', 'Precision', 'Recall', 'AUC']
usage: python tools/exp_losses_metrics.py <scale> [<rounds> [<batches> [<out.jsonl> [<variants> [<label>]]]]]
       <variants>: comma-separated subset (default: all).  The first two also run on a tree without the feature, where compile()
       ignores both arguments and the batch runs amar_bce_grad_f32: that run, labelled e.g. `parent`, is their reference point.
Per model every variant gets its own model and trainer, four batches (eager, capture, two replays), then <rounds> rounds; in a round
every variant replays <batches> batches, timed with the host clock around a device synchronise — the variants alternate inside a round,
so a drift of the machine meets all of them.  Reported: the median over the rounds of the ms per batch and the rounds' smallest and
largest value (the run-to-run spread)."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

VARIANTS = {'bce_none': dict(loss='binary_crossentropy', metrics=None),
            'bce_accuracy': dict(loss='binary_crossentropy', metrics=['accuracy']),
            'mse_all': dict(loss='mean_squared_error', metrics=['accuracy', 'Precision', 'Recall', 'AUC'])}
HYBRID_GRID1 = dict(embedding_dim=8, n_hiddens=[8, 8], dense_units=[[24, 24], [256, 64], [64, 64]], clf_units=[64, 64], feature_based=True)


def main():
    scale = int(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    batches = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    out = sys.argv[4] if len(sys.argv) > 4 else None
    names = sys.argv[5].split(',') if len(sys.argv) > 5 else list(VARIANTS)
    label = sys.argv[6] if len(sys.argv) > 6 else 'feature'
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
    prepared = []
    for _ in range(8):
        idx = torch.randint(0, pairs.shape[0], (bs,), device=dev, generator=gen)
        prepared.append((pairs[idx, 0].to(torch.int32), pairs[idx, 1].to(torch.int32),
                         (torch.rand(bs, device=dev, generator=gen) < 0.57).to(torch.float32)))
    bert = torch.randn((n, 768), device=dev, generator=gen) * 0.5

    def build(kind, compile_args):
        engine.set_seed(42)
        if kind == 'BasicGCN':
            model = basic.BasicGCN(a, embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
        else:
            model = hybrid.HybridBertGCN(a, **HYBRID_GRID1)
            model.set_bert_table(bert)
        model.compile(**compile_args)
        return model

    for kind in ('BasicGCN', 'HybridBertGCN'):
        runs = []
        for name in names:
            tr = training.Trainer(build(kind, VARIANTS[name]), rule='Adam')
            for k in range(4):
                tr.train_batch_graphed(*prepared[k % 8])
            torch.cuda.synchronize()
            assert tr._graphs
            runs.append({'variant': name, 'trainer': tr, 'ms': []})
        for _ in range(rounds):
            for run in runs:
                tr = run['trainer']
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(batches):
                    tr.train_batch_graphed(*prepared[k % 8])
                torch.cuda.synchronize()
                run['ms'].append(1e3 * (time.perf_counter() - t0) / batches)
        base = None
        for run in runs:
            ms = sorted(run['ms'])
            median = ms[len(ms) // 2]
            base = base if base is not None else median
            tr = run['trainer']
            counted = int(tr._counters[:4].sum().item()) if getattr(tr, '_counters', None) is not None else 0
            rec = {'tree': label, 'scale': scale, 'model': kind, 'variant': run['variant'], 'batch_ms_median': round(median, 4),
                   'batch_ms_min': round(ms[0], 4), 'batch_ms_max': round(ms[-1], 4), 'vs_first_variant': round(median / base, 4),
                   'rounds': rounds, 'batches_per_round': batches, 'pairs_counted': counted,
                   'loss_sum_finite': bool(abs(tr.pop_loss_sum()) < float('inf'))}
            print(json.dumps(rec), flush=True)
            if out:
                os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                with open(out, 'a') as fp:
                    fp.write(json.dumps(rec) + '\n')
        del runs


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""What a learning rate kept on the device costs a replayed training batch: Adam with a constant rate against Adam under
ExponentialDecay, on BasicGCN and HybridBertGCN at ml1m(s).
usage: python tools/exp_lr_schedules.py <scale> [<rounds> [<batches> [<out.jsonl> [<variants> [<tree label>]]]]]
       (BasicGCN 8 x 2, dense [24, 24], clf [48, 48]; HybridBertGCN grid1 with a resident 768-d table; batch 1 024)
       <variants>: comma-separated subset of constant,exponential (default: both).  `constant` alone runs on a tree without the feature
       too: copy this file into the parent commit's tree, run it there with the label `parent`, and run it here with the label `this` —
       in ONE session, the two commands alternating, so that a drift of the machine meets both trees.
Per model every variant gets its own trainer, four batches (eager, capture, two replays), then <rounds> rounds; in a round every variant
replays <batches> batches, timed with the host clock around a device synchronise; the variants alternate inside a round.  Reported: the
median over the rounds of the ms per batch and the rounds' smallest and largest value (the run-to-run spread), and `dynamic_rate`: False
means the trainer advances with the entry points that take the rate as an argument — the launches of the parent commit."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

HYBRID_GRID1 = dict(embedding_dim=8, n_hiddens=[8, 8], dense_units=[[24, 24], [256, 64], [64, 64]], clf_units=[64, 64], feature_based=True)


def variants(names):
    out = {}
    for name in names:
        if name == 'constant':
            out[name] = dict(learning_rate=1e-3)
        elif name == 'exponential':
            from deep_cbrs_amar_renaissance_amd.utilities.schedules import ExponentialDecay
            out[name] = dict(learning_rate=ExponentialDecay(1e-3, 1000, 0.96))
        else:
            raise SystemExit("no variant '{}': constant, exponential".format(name))
    return out


def main():
    scale = int(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    batches = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    out = sys.argv[4] if len(sys.argv) > 4 else None
    names = sys.argv[5].split(',') if len(sys.argv) > 5 else ['constant', 'exponential']
    tree = sys.argv[6] if len(sys.argv) > 6 else 'this'
    from deep_cbrs_amar_renaissance_amd import capi, engine, training
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    from deep_cbrs_amar_renaissance_amd.utilities.math import gcn_filter_device
    capi.load()
    chosen = variants(names)
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

    def build(kind):
        engine.set_seed(42)
        if kind == 'BasicGCN':
            return basic.BasicGCN(a, embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
        model = hybrid.HybridBertGCN(a, **HYBRID_GRID1)
        model.set_bert_table(bert)
        return model

    for kind in ('BasicGCN', 'HybridBertGCN'):
        runs = []
        for name, hyper in chosen.items():
            tr = training.Trainer(build(kind), rule='Adam', **hyper)
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
        for run in runs:
            ms = sorted(run['ms'])
            tr = run['trainer']
            rec = {'tree': tree, 'scale': scale, 'model': kind, 'variant': run['variant'], 'batch_ms_median': round(ms[len(ms) // 2], 4),
                   'batch_ms_min': round(ms[0], 4), 'batch_ms_max': round(ms[-1], 4), 'rounds': rounds, 'batches_per_round': batches,
                   'dynamic_rate': bool(getattr(tr, 'dynamic_rate', False)), 'steps': tr.t,
                   'loss_sum_finite': bool(abs(tr.pop_loss_sum()) < float('inf'))}
            print(json.dumps(rec), flush=True)
            if out:
                os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                with open(out, 'a') as fp:
                    fp.write(json.dumps(rec) + '\n')
        del runs


if __name__ == '__main__':
    main()

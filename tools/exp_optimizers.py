#!/usr/bin/env python
"""The update launch of a replayed training batch under every optimizer rule: its time and the bytes it moves.
usage: python tools/exp_optimizers.py <scale> [<reps> [<out.jsonl>]]      (BasicGCN 8 x 2, dense [24, 24], clf [48, 48], batch 1 024)
Per rule: a trainer runs four batches (eager, capture, two replays), then the update launch of the captured batch — the slot table the
graph replays, the gradient buffers of that graph — is timed alone with device events over <reps> launches (alternating with the other
rules' launches, so that a drift of the machine meets all of them).  Bytes: w and every state array read and written, the gradient (or
its G deferred partials) read."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

RULES = [('Adam', {}), ('SGD', {}), ('SGD', dict(momentum=0.9)), ('SGD', dict(momentum=0.9, nesterov=True)), ('RMSprop', {}),
         ('RMSprop', dict(momentum=0.9)), ('RMSprop', dict(centered=True)), ('RMSprop', dict(momentum=0.9, centered=True)),
         ('Adagrad', {}), ('Adamax', {}), ('Nadam', {}), ('AMSGrad', {})]


def main():
    scale = int(sys.argv[1])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    out = sys.argv[3] if len(sys.argv) > 3 else None
    from deep_cbrs_amar_renaissance_amd import capi, engine, training
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.math import gcn_filter_device
    capi.load()
    dev = torch.device('cuda')
    data = synthetic.ml1m_device(scale, device=dev)
    n = data['n_users'] + data['n_items']
    a = gcn_filter_device(data['train_pos'][:, 0], data['train_pos'][:, 1], n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    pairs, bs = data['train_pos'], 1024
    idx = torch.randint(0, pairs.shape[0], (bs,), device=dev, generator=gen)
    batch = (pairs[idx, 0].to(torch.int32), pairs[idx, 1].to(torch.int32), (torch.rand(bs, device=dev, generator=gen) < 0.57).to(torch.float32))
    launches = []
    for rule, hyper in RULES:
        engine.set_seed(42)
        model = basic.BasicGCN(a, embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
        tr = training.Trainer(model, rule=rule, **hyper)
        for _ in range(4):
            tr.train_batch_graphed(*batch)
        torch.cuda.synchronize()
        g = tr._g
        n_slots = len(g['keep'])
        blocks = sum((e[0].numel() + 1023) // 1024 for e in g['keep'])
        floats = 0
        for e in g['keep']:
            grad = e[1]
            floats += e[0].numel() * (2 + 2 * tr.spec.n_arrays) + (grad.partials.numel() if isinstance(grad, capi.DeferredGradient) else grad.numel())

        def launch(tr=tr, g=g, n_slots=n_slots, blocks=blocks):
            s = tr.spec
            capi.optim_multi(s.code, s.flags, s.hyper, g['slot_dev'], n_slots, blocks, tr._opt_state, reg_scale=float(bs), loss_acc=tr._loss_sum)
        name = rule + ''.join('+' + k for k, v in hyper.items() if v)
        launches.append({'rule': name, 'launch': launch, 'bytes': 4 * floats, 'keep': (tr, model), 'events': [],
                         'state_arrays': tr.spec.n_arrays, 'parameters': sum(e[0].numel() for e in g['keep']), 'slots': n_slots})
    for entry in launches:                                           # warm every launch
        for _ in range(5):
            entry['launch']()
    torch.cuda.synchronize()
    for _ in range(reps):                                            # alternate the rules inside the timed window
        for entry in launches:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            entry['launch']()
            stop.record()
            entry['events'].append((start, stop))
    torch.cuda.synchronize()
    adam = None
    for entry in launches:
        times = sorted(a_.elapsed_time(b_) for a_, b_ in entry['events'])
        us = 1e3 * times[len(times) // 2]
        adam = adam or (us, entry['bytes'])
        rec = {'scale': scale, 'rule': entry['rule'], 'state_arrays': entry['state_arrays'], 'parameters': entry['parameters'],
               'slots': entry['slots'], 'update_us_median': round(us, 2), 'update_us_p10': round(1e3 * times[len(times) // 10], 2),
               'update_us_p90': round(1e3 * times[(9 * len(times)) // 10], 2), 'bytes': entry['bytes'],
               'gb_per_s': round(entry['bytes'] / us / 1e3, 1), 'time_vs_adam': round(us / adam[0], 3),
               'bytes_vs_adam': round(entry['bytes'] / adam[1], 3), 'reps': reps}
        print(json.dumps(rec), flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, 'a') as fp:
                fp.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

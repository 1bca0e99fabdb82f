#!/usr/bin/env python
"""A replayed triplet batch under the listwise losses (SampledSoftmaxLoss, HardestNegativeBPRLoss, MarginRankingLoss) against the same
batch under BPRLoss, BasicLightGCN and BasicGCN at ml1m(s=1), batch 1 024, n_negatives in {1, 4, 16}.

One JSON line per (model, n_negatives, loss) in profiles/exp_group_losses.jsonl:
  us_per_batch_median / _min / _max  over the rounds; a round times BATCHES replayed batches of every variant one after the other
                                     (host clock around a device synchronise), so drift of the shared host hits the variants alike
  vs_bpr_us_median / _min / _max     the per-round difference to this tree's BPRLoss batch of the same model and n_negatives
With --parent DIR (a built checkout of the parent commit) every round also runs the BPRLoss variants from that tree in a child
process (and from this tree in another child, same code path), alternating: lines 'tree': 'parent' / 'this (child)'; the yardstick
of a BPRLoss batch is the parent's, and the two children show what a process boundary itself moves.
--bpr-only: what a child runs (BPRLoss variants only, JSON lines on stdout, no file).  AMAR_TREE: the tree to import from.
The entry points a BPRLoss batch calls are listed once per tree ('bpr_entry_points': the amar_* symbols called during one eager batch).

    python tools/exp_group_losses.py [rounds] [--parent DIR]        (repo root, GPU box; writes profiles/exp_group_losses.jsonl)
"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get('AMAR_TREE', HERE)
sys.path.insert(0, ROOT)
import numpy as np
import torch

CFG = {'BasicLightGCN': dict(embedding_dim=16, n_layers=2, dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4),
       'BasicGCN': dict(embedding_dim=16, n_hiddens=[16, 16], dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4)}
NEGATIVES = (1, 4, 16)
BATCHES = 300


def sequences():
    from deep_cbrs_amar_renaissance_amd.data import loaders, preprocess, synthetic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphTriplets
    ds = synthetic.ml1m(1, with_props=False)
    (train, _), (users, items) = loaders.index_ratings(ds.train, ds.test)
    train = train[np.isin(train[:, 0], train[train[:, 2] == 1, 0])]
    adj = preprocess.build_adjacency_matrix(train, users, items)
    return {K: UserItemGraphTriplets(train, users, items, adj, batch_size=1024, n_negatives=K) for K in NEGATIVES}


def loss_variants(bpr_only):
    from deep_cbrs_amar_renaissance_amd.utilities import losses
    out = {'BPRLoss': losses.BPRLoss}
    if not bpr_only:
        out.update({'SampledSoftmaxLoss(0.2)': lambda: losses.SampledSoftmaxLoss(temperature=0.2),
                    'HardestNegativeBPRLoss': losses.HardestNegativeBPRLoss, 'MarginRankingLoss(0.5)': losses.MarginRankingLoss})
    return out


class Variant:
    """A model with its trainer and sampler, warmed until its batch is replayed from the captured graph."""

    def __init__(self, cls, seq, loss):
        from deep_cbrs_amar_renaissance_amd import engine, training
        from deep_cbrs_amar_renaissance_amd.experiment import Adam
        from deep_cbrs_amar_renaissance_amd.models import basic
        engine.set_seed(42)
        self.model = getattr(basic, cls)(seq.adj_matrix, **CFG[cls])
        self.model.compile(loss=loss, optimizer=Adam(learning_rate=1e-3))
        self.model(seq[0][0])
        self.trainer = training.Trainer(self.model)
        self.sampler = self.trainer.sampler_for(seq)
        for _ in range(5):
            self.trainer.train_sampled(self.sampler)
        torch.cuda.synchronize()
        assert self.trainer._graphs

    def us_per_batch(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(BATCHES):
            self.trainer.train_sampled(self.sampler)
        torch.cuda.synchronize()
        self.trainer.pop_loss_sum()
        return (time.perf_counter() - t0) * 1e6 / BATCHES


def bpr_entry_points(cls, seq):
    """The amar_* symbols one eager BPRLoss batch calls, in first-call order."""
    from deep_cbrs_amar_renaissance_amd import capi, engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    engine.set_seed(42)
    model = getattr(basic, cls)(seq.adj_matrix, **CFG[cls])
    model.compile(loss=BPRLoss())
    model(seq[0][0])
    trainer = training.Trainer(model)
    sampler = trainer.sampler_for(seq)
    trainer.train_sampled(sampler, graph=False)
    lib, seen = capi.load(), []

    class Spy:
        def __getattr__(self, name):
            if name.startswith('amar_') and name not in seen:
                seen.append(name)
            return getattr(lib, name)
    original = capi.load
    capi.load = lambda: Spy()
    try:
        trainer.train_sampled(sampler, graph=False)
        torch.cuda.synchronize()
    finally:
        capi.load = original
    return seen


def stats(values, prefix):
    return {prefix + '_median': round(float(np.median(values)), 2), prefix + '_min': round(float(min(values)), 2),
            prefix + '_max': round(float(max(values)), 2)}


def measure(rounds, bpr_only):
    seqs = sequences()
    variants = {(cls, K, name): Variant(cls, seqs[K], make()) for cls in CFG for K in NEGATIVES
                for name, make in loss_variants(bpr_only).items()}
    times = {key: [] for key in variants}
    for _ in range(rounds):
        for key, v in variants.items():                               # interleaved: every variant in every round
            times[key].append(v.us_per_batch())
    lines = []
    for (cls, K, name), t in times.items():
        rec = {'dataset': 'ml1m(s=1)', 'model': cls, 'n_negatives': K, 'loss': name, 'batch': 1024, 'rounds': rounds,
               'batches_per_round': BATCHES}
        rec.update(stats(t, 'us_per_batch'))
        if name != 'BPRLoss':
            rec.update(stats(np.array(t) - np.array(times[(cls, K, 'BPRLoss')]), 'vs_bpr_us'))
        lines.append(rec)
    lines.append({'bpr_entry_points': {cls: bpr_entry_points(cls, seqs[4]) for cls in CFG}})
    return lines


def children(parent, rounds):
    """BPRLoss batches from the parent's tree and from this one, one child process each per repeat, alternating."""
    out = {'parent': [], 'this (child)': []}
    for _ in range(3):
        for tree, root in (('parent', parent), ('this (child)', HERE)):
            env = dict(os.environ, AMAR_TREE=os.path.abspath(root))
            done = subprocess.run([sys.executable, os.path.abspath(__file__), str(rounds), '--bpr-only'], env=env, capture_output=True,
                                  text=True, timeout=600, check=True)
            out[tree].append([json.loads(line) for line in done.stdout.splitlines() if line.startswith('{')])
    lines = []
    for tree, runs in out.items():
        for k, rec in enumerate(runs[0]):
            if 'bpr_entry_points' in rec:
                lines.append(dict(rec, tree=tree))
                continue
            med = [run[k]['us_per_batch_median'] for run in runs]
            rec = {key: rec[key] for key in ('dataset', 'model', 'n_negatives', 'loss', 'batch', 'rounds', 'batches_per_round')}
            rec.update(tree=tree, processes=len(runs), us_per_batch_medians=med)
            rec.update(stats(med, 'us_per_batch'))
            lines.append(rec)
    return lines


def main():
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    bpr_only = '--bpr-only' in sys.argv
    parent = sys.argv[sys.argv.index('--parent') + 1] if '--parent' in sys.argv else None
    if parent in args:
        args.remove(parent)
    rounds = int(args[0]) if args else 7
    lines = measure(rounds, bpr_only)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if bpr_only:
        return
    if parent:
        more = children(parent, rounds)
        for rec in more:
            print(json.dumps(rec), flush=True)
        lines += more
    with open(os.path.join(HERE, 'profiles', 'exp_group_losses.jsonl'), 'w') as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

"""Directed graphs: what the device transpose costs, and what a training batch costs on a directed graph.

Appends JSON lines to profiles/exp_directed.jsonl (one GPU process; warm-up, repeats, median and spread reported):

  transpose   amar_csr_transpose_i32 on the un-symmetrised ml1m(s) rating graph, s in --scales, beside scipy transposing the same CSR
              on the host plus the download and the upload it would need.  Information only.
  batch       a replayed training batch of BasicGCN and BasicGAT at ml1m(s=1) on the directed graph, beside the same model on the
              symmetrised graph.  Information only: the graphs differ in size.
  train_s1    with --bench-json FILE [FILE ...] (branch) and --parent-json FILE [FILE ...] (parent commit): the `train_s1` figure of
              bench.py result lines from both commits, run in one session — the one guard of the change: a symmetric graph takes
              the old path, so the branch should sit inside the spread the parent shows across its own repeats.

    python tools/exp_directed.py --scales 1 8 64
    python tools/exp_directed.py --bench-json branch_1.json branch_2.json --parent-json parent_1.json parent_2.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'exp_directed.jsonl')


def emit(record):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'a') as f:
        f.write(json.dumps(record) + '\n')
    print(json.dumps(record), flush=True)


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'n': len(xs)}


def directed_csr(scale):
    import torch
    from deep_cbrs_amar_renaissance_amd.data import loaders, synthetic
    ds = synthetic.ml1m(scale)
    (train, _), (users, items) = loaders.index_ratings(ds.train, ds.test)
    pos = train[train[:, 2] == 1] if train.shape[1] > 2 else train
    n = len(users) + len(items)
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    row, col = pos[order, 0], pos[order, 1]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int32)
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(col.astype(np.int32)).cuda(), n


def time_transpose(scale, repeats):
    import torch
    from scipy import sparse
    from deep_cbrs_amar_renaissance_amd import capi
    rowptr, colidx, n = directed_csr(scale)
    for _ in range(2):
        capi.csr_transpose(rowptr, colidx, n)
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        capi.csr_transpose(rowptr, colidx, n)
        torch.cuda.synchronize()
        dev.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        m = sparse.csr_matrix((np.arange(colidx.numel(), dtype=np.int32), colidx.cpu().numpy(), rowptr.cpu().numpy()), shape=(n, n)).tocsc()
        back = [torch.from_numpy(a).cuda() for a in (m.indptr, m.indices, m.data)]
        torch.cuda.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
        del back
    emit({'what': 'transpose', 'scale': scale, 'n': n, 'nnz': int(colidx.numel()), 'device_ms (incl. the wrapper\'s checks)': spread(dev),
          'scipy_plus_copies_ms': spread(host)})


def time_batches(repeats):
    import torch
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    g = helpers.ml1m_indexed(1)
    directed = build_adjacency_matrix(g['train'], g['users'], g['items'], symmetric_adjacency=False)
    rng = np.random.default_rng(0)
    pick = rng.integers(0, len(g['train']), 1024)
    u, i, y = g['train'][pick, 0], g['train'][pick, 1], g['train'][pick, 2]
    for cls in ('BasicGCN', 'BasicGAT'):
        for label, adj in (('symmetrised', g['adj_ui']), ('directed', directed)):
            engine.set_seed(42)
            model = getattr(basic, cls)(adj, embedding_dim=16, n_hiddens=[16, 16], dense_units=[48, 48], clf_units=[64, 64], l2_regularizer=1e-4)
            trainer = training.Trainer(model)
            for _ in range(5):                                     # eager, capture, replays
                trainer.train_batch_graphed(u, i, y)
            torch.cuda.synchronize()
            times = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(50):
                    trainer.train_batch_graphed(u, i, y)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0) / 50)
            emit({'what': 'batch', 'model': cls, 'graph': label, 'nnz': int(trainer.tapes[0].seq.adj_matrix.nnz), 'ms_per_batch': spread(times)})


def train_s1_of(paths):
    vals = []
    for p in paths:
        for line in open(p):
            line = line.strip()
            if line.startswith('{') and 'train_s1' in line:
                vals.append(float(json.loads(line)['train_s1']['ms_per_batch']))
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='*', default=[1, 8, 64])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--skip-batches', action='store_true')
    ap.add_argument('--bench-json', nargs='*', default=[])
    ap.add_argument('--parent-json', nargs='*', default=[])
    args = ap.parse_args()
    if args.bench_json or args.parent_json:
        branch, parent = train_s1_of(args.bench_json), train_s1_of(args.parent_json)
        emit({'what': 'train_s1', 'branch_ms_per_batch': branch, 'parent_ms_per_batch': parent,
              'inside_parent_spread': bool(parent and branch and min(parent) <= statistics.median(branch) <= max(parent))})
        return
    for s in args.scales:
        time_transpose(s, args.repeats)
    if not args.skip_batches:
        time_batches(args.repeats)


if __name__ == '__main__':
    main()

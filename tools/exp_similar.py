"""Similar-item search (similar_items(), every item, k = 10, cosine, space='graph', the item itself excluded) on BasicGCN at
ml1m(s=1) and ml1m(s=8): the fused kernel (amar_nearest_f32) against a yardstick built here from library calls on the same
device table — torch.nn.functional.normalize, a chunked torch.mm (chunks of at most --chunk-floats scores), the diagonal set to
-inf, torch.topk.

Per scale, one JSON line: the end-to-end similar_items() call (propagation, search, lists to the host), the search alone
(capi.nearest on the cached table) and the yardstick, each as the median of --rounds rounds with its min / max (the run-to-run
spread); the two are timed alternately inside every round, after a warm-up of both; every timed window runs --inner calls and
ends in a device synchronise.  Also: the largest intermediate the yardstick allocates (a chunk's score matrix) against the
kernel's workspace, and how many lists agree between the two.

Usage: python tools/exp_similar.py [--scales 1 8] [--rounds 7] [--inner 5] [--out profiles/exp_similar.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def _window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def _stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'all_ms': [round(x, 4) for x in ms]}


def yardstick(table, k, chunk_floats):
    """Library calls only: normalise, chunked mm, diagonal to -inf, topk.  Returns (rows int64 [n, k], scores, bytes of a chunk's scores)."""
    n = table.shape[0]
    unit = torch.nn.functional.normalize(table, dim=1, eps=0.0).nan_to_num_(0.0)
    chunk = max(1, min(n, chunk_floats // max(1, n)))
    rows, scores = [], []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        s = torch.mm(unit[lo:hi], unit.t())
        s[torch.arange(hi - lo, device=s.device), torch.arange(lo, hi, device=s.device)] = float('-inf')
        top = torch.topk(s, min(k, n), dim=1)
        rows.append(top.indices)
        scores.append(top.values)
    return torch.cat(rows), torch.cat(scores), chunk * n * 4


def run_scale(scale, args):
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    d = helpers.ml1m_indexed(scale)
    nu, ni = len(d['users']), len(d['items'])
    engine.set_seed(1)
    model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
    train = _Train(d['train'], nu, ni)
    k = 10
    table = model._item_embeddings(train, 'graph')
    width = int(table.shape[1])
    q_rows = torch.arange(ni, dtype=torch.int32, device=table.device)
    excl = (torch.arange(ni + 1, dtype=torch.int32, device=table.device), q_rows)
    kernel = lambda: capi.nearest(table, table, k, metric='cosine', query_rows=q_rows, excl_ptr=excl[0], excl_rows=excl[1])
    yard = lambda: yardstick(table, k, args.chunk_floats)
    whole = lambda: model.similar_items(train, k=k, metric='cosine', space='graph')
    for fn in (kernel, yard, whole):                       # warm-up: code objects, library algorithm choices, the allocator
        _window(fn, 2)
    t_kernel, t_yard, t_whole = [], [], []
    for _ in range(args.rounds):
        t_kernel.append(_window(kernel, args.inner)[0])
        t_yard.append(_window(yard, args.inner)[0])
        t_whole.append(_window(whole, args.inner)[0])
    (k_rows, k_scores), (y_rows, y_scores, y_bytes) = kernel(), yard()
    same = (k_rows.to(torch.int64) == y_rows).all(dim=1)
    lib = capi.load()
    slices = int(lib.amar_nearest_slices(ni, ni, width, 0))
    ws_floats = int(lib.amar_nearest_workspace_floats(ni, ni, k, capi.NEAREST_METRICS['cosine'], slices))
    res = {'case': 'BasicGCN graph space ml1m(s={})'.format(scale), 'items': ni, 'width': width, 'k': k, 'metric': 'cosine',
           'pairs': ni * ni, 'rounds': args.rounds, 'calls_per_window': args.inner,
           'kernel': _stats(t_kernel), 'yardstick': _stats(t_yard), 'similar_items_end_to_end': _stats(t_whole),
           'kernel_over_yardstick': float(np.median(t_kernel) / np.median(t_yard)),
           'table_slices': slices, 'kernel_workspace_bytes': 4 * ws_floats + (4 * ni * slices * k if slices > 1 else 0),
           'score_matrix_bytes': 4 * ni * ni, 'yardstick_largest_intermediate_bytes': int(y_bytes),
           'lists_equal_to_yardstick': int(same.sum()), 'lists': ni,
           'max_score_diff_to_yardstick': float((k_scores - y_scores).abs().max())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--chunk-floats', type=int, default=1 << 27, help='scores per yardstick chunk (512 MB)')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_similar.py measures on the GPU: no device found")
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    torch.cuda.set_device(0)
    for s in args.scales:
        line = json.dumps(run_scale(s, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

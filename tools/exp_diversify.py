"""Diversified re-ranking (recommend_diverse(), every user, k = 10, cosine, space='graph', trade_off = 0.7) on BasicGCN at ml1m(s=1)
and ml1m(s=8), pools of P = 50 and P = 64: the fused launch (amar_rerank_mmr_f32) against a yardstick built here from library calls
on the same device pools and table — a gather of the pools' rows [m, P, d], torch.nn.functional.normalize, torch.bmm to the
[m, P, P] similarity tensor, the min-max relevance, then a k-step loop of masked argmax / gather / torch.maximum.

Per scale and P, one JSON line: the re-rank launch alone and the yardstick, each as the median of --rounds rounds with its
min / max (the run-to-run spread); the two are timed alternately inside every round, after a warm-up of both; every timed window
runs --inner calls between two device events.  Also: the yardstick's largest intermediate in bytes against the kernel's workspace
(none), how many lists agree between the two, and what recommend_diverse(pool=P) costs over recommend(k=P) (both with the lists
kept on the device, timed the same way).

Usage: python tools/exp_diversify.py [--scales 1 8] [--pools 50 64] [--rounds 7] [--inner 5] [--out profiles/exp_diversify.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def _window(fn, inner):
    """ms per call of `inner` calls between two device events, and the last result."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner, out


def _stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'all_ms': [round(x, 4) for x in ms]}


def yardstick(pool_items, pool_scores, table, k, trade_off):
    """Library calls only.  Returns (items int32 [m, k] (-1 where the pool ran out), bytes of the largest intermediate)."""
    m, P = pool_items.shape
    valid = pool_items >= 0
    rows = table[pool_items.clamp(min=0).to(torch.int64)]                              # [m, P, d]
    rows = torch.nn.functional.normalize(rows, dim=2, eps=0.0).nan_to_num_(0.0) * valid[:, :, None]
    sim = torch.bmm(rows, rows.transpose(1, 2))                                        # [m, P, P]
    inf = float('inf')
    lo = torch.where(valid, pool_scores, torch.full_like(pool_scores, inf)).min(dim=1, keepdim=True).values
    hi = torch.where(valid, pool_scores, torch.full_like(pool_scores, -inf)).max(dim=1, keepdim=True).values
    rel = torch.where(hi > lo, (pool_scores - lo) / (hi - lo), torch.ones_like(pool_scores))
    avail = valid.clone()
    pen = torch.full_like(pool_scores, -inf)
    every = torch.arange(m, device=pool_items.device)
    picks, alive = [], []
    for s in range(k):
        v = trade_off * rel if s == 0 else trade_off * rel - (1.0 - trade_off) * pen
        key = torch.where(avail, pool_scores if s == 0 else v, torch.full_like(v, -inf))
        t = key.argmax(dim=1)
        alive.append(avail[every, t])
        picks.append(t)
        avail[every, t] = False
        pen = torch.maximum(pen, sim[every, t])
    pos, alive = torch.stack(picks, dim=1), torch.stack(alive, dim=1)
    items = torch.where(alive, torch.gather(pool_items, 1, pos), torch.full_like(pos, -1, dtype=pool_items.dtype))
    return items, max(sim.numel(), rows.numel()) * 4


def run_case(model, train, scale, P, args):
    from deep_cbrs_amar_renaissance_amd import capi, recommend as rec
    k, lam = 10, 0.7
    with rec.device_lists():
        _, pool_items, pool_scores = model.recommend(train, k=P)
    pool_items, pool_scores = pool_items.contiguous(), pool_scores.contiguous()
    table = rec._as_device_matrix(model._item_embeddings(train, 'graph'), pool_items.device, 'table')
    m, width = int(pool_items.shape[0]), int(table.shape[1])
    kernel = lambda: capi.rerank_mmr(pool_items, pool_scores, table, k, trade_off=lam, metric='cosine')
    yard = lambda: yardstick(pool_items, pool_scores, table, k, lam)

    def plain():
        with rec.device_lists():
            return model.recommend(train, k=P)

    def diverse():
        with rec.device_lists():
            return model.recommend_diverse(train, k=k, pool=P, trade_off=lam, metric='cosine', space='graph')

    for fn in (kernel, yard, plain, diverse):                # warm-up: code objects, library algorithm choices, the allocator
        _window(fn, 2)
    t_kernel, t_yard, t_plain, t_diverse = [], [], [], []
    for _ in range(args.rounds):
        t_kernel.append(_window(kernel, args.inner)[0])
        t_yard.append(_window(yard, args.inner)[0])
        t_plain.append(_window(plain, args.inner)[0])
        t_diverse.append(_window(diverse, args.inner)[0])
    (k_items, _), (y_items, y_bytes) = kernel(), yard()
    same = (k_items == y_items).all(dim=1)
    return {'case': 'BasicGCN graph space ml1m(s={})'.format(scale), 'lists': m, 'items': len(train.items), 'width': width, 'pool': P,
            'k': k, 'trade_off': lam, 'metric': 'cosine', 'rounds': args.rounds, 'calls_per_window': args.inner,
            'kernel': _stats(t_kernel), 'yardstick': _stats(t_yard),
            'kernel_over_yardstick': float(np.median(t_kernel) / np.median(t_yard)),
            'kernel_workspace_bytes': 0, 'kernel_lds_bytes_per_list': 17408,
            'yardstick_largest_intermediate_bytes': int(y_bytes), 'similarity_tensor_bytes': 4 * m * P * P,
            'recommend_pool': _stats(t_plain), 'recommend_diverse': _stats(t_diverse),
            'diverse_over_recommend_ms': float(np.median(t_diverse) - np.median(t_plain)),
            'lists_equal_to_yardstick': int(same.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--pools', type=int, nargs='+', default=[50, 64])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_diversify.py measures on the GPU: no device found")
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    capi.load()
    torch.cuda.set_device(0)
    for s in args.scales:
        d = helpers.ml1m_indexed(s)
        nu, ni = len(d['users']), len(d['items'])
        engine.set_seed(1)
        model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
        train = _Train(d['train'], nu, ni)
        for P in args.pools:
            line = json.dumps(run_case(model, train, s, P, args))
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'a') as f:
                    f.write(line + '\n')
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

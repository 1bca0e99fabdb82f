"""Calibrated re-ranking (recommend_calibrated(), every user's pool of P = 64, k = 10, trade_off 0.5, smoothing 0.01, default categories)
on BasicGCN over the 'unary-uip' graph at ml1m(s=1) and ml1m(s=8).  The fused launch (amar_rerank_calibrated_f32) against a yardstick
built here from library calls on the same device pools and CSRs:

  target      a sparse product of the users' liked indicator [m, |I|] with the dense category rows [|I|, G] (1/len per cell),
              divided by the support;
  greedy      per chunk of users a gather of the pool's dense category rows [c, P, G], then k steps of: the candidate lists'
              distributions (n + row) / (|S+| + 1) (n / |S+| for a neutral candidate), log, sum over G, a masked argmax, and the
              update of n.

The yardstick works through the users in chunks sized so that the gathered rows stay near 1 GiB; its peak workspace is what
torch.cuda.max_memory_allocated reports above the inputs.  One JSON line per case: kernel and yardstick as min / median / max of
--samples timed calls between device events, taken alternately after a warm-up of both; recommend_calibrated(pool=64) against
recommend(k=64); and, under 'existing', the entry points that recommend(k=10) and recommend_diverse(k=10, pool=50) call with their
times (--existing-only prints that part alone, so that it can be run from a checkout of the parent commit and compared).

Usage: python tools/exp_calibrate.py [--scales 1 8] [--samples 5] [--out profiles/exp_calibrate.jsonl] [--existing-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, K, TRADE_OFF, SMOOTHING = 64, 10, 0.5, 0.01


class _Train:
    def __init__(self, ratings, n_users, n_items, adj):
        self.ratings, self.users, self.items, self.adj_matrix = ratings, np.arange(n_users), np.arange(n_items), adj


def _timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def _wall(fn):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ms):
    return {'min_ms': float(min(ms)), 'median_ms': float(np.median(ms)), 'max_ms': float(max(ms)), 'samples': len(ms)}


def make_yardstick(pool, scores, liked, cats):
    """Returns fn() -> chosen item rows int64 [m, K] (-1 padded)."""
    dev = pool.device
    m, G = int(pool.shape[0]), int(cats[2])
    cptr, cids = cats[0].to(torch.int64), cats[1].to(torch.int64)
    n_items = int(cptr.numel()) - 1
    lens = cptr[1:] - cptr[:-1]
    dense = torch.zeros((n_items + 1, G), dtype=torch.float32, device=dev)            # the dense rows are an input, built once; row |I| is padding
    dense[torch.repeat_interleave(torch.arange(n_items, device=dev), lens), cids] = torch.repeat_interleave(1.0 / lens.clamp(min=1).to(torch.float32), lens)
    has_row = torch.cat([lens > 0, torch.zeros(1, dtype=torch.bool, device=dev)])
    lptr, litems = liked[0].to(torch.int64), liked[1].to(torch.int64)
    ind = torch.sparse_csr_tensor(lptr, litems, has_row[litems].to(torch.float32), size=(m, n_items + 1))
    p64 = pool.to(torch.int64)
    valid = (p64 >= 0) & (p64 < n_items)
    idx = torch.where(valid, p64, torch.full_like(p64, n_items))
    chunk = max(1, (1 << 28) // (P * G))
    alpha, lam = SMOOTHING, TRADE_OFF

    def run():
        support = torch.sparse.mm(ind, has_row.to(torch.float32)[:, None])[:, 0]
        target = torch.sparse.mm(ind, dense) / support.clamp(min=1.0)[:, None]           # [m, G]
        out = []
        for lo in range(0, m, chunk):
            ix, ok, sc, p = idx[lo:lo + chunk], valid[lo:lo + chunk], scores[lo:lo + chunk], target[lo:lo + chunk]
            c = int(ix.shape[0])
            rows = dense[ix]                                                             # [c, P, G]
            full = has_row[ix]                                                           # [c, P]
            lo_s = torch.where(ok, sc, torch.full_like(sc, float('inf'))).min(1, keepdim=True).values
            hi_s = torch.where(ok, sc, torch.full_like(sc, float('-inf'))).max(1, keepdim=True).values
            rel = torch.where(hi_s > lo_s, (sc - lo_s) / (hi_s - lo_s), torch.ones_like(sc))
            has_target = (support[lo:lo + chunk] > 0)[:, None]
            n = torch.zeros((c, G), dtype=torch.float32, device=dev)
            cnt = torch.zeros((c, 1), dtype=torch.float32, device=dev)
            free = ok.clone()
            ap = (alpha * p)[:, None, :]
            live = (p > 0)[:, None, :]
            chosen = torch.full((c, K), -1, dtype=torch.int64, device=dev)
            ar = torch.arange(c, device=dev)
            for s in range(K):
                norm = (cnt + full.to(torch.float32)).clamp(min=1.0)[:, :, None]
                q = (n[:, None, :] + rows) / norm
                term = torch.where(live, p[:, None, :] * torch.log(p[:, None, :].clamp(min=1e-38) / ((1.0 - alpha) * q + ap).clamp(min=1e-38)), torch.zeros_like(q))
                v = lam * rel - (1.0 - lam) * term.sum(2)
                key = torch.where(has_target, v, sc).masked_fill(~free, float('-inf'))
                t = key.argmax(1)
                got = free[ar, t]
                chosen[:, s] = torch.where(got, ix[ar, t], torch.full_like(t, -1))
                n = n + rows[ar, t] * got[:, None]
                cnt = cnt + (full[ar, t] & got)[:, None].to(torch.float32)
                free[ar, t] = False
            out.append(chosen)
        return torch.cat(out)
    return run


def existing_paths(model, train, samples):
    """The entry points recommend(k=10) and recommend_diverse(k=10, pool=50) call, and their wall times."""
    from deep_cbrs_amar_renaissance_amd import capi
    called = []
    launch, call = capi._launch, capi._call

    def spy(fn):
        def wrapped(symbol, *args):
            called.append(symbol)
            return fn(symbol, *args)
        return wrapped

    out = {}
    for name, fn in (('recommend', lambda: model.recommend(train, k=10)),
                     ('recommend_diverse', lambda: model.recommend_diverse(train, k=10, pool=50))):
        fn()
        capi._launch, capi._call = spy(launch), spy(call)
        try:
            del called[:]
            fn()
        finally:
            capi._launch, capi._call = launch, call
        out[name] = dict(_stats([_wall(fn)[0] for _ in range(samples)]), entry_points=list(called))
    return out


def run_case(scale, args):
    from deep_cbrs_amar_renaissance_amd import engine, recommend as rec
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    d = helpers.ml1m_indexed(scale)
    nu, ni = len(d['users']), len(d['items'])
    adj = d['adj_uip']
    engine.set_seed(1)
    model = basic.BasicGCN(adj, embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
    train = _Train(d['train'], nu, ni, adj)
    line = {'case': 'BasicGCN ml1m(s={}) unary-uip'.format(scale), 'lists': nu, 'items': ni,
            'existing': existing_paths(model, train, args.samples)}
    if args.existing_only:
        return line
    with rec.device_lists():
        _, pool, scores = model.recommend(train, k=P)
    pool, scores = pool.contiguous(), scores.contiguous()
    liked, cats = rec._liked_device(train, nu, ni), rec._cats_device(train, ni, None)
    kernel = lambda: rec.rerank_calibrated(pool, scores, None, liked, cats, K, trade_off=TRADE_OFF, smoothing=SMOOTHING)[0]
    yard = make_yardstick(pool, scores, liked, cats)
    for fn in (kernel, yard):
        fn(), fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y_items = yard()
    torch.cuda.synchronize()
    y_peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    k_items = kernel()
    torch.cuda.synchronize()
    k_peak = torch.cuda.max_memory_allocated() - base
    t_kernel, t_yard = [], []
    for _ in range(args.samples):
        t_kernel.append(_timed(kernel)[0])
        t_yard.append(_timed(yard)[0])
    t_cal = [_wall(lambda: model.recommend_calibrated(train, k=K, pool=P, trade_off=TRADE_OFF, smoothing=SMOOTHING))[0] for _ in range(args.samples)]
    t_rec = [_wall(lambda: model.recommend(train, k=P))[0] for _ in range(args.samples)]
    line.update({'P': P, 'k': K, 'trade_off': TRADE_OFF, 'smoothing': SMOOTHING, 'categories': int(cats[2]), 'longest_category_row': int(cats[3]),
                 'category_links': int(cats[1].numel()), 'liked_total': int(liked[1].numel()),
                 'liked_longest': int((liked[0][1:] - liked[0][:-1]).max()),
                 'kernel': _stats(t_kernel), 'yardstick': _stats(t_yard), 'kernel_over_yardstick': float(np.median(t_kernel) / np.median(t_yard)),
                 'kernel_workspace_bytes': 0, 'kernel_outputs_bytes': int(k_peak), 'yardstick_peak_workspace_bytes': int(y_peak),
                 'm_P_G_tensor_bytes': nu * P * int(cats[2]) * 4,
                 'lists_equal_to_yardstick': int((k_items.to(torch.int64) == y_items).all(dim=1).sum()),
                 'recommend_calibrated_pool_64': _stats(t_cal), 'recommend_k_64': _stats(t_rec),
                 'recommend_calibrated_minus_recommend_ms': float(np.median(t_cal) - np.median(t_rec))})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', nargs='+', type=int, default=[1, 8])
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--existing-only', action='store_true')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_calibrate.py measures on the GPU: no device found")
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    torch.cuda.set_device(0)
    for scale in args.scales:
        line = json.dumps(run_case(scale, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

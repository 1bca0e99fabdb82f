"""Explanations (explain(), every user's top 10, cosine, space='graph', n_evidence = 3, n_properties = 3) on BasicGCN: ml1m(s=1) and
ml1m(s=8) on the 'unary' graph (evidence only: the graph holds no properties) and ml1m(s=1) on the 'unary-uip' graph (evidence and
shared properties).  The fused launch (amar_explain_f32) against a yardstick built here from library calls on the same device lists,
table and CSRs:

  evidence    liked lists padded to the longest, per chunk of users a gather of their rows [c, Lmax, d] and of the targets' rows
              [c, K, d] (both normalised once per table), torch.bmm to [c, K, Lmax], a mask (padding, the target itself), torch.topk;
  properties  the positive similarities scattered into a dense [c K, |I|] matrix, a sparse membership product with the |I| x |P|
              item-property matrix for the sums and one with the indicator for the supports, a mask by the target's own row, the
              IDF weights, torch.topk.

The yardstick works through the users in chunks sized so that its gathered rows stay near 1 GiB; its peak workspace is what
torch.cuda.max_memory_allocated reports above the inputs.  One JSON line per case: kernel and yardstick as the median of --rounds
timed calls with min / max, timed alternately after a warm-up of both, the peak workspace, and how many evidence lists agree.

Usage: python tools/exp_explain.py [--cases 1:unary 8:unary 1:unary-uip] [--rounds 20] [--out profiles/exp_explain.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, E, Q = 10, 3, 3


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


def _stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'calls': len(ms)}


def make_yardstick(lists, liked, table, props):
    """Returns fn() -> (evidence rows int64 [m, K, E] (-1 padded), property indices int64 [m, K, Q] or None)."""
    dev = table.device
    m, n_items = int(lists.shape[0]), int(table.shape[0])
    ptr, items = liked[0].to(torch.int64), liked[1].to(torch.int64)
    cnt = ptr[1:] - ptr[:-1]
    l_max = max(1, int(cnt.max()))
    pad = torch.full((m, l_max), -1, dtype=torch.int64, device=dev)               # the padded liked lists are an input, built once
    col = torch.arange(int(items.numel()), device=dev) - torch.repeat_interleave(ptr[:-1], cnt)
    pad[torch.repeat_interleave(torch.arange(m, device=dev), cnt), col] = items
    unit = torch.nn.functional.normalize(table, dim=1, eps=0.0).nan_to_num_(0.0)
    chunk = max(1, (1 << 28) // (l_max * int(table.shape[1])))
    member = weights = None
    if props is not None:
        pptr, pids, weights = props[0].to(torch.int64), props[1].to(torch.int64), props[2]
        n_props = int(weights.numel())
        member = torch.sparse_csr_tensor(pptr, pids, torch.ones(int(pids.numel()), device=dev), size=(n_items, n_props))
        member_t = member.to_dense().t().contiguous().to_sparse_csr()                # [|P|, |I|]
        own = member.to_dense() > 0                                                   # [|I|, |P|]
        chunk = min(chunk, max(1, (1 << 27) // (K * max(n_props, n_items))))
    l64 = lists.to(torch.int64)

    def run():
        ev_out, pr_out = [], []
        for lo in range(0, m, chunk):
            tg, lk = l64[lo:lo + chunk], pad[lo:lo + chunk]
            c = int(tg.shape[0])
            sim = torch.bmm(unit[tg.clamp(min=0)], unit[lk.clamp(min=0)].transpose(1, 2))           # [c, K, Lmax]
            dead = (lk < 0)[:, None, :] | (lk[:, None, :] == tg[:, :, None]) | (tg < 0)[:, :, None]
            top = torch.topk(sim.masked_fill(dead, float('-inf')), min(E, l_max), dim=2)
            ev = torch.gather(lk[:, None, :].expand(c, K, l_max), 2, top.indices)
            ev_out.append(torch.where(torch.isinf(top.values), torch.full_like(ev, -1), ev))
            if member is not None:
                pos = sim.clamp(min=0).masked_fill(dead, 0.0)
                dense = torch.zeros((c * K, n_items + 1), device=dev)
                hit = torch.zeros((c * K, n_items + 1), device=dev)
                idx = torch.where(lk < 0, torch.full_like(lk, n_items), lk)[:, None, :].expand(c, K, l_max).reshape(c * K, l_max)
                dense.scatter_(1, idx, pos.reshape(c * K, l_max))
                hit.scatter_(1, idx, (~dead).reshape(c * K, l_max).to(torch.float32))
                sums = torch.sparse.mm(member_t, dense[:, :n_items].t()).t()                        # [c K, |P|]
                sup = torch.sparse.mm(member_t, hit[:, :n_items].t()).t()
                keep = own[tg.clamp(min=0).reshape(-1)] & (sup > 0) & (tg.reshape(-1) >= 0)[:, None]
                best = torch.topk((sums * weights[None, :]).masked_fill(~keep, float('-inf')), Q, dim=1)
                pr_out.append(torch.where(torch.isinf(best.values), torch.full_like(best.indices, -1), best.indices).reshape(c, K, Q))
        return torch.cat(ev_out), (torch.cat(pr_out) if pr_out else None)
    return run


def run_case(scale, kind, args):
    from deep_cbrs_amar_renaissance_amd import engine, recommend as rec
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    d = helpers.ml1m_indexed(scale)
    nu, ni = len(d['users']), len(d['items'])
    adj = d['adj_uip'] if kind == 'unary-uip' else d['adj_ui']
    engine.set_seed(1)
    model = basic.BasicGCN(adj, embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
    train = _Train(d['train'], nu, ni, adj)
    with rec.device_lists():
        _, lists, _ = model.recommend(train, k=K)
    lists = lists.contiguous()
    table = rec._as_device_matrix(model._item_embeddings(train, 'graph'), lists.device, 'table')
    liked, props = rec._liked_device(train, nu, ni), rec._props_device(train, ni, 'idf')
    kernel = lambda: rec.explain_lists(lists, None, liked, table, props, E, Q, 'cosine')
    yard = make_yardstick(lists, liked, table, props)
    for fn in (kernel, yard):
        fn(), fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y_ev, y_pr = yard()
    torch.cuda.synchronize()
    y_peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    out = kernel()
    torch.cuda.synchronize()
    k_peak = torch.cuda.max_memory_allocated() - base
    t_kernel, t_yard = [], []
    for _ in range(args.rounds):
        t_kernel.append(_timed(kernel)[0])
        t_yard.append(_timed(yard)[0])
    same_ev = (out[0].to(torch.int64) == y_ev).all(dim=2).all(dim=1)
    line = {'case': 'BasicGCN graph space ml1m(s={}) {}'.format(scale, kind), 'lists': int(lists.shape[0]), 'items': ni,
            'width': int(table.shape[1]), 'k': K, 'n_evidence': E, 'n_properties': Q if props is not None else 0, 'metric': 'cosine',
            'liked_total': int(liked[1].numel()), 'liked_longest': int((liked[0][1:] - liked[0][:-1]).max()),
            'properties': int(props[2].numel()) if props is not None else 0, 'longest_property_row': int(props[3]) if props is not None else 0,
            'kernel': _stats(t_kernel), 'yardstick': _stats(t_yard), 'kernel_over_yardstick': float(np.median(t_kernel) / np.median(t_yard)),
            'kernel_workspace_bytes': 0, 'kernel_outputs_bytes': int(k_peak), 'yardstick_peak_workspace_bytes': int(y_peak),
            'evidence_lists_equal_to_yardstick': int(same_ev.sum())}
    if props is not None:
        line['property_lists_equal_to_yardstick'] = int((out[2].to(torch.int64) == y_pr).all(dim=2).all(dim=1).sum())
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['1:unary', '8:unary', '1:unary-uip'])
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_explain.py measures on the GPU: no device found")
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    torch.cuda.set_device(0)
    for case in args.cases:
        scale, kind = case.split(':')
        line = json.dumps(run_case(int(scale), kind, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

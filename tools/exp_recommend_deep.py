"""Cursor paging (recommend_after(), recommend_deep()) for BasicGCN with the default head at ml1m(s=1) and ml1m(s=8), every user,
training items excluded.  Four measurements on the towers of one call, alternating inside every repetition:

  (a) one page:   amar_recommend_after_f32 at k = 64 with second-page cursors (the last column of the first page) against
                  amar_recommend_f32 at k = 64 on the same users: the same pairs scored, one more compare per pair.
  (b) old way:    the same second page by merging page 1 into every user's exclusion CSR on the host (copy back, numpy merge, upload)
                  and calling amar_recommend_f32: the only way the library could produce it before.  Its output must EQUAL (a)'s
                  (item rows and score bits) before any time is recorded; the host merge is timed with it.
  (c) deep lists: deep_fused (ceil(k / 64) launches, the catalogue rescored per page) and deep_pairs (chunks scored once, one
                  amar_topk_segmented_after_f32 call per page) at k = 128, 256, 1024 against what a user would otherwise write:
                  pair-route scores of users x items in chunks, the exclusion mask and torch.topk(k).
  (d) regression: amar_recommend_f32 at k = 10 through this tree's library and, with --parent-lib, through a library built from the
                  parent commit, alternating: nothing that call runs was edited, so the two must sit within run-to-run spread.

A sample is the host clock around `inner` back-to-back calls that end in a device synchronise, divided by `inner`; reported are the
median over the repetitions and the spread (min, max).  One JSON line per scale goes to stdout and to --out.

Usage: python tools/exp_recommend_deep.py [--scales 1 8] [--reps 5] [--parent-lib PATH] [--out profiles/exp_recommend_deep.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEEP_KS = (128, 256, 1024)


class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def _sample(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def _stats(samples):
    return {'median_ms': float(np.median(samples)), 'min_ms': float(min(samples)), 'max_ms': float(max(samples)),
            'samples_ms': [round(x, 4) for x in samples]}


def _same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def run_scale(scale, model, train, reps, parent):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = len(train.users), len(train.items)
    towers = model.rs._recommend_split(*model._recommend_tables(train))
    plan = towers[2]
    blob, dims, acts = plan['rest']
    tu, ti = towers[0], towers[1]
    head = (tu, ti, blob, dims, acts, plan['in_act'])
    pair_towers = model.rs.towers(*model._recommend_tables(train))
    score_fn = lambda u, i: model.rs.score_towers(pair_towers, u, i)
    dev = tu.device
    excl = rec._exclusion_device(train, nu, ni, True)
    kw = dict(excl_ptr=excl[0], excl_items=excl[1])
    res = {'case': 'BasicGCN default head ml1m(s={})'.format(scale), 'scale': scale, 'users': nu, 'items': ni, 'rest_dims': list(dims),
           'route': capi.rank_route('recommend', dims), 'exclusion_entries': int(excl[1].numel())}

    # ---- (a) one page, (b) the old way --------------------------------------------------------------------------------------------
    p1_i, p1_s = capi.recommend(*head, 64, **kw)
    cur_i, cur_s = p1_i[:, -1].contiguous(), p1_s[:, -1].contiguous()
    e_ptr, e_items = excl[0].cpu().numpy().astype(np.int64), excl[1].cpu().numpy().astype(np.int64)
    e_user = np.repeat(np.arange(nu, dtype=np.int64), np.diff(e_ptr))

    def first_page():
        return capi.recommend(*head, 64, **kw)

    def after_page():
        return capi.recommend_after(*head, 64, cur_i, cur_s, **kw)

    def merge_on_host():
        shown = p1_i.cpu().numpy().astype(np.int64)                        # the page a front end has: copied back, merged, uploaded
        u, r = np.nonzero(shown >= 0)
        key = np.unique(np.concatenate([e_user * ni + e_items, u * ni + shown[u, r]]))
        ptr = np.zeros(nu + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // ni, minlength=nu), out=ptr[1:])
        return torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy((key % ni).astype(np.int32)).to(dev)

    def old_way():
        m_ptr, m_items = merge_on_host()
        return capi.recommend(*head, 64, excl_ptr=m_ptr, excl_items=m_items)

    res['after_equals_old_way'] = _same(after_page(), old_way())
    assert res['after_equals_old_way'], res['case']
    start = (torch.full((nu,), -1, dtype=torch.int32, device=dev), torch.full((nu,), float('inf'), dtype=torch.float32, device=dev))
    res['start_cursor_equals_recommend'] = _same(capi.recommend_after(*head, 64, *start, **kw), (p1_i, p1_s))
    assert res['start_cursor_equals_recommend'], res['case']
    a0, a1, b, h = [], [], [], []
    for _ in range(reps):                                                # alternating: drift hits all alike
        a0.append(_sample(first_page, 5))
        a1.append(_sample(after_page, 5))
        b.append(_sample(old_way, 1))
        h.append(_sample(merge_on_host, 1))
    res.update({'recommend_k64': _stats(a0), 'after_k64': _stats(a1), 'old_way_k64': _stats(b), 'old_way_host_merge': _stats(h)})
    res['after_over_recommend'] = res['after_k64']['median_ms'] / res['recommend_k64']['median_ms']
    res['old_way_over_after'] = res['old_way_k64']['median_ms'] / res['after_k64']['median_ms']

    # ---- (c) deep lists -------------------------------------------------------------------------------------------------------------
    chunk = max(1, rec.PAIRS_PER_CHUNK // ni)
    items32 = torch.arange(ni, dtype=torch.int32, device=dev)
    e_ptr64, e_items64 = excl[0].to(torch.int64), excl[1].to(torch.int64)

    def yardstick(k):
        out_i, out_s = [], []
        for lo in range(0, nu, chunk):
            hi = min(nu, lo + chunk)
            u = torch.arange(lo, hi, dtype=torch.int32, device=dev)
            s = score_fn(torch.repeat_interleave(u, ni), items32.repeat(hi - lo)).view(hi - lo, ni)
            rows = torch.repeat_interleave(torch.arange(hi - lo, device=dev), e_ptr64[lo + 1:hi + 1] - e_ptr64[lo:hi])
            s[rows, e_items64[int(e_ptr[lo]):int(e_ptr[hi])]] = float('-inf')
            sc, it = torch.topk(s, min(k, ni), dim=1)
            out_i.append(it)
            out_s.append(sc)
        return torch.cat(out_i), torch.cat(out_s)

    res['deep'] = {}
    with rec.device_lists():
        for k in DEEP_KS:
            fused = lambda: rec.deep_fused(towers, plan, train, k, None, True)
            paired = lambda: rec.deep_pairs(score_fn, train, k, None, True, device=dev)
            torch_way = lambda: yardstick(k)
            _, f_i, f_s = fused()
            _, p_i, p_s = paired()
            y_i, y_s = torch_way()
            fin = torch.isfinite(f_s) & torch.isfinite(y_s)
            entry = {'pages': len(rec.page_sizes(k)),
                     'fused_rows_equal_to_torch': float(((f_i == y_i) | ~fin).all(1).float().mean()),
                     'pairs_rows_equal_to_torch': float(((p_i == y_i) | ~fin).all(1).float().mean()),
                     'max_score_diff_fused_to_torch': float((f_s - y_s)[fin].abs().max()) if bool(fin.any()) else 0.0}
            f, p, y = [], [], []
            for _ in range(reps):
                f.append(_sample(fused, 1))
                p.append(_sample(paired, 1))
                y.append(_sample(torch_way, 1))
            entry.update({'deep_fused': _stats(f), 'deep_pairs': _stats(p), 'torch_topk': _stats(y)})
            entry['fused_over_torch'] = entry['deep_fused']['median_ms'] / entry['torch_topk']['median_ms']
            entry['pairs_over_torch'] = entry['deep_pairs']['median_ms'] / entry['torch_topk']['median_ms']
            res['deep'][str(k)] = entry

    # ---- (d) amar_recommend_f32 at k = 10: this tree's library and the parent commit's ------------------------------------------------
    slices, out_i, out_s, ws_i, ws_s = capi._sliced_topk('amar_recommend_slices', (nu, ni, (ctypes.c_int32 * len(dims))(*dims), len(acts)), 0, nu, 10, dev)
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    acts_c = (ctypes.c_int32 * len(acts))(*[capi.ACT_CODES[a] for a in acts])
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def raw(lib):
        code = lib.amar_recommend_f32(p(tu), int(tu.stride(0)), nu, p(ti), int(ti.stride(0)), ni, int(tu.shape[1]), p(blob), dims_c, acts_c, len(acts),
                                      capi.ACT_CODES[plan['in_act']], None, nu, p(excl[0]), p(excl[1]), 10, int(slices) if slices > 1 else 1,
                                      p(ws_i), p(ws_s), p(out_i), p(out_s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0, code

    this = capi.load()
    raw(this)
    torch.cuda.synchronize()
    mine = (out_i.clone(), out_s.clone())
    t, q = [], []
    if parent is not None:
        raw(parent)
        torch.cuda.synchronize()
        res['parent_equal'] = _same(mine, (out_i, out_s))
    for _ in range(reps):
        t.append(_sample(lambda: raw(this), 10))
        if parent is not None:
            q.append(_sample(lambda: raw(parent), 10))
    res['recommend_k10_this'] = _stats(t)
    if parent is not None:
        res['recommend_k10_parent'] = _stats(q)
        res['this_over_parent'] = res['recommend_k10_this']['median_ms'] / res['recommend_k10_parent']['median_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help="libamar_hip.so built from the parent commit, for measurement (d)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_recommend_deep.jsonl'))
    args = ap.parse_args()
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    capi.load()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.amar_recommend_f32.restype, parent.amar_recommend_f32.argtypes = capi.SIGNATURES['amar_recommend_f32']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        for s in args.scales:
            d = helpers.ml1m_indexed(s)
            nu, ni = len(d['users']), len(d['items'])
            engine.set_seed(1)
            model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
            helpers.spread_scores(model)
            train = _Train(d['train'], nu, ni)
            line = json.dumps(run_scale(s, model, train, args.reps, parent))
            print(line, flush=True)
            out.write(line + '\n')
            out.flush()
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

"""Recommendation from per-user candidate lists (recommend_from(), k = 10, every user, training items excluded) for BasicGCN with the
default head at ml1m(s=1) and ml1m(s=8): every user gets its own random list of 100 or of 1 000 items, drawn at a fixed seed.
Timed, alternating inside every repetition:

  lists:      the new launch alone, amar_recommend_lists_f32 over the CSR of the lists already on the device (sum |C_u| pairs);
  from_call:  the whole model.recommend_from() call on a device tensor [m, P] (propagation, towers, the device sort / compaction,
              the launch, the copy back) and on host lists (the host normalisation and the upload instead);
  (a) pairs:  the whole model.recommend_among(candidates=[one list per user]) call, which is the pair route — the only way the
              library could serve per-user lists before: a dense bool [chunk, |I|] mask, nonzero(), the pair list scored into
              memory, amar_topk_segmented_f32.  Its lists must equal the new ones, its scores within 2e-6 (another score routine);
  (b) complement: amar_recommend_f32 with the complement of every user's list merged into its exclusion row, where that CSR
              stays below 2^30 entries (else skipped).  Its output must EQUAL the new launch's (item rows and score bits).

Peak device workspace of the launch, of (a) and of (b) is recorded.  With --parent-lib (a libamar_hip.so built from the parent
commit) amar_recommend_f32 at k = 10 is also run through both libraries on the same towers: equal bits, both times.

A sample is the host clock around `inner` back-to-back calls that end in a device synchronise, divided by `inner`; reported are the
median over the repetitions and the spread (min, max).  One JSON line per case goes to stdout and to --out.

Usage: python tools/exp_recommend_from.py [--scales 1 8] [--lengths 100 1000] [--reps 5] [--parent-lib PATH]
                                          [--out profiles/exp_recommend_from.jsonl]
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

K = 10
CSR_LIMIT = 1 << 30      # entries of an exclusion CSR: the selector's binary search adds two int32 positions (lo + hi)


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


def _peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def merged_exclusions(excl, kept, nu, ni, dev, chunk=1024):
    """The exclusion CSR with every item outside user u's list (kept: bool [nu, ni] by chunks, a callable lo, hi -> mask) added to
    row u, built on the device in chunks of users: (ptr int32 [nu + 1], items int32)."""
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    counts, cols = [], []
    for lo in range(0, nu, chunk):
        uc = torch.arange(lo, min(nu, lo + chunk), device=dev)
        banned = ~rec._unseen_mask(uc, ni, excl, dev) | ~kept(lo, min(nu, lo + chunk))
        counts.append(banned.sum(1))
        cols.append(banned.nonzero(as_tuple=True)[1].to(torch.int32))
    ptr = torch.zeros(nu + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.cat(counts), 0, out=ptr[1:])
    assert int(ptr[-1]) < CSR_LIMIT
    return ptr.to(torch.int32), torch.cat(cols)


def parent_recommend(lib, tu, ti, blob, dims, acts, in_act, k, excl):
    """amar_recommend_f32 through another build of the library (one slice count for both: the automatic one of this tree)."""
    from deep_cbrs_amar_renaissance_amd import capi
    sig = capi.SIGNATURES['amar_recommend_f32']
    lib.amar_recommend_f32.restype, lib.amar_recommend_f32.argtypes = sig
    lib.amar_recommend_slices.restype, lib.amar_recommend_slices.argtypes = capi.SIGNATURES['amar_recommend_slices']
    nu, ni, c1 = tu.shape[0], ti.shape[0], tu.shape[1]
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    acts_c = (ctypes.c_int32 * len(acts))(*[capi.ACT_CODES[a] for a in acts])
    slices = int(lib.amar_recommend_slices(nu, ni, dims_c, len(acts), 0))
    out_i = torch.empty((nu, k), dtype=torch.int32, device=tu.device)
    out_s = torch.empty((nu, k), dtype=torch.float32, device=tu.device)
    ws_i = torch.empty((nu * slices * k,), dtype=torch.int32, device=tu.device)
    ws_s = torch.empty((nu * slices * k,), dtype=torch.float32, device=tu.device)

    def call():
        rc = lib.amar_recommend_f32(tu.data_ptr(), tu.stride(0), nu, ti.data_ptr(), ti.stride(0), ni, c1, blob.data_ptr(), dims_c, acts_c,
                                    len(acts), capi.ACT_CODES[in_act], None, nu, excl[0].data_ptr(), excl[1].data_ptr(), k, slices,
                                    ws_i.data_ptr(), ws_s.data_ptr(), out_i.data_ptr(), out_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out_i, out_s
    return call


def run_case(scale, length, model, train, reps, seed, parent):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = len(train.users), len(train.items)
    length = min(length, ni)
    towers = model.rs._recommend_split(*model._recommend_tables(train), kind='lists')
    plan = towers[2]
    blob, dims, acts = plan['rest']
    tu, ti = towers[0], towers[1]
    dev = tu.device
    excl = rec._exclusion_device(train, nu, ni, True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    rows = torch.rand((nu, ni), device=dev, generator=gen).argsort(dim=1)[:, :length]           # a uniform sample per user
    padded = (rows + nu).contiguous()                                                        # node ids [nu, P], any order
    ptr, items = rec.device_candidate_csr(padded, nu, ni)
    torch.cuda.synchronize()
    host_lists = padded.cpu().numpy()

    def lists():
        return capi.recommend_lists(tu, ti, blob, dims, acts, plan['in_act'], K, ptr, items, excl_ptr=excl[0], excl_items=excl[1])

    res = {'case': 'BasicGCN default head ml1m(s={}) lists of {}'.format(scale, length), 'scale': scale, 'users': nu, 'items': ni,
           'list_length': length, 'pairs_lists': int(ptr[-1]), 'pairs_catalogue': nu * ni, 'k': K, 'rest_dims': list(dims),
           'lists_route': capi.rank_route('lists', dims), 'exclusion_entries': int(excl[1].numel())}
    li, ls = lists()
    torch.cuda.synchronize()
    # (a) the pair route: the same items, scores of another routine
    per_user = [host_lists[u] for u in range(nu)]
    pa = model.recommend_among(train, per_user, k=K)
    new = model.recommend_from(train, padded, k=K)
    both = np.isfinite(pa[2]) & np.isfinite(new[2])
    res['rows_equal_to_pairs'] = float(((pa[1] == new[1]) | ~both).all(1).mean())
    res['max_score_diff_to_pairs'] = float(np.abs(pa[2] - new[2])[both].max()) if both.any() else 0.0
    assert np.array_equal(new[1], np.where(li.cpu().numpy() >= 0, li.cpu().numpy() + nu, -1))
    res['lists_peak_workspace_mb'] = _peak_mb(lists)
    res['pairs_peak_workspace_mb'] = _peak_mb(lambda: model.recommend_among(train, per_user, k=K))
    # (b) the complement in the exclusion CSR
    complement = None
    if int(excl[1].numel()) + nu * (ni - length) < CSR_LIMIT:
        def kept(lo, hi):
            mask = torch.zeros((hi - lo, ni), dtype=torch.bool, device=dev)
            mask.scatter_(1, rows[lo:hi], True)
            return mask
        m_ptr, m_items = merged_exclusions(excl, kept, nu, ni, dev)

        def complement():
            return capi.recommend(tu, ti, blob, dims, acts, plan['in_act'], K, excl_ptr=m_ptr, excl_items=m_items)
        ci, cs = complement()
        torch.cuda.synchronize()
        res['equal_to_complement'] = bool(torch.equal(li, ci) and torch.equal(ls.view(torch.int32), cs.view(torch.int32)))
        assert res['equal_to_complement'], res['case']
        res['complement_csr_mb'] = (m_ptr.numel() + m_items.numel()) * 4 / 2.0 ** 20
        res['complement_peak_workspace_mb'] = _peak_mb(complement)
    a, b, c, d, e = [], [], [], [], []
    for _ in range(reps):                                                # alternating: drift hits all alike
        a.append(_sample(lists, 10))
        if complement is not None:
            b.append(_sample(complement, 5))
        c.append(_sample(lambda: model.recommend_from(train, padded, k=K), 1))
        d.append(_sample(lambda: model.recommend_from(train, host_lists, k=K), 1))
        e.append(_sample(lambda: model.recommend_among(train, per_user, k=K), 1))
    res.update({'lists': _stats(a), 'from_call_device_lists': _stats(c), 'from_call_host_lists': _stats(d), 'pairs_call': _stats(e)})
    res['pairs_call_over_from_call'] = res['pairs_call']['median_ms'] / res['from_call_device_lists']['median_ms']
    if complement is not None:
        res['complement'] = _stats(b)
        res['complement_over_lists'] = res['complement']['median_ms'] / res['lists']['median_ms']
    if parent is not None:
        here = lambda: capi.recommend(tu, ti, blob, dims, acts, plan['in_act'], K, excl_ptr=excl[0], excl_items=excl[1])
        there = parent_recommend(parent, tu, ti, blob, dims, acts, plan['in_act'], K, excl)
        hi_, hs = here()
        ti_, ts = there()
        torch.cuda.synchronize()
        res['recommend_equal_to_parent'] = bool(torch.equal(hi_, ti_) and torch.equal(hs.view(torch.int32), ts.view(torch.int32)))
        assert res['recommend_equal_to_parent']
        h, t = [], []
        for _ in range(reps):
            h.append(_sample(here, 5))
            t.append(_sample(there, 5))
        res.update({'recommend_this_tree': _stats(h), 'recommend_parent_library': _stats(t)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--lengths', type=int, nargs='+', default=[100, 1000])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_recommend_from.jsonl'))
    args = ap.parse_args()
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    capi.load()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        for s in args.scales:
            d = helpers.ml1m_indexed(s)
            nu, ni = len(d['users']), len(d['items'])
            engine.set_seed(1)
            model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
            helpers.spread_scores(model)
            train = _Train(d['train'], nu, ni)
            for length in args.lengths:
                line = json.dumps(run_case(s, length, model, train, args.reps, 1000 * s + length, parent))
                print(line, flush=True)
                out.write(line + '\n')
                out.flush()
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

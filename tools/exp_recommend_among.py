"""Recommendation among candidates (recommend_among(), k = 10, every user, training items excluded) for BasicGCN with the default
head at ml1m(s=1) and ml1m(s=8): candidate sets of 100 %, 10 % and 1 % of the catalogue, drawn at a fixed seed.  Three things are
timed on the towers of one call, the launch alone, alternating inside every repetition:

  (a) among:      the new call, one amar_recommend_among_f32 launch (two with slices) over |U| x |C| pairs;
  (b) complement: amar_recommend_f32 over the same users with the complement of the candidates merged into every user's exclusion
                  CSR — the only way the library could produce these lists before; |U| x |I| pairs scored, |U| x (|I| - |C|) more
                  CSR entries held.  Its output must EQUAL (a)'s (item rows and score bits) before any time is recorded.  The
                  selector's binary search takes CSR positions below 2^30, so a case whose merged CSR would pass that lists the
                  first m users it has room for (`listed_users`), in (a), (b) and (c) alike;
  (c) torch:      what a user would otherwise write — pair-route scores of users x candidates in chunks (the pair stage's kernel
                  over explicit pair lists), the exclusion mask and torch.topk — with its peak workspace.

A sample is the host clock around `inner` back-to-back calls that end in a device synchronise, divided by `inner`; reported are the
median over the repetitions and the spread (min, max).  One JSON line per case goes to stdout and to --out.

Usage: python tools/exp_recommend_among.py [--scales 1 8] [--shares 1.0 0.1 0.01] [--reps 5] [--out profiles/exp_recommend_among.jsonl]
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


CSR_LIMIT = 1 << 30      # entries of an exclusion CSR: the selector's binary search adds two int32 positions (lo + hi)


def merged_exclusions(excl, keep_row, nu, ni, dev, m, chunk=1024):
    """The exclusion CSR with every item outside the candidates added to the rows of the first m users (the listed ones; the other
    rows stay as they are), built on the device in chunks of users: (ptr int32 [nu + 1], items int32)."""
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    counts, cols = [], []
    for lo in range(0, nu, chunk):
        uc = torch.arange(lo, min(nu, lo + chunk), device=dev)
        unseen = rec._unseen_mask(uc, ni, excl, dev)
        banned = ~unseen
        banned[:max(0, min(m - lo, len(uc)))] |= ~keep_row[None, :]
        counts.append(banned.sum(1))
        cols.append(banned.nonzero(as_tuple=True)[1].to(torch.int32))
    ptr = torch.zeros(nu + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.cat(counts), 0, out=ptr[1:])
    assert int(ptr[-1]) < CSR_LIMIT
    return ptr.to(torch.int32), torch.cat(cols)


def run_case(scale, share, model, train, reps, seed):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = len(train.users), len(train.items)
    rng = np.random.default_rng(seed)
    n_cand = ni if share >= 1.0 else max(1, int(round(share * ni)))
    cand = np.sort(rng.choice(ni, size=n_cand, replace=False)).astype(np.int64)
    towers = model.rs._recommend_split(*model._recommend_tables(train))
    plan = towers[2]
    blob, dims, acts = plan['rest']
    tu, ti = towers[0], towers[1]
    pair_towers = model.rs.towers(*model._recommend_tables(train))
    dev = tu.device
    excl = rec._exclusion_device(train, nu, ni, True)
    keep_row = torch.zeros(ni, dtype=torch.bool, device=dev)
    cand_d = torch.from_numpy(cand).to(dev)
    keep_row[cand_d] = True
    # (b) needs |I| - |C| more CSR entries per listed user; where all users would pass CSR_LIMIT the case lists the first m users, in
    # all three measurements alike
    m = nu if n_cand == ni else min(nu, (CSR_LIMIT - 1 - int(excl[1].numel())) // (ni - n_cand))
    u_dev = None if m == nu else torch.arange(m, dtype=torch.int32, device=dev)
    m_ptr, m_items = merged_exclusions(excl, keep_row, nu, ni, dev, m)
    cand32 = cand.astype(np.int32)

    def among():
        return capi.recommend_among(tu, ti, blob, dims, acts, plan['in_act'], K, cand32, users=u_dev, excl_ptr=excl[0], excl_items=excl[1])

    def complement():
        return capi.recommend(tu, ti, blob, dims, acts, plan['in_act'], K, users=u_dev, excl_ptr=m_ptr, excl_items=m_items)

    chunk = max(1, rec.PAIRS_PER_CHUNK // n_cand)                         # users per chunk of the torch yardstick
    pos = torch.full((ni,), -1, dtype=torch.int64, device=dev)            # item row -> candidate position
    pos[cand_d] = torch.arange(n_cand, device=dev)
    cand_i32 = cand_d.to(torch.int32)
    e_ptr64, e_items64 = excl[0].to(torch.int64), excl[1].to(torch.int64)
    e_ptr_host = e_ptr64.cpu().numpy()
    kk = min(K, n_cand)

    def yardstick():
        out_i, out_s = [], []
        for lo in range(0, m, chunk):
            hi = min(m, lo + chunk)
            u = torch.arange(lo, hi, dtype=torch.int32, device=dev)
            s = model.rs.score_towers(pair_towers, torch.repeat_interleave(u, n_cand), cand_i32.repeat(hi - lo)).view(hi - lo, n_cand)
            e0, e1 = int(e_ptr_host[lo]), int(e_ptr_host[hi])
            rows = torch.repeat_interleave(torch.arange(hi - lo, device=dev), e_ptr64[lo + 1:hi + 1] - e_ptr64[lo:hi])
            at = pos[e_items64[e0:e1]]
            s[rows[at >= 0], at[at >= 0]] = float('-inf')
            sc, it = torch.topk(s, kk, dim=1)
            out_i.append(cand_d[it])
            out_s.append(sc)
        return torch.cat(out_i), torch.cat(out_s)

    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    lib = capi.load()
    res = {'case': 'BasicGCN default head ml1m(s={}) candidates {:g} %'.format(scale, 100 * share), 'scale': scale, 'users': nu, 'items': ni,
           'share': share, 'candidates': n_cand, 'listed_users': m, 'pairs_among': m * n_cand, 'pairs_complement': m * ni, 'k': K, 'rest_dims': list(dims),
           'among_route': capi.rank_route('among', dims), 'among_slices': int(lib.amar_recommend_slices(m, n_cand, dims_c, len(dims) - 1, 0)),
           'complement_slices': int(lib.amar_recommend_slices(m, ni, dims_c, len(dims) - 1, 0)),
           'exclusion_entries': int(excl[1].numel()), 'complement_exclusion_entries': int(m_items.numel()),
           'yardstick_users_per_chunk': chunk}
    # the lists must be the same before any time is recorded
    ai, as_ = among()
    ci, cs = complement()
    torch.cuda.synchronize()
    res['equal_to_complement'] = bool(torch.equal(ai, ci) and torch.equal(as_.view(torch.int32), cs.view(torch.int32)))
    assert res['equal_to_complement'], res['case']
    yi, ys = yardstick()
    ai_h, as_h, yi_h, ys_h = ai.cpu().numpy()[:, :kk], as_.cpu().numpy()[:, :kk], yi.cpu().numpy(), ys.cpu().numpy()
    both = np.isfinite(as_h) & np.isfinite(ys_h)
    res['rows_equal_to_torch'] = float(((ai_h == yi_h) | ~both).all(1).mean())
    res['max_score_diff_to_torch'] = float(np.abs(as_h - ys_h)[both].max()) if both.any() else 0.0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yardstick()
    torch.cuda.synchronize()
    res['yardstick_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    torch.cuda.reset_peak_memory_stats()
    among()
    torch.cuda.synchronize()
    res['among_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    torch.cuda.reset_peak_memory_stats()
    complement()
    torch.cuda.synchronize()
    res['complement_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    res['complement_csr_mb'] = (m_ptr.numel() + m_items.numel()) * 4 / 2.0 ** 20
    a, b, c = [], [], []
    for _ in range(reps):                                                # alternating: drift hits all three alike
        a.append(_sample(among, 10))
        b.append(_sample(complement, 5))
        c.append(_sample(yardstick, 2))
    res.update({'among': _stats(a), 'complement': _stats(b), 'torch': _stats(c)})
    res['complement_over_among'] = res['complement']['median_ms'] / res['among']['median_ms']
    res['torch_over_among'] = res['torch']['median_ms'] / res['among']['median_ms']
    full = [_sample(lambda: model.recommend_among(train, cand + nu, k=K, users=None if m == nu else np.arange(m)), 1) for _ in range(3)]
    res['recommend_among_call_ms'] = _stats(full)                        # propagation, towers, the candidate upload and the copy back included
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--shares', type=float, nargs='+', default=[1.0, 0.1, 0.01])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_recommend_among.jsonl'))
    args = ap.parse_args()
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    capi.load()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        for s in args.scales:
            d = helpers.ml1m_indexed(s)
            nu, ni = len(d['users']), len(d['items'])
            engine.set_seed(1)
            model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
            helpers.spread_scores(model)
            train = _Train(d['train'], nu, ni)
            for share in args.shares:
                line = json.dumps(run_case(s, share, model, train, args.reps, 1000 * s + int(round(1000 * share))))
                print(line, flush=True)
                out.write(line + '\n')
                out.flush()
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

"""Group recommendation (recommend_group(), k = 10, the members' training items excluded) for BasicGCN with the default head at
ml1m(s=1) and ml1m(s=8): random groups of 2, 4 and 8 distinct users, count = |U| / size, so that every case scores about |U| x |I|
pairs.  Three things are timed on the towers of one call, alternating inside every repetition:

  (a) group:   the new call, one amar_recommend_group_f32 launch (two with item slices);
  (b) members: amar_recommend_f32 over the same member rows at the same k — the same scoring work with a selection per member
               instead of one per group: the floor the score stage sets;
  (c) torch:   what a user would otherwise write — pair-route scores of members x |I| in chunks of groups (the pair stage's kernel
               over explicit pair lists), a torch sum over the members, the exclusion mask and torch.topk — with its peak workspace.

A sample is the host clock around `inner` back-to-back calls that end in a device synchronise, divided by `inner`; reported are the
median over the repetitions and the spread (min, max).  (a) is also checked against (c) (same items; scores within 1e-6: torch sums
in another order).  One JSON line per case goes to stdout and to --out.

Usage: python tools/exp_group_recommend.py [--scales 1 8] [--sizes 2 4 8] [--reps 7] [--out profiles/exp_group_recommend.jsonl]
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


def run_case(scale, size, model, train, reps, seed):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = len(train.users), len(train.items)
    count = nu // size
    rng = np.random.default_rng(seed)
    groups = [rng.choice(nu, size=size, replace=False) for _ in range(count)]
    ptr, members = rec.group_csr(groups, nu)
    eptr, eitems = rec.group_exclusion_csr(train.ratings, ptr, members, nu, ni)
    towers = model.rs._recommend_split(*model._recommend_tables(train))
    plan = towers[2]
    blob, dims, acts = plan['rest']
    tu, ti = towers[0], towers[1]
    pair_towers = model.rs.towers(*model._recommend_tables(train))       # the pair route's towers (split form where the head has one)
    dev = tu.device
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    ptr_d, mem_d, eptr_d, eitems_d = i32(ptr), i32(members), i32(eptr), i32(eitems)
    excl = rec._exclusion_device(train, nu, ni, True)

    def group():
        return capi.recommend_group(tu, ti, blob, dims, acts, plan['in_act'], K, ptr_d, mem_d, strategy='mean', excl_ptr=eptr_d,
                                    excl_items=eitems_d)

    def per_member():
        return capi.recommend(tu, ti, blob, dims, acts, plan['in_act'], K, users=mem_d, excl_ptr=excl[0], excl_items=excl[1])

    chunk = max(1, rec.PAIRS_PER_CHUNK // (ni * size))                   # groups per chunk of the torch yardstick
    all_items = torch.arange(ni, dtype=torch.int32, device=dev)
    eptr64 = torch.from_numpy(eptr).to(dev)
    eitems64 = torch.from_numpy(eitems).to(dev)
    mem2d = mem_d.view(count, size)

    def yardstick():
        out_i, out_s = [], []
        for lo in range(0, count, chunk):
            hi = min(count, lo + chunk)
            u = mem2d[lo:hi].reshape(-1)
            s = model.rs.score_towers(pair_towers, torch.repeat_interleave(u, ni), all_items.repeat(u.numel())).view(hi - lo, size, ni)
            agg = s.sum(1) / float(size)
            e0, e1 = int(eptr[lo]), int(eptr[hi])
            rows = torch.repeat_interleave(torch.arange(hi - lo, device=dev), eptr64[lo + 1:hi + 1] - eptr64[lo:hi])
            agg[rows, eitems64[e0:e1]] = float('-inf')
            sc, it = torch.topk(agg, K, dim=1)
            out_i.append(it)
            out_s.append(sc)
        return torch.cat(out_i), torch.cat(out_s)

    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    lib = capi.load()
    res = {'case': 'BasicGCN default head ml1m(s={}) groups of {}'.format(scale, size), 'scale': scale, 'users': nu, 'items': ni,
           'group_size': size, 'groups': count, 'members': int(members.size), 'pairs': int(members.size) * ni, 'k': K, 'strategy': 'mean',
           'rest_dims': list(dims), 'group_slices': int(lib.amar_recommend_group_slices(count, int(members.size), ni, dims_c, len(dims) - 1, 0)),
           'member_slices': int(lib.amar_recommend_slices(int(members.size), ni, dims_c, len(dims) - 1, 0)),
           'yardstick_groups_per_chunk': chunk}
    for fn in (group, per_member, yardstick):                            # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yardstick()
    torch.cuda.synchronize()
    res['yardstick_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    torch.cuda.reset_peak_memory_stats()
    group()
    torch.cuda.synchronize()
    res['group_peak_workspace_mb'] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    a, b, c = [], [], []
    for _ in range(reps):                                                # alternating: drift hits all three alike
        a.append(_sample(group, 20))
        b.append(_sample(per_member, 20))
        c.append(_sample(yardstick, 2))
    res.update({'group': _stats(a), 'members': _stats(b), 'torch': _stats(c)})
    res['group_over_members'] = res['group']['median_ms'] / res['members']['median_ms']
    res['torch_over_group'] = res['torch']['median_ms'] / res['group']['median_ms']
    full = [_sample(lambda: model.recommend_group(train, groups, k=K), 1) for _ in range(3)]
    res['recommend_group_call_ms'] = _stats(full)                       # propagation, towers, host CSRs and the copy back included
    gi, gs = group()
    yi, ys = yardstick()
    gi, gs, yi, ys = gi.cpu().numpy(), gs.cpu().numpy(), yi.cpu().numpy(), ys.cpu().numpy()
    res['rows_equal_to_torch'] = float((gi == yi).all(1).mean())
    res['max_score_diff_to_torch'] = float(np.abs(gs - ys)[np.isfinite(gs) & np.isfinite(ys)].max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 4, 8])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_group_recommend.jsonl'))
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
            for size in args.sizes:
                line = json.dumps(run_case(s, size, model, train, args.reps, 100 * s + size))
                print(line, flush=True)
                out.write(line + '\n')
                out.flush()
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

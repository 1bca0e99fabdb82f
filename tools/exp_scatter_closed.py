#!/usr/bin/env python
"""The two launches of the pair stage on bench.py's workload, by window size of the plan and by form of the second launch
(amar_scatter_f32: one store per score; amar_scatter_closed_f32: windows finished in LDS — one workgroup per window up to 32 Ki
scores, two per window above).  Both launches are timed inside the same sequence, as they run in a step; the figure to compare is
their SUM.  python tools/exp_scatter_closed.py [scale] [window,window,...]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.models import basic
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    windows = [int(w) for w in sys.argv[2].split(',')] if len(sys.argv) > 2 else [65536, 32768, 16384]
    capi.load()
    dev = torch.device('cuda')
    data = synthetic.ml1m_device(scale, device=dev)
    nu = data['n_users']
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    perm = torch.randperm(data['test'].shape[0], device=dev, generator=g)
    u = data['test'][perm, 0].to(torch.int32).contiguous()
    i = data['test'][perm, 1].to(torch.int32).contiguous()
    engine.set_seed(1)
    rs = basic.BasicRS([24, 24], [48, 48])
    rs.build_head(24, 24)
    emb = torch.randn((nu + data['n_items'], 24), device=dev, generator=g)
    tw = rs.towers(emb[:nu], emb[nu:])
    os.environ.pop('AMAR_PAIR_SCATTER', None)
    direct = rs.score_towers(tw, u, i, 0, nu)
    print('ml1m(s=%d): %d pairs' % (scale, u.numel()), flush=True)
    raw_chain, raw_scatter = capi.chain, capi.scatter
    for window in windows:
        plan = basic.PairPlan(u, i, window=window)
        if plan.mid_index is None:
            print('window %d: the list is too short for the two-step way back' % window, flush=True)
            continue
        for form in ('global', 'lds'):
            os.environ['AMAR_PAIR_SCATTER'] = form
            route = capi.scatter_route(u.numel(), 1, plan.max_window, True)
            if route != form:
                print('window %7d  %-6s: not taken (route %s)' % (window, form, route), flush=True)
                continue
            marks = []

            def timed(raw):
                def call(*a, **k):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    raw(*a, **k)
                    e1.record()
                    marks.append((e0, e1))
                return call
            capi.chain, capi.scatter = timed(raw_chain), timed(raw_scatter)
            try:
                for _ in range(5):
                    got = rs.score_towers(tw, u, i, 0, nu, pair_plan=plan)
                torch.cuda.synchronize()
                del marks[:]
                for _ in range(40):
                    rs.score_towers(tw, u, i, 0, nu, pair_plan=plan)
                torch.cuda.synchronize()
            finally:
                capi.chain, capi.scatter = raw_chain, raw_scatter
            med = lambda xs: sorted(xs)[len(xs) // 2]
            pair = med([e0.elapsed_time(e1) for e0, e1 in marks[0::2]])
            back = med([e0.elapsed_time(e1) for e0, e1 in marks[1::2]])
            both = med([marks[k][0].elapsed_time(marks[k + 1][1]) for k in range(0, len(marks), 2)])
            print('window %7d (%4d windows)  %-6s: pair launch %.4f ms + second launch %.4f ms = %.4f (first start to second end %.4f); '
                  'same bits as the direct call: %s' % (window, plan.n_windows, form, pair, back, pair + back, both, torch.equal(got, direct)), flush=True)
    os.environ.pop('AMAR_PAIR_SCATTER', None)


if __name__ == '__main__':
    main()

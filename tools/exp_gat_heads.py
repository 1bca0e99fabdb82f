#!/usr/bin/env python
"""Multi-head GAT: the fused row kernels (amar_gat_heads_f32 / amar_gat_heads_bwd_f32) against the composition a user could write
without them — `heads` launches of amar_gat_layer_f32 / amar_gat_bwd_f32 on the heads' column slices, their scalars precomputed —
on the ML-1M-shape synthetic user-item graph (development aid for DESIGN.md §7g).

Per (heads, channels) and per direction: REPEATS windows of each side, alternating, every window timed with device events around
ITERS calls after a warm-up; the file keeps every window's ms per call, so the run-to-run spread of both sides is on record, and
the largest relative difference between the two sides' results at the timed size.
Both sides are timed as bare C-ABI launches on buffers allocated beforehand (no allocation, no wrapper checks inside a window); the
script exits non-zero if the fused form is not faster outside the spread anywhere.
`python tools/exp_gat_heads.py [--out profiles/exp_gat_heads.jsonl] [--scale 1 8]`."""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

SHAPES = [(4, 8), (8, 8), (4, 16)]
REPEATS = 7


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(fused, composed, iters):
    for fn in (fused, composed):                                     # warm-up: code objects, the allocator's blocks
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {'fused': [], 'composed': []}
    for _ in range(REPEATS):                                         # alternating: both sides see the same neighbours on the machine
        times['fused'].append(window(fused, iters))
        times['composed'].append(window(composed, iters))
    return {k: {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'windows': [round(t, 5) for t in v]}
            for k, v in times.items()}


def rel_diff(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def train_batches(scale, g, batch=4096, iters=20):
    """One whole replayed training batch (forward, reverse with the attention-vector gradients, one optimizer launch) of a two-layer
    BasicGAT with one head and with four heads, concatenated and averaged: ms per batch, every window kept.  On record only."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    u, i, y = g['train'][:batch, 0], g['train'][:batch, 1], g['train'][:batch, 2]
    out = []
    for heads, concat in ((1, True), (4, True), (4, False)):
        engine.set_seed(1)
        model = basic.BasicGAT(g['adj_ui'], attn_heads=heads, concat_heads=concat, embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24],
                               clf_units=[48, 48], l2_regularizer=1e-4)
        trainer = training.Trainer(model)
        step = lambda: trainer.train_batch_graphed(u, i, y)          # noqa: E731  (eager once, captured once, then replayed)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        v = [window(step, iters) for _ in range(REPEATS)]
        line = {'graph': 'ml1m(s={}) user-item'.format(scale), 'op': 'replayed training batch', 'model': 'BasicGAT 8-8-8', 'batch': batch,
                'heads': heads, 'channels': 8, 'concat_heads': concat, 'replayed': trainer._g is not None, 'iters_per_window': iters,
                'ms_per_batch': {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'windows': [round(t, 5) for t in v]}}
        print(json.dumps(line), flush=True)
        out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_gat_heads.jsonl'))
    ap.add_argument('--scale', type=int, nargs='+', default=[1, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_gat_heads.py measures on the GPU; none found")
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd.utilities.math import convert_to_tensor
    from tests import helpers
    lib = capi.load()
    dev = torch.device('cuda')
    stream = torch.cuda.current_stream().cuda_stream
    T = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(dev)   # noqa: E731
    E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)                  # noqa: E731
    P = lambda t: t.data_ptr()                                                              # noqa: E731
    lines = []
    for scale in args.scale:
        g = helpers.ml1m_indexed(scale)
        a = convert_to_tensor(g['adj_ui'], with_values=False, drop_diagonal=True)
        n, nnz = int(a.shape[0]), int(a.colidx.numel())
        rp, ci = P(a.rowptr), P(a.colidx)
        rng = np.random.default_rng(0)
        for heads, c in SHAPES:
            hc = heads * c
            x, w = T(rng.standard_normal((n, 8))), T(rng.uniform(-0.6, 0.6, (8, heads, c)))
            a_s, a_n, b = T(rng.uniform(-1, 1, (c, heads, 1))), T(rng.uniform(-1, 1, (c, heads, 1))), T(rng.uniform(-0.1, 0.1, hc))
            hd, s = E(n, hc), E(n, 2 * heads)
            capi.rowwise_xw_heads(x, w, hd, a_s, a_n, s)
            # Both sides call the C-ABI directly on buffers allocated here, outside the timed windows: a window holds launches only.
            # The composition's operands per head: contiguous scalars and attention vectors, its own outputs and scratch.
            s_h = [s[:, h].contiguous() for h in range(heads)]
            t_h = [s[:, heads + h].contiguous() for h in range(heads)]
            as_h = [a_s[:, h, 0].contiguous() for h in range(heads)]
            an_h = [a_n[:, h, 0].contiguous() for h in range(heads)]
            y_f, y_c, dy = E(n, hc), E(n, hc), T(rng.standard_normal((n, hc)))
            dout_f, scr_f, ds_f, dh_f = E(n, hc), E(3 * heads * n), E(n, 2 * heads), E(n, hc)
            dout_c, scr_c, ds_c, dt_c = [E(n, c) for _ in range(heads)], [E(3 * n) for _ in range(heads)], E(heads, n), E(heads, n)
            dh_c = E(n, hc)                                           # (the composition writes its dH blocks into one strided buffer)
            off = lambda t, h: P(t) + 4 * h * c                       # noqa: E731  column block h of an [n, hc] buffer

            def fwd_fused():
                lib.amar_gat_heads_f32(rp, ci, P(hd), hc, heads, c, P(s), P(b), P(y_f), hc, None, 1, 1, n, stream)

            def fwd_composed():
                for h in range(heads):
                    lib.amar_gat_layer_f32(rp, ci, off(hd, h), hc, c, P(s_h[h]), P(t_h[h]), off(b, h), off(y_c, h), hc, 1, n, stream)

            def bwd_fused():
                lib.amar_gat_heads_bwd_f32(rp, ci, rp, ci, P(hd), hc, heads, c, P(s), P(y_f), hc, P(dy), hc, P(b), P(a_s), P(a_n), None,
                                           P(dout_f), P(scr_f), P(ds_f), P(dh_f), hc, 1, 1, n, stream)

            def bwd_composed():
                for h in range(heads):
                    lib.amar_gat_bwd_f32(rp, ci, off(hd, h), hc, c, P(s_h[h]), P(t_h[h]), off(y_c, h), hc, off(dy, h), hc, off(b, h),
                                         P(as_h[h]), P(an_h[h]), P(dout_c[h]), P(scr_c[h]), P(ds_c[h]), P(dt_c[h]), off(dh_c, h), hc, 1, n, stream)

            for op, fused, composed, iters, launches in (('forward', fwd_fused, fwd_composed, 1000 if scale == 1 else 200, (1, heads)),
                                                         ('reverse', bwd_fused, bwd_composed, 300 if scale == 1 else 60, (2, 2 * heads))):
                res = compare(fused, composed, iters)
                diff = rel_diff(y_f, y_c) if op == 'forward' else rel_diff(dh_f, dh_c)
                line = {'graph': 'ml1m(s={}) user-item'.format(scale), 'rows': n, 'entries': nnz, 'heads': heads, 'channels': c, 'op': op,
                        'ms_per_call': res, 'launches': {'fused': launches[0], 'composed': launches[1]}, 'iters_per_window': iters,
                        'windows_per_side': REPEATS, 'max_rel_diff_fused_vs_composed': diff,
                        'fused_faster_outside_spread': res['fused']['max'] < res['composed']['min']}
                print(json.dumps(line), flush=True)
                lines.append(line)
        lines.extend(train_batches(scale, g))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
    slower = [(l['graph'], l['heads'], l['channels'], l['op']) for l in lines if not l.get('fused_faster_outside_spread', True)]
    if slower:
        raise SystemExit("the fused form is not faster outside the spread for: {}".format(slower))


if __name__ == '__main__':
    main()

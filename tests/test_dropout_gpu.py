"""GPU: training-time dropout (node masks of the GNN stacks, GAT attention masks) against the numpy restatement of the draws and a
float64 torch forward with those masks injected (pytest -m gpu)."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import graph as ograph
from oracle import train as otrain
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _step(value=0):
    return torch.full((1,), value, dtype=torch.int64, device=DEV)


# ---- amar_dropout_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 8, 16, 32, 64])
def test_dropout_kernel_equals_the_numpy_mask_bit_for_bit(hip, C):
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_node_mask, dropout_scale
    n, seed, site, rate = 333, 0xC0FFEE1234567, 9, 0.3
    rng = np.random.default_rng(C)
    x = rng.standard_normal((n, C)).astype(np.float32)
    wide = rng.standard_normal((n, C + 24)).astype(np.float32)
    step = _step(5)
    drop = hip.Dropout(seed, step, site, rate)

    def want(src, s):
        return torch.from_numpy(src) * torch.from_numpy(dropout_node_mask(seed, s, site, src.shape, rate).astype(np.float32)) * \
            torch.tensor(dropout_scale(rate))                        # one float32 multiply per element: bits, not a tolerance

    # contiguous, out of place and in place
    xd = _t(x)
    out = hip.dropout(xd, drop, out=torch.empty_like(xd))
    assert torch.equal(out.cpu(), want(x, 5)) and torch.equal(xd.cpu(), torch.from_numpy(x))
    hip.dropout(xd, drop)
    assert torch.equal(xd.cpu(), want(x, 5))
    assert not (xd.cpu() == 0).all() and (xd.cpu() == 0).any()
    # dropped values are +0.0, not -0.0
    assert not torch.signbit(xd.cpu()[xd.cpu() == 0]).any()
    # strided slices of a wider buffer (16-byte aligned at column 8; misaligned at column 3: the scalar path, same bits)
    for c0 in (8, 3):
        wd = _t(wide)
        sl = wd[:, c0:c0 + C]
        o2 = torch.zeros((n, C + 8), device=DEV)
        hip.dropout(sl, drop, out=o2[:, 4:4 + C])
        assert torch.equal(o2[:, 4:4 + C].cpu(), want(wide[:, c0:c0 + C], 5)) and float(o2[:, :4].abs().sum() + o2[:, 4 + C:].abs().sum()) == 0.0
        hip.dropout(sl, drop)
        got = wd.cpu().numpy()
        assert torch.equal(torch.from_numpy(got[:, c0:c0 + C].copy()), want(wide[:, c0:c0 + C], 5))
        assert np.array_equal(got[:, :c0], wide[:, :c0]) and np.array_equal(got[:, c0 + C:], wide[:, c0 + C:])
    # the step is read from device memory: one captured launch, two step values, no new capture; the entry does not advance it
    from deep_cbrs_amar_renaissance_amd.engine import capture_graph
    src, dst = _t(x), torch.empty((n, C), device=DEV)
    hip.dropout(src, drop, out=dst)
    graph, _ = capture_graph(lambda: hip.dropout(src, drop, out=dst))
    for s in (5, (3 << 32) | 77):
        step.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), want(x, s)) and int(step.item()) == s
    hip.dropout_advance(step)
    assert int(step.item()) == ((3 << 32) | 77) + 1
    # rate 0 keeps everything unchanged
    keep_all = hip.dropout(_t(x), hip.Dropout(seed, step, site, 0.0), out=torch.empty((n, C), device=DEV))
    assert torch.equal(keep_all.cpu(), torch.from_numpy(x))


def test_dropout_kernel_on_a_width_that_is_no_multiple_of_four(hip):
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_node_mask, dropout_scale
    x = np.random.default_rng(0).standard_normal((70, 6)).astype(np.float32)
    step = _step(2)
    out = hip.dropout(_t(x), hip.Dropout(4, step, 200, 0.5), out=torch.empty((70, 6), device=DEV))
    want = torch.from_numpy(x) * torch.from_numpy(dropout_node_mask(4, 2, 200, x.shape, 0.5).astype(np.float32)) * torch.tensor(dropout_scale(0.5))
    assert torch.equal(out.cpu(), want)
    with pytest.raises(ValueError):
        hip.Dropout(4, step, 0, 0.5)
    with pytest.raises(ValueError):
        hip.Dropout(4, step, 1, 1.0)


# ---- GAT with attention dropout --------------------------------------------------------------------------------------------------
def _coo_edge_mask(seed, step, site, tgt, src, n, self_loop, rate):
    """Keep bits for edges given as (target, source) arrays in ANY order (parallel entries are exchangeable: same h_j, same alpha):
    sorted into CSR order for the restatement, scattered back.  Returns (mask per edge, mask per added self loop or None)."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_edge_mask
    order = np.lexsort((src, tgt))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))])
    m, loops = dropout_edge_mask(seed, step, site, rowptr, src[order], self_loop, rate)
    mask = np.empty(len(tgt), dtype=bool)
    mask[order] = m
    return mask, loops


def _gat64(h, a_s, a_n, bias, tgt, src, keep_scale):
    """Spektral GATConv._call_single from H on (float64 torch): softmax over the undropped logits, coefficients times keep * scale."""
    n = h.shape[0]
    T, S = torch.as_tensor(tgt, dtype=torch.long), torch.as_tensor(src, dtype=torch.long)
    e = (h @ a_s)[T] + (h @ a_n)[S]
    e = torch.where(e > 0, e, 0.2 * e)
    mx = torch.full((n,), -1e30, dtype=torch.float64).scatter_reduce(0, T, e.detach(), 'amax')
    ex = torch.exp(e - mx[T])
    alpha = ex / (torch.zeros(n, dtype=torch.float64).index_add(0, T, ex) + 1e-9)[T]
    if keep_scale is not None:
        alpha = alpha * torch.as_tensor(keep_scale, dtype=torch.float64)
    return torch.relu(torch.zeros_like(h).index_add(0, T, alpha[:, None] * h[S]) + bias)


def _edges_with_masks(a, n, self_loop, seed, step, site, rate):
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_edge_mask, dropout_scale
    rowptr, colidx = a.rowptr.cpu().numpy(), a.colidx.cpu().numpy()
    tgt, src = np.repeat(np.arange(n), np.diff(rowptr)), colidx.astype(np.int64)
    mask, loops = dropout_edge_mask(seed, step, site, rowptr, colidx, self_loop, rate)
    if self_loop:
        tgt, src, mask = np.concatenate([tgt, np.arange(n)]), np.concatenate([src, np.arange(n)]), np.concatenate([mask, loops])
    return tgt, src, mask.astype(np.float64) * float(dropout_scale(rate)), mask


def _gat_graph(shape, seed):
    """'ui': a random symmetric multigraph (duplicates kept); 'uip': the user-item-property graph, whose duplicated item-property
    links are parallel entries."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import convert_to_tensor
    if shape == 'uip':
        g = helpers.tiny_graph(n_users=120, n_items=90, n_ratings=1500, seed=seed, n_props=40, n_links=300)
        adj = g['adj']
    else:
        g = helpers.tiny_graph(n_users=200, n_items=150, n_ratings=2800, seed=seed)
        adj = g['adj']
    a = convert_to_tensor(adj, with_values=False, drop_diagonal=True)
    return a, adj.shape[0]


@pytest.mark.parametrize('C', [4, 8, 16, 32, 64, 24, 48])
@pytest.mark.parametrize('self_loop', [True, False])
@pytest.mark.parametrize('shape', ['ui', 'uip'])
def test_gat_layer_with_attention_dropout(hip, C, self_loop, shape):
    """The bound and the widths of test_kernels_gpu.py:test_gat_layer, on both graph shapes, masks from the restatement."""
    a, n = _gat_graph(shape, C)
    if shape == 'uip':
        rp, ci = a.rowptr.cpu().numpy(), a.colidx.cpu().numpy()
        rows = np.repeat(np.arange(n), np.diff(rp))
        assert ((rows[1:] == rows[:-1]) & (ci[1:] == ci[:-1])).any(), "the UIP graph must hold parallel entries"
    F = 8
    rng = np.random.default_rng(C)
    x = rng.standard_normal((n, F)).astype(np.float32)
    w = rng.uniform(-0.6, 0.6, (F, C)).astype(np.float32)
    a_s, a_n = rng.uniform(-1, 1, C).astype(np.float32), rng.uniform(-1, 1, C).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    h = torch.empty((n, C), device=DEV)
    ss, sn = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.rowwise_xw(_t(x), _t(w), h, a_self=_t(a_s), a_neigh=_t(a_n), s_self=ss, s_neigh=sn)
    seed, site, rate, step = 99, 6, 0.4, _step(3)
    y = torch.empty((n, C), device=DEV)
    hip.gat_layer_dropout(a.rowptr, a.colidx, h, ss, sn, _t(b), y, hip.Dropout(seed, step, site, rate), self_loop=self_loop)
    tgt, src, ks, mask = _edges_with_masks(a, n, self_loop, seed, 3, site, rate)
    assert 0.45 < mask.mean() < 0.75
    T64 = lambda v: torch.tensor(np.asarray(v, dtype=np.float64))   # noqa: E731
    want = _gat64(T64(x) @ T64(w), T64(a_s), T64(a_n), T64(b), tgt, src, ks).numpy()
    assert helpers.rel_err(y.cpu().numpy(), want) < 1e-5
    assert int(step.item()) == 3
    # rate 0 through the new entry: the bits of amar_gat_layer_f32
    y0, y1 = torch.empty((n, C), device=DEV), torch.empty((n, C), device=DEV)
    hip.gat_layer(a.rowptr, a.colidx, h, ss, sn, _t(b), y0, self_loop=self_loop)
    hip.gat_layer_dropout(a.rowptr, a.colidx, h, ss, sn, _t(b), y1, hip.Dropout(seed, step, site, 0.0), self_loop=self_loop)
    assert torch.equal(y0, y1)


@pytest.mark.parametrize('C', [4, 8, 16, 32, 64, 24, 48])
@pytest.mark.parametrize('self_loop', [True, False])
def test_gat_bwd_with_attention_dropout(hip, C, self_loop):
    """amar_gat_bwd_dropout_f32 against float64 autograd of the restated forward with the same masks: the bounds of
    test_training_gpu.py:test_gat_bwd_kernel (2e-4 of the largest reference magnitude), on a graph with parallel entries."""
    a, n = _gat_graph('uip', C)
    rng = np.random.default_rng(C)
    h = rng.standard_normal((n, C)).astype(np.float32) * 0.7
    a_s, a_n = rng.standard_normal(C).astype(np.float32) * 0.5, rng.standard_normal(C).astype(np.float32) * 0.5
    bias = rng.standard_normal(C).astype(np.float32) * 0.1
    dy = rng.standard_normal((n, C)).astype(np.float32)
    seed, site, rate, step = 1234567, 8, 0.35, _step(11)
    drop = hip.Dropout(seed, step, site, rate)
    tgt, src, ks, _ = _edges_with_masks(a, n, self_loop, seed, 11, site, rate)
    ht = torch.tensor(h.astype(np.float64), requires_grad=True)
    ast, ant = torch.tensor(a_s.astype(np.float64), requires_grad=True), torch.tensor(a_n.astype(np.float64), requires_grad=True)
    y = _gat64(ht, ast, ant, torch.tensor(bias.astype(np.float64)), tgt, src, ks)
    (y * torch.tensor(dy.astype(np.float64))).sum().backward()
    hd, sd, nd = _t(h), torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.rowwise_xw(hd, torch.eye(C, device=DEV).contiguous(), torch.empty((n, C), device=DEV), a_self=_t(a_s), a_neigh=_t(a_n), s_self=sd, s_neigh=nd)
    yd = torch.empty((n, C), device=DEV)
    hip.gat_layer_dropout(a.rowptr, a.colidx, hd, sd, nd, _t(bias), yd, drop, self_loop=self_loop)
    assert helpers.rel_err(yd.cpu().numpy(), y.detach().numpy()) < 1e-5
    dout, ds, dt, dh = hip.gat_bwd_dropout(a.rowptr, a.colidx, hd, sd, nd, yd, _t(dy), _t(bias), _t(a_s), _t(a_n), drop, self_loop=self_loop)
    assert np.array_equal(dout.cpu().numpy(), dy * (yd.cpu().numpy() > 0))
    assert np.abs(dh.cpu().numpy() - ht.grad.numpy()).max() <= 2e-4 * np.abs(ht.grad.numpy()).max()
    das = (hd.double() * ds.double()[:, None]).sum(0).cpu().numpy()
    dan = (hd.double() * dt.double()[:, None]).sum(0).cpu().numpy()
    scale = max(np.abs(ant.grad.numpy()).max(), np.abs(ast.grad.numpy()).max())
    assert np.abs(das - ast.grad.numpy()).max() <= 2e-4 * scale and np.abs(dan - ant.grad.numpy()).max() <= 2e-4 * scale
    # no float atomics: the same call again gives the same bits; rate 0 gives amar_gat_bwd_f32's result
    again = hip.gat_bwd_dropout(a.rowptr, a.colidx, hd, sd, nd, yd, _t(dy), _t(bias), _t(a_s), _t(a_n), drop, self_loop=self_loop)
    assert all(torch.equal(p, q) for p, q in zip((dout, ds, dt, dh), again))
    y0 = torch.empty((n, C), device=DEV)
    hip.gat_layer(a.rowptr, a.colidx, hd, sd, nd, _t(bias), y0, self_loop=self_loop)
    plain = hip.gat_bwd(a.rowptr, a.colidx, hd, sd, nd, y0, _t(dy), _t(bias), _t(a_s), _t(a_n), self_loop=self_loop)
    zero = hip.gat_bwd_dropout(a.rowptr, a.colidx, hd, sd, nd, y0, _t(dy), _t(bias), _t(a_s), _t(a_n), hip.Dropout(seed, step, site, 0.0),
                               self_loop=self_loop)
    # (separate instantiations of the kernels: the compiler may contract their multiply-adds differently, so closeness, not bits)
    for p, q in zip(plain, zero):
        print('gat_bwd rate 0 vs plain: max |diff|', float((p - q).abs().max()), 'of', float(p.abs().max()))
        assert float((p - q).abs().max()) <= 1e-5 * float(p.abs().max()) + 1e-12


# ---- whole models: float64 torch forward with the masks of the restatement injected ----------------------------------------------
class _Masks:
    """What the Trainer's tapes draw at one step, per stack index (training._StackTape.enable_dropout numbers the sites)."""

    def __init__(self, trainer, step):
        self.seed, self.step, self.calls = trainer.dropout_seed, step, 0
        self.rates = [t.dropout_rates() for t in trainer.tapes]

    def node(self, stack, k, shape, dtype):
        from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_node_mask, dropout_scale
        rate = self.rates[stack][0]
        if not rate:
            return None
        m = dropout_node_mask(self.seed, self.step, 64 * stack + 2 * k + 1, shape, rate)
        return torch.as_tensor(m.astype(np.float64) * float(dropout_scale(rate)), dtype=dtype)

    def edge(self, stack, k, tgt, src, n, dtype):
        from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_scale
        rate = self.rates[stack][1][k] if self.rates[stack][1] else 0.0
        if not rate:
            return None
        loop = tgt == src                                            # (the oracle's list: stored diagonal dropped, one loop per node, reordered)
        m, loops = _coo_edge_mask(self.seed, self.step, 64 * stack + 2 * k + 2, tgt[~loop], src[~loop], n, True, rate)
        full = np.empty(len(tgt), dtype=bool)
        full[~loop], full[loop] = m, loops[tgt[loop]]
        return torch.as_tensor(full.astype(np.float64) * float(dropout_scale(rate)), dtype=dtype)


def _masked_stack(masks):
    """oracle.train._torch_stack with dropout: every layer's output times its node mask before it is kept and handed on
    (the reference's loop, gnn.py:76-81), GAT coefficients times the edge mask after the softmax.  masks None: the oracle's ops."""

    def stack(adj, x, st, self_loops=True, force_mean=True):
        kind, layers = st['kind'], st['layers']
        index = masks.calls if masks is not None else 0
        if masks is not None:
            masks.calls += 1
        n = x.shape[0]
        hs = [x]

        def keep(k, x):
            m = masks.node(index, k, tuple(x.shape), x.dtype) if masks is not None else None
            return x if m is None else x * m
        if kind in ('gcn', 'lightgcn', 'dgcf'):
            a = (ograph.dgcf_adjacency(adj) if kind == 'dgcf' else ograph.gcn_filter(adj)).tocoo()
            a_t = torch.sparse_coo_tensor(np.stack([a.row, a.col]), a.data.astype(np.float64), a.shape).coalesce()
            for k, lw in enumerate(layers):
                if kind == 'gcn':
                    x = torch.relu(torch.sparse.mm(a_t, x @ lw['kernel']) + lw['bias'])
                elif kind == 'lightgcn':
                    x = torch.sparse.mm(a_t, x)
                else:
                    x = torch.sparse.mm(a_t, x * torch.sigmoid(lw['w']))
                x = keep(k, x)
                hs.append(x)
        else:
            row, col, _ = ograph.reordered_coo(adj)
            assert self_loops
            row, col = ograph.add_self_loops_edges(row, col, n)
            src_np, tgt_np = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
            src, tgt = torch.as_tensor(src_np), torch.as_tensor(tgt_np)
            count = torch.bincount(tgt, minlength=n).to(x.dtype).clamp(min=1.0)
            for k, lw in enumerate(layers):
                if kind == 'sage':
                    agg = torch.zeros_like(x).index_add(0, tgt, x[src]) / count[:, None]
                    z = torch.cat([x, agg], 1) @ lw['kernel'] + lw['bias']
                    z = z * torch.rsqrt(torch.clamp((z * z).sum(1, keepdim=True), min=1e-12))
                    x = torch.relu(z)
                else:
                    h = x @ lw['kernel']
                    e = (h @ lw['attn_self'])[tgt] + (h @ lw['attn_neigh'])[src]
                    e = torch.where(e > 0, e, 0.2 * e)
                    seg_max = torch.full((n,), -float('inf'), dtype=x.dtype).scatter_reduce(0, tgt, e.detach(), 'amax')
                    ex = torch.exp(e - seg_max[tgt])
                    alpha = ex / (torch.zeros(n, dtype=x.dtype).index_add(0, tgt, ex) + 1e-9)[tgt]
                    em = masks.edge(index, k, tgt_np, src_np, n, x.dtype) if masks is not None else None
                    if em is not None:
                        alpha = alpha * em
                    x = torch.relu(torch.zeros_like(h).index_add(0, tgt, alpha[:, None] * h[src]) + lw['bias'])
                x = keep(k, x)
                hs.append(x)
        final_node = st.get('final_node', 'concatenation')
        if force_mean and kind in ('lightgcn', 'dgcf'):
            final_node = 'mean'
        if final_node == 'concatenation':
            return torch.cat(hs, 1)
        if final_node == 'last':
            return hs[-1]
        if final_node == 'w-sum':
            w = st['reduction_w'].reshape(-1)
            return sum((w[k] * w[k]) * h for k, h in enumerate(hs))
        return sum(hs) / (len(hs) if final_node == 'mean' else 1)
    return stack


def _assert_grads(trainer, grads, flat):
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)      # the trainer folds the L2 term into the Adam kernel
        assert np.abs(got - gw).max() <= 2e-4 * np.abs(gw).max() + 1e-10, tuple(prm.shape)


def _check_model(monkeypatch, model, trainer, adjs, oracle_gnn, oracle_head, flatten, u, i, y, **kw):
    """Pins the masked float64 forward at rate 0 against oracle.train.torch_model_grads, then compares the Trainer's loss and
    gradients at step 0 and at step 1 (another mask) with it."""
    plain = otrain.torch_model_grads(adjs, oracle_gnn, oracle_head, u, i, y, l2=1e-4, **kw)
    monkeypatch.setattr(otrain, '_torch_stack', _masked_stack(None))
    pinned = otrain.torch_model_grads(adjs, oracle_gnn, oracle_head, u, i, y, l2=1e-4, **kw)
    assert abs(plain[0] - pinned[0]) < 1e-12 and np.abs(plain[2] - pinned[2]).max() < 1e-12
    for a, b in zip(flatten(plain[1]).values(), flatten(pinned[1]).values()):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
    losses = []
    for step in (0, 1):
        assert int(trainer.dropout_step.item()) == step
        loss, grads = trainer.loss_and_grads(u, i, y, **({'bert': kw['bert']} if 'bert' in kw else {}))
        monkeypatch.setattr(otrain, '_torch_stack', _masked_stack(_Masks(trainer, step)))
        want_loss, want, _ = otrain.torch_model_grads(adjs, oracle_gnn, oracle_head, u, i, y, l2=1e-4, **kw)
        assert abs(loss - want_loss) < 1e-5
        _assert_grads(trainer, grads, flatten(want))
        losses.append(want_loss)
    assert abs(losses[0] - plain[0]) > 1e-6 and abs(losses[0] - losses[1]) > 1e-7      # the masks bite, and differ between steps


def _flatten_single(model):
    from tests.test_training_gpu import _flatten_oracle_grads
    return lambda grads: _flatten_oracle_grads(model, grads)


@pytest.mark.parametrize('cls,extra', [('BasicGCN', dict(dropout=0.2)), ('BasicLightGCN', dict(dropout=0.2)),
                                       ('BasicGraphSage', dict(dropout=0.2)), ('BasicDGCF', dict(dropout=0.2)),
                                       ('BasicGAT', dict(dropout=0.2)), ('BasicGAT', dict(dropout_rate=0.2)),
                                       ('BasicGAT', dict(dropout=0.3, dropout_rate=0.2)),
                                       ('BasicGCN', dict(dropout=0.2, final_node='mean')), ('BasicGAT', dict(dropout=0.2, dropout_rate=0.2, final_node='w-sum'))])
@pytest.mark.parametrize('graph', ['ui', 'uip'])
def test_gradients_with_dropout_match_float64_autograd(hip, monkeypatch, cls, extra, graph):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(5)
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9,
                           n_props=30 if graph == 'uip' else 0, n_links=90 if graph == 'uip' else 0)
    model = getattr(basic, cls)(g['adj'], **dict(CFG, **extra))
    helpers.randomize_biases(model, seed=6)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    if cls == 'BasicDGCF':                                    # gates away from their all-ones start
        model.gnn.build_layers()
        with torch.no_grad():
            for layer in model.gnn.gnn_layers.seq_layers:
                layer.w.add_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, tuple(layer.w.shape)).astype(np.float32)).to(layer.w.device))
    _check_model(monkeypatch, model, trainer, g['adj'], helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs),
                 _flatten_single(model), g['u_ids'], g['i_ids'], y)


def test_hybrid_gradients_with_dropout(hip, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    engine.set_seed(11)
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=4)
    cfg = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[[24, 16], [32, 24], [16, 16]], clf_units=[24, 16],
               l2_regularizer=1e-4, feature_based=True, fusion_method='concatenate', residual=False, dropout=0.2)
    model = hybrid.HybridBertGCN(g['adj'], **cfg)
    rng = np.random.default_rng(3)
    table = rng.standard_normal((g['adj'].shape[0], 40)).astype(np.float32) * 0.5
    model.set_bert_table(table)
    y = rng.integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    helpers.randomize_biases(model, seed=7)
    u, i = g['u_ids'], g['i_ids']
    _check_model(monkeypatch, model, trainer, g['adj'], helpers.gnn_to_oracle(model.gnn), helpers.hybrid_head_to_oracle(model.rs),
                 _flatten_single(model), u, i, y, bert=(table[u], table[i]), feature_based=True)


@pytest.mark.parametrize('kind,extra', [('GCN', dict(dropout=0.2)), ('GAT', dict(dropout=0.2, dropout_rate=0.2))])
def test_two_step_gradients_with_dropout(hip, monkeypatch, kind, extra):
    """Both stacks of a TwoStep model drop, each with its own sites (stack index 0: item-property, 1: user-item)."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests.test_twostep_twoway_gpu import _flatten, _perturb
    engine.set_seed(5)
    g = helpers.kg_graph(n_users=60, n_items=45, n_props=30, n_ratings=900, n_links=120, seed=11)
    adjs = (g['adj_ui'], g['adj_ip'])
    model = getattr(basic, 'BasicTS' + kind)(g['n_users'], g['n_items'], adjs, **dict(CFG, item_node='mean', **extra))
    _perturb(model, 29)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    assert trainer.layout == 'two_step' and [d.site for d in trainer.tapes[1].node_drop] == [65, 67]
    _check_model(monkeypatch, model, trainer, adjs, helpers.two_step_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs),
                 lambda grads: _flatten(model, grads, 'two_step'), g['u_ids'], g['i_ids'], y, n_users=g['n_users'], n_items=g['n_items'])


# ---- fit() ---------------------------------------------------------------------------------------------------------------------
def _bce_sequence(batch_size=128, shuffle=False):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    g = helpers.tiny_graph(n_users=70, n_items=50, n_ratings=1400, seed=3)
    return g, UserItemGraph(g['ratings'][:1280], g['users'], g['items'], g['adj'], batch_size=batch_size, shuffle=shuffle)


def _bce_model(g, cls, seed=8, **extra):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(seed)
    model = getattr(basic, cls)(g['adj'], **dict(CFG, **extra))
    helpers.randomize_biases(model, seed=1)
    model.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=1e-3), metrics=['accuracy'])
    model((g['u_ids'], g['i_ids']))
    return model


def _bpr_model(seq, cls, seed=8, **extra):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    engine.set_seed(seed)
    model = getattr(basic, cls)(seq.adj_matrix, **dict(CFG, **extra))
    helpers.randomize_biases(model, seed=1)
    model.compile(loss=BPRLoss(), optimizer=Adam(learning_rate=1e-3))
    model(seq[0][0])
    return model


@pytest.mark.parametrize('cls,extra', [('BasicGCN', dict(dropout=0.2)), ('BasicGAT', dict(dropout=0.2, dropout_rate=0.2)),
                                       ('BasicGraphSage', dict(dropout=0.2))])
@pytest.mark.parametrize('loss', ['bce', 'bpr'])
def test_fit_replayed_equals_eager_with_dropout(hip, monkeypatch, cls, extra, loss):
    """10 steps per epoch, 2 epochs: the captured graph draws a new mask at every replay (the step counter lives on the device) and
    gives the weights of the same body run eagerly, bit for bit; one seed repeats, another seed does not."""
    from tests.test_bpr_gpu import _sample_sequence
    if loss == 'bpr':
        seq = _sample_sequence()
        make = lambda seed: _bpr_model(seq, cls, seed=seed, **extra)     # noqa: E731
    else:
        g, seq = _bce_sequence()
        make = lambda seed: _bce_model(g, cls, seed=seed, **extra)       # noqa: E731
    assert len(seq) >= 4
    models, hist = [], []
    for env, seed in (('0', 8), ('1', 8), ('1', 8), ('1', 9)):
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = make(seed)
        hist.append(m.fit(seq, epochs=2, verbose=False)['loss'])
        models.append(m)
    eager, replayed, again, other = models
    assert replayed._trainer._graphs and not eager._trainer._graphs
    assert hist[0] == hist[1] == hist[2] and np.isfinite(hist[0]).all()
    for pa, pb, pc in zip(eager.parameters(), replayed.parameters(), again.parameters()):
        assert torch.equal(pa, pb) and torch.equal(pb, pc), tuple(pa.shape)
    steps = 2 * len(seq)
    for m in models:
        assert m._trainer.t == steps and int(m._trainer.dropout_step.item()) == steps
    assert replayed._trainer.dropout_seed == eager._trainer.dropout_seed != other._trainer.dropout_seed
    # (seed 9 also initialises other weights; the masks themselves are compared below)
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_node_mask
    tape = replayed._trainer.tapes[0]
    n, c = replayed.gnn.gnn_layers.adj_matrix.shape[0], 8
    masks = [dropout_node_mask(t.dropout_seed, 2, tape.node_drop[0].site, (n, c), 0.2) for t in (replayed._trainer, other._trainer)]
    assert (masks[0] != masks[1]).any()


def test_replayed_steps_draw_the_masks_of_the_restatement(hip, monkeypatch):
    """After a replayed epoch, the tape's forward at step values 2 and 3 (the launches the graph replays, reading the same device
    counter): the first layer's slice is zero exactly where the restatement says, and the two steps' masks differ."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_node_mask
    monkeypatch.setenv('AMAR_TRAIN_GRAPH', '1')
    g, seq = _bce_sequence()
    model = _bce_model(g, 'BasicLightGCN', dropout=0.5)
    model.fit(seq, epochs=1, verbose=False)                        # 10 steps: 1 eager, 9 replayed
    trainer = model._trainer
    assert trainer._graphs and int(trainer.dropout_step.item()) == len(seq)
    tape, site = trainer.tapes[0], trainer.tapes[0].node_drop[0].site
    n = model.gnn.gnn_layers.adj_matrix.shape[0]
    graph = next(iter(trainer._graphs.values()))['graph']
    seen = []
    for step in (2, 3):
        trainer.dropout_step.fill_(step)
        cat = {}
        orig = tape.forward

        def spy(x0=None, _orig=orig):
            out = _orig(x0)
            cat['slice'] = tape.cat[:, 8:16].clone()
            return out
        monkeypatch.setattr(tape, 'forward', spy)
        with torch.no_grad():
            trainer._propagation_forward()                           # the same launches as the graph's forward, at this step value
        monkeypatch.setattr(tape, 'forward', orig)
        want = dropout_node_mask(trainer.dropout_seed, step, site, (n, 8), 0.5)
        got = cat['slice'].cpu().numpy()
        assert (got[~want] == 0).all() and (got[want] != 0).mean() > 0.9       # (a kept value may itself be 0: a node without edges)
        seen.append(want)
    assert (seen[0] != seen[1]).mean() > 0.3
    assert graph is not None


@pytest.mark.parametrize('cls,extra', [('BasicGCN', dict(dropout=0.3)), ('BasicGAT', dict(dropout=0.3, dropout_rate=0.4)),
                                       ('BasicLightGCN', dict(dropout=0.3))])
def test_inference_ignores_dropout(hip, cls, extra):
    """A model with rates set and one without, same weights: predict(), evaluate(), recommend() bit-identical."""
    g, seq = _bce_sequence()
    plain, dropped = _bce_model(g, cls), _bce_model(g, cls, **extra)
    for pa, pb in zip(plain.parameters(), dropped.parameters()):
        assert torch.equal(pa, pb)
    assert np.array_equal(np.asarray(plain.predict(seq)), np.asarray(dropped.predict(seq)))
    assert plain.evaluate(seq) == dropped.evaluate(seq)
    with torch.no_grad():
        assert torch.equal(plain((g['u_ids'], g['i_ids'])), dropped((g['u_ids'], g['i_ids'])))
    for a, b in zip(plain.recommend(seq, k=5), dropped.recommend(seq, k=5)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # after training with dropout, evaluate() still is the loss of the undropped forward
    dropped.fit(seq, epochs=1, verbose=False)
    twin = _bce_model(g, cls)
    with torch.no_grad():
        for pa, pb in zip(twin.parameters(), dropped.parameters()):
            pa.copy_(pb)
    assert twin.evaluate(seq) == dropped.evaluate(seq)


@pytest.mark.parametrize('cls,key', [('BasicGCN', 'dropout'), ('BasicGAT', 'dropout'), ('BasicGAT', 'dropout_rate')])
@pytest.mark.parametrize('none', [0.0, None])
def test_fit_with_rate_zero_equals_fit_without_the_key(hip, cls, key, none):
    g, seq = _bce_sequence()
    a, b = _bce_model(g, cls), _bce_model(g, cls, **{key: none})
    ha, hb = a.fit(seq, epochs=2, verbose=False)['loss'], b.fit(seq, epochs=2, verbose=False)['loss']
    assert b._trainer.dropout_step is None and b._trainer.dropout_key == ()
    assert all(k[:3] == (128, False, 'bce') and len(k) == 3 for k in b._trainer._graphs)
    if cls == 'BasicGCN':                                          # (its scatter owns its rows: no float atomics anywhere in the step)
        assert ha == hb
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb), tuple(pa.shape)


@pytest.mark.parametrize('cls,extra', [('BasicGCN', dict(dropout=0.2)), ('BasicGAT', dict(dropout=0.2, dropout_rate=0.2))])
def test_fit_with_dropout_learns_a_separable_task(hip, cls, extra):
    """The task and the criterion of test_training_gpu.py:test_fit_learns_a_separable_task, with dropout."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    engine.set_seed(11)
    g = helpers.tiny_graph(n_users=100, n_items=80, n_ratings=4000, seed=5)
    model = getattr(basic, cls)(g['adj'], **dict(CFG, l2_regularizer=1e-6, **extra))
    model.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=0.01), metrics=['accuracy'])
    seq = UserItemGraph(g['ratings'], g['users'], g['items'], g['adj'], batch_size=512, shuffle=True)
    before = model.evaluate(seq)
    hist = model.fit(seq, epochs=12, verbose=False)
    after = model.evaluate(seq)
    print('dropout fit', cls, 'loss', hist['loss'][0], '->', hist['loss'][-1], 'evaluate', before, '->', after)
    assert hist['loss'][-1] < hist['loss'][0] - 0.02
    assert after[0] < before[0] and after[1] > max(before[1], 0.6)


def test_graph_key_carries_the_dropout_state(hip):
    from deep_cbrs_amar_renaissance_amd import training
    g, seq = _bce_sequence()
    model = _bce_model(g, 'BasicGAT', dropout=0.2, dropout_rate=0.1)
    model.fit(seq, epochs=1, verbose=False)
    tr = model._trainer
    (key,) = tr._graphs.keys()
    assert key[:3] == (128, False, 'bce') and key[3:] == tr.dropout_key
    assert tr.dropout_key == (tr.dropout_seed, tr.dropout_step.data_ptr(), ((0.2, (0.1, 0.1)),))
    with pytest.raises(NotImplementedError):
        training._StackTape(model.gnn.gnn_layers).enable_dropout(1, tr.dropout_step, 3)


def test_experiment_with_gat_dropout_runs_to_its_metrics(hip, tmp_path, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update({k: v for k, v in paths.items() if k != 'props_triples_filepath'})
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    grid = {'linear': {'gat-dropout': {
        'model': {'name': 'basic.BasicGAT', 'dropout_rate': 0.2, 'dropout': 0.1, 'embedding_dim': 8, 'n_hiddens': [8, 8],
                  'dense_units': [24, 24], 'clf_units': [48, 48]},
        'dataset': {'load_function_name': 'load_user_item_graph'}}}}
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump(grid))
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('dropout', str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log)
    assert len(multi.experiments) == 1
    results = multi.run()
    (metrics,) = results.values()
    assert metrics is not None and list(metrics.index) == ['precision_at', 'recall_at', 'f1_at']
    assert ((metrics.values >= 0) & (metrics.values <= 1)).all()
    assert glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'artifacts' / 'predictions' / 'top_5' / 'results.tsv'))

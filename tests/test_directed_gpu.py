"""Training on directed graphs (dataset.symmetric_adjacency: False): the device CSR transpose and every reverse pass on A^T
(pytest -m gpu).  Bounds are those of the tests named in each docstring: the same kernels, the same criteria."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml
from scipy import sparse

from oracle import models as om
from oracle import train as otrain
from tests import directed_ref as dr
from tests import helpers
from tests import sage_agg_ref as sref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the transpose kernel -----------------------------------------------------------------------------------------------------
def _check_transpose(hip, rowptr, colidx, n_cols, fast=False):
    want = (dr.stable_transpose_fast if fast else dr.stable_transpose)(rowptr, colidx, n_cols)
    runs = [hip.csr_transpose(_t(np.asarray(rowptr, np.int32)), _t(np.asarray(colidx, np.int32)), n_cols) for _ in range(2)]
    for name, w, g0, g1 in zip(('t_rowptr', 't_colidx', 'perm'), want, runs[0], runs[1]):
        assert g0.dtype == torch.int32 and np.array_equal(g0.cpu().numpy(), w), name
        assert torch.equal(g0, g1), name                            # the same bits on every run
    return runs[0]


@pytest.mark.parametrize('name', ['ui', 'uip', 'mixed'])
def test_transpose_kernel_on_the_small_graphs(hip, name):
    adj = dr.graph(name)['adj']
    rowptr, colidx, _ = dr.csr_of(adj)
    _check_transpose(hip, rowptr, colidx, adj.shape[1])


def test_transpose_kernel_edge_shapes(hip):
    _check_transpose(hip, np.zeros(1, np.int32), np.zeros(0, np.int32), 0)                   # n = 0
    _check_transpose(hip, np.zeros(1, np.int32), np.zeros(0, np.int32), 5)                   # no rows, some columns
    _check_transpose(hip, np.zeros(8, np.int32), np.zeros(0, np.int32), 6)                   # nnz = 0
    _check_transpose(hip, np.array([0, 7], np.int32), np.array([0, 3, 3, 3, 9, 11, 11], np.int32), 12)      # a single row
    rng = np.random.default_rng(1)
    rect = sparse.coo_matrix((np.ones(4000, np.float32), (rng.integers(0, 37, 4000), rng.integers(0, 301, 4000))), shape=(37, 301))
    rowptr, colidx, _ = dr.csr_of(rect)
    _check_transpose(hip, rowptr, colidx, 301)                                               # rectangular, many duplicates
    # unsorted columns inside the rows: the definition does not need them sorted
    shuffled = colidx.copy()
    for i in range(37):
        rng.shuffle(shuffled[rowptr[i]:rowptr[i + 1]])
    _check_transpose(hip, rowptr, shuffled, 301, fast=True)
    with pytest.raises(ValueError):
        hip.csr_transpose(_t(np.array([0, 2], np.int32)), _t(np.array([0, 5], np.int32)), 5)    # a column outside the matrix
    with pytest.raises(ValueError):
        hip.csr_transpose(_t(np.array([0, 1], np.int32)), _t(np.array([0, 1], np.int32)), 5)    # rowptr does not end at nnz


def test_transpose_kernel_on_hub_columns(hip, ml1m_s1):
    """The un-symmetrised ml1m(s=1) training graph (item columns of thousands of raters: LDS sorts of every length up to the tile)
    and one column of 150 000 entries among short ones (the in-memory sort of a long output row)."""
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    adj = build_adjacency_matrix(ml1m_s1['train'], ml1m_s1['users'], ml1m_s1['items'], symmetric_adjacency=False)
    rowptr, colidx, _ = dr.csr_of(adj)
    assert np.bincount(colidx).max() > 1000
    _check_transpose(hip, rowptr, colidx, adj.shape[1], fast=True)
    rng = np.random.default_rng(2)
    n_rows, n_cols = 160000, 5000
    rows = np.concatenate([np.arange(150000), rng.integers(0, n_rows, 400000), np.arange(9000)])
    cols = np.concatenate([np.full(150000, 77), rng.integers(0, n_cols, 400000), np.full(9000, 4999)])       # 9 000+: just past the LDS tile
    m = sparse.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_rows, n_cols))
    rowptr, colidx, _ = dr.csr_of(m)
    assert np.bincount(colidx).max() >= 150000
    _check_transpose(hip, rowptr, colidx, n_cols, fast=True)


@pytest.mark.parametrize('name', ['uip', 'mixed'])
def test_device_csr_transposed(hip, name):
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR, gcn_filter
    adj = dr.graph(name)['adj']
    a = DeviceCSR.from_scipy(gcn_filter(adj))                        # valued, with the factors of the value-free images
    assert a.gcn_filtered and a.mult is not None and not a.is_symmetric()
    at = a.transposed()
    assert at is a.transposed() and at is not a and at.shape == (a.shape[1], a.shape[0])
    assert (abs(at.to_scipy() - a.to_scipy().T) > 0).nnz == 0       # the same values, bit for bit, at the transposed places
    assert at.dinv is a.dinv and torch.equal(at.mult, a.mult[at.perm.long()]) and torch.equal(at.vals, a.vals[at.perm.long()])
    assert at.transposed() is a
    # ... and transposing the image again with the kernel gives A's arrays exactly
    r2, c2, p2 = hip.csr_transpose(at.rowptr, at.colidx, at.shape[1])
    assert torch.equal(r2, a.rowptr) and torch.equal(c2, a.colidx) and torch.equal(at.vals[p2.long()], a.vals)
    sym = DeviceCSR.from_scipy(gcn_filter(dr.tiny('ui')['adj_sym']))
    assert sym.is_symmetric() and sym.transposed() is sym


# ---- 2. forward guard ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['BasicGCN', 'BasicLightGCN', 'BasicGraphSage', 'BasicGAT', 'BasicDGCF'])
@pytest.mark.parametrize('name', ['ui', 'mixed'])
def test_forward_on_a_directed_graph_matches_the_oracle(hip, cls, name):
    """Node representations and scores against the numpy oracle (bounds of test_models_gpu.py:test_other_reductions /
    __graft_entry__.smoke: 1e-5 relative on the table, 1e-4 on the scores)."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(5)
    g = dr.graph(name)
    model = getattr(basic, cls)(g['adj'], **CFG)
    helpers.randomize_biases(model, seed=6)
    got = model.gnn(None).cpu().numpy()
    want = om.propagate(g['adj'], helpers.gnn_to_oracle(model.gnn), np.float64)
    assert got.shape == want.shape and helpers.rel_err(got, want) < 1e-5
    scores = model((g['u_ids'], g['i_ids'])).cpu().numpy()
    want_s = om.basic_gnn_scores(g['adj'], helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs), g['u_ids'], g['i_ids'])
    assert np.abs(scores - want_s).max() < 1e-4


@pytest.mark.parametrize('aggregate', ['sum', 'max', 'min'])
@pytest.mark.parametrize('name', ['ui', 'mixed'])
def test_forward_of_the_other_aggregators_on_a_directed_graph(hip, aggregate, name):
    """test_sage_aggregate_gpu.py:test_basic_graphsage_scores_tiny on the directed graphs ('mean' is in the test above)."""
    from tests.test_sage_aggregate_gpu import _model
    g = dr.graph(name)
    model, gnn, head = _model(g, aggregate)
    got = model((g['u_ids'], g['i_ids'])).cpu().numpy().reshape(-1)
    _, _, want = sref.torch_model_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], np.zeros(len(g['u_ids'])), aggregate)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-4


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------
def _assert_grads(trainer, grads, flat, violated=None):
    """The criterion of test_training_gpu.py:test_gradients_match_oracle.  violated: a parameter for which it must NOT hold."""
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)      # the trainer folds the L2 term into amar_adam_f32
        err, bound = np.abs(got - gw).max(), 2e-4 * np.abs(gw).max() + 1e-10
        print('gradient', tuple(prm.shape), 'err', err, 'bound', bound)
        if violated is None:
            assert err <= bound, tuple(prm.shape)
        elif prm is violated:
            assert err > bound, "the graph does not tell A from A^T"


def _wrong_transpose_violates(monkeypatch, model, g, y, flat_of):
    """With A in place of A^T in the reverse pass, the node table's gradient must miss the criterion: the graph tells the two apart."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    with monkeypatch.context() as mp:
        mp.setattr(DeviceCSR, 'transposed', lambda self: self)
        wrong = training.Trainer(model)
        assert wrong.tapes[0].at is wrong.tapes[0].seq.adj_matrix
        _, grads = wrong.loss_and_grads(g['u_ids'], g['i_ids'], y)
    _assert_grads(wrong, grads, flat_of, violated=model.gnn.gnn_layers.embeddings)


# (the weight-free stacks reduce by 'mean' whatever final_node says — gnn.py — so 'w-sum' is a case of the three weighted kinds only,
# as in test_training_gpu.py:test_weighted_sum_reduction_gradients_match_autograd_oracle)
GRADIENT_CASES = [(cls, final_node) for cls in ('BasicGCN', 'BasicLightGCN', 'BasicGraphSage', 'BasicGAT', 'BasicDGCF')
                  for final_node in ('concatenation', 'mean', 'w-sum') if not (final_node == 'w-sum' and cls in ('BasicLightGCN', 'BasicDGCF'))]


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('cls,final_node', GRADIENT_CASES)
@pytest.mark.parametrize('name', ['ui', 'uip', 'mixed'])
def test_gradients_on_a_directed_graph_match_the_oracle(hip, cls, name, fused, final_node, monkeypatch):
    """The bodies of test_training_gpu.py:test_gradients_match_oracle (GCN, LightGCN: the manual numpy reverse pass with a_hat.T) and
    :test_gradients_match_autograd_oracle (the others: float64 autograd of the restated forward), same CFG and criteria."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests.test_training_gpu import _flatten_oracle_grads
    monkeypatch.setenv('AMAR_DENSE_BWD', '1' if fused else '0')
    monkeypatch.setenv('AMAR_DENSE_STACK', '1' if fused else '0')
    monkeypatch.setenv('AMAR_DENSE_STACK_BWD', '1' if fused else '0')
    engine.set_seed(5)
    g = dr.graph(name)
    model = getattr(basic, cls)(g['adj'], **dict(CFG, final_node=final_node))
    helpers.randomize_biases(model, seed=6)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    tape = trainer.tapes[0]
    assert tape.at is not tape.seq.adj_matrix and tape.at is tape.seq.adj_matrix.transposed()
    loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    if cls == 'BasicDGCF':                                    # gates away from their all-ones start
        with torch.no_grad():
            for layer in model.gnn.gnn_layers.seq_layers:
                layer.w.add_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, tuple(layer.w.shape)).astype(np.float32)).to(layer.w.device))
        loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    if final_node == 'w-sum':                                 # ... and so the reduction weights
        with torch.no_grad():
            model.gnn.gnn_layers.reduce.w.copy_(torch.tensor([0.7, -1.3, 0.4], device=DEV).view(3, 1, 1))
        loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    with torch.no_grad():
        e_inf = model.gnn.gnn_layers(None)
        e_trn = trainer._propagation_forward()
    assert float((e_inf - e_trn).abs().max()) < 2e-6
    # (the manual numpy reverse pass restates GCN under 'concatenation' and LightGCN, which reduces by 'mean' whatever final_node says)
    manual = cls == 'BasicLightGCN' or (cls == 'BasicGCN' and final_node == 'concatenation')
    oracle = otrain.loss_and_grads if manual else otrain.torch_model_grads
    want_loss, want, _ = oracle(g['adj'], helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs),
                                g['u_ids'], g['i_ids'], y, l2=1e-4)
    assert abs(loss - want_loss) < 1e-5
    flat = _flatten_oracle_grads(model, want)
    _assert_grads(trainer, grads, flat)
    if name == 'mixed':
        _wrong_transpose_violates(monkeypatch, model, g, y, flat)


@pytest.mark.parametrize('aggregate', ['sum', 'max', 'min'])
@pytest.mark.parametrize('name', ['ui', 'uip', 'mixed'])
def test_gradients_of_the_other_aggregators_on_a_directed_graph(hip, aggregate, name, monkeypatch):
    """test_sage_aggregate_gpu.py:test_gradients_match_autograd_oracle on the directed graphs (its seed 11 also makes the float32 and
    the float64 run of the reference select the same entries on these three graphs: checked on the host, asserted below)."""
    from deep_cbrs_amar_renaissance_amd import training
    from tests.test_sage_aggregate_gpu import _model
    from tests.test_training_gpu import _flatten_oracle_grads
    g = dr.graph(name)
    model, gnn, head = _model(g, aggregate)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    assert sref.same_selection(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, aggregate, l2=1e-4)
    trainer = training.Trainer(model)
    loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    want_loss, want, _ = sref.torch_model_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, aggregate, l2=1e-4)
    assert abs(loss - want_loss) < 1e-5
    flat = _flatten_oracle_grads(model, want)
    _assert_grads(trainer, grads, flat)
    if name == 'mixed':
        _wrong_transpose_violates(monkeypatch, model, g, y, flat)


# ---- 4. the GAT reverse kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 8, 16, 24, 32, 48, 64])
@pytest.mark.parametrize('self_loop', [True, False])
@pytest.mark.parametrize('rate', [None, 0.35])
def test_gat_bwd_directed_kernel(hip, C, self_loop, rate):
    """test_training_gpu.py:test_gat_bwd_kernel / test_dropout_gpu.py:test_gat_bwd_with_attention_dropout through the directed entry
    points on `mixed`: float64 autograd of the restated forward over the list's own (target = row, source = column) pairs."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    from tests.test_dropout_gpu import _edges_with_masks, _gat64, _step
    adj = dr.mixed()['adj']
    a = DeviceCSR.from_scipy(adj, with_values=False, drop_diagonal=True)
    at = a.transposed()
    assert at is not a
    n = adj.shape[0]
    rng = np.random.default_rng(C)
    h = rng.standard_normal((n, C)).astype(np.float32) * 0.7
    a_s, a_n = rng.standard_normal(C).astype(np.float32) * 0.5, rng.standard_normal(C).astype(np.float32) * 0.5
    bias = rng.standard_normal(C).astype(np.float32) * 0.1
    dy = rng.standard_normal((n, C)).astype(np.float32)
    seed, site, step = 1234567, 8, _step(11)
    if rate is None:
        rowptr, colidx = a.rowptr.cpu().numpy(), a.colidx.cpu().numpy()
        tgt, src, ks = np.repeat(np.arange(n), np.diff(rowptr)), colidx.astype(np.int64), None
        if self_loop:
            tgt, src = np.concatenate([tgt, np.arange(n)]), np.concatenate([src, np.arange(n)])
    else:
        tgt, src, ks, mask = _edges_with_masks(a, n, self_loop, seed, 11, site, rate)
        assert 0.5 < mask.mean() < 0.8
    ht = torch.tensor(h.astype(np.float64), requires_grad=True)
    ast, ant = torch.tensor(a_s.astype(np.float64), requires_grad=True), torch.tensor(a_n.astype(np.float64), requires_grad=True)
    y = _gat64(ht, ast, ant, torch.tensor(bias.astype(np.float64)), tgt, src, ks)
    (y * torch.tensor(dy.astype(np.float64))).sum().backward()
    hd, sd, nd = _t(h), torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.rowwise_xw(hd, torch.eye(C, device=DEV).contiguous(), torch.empty((n, C), device=DEV), a_self=_t(a_s), a_neigh=_t(a_n), s_self=sd, s_neigh=nd)
    yd = torch.empty((n, C), device=DEV)
    args = (a.rowptr, a.colidx, hd, sd, nd, yd, _t(dy), _t(bias), _t(a_s), _t(a_n))
    if rate is None:
        hip.gat_layer(a.rowptr, a.colidx, hd, sd, nd, _t(bias), yd, self_loop=self_loop)
        run = lambda tr: hip.gat_bwd(*args, self_loop=self_loop, transposed=tr)                             # noqa: E731
    else:
        drop = hip.Dropout(seed, step, site, rate)
        hip.gat_layer_dropout(a.rowptr, a.colidx, hd, sd, nd, _t(bias), yd, drop, self_loop=self_loop)
        run = lambda tr: hip.gat_bwd_dropout(*args, drop, self_loop=self_loop, transposed=tr)               # noqa: E731
    assert helpers.rel_err(yd.cpu().numpy(), y.detach().numpy()) < 1e-5
    dout, ds, dt, dh = run((at.rowptr, at.colidx))
    assert np.array_equal(dout.cpu().numpy(), dy * (yd.cpu().numpy() > 0))
    err = np.abs(dh.cpu().numpy() - ht.grad.numpy()).max()
    print('gat_bwd directed', C, self_loop, rate, 'dH err', err, 'of', np.abs(ht.grad.numpy()).max())
    assert err <= 2e-4 * np.abs(ht.grad.numpy()).max()
    das = (hd.double() * ds.double()[:, None]).sum(0).cpu().numpy()
    dan = (hd.double() * dt.double()[:, None]).sum(0).cpu().numpy()
    scale = max(np.abs(ant.grad.numpy()).max(), np.abs(ast.grad.numpy()).max())
    assert np.abs(das - ast.grad.numpy()).max() <= 2e-4 * scale and np.abs(dan - ant.grad.numpy()).max() <= 2e-4 * scale
    assert all(torch.equal(p, q) for p, q in zip((dout, ds, dt, dh), run((at.rowptr, at.colidx))))          # no float atomics
    # the structure in place of its transpose: the source walk's results must miss the bound (the graph tells the two apart) ...
    wrong = run(None)
    # (not finite counts as a miss: without the self loop a row that is empty in A has no softmax statistics to be read through A's columns)
    assert not np.abs(wrong[3].cpu().numpy() - ht.grad.numpy()).max() <= 2e-4 * np.abs(ht.grad.numpy()).max()
    # ... and one structure passed twice through the directed entry point is the symmetric entry point, bit for bit
    # (compared as bit patterns: the non-finite values of the deliberately wrong walk are not equal to themselves as floats)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(wrong, run((a.rowptr, a.colidx))))


# ---- 5. the max / min reverse alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [4, 8, 24, 32])
@pytest.mark.parametrize('op', ['max', 'min'])
@pytest.mark.parametrize('self_loop', [True, False])
def test_reverse_aggregate_on_the_transposed_list(hip, F, op, self_loop):
    """test_sage_aggregate_gpu.py:test_reverse_aggregate on `mixed`, ties planted across duplicate entries and across the sources of
    one target; the reverse launch gets the TRANSPOSED structure."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    g = dr.mixed()
    m = g['adj'].tocoo()
    n, nu = m.shape[0], g['n_users']
    a = DeviceCSR.from_scipy(m, with_values=False, drop_diagonal=True)          # row i lists the sources of target i
    at = a.transposed()
    rng = np.random.default_rng(F)
    x = np.maximum(rng.standard_normal((n, F)), 0).astype(np.float32) * (1.0 if op == 'max' else -1.0)     # half of every column ties at 0
    x[nu + 2] = 30.0 if op == 'max' else -30.0               # the doubled entry (9 <- n_users + 2) attains the extremum twice
    x[nu + 3] = x[nu + 2]                                    # ... and row 11's doubled entry ties with nothing else
    d = rng.standard_normal((n, F)).astype(np.float32)
    base = rng.standard_normal((n, F)).astype(np.float32)
    src, tgt = sref.with_self_loops(m.col, m.row, n, self_loop)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    agg_t = sref.torch_aggregate(xt, torch.as_tensor(src), torch.as_tensor(tgt), n, op)
    (agg_t * torch.tensor(d.astype(np.float64))).sum().backward()
    want = xt.grad.numpy()
    xa = torch.zeros((n, 2 * F), device=DEV)
    xa[:, :F] = _t(x)
    cnt = torch.empty((n, F), device=DEV)
    hip.sage_aggregate(a.rowptr, a.colidx, xa[:, :F], xa[:, F:], op, cnt=cnt, self_loop=self_loop)
    assert float(cnt[9].min()) >= 2.0
    outs = []
    for _ in range(2):
        dx = _t(base).clone()
        hip.sage_aggregate_bwd(at.rowptr, at.colidx, xa[:, :F], xa[:, F:], cnt, _t(d), dx, self_loop=self_loop)
        outs.append(dx)
    got = outs[0].cpu().numpy().astype(np.float64) - base
    err = np.abs(got - want).max()
    print('reverse aggregate on A^T', F, op, self_loop, 'max err', err, 'max |g|', np.abs(want).max())
    assert err <= 2e-4 * np.abs(want).max() + 1e-10
    assert torch.equal(outs[0], outs[1])
    dx = _t(base).clone()                                    # the list itself in place of its transpose misses
    hip.sage_aggregate_bwd(a.rowptr, a.colidx, xa[:, :F], xa[:, F:], cnt, _t(d), dx, self_loop=self_loop)
    assert np.abs(dx.cpu().numpy().astype(np.float64) - base - want).max() > 2e-4 * np.abs(want).max() + 1e-10


# ---- 6. TwoStep / TwoWay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['GCN', 'GraphSage', 'GAT', 'LightGCN', 'DGCF'])
@pytest.mark.parametrize('layout,node', [('two_step', 'mean'), ('two_way', 'mean'), ('two_way', 'concatenation')])
def test_two_step_two_way_gradients_on_directed_graphs(hip, kind, layout, node):
    """test_twostep_twoway_gpu.py:test_gradients_match_autograd_oracle on helpers.kg_graph(symmetric=False): every stack transposes its
    own graph (the two-hop user-property graph is one-directional too)."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests.test_twostep_twoway_gpu import _flatten, _perturb
    engine.set_seed(5)
    g = helpers.kg_graph(n_users=60, n_items=45, n_props=30, n_ratings=900, n_links=120, seed=11, symmetric=False)
    if layout == 'two_step':
        adjs = (g['adj_ui'], g['adj_ip'])
        model = getattr(basic, 'BasicTS' + kind)(g['n_users'], g['n_items'], adjs, **dict(CFG, item_node=node))
        ow = helpers.two_step_to_oracle
    else:
        adjs = (g['adj_ui'], g['adj_ip'], g['adj_up'])
        model = getattr(basic, 'BasicTW' + kind)(g['n_users'], g['n_items'], adjs, **dict(CFG, user_item_node=node))
        ow = helpers.two_way_to_oracle
    assert all((sparse.csr_matrix(m) != sparse.csr_matrix(m).T).nnz for m in adjs)
    _perturb(model, 29)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    assert trainer.layout == layout and all(t.at is not t.seq.adj_matrix for t in trainer.tapes)
    loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    with torch.no_grad():
        e_inf = model.gnn(None)
        assert float((e_inf - trainer._propagation_forward()).abs().max()) <= 2e-6 * float(e_inf.abs().max())
    want_loss, want, _ = otrain.torch_model_grads(adjs, ow(model.gnn), helpers.basic_head_to_oracle(model.rs), g['u_ids'], g['i_ids'], y,
                                                  l2=1e-4, n_users=g['n_users'], n_items=g['n_items'])
    assert abs(loss - want_loss) < 1e-5
    _assert_grads(trainer, grads, _flatten(model, want, layout))


# ---- 7. dropout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls,extra', [('BasicGCN', dict(dropout=0.3)), ('BasicGAT', dict(dropout=0.2, dropout_rate=0.3))])
@pytest.mark.parametrize('name', ['ui', 'mixed'])
def test_gradients_with_dropout_on_a_directed_graph(hip, monkeypatch, cls, extra, name):
    """test_dropout_gpu.py:test_gradients_with_dropout_match_float64_autograd with its own helpers (the masks restated in numpy)."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests.test_dropout_gpu import _check_model, _flatten_single
    engine.set_seed(5)
    g = dr.graph(name)
    model = getattr(basic, cls)(g['adj'], **dict(CFG, **extra))
    helpers.randomize_biases(model, seed=6)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    _check_model(monkeypatch, model, trainer, g['adj'], helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs),
                 _flatten_single(model), g['u_ids'], g['i_ids'], y)


# ---- 8. Adam ---------------------------------------------------------------------------------------------------------------------
def test_adam_steps_on_a_directed_graph_match_the_oracle(hip):
    """test_training_gpu.py:test_adam_steps_match_oracle on ui."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(8)
    g = dr.tiny('ui', seed=3)
    model = basic.BasicGCN(g['adj'], **CFG)
    helpers.randomize_biases(model, seed=1)
    y = np.random.default_rng(4).integers(0, 2, len(g['u_ids']))
    gnn, head = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
    gnn = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in gnn.items()}
    gnn['layers'] = [{k: v.astype(np.float64) for k, v in lw.items()} for lw in gnn['layers']]
    head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in net] for k, net in head.items()}
    state = {}
    trainer = training.Trainer(model)
    for t in range(1, 4):
        trainer.train_batch(g['u_ids'], g['i_ids'], y)
        _, og, _ = otrain.loss_and_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, l2=1e-4)

        def upd(key, w, gr):
            m, v = state.get(key, (np.zeros_like(w), np.zeros_like(w)))
            w2, m, v = otrain.adam_update(w, gr, m, v, t)
            state[key] = (m, v)
            return w2
        gnn['embeddings'] = upd('emb', gnn['embeddings'], og['gnn']['embeddings'])
        for k, lw in enumerate(gnn['layers']):
            for nm in ('kernel', 'bias'):
                lw[nm] = upd(('l', k, nm), lw[nm], og['gnn']['layers'][k][nm])
        for name in head:
            head[name] = [(upd((name, k, 'w'), w, og['head'][name][k][0]), upd((name, k, 'b'), b, og['head'][name][k][1]))
                          for k, (w, b) in enumerate(head[name])]
    got = helpers.gnn_to_oracle(model.gnn)
    assert np.abs(got['embeddings'] - gnn['embeddings']).max() < 2e-5
    assert np.abs(got['layers'][0]['kernel'] - gnn['layers'][0]['kernel']).max() < 2e-5
    gh = helpers.basic_head_to_oracle(model.rs)
    assert np.abs(gh['clf'][-1][0] - head['clf'][-1][0]).max() < 2e-5


# ---- 9. replay -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['BasicGCN', 'BasicGraphSage', 'BasicGAT', 'BasicLightGCN', 'BasicDGCF'])
def test_graph_replayed_batches_equal_eager_batches_on_a_directed_graph(hip, cls):
    """test_training_gpu.py:test_graph_replayed_batches_equal_eager_batches on `mixed`: the transposed image exists before the capture."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = dr.mixed()
    rng = np.random.default_rng(4)
    batches = [(g['u_ids'][k * 64:(k + 1) * 64], g['i_ids'][k * 64:(k + 1) * 64], rng.integers(0, 2, 64)) for k in range(4)]
    models = []
    for _ in range(2):
        engine.set_seed(8)
        m = getattr(basic, cls)(g['adj'], **CFG)
        helpers.randomize_biases(m, seed=1)
        models.append(m)
    eager, graphed = training.Trainer(models[0]), training.Trainer(models[1])
    assert graphed.tapes[0].at is not graphed.tapes[0].seq.adj_matrix
    loss_eager = 0.0
    for epoch in range(3):
        for u, i, y in batches:
            loss_eager += eager.train_batch(u, i, y) * len(y)
            graphed.train_batch_graphed(u, i, y)
    assert graphed._g is not None and 'graph' in graphed._g and graphed.t == eager.t == 12
    assert abs(graphed.pop_loss_sum() - loss_eager) < 1e-3 * abs(loss_eager)
    for pa, pb in zip(models[0].parameters(), models[1].parameters()):
        assert torch.allclose(pa, pb, rtol=1e-4, atol=1e-6), tuple(pa.shape)


# ---- 10. BPR ---------------------------------------------------------------------------------------------------------------------
def _directed_sample_sequence(batch_size):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphPosNegSample
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    g = helpers.tiny_graph(n_users=70, n_items=50, n_ratings=1400, seed=3)
    r = g['ratings'].copy()
    first = np.unique(r[:, 0], return_index=True)[1]
    r[first, 2] = 1
    adj = build_adjacency_matrix(r, g['users'], g['items'], type_adjacency='binary', symmetric_adjacency=False)
    assert (sparse.csr_matrix(adj) != sparse.csr_matrix(adj).T).nnz
    return UserItemGraphPosNegSample(r, g['users'], g['items'], adj, batch_size=batch_size, seed=42)


@pytest.mark.parametrize('cls', ['BasicGCN', 'BasicGAT'])
def test_bpr_on_the_directed_binary_graph(hip, cls):
    """test_bpr_gpu.py:test_bpr_gradients_match_autograd on the un-symmetrised 'binary' graph, then one epoch of fit()."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests.test_bpr_gpu import _bpr64, _targets_for
    from tests.test_training_gpu import _flatten_oracle_grads
    seq = _directed_sample_sequence(255)
    engine.set_seed(5)
    model = getattr(basic, cls)(seq.adj_matrix, **CFG)
    helpers.randomize_biases(model, seed=6)
    model.compile(loss=BPRLoss(), optimizer=Adam(learning_rate=1e-3))
    (u, i), y = seq.device_batch(0)                                   # the first batch of the epoch
    trainer = training.Trainer(model)
    loss, grads = trainer.loss_and_grads(u, i, y)
    gnn, head = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
    _, _, p = otrain.torch_model_grads(seq.adj_matrix, gnn, head, u, i, y, l2=1e-4)
    want_data, dz = _bpr64(p)
    c = dz / (p * (1 - p))
    bce_loss, want, _ = otrain.torch_model_grads(seq.adj_matrix, gnn, head, u, i, _targets_for(p, c), l2=1e-4)
    yt, pc = _targets_for(p, c), np.clip(p, 1e-7, 1 - 1e-7)
    l2_part = bce_loss - float(-np.mean(yt * np.log(pc + 1e-7) + (1 - yt) * np.log(1 - pc + 1e-7)))
    assert abs(loss - (want_data + l2_part)) < 1e-5
    flat = _flatten_oracle_grads(model, want)
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)
        assert np.abs(got - gw).max() <= 2e-4 * np.abs(gw).max() + 2e-6 * np.abs(dz).sum(), tuple(prm.shape)
    model._trainer = trainer
    hist = model.fit(seq, epochs=1, verbose=False)['loss']
    assert len(hist) == 1 and np.isfinite(hist[0]) and 0.0 < hist[0] < 1.0


# ---- 11. end to end --------------------------------------------------------------------------------------------------------------
def test_fit_learns_a_separable_task_on_the_directed_graph(hip):
    """test_training_gpu.py:test_fit_learns_a_separable_task on its un-symmetrised graph, same thresholds."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(11)
    g = dr.tiny('ui', n_users=100, n_items=80, n_ratings=4000, seed=5)
    model = basic.BasicGCN(g['adj'], **dict(CFG, l2_regularizer=1e-6))
    model.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=0.01), metrics=['accuracy'])
    seq = UserItemGraph(g['ratings'], g['users'], g['items'], g['adj'], batch_size=512, shuffle=True)
    before = model.evaluate(seq)
    hist = model.fit(seq, epochs=12, verbose=False)
    after = model.evaluate(seq)
    assert hist['loss'][-1] < hist['loss'][0] - 0.02
    assert after[0] < before[0] and after[1] > max(before[1], 0.6)


def test_experiment_with_symmetric_adjacency_false_runs_to_its_metrics(hip, tmp_path, monkeypatch):
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
    cfg['dataset']['symmetric_adjacency'] = False
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    small = {'embedding_dim': [8], 'n_hiddens': [[8, 8]], 'n_layers': [2], 'dense_units': [[24, 24]], 'clf_units': [[48, 48]]}
    grid = {'grid': {'directed': {'model': dict(small, name=['basic.BasicGCN', 'basic.BasicGAT']),
                                  'dataset': {'load_function_name': ['load_user_item_graph']}}}}
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump(grid))
    monkeypatch.chdir(tmp_path)
    seen = []
    from deep_cbrs_amar_renaissance_amd import training
    real = training._StackTape.__init__

    def spy(self, seq):
        real(self, seq)
        seen.append(self.at is not seq.adj_matrix)
    monkeypatch.setattr(training._StackTape, '__init__', spy)
    run_log = setup_mlflow('directed', str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log)
    assert len(multi.experiments) == 2
    results = multi.run()
    assert len(results) == 2 and seen == [True, True]                # both models trained on a graph that is not its own transpose
    for metrics in results.values():
        assert metrics is not None and list(metrics.index) == ['precision_at', 'recall_at', 'f1_at']
        assert ((metrics.values >= 0) & (metrics.values <= 1)).all()
    assert len(glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'artifacts' / 'predictions' / 'top_5' / 'results.tsv'))) == 2


# ---- 12. symmetric graphs untouched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['BasicGCN', 'BasicGraphSage', 'BasicGAT', 'BasicLightGCN', 'BasicDGCF'])
def test_a_symmetric_graph_launches_no_transpose(hip, cls, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import capi, engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    calls = []
    real = capi.csr_transpose
    monkeypatch.setattr(capi, 'csr_transpose', lambda *a, **k: calls.append(1) or real(*a, **k))
    engine.set_seed(5)
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9, n_props=30, n_links=90)
    model = getattr(basic, cls)(g['adj'], **CFG)
    trainer = training.Trainer(model)
    tape = trainer.tapes[0]
    assert tape.at is tape.seq.adj_matrix and not calls
    trainer.loss_and_grads(g['u_ids'], g['i_ids'], np.random.default_rng(2).integers(0, 2, len(g['u_ids'])))
    assert not calls
    # ... and a directed one launches exactly one per stack
    d = getattr(basic, cls)(dr.mixed()['adj'], **CFG)
    training.Trainer(d)
    training.Trainer(d)                                              # cached on the graph
    assert len(calls) == 1

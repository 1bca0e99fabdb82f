"""GPU: GAT with several attention heads (amar_rowwise_xw_heads_f32, amar_gat_heads_f32, amar_gat_heads_bwd_f32) against
tests/gat_heads_ref.py, from the entry points up to fit() (pytest -m gpu).

Bars: the forward is held to the single-head kernel test's `rel_err < 1e-5` (test_kernels_gpu.py::test_gat_layer); the reverse to
2e-4 of the largest reference magnitude (test_training_gpu.py::test_gat_bwd_kernel, ::test_gradients_match_autograd_oracle); model
scores to 1e-4 absolute, as the other model-level score tests."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml
from scipy import sparse

from tests import helpers, gat_heads_ref as ref
from tests.gat_heads_ladder_ref import NEW_SHAPES
from tests.helpers import rel_err
from tests.test_kernels_gpu import _rand_csr, _dev_csr, _t

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
# (heads, channels): 2 lanes per entry; 6 padded to 8; 16, full; 16 as two heads of 8 quads; 16 as four of 4; 16 as sixteen of 1;
# then heads of 3 and of 6 quads: no power of two, so the sums over a head's lanes and the averaging gather take their indexed form
SHAPES = [(2, 4), (3, 8), (8, 8), (2, 32), (4, 16), (16, 4), (2, 12), (2, 24)]
SHAPES += NEW_SHAPES                                                 # 16 floats as two heads of 2 quads, as four of 1; 12 padded to 16


def _graph(seed, symmetric=False, n=350):
    """test_gat_layer's graph: 350 rows, average degree 8, duplicate entries, no diagonal, a tenth of the rows empty and one row of
    (up to) 700 entries: longer than a wavefront, and than 64 / LPN entries for every LPN.  symmetric: the multiset plus its transpose."""
    m = _rand_csr(n, 8, seed=seed, dup=True)
    r, c = m.row[m.row != m.col], m.col[m.row != m.col]
    if symmetric:
        # (every tenth node, the long row's excepted, loses its entries in both directions: the transpose would fill the empty rows)
        iso = np.arange(n) % 10 == 3
        iso[np.bincount(r, minlength=n).argmax()] = False
        r, c = r[~iso[r] & ~iso[c]], c[~iso[r] & ~iso[c]]
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
    m = sparse.coo_matrix((np.ones(len(r), dtype=np.float32), (r, c)), shape=(n, n))
    a = _dev_csr(m, with_values=False, drop_diagonal=True)
    deg = np.diff(a.rowptr.cpu().numpy())
    assert deg.max() > 64 and (deg == 0).any()
    return m, a


def _weights(rng, heads, c, concat, scale=1.0):
    a_s = (rng.uniform(-1, 1, (c, heads, 1)) * scale).astype(np.float32)
    a_n = (rng.uniform(-1, 1, (c, heads, 1)) * scale).astype(np.float32)
    return a_s, a_n, rng.uniform(-0.1, 0.1, heads * c if concat else c).astype(np.float32)


@pytest.mark.parametrize('heads,c', SHAPES)
@pytest.mark.parametrize('concat', [True, False])
@pytest.mark.parametrize('self_loop', [True, False])
def test_forward_entries(hip, heads, c, concat, self_loop):
    n, f, hc = 350, 8, heads * c
    m, a = _graph(seed=hc + heads)
    rng = np.random.default_rng(hc)
    x = rng.standard_normal((n, f)).astype(np.float32)
    w = rng.uniform(-0.6, 0.6, (f, heads, c)).astype(np.float32)
    a_s, a_n, b = _weights(rng, heads, c, concat)
    # Hd and Y are column slices of wider buffers, as in the stack's `cat`
    width = hc if concat else c
    hbuf, ybuf = torch.full((n, hc + 8), 3.0, device=DEV), torch.full((n, width + 12), -7.0, device=DEV)
    hd, y = hbuf[:, 4:4 + hc], ybuf[:, 8:8 + width]
    s = torch.empty((n, 2 * heads), device=DEV)
    hip.rowwise_xw_heads(_t(x), _t(w), hd, _t(a_s), _t(a_n), s)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    hd64 = (x64 @ w64.reshape(f, hc)).reshape(n, heads, c)
    assert rel_err(hd.cpu().numpy(), hd64.reshape(n, hc)) < 2e-6
    s64 = np.concatenate([np.einsum('nhc,ch->nh', hd64, a_s[:, :, 0].astype(np.float64)),
                          np.einsum('nhc,ch->nh', hd64, a_n[:, :, 0].astype(np.float64))], axis=1)
    assert rel_err(s.cpu().numpy(), s64) < 2e-6                       # [n, 2H]: the heads' self scalars, then their neighbour scalars
    tape = torch.empty((n, hc), device=DEV)
    hip.gat_heads(a.rowptr, a.colidx, hd, heads, s, _t(b), y, concat=concat, self_loop=self_loop, out_tape=tape)
    want = ref.gat_heads_conv_np(x64, m.col, m.row, w64, a_s.astype(np.float64), a_n.astype(np.float64), b.astype(np.float64), concat, self_loop)
    got, whole = y.cpu().numpy(), ybuf.cpu().numpy()
    err = rel_err(got, want)
    print('gat_heads', heads, c, concat, self_loop, 'rel_err', err)
    assert err < 1e-5
    assert np.all(whole[:, :8] == -7.0) and np.all(whole[:, 8 + width:] == -7.0) and np.all(hbuf.cpu().numpy()[:, :4] == 3.0), "wrote outside its slice"
    empty = np.diff(a.rowptr.cpu().numpy()) == 0
    if not self_loop:
        assert np.array_equal(got[empty], np.broadcast_to(np.maximum(b, 0), got[empty].shape))        # nothing to attend to: ReLU(bias)
    # the tape holds the heads' outputs before joining and bias
    out = tape.cpu().numpy().astype(np.float64).reshape(n, heads, c)
    joined = out.reshape(n, hc) if concat else out.mean(1)
    assert np.abs(np.maximum(joined + b, 0) - got).max() < 1e-6
    if concat:
        # every head's column block against the single-head kernel on that head's slice and scalars
        for h in range(heads):
            yh = torch.empty((n, c), device=DEV)
            hip.gat_layer(a.rowptr, a.colidx, hd[:, h * c:(h + 1) * c], s[:, h].contiguous(), s[:, heads + h].contiguous(), _t(b[h * c:(h + 1) * c]), yh,
                          self_loop=self_loop)
            assert rel_err(got[:, h * c:(h + 1) * c], yh.cpu().numpy().astype(np.float64)) < 1e-5, h
    again = torch.empty((n, width), device=DEV)
    hip.gat_heads(a.rowptr, a.colidx, hd, heads, s, _t(b), again, concat=concat, self_loop=self_loop)
    assert torch.equal(again, y.contiguous())                        # fixed summation order; the tape is optional


def test_entries_refuse_unsupported_shapes(hip):
    _, a = _graph(seed=1)
    n = 350
    for heads, c in ((9, 8), (2, 6), (3, 24)):
        hc = heads * c
        hd, s, b, y = (torch.zeros((n, hc), device=DEV), torch.zeros((n, 2 * heads), device=DEV), torch.zeros(hc, device=DEV),
                       torch.zeros((n, hc), device=DEV))
        with pytest.raises(hip.AmarError, match='not supported'):
            hip.gat_heads(a.rowptr, a.colidx, hd, heads, s, b, y)
        with pytest.raises(hip.AmarError, match='not supported'):
            hip.gat_heads_bwd(a.rowptr, a.colidx, hd, heads, s, y, y, b, torch.zeros((c, heads, 1), device=DEV), torch.zeros((c, heads, 1), device=DEV))
        with pytest.raises(hip.AmarError, match='not supported'):
            hip.rowwise_xw_heads(torch.zeros((n, 8), device=DEV), torch.zeros((8, heads, c), device=DEV), hd, torch.zeros((c, heads, 1), device=DEV),
                                 torch.zeros((c, heads, 1), device=DEV), s)
    with pytest.raises(ValueError):                                  # the averaging form needs the forward's tape
        hip.gat_heads_bwd(a.rowptr, a.colidx, torch.zeros((n, 16), device=DEV), 2, torch.zeros((n, 4), device=DEV), torch.zeros((n, 8), device=DEV),
                          torch.zeros((n, 8), device=DEV), torch.zeros(8, device=DEV), torch.zeros((8, 2, 1), device=DEV),
                          torch.zeros((8, 2, 1), device=DEV), concat=False)


@pytest.mark.parametrize('heads,c', SHAPES)
@pytest.mark.parametrize('concat', [True, False])
@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('self_loop', [True, False])
def test_reverse_entry(hip, heads, c, concat, symmetric, self_loop):
    """amar_gat_heads_bwd_f32 against float64 autograd of the restatement on the identical float32 inputs: dHd, ds, dt, dout; a
    symmetric multiset through one structure, a directed one through the structure and its stable transpose; two runs, equal bits."""
    n, hc = 350, heads * c
    _, a = _graph(seed=hc + 3 * heads, symmetric=symmetric)
    at = a.transposed()
    assert (at is a) == symmetric
    rng = np.random.default_rng(hc + 1)
    hd = (rng.standard_normal((n, hc)) * 0.7).astype(np.float32)
    a_s, a_n, b = _weights(rng, heads, c, concat, scale=0.5)
    width = hc if concat else c
    dy = rng.standard_normal((n, width)).astype(np.float32)
    rowptr, colidx = a.rowptr.cpu().numpy(), a.colidx.cpu().numpy()
    src, tgt = ref.edges(colidx.astype(np.int64), np.repeat(np.arange(n), np.diff(rowptr)), n, self_loop)
    ht = torch.tensor(hd.astype(np.float64), requires_grad=True)
    keep = {}
    y64 = ref.torch_gat_heads(ht.view(n, heads, c), torch.tensor(a_s.astype(np.float64)), torch.tensor(a_n.astype(np.float64)),
                              torch.tensor(b.astype(np.float64)), src, tgt, concat, keep=keep)
    (y64 * torch.tensor(dy.astype(np.float64))).sum().backward()
    # device: the scalars from the same Hd (an identity projection), the forward with its tape, the reverse
    hdev, s = torch.empty((n, hc), device=DEV), torch.empty((n, 2 * heads), device=DEV)
    hip.rowwise_xw_heads(_t(hd), torch.eye(hc, device=DEV).view(hc, heads, c).contiguous(), hdev, _t(a_s), _t(a_n), s)
    assert torch.equal(hdev, _t(hd))
    y, tape = torch.empty((n, width), device=DEV), torch.empty((n, hc), device=DEV)
    hip.gat_heads(a.rowptr, a.colidx, hdev, heads, s, _t(b), y, concat=concat, self_loop=self_loop, out_tape=tape)
    assert rel_err(y.cpu().numpy(), y64.detach().numpy()) < 1e-5
    run = lambda: hip.gat_heads_bwd(a.rowptr, a.colidx, hdev, heads, s, y, _t(dy), _t(b), _t(a_s), _t(a_n), concat=concat, self_loop=self_loop,   # noqa: E731
                                    out_tape=None if concat else tape, transposed=None if symmetric else (at.rowptr, at.colidx))
    dout, ds, dh = run()
    assert np.array_equal(dout.cpu().numpy(), dy * (y.cpu().numpy() > 0))
    want_h, want_s, want_t = ht.grad.numpy(), keep['s'].grad.numpy(), keep['t'].grad.numpy()
    err_h = np.abs(dh.cpu().numpy() - want_h).max()
    got_s = ds.cpu().numpy().astype(np.float64)
    err_s, err_t = np.abs(got_s[:, :heads] - want_s).max(), np.abs(got_s[:, heads:] - want_t).max()
    scale = max(np.abs(want_s).max(), np.abs(want_t).max())
    print('gat_heads_bwd', heads, c, concat, symmetric, self_loop, 'dHd', err_h, 'of', np.abs(want_h).max(), 'ds', err_s, 'dt', err_t, 'of', scale)
    assert err_h <= 2e-4 * np.abs(want_h).max()
    assert err_s <= 2e-4 * scale and err_t <= 2e-4 * scale
    assert all(torch.equal(p, q) for p, q in zip((dout, ds, dh), run()))                                   # no float atomics


# ---- models ----------------------------------------------------------------------------------------------------------------------
def _model(g, cls='BasicGAT', seed=5, **extra):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(seed)
    model = getattr(basic, cls)(g['adj'], **dict(CFG, **extra))
    helpers.randomize_biases(model, seed=6)
    return model


HEAD_MODES = [dict(attn_heads=2, concat_heads=True), dict(attn_heads=4, concat_heads=False)]


@pytest.mark.parametrize('extra', HEAD_MODES)
@pytest.mark.parametrize('graph', ['ui', 'uip'])
def test_basic_gat_scores_and_gradients(hip, extra, graph):
    """BasicGAT scores and every parameter gradient of one BCE step against autograd of the restatement."""
    from deep_cbrs_amar_renaissance_amd import training
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9, n_props=30 if graph == 'uip' else 0, n_links=90 if graph == 'uip' else 0)
    model = _model(g, **extra)
    got = model((g['u_ids'], g['i_ids'])).cpu().numpy().reshape(-1)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    want_loss, want, want_p = ref.torch_model_grads(g['adj'], ref.gnn_to_ref(model.gnn), helpers.basic_head_to_oracle(model.rs), g['u_ids'], g['i_ids'],
                                                    y, l2=1e-4)
    assert got.shape == want_p.shape == (len(g['u_ids']),) and np.abs(got - want_p).max() < 1e-4
    trainer = training.Trainer(model)
    loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    with torch.no_grad():
        e_inf = model.gnn.gnn_layers(None)
        e_trn = trainer._propagation_forward()
    assert e_inf.shape[1] == (40 if extra['concat_heads'] else 24) and float((e_inf - e_trn).abs().max()) < 2e-6
    assert abs(loss - want_loss) < 1e-5
    flat = ref.flatten_grads(model, want)
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got_g = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got_g += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)      # the trainer folds the L2 term into the optimizer kernel
        err = np.abs(got_g - gw).max()
        print('gradient', extra, graph, tuple(prm.shape), 'err', err, 'max |g|', np.abs(gw).max())
        assert err <= 2e-4 * np.abs(gw).max() + 1e-10, tuple(prm.shape)


def test_gradients_on_a_directed_graph(hip):
    """A directed user-item graph: the reverse pass walks A^T (the tape's stable transpose) for the sources."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9)
    adj = build_adjacency_matrix(g['ratings'], g['users'], g['items'], symmetric_adjacency=False)
    assert (adj != adj.T).nnz
    model = _model(dict(g, adj=adj), attn_heads=2)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    trainer = training.Trainer(model)
    assert trainer.tapes[0].at is not model.gnn.gnn_layers.adj_matrix
    loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    want_loss, want, _ = ref.torch_model_grads(adj, ref.gnn_to_ref(model.gnn), helpers.basic_head_to_oracle(model.rs), g['u_ids'], g['i_ids'], y, l2=1e-4)
    assert abs(loss - want_loss) < 1e-5
    for prm, gw in ref.flatten_grads(model, want).items():
        got_g = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64) + 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)
        assert np.abs(got_g - gw).max() <= 2e-4 * np.abs(gw).max() + 1e-10, tuple(prm.shape)


def test_two_step_scores_and_gradients(hip):
    """BasicTSGAT with the 'concatenation' hand-over: step one hands over 8 + 16 + 16 columns, step two's layers are 2 x 24 wide."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = helpers.kg_graph(seed=3)
    engine.set_seed(5)
    model = basic.BasicTSGAT(g['n_users'], g['n_items'], (g['adj_ui'], g['adj_ip']), attn_heads=2, **dict(CFG, item_node='concatenation'))
    model((g['u_ids'], g['i_ids']))
    helpers.randomize_biases(model, seed=4)
    got = model((g['u_ids'], g['i_ids'])).cpu().numpy().reshape(-1)
    assert model.gnn.step_two_gnn_layers.layer_widths() == [40, 48, 48]
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    want_loss, want, want_p = ref.torch_model_grads((g['adj_ui'], g['adj_ip']), ref.gnn_to_ref(model.gnn), helpers.basic_head_to_oracle(model.rs),
                                                    g['u_ids'], g['i_ids'], y, l2=1e-4, n_users=g['n_users'], n_items=g['n_items'])
    assert got.shape == want_p.shape and np.abs(got - want_p).max() < 1e-4
    trainer = training.Trainer(model)
    loss, grads = trainer.loss_and_grads(g['u_ids'], g['i_ids'], y)
    assert abs(loss - want_loss) < 1e-5
    flat = ref.flatten_grads(model, want)
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got_g = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64) + 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)
        assert np.abs(got_g - gw).max() <= 2e-4 * np.abs(gw).max() + 1e-10, tuple(prm.shape)


def test_hybrid_bert_gat_scores(hip):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9)
    bert = synthetic.entity_embeddings(140, 32, 'bert')
    engine.set_seed(5)
    model = hybrid.HybridBertGAT(g['adj'], attn_heads=2, **dict(CFG, dense_units=[[24, 24], [16, 8], [16, 16]], clf_units=[16, 16], feature_based=True))
    model.rs.build_head(model.gnn.output_dim(), 32)
    helpers.randomize_biases(model, seed=17)
    u, i = g['u_ids'], g['i_ids']
    got = model((u, i, bert[u], bert[i])).cpu().numpy().reshape(-1)
    _, _, want = ref.torch_model_grads(g['adj'], ref.gnn_to_ref(model.gnn), helpers.hybrid_head_to_oracle(model.rs), u, i, np.zeros(len(u)),
                                       bert=(bert[u], bert[i]))
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-4


@pytest.mark.parametrize('extra', HEAD_MODES)
def test_graph_replayed_batches_equal_eager_batches(hip, extra):
    """The step's body run eagerly at every batch on one trainer and replayed from the captured hipGraph on the other: the weights
    agree bit for bit (the pattern of test_sage_aggregate_gpu.py)."""
    from deep_cbrs_amar_renaissance_amd import training
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=3)
    rng = np.random.default_rng(4)
    batches = [(g['u_ids'][k * 64:(k + 1) * 64], g['i_ids'][k * 64:(k + 1) * 64], rng.integers(0, 2, 64)) for k in range(4)]
    models = [_model(g, seed=8, **extra) for _ in range(2)]
    eager, graphed = training.Trainer(models[0]), training.Trainer(models[1])
    for epoch in range(3):
        for u, i, y in batches:
            eager.train_batch_graphed(u, i, y, graph=False)
            graphed.train_batch_graphed(u, i, y)
    assert graphed._g is not None and graphed.t == eager.t == 12
    assert abs(graphed.pop_loss_sum() - eager.pop_loss_sum()) < 1e-6
    for pa, pb in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(pa, pb), tuple(pa.shape)


def test_fit_refuses_attention_dropout_and_trains_with_stack_dropout(hip, monkeypatch):
    from tests.test_dropout_gpu import _bce_sequence, _bce_model
    g, seq = _bce_sequence()
    refused = _bce_model(g, 'BasicGAT', attn_heads=2, dropout_rate=0.3)                # builds and scores: inference ignores the rate
    assert np.isfinite(refused((g['u_ids'], g['i_ids'])).cpu().numpy()).all()
    with pytest.raises(NotImplementedError, match='attn_heads'):
        refused.fit(seq, epochs=1, verbose=False)
    models, hist = [], []
    for env in ('0', '1'):                                                             # eager, then replayed from the captured hipGraph
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = _bce_model(g, 'BasicGAT', attn_heads=2, dropout=0.2)
        hist.append(m.fit(seq, epochs=2, verbose=False)['loss'])
        models.append(m)
    assert models[1]._trainer._graphs and not models[0]._trainer._graphs
    assert hist[0] == hist[1] and np.isfinite(hist[0]).all()
    for pa, pb in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(pa, pb), tuple(pa.shape)


def test_one_head_is_the_unchanged_path(hip):
    """The key left out and attn_heads=1: bit-equal scores, and bit-equal weights after one training step."""
    from deep_cbrs_amar_renaissance_amd import training
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    plain, one = _model(g), _model(g, attn_heads=1, concat_heads=True)
    assert torch.equal(plain((g['u_ids'], g['i_ids'])), one((g['u_ids'], g['i_ids'])))
    for m in (plain, one):
        training.Trainer(m).train_batch(g['u_ids'], g['i_ids'], y)
    for (na, pa), (nb, pb) in zip(plain.named_parameters(), one.named_parameters()):
        assert na == nb and torch.equal(pa, pb), na
    averaged = _model(g, attn_heads=1, concat_heads=False)           # one head averaged is that head
    assert averaged.gnn.gnn_layers.layer_widths() == [8, 8, 8]
    assert torch.equal(_model(g)((g['u_ids'], g['i_ids'])), averaged((g['u_ids'], g['i_ids'])))


def test_recommend_and_weight_files_round_trip(hip, tmp_path):
    from tests.test_dropout_gpu import _bce_sequence, _bce_model
    g, seq = _bce_sequence()
    model = _bce_model(g, 'BasicGAT', attn_heads=4)
    model.fit(seq, epochs=1, verbose=False)
    users, items, scores = model.recommend(seq, k=5)
    assert np.asarray(items).shape == (len(np.asarray(users)), 5) and np.isfinite(np.asarray(scores)[:, 0]).all()
    path = str(tmp_path / 'weights')
    model.save_weights(path)
    other = _bce_model(g, 'BasicGAT', seed=9, attn_heads=4)
    other.load_weights(path)
    _, items2, scores2 = other.recommend(seq, k=5)
    assert np.array_equal(np.asarray(items), np.asarray(items2)) and np.array_equal(np.asarray(scores), np.asarray(scores2))


def test_experiment_with_four_heads_runs_to_its_metrics(hip, tmp_path, monkeypatch):
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
    grid = {'linear': {'gat-heads': {
        'model': {'name': 'basic.BasicGAT', 'attn_heads': 4, 'embedding_dim': 8, 'n_hiddens': [8, 8], 'dense_units': [24, 24], 'clf_units': [48, 48]},
        'dataset': {'load_function_name': 'load_user_item_graph'}}}}
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump(grid))
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('heads', str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log)
    assert len(multi.experiments) == 1
    results = multi.run()
    (metrics,) = results.values()
    assert metrics is not None and list(metrics.index) == ['precision_at', 'recall_at', 'f1_at']
    assert ((metrics.values >= 0) & (metrics.values <= 1)).all()
    assert glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'artifacts' / 'predictions' / 'top_5' / 'results.tsv'))

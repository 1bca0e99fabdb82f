"""GPU: the compiled loss and metrics on the device — amar_loss_grad_f32 per loss against the float64 restatement (kinks, strided p,
lane / wavefront / workgroup / grid-stride sizes), its cross-entropy code against amar_bce_grad_f32 bit for bit, the metric counters
against their numpy statement, the Trainer's gradients under every loss against autograd, fit() replayed = eager, metrics of fit() =
metrics of evaluate(), the head-only and hybrid trainers, and the experiment end to end (pytest -m gpu)."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import train as otrain
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
SIZES = [1, 63, 64, 65, 257, 1025]                                    # lane, wavefront, workgroup (256) and grid-stride edges
LOSSES = ['binary_crossentropy', {'name': 'binary_crossentropy', 'label_smoothing': 0.1}, 'mse', 'mae', 'hinge', 'squared_hinge',
          {'name': 'huber', 'delta': 0.25}, 'log_cosh', 'poisson', 'binary_focal_crossentropy',
          {'name': 'binary_focal_crossentropy', 'gamma': 3.0, 'apply_class_balancing': True, 'alpha': 0.25}]
_ids = lambda v: v if isinstance(v, str) else '-'.join(str(x) for x in v.values())   # noqa: E731


def _resolve(loss):
    from deep_cbrs_amar_renaissance_amd.utilities.losses import resolve_loss
    return resolve_loss(loss)[:2]


def _kink_inputs(B, seed):
    """Random (p, y) with the kinks planted in front: p = y, s p = 1 (p = 1, y = 1), p in {0, 1e-7, 1 - 1e-7, 1} for both labels,
    |e| = 0.25 (Huber's delta in LOSSES) from either side."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, B).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    edge = [np.float32(0), np.float32(1e-7), np.float32(1) - np.float32(1e-7), np.float32(1)]
    planted = [(v, lab) for lab in (1.0, 0.0) for v in edge] + [(np.float32(0.25), 0.0), (np.float32(0.75), 1.0), (np.float32(0.5), 1.0)]
    planted = [(np.float32(1), 1.0)] + planted[1:] + planted[:1]     # p = y = 1 first, so that B = 1 holds a kink too
    for j, (v, lab) in enumerate(planted[:B]):
        p[j], y[j] = v, lab
    return p, y


def _device_p(p, strided):
    if not strided:
        return torch.from_numpy(p).to(DEV)
    wide = torch.full((len(p), 3), 7.0, device=DEV)
    wide[:, 1] = torch.from_numpy(p).to(DEV)
    return wide[:, 1:2]                                              # a [B, 1] column with ldp = 3


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('B', SIZES)
@pytest.mark.parametrize('loss', LOSSES, ids=_ids)
def test_loss_grad_kernel_against_float64(hip, loss, B, strided):
    """Tolerances: tests/test_bpr_gpu.py:test_bpr_grad_kernel's, element by element (terms rtol 2e-6 / atol 1e-7, dz rtol 2e-5 /
    atol 1e-9, mean loss 1e-5), the tighter of the two sets in use for this comparison; test_bce_grad_clip_points' 1e-5 of the
    largest magnitude follows from them wherever a batch holds more than its planted zeros."""
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    code, hyper = _resolve(loss)
    p, y = _kink_inputs(B, seed=B + 7 * code)
    dz = torch.full((B, 1), float('nan'), device=DEV)
    terms = torch.full((B,), float('nan'), device=DEV)
    hip.loss_grad(code, hyper, _device_p(p, strided), torch.from_numpy(y).to(DEV), dz, terms)
    p64 = p.astype(np.float64)
    want_t = L.loss_terms(code, hyper, y, p64, f32_constants=True)
    through = p64 * (1.0 - p64)
    with np.errstate(invalid='ignore'):
        want_dz = np.where(through == 0, 0.0, L.loss_dp(code, hyper, y, p64, f32_constants=True) * through / B)
    gt, gd = terms.cpu().numpy().astype(np.float64), dz.cpu().numpy().reshape(-1).astype(np.float64)
    assert np.isfinite(gt).all() and np.isfinite(gd).all()
    np.testing.assert_allclose(gt, want_t, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(gd, want_dz, rtol=2e-5, atol=1e-9)
    if B > 1:
        assert helpers.rel_err(gt, want_t) < 1e-5 and helpers.rel_err(gd, want_dz) < 1e-5
    mean64 = float(want_t.mean())
    assert abs(gt.sum() / B - mean64) <= 1e-5 * abs(mean64) + 1e-7     # sum(terms) = B x batch loss (1e-7: the terms' own floor)
    # exactly 0 where the loss is flat or clipped, and where the sigmoid passes nothing back
    e32 = np.float32(1e-7)
    assert (gd[(p == 0) | (p == 1)] == 0).all()
    if code == L.BCE:
        assert (gd[(p < e32) | (p > np.float32(1) - e32)] == 0).all()
    if code in (L.HINGE, L.SQUARED_HINGE):
        beyond = (2 * y - 1) * p64 >= 1
        assert (gd[beyond] == 0).all() and (gt[beyond] == 0).all()
    if code == L.MAE:
        assert (gd[p == y] == 0).all()


@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('B', SIZES)
def test_cross_entropy_code_gives_the_bits_of_bce_grad(hip, B, strided):
    p, y = _kink_inputs(B, seed=B)
    pd, yd = _device_p(p, strided), torch.from_numpy(y).to(DEV)
    out = [(torch.full((B, 1), 3.0, device=DEV), torch.full((B,), 3.0, device=DEV)) for _ in range(3)]
    hip.bce_grad(pd, yd, *out[0])
    hip.loss_grad(hip.LOSS_BCE, (0.0, 0.0, 0.0, 0.0), pd, yd, *out[1])
    counters = torch.zeros(hip.LOSS_COUNTERS, dtype=torch.int64, device=DEV)
    hip.loss_grad(hip.LOSS_BCE, None, pd, yd, *out[2], counters=counters)      # (counting changes nothing in what is written)
    for dz, terms in out[1:]:
        assert torch.equal(dz, out[0][0]) and torch.equal(terms, out[0][1])


def _counter_inputs(B, seed):
    """Random (p, y); one p in eight is an exact AUC threshold float32(k / 199) or its float neighbour on either side."""
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import auc_thresholds
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, B).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    thr = auc_thresholds()
    for n, j in enumerate(range(0, B, 8)):
        t = thr[(37 * n + B) % len(thr)]
        p[j] = (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)))[n % 3]
    if B > 16:
        p[1], p[2], p[3], p[4] = 0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1))
    return p, y


@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('B', SIZES)
def test_metric_counters_equal_the_numpy_statement(hip, B, strided):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import metric_counters
    assert hip.loss_counters() == hip.LOSS_COUNTERS == 402
    p, y = _counter_inputs(B, seed=3 * B + 1)
    pd, yd = _device_p(p, strided), torch.from_numpy(y).to(DEV)
    dz, terms = torch.empty((B, 1), device=DEV), torch.empty(B, device=DEV)
    want = metric_counters(p, y)
    assert want[:4].sum() == B and want[4:].sum() == B
    counters = torch.zeros(hip.LOSS_COUNTERS, dtype=torch.int64, device=DEV)
    hip.loss_grad(hip.LOSS_MSE, None, pd, yd, dz, terms, counters=counters)
    assert np.array_equal(counters.cpu().numpy(), want)
    hip.loss_grad(hip.LOSS_HINGE, None, pd, yd, dz, terms, counters=counters)   # a second launch adds: every cell doubles
    assert np.array_equal(counters.cpu().numpy(), 2 * want)
    again = torch.zeros_like(counters)                                # two runs, the same bits
    hip.loss_grad(hip.LOSS_MSE, None, pd, yd, dz, terms, counters=again)
    assert np.array_equal(again.cpu().numpy(), want)
    before = counters.clone()                                         # a null pointer writes nothing
    hip.loss_grad(hip.LOSS_MSE, None, pd, yd, dz, terms)
    assert torch.equal(counters, before)


def test_loss_grad_refuses_bad_arguments(hip):
    p, y = torch.rand(8, device=DEV), torch.zeros(8, device=DEV)
    dz, terms = torch.empty((8, 1), device=DEV), torch.empty(8, device=DEV)
    with pytest.raises(ValueError):
        hip.loss_grad(99, None, p, y, dz, terms)
    with pytest.raises(ValueError):
        hip.loss_grad(hip.LOSS_MSE, None, p, y[:7], dz, terms)
    with pytest.raises(ValueError):
        hip.loss_grad(hip.LOSS_MSE, None, p, y, dz, terms, counters=torch.zeros(10, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        hip.loss_grad(hip.LOSS_BCE, (2.0, 0.0, 0.0, 0.0), p, y, dz, terms)      # label_smoothing outside [0, 1]


# ---- the Trainer's gradients under every loss ----------------------------------------------------------------------------------------

def _torch_mean_loss(code, hyper, p, y):
    """The mean loss written in torch (float64) for autograd: Keras' formulas, independent of the numpy restatement's gradients."""
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    ls, shape, alpha, balance = hyper
    e, s, eps = p - y, 2 * y - 1, 1e-7

    def bce(t):
        pc = torch.clamp(p, eps, 1 - eps)
        return -(t * torch.log(pc + eps) + (1 - t) * torch.log(1 - pc + eps))
    if code == L.BCE:
        terms = bce(y * (1 - ls) + 0.5 * ls)
    elif code == L.MSE:
        terms = e * e
    elif code == L.MAE:
        terms = e.abs()
    elif code == L.HINGE:
        terms = torch.clamp(1 - s * p, min=0)
    elif code == L.SQUARED_HINGE:
        terms = torch.clamp(1 - s * p, min=0) ** 2
    elif code == L.HUBER:
        terms = torch.where(e.abs() <= shape, 0.5 * e * e, shape * e.abs() - 0.5 * shape * shape)
    elif code == L.LOG_COSH:
        terms = e + torch.nn.functional.softplus(-2 * e) - np.log(2.0)
    elif code == L.POISSON:
        terms = p - y * torch.log(p + eps)
    else:
        t = y * (1 - ls) + 0.5 * ls
        weight = t * alpha + (1 - t) * (1 - alpha) if balance else 1.0
        terms = weight * (1 - (t * p + (1 - t) * (1 - p))) ** shape * bce(t)
    return terms.mean()


@pytest.fixture(scope='module')
def tiny_model():
    """The graph and sizes of tests/test_bpr_gpu.py:test_bpr_gradients_match_autograd, one batch, and the oracle's probabilities."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests.test_bpr_gpu import _sample_sequence
    seq = _sample_sequence(batch_size=255)
    engine.set_seed(5)
    model = basic.BasicGCN(seq.adj_matrix, **CFG)
    helpers.randomize_biases(model, seed=6)
    (u, i), y = seq.device_batch(3)
    gnn, head = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
    _, _, p = otrain.torch_model_grads(seq.adj_matrix, gnn, head, u, i, y, l2=1e-4)
    return {'seq': seq, 'model': model, 'u': u, 'i': i, 'y': np.asarray(y, dtype=np.float64), 'gnn': gnn, 'head': head,
            'p': np.asarray(p, dtype=np.float64).reshape(-1)}


@pytest.mark.parametrize('loss', LOSSES, ids=_ids)
def test_trainer_gradients_match_autograd(hip, tiny_model, loss):
    """As test_bpr_gradients_match_autograd: the oracle's autograd runs a cross-entropy whose targets give it the cotangent
    d(loss)/dp that torch autograd takes from the loss written in torch, so its gradients are autograd of that loss + the L2 terms."""
    from deep_cbrs_amar_renaissance_amd import training
    from tests.test_bpr_gpu import _targets_for
    from tests.test_training_gpu import _flatten_oracle_grads
    t = tiny_model
    model, p, y = t['model'], t['p'], t['y']
    code, hyper = _resolve(loss)
    model.compile(loss=loss, metrics=['accuracy', 'AUC'])
    trainer = training.Trainer(model)
    got_loss, grads = trainer.loss_and_grads(t['u'], t['i'], y)
    pt = torch.tensor(p, requires_grad=True)
    want_data = _torch_mean_loss(code, hyper, pt, torch.tensor(y))
    c = torch.autograd.grad(want_data, pt)[0].numpy()
    yt = _targets_for(p, c)
    bce_loss, want, _ = otrain.torch_model_grads(t['seq'].adj_matrix, t['gnn'], t['head'], t['u'], t['i'], yt, l2=1e-4)
    pc = np.clip(p, 1e-7, 1 - 1e-7)
    l2_part = bce_loss - float(-np.mean(yt * np.log(pc + 1e-7) + (1 - yt) * np.log(1 - pc + 1e-7)))
    assert abs(got_loss - (float(want_data) + l2_part)) < 1e-5
    flat = _flatten_oracle_grads(model, want)
    assert set(flat) == set(grads)
    dz = c * p * (1 - p)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)
        assert np.abs(got - gw).max() <= 2e-4 * np.abs(gw).max() + 2e-6 * np.abs(dz).sum(), tuple(prm.shape)


# ---- fit() and evaluate() -------------------------------------------------------------------------------------------------------------

def _sequence(n=1280, batch_size=128):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    g = helpers.tiny_graph(n_users=70, n_items=50, n_ratings=1400, seed=3)
    return g, UserItemGraph(g['ratings'][:n], g['users'], g['items'], g['adj'], batch_size=batch_size, shuffle=False)


def _model(g, loss, metrics=None, optimizer=None, seed=8, **extra):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(seed)
    model = basic.BasicGCN(g['adj'], **dict(CFG, **extra))
    helpers.randomize_biases(model, seed=1)
    model.compile(loss=loss, optimizer=optimizer or Adam(learning_rate=1e-3), metrics=metrics)
    model((g['u_ids'], g['i_ids']))
    return model


@pytest.mark.parametrize('loss', ['mse', {'name': 'binary_focal_crossentropy', 'gamma': 3.0}], ids=_ids)
def test_fit_replayed_equals_eager(hip, monkeypatch, loss):
    """AMAR_TRAIN_GRAPH=0 against the replayed graph: the same weights bit for bit and the same history, metrics included.  (A model
    that drops, as in the other tests of this statement: without dropout AMAR_TRAIN_GRAPH=0 steps through train_batch, whose Adam
    takes its step size from the host in float64 and agrees with the replayed one to rounding only.)"""
    g, seq = _sequence()
    models, hist = [], []
    for env in ('0', '1'):
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = _model(g, loss, metrics=['accuracy', 'Precision', 'Recall', 'AUC'], dropout=0.2)
        hist.append(m.fit(seq, epochs=2, verbose=False))
        models.append(m)
    assert models[1]._trainer._graphs and not models[0]._trainer._graphs
    assert list(hist[0]) == ['loss', 'accuracy', 'precision', 'recall', 'auc'] and hist[0] == hist[1]
    assert all(len(v) == 2 and np.isfinite(v).all() for v in hist[0].values())
    for pa, pb in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(pa, pb), tuple(pa.shape)


def test_mse_trains_other_weights_than_cross_entropy(hip):
    """Fails before this feature: 'mean_squared_error' trained binary cross-entropy."""
    g, seq = _sequence()
    a, b = _model(g, 'mean_squared_error'), _model(g, 'binary_crossentropy')
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    ha, hb = a.fit(seq, epochs=1, verbose=False), b.fit(seq, epochs=1, verbose=False)
    assert list(ha) == list(hb) == ['loss'] and ha['loss'][0] != hb['loss'][0]
    assert any(not torch.equal(pa, pb) for pa, pb in zip(a.parameters(), b.parameters()))
    assert {k[2] for k in a._trainer._graphs} == {'bce'} and all(v['compiled'][0] == hip.LOSS_MSE for v in a._trainer._graphs.values())


def test_fit_metrics_equal_evaluate_metrics_when_the_weights_stand_still(hip):
    """SGD(learning_rate=0), no dropout, batches of 128 and 72: every epoch's metrics are those of evaluate() on the same Sequence —
    accumulation across batches, the eager odd-sized batch (epoch 1: both batches eager, 2: both captured, 3: replayed) and the
    epoch reset."""
    from deep_cbrs_amar_renaissance_amd.experiment import SGD
    g, seq = _sequence(n=200)
    names = ['accuracy', 'Precision', 'Recall', 'AUC']
    model = _model(g, 'mse', metrics=names, optimizer=SGD(learning_rate=0.0))
    before = [p.detach().clone() for p in model.parameters()]
    hist = model.fit(seq, epochs=3, verbose=False)
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert len(model._trainer._graphs) == 2
    out = model.evaluate(seq)
    assert len(out) == 5
    for k, name in enumerate(['accuracy', 'precision', 'recall', 'auc']):
        assert hist[name] == [out[1 + k]] * 3, name
    assert 0 < out[1] < 1 and 0 < out[4] < 1
    # a second compile() with other metrics captures anew and reports only those
    model.compile(loss='mse', optimizer=model.optimizer, metrics=['AUC'])
    hist = model.fit(seq, epochs=2, verbose=False)
    assert list(hist) == ['loss', 'auc'] and hist['auc'] == [out[4]] * 2
    model.compile(loss='mse', optimizer=model.optimizer)
    assert list(model.fit(seq, epochs=2, verbose=False)) == ['loss']
    assert all(v['compiled'] == (hip.LOSS_MSE, (0.0, 0.0, 0.0, 0.0), False) for v in model._trainer._graphs.values())


def test_evaluate_returns_values_in_compile_order(hip):
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import metric_counters, metric_values
    g, seq = _sequence(n=200)
    model = _model(g, {'name': 'huber', 'delta': 0.5}, metrics=['AUC', 'accuracy'])
    pred = model.predict(seq).reshape(-1)
    y = np.concatenate([seq[b][1] for b in range(len(seq))])
    out = model.evaluate(seq)
    values = metric_values(metric_counters(pred, y), ['auc', 'accuracy'])
    assert out[1:] == [values['auc'], values['accuracy']]
    reg = sum(1e-4 * float((w.detach().double() ** 2).sum()) for w in model.parameters() if getattr(w, 'regularizer', None) is not None)
    assert abs(out[0] - (L.loss_value({'name': 'huber', 'delta': 0.5}, y, pred.astype(np.float64)) + reg)) < 1e-9
    default = _model(g, None)
    loss, acc = default.evaluate(seq)                                 # the default compile: [loss, accuracy]
    assert acc == float(np.mean((default.predict(seq).reshape(-1) > 0.5) == (y > 0.5))) and np.isfinite(loss)
    only_acc = _model(g, 'hinge', metrics=['acc'])
    assert len(only_acc.evaluate(seq)) == 2


def test_errors_are_raised_again_where_fit_reads_the_loss(hip):
    g, seq = _sequence(n=200)
    model = _model(g, 'mse')
    model.loss = 'categorical_crossentropy'                          # (set behind compile()'s back)
    with pytest.raises(NotImplementedError):
        model.fit(seq, epochs=1, verbose=False)
    model.loss = 'no_such_loss'
    with pytest.raises(ValueError):
        model.fit(seq, epochs=1, verbose=False)


# ---- the other two call sites, and a hybrid graph model -------------------------------------------------------------------------------

def _check_hinge_history(hist, epochs=1):
    assert list(hist) == ['loss', 'accuracy', 'auc']
    assert all(len(v) == epochs and np.isfinite(v).all() for v in hist.values())
    assert 0 <= hist['accuracy'][0] <= 1 and 0 <= hist['auc'][0] <= 1


@pytest.mark.parametrize('kind', ['BasicRS', 'HybridCBRS', 'HybridBertGCN'])
def test_hinge_with_metrics_on_the_other_trainers(hip, kind):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import HybridUserItemEmbeddings, UserItemEmbeddings, UserItemGraphEmbeddings
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    engine.set_seed(4)
    rng = np.random.default_rng(6)
    g = helpers.tiny_graph(n_users=70, n_items=50, n_ratings=1400, seed=3)
    n = g['adj'].shape[0]
    table, bert = (rng.standard_normal((n, d)).astype(np.float32) * 0.5 for d in (16, 24))
    r = g['ratings'][:599]                                            # batches of 200, 200, 199
    if kind == 'BasicRS':
        seq = UserItemEmbeddings(r, g['users'], g['items'], table, batch_size=200)
        model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
    elif kind == 'HybridCBRS':
        seq = HybridUserItemEmbeddings(r, g['users'], g['items'], table, bert, batch_size=200)
        model = hybrid.HybridCBRS(feature_based=True, dense_units=[[24, 16], [32, 16], [16, 8]], clf_units=[16])
    else:
        seq = UserItemGraphEmbeddings(r, g['users'], g['items'], g['adj'], bert, batch_size=200)
        model = hybrid.HybridBertGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[[24, 16], [32, 24], [16, 16]],
                                     clf_units=[24, 16], l2_regularizer=1e-4, feature_based=True, fusion_method='concatenate', residual=False)
    model.compile(loss='hinge', metrics=['accuracy', 'AUC'])
    hist = model.fit(seq, epochs=2, verbose=False)
    _check_hinge_history(hist, epochs=2)
    assert model._trainer._graphs                                      # the second epoch replayed
    out = model.evaluate(seq)
    assert len(out) == 3 and np.isfinite(out).all()


# ---- the experiment -------------------------------------------------------------------------------------------------------------------

def test_experiment_with_a_mapping_loss_logs_every_metric(hip, tmp_path, monkeypatch):
    """The config of tests/test_experiment_gpu.py with `loss: {name: huber, delta: 0.5}` and `metrics: [accuracy, AUC]`."""
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
    cfg['dataset'].update({'load_function_name': 'load_user_item_graph', 'graph_filepath': 'unused.json', 'bert_user_filepath': 'unused.json',
                           'bert_item_filepath': 'unused.json'})
    cfg['model'].update({'name': 'basic.BasicGCN', 'embedding_dim': 8, 'n_hiddens': [8, 8], 'dense_units': [24, 24], 'clf_units': [48, 48]})
    cfg['parameters'].update({'loss': {'name': 'huber', 'delta': 0.5}, 'metrics': ['accuracy', 'AUC']})
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump({'linear': {'huber': None}}))
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('loss test', str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log)
    results = multi.run()
    assert list(results) == ['huber'] and results['huber'] is not None
    logs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    assert len(logs) == 1
    metrics = {}
    for line in open(logs[0]):
        record = json.loads(line)
        if record['event'] == 'metrics':
            metrics.update(record['metrics'])
    assert np.isfinite(metrics['test_loss']) and metrics['test_loss'] > 0.0
    assert 0.0 <= metrics['test_accuracy'] <= 1.0 and 0.0 <= metrics['test_auc'] <= 1.0

"""GPU: the weighted training loss on the device — amar_loss_grad_weighted_f32 against amar_loss_grad_f32 bit for bit (unit weights,
float32 products, zero weights) and against the float64 restatement, the Trainer's gradients under class_weight and sample weights
(exact doubling, unit weights, autograd), and fit() / evaluate(): unit weights change no bit, doubled weights = a doubled rate,
replayed = eager, the epoch loss, the BPR refusals and the misspelt keyword (pytest -m gpu)."""
import types

import numpy as np
import pytest
import torch

from oracle import train as otrain
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SMALL = [1, 63, 64, 65, 256, 257]                                    # lane, wavefront and workgroup (256) edges
STRIDE = 8192 * 256 + 3                                              # past the largest grid (8 192 workgroups): the grid-stride loop
LOSSES = ['binary_crossentropy', {'name': 'binary_crossentropy', 'label_smoothing': 0.1}, 'mse', 'mae', 'hinge', 'squared_hinge',
          {'name': 'huber', 'delta': 0.25}, 'log_cosh', 'poisson', 'binary_focal_crossentropy',
          {'name': 'binary_focal_crossentropy', 'gamma': 3.0, 'apply_class_balancing': True, 'alpha': 0.25}]
_ids = lambda v: v if isinstance(v, str) else '-'.join(str(x) for x in v.values())   # noqa: E731
GCN = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48])       # tests/test_training_gpu.py: CFG
HYBRID = dict(embedding_dim=8, n_hiddens=[8, 8], dense_units=[[16], [16], [16]], clf_units=[16], feature_based=True)   # ... its smallest hybrid


def _resolve(loss):
    from deep_cbrs_amar_renaissance_amd.utilities.losses import resolve_loss
    return resolve_loss(loss)[:2]


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------

_INPUTS = {}


def _inputs(B):
    """(p, y, sample_w, [contiguous p, strided p], y, sample_w on the device) for B pairs, made once: the kinks of
    tests/test_losses_metrics_gpu.py in front (labels of both classes), float32 weights in [0, 3) with exact 0s and 1s among them."""
    if B not in _INPUTS:
        from tests.test_losses_metrics_gpu import _device_p, _kink_inputs
        p, y = _kink_inputs(B, seed=B % 1000)
        rng = np.random.default_rng(B % 1000 + 1)
        w = rng.uniform(0, 3, B).astype(np.float32)
        w[1::7], w[2::11] = 0.0, 1.0
        _INPUTS[B] = (p, y, w, [_device_p(p, False), _device_p(p, True)], torch.from_numpy(y).to(DEV), torch.from_numpy(w).to(DEV))
    return _INPUTS[B]


def _run(hip, code, hyper, pd, yd, count, sample_weight=None, class_weight=None):
    B = yd.numel()
    dz, terms = torch.full((B, 1), float('nan'), device=DEV), torch.full((B,), float('nan'), device=DEV)
    counters = torch.zeros(hip.LOSS_COUNTERS, dtype=torch.int64, device=DEV) if count else None
    hip.loss_grad(code, hyper, pd, yd, dz, terms, counters=counters, sample_weight=sample_weight, class_weight=class_weight)
    return dz, terms, counters


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('B', SMALL + [STRIDE])
@pytest.mark.parametrize('loss', LOSSES, ids=_ids)
def test_weighted_kernel_against_the_unweighted_bits(hip, loss, B):
    """The three exact statements of the kernel's contract (the weight multiplies the finished float32 output, last), for contiguous
    and strided p, with and without the counter block."""
    code, hyper = _resolve(loss)
    _, _, _, pds, yd, wd = _inputs(B)
    ones, pair_ones = torch.ones(B, device=DEV), torch.ones(2, device=DEV)
    pair = torch.tensor([0.75, 2.5], device=DEV)
    zeros = torch.zeros(B, device=DEV)
    for pd in pds:
        for count in (False, True):
            base = _run(hip, code, hyper, pd, yd, count)
            assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()
            # 1. unit weights: the unweighted bits, counters included
            assert _same(_run(hip, code, hyper, pd, yd, count, sample_weight=ones), base)
            assert _same(_run(hip, code, hyper, pd, yd, count, class_weight=pair_ones), base)
            assert _same(_run(hip, code, hyper, pd, yd, count, sample_weight=ones, class_weight=pair_ones), base)
            # 2. float32 products, computed by torch on the same device
            per_class = pair[(yd > 0.5).long()]
            for kwargs, w in (({'sample_weight': wd}, wd), ({'class_weight': pair}, per_class),
                              ({'sample_weight': wd, 'class_weight': pair}, wd * per_class)):
                dz, terms, counters = _run(hip, code, hyper, pd, yd, count, **kwargs)
                assert torch.equal(terms, w * base[1]) and torch.equal(dz, w.reshape(-1, 1) * base[0])
                assert counters is None or torch.equal(counters, base[2])            # the counters do not see the weights
            # 3. weight 0: exactly 0, and the pair is still counted
            for kwargs in ({'sample_weight': zeros}, {'class_weight': torch.zeros(2, device=DEV)}):
                dz, terms, counters = _run(hip, code, hyper, pd, yd, count, **kwargs)
                assert (terms == 0).all() and (dz == 0).all()
                assert counters is None or (torch.equal(counters, base[2]) and int(counters[:4].sum()) == B)


@pytest.mark.parametrize('loss', LOSSES, ids=_ids)
def test_weighted_kernel_against_float64(hip, loss):
    """Weights in [0.25, 4].  The bound is the one tests/test_losses_metrics_gpu.py holds for the unweighted kernel (terms: rtol 2e-6,
    atol 1e-7; dz: rtol 2e-5, atol 1e-9, element by element on the unweighted value) multiplied by max |w|: the weighted output is
    w_i x the unweighted one, so its error is at most max |w| x the unweighted error, plus the product's own rounding (2^-24
    relative, a thirtieth of the tightest rtol)."""
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    from tests.test_losses_metrics_gpu import _device_p, _kink_inputs
    code, hyper = _resolve(loss)
    for B in SMALL + [1025]:
        p, y = _kink_inputs(B, seed=B + 7 * code)
        rng = np.random.default_rng(B + code)
        sw = rng.uniform(0.25, 2.0, B).astype(np.float32)
        cw = np.array([0.5, 2.0], dtype=np.float32)
        for strided in (False, True):
            dz, terms, _ = _run(hip, code, hyper, _device_p(p, strided), torch.from_numpy(y).to(DEV), False,
                                sample_weight=torch.from_numpy(sw).to(DEV), class_weight=torch.from_numpy(cw).to(DEV))
            w = L.pair_weights(y, sw, cw)
            wmax = float(np.abs(w).max())
            assert w.min() >= 0.125 and wmax <= 4.0
            p64 = p.astype(np.float64)
            t0 = L.loss_terms(code, hyper, y, p64, f32_constants=True)
            through = p64 * (1.0 - p64)
            with np.errstate(invalid='ignore'):
                d0 = np.where(through == 0, 0.0, L.loss_dp(code, hyper, y, p64, f32_constants=True) * through / B)
            want_t = L.loss_terms(code, hyper, y, p64, f32_constants=True, sample_weight=sw, class_weight=cw)
            assert np.array_equal(want_t, w * t0)
            gt, gd = terms.cpu().numpy().astype(np.float64), dz.cpu().numpy().reshape(-1).astype(np.float64)
            err_t, err_d = np.abs(gt - want_t), np.abs(gd - w * d0)
            bound_t, bound_d = wmax * (2e-6 * np.abs(t0) + 1e-7), wmax * (2e-5 * np.abs(d0) + 1e-9)
            print(_ids(loss), B, strided, 'terms: worst error / bound', float((err_t / bound_t).max()), 'dz:', float((err_d / bound_d).max()))
            assert (err_t <= bound_t).all() and (err_d <= bound_d).all()
            assert abs(gt.sum() / B - float(want_t.sum() / B)) <= wmax * (1e-5 * abs(float(t0.mean())) + 1e-7)


def test_weighted_entry_refuses_bad_arguments(hip):
    import ctypes
    p, y = torch.rand(8, device=DEV), torch.zeros(8, device=DEV)
    dz, terms = torch.empty((8, 1), device=DEV), torch.empty(8, device=DEV)
    w, pair = torch.ones(8, device=DEV), torch.ones(2, device=DEV)
    lib, stream = hip.load(), torch.cuda.current_stream().cuda_stream
    args = (p.data_ptr(), 1, y.data_ptr())
    assert lib.amar_loss_grad_weighted_f32(hip.LOSS_MSE, None, *args, None, None, dz.data_ptr(), terms.data_ptr(), 8, None, stream) == -1
    assert lib.amar_loss_grad_weighted_f32(hip.LOSS_MSE, None, *args, w.data_ptr(), None, dz.data_ptr(), terms.data_ptr(), 0, None, stream) == -1
    assert lib.amar_loss_grad_weighted_f32(99, None, *args, w.data_ptr(), None, dz.data_ptr(), terms.data_ptr(), 8, None, stream) == -1
    hyper = (ctypes.c_float * 4)(2.0, 0.0, 0.0, 0.0)                         # label_smoothing outside [0, 1]
    assert lib.amar_loss_grad_weighted_f32(hip.LOSS_BCE, hyper, *args, w.data_ptr(), None, dz.data_ptr(), terms.data_ptr(), 8, None, stream) == -1
    assert lib.amar_loss_grad_weighted_f32(hip.LOSS_MSE, None, *args, w.data_ptr(), pair.data_ptr(), dz.data_ptr(), terms.data_ptr(), 8, None,
                                           stream) == 0
    with pytest.raises(ValueError):
        hip.loss_grad(hip.LOSS_MSE, None, p, y, dz, terms, sample_weight=w[:7])
    with pytest.raises(ValueError):
        hip.loss_grad(hip.LOSS_MSE, None, p, y, dz, terms, class_weight=torch.ones(3, device=DEV))
    with pytest.raises(ValueError):
        hip.loss_grad(hip.LOSS_MSE, None, p, y, dz, terms, sample_weight=w.double())


# ---- the Trainer's gradients ------------------------------------------------------------------------------------------------------------

def _graph():
    return helpers.tiny_graph(n_users=60, n_items=50, n_ratings=1200, seed=1)     # the smallest graph of tests/test_training_gpu.py


def _trainer_case(kind):
    """(model, trainer, oracle gnn / head, batch, BERT table or None) of the GCN-kind model or the hybrid head, L2 off."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    g = _graph()
    engine.set_seed(5)
    table = None
    if kind == 'BasicGCN':
        model = basic.BasicGCN(g['adj'], l2_regularizer=None, **GCN)
        head = helpers.basic_head_to_oracle
    else:
        model = hybrid.HybridBertGCN(g['adj'], l2_regularizer=None, **HYBRID)
        table = np.random.default_rng(3).standard_normal((g['adj'].shape[0], 24)).astype(np.float32) * 0.5
        model.set_bert_table(table)
        head = helpers.hybrid_head_to_oracle
    trainer = training.Trainer(model)
    helpers.randomize_biases(model, seed=6)
    assert all(trainer._l2(prm) == 0.0 for prm in trainer.params)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    return g, model, trainer, helpers.gnn_to_oracle(model.gnn), head(model.rs), y, table


@pytest.mark.parametrize('kind', ['BasicGCN', 'HybridBertGCN'])
def test_trainer_gradients_under_weights(hip, kind):
    from tests.test_bpr_gpu import _targets_for
    from tests.test_training_gpu import _flatten_oracle_grads
    g, model, trainer, gnn, head, y, table = _trainer_case(kind)
    u, i, B = g['u_ids'], g['i_ids'], len(y)
    loss0, g0 = trainer.loss_and_grads(u, i, y)
    g0 = {k: v.clone() for k, v in g0.items()}
    # class_weight = {0: 2, 1: 2}: dz is doubled exactly by the kernel's last multiplication, and a power-of-two scaling passes through
    # the linear reverse pass unchanged (every product and every partial sum is doubled exactly, no rounding moves)
    trainer.set_class_weight({0: 2.0, 1: 2.0})
    loss2, g2 = trainer.loss_and_grads(u, i, y)
    assert loss2 == 2.0 * loss0 and set(g2) == set(g0)
    for prm in g0:
        assert torch.equal(g2[prm], 2.0 * g0[prm]), tuple(prm.shape)
    # unit weights, through both arguments: the unweighted bits
    trainer.set_class_weight({0: 1.0, 1: 1.0})
    loss1, g1 = trainer.loss_and_grads(u, i, y, sample_weight=np.ones(B))
    assert loss1 == loss0 and all(torch.equal(g1[prm], g0[prm]) for prm in g0)
    trainer.set_class_weight(None)                                        # off again: the unweighted launch
    loss1, g1 = trainer.loss_and_grads(u, i, y)
    assert loss1 == loss0 and all(torch.equal(g1[prm], g0[prm]) for prm in g0)
    # random weights against autograd (float64, CPU) of the weighted loss written here: sum_j w_j l_j / B.  As
    # tests/test_losses_metrics_gpu.py:test_trainer_gradients_match_autograd, the oracle's cross-entropy is given the targets at which
    # its cotangent d(loss)/dp is the one torch autograd takes from this loss.  Tolerance: tests/test_training_gpu.py's, for both kinds.
    rng = np.random.default_rng(8)
    sw, cw = rng.uniform(0.25, 2.0, B).astype(np.float32), {0: 0.5, 1: 2.0}
    trainer.set_class_weight(cw)
    got_loss, grads = trainer.loss_and_grads(u, i, y, sample_weight=sw)
    bert = (table[u], table[i]) if table is not None else None
    _, _, p = otrain.torch_model_grads(g['adj'], gnn, head, u, i, y, l2=0.0, bert=bert)
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    pt, yt, eps = torch.tensor(p, requires_grad=True), torch.tensor(y, dtype=torch.float64), 1e-7
    w = torch.tensor(sw, dtype=torch.float64) * torch.where(yt > 0.5, torch.tensor(cw[1], dtype=torch.float64), torch.tensor(cw[0], dtype=torch.float64))
    pc = torch.clamp(pt, eps, 1 - eps)
    want_loss = (w * -(yt * torch.log(pc + eps) + (1 - yt) * torch.log(1 - pc + eps))).sum() / B
    c = torch.autograd.grad(want_loss, pt)[0].numpy()
    _, want, _ = otrain.torch_model_grads(g['adj'], gnn, head, u, i, _targets_for(p, c), l2=0.0, bert=bert)
    assert abs(got_loss - float(want_loss.detach())) < 4 * 1e-5                   # (tests/test_training_gpu.py's 1e-5, times max |w| = 4)
    flat = _flatten_oracle_grads(model, want)
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        assert np.abs(got - gw).max() <= 2e-4 * np.abs(gw).max() + 1e-10, tuple(prm.shape)
    assert any(not torch.equal(grads[prm], g0[prm]) for prm in g0)


# ---- fit() and evaluate() ---------------------------------------------------------------------------------------------------------------

def _sequence(g, n=600, batch_size=128, **kwargs):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    return UserItemGraph(g['ratings'][:n], g['users'], g['items'], g['adj'], batch_size=batch_size, **kwargs)    # batches of 128 .. and 88


def _model(g, optimizer=None, loss=None, seed=8, l2=None, metrics=None, **extra):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(seed)
    model = basic.BasicGCN(g['adj'], l2_regularizer=l2, **dict(GCN, **extra))
    helpers.randomize_biases(model, seed=1)
    model.compile(loss=loss, optimizer=optimizer or Adam(learning_rate=1e-3), metrics=metrics)
    model((g['u_ids'], g['i_ids']))
    return model


def _same_weights(a, b):
    return all(torch.equal(pa, pb) for pa, pb in zip(a.parameters(), b.parameters()))


@pytest.mark.parametrize('graph', ['1', '0'], ids=['replayed', 'eager'])
def test_fit_with_unit_weights_changes_no_bit(hip, monkeypatch, graph):
    monkeypatch.setenv('AMAR_TRAIN_GRAPH', graph)
    g = _graph()
    plain, weighted = _model(g, l2=1e-4), _model(g, l2=1e-4)
    h0 = plain.fit(_sequence(g, shuffle=True), epochs=3, verbose=False)
    h1 = weighted.fit(_sequence(g, shuffle=True, sample_weight=np.ones(600)), epochs=3, verbose=False, class_weight={0: 1.0, 1: 1.0})
    assert h0 == h1 and len(h0['loss']) == 3 and _same_weights(plain, weighted)
    assert bool(getattr(weighted._trainer, '_graphs', None)) == (graph == '1')       # (eager batches keep no graph state)
    if graph == '1':                                                      # whether weights are present is in the key, their values are not
        assert all(k[-1] == ('weights', True, True) for k in weighted._trainer._graphs)
        assert not any(isinstance(k[-1], tuple) and k[-1][:1] == ('weights',) for k in plain._trainer._graphs)


@pytest.mark.parametrize('graph', ['1', '0'], ids=['replayed', 'eager'])
def test_fit_with_doubled_weights_is_fit_at_the_doubled_rate(hip, monkeypatch, graph):
    """Plain SGD, L2 off: w - eta (2 g) and w - (2 eta) g are the same float32 operation on the same numbers, and 2 g is exact (see
    test_trainer_gradients_under_weights); the reported loss is doubled, exactly.  Fails before this feature: class_weight was dropped."""
    from deep_cbrs_amar_renaissance_amd.experiment import SGD
    monkeypatch.setenv('AMAR_TRAIN_GRAPH', graph)
    g = _graph()
    doubled_rate, doubled_weights = _model(g, optimizer=SGD(learning_rate=0.1)), _model(g, optimizer=SGD(learning_rate=0.05))
    start = [p.detach().clone() for p in doubled_rate.parameters()]
    h0 = doubled_rate.fit(_sequence(g), epochs=3, verbose=False)
    h1 = doubled_weights.fit(_sequence(g), epochs=3, verbose=False, class_weight={0: 2, 1: 2})
    assert _same_weights(doubled_rate, doubled_weights)
    assert any(not torch.equal(a, b) for a, b in zip(start, doubled_rate.parameters()))
    assert h1['loss'] == [2.0 * v for v in h0['loss']]


def test_fit_replayed_equals_eager_with_sample_weights(hip, monkeypatch):
    """Random sample weights, a class pair and a shuffling Sequence; a model that drops, as in the other tests of this statement
    (without dropout AMAR_TRAIN_GRAPH=0 steps through train_batch, whose Adam takes its step size from the host in float64)."""
    g = _graph()
    sw = np.random.default_rng(11).uniform(0.0, 3.0, 600)
    models, hist = [], []
    for env in ('0', '1'):
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = _model(g, l2=1e-4, dropout=0.2)
        hist.append(m.fit(_sequence(g, shuffle=True, seed=7, sample_weight=sw), epochs=3, verbose=False, class_weight={0: 0.5, '1': 3.0}))
        models.append(m)
    assert models[1]._trainer._graphs and not models[0]._trainer._graphs
    assert hist[0] == hist[1] and np.isfinite(hist[0]['loss']).all()
    assert _same_weights(*models)
    unweighted = _model(g, l2=1e-4, dropout=0.2)
    unweighted.fit(_sequence(g, shuffle=True, seed=7), epochs=3, verbose=False)
    assert not _same_weights(unweighted, models[1])                       # (the weights did train another loss)


def test_epoch_loss_and_evaluate_equal_the_float64_restatement(hip):
    """SGD at rate 0 (the weights stand still), batches of 128 and 72, first eager, then captured and replayed: every epoch's loss is
    sum_j w_j l_j / N over all pairs with w = sample weight x class weight, plus the L2 term; evaluate() applies the Sequence's sample
    weights and never the class weights.  Bound of the training loss: the terms' rtol 2e-6 plus a float32 sum of at most 128 terms
    (128 x 2^-24 = 8e-6), rounded up to 2e-5 of the value; evaluate() restates in float64 (1e-9, as
    tests/test_losses_metrics_gpu.py:test_evaluate_returns_values_in_compile_order)."""
    from deep_cbrs_amar_renaissance_amd.experiment import SGD
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    g = _graph()
    loss = {'name': 'huber', 'delta': 0.5}
    sw = np.random.default_rng(12).uniform(0.0, 3.0, 200)
    seq = _sequence(g, n=200, sample_weight=sw)
    model = _model(g, optimizer=SGD(learning_rate=0.0), loss=loss, l2=1e-4, metrics=['accuracy'])
    hist = model.fit(seq, epochs=3, verbose=False, class_weight={0: 0.5, 1: 3.0})
    assert len(model._trainer._graphs) == 2
    pred = model.predict(seq).reshape(-1).astype(np.float64)
    y = g['ratings'][:200, 2]
    reg = sum(1e-4 * float((w.detach().double() ** 2).sum()) for w in model.parameters() if getattr(w, 'regularizer', None) is not None)
    assert reg > 0
    want_fit = L.loss_value(loss, y, pred, sample_weight=seq.sample_weight, class_weight=(0.5, 3.0)) + reg
    assert all(abs(v - want_fit) <= 2e-5 * want_fit for v in hist['loss']), (hist['loss'], want_fit)
    want_eval = L.loss_value(loss, y, pred, sample_weight=seq.sample_weight) + reg
    out = model.evaluate(seq)
    assert abs(out[0] - want_eval) < 1e-9 and abs(want_eval - want_fit) > 1e-2
    assert hist['accuracy'] == [out[1]] * 3 == [float(np.mean((pred > 0.5) == (y > 0.5)))] * 3      # metrics stay unweighted
    plain = model.evaluate(_sequence(g, n=200))
    assert abs(plain[0] - (L.loss_value(loss, y, pred) + reg)) < 1e-9 and plain[1] == out[1]
    # validation_data applies the Sequence's weights, too: val_loss is evaluate()'s
    hist = model.fit(seq, epochs=1, verbose=False, validation_data=seq)
    assert hist['val_loss'] == [out[0]] and abs(hist['loss'][0] - want_eval) <= 2e-5 * want_eval       # (no class_weight in this fit)


def test_new_class_weights_do_not_capture_again(hip):
    g = _graph()
    model = _model(g)
    seq = _sequence(g, n=256)
    model.fit(seq, epochs=2, verbose=False, class_weight={0: 1.0, 1: 3.0})
    trainer = model._trainer
    captures, buffer = trainer.capture_count, trainer._class_w.data_ptr()
    assert captures == 1 and trainer._class_w.tolist() == [1.0, 3.0]
    model.fit(seq, epochs=1, verbose=False, class_weight={0: 2.0, 1: 0.5})
    assert trainer.capture_count == captures and trainer._class_w.data_ptr() == buffer and trainer._class_w.tolist() == [2.0, 0.5]
    model.fit(seq, epochs=2, verbose=False)                               # no weights: the unweighted graph, under its old key
    assert trainer.capture_count == captures + 1 and not trainer._class_weighted
    assert sorted(len(k) for k in trainer._graphs) == [3, 4]


@pytest.mark.parametrize('kind', ['BasicRS', 'HybridCBRS', 'HybridBertGCN'])
def test_the_other_fit_loops_carry_the_weights(hip, kind):
    """The head-only trainers on resident tables and the hybrid graph model on its ids Sequence: unit weights change no bit; with
    all pairs in one batch the first epoch's loss is computed before any update, and doubled weights, given either way, double it
    exactly."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import HybridUserItemEmbeddings, UserItemEmbeddings, UserItemGraphEmbeddings
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    g = _graph()
    n = g['adj'].shape[0]
    rng = np.random.default_rng(6)
    table, bert = (rng.standard_normal((n, d)).astype(np.float32) * 0.5 for d in (16, 24))
    r = g['ratings'][:328]                                                # batches of 128, 128, 72

    def run(sample_weight=None, epochs=2, batch_size=128, **fit_args):
        engine.set_seed(4)
        extra = {} if sample_weight is None else {'sample_weight': sample_weight}
        if kind == 'BasicRS':
            seq = UserItemEmbeddings(r, g['users'], g['items'], table, batch_size=batch_size, **extra)
            model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
        elif kind == 'HybridCBRS':
            seq = HybridUserItemEmbeddings(r, g['users'], g['items'], table, bert, batch_size=batch_size, **extra)
            model = hybrid.HybridCBRS(feature_based=True, dense_units=[[24, 16], [32, 16], [16, 8]], clf_units=[16])
        else:
            seq = UserItemGraphEmbeddings(r, g['users'], g['items'], g['adj'], bert, batch_size=batch_size, **extra)
            model = hybrid.HybridBertGCN(g['adj'], l2_regularizer=None, **HYBRID)
        model.compile(optimizer=types.SimpleNamespace(learning_rate=5e-3, beta_1=0.9))
        hist = model.fit(seq, epochs=epochs, verbose=False, **fit_args)
        return model, hist['loss']
    plain, h0 = run()
    ones, h1 = run(sample_weight=np.ones(len(r)), class_weight={0: 1, 1: 1})
    assert h0 == h1 and _same_weights(plain, ones) and ones._trainer._graphs
    # one batch of all 328 pairs, one epoch: its loss is computed before any update
    _, single = run(epochs=1, batch_size=328)
    _, doubled = run(epochs=1, batch_size=328, sample_weight=np.full(len(r), 2.0))
    _, by_class = run(epochs=1, batch_size=328, class_weight={0: 2.0, 1: 2.0})
    assert doubled == by_class == [2.0 * single[0]]


def test_bpr_training_and_evaluation_refuse_weights(hip):
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests.test_bpr_gpu import _sample_sequence
    g = _graph()
    sampled = _sample_sequence()
    model = _model(dict(helpers.tiny_graph(n_users=70, n_items=50, n_ratings=1400, seed=3), adj=sampled.adj_matrix), loss=BPRLoss())
    with pytest.raises(ValueError):
        model.fit(sampled, epochs=1, verbose=False, class_weight={0: 1.0, 1: 3.0})
    sampled.sample_weight = np.ones(len(sampled.ratings))
    with pytest.raises(ValueError):
        model.fit(sampled, epochs=1, verbose=False)
    pairs = _model(g, loss=BPRLoss())                                     # BPRLoss on a Sequence of labelled pairs (halves of a batch)
    with pytest.raises(ValueError):
        pairs.fit(_sequence(g, n=256), epochs=1, verbose=False, class_weight={0: 1.0, 1: 3.0})
    weighted = _sequence(g, n=256, sample_weight=np.ones(256))
    with pytest.raises(ValueError):
        pairs.fit(weighted, epochs=1, verbose=False)
    with pytest.raises(ValueError):
        pairs.evaluate(weighted)
    assert np.isfinite(pairs.evaluate(_sequence(g, n=256))[0])


def test_fit_refuses_a_keyword_it_does_not_know(hip):
    """Fails before this feature: every fit() ended in **kwargs, and `clas_weight` trained the unweighted loss without a word."""
    g = _graph()
    model = _model(g)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(TypeError):
        model.fit(_sequence(g, n=256), epochs=1, verbose=False, clas_weight={0: 1.0, 1: 3.0})
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert model.fit(_sequence(g, n=256), epochs=1, verbose=False, workers=4)['loss']          # (what the experiment passes)
    with pytest.raises(ValueError):
        model.fit(_sequence(g, n=256), epochs=1, verbose=False, class_weight={0: 1.0, 2: 3.0})
    with pytest.raises(ValueError):                                       # a class of the Sequence's labels without a weight
        model.fit(_sequence(g, n=256), epochs=1, verbose=False, class_weight={1: 3.0})

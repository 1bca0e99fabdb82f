"""GPU: the optimizers besides Adam — amar_optim_advance_f32 / amar_optim_f32 / amar_optim_multi_f32 against the float64 rules of
tests/optimizer_ref.py, the multi-slot form against the single-tensor form bit for bit, training steps against the oracle's gradients
pushed through those rules, replayed = eager batches, fit() and one experiment through the public surface (pytest -m gpu).

Errors of the kernels are measured per element against the element's own scale (optimizer_ref.scales: the magnitudes of its terms), as
tests/test_entry_points_gpu.py does for Adam; every buffer a kernel must not touch starts as a sentinel."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import train as otrain
from tests import entry_point_ref as ref
from tests import helpers
from tests import optimizer_ref as oref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = np.float32(-7.25)
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)

# every rule and flag combination: id -> (rule, hyper-parameters besides Keras' defaults)
CASES = {
    'sgd': ('SGD', {}),
    'sgd-momentum': ('SGD', dict(momentum=0.9)),
    'sgd-nesterov': ('SGD', dict(momentum=0.9, nesterov=True)),
    'rmsprop': ('RMSprop', {}),
    'rmsprop-momentum': ('RMSprop', dict(momentum=0.9)),
    'rmsprop-centered': ('RMSprop', dict(centered=True)),
    'rmsprop-centered-momentum': ('RMSprop', dict(momentum=0.9, centered=True)),
    'adagrad': ('Adagrad', {}),
    'adamax': ('Adamax', {}),
    'nadam': ('Nadam', {}),
    'amsgrad': ('AMSGrad', {}),
}
LARGE = ['sgd-nesterov', 'rmsprop-centered-momentum', 'adagrad', 'adamax', 'nadam', 'amsgrad']        # one per rule


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _spec(case, **more):
    from deep_cbrs_amar_renaissance_amd import training
    rule, hyper = CASES[case]
    return training.OptimizerSpec(rule=rule, **dict(hyper, **more))


def _h32(case, **more):
    rule, hyper = CASES[case]
    return rule, oref.as_float32(oref.hyper_of(rule, **dict(hyper, **more)))


def _arrays(rng, rule, h, n, planted=True):
    """w, g and the rule's state arrays (float32): moments ~ 0.1 N(0, 1), accumulators in (0.05, 1) — centered RMSprop's rms above its
    mg^2 by that much, as a true second moment is.  The first three elements have zero gradient and zero state; for centered RMSprop
    the next three start from rms = fl(c c), mg = c, g = c (the difference rms - mg^2 rounds to either side of 0)."""
    w, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    names = oref.state_names(rule, h)
    arrays = {}
    for name in names:
        if name in ('a', 'mg', 'mom', 'm'):
            arrays[name] = (rng.standard_normal(n) * 0.1).astype(np.float32)
    for name in names:
        if name not in arrays:
            arrays[name] = (rng.uniform(0.05, 1, n) + (arrays['mg'].astype(np.float64) ** 2 if name == 'rms' and 'mg' in arrays else 0)).astype(np.float32)
    arrays = [arrays[name] for name in names]
    if planted:
        z = slice(0, min(n, 3))
        g[z] = 0
        for a in arrays:
            a[z] = 0
        if 'mg' in names and n >= 6:
            c = np.array([0.3, -1.7, 1e-3], dtype=np.float32)
            g[3:6], arrays[0][3:6], arrays[1][3:6] = c, c * c, c
    return w, g, arrays


def _check64(rule, h, sc, got_w, got_s, w, parts, arrays, l2):
    """w and every state array against float64, per element against optimizer_ref.scales, below the 1e-6 of _adam_check64.  Centered
    RMSprop's planted elements 3..5 (rms = fl(c c), mg = c, g = c) must be finite and are not compared: their rms - mg^2 cancels
    completely, so float32 rounding decides between 0 and a tiny positive denominator and no first-order scale describes the result."""
    want_w, want_s = oref.step(rule, h, sc, w, np.asarray(parts, dtype=np.float64).reshape(-1, w.size).sum(0), arrays, l2)
    scale_w, scale_s = oref.scales(rule, h, sc, w, parts, arrays, l2)
    names = oref.state_names(rule, h)
    keep = np.ones(w.size, dtype=bool)
    if 'mg' in names and w.size >= 6:
        keep[3:6] = False
    worst = {}
    for name, a, b, s in zip(['w'] + names, [got_w] + list(got_s), [want_w] + want_s, [scale_w] + scale_s):
        assert np.isfinite(a).all(), name
        worst[name] = ref.scaled_error(a[keep], b[keep], s[keep])
    print('{}: max |got - float64| / scale = {}'.format(rule, {k: '{:.2e}'.format(v) for k, v in worst.items()}))
    for name, err in worst.items():
        assert err < 1e-6, (name, err)


@pytest.mark.parametrize('case', ['sgd', 'adamax', 'nadam', 'amsgrad'])
def test_advance_counts_and_writes_the_scalars_of_the_step(hip, case):
    spec = _spec(case, learning_rate=2e-3)
    rule, h = _h32(case, learning_rate=2e-3)
    state = torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV)
    p = 1.0
    for t in range(1, 11):
        hip.optim_advance(state, spec.code, spec.flags, spec.hyper)
        got = state.cpu().numpy()
        sc = oref.scalars(rule, h, t, p)
        p = sc.get('P', 1.0)
        assert got[0] == t

        def ulps(x, want):
            return abs(float(x) - float(np.float32(want))) / float(np.spacing(np.float32(want)))
        assert ulps(got[1], sc['step']) <= 1
        if rule == 'Nadam':
            # P_t is kept in float32 between steps: one rounding per step so far
            assert ulps(got[2], sc['mu']) <= 1 and ulps(got[3], sc['mu_next']) <= 1 and ulps(got[4], sc['P']) <= t and ulps(got[5], sc['omb2']) <= 1
            lr = h['learning_rate']
            assert ulps(got[6], lr * (1 - sc['mu']) / (1 - sc['P'])) <= 2 and ulps(got[7], lr * sc['mu_next'] / (1 - sc['P'] * sc['mu_next'])) <= 2
        else:
            assert not got[2:].any()


def _three_steps(hip, case, n, l2, seed):
    spec = _spec(case)
    rule, h = _h32(case)
    rng = np.random.default_rng(seed)
    w, g, arrays = _arrays(rng, rule, h, n)
    state = torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV)
    dw, ds = _t(w), [_t(a) for a in arrays]
    spare = [torch.full((n,), float(SENTINEL), device=DEV) for _ in range(3 - len(arrays))]       # pointers of arrays the rule does not have
    p = 1.0
    for t in range(1, 4):
        hip.optim_advance(state, spec.code, spec.flags, spec.hyper)
        hip.optim(spec.code, spec.flags, spec.hyper, dw, _t(g), ds + spare, state, l2=l2)
        sc = oref.scalars(rule, h, t, p)
        p = sc.get('P', 1.0)
        got_w, got_s = dw.cpu().numpy(), [a.cpu().numpy() for a in ds]
        _check64(rule, h, sc, got_w, got_s, w, g, arrays, l2)
        z = slice(0, min(n, 3))
        if l2 == 0.0:
            assert np.array_equal(got_w[z], w[z])                     # zero gradient on zero state: finite, and no move
        assert n <= 6 or np.abs(got_w[6:] - w[6:]).max() > 0          # (the update is not zero elsewhere)
        w, arrays = got_w, got_s
        g = rng.standard_normal(n).astype(np.float32)
        g[z] = 0
    assert all(np.all(s.cpu().numpy() == SENTINEL) for s in spare)
    assert float(state[0]) == 3


@pytest.mark.parametrize('l2', [0.0, 1e-3])
@pytest.mark.parametrize('n', [1, 1027, 4100])
@pytest.mark.parametrize('case', list(CASES))
def test_single_tensor_form_follows_the_float64_rule(hip, case, n, l2):
    _three_steps(hip, case, n, l2, seed=n)


@pytest.mark.parametrize('case', LARGE)
def test_single_tensor_form_above_one_grid_pass(hip, case):
    _three_steps(hip, case, 2_100_003, 1e-3, seed=7)                  # 8 192 x 256 elements are one pass of the grid


def test_argument_checks(hip):
    spec = _spec('adamax')
    x = torch.zeros(8, device=DEV)
    state = torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV)
    with pytest.raises(ValueError):
        hip.optim(spec.code, spec.flags, spec.hyper, x, x.clone(), [x.clone()], state)             # Adamax needs two arrays
    with pytest.raises(ValueError):
        hip.optim(99, 0, spec.hyper, x, x.clone(), [], state)
    with pytest.raises(ValueError):
        hip.optim_advance(state, hip.OPT_ADAGRAD, hip.OPT_NESTEROV, spec.hyper)
    with pytest.raises(ValueError):
        hip.optim(spec.code, spec.flags, spec.hyper, x, x.clone(), [x.clone(), x.clone()], state[:2].clone())   # an Adam-sized state


def _multi_layout():
    """Slots (n, vector path?, g_groups, l2) cut from ONE sentinel-filled buffer with gaps between them, as the Adam test's: every array of
    a vector slot is 16-byte aligned with n % 4 == 0, the scalar slots have n % 4 != 0 or a w offset by one float."""
    spec = [(1, False, 0, 0.0), (1023, False, 0, 1e-3), (1024, True, 0, 1e-3), (4100, True, 0, 0.0), (2048, 'offset', 0, 1e-3)]
    for groups in (1, 4, 17):
        spec += [(1028, True, groups, 1e-3 if groups % 2 else 0.0), (1027, False, groups, 0.0 if groups % 2 else 1e-3)]
    return spec


@pytest.mark.parametrize('case', list(CASES))
def test_multi_form_equals_the_single_form_bit_for_bit(hip, case):
    """optim_multi_kernel: vector and scalar path (by n % 4 and by alignment), block boundaries, deferred partial gradients (sixteen /
    four in flight, with tails), slot lookup by block number, the per-block atomic into loss_acc.  Every slot equals amar_optim_f32 on
    the partials summed in order in float32, bit for bit; gaps, gradients and the state arrays the rule does not have keep their bytes."""
    spec = _spec(case)
    rule, h = _h32(case)
    n_arrays = len(oref.state_names(rule, h))
    assert spec.n_arrays == n_arrays
    rng = np.random.default_rng(11)
    layout = _multi_layout()
    GAP = 8                                                           # floats (a multiple of 4: alignment survives)
    total = sum(4 * (n + 4 + GAP) + max(g, 1) * (n + 4) + GAP for n, _, g, _ in layout) + 64
    host = np.full(total, SENTINEL, dtype=np.float32)
    pos, slots = GAP, []

    def take(count, offset_one):
        nonlocal pos
        start = pos + (1 if offset_one else 0)
        pos = (start + count + GAP + 3) // 4 * 4
        return slice(start, start + count)
    for n, kind, groups, l2 in layout:
        w, g, arrays = _arrays(rng, rule, h, n)
        parts = np.stack([g] + [rng.standard_normal(n).astype(np.float32) for _ in range(max(groups, 1) - 1)])
        s = {'n': n, 'kind': kind, 'groups': groups, 'l2': l2, 'parts': parts, 'w': take(n, kind == 'offset'),
             's': [take(n, False) for _ in range(3)], 'g': take(max(groups, 1) * n, False)}
        host[s['w']], host[s['g']] = w, parts.reshape(-1)
        for k, a in enumerate(arrays):
            host[s['s'][k]] = a                                        # (the areas of arrays the rule does not have keep the sentinel)
        slots.append(s)
    assert pos <= total
    state = torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV)
    for _ in range(5):
        hip.optim_advance(state, spec.code, spec.flags, spec.hyper)
    reg_scale = 0.5
    results = {}
    for with_loss in (False, True):
        buf = _t(host)
        entries = []
        for s in slots:
            g = buf[s['g']]
            entries.append((buf[s['w']], hip.DeferredGradient(g, s['groups'], (s['n'],)) if s['groups'] else g, [buf[k] for k in s['s']], s['l2']))
            used = [entries[-1][0], g] + entries[-1][2][:n_arrays]
            assert (s['n'] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in used)) == (s['kind'] is True), (s['n'], s['kind'])
        table, blocks = hip.optim_slot_table(entries)
        assert blocks == sum((s['n'] + 1023) // 1024 for s in slots)
        loss = torch.full((1,), 2.5, device=DEV) if with_loss else None
        hip.optim_multi(spec.code, spec.flags, spec.hyper, table.to(DEV), len(slots), blocks, state, reg_scale=reg_scale, loss_acc=loss)
        torch.cuda.synchronize()
        results[with_loss] = buf.cpu().numpy()
    after = results[True]
    assert np.array_equal(results[True].view(np.int32), results[False].view(np.int32))            # loss_acc = NULL changes nothing else
    written = np.zeros(total, dtype=bool)
    for s in slots:
        for sl in [s['w']] + s['s'][:n_arrays]:
            written[sl] = True
    assert np.array_equal(after[~written].view(np.int32), host[~written].view(np.int32))          # gaps, gradients, unused state areas
    reg64 = 0.0
    for s in slots:
        g32 = ref.sum_groups_f32(s['parts'])
        single_w = _t(host[s['w']].copy())
        single_s = [_t(host[k].copy()) for k in s['s']]
        hip.optim(spec.code, spec.flags, spec.hyper, single_w, _t(g32), single_s, state, l2=s['l2'])
        for name, sl, t in zip(['w', 's0', 's1', 's2'], [s['w']] + s['s'], [single_w] + single_s):
            assert np.array_equal(after[sl].view(np.int32), t.cpu().numpy().view(np.int32)), (s['n'], s['kind'], s['groups'], name)
        assert not np.array_equal(after[s['w']], host[s['w']]) or s['n'] <= 3
        if s['l2']:
            reg64 += float(np.float32(s['l2'])) * float(np.sum(host[s['w']].astype(np.float64) ** 2))
    want_loss = 2.5 + reg_scale * reg64
    got_loss = float(loss[0])
    print('loss_acc {:.9g}, float64 {:.9g}'.format(got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * want_loss


# ---- model level ------------------------------------------------------------------------------------------------------------------------

def _gcn_pair(count=1):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=3)
    models = []
    for _ in range(count):
        engine.set_seed(8)
        m = basic.BasicGCN(g['adj'], **CFG)
        helpers.randomize_biases(m, seed=1)
        models.append(m)
    return g, models


_ORACLE_START = {}


def _oracle_start():
    """The model of test_adam_steps_match_oracle in float64 and the oracle's gradient at its initial weights (computed once: the
    learning rates below are taken from it, never from the code under test)."""
    if not _ORACLE_START:
        g, (model,) = _gcn_pair()
        y = np.random.default_rng(4).integers(0, 2, len(g['u_ids']))
        gnn, head = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
        gnn = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in gnn.items()}
        gnn['layers'] = [{k: v.astype(np.float64) for k, v in lw.items()} for lw in gnn['layers']]
        head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in net] for k, net in head.items()}
        _, og, _ = otrain.loss_and_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, l2=1e-4)
        gmax = max(float(np.abs(a).max()) for a in (og['gnn']['embeddings'], og['gnn']['layers'][0]['kernel'], og['head']['clf'][-1][0]))
        _ORACLE_START.update(g=g, y=y, gnn=gnn, head=head, gmax=gmax)
    return _ORACLE_START


def _learning_rate(case, gmax):
    """A learning rate at which the rule's first step moves the watched weights by about 1e-3, from the header's formulas on zero state and
    the largest reference gradient gmax: SGD moves by lr g; Adagrad by lr g / sqrt(0.1 + g^2); RMSprop by lr g / sqrt(0.1 g^2) = 3.2 lr
    (centered: / sqrt(0.09 g^2) = 3.3 lr); Adamax, Nadam and AMSGrad by about lr."""
    rule = CASES[case][0]
    if rule == 'SGD':
        return 1e-3 / gmax
    if rule == 'Adagrad':
        return 1e-3 * np.sqrt(0.1 + gmax * gmax) / gmax
    return 3e-4 if rule == 'RMSprop' else 1e-3


@pytest.mark.parametrize('case', list(CASES))
def test_training_steps_match_the_oracle_through_the_float64_rule(hip, case):
    """test_adam_steps_match_oracle for the other rules: three train_batch steps against the oracle's float64 gradients pushed through
    tests/optimizer_ref.py.  That test allows 2e-5 after three steps of about 1e-3 each; here the bound is 2e-5 x (the largest single
    step of the float64 reference on the watched weights / 1e-3) — momentum, Nesterov and RMSprop's 3.2 lr first step make a rule's
    steps larger than its learning rate's nominal 1e-3.  The ratio is measured on the reference, never on the code under test."""
    from deep_cbrs_amar_renaissance_amd import training
    start = _oracle_start()
    g, y = start['g'], start['y']
    _, (model,) = _gcn_pair()
    gnn = dict(start['gnn'], layers=[dict(lw) for lw in start['gnn']['layers']])
    head = {k: list(net) for k, net in start['head'].items()}
    rule, hyper = CASES[case]
    lr = float(_learning_rate(case, start['gmax']))
    opt = oref.Optimizer(rule, **dict(hyper, learning_rate=lr))
    trainer = training.Trainer(model, rule=rule, **dict(hyper, learning_rate=lr))
    assert trainer.spec.rule == rule and not trainer.spec.adam
    largest = 0.0
    for t in range(1, 4):
        trainer.train_batch(g['u_ids'], g['i_ids'], y)
        _, og, _ = otrain.loss_and_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, l2=1e-4)     # (the L2 gradient is in og)
        opt.advance()
        watched = (gnn['embeddings'], gnn['layers'][0]['kernel'], head['clf'][-1][0])
        gnn['embeddings'] = opt.update('emb', gnn['embeddings'], og['gnn']['embeddings'])
        for k, lw in enumerate(gnn['layers']):
            for nm in ('kernel', 'bias'):
                lw[nm] = opt.update(('l', k, nm), lw[nm], og['gnn']['layers'][k][nm])
        for name in head:
            head[name] = [(opt.update((name, k, 'w'), w, og['head'][name][k][0]), opt.update((name, k, 'b'), b, og['head'][name][k][1]))
                          for k, (w, b) in enumerate(head[name])]
        now = (gnn['embeddings'], gnn['layers'][0]['kernel'], head['clf'][-1][0])
        largest = max(largest, max(float(np.abs(a - b).max()) for a, b in zip(now, watched)))
    bound = 2e-5 * largest / 1e-3
    got, gh = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
    errs = [float(np.abs(got['embeddings'] - gnn['embeddings']).max()),
            float(np.abs(got['layers'][0]['kernel'] - gnn['layers'][0]['kernel']).max()),
            float(np.abs(gh['clf'][-1][0] - head['clf'][-1][0]).max())]
    print('{}: lr {:.3g}, largest reference step {:.3g}, bound {:.3g}, errors {}'.format(case, lr, largest, bound, ['{:.2e}'.format(e) for e in errs]))
    assert 2e-4 < largest < 2e-2                                      # (steps of about 1e-3: the learning rate did its job)
    assert trainer.t == 3 and float(trainer._opt_state[0]) == 3
    assert all(len(a) == trainer.spec.n_arrays for a in trainer.opt_arrays.values())
    assert max(errs) < bound


@pytest.mark.parametrize('case', list(CASES))
def test_replayed_batches_equal_eager_batches(hip, case):
    """test_graph_replayed_batches_equal_eager_batches under every rule: train_batch_graphed (hipGraph replay, the rule's device state
    included) == train_batch, step for step, at that test's tolerances."""
    from deep_cbrs_amar_renaissance_amd import training
    g, models = _gcn_pair(2)
    rng = np.random.default_rng(4)
    batches = [(g['u_ids'][k * 64:(k + 1) * 64], g['i_ids'][k * 64:(k + 1) * 64], rng.integers(0, 2, 64)) for k in range(4)]
    rule, hyper = CASES[case]
    eager, graphed = (training.Trainer(m, rule=rule, **hyper) for m in models)
    loss_eager = 0.0
    for epoch in range(3):
        for u, i, y in batches:
            loss_eager += eager.train_batch(u, i, y) * len(y)
            graphed.train_batch_graphed(u, i, y)
    assert graphed._graphs and graphed.t == eager.t == 12
    assert float(graphed._opt_state[0]) == float(eager._opt_state[0]) == 12
    assert abs(graphed.pop_loss_sum() - loss_eager) < 1e-3 * abs(loss_eager)
    before = _gcn_pair()[1][0]
    for pa, pb, p0 in zip(models[0].parameters(), models[1].parameters(), before.parameters()):
        # identical kernels, identical order; only the float atomics of the embedding scatter may differ in the last bits
        assert torch.allclose(pa, pb, rtol=1e-4, atol=1e-6), tuple(pa.shape)
        assert not torch.equal(pa, p0)                                # (and it trained)


def test_replayed_head_batches_equal_eager_batches(hip):
    """HeadTrainer (BasicRS on a resident table) under Nadam, whose running product lives in the device state both paths advance."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    rng = np.random.default_rng(6)
    table = rng.standard_normal((90, 32)).astype(np.float32) * 0.5
    batches = [(rng.integers(0, 50, 64), rng.integers(50, 90, 64), rng.integers(0, 2, 64)) for _ in range(4)]
    trainers = []
    for _ in range(2):
        engine.set_seed(4)
        model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
        model((table[batches[0][0]], table[batches[0][1]]))          # builds the weights
        helpers.randomize_biases(model, seed=8)
        tr = training.HeadTrainer(model, rule='Nadam', learning_rate=2e-3)
        tr.set_tables([table])
        trainers.append(tr)
    eager, graphed = trainers
    for epoch in range(3):
        for u, i, y in batches:
            eager.train_batch(u, i, y)
            graphed.train_batch_graphed(u, i, y)
    assert graphed._graphs and graphed.t == eager.t == 12
    assert torch.equal(graphed._opt_state, eager._opt_state) and float(eager._opt_state[0]) == 12
    for pa, pb in zip(eager.model.parameters(), graphed.model.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-4, atol=1e-6), tuple(pa.shape)


def test_replayed_bpr_batches_equal_eager_batches(hip):
    """The BPR body (ids drawn on the device) under RMSprop with momentum: replayed == the same body run eagerly."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests.test_bpr_gpu import _sample_sequence
    seq = _sample_sequence()
    trainers = []
    for _ in range(2):
        engine.set_seed(8)
        model = basic.BasicGCN(seq.adj_matrix, **CFG)
        helpers.randomize_biases(model, seed=1)
        model.compile(loss=BPRLoss())
        model(seq[0][0])
        trainers.append(training.Trainer(model, rule='RMSprop', momentum=0.9))
    eager, graphed = trainers
    samplers = [tr.sampler_for(seq) for tr in trainers]
    for _ in range(12):
        eager.train_sampled(samplers[0], graph=False)
        graphed.train_sampled(samplers[1], graph=True)
    assert graphed._graphs and not eager._graphs and graphed.t == eager.t == 12
    assert float(graphed._opt_state[0]) == float(eager._opt_state[0]) == 12
    total = eager.pop_loss_sum()
    assert abs(graphed.pop_loss_sum() - total) < 1e-3 * abs(total)
    for pa, pb in zip(eager.model.parameters(), graphed.model.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-4, atol=1e-6), tuple(pa.shape)


# ---- the public surface -----------------------------------------------------------------------------------------------------------------

def _separable_task():
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(11)
    g = helpers.tiny_graph(n_users=100, n_items=80, n_ratings=4000, seed=5)
    model = basic.BasicGCN(g['adj'], **dict(CFG, l2_regularizer=1e-6))
    seq = UserItemGraph(g['ratings'], g['users'], g['items'], g['adj'], batch_size=512, shuffle=True)
    return model, seq


@pytest.mark.parametrize('name', ['SGD', 'RMSprop'])
def test_fit_learns_a_separable_task(hip, name):
    """test_fit_learns_a_separable_task compiled with SGD + momentum and with RMSprop, held to that test's thresholds.  RMSprop
    normalises every weight's step as Adam does and gets that test's 12 epochs.  SGD's steps are proportional to the gradients, which
    are small on the node table behind two Dense stacks: it first learns the label prior (loss 0.675 = the entropy of the 59 / 41
    labels) and leaves that plateau only after some 50 epochs, so it trains for 200 (8 replayed batches each: a fraction of a second)."""
    from deep_cbrs_amar_renaissance_amd import experiment
    model, seq = _separable_task()
    optimizer, epochs = (experiment.SGD(learning_rate=0.5, momentum=0.9), 200) if name == 'SGD' else (experiment.RMSprop(learning_rate=0.01), 12)
    model.compile(loss='binary_crossentropy', optimizer=optimizer, metrics=['accuracy'])
    before = model.evaluate(seq)
    hist = model.fit(seq, epochs=epochs, verbose=False)
    after = model.evaluate(seq)
    trainer = model._trainer
    assert trainer.spec.rule == name and trainer._graphs and trainer.t == epochs * len(seq)
    print(name, 'loss', hist['loss'][0], '->', hist['loss'][-1], 'evaluate', before, '->', after)
    assert hist['loss'][-1] < hist['loss'][0] - 0.02
    assert after[0] < before[0] and after[1] > max(before[1], 0.6)


def test_compiling_with_another_optimizer_trains_from_fresh_state(hip):
    from deep_cbrs_amar_renaissance_amd import experiment
    model, seq = _separable_task()
    model.compile(loss='binary_crossentropy', optimizer=experiment.Adam(learning_rate=0.01), metrics=['accuracy'])
    model.fit(seq, epochs=1, verbose=False)
    first = model._trainer
    assert first.spec.adam and first.t == len(seq) and all(len(a) == 2 for a in first.opt_arrays.values())
    model.compile(loss='binary_crossentropy', optimizer=experiment.Adam(learning_rate=0.01), metrics=['accuracy'])
    model.fit(seq, epochs=1, verbose=False)
    assert model._trainer is first and first.t == 2 * len(seq)       # an equal Adam: the trainer and its moments stay
    model.compile(loss='binary_crossentropy', optimizer=experiment.RMSprop(learning_rate=0.01, momentum=0.5, centered=True), metrics=['accuracy'])
    weights = [p.detach().clone() for p in model.parameters()]
    model.fit(seq, epochs=1, verbose=False)
    second = model._trainer
    assert second is not first and second.spec.rule == 'RMSprop' and second.t == len(seq)
    assert all(len(a) == 3 for a in second.opt_arrays.values()) and float(second._opt_state[0]) == len(seq)
    assert all(float(a[0].abs().max()) > 0 for a in second.opt_arrays.values())                     # rms of every parameter moved off zero
    assert all(not torch.equal(a, b) for a, b in zip(weights, model.parameters()))
    model.compile(loss='binary_crossentropy', optimizer=experiment.SGD(learning_rate=0.1), metrics=['accuracy'])
    model.fit(seq, epochs=1, verbose=False)
    assert model._trainer is not second and all(len(a) == 0 for a in model._trainer.opt_arrays.values()) and model._trainer.t == len(seq)


def test_experiment_runs_with_sgd(hip, tmp_path, monkeypatch):
    """The config of tests/test_experiment_gpu.py with `optimizer: {name: SGD, learning_rate, momentum}`: end to end, a finite test loss."""
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
    cfg['parameters']['optimizer'] = {'name': 'SGD', 'learning_rate': 0.05, 'momentum': 0.9, 'beta_1': 0.9}
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump({'linear': {'sgd': None}}))
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('optimizer test', str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log)
    results = multi.run()
    assert list(results) == ['sgd'] and results['sgd'] is not None
    logs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    assert len(logs) == 1
    metrics = {}
    for line in open(logs[0]):
        record = json.loads(line)
        if record['event'] == 'metrics':
            metrics.update(record['metrics'])
    assert np.isfinite(metrics['test_loss']) and metrics['test_loss'] > 0.0 and 0.0 <= metrics['test_accuracy'] <= 1.0
    assert metrics['training_time'] > 0

"""GPU: learning-rate schedules on the device — amar_lr_rates_f32 against the float64 formulas of tests/lr_schedule_ref.py, the two
advance entry points that evaluate a schedule (amar_adam_advance_lr_f32, amar_optim_advance_lr_f32) against the ones that take the rate
as an argument, fit()'s three batch steps under a schedule, a rate set between replays (LearningRateScheduler, ReduceLROnPlateau) and one
experiment through the public surface (pytest -m gpu).

The model-level tests train the tiny synthetic graph and CFG of tests/test_optimizers_gpu.py."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml

from tests import helpers
from tests import lr_schedule_ref as lref
from tests import optimizer_ref as oref
from tests.test_optimizers_gpu import CFG, _gcn_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = np.float32(-7.25)
HIGH = (1 << 24) - 64                                                 # the last 64 steps a float32 counter counts exactly


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ---- 1. amar_lr_rates_f32 ---------------------------------------------------------------------------------------------------------------

def _kernel_cases():
    """id -> (schedule at steps 0 .. 4095, schedule at the last 64 steps below 2^24), each (host object, reference on the float32-rounded
    parameters the device receives).  The large-step forms have decay_steps of the order of the step (exact in float32), so the rate
    still moves there; cosine's 2^25 keeps the step away from the end of the decay, where 1 + cos cancels and no two libms agree to a
    float32 spacing."""
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    f = lref.as_float32
    big = float(1 << 25)
    return {
        'exponential': ((S.ExponentialDecay(0.1, 1000, 0.5), lambda s: lref.exponential(s, f(0.1), 1000.0, f(0.5))),
                        (S.ExponentialDecay(0.1, 4e6, 0.5), lambda s: lref.exponential(s, f(0.1), 4e6, f(0.5)))),
        'exponential-staircase': ((S.ExponentialDecay(0.05, 7, 0.96, staircase=True), lambda s: lref.exponential(s, f(0.05), 7.0, f(0.96), True)),
                                  (S.ExponentialDecay(0.05, HIGH + 40, 0.96, staircase=True), lambda s: lref.exponential(s, f(0.05), float(HIGH + 40), f(0.96), True))),
        'inverse-time': ((S.InverseTimeDecay(0.1, 300, 0.7), lambda s: lref.inverse_time(s, f(0.1), 300.0, f(0.7))),
                         (S.InverseTimeDecay(0.1, 1, 1e-3), lambda s: lref.inverse_time(s, f(0.1), 1.0, f(1e-3)))),
        'inverse-time-staircase': ((S.InverseTimeDecay(0.1, 13, 0.3, staircase=True), lambda s: lref.inverse_time(s, f(0.1), 13.0, f(0.3), True)),
                                   (S.InverseTimeDecay(0.1, HIGH + 40, 0.3, staircase=True), lambda s: lref.inverse_time(s, f(0.1), float(HIGH + 40), f(0.3), True))),
        'polynomial': ((S.PolynomialDecay(0.1, 3000), lambda s: lref.polynomial(s, f(0.1), 3000.0, f(1e-4), 1.0)),
                       (S.PolynomialDecay(0.1, big, 0.01, power=2.5), lambda s: lref.polynomial(s, f(0.1), big, f(0.01), 2.5))),
        'polynomial-cycle': ((S.PolynomialDecay(0.1, 700, 0.01, power=0.5, cycle=True), lambda s: lref.polynomial(s, f(0.1), 700.0, f(0.01), 0.5, True)),
                             (S.PolynomialDecay(0.1, 3e6, 0.01, power=0.5, cycle=True), lambda s: lref.polynomial(s, f(0.1), 3e6, f(0.01), 0.5, True))),
        'cosine': ((S.CosineDecay(0.1, 3000), lambda s: lref.cosine(s, f(0.1), 3000.0, 0.0)),
                   (S.CosineDecay(0.1, big, alpha=0.1), lambda s: lref.cosine(s, f(0.1), big, f(0.1)))),
        'piecewise': ((S.PiecewiseConstantDecay([5, 10, 2000], [1, .5, .1, .01]), lambda s: lref.piecewise(s, [5, 10, 2000], f([1, .5, .1, .01]))),
                      (S.PiecewiseConstantDecay([HIGH + 20, HIGH + 40], [1, .5, .1]), lambda s: lref.piecewise(s, [HIGH + 20, HIGH + 40], f([1, .5, .1])))),
    }


@pytest.mark.parametrize('case', ['exponential', 'exponential-staircase', 'inverse-time', 'inverse-time-staircase', 'polynomial',
                                  'polynomial-cycle', 'cosine', 'piecewise'])
def test_lr_rates_follow_the_float64_formulas(hip, case):
    """Within 1 float32 ulp: the kernel and the reference evaluate one formula in double (pow / cos of two libms differ by about 1e-16)
    and round once, so the float32 values agree or are neighbours.  PIECEWISE copies a value: exact."""
    lr_state = torch.tensor([0.75, 0.5], device=DEV)
    for (schedule, reference), first, n in zip(_kernel_cases()[case], (0, HIGH), (4096, 64)):
        out = torch.full((n + 8,), float(SENTINEL), device=DEV)
        hip.lr_rates(hip.lr_schedule(schedule), lr_state, first, n, out)
        got = out.cpu().numpy()
        steps = np.arange(first, first + n)
        want = lref.rate32(reference(steps))
        worst = float(lref.ulps32(got[:n], want).max())
        print('{} from step {}: worst {} ulp, {} of {} differ, rates {:.6g} .. {:.6g}'.format(case, first, worst, int((got[:n] != want).sum()), n,
                                                                                     got[0], got[n - 1]))
        assert np.all(got[n:] == SENTINEL)
        assert worst <= (0 if case == 'piecewise' else 1)
        assert got[0] != got[n - 1]                                   # (the rate moves over the window: the formula is exercised)
        host = np.array([schedule(int(s)) for s in steps[:: max(1, n // 64)]])
        assert lref.ulps32(host, want[:: max(1, n // 64)]).max() <= (0 if case == 'piecewise' else 1)
    assert np.array_equal(lr_state.cpu().numpy(), np.float32([0.75, 0.5]))


def test_lr_rates_constant_reads_the_base_rate(hip):
    lr_state = torch.tensor([0.0123, 0.5], device=DEV)
    want = np.float32(0.0123)
    for first, n in ((0, 4096), (HIGH, 64)):
        out = torch.full((n + 8,), float(SENTINEL), device=DEV)
        hip.lr_rates(hip.lr_schedule(None), lr_state, first, n, out)
        got = out.cpu().numpy()
        assert np.all(got[:n] == want) and np.all(got[n:] == SENTINEL)
    with pytest.raises(ValueError):
        hip.lr_rates(hip.lr_schedule(None), lr_state, HIGH, 65)       # past 2^24
    with pytest.raises(ValueError):
        hip.lr_rates(hip.lr_schedule(None), lr_state[:1], 0, 4)
    assert hip.lr_rates(hip.lr_schedule(None), lr_state, 7, 0).numel() == 0


# ---- 2. the advance entry points --------------------------------------------------------------------------------------------------------

RULES = ['Adam', 'SGD', 'Adamax', 'Nadam', 'AMSGrad']


def _advance_pair(hip, rule, lr):
    """(advance with the rate as an argument, advance with a schedule and lr_state, state size)."""
    from deep_cbrs_amar_renaissance_amd import training
    if rule == 'Adam':
        return (lambda st: hip.adam_advance(st, lr, 0.9, 0.999),
                lambda st, sched, lr_state: hip.adam_advance_lr(st, sched, lr_state, 0.9, 0.999), 2)
    spec = training.OptimizerSpec(rule=rule, learning_rate=lr)
    other = training.OptimizerSpec(rule=rule, learning_rate=123.0)    # hyper->learning_rate is not read by the _lr entry point
    return (lambda st: hip.optim_advance(st, spec.code, spec.flags, spec.hyper),
            lambda st, sched, lr_state: hip.optim_advance_lr(st, other.code, other.flags, other.hyper, sched, lr_state), hip.OPTIM_STATE_FLOATS)


@pytest.mark.parametrize('rule', RULES)
def test_advance_under_a_constant_schedule_gives_the_bits_of_the_argument_form(hip, rule):
    lr = 2e-3
    by_argument, by_state, size = _advance_pair(hip, rule, lr)
    a, b = torch.zeros(size, device=DEV), torch.zeros(size, device=DEV)
    lr_state = torch.tensor([lr, -1.0], device=DEV)
    constant = hip.lr_schedule(None)
    for t in range(1, 11):
        by_argument(a)
        by_state(b, constant, lr_state)
        assert np.array_equal(_bits(a), _bits(b)), (t, a.cpu().numpy(), b.cpu().numpy())
        assert float(a[0]) == t
        assert np.array_equal(lr_state.cpu().numpy(), np.float32([lr, lr]))


@pytest.mark.parametrize('rule', RULES)
def test_advance_under_a_staircase_schedule(hip, rule):
    """state[0] counts; lr_state[1] is amar_lr_rates_f32 of that step, bit for bit; lr_state[0] is left alone; the scalars follow
    optimizer_ref.scalars fed the rate read back, within the ulp bounds of test_advance_counts_and_writes_the_scalars_of_the_step (Adam's
    step size is AMSGrad's)."""
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    _, by_state, size = _advance_pair(hip, rule, 0.0)
    sched = hip.lr_schedule(S.ExponentialDecay(2e-3, 3, 0.5, staircase=True))
    rates = hip.lr_rates(sched, torch.zeros(2, device=DEV), 0, 10).cpu().numpy()
    assert len(set(rates.tolist())) == 4                              # steps 0-2, 3-5, 6-8, 9
    state = torch.zeros(size, device=DEV)
    lr_state = torch.tensor([0.75, -1.0], device=DEV)
    h = oref.as_float32(oref.hyper_of('AMSGrad' if rule == 'Adam' else rule))
    p = 1.0

    def ulps(x, want):
        return abs(float(x) - float(np.float32(want))) / float(np.spacing(np.float32(want)))
    for t in range(1, 11):
        by_state(state, sched, lr_state)
        got, lrs = state.cpu().numpy(), lr_state.cpu().numpy()
        assert got[0] == t
        assert lrs.view(np.int32)[1] == rates.view(np.int32)[t - 1] and lrs[0] == np.float32(0.75)
        sc = oref.scalars('AMSGrad' if rule == 'Adam' else rule, dict(h, learning_rate=float(lrs[1])), t, p)
        p = sc.get('P', 1.0)
        assert ulps(got[1], sc['step']) <= 1
        if rule == 'Nadam':
            assert ulps(got[2], sc['mu']) <= 1 and ulps(got[3], sc['mu_next']) <= 1 and ulps(got[4], sc['P']) <= t and ulps(got[5], sc['omb2']) <= 1
            lr = float(lrs[1])
            assert ulps(got[6], lr * (1 - sc['mu']) / (1 - sc['P'])) <= 2 and ulps(got[7], lr * sc['mu_next'] / (1 - sc['P'] * sc['mu_next'])) <= 2
        else:
            assert not got[2:].any()


def test_advance_argument_checks(hip):
    from deep_cbrs_amar_renaissance_amd import training
    spec = training.OptimizerSpec(rule='SGD')
    constant = hip.lr_schedule(None)
    lr_state = torch.zeros(2, device=DEV)
    with pytest.raises(ValueError):
        hip.adam_advance_lr(torch.zeros(3, device=DEV), constant, lr_state, 0.9, 0.999)
    with pytest.raises(ValueError):
        hip.adam_advance_lr(torch.zeros(2, device=DEV), constant, torch.zeros(3, device=DEV), 0.9, 0.999)
    with pytest.raises(ValueError):
        hip.optim_advance_lr(torch.zeros(2, device=DEV), spec.code, spec.flags, spec.hyper, constant, lr_state)
    with pytest.raises(ValueError):
        hip.optim_advance_lr(torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV), hip.OPT_ADAGRAD, hip.OPT_NESTEROV, spec.hyper, constant, lr_state)
    with pytest.raises(ValueError):
        hip.optim_advance_lr(torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV), spec.code, spec.flags, spec.hyper, hip.LrSchedule(99, 0), lr_state)


# ---- 3. the trainer ---------------------------------------------------------------------------------------------------------------------

# rule -> (hyper-parameters, rate).  Adam's are exact in float32: a static-rate Adam forms the step size of its first (eager) batch on
# the host from the Python doubles, a dynamic one on the device from the float32 members, and only equal inputs can give equal bits.
TRAINED = {
    'Adam': (dict(beta_1=0.875, beta_2=1.0 - 2.0 ** -10, epsilon=1e-7), 2.0 ** -9),
    'SGD': (dict(momentum=0.9), 0.05),
    'Nadam': ({}, 2e-3),
}


def _batches(g, count=4, size=64, seed=4):
    rng = np.random.default_rng(seed)
    return [(g['u_ids'][k * size:(k + 1) * size], g['i_ids'][k * size:(k + 1) * size], rng.integers(0, 2, size)) for k in range(count)]


def _equal_models(a, b):
    return all(torch.equal(pa, pb) for pa, pb in zip(a.parameters(), b.parameters()))


@pytest.mark.parametrize('rule', list(TRAINED))
def test_a_schedule_of_one_value_trains_the_bits_of_the_plain_rate(hip, rule):
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    hyper, r = TRAINED[rule]
    g, models = _gcn_pair(2)
    before = [p.detach().clone() for p in models[0].parameters()]
    plain = training.Trainer(models[0], rule=rule, learning_rate=r, **hyper)
    sched = training.Trainer(models[1], rule=rule, learning_rate=S.PiecewiseConstantDecay([3], [r, r]), **hyper)
    assert not plain.dynamic_rate and sched.dynamic_rate
    batches = _batches(g, count=3)
    for k in range(6):
        u, i, y = batches[k % 3]
        plain.train_batch_graphed(u, i, y)
        sched.train_batch_graphed(u, i, y)
        assert _equal_models(*models), (rule, k)
    assert plain.t == sched.t == 6 and plain.capture_count == sched.capture_count == 1
    assert not any(torch.equal(a, b) for a, b in zip(before, models[0].parameters()))
    assert sched.pop_learning_rate() == float(np.float32(r)) and sched.get_learning_rate() == float(np.float32(r))


def test_the_first_step_is_step_zero(hip):
    """PiecewiseConstantDecay([2], [r, 0]) under plain SGD on a model without L2: steps 0, 1, 2 move the weights, from step 3 on no
    bit changes (w - 0 * g = w) — the schedule is read at the zero-based step, through the eager first batch and the replayed ones."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=3)
    engine.set_seed(8)
    model = basic.BasicGCN(g['adj'], **dict(CFG, l2_regularizer=0.0))
    helpers.randomize_biases(model, seed=1)
    trainer = training.Trainer(model, rule='SGD', learning_rate=S.PiecewiseConstantDecay([2], [0.05, 0.0]))
    assert all(trainer._l2(p) == 0.0 for p in trainer.params)
    batches = _batches(g, count=3)
    moved, rates = [], []
    for k in range(6):
        last = [p.detach().clone() for p in model.parameters()]
        trainer.train_batch_graphed(*batches[k % 3])
        moved.append(any(not torch.equal(a, b) for a, b in zip(last, model.parameters())))
        rates.append(trainer.pop_learning_rate())
    assert moved == [True, True, True, False, False, False]
    assert rates == [float(np.float32(0.05))] * 3 + [0.0] * 3 and trainer.capture_count == 1


@pytest.mark.parametrize('rule', list(TRAINED))
def test_replayed_batches_equal_eager_batches_under_a_schedule(hip, rule):
    """train_batch (eager: amar_*_advance_lr_f32, then the single-tensor updates reading the device state) against train_batch_graphed
    (the replayed graph), twelve batches under ExponentialDecay(decay_steps=2, staircase=True): the same weights, optimizer state and
    rate state, bit for bit."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    hyper, r = TRAINED[rule]
    g, models = _gcn_pair(2)
    schedule = S.ExponentialDecay(r, 2, 0.5, staircase=True)
    eager, graphed = (training.Trainer(m, rule=rule, learning_rate=schedule, **hyper) for m in models)
    batches = _batches(g)
    for k in range(12):
        u, i, y = batches[k % 4]
        eager.train_batch(u, i, y)
        graphed.train_batch_graphed(u, i, y)
        worst = max(float((pa - pb).abs().max()) for pa, pb in zip(models[0].parameters(), models[1].parameters()))
        print('{} step {}: max |eager - replayed| = {:.3g}'.format(rule, k, worst))
        assert _equal_models(*models), (rule, k)
        assert torch.equal(eager._lr_state, graphed._lr_state)
        assert lref.ulps32(graphed._lr_state[1:].cpu().numpy(), [schedule(k)]).max() <= 1
    assert graphed._graphs and not eager._graphs and graphed.t == eager.t == 12
    assert torch.equal(eager._opt_state, graphed._opt_state) and float(eager._opt_state[0]) == 12


def test_replayed_head_and_bpr_loops_follow_a_schedule(hip):
    """The other two training loops: HeadTrainer on a resident table and the BPR-sampled body, replayed against eager, under a
    schedule that changes every second step."""
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests.test_bpr_gpu import _sample_sequence
    schedule = S.ExponentialDecay(2e-3, 2, 0.5, staircase=True)
    rng = np.random.default_rng(6)
    table = rng.standard_normal((90, 32)).astype(np.float32) * 0.5
    batches = [(rng.integers(0, 50, 64), rng.integers(50, 90, 64), rng.integers(0, 2, 64)) for _ in range(4)]
    trainers = []
    for _ in range(2):
        engine.set_seed(4)
        model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
        model((table[batches[0][0]], table[batches[0][1]]))
        helpers.randomize_biases(model, seed=8)
        tr = training.HeadTrainer(model, rule='Nadam', learning_rate=schedule)
        tr.set_tables([table])
        trainers.append(tr)
    eager, graphed = trainers
    for k in range(8):
        eager.train_batch(*batches[k % 4])
        graphed.train_batch_graphed(*batches[k % 4])
    assert graphed._graphs and torch.equal(graphed._opt_state, eager._opt_state) and torch.equal(graphed._lr_state, eager._lr_state)
    assert lref.ulps32(graphed._lr_state[1:].cpu().numpy(), [schedule(7)]).max() <= 1 and _equal_models(eager.model, graphed.model)
    seq = _sample_sequence()
    trainers = []
    for _ in range(2):
        engine.set_seed(8)
        model = basic.BasicGCN(seq.adj_matrix, **CFG)
        helpers.randomize_biases(model, seed=1)
        model.compile(loss=BPRLoss())
        model(seq[0][0])
        trainers.append(training.Trainer(model, rule='Adam', learning_rate=schedule))
    eager, graphed = trainers
    samplers = [tr.sampler_for(seq) for tr in trainers]
    for _ in range(8):
        eager.train_sampled(samplers[0], graph=False)
        graphed.train_sampled(samplers[1], graph=True)
    assert graphed._graphs and not eager._graphs and graphed.capture_count == 1
    assert torch.equal(graphed._opt_state, eager._opt_state) and torch.equal(graphed._lr_state, eager._lr_state)
    assert lref.ulps32(graphed._lr_state[1:].cpu().numpy(), [schedule(7)]).max() <= 1 and _equal_models(eager.model, graphed.model)


# ---- 4. setting the rate ----------------------------------------------------------------------------------------------------------------

def _fit_task(optimizer, shuffle=False, seed=11):
    """BasicGCN on 1 536 ratings in three batches of 512 (one shape: one capture), compiled with `optimizer`."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(seed)
    g = helpers.tiny_graph(n_users=100, n_items=80, n_ratings=1536, seed=5)
    model = basic.BasicGCN(g['adj'], **dict(CFG, l2_regularizer=1e-6))
    seq = UserItemGraph(g['ratings'], g['users'], g['items'], g['adj'], batch_size=512, shuffle=shuffle)
    assert len(seq) == 3
    model.compile(loss='binary_crossentropy', optimizer=optimizer, metrics=['accuracy'])
    return g, model, seq


class _Captures:
    def __init__(self):
        self.counts = []

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        self.counts.append(self.model._trainer.capture_count)
        self.logs = dict(logs)


def test_learning_rate_scheduler_equals_the_piecewise_schedule(hip):
    from deep_cbrs_amar_renaissance_amd import experiment as ex, training
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    from deep_cbrs_amar_renaissance_amd.utilities.keras import LearningRateScheduler
    rates = [0.01, 0.004, 0.0005]
    n = 3
    _, by_callback, seq_a = _fit_task(ex.Adam(learning_rate=0.02))
    _, by_schedule, seq_b = _fit_task(ex.Adam(learning_rate=S.PiecewiseConstantDecay([n - 1, 2 * n - 1], rates)))
    spy = _Captures()
    ha = by_callback.fit(seq_a, epochs=3, verbose=False, callbacks=[LearningRateScheduler(lambda epoch, lr: rates[epoch]), spy])
    hb = by_schedule.fit(seq_b, epochs=3, verbose=False)
    want = [float(np.float32(r)) for r in rates]
    assert ha['lr'] == want and hb['lr'] == want and spy.logs['lr'] == want[-1]
    assert ha['loss'] == hb['loss'] and _equal_models(by_callback, by_schedule)
    trainer = by_callback._trainer
    # one shape, one capture — made under the first set rate; the sets of epochs 1 and 2 add none
    assert spy.counts == [1, 1, 1] and trainer.capture_count == 1 and trainer.t == 9
    # a set is one float on the device: moments, step count and captured graphs stay, and the rate holds across fit() calls
    moments = [a[0].clone() for a in trainer.opt_arrays.values()]
    training.set_learning_rate(by_callback, 0.003)
    assert training.get_learning_rate(by_callback) == float(np.float32(0.003))
    assert trainer.t == 9 and trainer.capture_count == 1 and all(torch.equal(a, b) for a, b in zip(moments, (a[0] for a in trainer.opt_arrays.values())))
    assert float(trainer._opt_state[0]) == 9
    again = by_callback.fit(seq_a, epochs=1, verbose=False)
    assert by_callback._trainer is trainer and again['lr'] == [float(np.float32(0.003))] and trainer.capture_count == 1 and trainer.t == 12
    # under a schedule the rate cannot be set (as in Keras), and is read off the schedule
    with pytest.raises(ValueError):
        training.set_learning_rate(by_schedule, 0.01)
    assert training.get_learning_rate(by_schedule) == want[-1]
    with pytest.raises(ValueError):
        by_schedule.fit(seq_b, epochs=1, verbose=False, callbacks=[LearningRateScheduler(lambda epoch, lr: 0.01)])


def test_the_first_set_drops_the_captured_graphs_once(hip):
    from deep_cbrs_amar_renaissance_amd import experiment as ex, training
    _, model, seq = _fit_task(ex.SGD(learning_rate=0.05, momentum=0.9))
    h = model.fit(seq, epochs=1, verbose=False)
    trainer = model._trainer
    assert 'lr' not in h and not trainer.dynamic_rate and trainer.capture_count == 1
    assert training.get_learning_rate(model) == float(np.float32(0.05))
    state = trainer._opt_state.clone()
    arrays = [a[0].clone() for a in trainer.opt_arrays.values()]
    training.set_learning_rate(model, 0.02)
    assert trainer.dynamic_rate and not trainer._graphs and trainer.t == 3
    assert torch.equal(state, trainer._opt_state) and all(torch.equal(a, b[0]) for a, b in zip(arrays, trainer.opt_arrays.values()))
    h = model.fit(seq, epochs=2, verbose=False)
    assert model._trainer is trainer and h['lr'] == [float(np.float32(0.02))] * 2 and trainer.capture_count == 2 and trainer.t == 9
    training.set_learning_rate(model, 0.01)
    h = model.fit(seq, epochs=1, verbose=False)
    assert h['lr'] == [float(np.float32(0.01))] and trainer.capture_count == 2
    with pytest.raises(ValueError):
        training.set_learning_rate(model, float('nan'))


def test_a_rate_set_in_mid_fit_fills_the_history(hip):
    """A callback of the caller's own that sets the rate after epoch 1: the epochs before it ran at the compiled rate and say so."""
    from deep_cbrs_amar_renaissance_amd import experiment as ex, training

    class SetAfter:
        def set_model(self, model):
            self.model = model

        def on_epoch_end(self, epoch, logs=None):
            if epoch == 1:
                training.set_learning_rate(self.model, 0.02)
    _, model, seq = _fit_task(ex.SGD(learning_rate=0.05))
    h = model.fit(seq, epochs=4, verbose=False, callbacks=[SetAfter()])
    assert h['lr'] == [float(np.float32(r)) for r in (0.05, 0.05, 0.02, 0.02)] and len(h['loss']) == 4
    assert model._trainer.capture_count == 2 and model._trainer.t == 12


def test_reduce_lr_on_plateau_in_fit(hip):
    """patience=1, factor=0.5 and a min_delta no epoch can beat: epoch 0 sets best (anything beats +inf), every later epoch waits once and
    halves the rate, down to min_lr.  history['lr'] is the rate each epoch trained with."""
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.utilities.keras import ReduceLROnPlateau
    g, model, seq = _fit_task(ex.Adam(learning_rate=0.01), shuffle=True)
    val = UserItemGraph(g['ratings'][:256], g['users'], g['items'], g['adj'], batch_size=128)
    cb = ReduceLROnPlateau(monitor='val_loss', factor=0.5, patience=1, min_delta=1e9, min_lr=0.002)
    h = model.fit(seq, epochs=6, verbose=False, validation_data=val, callbacks=[cb])
    f = lambda x: float(np.float32(x))   # noqa: E731
    want = [f(0.01), f(0.01), f(f(0.01) * 0.5), f(f(f(0.01) * 0.5) * 0.5), f(0.002), f(0.002)]
    print('lr', h['lr'], 'val_loss', h['val_loss'])
    assert h['lr'] == want and len(h['val_loss']) == 6
    assert model._trainer.get_learning_rate() == f(0.002) and model._trainer.capture_count == 1


def test_a_static_fit_returns_the_keys_it_always_did(hip):
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    _, model, seq = _fit_task(ex.Adam(learning_rate=0.01))
    h = model.fit(seq, epochs=2, verbose=False)
    assert list(h) == ['loss', 'accuracy'] and not model._trainer.dynamic_rate and model._trainer._lr_state is None
    _, model, seq = _fit_task(ex.Adam(learning_rate=0.01, decay=0.5))
    h = model.fit(seq, epochs=2, verbose=False)
    assert list(h) == ['loss', 'accuracy', 'lr']
    assert h['lr'] == [float(np.float32(lref.inverse_time(s, lref.as_float32(0.01), 1.0, 0.5)[0])) for s in (2, 5)]


# ---- 5. experiment ----------------------------------------------------------------------------------------------------------------------

def test_experiment_with_a_schedule_mapping_and_reduce_lr(hip, tmp_path, monkeypatch):
    """`parameters.optimizer.learning_rate` as a mapping together with `parameters.validation.reduce_lr`: the run completes and logs `lr`
    with every epoch's values.  The rate logged is the one ReduceLROnPlateau reports, the rate in force after the epoch: the schedule at
    the step count.  (With its default min_delta and a patience of 5 the callback does not come to reduce, which a schedule refuses.)"""
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:12000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:2000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update({k: v for k, v in paths.items() if k != 'props_triples_filepath'})
    cfg['dataset'].update({'load_function_name': 'load_user_item_graph', 'graph_filepath': 'unused.json', 'bert_user_filepath': 'unused.json',
                           'bert_item_filepath': 'unused.json'})
    cfg['model'].update({'name': 'basic.BasicGCN', 'embedding_dim': 8, 'n_hiddens': [8, 8], 'dense_units': [24, 24], 'clf_units': [48, 48]})
    cfg['parameters']['epochs'] = 3
    mapping = {'name': 'ExponentialDecay', 'initial_learning_rate': 0.01, 'decay_steps': 5, 'decay_rate': 0.5, 'staircase': True}
    cfg['parameters']['optimizer'] = {'name': 'Adam', 'learning_rate': mapping}
    cfg['parameters']['validation'] = {'fraction': 0.1, 'reduce_lr': {'monitor': 'val_loss', 'factor': 0.5, 'patience': 5}}
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump({'linear': {'schedule': None}}))
    seen = {}
    original = experiment.Experimenter.train

    def spy(self):
        seen['exp'] = self
        return original(self)
    monkeypatch.setattr(experiment.Experimenter, 'train', spy)
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('lr test', str(tmp_path / 'mlruns'))
    results = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log).run()
    assert list(results) == ['schedule'] and results['schedule'] is not None
    exp = seen['exp']
    schedule = S.ExponentialDecay(0.01, 5, 0.5, staircase=True)
    trainer = exp.model._trainer
    assert trainer.spec.schedule == schedule and trainer.dynamic_rate and trainer.t == 3 * len(exp.trainset)
    logs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    assert len(logs) == 1
    steps, final = {}, {}
    for line in open(logs[0]):
        record = json.loads(line)
        if record['event'] == 'metrics' and 'step' in record:
            steps[record['step']] = record['metrics']
        elif record['event'] == 'metrics':
            final.update(record['metrics'])
    n = len(exp.trainset)
    assert sorted(steps) == [0, 1, 2] and all('val_loss' in steps[e] and 'loss' in steps[e] for e in steps)
    assert [steps[e]['lr'] for e in range(3)] == [float(schedule((e + 1) * n)) for e in range(3)]
    assert steps[2]['lr'] < steps[0]['lr'] < 0.01
    assert np.isfinite(final['test_loss']) and final['training_time'] > 0

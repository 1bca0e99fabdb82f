"""Optimizers, host side: the numpy restatement of the rules (tests/optimizer_ref.py) against torch.optim where the two are algebraically
identical and against steps written out by hand elsewhere, and the surface the feature adds (classes, resolution, declarations)."""
import math
import os
import re

import numpy as np
import pytest

from tests import optimizer_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_ref(rule, w0, grads, l2=0.0, **hyper):
    opt = oref.Optimizer(rule, **hyper)
    w, trace = np.array(w0, dtype=np.float64), []
    for g in grads:
        opt.advance()
        w = opt.update('w', w, g, l2)
        trace.append(w.copy())
    return trace, opt


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize('kind', ['sgd', 'sgd-momentum', 'sgd-nesterov', 'adagrad'])
def test_rules_shared_with_torch_optim_agree(kind):
    """torch.optim.SGD keeps buf = momentum buf + g and steps by -lr buf: with a constant learning rate that is Keras' a = -lr buf; its
    Adagrad is Keras' with lr_decay = 0.  Float64 on the CPU, 5 steps, 1e-12 relative."""
    import torch
    rng = np.random.default_rng(3)
    w0, grads = rng.standard_normal(17), rng.standard_normal((5, 17))
    if kind == 'adagrad':
        hyper = dict(learning_rate=0.05, initial_accumulator_value=0.1, epsilon=1e-7)
        trace, _ = _run_ref('Adagrad', w0, grads, **hyper)
        p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
        topt = torch.optim.Adagrad([p], lr=0.05, lr_decay=0.0, initial_accumulator_value=0.1, eps=1e-7)
    else:
        hyper = dict(learning_rate=0.05, momentum=0.0 if kind == 'sgd' else 0.9, nesterov=kind == 'sgd-nesterov')
        trace, _ = _run_ref('SGD', w0, grads, **hyper)
        p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
        topt = torch.optim.SGD([p], lr=0.05, momentum=hyper['momentum'], nesterov=hyper['nesterov'])
    for k, g in enumerate(grads):
        p.grad = torch.tensor(g, dtype=torch.float64)
        topt.step()
        assert _rel(trace[k], p.detach().numpy()) < 1e-12, (kind, k)


W0 = (0.5, -1.25, 2.0)
G1 = (0.3, -0.02, 1.5)
G2 = (-0.1, 0.04, 1.0)


@pytest.mark.parametrize('centered', [False, True])
@pytest.mark.parametrize('momentum', [0.0, 0.8])
def test_rmsprop_first_and_second_step_by_hand(centered, momentum):
    lr, rho, eps = 0.01, 0.9, 1e-7
    trace, opt = _run_ref('RMSprop', W0, [G1, G2], learning_rate=lr, rho=rho, momentum=momentum, epsilon=eps, centered=centered)
    for e in range(3):
        w, rms, mg, mom = W0[e], 0.0, 0.0, 0.0
        for k, g in enumerate((G1[e], G2[e])):
            rms = rho * rms + (1 - rho) * g * g
            mg = rho * mg + (1 - rho) * g
            d = max(rms - mg * mg, 0.0) if centered else rms
            if momentum:
                mom = momentum * mom + lr * g / math.sqrt(d + eps)           # epsilon inside the root
                w = w - mom
            else:
                w = w - lr * g / (math.sqrt(d) + eps)
            assert abs(trace[k][e] - w) <= 1e-14 * abs(w), (e, k)
        assert abs(opt.state['w'][0][e] - rms) <= 1e-15 * rms
    # the first step from zero state in closed form: rms = 0.1 g^2, so w moves by lr g / (sqrt(0.1) |g| + eps) without momentum
    if not centered and not momentum:
        assert abs(trace[0][0] - (0.5 - 0.01 * 0.3 / (math.sqrt(0.1) * 0.3 + 1e-7))) < 1e-15
    assert oref.state_names('RMSprop', opt.h) == ['rms'] + (['mg'] if centered else []) + (['mom'] if momentum else [])


def test_adamax_first_and_second_step_by_hand():
    lr, b1, b2, eps = 0.002, 0.9, 0.999, 1e-7
    trace, _ = _run_ref('Adamax', W0, [G1, G2], learning_rate=lr, beta_1=b1, beta_2=b2, epsilon=eps)
    for e in range(3):
        w, m, u = W0[e], 0.0, 0.0
        for k, g in enumerate((G1[e], G2[e])):
            t = k + 1
            m = b1 * m + (1 - b1) * g
            u = max(b2 * u, abs(g))
            w = w - (lr / (1 - b1 ** t)) * m / (u + eps)
            assert abs(trace[k][e] - w) <= 1e-14 * abs(w), (e, k)
    # first step: m / (1 - b1) = g and u = |g|: every weight moves by lr against its gradient's sign (up to epsilon)
    assert abs(trace[0][2] - (2.0 - 0.002 * 1.5 / (1.5 + 1e-7))) < 1e-15


def test_nadam_first_and_second_step_by_hand():
    lr, b1, b2, eps = 0.002, 0.9, 0.999, 1e-7
    trace, opt = _run_ref('Nadam', W0, [G1, G2], learning_rate=lr, beta_1=b1, beta_2=b2, epsilon=eps)
    mu = [b1 * (1 - 0.5 * 0.96 ** (0.004 * t)) for t in (1, 2, 3)]
    assert abs(mu[0] - 0.9 * (1 - 0.5 * math.exp(0.004 * math.log(0.96)))) < 1e-15 and 0.45 < mu[0] < mu[1] < mu[2] < 0.4503
    for e in range(3):
        w, m, v, p = W0[e], 0.0, 0.0, 1.0
        for k, g in enumerate((G1[e], G2[e])):
            t = k + 1
            p = p * mu[k]                                                       # P_t, the running product
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            bar = (1 - mu[k]) * g / (1 - p) + mu[k + 1] * m / (1 - p * mu[k + 1])
            w = w - lr * bar / (math.sqrt(v / (1 - b2 ** t)) + eps)
            assert abs(trace[k][e] - w) <= 1e-14 * abs(w), (e, k)
    assert abs(opt.p - mu[0] * mu[1]) < 1e-16                                   # kept across steps


def test_amsgrad_first_and_second_step_by_hand():
    lr, b1, b2, eps = 0.002, 0.9, 0.999, 1e-7
    g2 = (-0.1, 0.04, 0.0)                                                      # a zero gradient: v falls below vhat, vhat stays
    trace, opt = _run_ref('AMSGrad', W0, [G1, g2], learning_rate=lr, beta_1=b1, beta_2=b2, epsilon=eps)
    for e in range(3):
        w, m, v, vhat = W0[e], 0.0, 0.0, 0.0
        for k, g in enumerate((G1[e], g2[e])):
            t = k + 1
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            vhat = max(vhat, v)
            w = w - (lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)) * m / (math.sqrt(vhat) + eps)
            assert abs(trace[k][e] - w) <= 1e-14 * abs(w), (e, k)
    m_, v_, vhat_ = opt.state['w']
    assert v_[2] < vhat_[2] == (1 - b2) * 1.5 * 1.5 and v_[0] == vhat_[0]
    # the first step equals Adam's (oracle.train.adam_update)
    from oracle import train as otrain
    want, _, _ = otrain.adam_update(np.array(W0), np.array(G1), np.zeros(3), np.zeros(3), 1, lr=lr, b1=b1, b2=b2, eps=eps)
    assert _rel(trace[0], want) < 1e-14


def test_l2_enters_the_gradient_first():
    trace, _ = _run_ref('SGD', W0, [G1], l2=0.25, learning_rate=0.1)
    assert np.allclose(trace[0], [w - 0.1 * (g + 2 * 0.25 * w) for w, g in zip(W0, G1)], rtol=1e-15, atol=0)


def test_scales_bound_a_float32_evaluation():
    """The per-element scales the GPU tests divide by: a float32 numpy evaluation of the same formulas stays far inside 1e-6 of them."""
    rng = np.random.default_rng(5)
    n = 2000
    for rule, hyper in (('SGD', dict(momentum=0.9, nesterov=True)), ('RMSprop', dict(momentum=0.9, centered=True)), ('Adagrad', {}),
                        ('Adamax', {}), ('Nadam', {}), ('AMSGrad', {})):
        h = oref.as_float32(oref.hyper_of(rule, **hyper))
        sc = oref.scalars(rule, h, 3, 0.45 * 0.45)
        w, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        arrays = [(rng.standard_normal(n) * 0.1).astype(np.float32) for _ in oref.state_names(rule, h)]
        names = oref.state_names(rule, h)
        for k, name in enumerate(names):
            if name in ('rms', 'acc', 'u', 'v', 'vhat'):
                arrays[k] = (arrays[names.index('mg')] ** 2 if name == 'rms' and 'mg' in names else 0) + rng.uniform(0.05, 1, n).astype(np.float32)
        want_w, want_s = oref.step(rule, h, sc, w, g, arrays, 1e-3)
        sw, ss = oref.scales(rule, h, sc, w, g, arrays, 1e-3)
        assert all((s_ >= np.abs(a_) * (1 - 1e-12)).all() for s_, a_ in zip(ss, want_s))
        got_w = np.float32(want_w)                                              # storing the exact result in float32 costs 6e-8 |w|
        assert float((np.abs(got_w.astype(np.float64) - want_w) / sw).max()) < 1e-7


# ---- the surface ----------------------------------------------------------------------------------------------------------------------

def test_constructor_defaults_are_keras():
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    assert vars(ex.SGD()) == dict(learning_rate=0.01, momentum=0.0, nesterov=False)
    assert vars(ex.RMSprop()) == dict(learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False)
    assert vars(ex.Adagrad()) == dict(learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7)
    for cls in (ex.Adamax, ex.Nadam):
        assert vars(cls()) == dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    assert vars(ex.Adam()) == dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False)
    assert ex.Adam().rule == 'Adam' and ex.Adam(amsgrad=True).rule == 'AMSGrad'
    for name, defaults in oref.DEFAULTS.items():                               # the reference restates the same table
        if name != 'AMSGrad':
            assert vars(getattr(ex, name)()) == defaults


def _experimenter_stub(optimizer_cfg):
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    stub = ex.Experimenter.__new__(ex.Experimenter)
    stub.config = ex.AttrDict({'parameters': {'optimizer': optimizer_cfg}})
    stub.optimizer_class = ex.optimizer_class(optimizer_cfg['name'])
    return stub


def test_every_name_resolves_and_config_keys_pass_the_filter():
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    assert set(ex.OPTIMIZERS) == {'Adam', 'SGD', 'RMSprop', 'Adagrad', 'Adamax', 'Nadam'}
    for name in ('SGD', 'RMSprop', 'Adagrad', 'Adamax', 'Nadam', 'Adam'):
        stub = _experimenter_stub({'name': name, 'learning_rate': 0.125, 'beta_1': 0.8, 'momentum': 0.5})
        stub.build_optimizer()                                               # keys the class does not take are dropped, as in the reference
        assert type(stub.optimizer) is ex.OPTIMIZERS[name] and stub.optimizer.learning_rate == 0.125
        assert getattr(stub.optimizer, 'beta_1', 0.8) == 0.8 and getattr(stub.optimizer, 'momentum', 0.5) == 0.5
    stub = _experimenter_stub({'name': 'Adam', 'learning_rate': 0.001, 'amsgrad': True})
    stub.build_optimizer()
    assert stub.optimizer.amsgrad is True and stub.optimizer.rule == 'AMSGrad'
    stub = _experimenter_stub({'name': 'SGD', 'learning_rate': 0.1, 'momentum': 0.9, 'nesterov': True})
    stub.build_optimizer()
    assert (stub.optimizer.momentum, stub.optimizer.nesterov) == (0.9, True)


@pytest.mark.parametrize('name', ['Adadelta', 'Ftrl', 'adam'])
def test_an_unknown_name_says_what_is_supported(name):
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    with pytest.raises(ValueError) as err:
        ex.optimizer_class(name)
    assert all(known in str(err.value) for known in ex.OPTIMIZERS) and name in str(err.value)


def test_trainer_spec_reads_objects_and_keywords():
    import types
    from deep_cbrs_amar_renaissance_amd import capi, experiment as ex, training
    spec = training.OptimizerSpec(types.SimpleNamespace(learning_rate=5e-3, beta_1=0.8))      # no rule name: Adam
    assert spec.rule == 'Adam' and spec.adam and spec.n_arrays == 2
    assert spec.values == dict(learning_rate=5e-3, beta_1=0.8, beta_2=0.999, epsilon=1e-7)
    assert training.OptimizerSpec(None).key == training.OptimizerSpec(ex.Adam()).key
    assert training.OptimizerSpec(ex.Adam()).key != training.OptimizerSpec(ex.Adam(learning_rate=0.01)).key
    assert training.OptimizerSpec(ex.Adam()).key != training.OptimizerSpec(ex.Adam(amsgrad=True)).key
    want = {('SGD', ()): 0, ('SGD', (('momentum', 0.9),)): 1, ('RMSprop', ()): 1, ('RMSprop', (('centered', True),)): 2,
            ('RMSprop', (('momentum', 0.5),)): 2, ('RMSprop', (('centered', True), ('momentum', 0.5))): 3, ('Adagrad', ()): 1,
            ('Adamax', ()): 2, ('Nadam', ()): 2}
    for (name, kw), count in want.items():
        opt = getattr(ex, name)(**dict(kw))
        spec = training.OptimizerSpec(opt)
        assert (spec.rule, spec.n_arrays) == (name, count) and not spec.adam
        assert spec.n_arrays == len(oref.state_names(name, oref.hyper_of(name, **dict(kw))))
    assert training.OptimizerSpec(ex.Adam(amsgrad=True)).n_arrays == 3
    nest = training.OptimizerSpec(rule='SGD', learning_rate=0.1, momentum=0.9, nesterov=True)
    assert nest.flags == capi.OPT_NESTEROV and nest.code == capi.OPT_SGD and abs(nest.hyper.momentum - 0.9) < 1e-7
    with pytest.raises(ValueError):
        training.OptimizerSpec(rule='Adadelta')
    with pytest.raises(TypeError):
        training.OptimizerSpec(rule='SGD', beta_1=0.9)


def test_argument_checks_need_no_device():
    from deep_cbrs_amar_renaissance_amd import capi
    lib = capi.load()
    assert lib.amar_optim_state_arrays(99, 0, 0.0) == -1                       # AMAR_EINVAL: no such rule
    assert lib.amar_optim_state_arrays(capi.OPT_SGD, capi.OPT_CENTERED, 0.0) == -1         # a flag of another rule
    assert lib.amar_optim_state_arrays(capi.OPT_SGD, 0, -0.5) == -1
    assert lib.amar_optim_state_arrays(capi.OPT_SGD, capi.OPT_NESTEROV, 0.0) == 0          # nesterov without momentum: plain SGD
    hyper = capi.optim_hyper()
    import ctypes
    assert lib.amar_optim_advance_f32(None, capi.OPT_SGD, 0, ctypes.byref(hyper), None) == -1
    assert lib.amar_optim_f32(capi.OPT_SGD, 0, None, None, None, None, None, None, 4, None, 0.0, None) == -1
    assert lib.amar_optim_f32(capi.OPT_SGD, 0, ctypes.byref(hyper), None, None, None, None, None, -1, None, 0.0, None) == -1
    assert lib.amar_optim_multi_f32(77, 0, ctypes.byref(hyper), None, 1, 1, None, 0.0, None, None) == -1
    assert ctypes.sizeof(capi.OptimSlot) == 64 and ctypes.sizeof(capi.OptimHyper) == 24
    # Adam as a rule: no flags, two arrays, refused like the others by every entry point that takes a rule
    assert capi.optim_state_arrays(capi.OPT_ADAM) == 2 and lib.amar_optim_state_arrays(capi.OPT_ADAM, 0, 0.9) == 2
    sched, dummy = capi.lr_schedule(None), ctypes.c_void_p(64)       # (a non-null address: the checks return before anything reads it)
    for flag in (capi.OPT_NESTEROV, capi.OPT_CENTERED, 1):
        assert lib.amar_optim_state_arrays(capi.OPT_ADAM, flag, 0.0) == -1
        assert lib.amar_optim_advance_f32(dummy, capi.OPT_ADAM, flag, ctypes.byref(hyper), None) == -1
        assert lib.amar_optim_f32(capi.OPT_ADAM, flag, ctypes.byref(hyper), dummy, dummy, dummy, dummy, None, 4, dummy, 0.0, None) == -1
        assert lib.amar_optim_multi_f32(capi.OPT_ADAM, flag, ctypes.byref(hyper), dummy, 1, 1, dummy, 0.0, None, None) == -1
        assert lib.amar_optim_advance_lr_f32(dummy, capi.OPT_ADAM, flag, ctypes.byref(hyper), ctypes.byref(sched), dummy, None) == -1
    assert lib.amar_optim_f32(capi.OPT_ADAM, 0, ctypes.byref(hyper), dummy, dummy, dummy, None, None, 4, dummy, 0.0, None) == -1   # needs s1
    assert lib.amar_optim_f32(capi.OPT_ADAM, 0, ctypes.byref(hyper), dummy, dummy, dummy, dummy, None, 0, dummy, 0.0, None) == 0   # n = 0


def test_spec_keys_are_what_cached_trainers_were_stored_under():
    """OptimizerSpec.key of eight representative specs, as literals taken from the commit before Adam became a rule of the shared
    kernels: a cached trainer is reused by this key."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    adam = (('beta_1', 0.9), ('beta_2', 0.999), ('epsilon', 1e-07), ('learning_rate', 0.001))
    adam32 = (('beta_1', 0.9), ('beta_2', 0.999), ('epsilon', 1e-07), ('learning_rate', 0.0010000000474974513))
    S_ = training.OptimizerSpec
    assert S_().key == ('Adam', adam, None)
    assert S_(learning_rate=S.ExponentialDecay(1e-3, 100, 0.9)).key == ('Adam', adam32, None, ('ExponentialDecay', 0.001, 100, 0.9, False))
    assert S_(decay=1e-4).key == ('Adam', adam32, None, ('InverseTimeDecay', 0.001, 1, 0.0001, False))
    assert S_(clipnorm=1.0).key == ('Adam', adam, ('clipnorm', 1.0))
    assert S_(rule='AMSGrad').key == ('AMSGrad', adam, None)
    assert S_(rule='SGD', momentum=0.9, nesterov=True).key == ('SGD', (('learning_rate', 0.01), ('momentum', 0.9), ('nesterov', True)), None)
    assert S_(rule='RMSprop', centered=True, momentum=0.5).key == \
        ('RMSprop', (('centered', True), ('epsilon', 1e-07), ('learning_rate', 0.001), ('momentum', 0.5), ('rho', 0.9)), None)
    assert S_(rule='Nadam').key == ('Nadam', adam, None)
    spec = S_()
    assert spec.adam and (spec.code, spec.flags, spec.n_arrays) == (7, 0, 2)
    with pytest.raises(AttributeError):
        spec.adam = False                                            # read-only


def test_new_entry_points_are_declared_and_bound():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    declared = set(re.findall(r'\b(amar_[a-z0-9_]+)\s*\(', header))
    for name in ('amar_optim_advance_f32', 'amar_optim_f32', 'amar_optim_multi_f32', 'amar_optim_state_arrays'):
        assert name in capi.SIGNATURES, name
        assert name in declared, name
    for define, value in (('AMAR_OPT_SGD', capi.OPT_SGD), ('AMAR_OPT_RMSPROP', capi.OPT_RMSPROP), ('AMAR_OPT_ADAGRAD', capi.OPT_ADAGRAD),
                          ('AMAR_OPT_ADAMAX', capi.OPT_ADAMAX), ('AMAR_OPT_NADAM', capi.OPT_NADAM), ('AMAR_OPT_AMSGRAD', capi.OPT_AMSGRAD), ('AMAR_OPT_ADAM', capi.OPT_ADAM),
                          ('AMAR_OPT_NESTEROV', capi.OPT_NESTEROV), ('AMAR_OPT_CENTERED', capi.OPT_CENTERED),
                          ('AMAR_OPTIM_STATE_FLOATS', capi.OPTIM_STATE_FLOATS)):
        found = re.search(r'#define\s+' + define + r'\s+(\w+)', header)
        assert found and int(found.group(1), 0) == value, define
    assert all(callable(getattr(capi, name)) for name in ('optim_advance', 'optim', 'optim_multi', 'optim_slot_table'))

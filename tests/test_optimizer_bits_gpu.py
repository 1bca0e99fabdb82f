"""GPU: the optimizer kernels and the training loops give the recorded bits (pytest -m gpu).  tests/golden/optimizer_bits.npz was written
by tools/record_optimizer_bits.py before Adam became one rule of the shared optimizer kernels (one element update, one multi-slot
kernel, one advance); that change is meant to move no bit of any rule, so every array of tests/optimizer_bits_cases.py must come out
equal.  Adam as a rule of the shared entry points (AMAR_OPT_ADAM) did not exist when the file was recorded: it is held against the
amar_adam_* entry points instead, bit for bit, on the same slots."""
import numpy as np
import pytest
import torch

from tests import optimizer_bits_cases as ob

pytestmark = pytest.mark.gpu
DEV = ob.DEV


@pytest.fixture(scope='module')
def golden():
    with np.load(ob.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same(got, golden, prefix):
    assert got and all(a.dtype == np.uint32 and a.ndim == 1 for a in got.values())
    moved = ob.moved(prefix, got, golden)
    print(prefix, len(got), 'arrays,', len(moved), 'moved', moved[:8])
    assert not moved, moved


@pytest.mark.parametrize('case', ['sgd', 'sgd-momentum', 'sgd-nesterov', 'rmsprop', 'rmsprop-momentum', 'rmsprop-centered',
                                  'rmsprop-centered-momentum', 'adagrad', 'adamax', 'nadam', 'amsgrad'])
def test_multi_kernel_repeats_the_recorded_bits(hip, golden, case):
    _same(ob.multi_bits(hip, case, ob._specs()[case]), golden, 'multi/{}/'.format(case))


def test_advance_entry_points_repeat_the_recorded_bits(hip, golden):
    _same(ob.advance_bits(hip), golden, 'advance/')


@pytest.mark.parametrize('model,rule,loop', ob.train_cases(), ids=lambda v: str(v))
def test_training_loops_repeat_the_recorded_bits(hip, golden, model, rule, loop):
    _same(ob.train_bits(model, rule, loop), golden, 'train/{}/{}/{}/'.format(model, rule, loop))


def test_adam_as_a_rule_equals_the_adam_entry_points(hip):
    """amar_optim_advance_f32 / amar_optim_f32 / amar_optim_multi_f32 under AMAR_OPT_ADAM against amar_adam_advance_f32 / amar_adam_dev_f32 /
    amar_adam_multi_f32 on the slots of the recorded cases: state[0:2] after every one of seven advances, every w, m and v of the
    multi-slot form and of the single-tensor form, bit for bit; the shared form leaves state[2:8] as it found it."""
    from deep_cbrs_amar_renaissance_amd import training
    spec = training.OptimizerSpec(rule='Adam', learning_rate=ob.LR, beta_1=ob.B1, beta_2=ob.B2, epsilon=ob.EPS)
    assert spec.code == hip.OPT_ADAM and spec.flags == 0 and spec.n_arrays == 2
    host, slots = ob.slot_buffer(np.random.default_rng(31), 2)
    state8 = torch.full((hip.OPTIM_STATE_FLOATS,), -7.25, device=DEV)
    state8[:2] = 0
    state2 = torch.zeros(2, device=DEV)
    for _ in range(7):
        hip.optim_advance(state8, spec.code, spec.flags, spec.hyper)
        hip.adam_advance(state2, ob.LR, ob.B1, ob.B2)
        assert torch.equal(state8[:2], state2) and bool((state8[2:] == -7.25).all())
    state8[2:] = 0
    shared, adam = ob._t(host), ob._t(host)
    entries = ob.optim_entries(hip, shared, slots)
    table, blocks = hip.optim_slot_table(entries)
    loss = torch.full((1,), 2.5, device=DEV)
    hip.optim_multi(spec.code, spec.flags, spec.hyper, table.to(DEV), len(slots), blocks, state8, reg_scale=0.5, loss_acc=loss)
    adam_table, adam_blocks = hip.adam_slot_table([(w, g, s[0], s[1], l2) for (w, g, s, l2) in ob.optim_entries(hip, adam, slots)])
    assert adam_blocks == blocks
    hip.adam_multi(adam_table.to(DEV), len(slots), blocks, state2, ob.B1, ob.B2, ob.EPS, reg_scale=0.5, loss_acc=None)
    torch.cuda.synchronize()
    a, b = shared.cpu().numpy().view(np.uint32), adam.cpu().numpy().view(np.uint32)
    assert np.array_equal(a, b) and not np.array_equal(a, host.view(np.uint32)) and float(loss[0]) > 2.5
    for s in slots:                                                   # the single-tensor forms, on the partials summed in group order
        parts = host[s['g']].reshape(max(s['groups'], 1), s['n'])
        g32 = parts[0].copy()
        for part in parts[1:]:
            g32 += part
        one = [ob._t(host[sl].copy()) for sl in [s['w']] + s['s']]
        two = [t.clone() for t in one]
        hip.optim(spec.code, spec.flags, spec.hyper, one[0], ob._t(g32), one[1:], state8, l2=s['l2'])
        hip.adam_dev(two[0], ob._t(g32), two[1], two[2], state2, ob.B1, ob.B2, ob.EPS, l2=s['l2'])
        for name, sl, x, y in zip('wmv', [s['w']] + s['s'], one, two):
            assert torch.equal(x, y), (s['n'], s['kind'], s['groups'], name)
            assert np.array_equal(x.cpu().numpy().view(np.uint32), a[sl]), (s['n'], s['kind'], s['groups'], name)

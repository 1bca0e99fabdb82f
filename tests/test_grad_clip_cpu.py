"""Gradient clipping, host side: the numpy restatement (tests/clip_ref.py) against cases computed by hand, and the surface the feature
adds: the optimizer classes take and keep the three keys, a config dict's keys reach them through Experimenter.build_optimizer's filter,
OptimizerSpec validates them and puts them into its key, the entry points are declared and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import clip_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_hand_cases():
    three_four = [(np.zeros(2), np.array([[3.0, 4.0]]), 0.0)]
    for mode in ('clipnorm', 'global_clipnorm'):
        got, nrm = cref.clip(mode, 1.0, three_four)
        assert np.allclose(got[0], [0.6, 0.8], rtol=1e-15, atol=0) and nrm.tolist() == [5.0]
    got, nrm = cref.clip('clipvalue', 3.5, three_four)
    assert got[0].tolist() == [3.0, 3.5] and nrm is None
    assert cref.clip('clipvalue', 1.0, [(np.zeros(2), np.array([[-3.0, 0.5]]), 0.0)])[0][0].tolist() == [-1.0, 0.5]
    # the finished gradient: partials added, 2 l2 w on top
    slot = (np.array([1.0, -2.0]), np.array([[1.0, 1.0], [2.0, 3.0]]), 0.25)
    assert cref.finished(*slot).tolist() == [3.5, 3.0]
    # per tensor against global: [3, 4] and [0, 12] have norms 5 and 12, together 13
    two = [(np.zeros(2), np.array([[3.0, 4.0]]), 0.0), (np.zeros(2), np.array([[0.0, 12.0]]), 0.0)]
    got, nrm = cref.clip('clipnorm', 6.0, two)
    assert nrm.tolist() == [5.0, 12.0] and got[0].tolist() == [3.0, 4.0] and np.allclose(got[1], [0.0, 6.0], rtol=1e-15)
    got, nrm = cref.clip('global_clipnorm', 6.5, two)
    assert nrm.tolist() == [13.0] and np.allclose(got[0], [1.5, 2.0], rtol=1e-15) and np.allclose(got[1], [0.0, 6.0], rtol=1e-15)
    assert cref.max_abs(two) == 12.0


@pytest.mark.parametrize('mode', cref.MODES)
def test_a_clip_that_does_not_bind_is_the_identity(mode):
    rng = np.random.default_rng(2)
    slots = [(rng.standard_normal(n), rng.standard_normal((g, n)), l2) for n, g, l2 in ((5, 1, 0.0), (7, 3, 0.01))]
    got, _ = cref.clip(mode, 1e30, slots)
    for a, slot in zip(got, slots):
        assert np.array_equal(a, cref.finished(*slot))
    zero, _ = cref.clip(mode, 1.0, [(np.zeros(4), np.zeros((2, 4)), 0.0)])
    assert np.array_equal(zero[0], np.zeros(4))                       # norm 0: scale 1, no NaN
    bounds, _ = cref.bounds(mode, 1e30, slots)
    exact = [3 * cref.U * (np.abs(s[1]).sum(0) + 2 * s[2] * np.abs(s[0])) for s in slots]
    exact[0] = exact[0] / 3                                           # (one group: one rounding)
    for b, e in zip(bounds, exact):
        assert np.allclose(b, cref.SLACK * e, rtol=1e-12)             # no norm term where the clip cannot bind


def test_bounds_of_a_binding_norm_written_out():
    """One group, l2 = 0, a binding clip: e_g = u |g|, e_norm = norm u (1 + n / 2 + 1), e_s = e_norm / norm + u, and the element's bound
    is 1.01 |g| s u (n / 2 + 5): the n-term sum behind the norm is what grows with the slot."""
    rng = np.random.default_rng(3)
    for n in (16, 4096):
        slots = [(np.zeros(n), rng.standard_normal((1, n)), 0.0)]
        b, e_norm = cref.bounds('clipnorm', 0.5, slots)
        g, nrm = cref.finished(*slots[0]), cref.norms('clipnorm', slots)
        assert nrm[0] > 0.5
        assert np.allclose(b[0], cref.SLACK * np.abs(g) * (0.5 / nrm[0]) * cref.U * (n / 2 + 5), rtol=1e-12)
        assert np.allclose(e_norm, cref.SLACK * nrm * cref.U * (n / 2 + 2), rtol=1e-12)
        b_global, e_global = cref.bounds('global_clipnorm', 0.5, slots)
        assert np.allclose(b_global[0], b[0], rtol=1e-12) and np.allclose(e_global, e_norm, rtol=1e-12)


def test_reference_optimizer_clips_before_the_update():
    opt = cref.Optimizer('SGD', clip=('global_clipnorm', 6.5), learning_rate=1.0)
    opt.advance()
    new = opt.update_all({'a': (np.zeros(2), np.array([3.0, 4.0])), 'b': (np.ones((1, 2)), np.array([[0.0, 12.0]]))})
    assert np.allclose(new['a'], [-1.5, -2.0], rtol=1e-15) and np.allclose(new['b'], [[1.0, -5.0]], rtol=1e-15)
    plain = cref.Optimizer('SGD', learning_rate=1.0)
    plain.advance()
    assert plain.update_all({'a': (np.zeros(2), np.array([3.0, 4.0]))})['a'].tolist() == [-3.0, -4.0]


# ---- the surface ------------------------------------------------------------------------------------------------------------------------

def _experimenter_stub(optimizer_cfg):
    from deep_cbrs_amar_renaissance_amd import experiment as ex
    stub = ex.Experimenter.__new__(ex.Experimenter)
    stub.config = ex.AttrDict({'parameters': {'optimizer': optimizer_cfg}})
    stub.optimizer_class = ex.optimizer_class(optimizer_cfg['name'])
    return stub


@pytest.mark.parametrize('name', ['Adam', 'SGD', 'RMSprop', 'Adagrad', 'Adamax', 'Nadam'])
@pytest.mark.parametrize('key', ['clipnorm', 'clipvalue', 'global_clipnorm'])
def test_config_keys_reach_the_spec_through_the_filter(name, key):
    """`parameters.optimizer: {name: ..., clipnorm: 0.75}` -> build_optimizer -> the optimizer object -> OptimizerSpec.clip (these keys
    used to be dropped by the signature filter and the user trained unclipped)."""
    from deep_cbrs_amar_renaissance_amd import experiment as ex, training
    stub = _experimenter_stub({'name': name, 'learning_rate': 0.125, key: 0.75})
    stub.build_optimizer()
    assert getattr(stub.optimizer, key) == 0.75
    assert [getattr(stub.optimizer, k) for k in ('clipnorm', 'clipvalue', 'global_clipnorm') if k != key] == [None, None]
    spec = training.OptimizerSpec(stub.optimizer)
    assert spec.clip == (key, 0.75) and spec.values['learning_rate'] == 0.125
    assert spec.key != training.OptimizerSpec(ex.OPTIMIZERS[name](learning_rate=0.125)).key
    assert spec.key != training.OptimizerSpec(ex.OPTIMIZERS[name](learning_rate=0.125, **{key: 0.5})).key
    assert spec.key == training.OptimizerSpec(ex.OPTIMIZERS[name](learning_rate=0.125, **{key: 0.75})).key
    stub = _experimenter_stub({'name': name, key: None})              # `clipnorm: null` in a config: off
    stub.build_optimizer()
    assert training.OptimizerSpec(stub.optimizer).clip is None


def test_spec_reads_keywords_and_objects():
    import types
    from deep_cbrs_amar_renaissance_amd import capi, experiment as ex, training
    assert training.OptimizerSpec(None).clip is None and training.OptimizerSpec(ex.SGD()).clip is None
    spec = training.OptimizerSpec(rule='SGD', learning_rate=0.1, global_clipnorm=2)
    assert spec.clip == ('global_clipnorm', 2.0) and spec.clip_mode == capi.CLIP_GLOBAL_NORM and spec.values['learning_rate'] == 0.1
    assert training.OptimizerSpec(rule='RMSprop', clipvalue=0.5).clip_mode == capi.CLIP_VALUE
    assert training.OptimizerSpec(types.SimpleNamespace(clipnorm=3.0)).clip_mode == capi.CLIP_NORM      # (no rule name: Adam)
    assert training.OptimizerSpec(ex.Adam(clipnorm=1.0), clipnorm=2.0).clip == ('clipnorm', 2.0)        # keywords win
    assert training.OptimizerSpec(ex.Adam(clipnorm=1.0), clipnorm=None).clip is None
    # an optimizer without a clip keeps the key's first two parts: rule and hyper-parameters
    assert training.OptimizerSpec(ex.Nadam(clipnorm=1.0)).key[:2] == training.OptimizerSpec(ex.Nadam()).key[:2]


@pytest.mark.parametrize('kwargs, reason', [
    (dict(clipnorm=1.0, global_clipnorm=1.0), 'both'),
    (dict(clipvalue=1.0, clipnorm=1.0), 'order'),
    (dict(clipvalue=1.0, global_clipnorm=1.0), 'order'),
    (dict(clipnorm=0.0), 'positive'), (dict(clipvalue=-1.0), 'positive'), (dict(global_clipnorm=float('nan')), 'positive'),
])
def test_refused_combinations_and_values_raise(kwargs, reason):
    from deep_cbrs_amar_renaissance_amd import experiment as ex, training
    with pytest.raises(ValueError) as err:
        training.OptimizerSpec(rule='SGD', **kwargs)
    assert reason in str(err.value)
    with pytest.raises(ValueError):
        training.OptimizerSpec(ex.Adam(**kwargs))


def test_entry_points_are_declared_and_bound_and_check_their_arguments():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    declared = set(re.findall(r'\b(amar_[a-z0-9_]+)\s*\(', header))
    for name in ('amar_grad_clip_workspace_floats', 'amar_grad_clip_f32'):
        assert name in capi.SIGNATURES and name in declared, name
    for define, value in (('AMAR_CLIP_VALUE', capi.CLIP_VALUE), ('AMAR_CLIP_NORM', capi.CLIP_NORM), ('AMAR_CLIP_GLOBAL_NORM', capi.CLIP_GLOBAL_NORM)):
        found = re.search(r'#define\s+' + define + r'\s+(\w+)', header)
        assert found and int(found.group(1), 0) == value, define
    assert ctypes.sizeof(capi.ClipSlot) == 40
    lib = capi.load()
    assert lib.amar_grad_clip_workspace_floats(3, 7) == 10
    assert lib.amar_grad_clip_workspace_floats(0, 7) == -1 and lib.amar_grad_clip_workspace_floats(3, 0) == -1
    assert lib.amar_grad_clip_workspace_floats(3, 2 ** 31) == -1
    table = (capi.ClipSlot * 1)()                                     # (never dereferenced: every call below is refused first)
    args = dict(mode=capi.CLIP_NORM, clip=1.0, slots=ctypes.addressof(table), n_slots=1, total_blocks=1, workspace=ctypes.addressof(table))
    for bad in (dict(mode=0), dict(mode=4), dict(clip=0.0), dict(clip=-1.0), dict(clip=float('nan')), dict(slots=None), dict(n_slots=0),
                dict(total_blocks=0), dict(total_blocks=2 ** 31), dict(workspace=None), dict(mode=capi.CLIP_GLOBAL_NORM, workspace=None)):
        a = dict(args, **bad)
        code = lib.amar_grad_clip_f32(a['mode'], a['clip'], a['slots'], a['n_slots'], a['total_blocks'], a['workspace'], None, 0.0, None, None)
        assert code == -1, bad                                        # AMAR_EINVAL

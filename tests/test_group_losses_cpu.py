"""Listwise ranking losses (SampledSoftmaxLoss, HardestNegativeBPRLoss, MarginRankingLoss) without a GPU: the closed-form gradients
of utilities/losses.py and of tests/group_loss_ref.py against float64 autograd, the conventions of the terms, the tie and kink
rules, resolve_loss / loss_kind, fit()'s refusals, the binding, and what float32 leaves on the softmax (the GPU test's bound)."""
import os
import re

import numpy as np
import pytest
import torch

from deep_cbrs_amar_renaissance_amd.utilities import losses
from deep_cbrs_amar_renaissance_amd.utilities.losses import (BPRLoss, HardestNegativeBPRLoss, MarginRankingLoss, SampledSoftmaxLoss,
                                                             group_loss_dp, group_loss_terms, loss_kind, loss_value, resolve_loss)
from tests import group_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = [(SampledSoftmaxLoss(), ref.SOFTMAX, 1.0), (SampledSoftmaxLoss(temperature=0.2), ref.SOFTMAX, 0.2),
          (HardestNegativeBPRLoss(), ref.HARDEST, 0.0), (MarginRankingLoss(), ref.MARGIN, 0.5), (MarginRankingLoss(margin=0.1), ref.MARGIN, 0.1)]
IDS = ['softmax', 'softmax_t0.2', 'hardest', 'margin', 'margin_m0.1']


def _torch_value(kind, hyper, p, K):
    """The batch loss as a float64 torch expression of p [B] (autograd's side of the comparison)."""
    h = p.numel() // 2
    G = h // K
    a, b = p[:h:K], p[h:2 * h].reshape(G, K)
    if kind == ref.SOFTMAX:
        l = -a / hyper + torch.logsumexp(torch.cat([a[:, None], b], dim=1) / hyper, dim=1)
    elif kind == ref.HARDEST:
        l = -torch.nn.functional.logsigmoid(a - b.max(dim=1).values)
    else:
        l = torch.clamp(hyper - a[:, None] + b, min=0.0).mean(dim=1)
    return l.mean()


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('loss, kind, hyper', LOSSES, ids=IDS)
def test_closed_form_gradient_is_autograd(loss, kind, hyper, K):
    rng = np.random.default_rng(10 * K + kind)
    B = 2 * K * 5 + 1                                                 # 5 groups and a dropped trailing element
    while True:                                                       # away from the hinge's kink (ties have probability 0)
        p = rng.uniform(0.02, 0.98, B)
        h = B // 2
        if kind != ref.MARGIN or np.abs(hyper - np.repeat(p[:h:K], K) + p[h:2 * h]).min() > 1e-3:
            break
    code, hy, _ = resolve_loss(loss)
    pt = torch.tensor(p, requires_grad=True)
    value = _torch_value(kind, hyper, pt, K)
    value.backward()
    want = pt.grad.numpy()
    assert abs(loss(None, p, n_negatives=K) - value.item()) < 1e-13
    assert abs(loss_value(loss, None, p, n_negatives=K) - value.item()) < 1e-13
    np.testing.assert_allclose(group_loss_dp(code, hy, p, K), want, rtol=1e-11, atol=1e-14)
    r_loss, r_terms, r_dz = ref.group_loss(kind, hyper, p, K)
    assert abs(r_loss - value.item()) < 1e-13
    np.testing.assert_allclose(r_dz, want * p * (1 - p), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(group_loss_terms(code, hy, p, K), r_terms, rtol=1e-12, atol=1e-14)
    # the positive side carries gradient (the hinge: where a negative is inside the margin) and sits on row g K alone
    assert np.all(want[:h][np.arange(h) % K != 0] == 0) and want[-1] == 0
    if kind != ref.MARGIN:
        assert np.all(want[:h:K] < 0)


@pytest.mark.parametrize('B', [2, 7, 64])
def test_softmax_with_one_negative_at_unit_temperature_is_bpr(B):
    p = np.random.default_rng(B).uniform(0, 1, B)
    assert SampledSoftmaxLoss()(None, p) == pytest.approx(BPRLoss()(None, p), rel=1e-14)
    assert loss_value('SampledSoftmaxLoss', None, p) == pytest.approx(loss_value('BPRLoss', None, p), rel=1e-14)
    code, hy, _ = resolve_loss('SampledSoftmaxLoss')
    x = p[:B // 2] - p[B // 2:2 * (B // 2)]
    want = np.zeros(B)
    want[:B // 2], want[B // 2:2 * (B // 2)] = -1 / (1 + np.exp(x)) / (B // 2), 1 / (1 + np.exp(x)) / (B // 2)
    np.testing.assert_allclose(group_loss_dp(code, hy, p, 1), want, rtol=1e-13)


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('loss, kind, hyper', LOSSES, ids=IDS)
def test_terms_sum_to_B_times_the_loss_and_the_silent_rows_are_zero(loss, kind, hyper, K):
    code, hy, _ = resolve_loss(loss)
    for B in (2 * K * 4, 2 * K * 4 + 1):
        p = np.random.default_rng(B).uniform(0, 1, B)
        terms, dp = group_loss_terms(code, hy, p, K), group_loss_dp(code, hy, p, K)
        assert np.sum(terms) == pytest.approx(B * loss(None, p, n_negatives=K), rel=1e-14)
        dz0, t0 = ref.must_be_zero(B, K)
        assert np.all(dp[dz0] == 0) and np.all(terms[t0] == 0)
        assert np.all(ref.group_loss(kind, hyper, p, K)[2][dz0] == 0) and np.all(ref.group_loss(kind, hyper, p, K)[1][t0] == 0)
        assert dz0.sum() == (B // 2) - (B // 2) // K + B % 2
    for empty in ([], [0.3]):
        assert loss(None, empty, n_negatives=K) == 0.0 and np.all(group_loss_dp(code, hy, empty, K) == 0)
    with pytest.raises(ValueError):
        group_loss_terms(code, hy, np.full(2 * K, 0.5), 0)
    with pytest.raises(ValueError):
        group_loss_terms(code, hy, np.full(2 * K + 2, 0.5), K + 2)


def test_hardest_negative_tie_goes_to_the_lowest_k():
    p = np.array([0.6, 0.6, 0.6, 0.6, 0.2, 0.7, 0.7, 0.1])           # one group, K = 4: negatives 0.2, 0.7, 0.7, 0.1
    code, hy, _ = resolve_loss(HardestNegativeBPRLoss())
    dp = group_loss_dp(code, hy, p, 4)
    g = 1 / (1 + np.exp(0.6 - 0.7))
    assert np.array_equal(dp != 0, [True, False, False, False, False, True, False, False])
    assert dp[0] == pytest.approx(-g) and dp[5] == pytest.approx(g)
    assert np.array_equal(ref.group_loss(ref.HARDEST, 0.0, p, 4)[2] != 0, dp != 0)
    allsame = np.array([0.5, 0.5, 0.3, 0.3])                          # K = 2, both negatives equal: k = 0 takes it
    assert np.array_equal(group_loss_dp(code, hy, allsame, 2) != 0, [True, False, True, False])


def test_margin_hinge_is_flat_exactly_at_the_kink():
    code, hy, _ = resolve_loss(MarginRankingLoss(margin=0.5))
    p = np.array([0.75, 0.75, 0.25, 0.5])                             # K = 2: hinge arguments 0.0 (the kink) and 0.25
    terms, dp = group_loss_terms(code, hy, p, 2), group_loss_dp(code, hy, p, 2)
    assert terms[0] == 4 * 0.125 and np.array_equal(dp, [-0.5, 0.0, 0.0, 0.5])
    assert np.array_equal(ref.group_loss(ref.MARGIN, 0.5, p, 2)[2], dp * p * (1 - p))
    beyond = np.array([1.0, 0.25])                                    # the margin is met: no loss, no gradient
    assert MarginRankingLoss()(None, beyond) == 0.0 and np.all(group_loss_dp(code, hy, beyond, 1) == 0)
    zero_margin = resolve_loss(MarginRankingLoss(margin=0.0))
    assert np.array_equal(group_loss_dp(zero_margin[0], zero_margin[1], np.array([0.5, 0.5]), 1), [0.0, 0.0])


def test_resolve_loss_names_instances_and_mappings():
    assert resolve_loss('SampledSoftmaxLoss') == (losses.SAMPLED_SOFTMAX, (1.0, 0.0, 0.0, 0.0), 'SampledSoftmaxLoss')
    assert resolve_loss(SampledSoftmaxLoss(temperature=0.2)) == (losses.SAMPLED_SOFTMAX, (0.2, 0.0, 0.0, 0.0), 'SampledSoftmaxLoss')
    assert resolve_loss({'name': 'SampledSoftmaxLoss', 'temperature': 0.2})[1] == (0.2, 0.0, 0.0, 0.0)
    assert resolve_loss({'class_name': 'MarginRankingLoss', 'margin': 0})[:2] == (losses.MARGIN_RANKING, (0.0, 0.0, 0.0, 0.0))
    assert resolve_loss('MarginRankingLoss')[1] == (0.5, 0.0, 0.0, 0.0)
    assert resolve_loss('HardestNegativeBPRLoss') == resolve_loss(HardestNegativeBPRLoss()) == \
        (losses.HARDEST_NEGATIVE, (0.0, 0.0, 0.0, 0.0), 'HardestNegativeBPRLoss')
    assert len({losses.BPR, losses.SAMPLED_SOFTMAX, losses.HARDEST_NEGATIVE, losses.MARGIN_RANKING}) == 4
    assert set(losses.GROUP_KINDS.values()) == set(ref.KINDS)
    for name in ('SampledSoftmaxLoss', 'HardestNegativeBPRLoss', 'MarginRankingLoss'):
        assert name in losses.supported_losses() and isinstance(getattr(losses, name), type)       # (the experiment's lookup)
        assert loss_kind(name) == loss_kind(getattr(losses, name)()) == loss_kind({'name': name}) == 'bpr'
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature='x')):
        with pytest.raises(ValueError):
            SampledSoftmaxLoss(**bad)
        with pytest.raises(ValueError):
            resolve_loss(dict(bad, name='SampledSoftmaxLoss'))
    for bad in (dict(margin=-0.1), dict(margin=float('inf'))):
        with pytest.raises(ValueError):
            MarginRankingLoss(**bad)
        with pytest.raises(ValueError):
            resolve_loss(dict(bad, name='MarginRankingLoss'))
    late = SampledSoftmaxLoss()
    late.temperature = 0.0
    with pytest.raises(ValueError):
        resolve_loss(late)
    for unknown in ({'name': 'SampledSoftmaxLoss', 'margin': 0.5}, {'name': 'MarginRankingLoss', 'temperature': 1.0},
                    {'name': 'HardestNegativeBPRLoss', 'temperature': 1.0}, {'name': 'SampledSoftmaxLoss', 'label_smoothing': 0.1}):
        with pytest.raises(ValueError, match='takes no hyper-parameter'):
            resolve_loss(unknown)
    with pytest.raises(ValueError):
        loss_value(SampledSoftmaxLoss(), None, np.full(4, 0.5), sample_weight=np.ones(4))


def test_loss_kind_is_unchanged_for_what_it_accepted_before():
    assert loss_kind(BPRLoss()) == loss_kind('BPRLoss') == 'bpr'
    for other in (None, 'binary_crossentropy', 'mse', {'name': 'huber', 'delta': 2.0}, {'name': 'BPRLoss'}, 3, object()):
        assert loss_kind(other) == 'bce'


def test_compiled_metrics_are_refused_as_under_bpr():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import resolve_compiled
    for loss in (SampledSoftmaxLoss(), 'HardestNegativeBPRLoss', {'name': 'MarginRankingLoss', 'margin': 0.3}):
        assert resolve_compiled(loss, ['accuracy'])[2] == [] and resolve_compiled(loss, None)[2] == []
        with pytest.raises(NotImplementedError, match='labels carry no meaning'):
            resolve_compiled(loss, ['AUC'])


class _Stub:
    """What fit() reads of a model before it builds a trainer."""
    gnn = object()
    optimizer = None

    def __init__(self, loss, metrics=None):
        self.loss, self.metrics = loss, metrics


@pytest.mark.parametrize('loss', [SampledSoftmaxLoss(temperature=0.2), 'HardestNegativeBPRLoss', {'name': 'MarginRankingLoss'}],
                         ids=['softmax', 'hardest', 'margin'])
def test_fit_refusals(loss):
    """Each refusal comes before anything touches the device."""
    from deep_cbrs_amar_renaissance_amd import training
    from tests import bpr_triplets_cases as cases
    from tests.test_bpr_gpu import _sample_sequence
    triplets = cases.triplet_sequence(batch_size=64, n_negatives=4)
    with pytest.raises(ValueError, match='class_weight cannot weigh BPR training'):
        training.fit(_Stub(loss), triplets, epochs=1, verbose=False, class_weight={0: 1.0, 1: 3.0})
    with pytest.raises(NotImplementedError, match='labels carry no meaning'):
        training.fit(_Stub(loss, ['accuracy', 'AUC']), triplets, epochs=1, verbose=False)
    with pytest.raises(ValueError, match='load_user_item_graph_triplets'):
        training.fit(_Stub(loss), _sample_sequence(batch_size=64), epochs=1, verbose=False)
    ratings = [((np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)), np.zeros(4))]
    with pytest.raises(ValueError, match='load_user_item_graph_triplets'):
        training.fit(_Stub(loss), ratings, epochs=1, verbose=False)
    head_only = type('HeadOnly', (), {'optimizer': None, 'loss': loss, 'metrics': None})()      # (no .gnn: BasicRS on rows)
    with pytest.raises(ValueError, match='load_user_item_graph_triplets'):
        training.fit(head_only, triplets, epochs=1, verbose=False)


def test_symbol_is_declared_and_bound():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    sym = 'amar_group_loss_grad_f32'
    assert sym in capi.SIGNATURES and re.search(r'\bint\s+' + sym + r'\s*\(', header) and callable(capi.group_loss_grad)
    assert len(capi.SIGNATURES[sym][1]) == 9
    for name, value in (('SOFTMAX', capi.GROUP_SOFTMAX), ('HARDEST', capi.GROUP_HARDEST), ('MARGIN', capi.GROUP_MARGIN)):
        assert re.search(r'#define\s+AMAR_GROUP_{}\s+{}\b'.format(name, value), header)
    assert (capi.GROUP_SOFTMAX, capi.GROUP_HARDEST, capi.GROUP_MARGIN) == ref.KINDS
    assert losses.GROUP_KINDS == {losses.SAMPLED_SOFTMAX: capi.GROUP_SOFTMAX, losses.HARDEST_NEGATIVE: capi.GROUP_HARDEST,
                                  losses.MARGIN_RANKING: capi.GROUP_MARGIN}


# ---- what float32 leaves on the softmax: the figure behind the GPU test's bound ---------------------------------------------------
@pytest.mark.parametrize('t', ref.TEMPERATURES)
def test_float32_sequential_softmax_figures(t):
    """ref.F32_SEQUENTIAL is the record of this measurement: a sequential float32 evaluation of the softmax against float64 on the
    very inputs of the GPU test, in units of the bound tests/test_bpr_gpu.py sets the BPR kernel (which the GPU test keeps for
    the softmax kernel too: ref.bounds)."""
    terms, dz = ref.measure_f32_sequential(t)
    print('temperature', t, 'terms', terms, 'dz', dz)
    for got, recorded in zip((terms, dz), ref.F32_SEQUENTIAL[t]):
        assert abs(got - recorded) <= 0.05 * recorded, (t, terms, dz)

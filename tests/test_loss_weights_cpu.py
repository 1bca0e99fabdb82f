"""CPU: the weights of the training loss on the host — resolve_class_weight (mapping forms, 'balanced', every refusal), the weighted
float64 restatement (w x the unweighted terms and gradients, the divisor B), the rating Sequences built with sample_weight
(three-element batches, each weight kept with its rating across reshuffles; two-element batches without it), fit()'s keywords, and
the new entry point in the header and the binding."""
import inspect
import os
import re

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd.utilities import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ['binary_crossentropy', {'name': 'binary_crossentropy', 'label_smoothing': 0.1}, 'mse', 'mae', 'hinge', 'squared_hinge',
          {'name': 'huber', 'delta': 0.25}, 'log_cosh', 'poisson', {'name': 'binary_focal_crossentropy', 'gamma': 3.0}]
_ids = lambda v: v if isinstance(v, str) else '-'.join(str(x) for x in v.values())   # noqa: E731


# ---- resolve_class_weight ---------------------------------------------------------------------------------------------------------------

def test_class_weight_mapping_forms():
    assert L.resolve_class_weight(None) is None
    assert L.resolve_class_weight({0: 1.0, 1: 3.0}) == (1.0, 3.0)
    assert L.resolve_class_weight({'0': 2, '1': '0.5'}) == (2.0, 0.5)        # YAML's keys (and a number YAML left a string)
    assert L.resolve_class_weight({1: 3}) == (1.0, 3.0)                     # a class left out weighs 1 ...
    assert L.resolve_class_weight({1: 3}, labels=[1, 1, 1]) == (1.0, 3.0)   # ... also against labels that do not hold it
    assert L.resolve_class_weight({0: 0.0, 1: 1.0}, labels=[0, 1]) == (0.0, 1.0)
    pair = L.resolve_class_weight({0: 1, 1: 2})
    assert all(type(v) is float for v in pair)


def test_class_weight_balanced_on_a_hand_counted_vector():
    labels = [1, 0, 1, 1, 0, 1, 1, 1]                                       # N = 8: two of class 0, six of class 1
    assert L.resolve_class_weight('balanced', labels) == (8 / (2 * 2), 8 / (2 * 6))
    assert L.resolve_class_weight('balanced', np.array([0.0, 1.0])) == (1.0, 1.0)


@pytest.mark.parametrize('value,labels', [
    ({0: 1.0, 2: 3.0}, None), ({'a': 1.0}, None), ({-1: 1.0, 1: 1.0}, None), ({True: 1.0}, None),        # other keys
    ({0: -1.0, 1: 1.0}, None), ({0: float('nan'), 1: 1.0}, None), ({0: 1.0, 1: float('inf')}, None),      # negative, non-finite
    ({0: 1.0, 1: 1e39}, None),                                                                            # (not finite as float32)
    ({1: 3.0}, [0, 1, 1]), ({0: 3.0}, [0, 1, 1]),                                                         # a class of the labels left out
    ('balanced', [1, 1, 1]), ('balanced', [0, 0]), ('balanced', []), ('balanced', None),                  # an empty class
    ('auto', [0, 1]), (3.0, None), ([1.0, 3.0], None)])
def test_class_weight_refusals(value, labels):
    with pytest.raises(ValueError):
        L.resolve_class_weight(value, labels)


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('loss', LOSSES, ids=_ids)
def test_weighted_terms_and_gradients_are_w_times_the_unweighted(loss):
    code, hyper, _ = L.resolve_loss(loss)
    rng = np.random.default_rng(code + 1)
    y = rng.integers(0, 2, 97)
    p = rng.uniform(0.01, 0.99, 97)
    sw = rng.uniform(0.0, 4.0, 97)
    cw = (0.5, 3.0)
    t0, d0 = L.loss_terms(code, hyper, y, p), L.loss_dp(code, hyper, y, p)
    per_class = np.where(y > 0.5, cw[1], cw[0])
    for kwargs, w in (({'sample_weight': sw}, sw), ({'class_weight': cw}, per_class), ({'class_weight': {0: 0.5, 1: 3.0}}, per_class),
                      ({'sample_weight': sw, 'class_weight': cw}, sw * per_class)):
        assert np.array_equal(L.loss_terms(code, hyper, y, p, **kwargs), w * t0)
        assert np.array_equal(L.loss_dp(code, hyper, y, p, **kwargs), w * d0)
    assert np.array_equal(L.pair_weights(y, sw, cw), sw * per_class) and L.pair_weights(y) is None
    assert L.loss_terms(code, hyper, y, p).dtype == np.float64


def test_the_class_is_read_from_the_label_before_smoothing():
    code, hyper, _ = L.resolve_loss({'name': 'binary_crossentropy', 'label_smoothing': 0.9})     # smoothed: 1 -> 0.55, 0 -> 0.45
    y, p = np.array([1.0, 0.0]), np.array([0.3, 0.3])
    got = L.loss_terms(code, hyper, y, p, class_weight=(2.0, 5.0))
    assert np.array_equal(got, np.array([5.0, 2.0]) * L.loss_terms(code, hyper, y, p))


def test_loss_value_divides_by_the_batch_size_not_by_the_weights():
    y, p, w = [0, 1, 0, 0], [.6, .4, .4, .6], [4.0, 0.0, 0.0, 0.0]
    terms = L.loss_terms(L.MSE, (0, 0, 0, 0), y, p)
    assert L.loss_value('mse', y, p, sample_weight=w) == 4.0 * terms[0] / 4            # (sum(w) = 4 would give the same: so ...)
    w = [1.0, 0.0, 0.0, 0.0]
    assert L.loss_value('mse', y, p, sample_weight=w) == terms[0] / 4                  # ... B = 4 against sum(w) = 1
    assert L.loss_value('mse', y, p, class_weight={0: 2.0, 1: 2.0}) == 2.0 * L.loss_value('mse', y, p)
    assert L.loss_value('mse', y, p, sample_weight=[1, 1, 1, 1]) == L.loss_value('mse', y, p)
    with pytest.raises(ValueError):
        L.loss_value('mse', y, p, sample_weight=[1.0, 2.0])
    with pytest.raises(ValueError):
        L.loss_value(L.BPRLoss(), y, p, sample_weight=w)


# ---- the Sequences ----------------------------------------------------------------------------------------------------------------------

def _ratings(n=53):
    rng = np.random.default_rng(4)
    return np.stack([rng.integers(0, 7, n), rng.integers(7, 16, n), np.arange(n)], axis=1)      # rating r carries the "label" r


def _sequences(sample_weight, **kwargs):
    from deep_cbrs_amar_renaissance_amd.data import datasets as D
    r = _ratings()
    users, items = np.arange(7), np.arange(9)
    table, bert = np.arange(32, dtype=np.float32).reshape(16, 2), np.arange(48, dtype=np.float32).reshape(16, 3)
    extra = {} if sample_weight is None else {'sample_weight': sample_weight}
    return r, [D.UserItemGraph(r, users, items, None, **kwargs, **extra),
               D.UserItemEmbeddings(r, users, items, table, **kwargs, **extra),
               D.HybridUserItemEmbeddings(r, users, items, table, bert, **kwargs, **extra),
               D.UserItemGraphEmbeddings(r, users, items, None, bert, **kwargs, **extra)]


@pytest.mark.parametrize('shuffle', [False, True])
def test_weighted_sequences_keep_each_weight_with_its_rating(shuffle):
    """Rating r has label r and weight r: every batch of every epoch must then satisfy w == y."""
    r, seqs = _sequences(np.arange(53, dtype=np.float64), batch_size=16, shuffle=shuffle, seed=3)
    for seq in seqs:
        orders = []
        for _ in range(3):
            seen = []
            for b in range(len(seq)):
                batch = seq[b]
                assert len(batch) == 3
                inputs, y, w = batch
                assert w.dtype == np.float32 and w.shape == y.shape and np.array_equal(w, y.astype(np.float32))
                assert len(inputs[0]) == len(y)
                seen.append(y)
            assert [len(s) for s in seen] == [16, 16, 16, 5]
            orders.append(np.concatenate(seen))
            assert np.array_equal(np.sort(orders[-1]), np.arange(53))
            seq.on_epoch_end()
        assert shuffle == (not np.array_equal(orders[0], orders[1]))          # (the check above saw more than one order)
        ids = seq.graph_ids if hasattr(seq, 'graph_ids') else seq
        assert np.array_equal(ids._batch_weights(1), ids._batch_ratings(1)[:, 2].astype(np.float32))


def test_sequences_without_sample_weight_yield_two_element_batches():
    _, seqs = _sequences(None, batch_size=16, shuffle=True)
    for seq in seqs:
        assert seq.sample_weight is None
        assert all(len(seq[b]) == 2 for b in range(len(seq)))
        ids = seq.graph_ids if hasattr(seq, 'graph_ids') else seq
        assert ids._batch_weights(0) is None


@pytest.mark.parametrize('bad', [np.ones(52), np.ones(54), np.ones((53, 1)), np.ones(0)])
def test_a_sample_weight_of_another_length_is_refused(bad):
    with pytest.raises(ValueError):
        _sequences(bad, batch_size=16)


# ---- fit()'s keywords, the header and the binding ---------------------------------------------------------------------------------------

def test_fit_names_its_keywords():
    """No **kwargs left on any fit loop: class_weight is a named argument, `workers` (which the experiment passes) is still taken, and
    a keyword fit() does not know is a TypeError before anything is read."""
    from deep_cbrs_amar_renaissance_amd import training
    params = inspect.signature(training.fit).parameters
    assert 'class_weight' in params and 'workers' in params
    assert not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())
    with pytest.raises(TypeError):
        training.fit(object(), [], clas_weight={0: 1.0, 1: 3.0})
    with pytest.raises(ValueError):
        training.fit(object(), [], class_weight={0: -1.0, 1: 3.0})


def test_binding_and_header_declare_the_weighted_entry_point():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    sym = 'amar_loss_grad_weighted_f32'
    assert sym in capi.SIGNATURES and re.search(r'\bint\s+' + sym + r'\s*\(', header)
    unweighted, weighted = capi.SIGNATURES['amar_loss_grad_f32'], capi.SIGNATURES[sym]
    assert weighted[0] is unweighted[0] and len(weighted[1]) == len(unweighted[1]) + 2       # the two weight pointers
    declared = re.search(sym + r'\s*\(([^)]*)\)', header).group(1)
    assert len(declared.split(',')) == len(weighted[1]) and 'sample_w' in declared and 'class_w' in declared
    params = inspect.signature(capi.loss_grad).parameters
    assert params['sample_weight'].default is None and params['class_weight'].default is None


def test_experiment_resolves_class_weight_against_the_training_rows_and_logs_it():
    import types
    from deep_cbrs_amar_renaissance_amd.experiment import Experimenter
    logged = []
    ratings = np.array([[0, 5, 1], [1, 5, 0], [2, 6, 1], [3, 6, 1]])
    for value, want in (('balanced', (4 / 2, 4 / 6)), ({'0': 1.0, '1': 3.0}, (1.0, 3.0)), (None, None)):
        fake = types.SimpleNamespace(parameters={'class_weight': value} if value is not None else {}, trainset=types.SimpleNamespace(ratings=ratings),
                                     run_log=types.SimpleNamespace(log_params=logged.append))
        assert Experimenter.class_weight(fake) == want
    assert logged == [{'class_weight.0': 2.0, 'class_weight.1': 4 / 6}, {'class_weight.0': 1.0, 'class_weight.1': 3.0}]
    with pytest.raises(ValueError):
        Experimenter.class_weight(types.SimpleNamespace(parameters={'class_weight': {1: 3.0}}, trainset=types.SimpleNamespace(ratings=ratings),
                                                        run_log=types.SimpleNamespace(log_params=logged.append)))

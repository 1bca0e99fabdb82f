"""GPU: validation during fit() — the full-ranking metrics kernel (amar_rank_metrics_f64) against the host function,
evaluate_ranking on both recommend() routes, fit() with validation_data / validation_ranking / callbacks leaving training bit for
bit as it was, the val_* history, early stopping with the best weights put back, the resident-table head (pytest -m gpu)."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests.test_dropout_gpu import _bce_model, _bce_sequence, _bpr_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-12                       # both sides are float64 sums of at most 66 terms in [0, 1] per user: only the summation order differs
N_USERS, N_ITEMS = 300, 500
METRICS = ('precision', 'recall', 'ndcg', 'hit')


class _Train:
    """The parts of a training Sequence recommend() reads."""

    def __init__(self, ratings, n_users, n_items, **tables):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)
        self.__dict__.update(tables)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------
def _relevant_sets(rng):
    """Per user the relevant item rows: user 0 none, 1 one element, 2 three hundred, 3 three (below every k > 3), 4 a hundred (above
    K = 64), 5 a few (its list is all padding); the others 0..40 at random (several more users without any)."""
    rel = {}
    for u in range(N_USERS):
        n = int(rng.integers(0, 41)) if rng.random() > 0.1 else 0
        rel[u] = np.sort(rng.choice(N_ITEMS, size=n, replace=False))
    rel[0] = np.zeros(0, dtype=np.int64)
    rel[1] = np.array([int(rng.integers(0, N_ITEMS))])
    rel[2] = np.sort(rng.choice(N_ITEMS, size=300, replace=False))
    rel[3] = np.sort(rng.choice(N_ITEMS, size=3, replace=False))
    rel[4] = np.sort(rng.choice(N_ITEMS, size=100, replace=False))
    rel[5] = np.sort(rng.choice(N_ITEMS, size=6, replace=False))
    return rel


def _test_ratings(rel, rng):
    """[P, 3] (user, item node id, label): the relevant pairs with label 1 in shuffled order, some twice, and label-0 pairs of other items."""
    rows = []
    for u, items in rel.items():
        rows += [(u, int(i) + N_USERS, 1) for i in items]
        rows += [(u, int(i) + N_USERS, 1) for i in items[:2]]                       # duplicates: the CSR holds every item once
        others = np.setdiff1d(rng.choice(N_ITEMS, size=5, replace=False), items)
        rows += [(u, int(i) + N_USERS, 0) for i in others]
    t = np.asarray(rows, dtype=np.int64)
    return t[rng.permutation(len(t))]


def _lists(users, rel, K, rng):
    """int32 [m, K] item rows, distinct inside a row, a random -1 tail; rows of user 2 hit the first and the last element of its
    relevant segment, user 3's rows hit all three of its items, user 5's rows are all padding."""
    out = np.full((len(users), K), -1, dtype=np.int32)
    for row, u in enumerate(users):
        length = int(rng.integers(0, K + 1)) if rng.random() < 0.5 else K
        pool = rng.permutation(N_ITEMS)
        if rng.random() < 0.7 and len(rel[u]):                                        # (hits are rare among 500 items otherwise)
            liked = rng.permutation(rel[u])[:K]
            pool = np.concatenate([liked, np.setdiff1d(pool, liked, assume_unique=True)])
            pool[:K] = rng.permutation(pool[:K])
        out[row, :length] = pool[:length]
        if u == 2:
            rest = np.setdiff1d(rng.permutation(N_ITEMS), [rel[2][0], rel[2][-1]], assume_unique=True)[:K]
            out[row] = rest
            out[row, 0] = rel[2][-1]
            out[row, K - 1] = rel[2][0]
        elif u == 3 and K >= 3:
            rest = np.setdiff1d(rng.permutation(N_ITEMS), rel[3], assume_unique=True)[:K]
            out[row] = rest
            out[row, [0, K // 2, K - 1]] = rel[3]
        elif u == 5:
            out[row] = -1
    return out


def _node_ids(lists):
    return np.where(lists >= 0, lists.astype(np.int64) + N_USERS, -1)


@pytest.fixture(scope='module')
def ranking_data():
    rng = np.random.default_rng(11 + helpers.seed_offset())
    rel = _relevant_sets(rng)
    return {'rel': rel, 'ratings': _test_ratings(rel, rng), 'rng': rng}


def _compare(got, want, ks):
    assert got['users_evaluated'] == want['users_evaluated'] and got['users_skipped'] == want['users_skipped']
    assert set(got) == set(want)
    for k in ks:
        for name in METRICS:
            key = '{}_at_{}'.format(name, k)
            assert abs(got[key] - want[key]) <= TOL, (key, got[key], want[key])


def _both(users, lists, ratings, ks, all_users=False):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics, full_ranking_metrics_device
    want = full_ranking_metrics(users, _node_ids(lists), ratings, ks)
    dev = torch.from_numpy(lists).to(DEV)
    got = full_ranking_metrics_device(None if all_users else users, dev, ratings, ks, N_USERS, N_ITEMS)
    again = full_ranking_metrics_device(None if all_users else users, dev, ratings, ks, N_USERS, N_ITEMS)
    assert got == again                                                              # the same bits on every run
    return got, want


@pytest.mark.parametrize('K,ks', [(64, [1, 5, 10, 64]), (1, [1]), (64, [1, 2, 3, 5, 10, 20, 50, 64])])
def test_kernel_against_the_host_function(hip, ranking_data, K, ks):
    assert 'amar_rank_metrics_f64' in hip.SIGNATURES
    d = ranking_data
    rng = np.random.default_rng(5 + K + len(ks) + helpers.seed_offset())
    users = np.arange(N_USERS)
    got, want = _both(users, _lists(users, d['rel'], K, rng), d['ratings'], ks, all_users=True)
    _compare(got, want, ks)
    assert want['users_skipped'] >= 1 and want['users_evaluated'] > 200
    if K == 64:
        assert want['hit_at_64'] > 0.5 and 0.0 < want['ndcg_at_64'] < 1.0            # (the data exercises hits, not only misses)
    special = np.array([0, 1, 2, 3, 4, 5])
    for m in (1, 7, 257):                                                            # subsets in arbitrary order, users repeated
        sub = np.concatenate([rng.permutation(special), rng.integers(0, N_USERS, size=300)])[:m] if m > 1 else np.array([2])
        if m == 257:
            sub[-1] = sub[0]
            sub = sub[rng.permutation(m)]
        got, want = _both(sub, _lists(sub, d['rel'], K, rng), d['ratings'], ks)
        _compare(got, want, ks)
        assert got['users_evaluated'] + got['users_skipped'] == m
    only_skipped = np.array([0, 0, 0])                                               # nobody evaluated: the sums (zeros), as on the host
    got, want = _both(only_skipped, _lists(only_skipped, d['rel'], K, rng), d['ratings'], ks)
    _compare(got, want, ks)
    assert got['users_evaluated'] == 0 and got['users_skipped'] == 3


def test_kernel_single_user_by_hand(hip):
    """One user, relevant rows {3, 7, 9}, list [7, 1, 9, -1]: hits at ranks 1 and 3."""
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics_device
    ratings = np.array([[0, 3 + 1, 1], [0, 7 + 1, 1], [0, 9 + 1, 1], [0, 1 + 1, 0]], dtype=np.int64)
    lists = torch.tensor([[7, 1, 9, -1]], dtype=torch.int32, device=DEV)
    got = full_ranking_metrics_device(None, lists, ratings, [1, 2, 4], 1, 12)
    d = 1.0 / np.log2(np.arange(4) + 2.0)
    assert got['users_evaluated'] == 1 and got['users_skipped'] == 0
    assert got['precision_at_1'] == 1.0 and got['precision_at_2'] == 0.5 and got['precision_at_4'] == 0.5
    assert abs(got['recall_at_4'] - 2.0 / 3.0) <= TOL and got['hit_at_1'] == 1.0
    assert abs(got['ndcg_at_4'] - (d[0] + d[2]) / (d[0] + d[1] + d[2])) <= TOL
    assert abs(got['ndcg_at_2'] - d[0] / (d[0] + d[1])) <= TOL and got['ndcg_at_1'] == 1.0


# ---- 2. evaluate_ranking on both routes ---------------------------------------------------------------------------------------------
def _held_out(g, rng, n=400):
    """Test ratings of a tiny_graph: pairs outside the training ratings, labels 0 / 1."""
    nu, ni = g['n_users'], g['n_items']
    seen = set((g['ratings'][:, 0] * ni + g['ratings'][:, 1] - nu).tolist())
    keys = np.array([k for k in rng.permutation(nu * ni) if k not in seen][:n])
    return np.stack([keys // ni, keys % ni + nu, (rng.random(len(keys)) < 0.5).astype(np.int64)], axis=1)


def _check_evaluate_ranking(model, train, test, route):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics
    assert model._recommend_route(train) == route
    ks = [1, 5, 10]
    for users in (None, np.array([5, 3, 3, 17, 0])):
        got = model.evaluate_ranking(train, test, ks, users=users)
        ru, ri, _ = model.recommend(train, k=10, users=users)
        want = full_ranking_metrics(ru, ri, test, ks)
        _compare(got, want, ks)
        assert want['users_evaluated'] > 0
    got = model.evaluate_ranking(train, test, [5], exclude_seen=False)
    _compare(got, full_ranking_metrics(*model.recommend(train, k=5, exclude_seen=False)[:2], test, [5]), [5])


def test_evaluate_ranking_fused_route(hip):
    g, _ = _bce_sequence()
    model = _bce_model(g, 'BasicGCN')
    helpers.spread_scores(model, 10.0)
    test = _held_out(g, np.random.default_rng(3))
    _check_evaluate_ranking(model, _Train(g['ratings'], g['n_users'], g['n_items']), test, 'fused')


def test_evaluate_ranking_pair_route(hip):
    """BasicRS without a hidden classifier layer: the head the pair route ranks."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    set_seed(7)
    g = helpers.tiny_graph(n_users=45, n_items=70, n_ratings=900, seed=9)
    table = np.random.default_rng(4).normal(0, 1, size=(g['n_users'] + g['n_items'], 32)).astype(np.float32)
    model = basic.BasicRS(dense_units=[64, 32], clf_units=[])
    model.build_head(32, 32)
    helpers.randomize_biases(model, seed=1)
    with torch.no_grad():
        model.clf.layers[-1].kernel.mul_(10.0)
    train = UserItemEmbeddings(g['ratings'], g['users'], g['items'], table)
    _check_evaluate_ranking(model, train, _held_out(g, np.random.default_rng(6)), 'pairs')


def test_models_without_recommend_refuse_ranking(hip):
    from deep_cbrs_amar_renaissance_amd import engine, training

    class Bare(engine.Model):
        pass

    with pytest.raises(NotImplementedError):
        Bare().evaluate_ranking(None, None, [5])
    with pytest.raises(NotImplementedError):
        training.fit(Bare(), [], epochs=1, validation_ranking={'trainset': None, 'ratings': None, 'ks': [5]})


# ---- 3. training is not disturbed ----------------------------------------------------------------------------------------------------
class _Noop:
    """Duck-typed callback with every hook, batch hooks included; counts its calls."""

    def __init__(self):
        self.calls = {}

    def _count(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        self._count('train_begin')

    def on_train_end(self, logs=None):
        self._count('train_end')

    def on_epoch_begin(self, epoch, logs=None):
        self._count('epoch_begin')

    def on_epoch_end(self, epoch, logs=None):
        self._count('epoch_end')

    def on_train_batch_begin(self, batch, logs=None):
        assert logs == {}
        self._count('batch_begin')

    def on_train_batch_end(self, batch, logs=None):
        assert logs == {}
        self._count('batch_end')


def _validation_args(g, seq_cls_ratings=None):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    test = _held_out(g, np.random.default_rng(2))
    val = UserItemGraph(test, g['users'], g['items'], g['adj'], batch_size=128)
    ranking = {'trainset': _Train(g['ratings'], g['n_users'], g['n_items']), 'ratings': test, 'ks': [5, 10], 'users': None}
    return val, ranking, test


@pytest.mark.parametrize('case', ['single', 'dropout', 'bpr'])
def test_validation_leaves_training_bit_for_bit(hip, case):
    from tests.test_bpr_gpu import _sample_sequence
    models, hists, cb = [], [], _Noop()
    for validated in (False, True):
        if case == 'bpr':
            seq = _sample_sequence()
            g = helpers.tiny_graph(n_users=70, n_items=50, n_ratings=1400, seed=3)
            g['adj'] = seq.adj_matrix
            g['ratings'] = seq.ratings
            model = _bpr_model(seq, 'BasicGCN', dropout=0.2)
        else:
            g, seq = _bce_sequence(shuffle=True)
            model = _bce_model(g, 'BasicGCN', **(dict(dropout=0.2) if case == 'dropout' else {}))
        kwargs = {}
        if validated:
            val, ranking, _ = _validation_args(g)
            kwargs = dict(validation_data=val, validation_ranking=ranking, callbacks=[cb])
        hists.append(model.fit(seq, epochs=3, verbose=False, **kwargs))
        models.append(model)
    assert hists[0]['loss'] == hists[1]['loss'] and len(hists[1]['val_loss']) == 3 and 'val_loss' not in hists[0]
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pa, pb), name
    assert models[0]._trainer.t == models[1]._trainer.t
    assert models[1].gnn.hoist is False and getattr(models[1].gnn, '_hoisted', None) is None and models[1]._towers is None
    steps = 3 * len(seq)
    assert cb.calls == {'train_begin': 1, 'train_end': 1, 'epoch_begin': 3, 'epoch_end': 3, 'batch_begin': steps, 'batch_end': steps}


# ---- 4. history ------------------------------------------------------------------------------------------------------------------------
class _EvaluateAtEpochEnd:
    def __init__(self, val):
        self.val, self.seen, self.logs = val, [], []

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        self.seen.append((epoch, self.model.evaluate(self.val)))
        self.logs.append(dict(logs))


def test_history_holds_what_evaluate_returns(hip):
    g, seq = _bce_sequence(shuffle=True)
    model = _bce_model(g, 'BasicGCN')
    val, ranking, test = _validation_args(g)
    spy = _EvaluateAtEpochEnd(val)
    h = model.fit(seq, epochs=3, verbose=False, validation_data=val, validation_ranking=ranking, callbacks=[spy])
    assert len(h['loss']) == len(h['val_loss']) == len(h['val_accuracy']) == len(h['val_ndcg_at_10']) == 3
    for epoch, (loss, acc) in spy.seen:
        assert h['val_loss'][epoch] == loss and h['val_accuracy'][epoch] == acc
    for epoch, logs in enumerate(spy.logs):
        assert logs['loss'] == h['loss'][epoch] and logs['val_loss'] == h['val_loss'][epoch]
        assert list(logs)[:2] == ['loss', 'accuracy']                                # training entries first, then val_*
    after = model.evaluate_ranking(ranking['trainset'], test, [5, 10])
    for name in METRICS:
        for k in (5, 10):
            assert h['val_{}_at_{}'.format(name, k)][-1] == after['{}_at_{}'.format(name, k)]
    assert 'val_users_evaluated' not in h


def test_validation_freq_and_initial_epoch(hip):
    g, seq = _bce_sequence()
    model = _bce_model(g, 'BasicGCN')
    val, _, _ = _validation_args(g)
    spy = _EvaluateAtEpochEnd(val)
    h = model.fit(seq, epochs=4, verbose=False, validation_data=val, validation_freq=2, callbacks=[spy])
    assert len(h['loss']) == 4 and len(h['val_loss']) == len(h['val_accuracy']) == 2
    assert h['val_loss'] == [spy.seen[1][1][0], spy.seen[3][1][0]]
    assert ['val_loss' in logs for logs in spy.logs] == [False, True, False, True]
    h = model.fit(seq, epochs=6, initial_epoch=4, verbose=False, validation_data=val)
    assert len(h['loss']) == len(h['val_loss']) == 2
    with pytest.raises(ValueError):
        model.fit(seq, epochs=1, verbose=False, validation_data=val, validation_freq=0)


# ---- 5. early stopping ------------------------------------------------------------------------------------------------------------------
class _Scripted:
    def __init__(self, values):
        self.values, self.snapshots = values, []

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        logs['scripted'] = self.values[epoch]
        self.snapshots.append([p.detach().clone() for p in self.model.parameters()])


def test_early_stopping_restores_the_best_epoch(hip):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.utilities.keras import EarlyStopping, set_weights_device
    g, seq = _bce_sequence(shuffle=True)
    model = _bce_model(g, 'BasicGCN')
    train = _Train(g['ratings'], g['n_users'], g['n_items'])
    pairs = UserItemGraph(g['ratings'][:300], g['users'], g['items'], g['adj'], batch_size=128)
    model.predict(pairs)                                                             # a captured predict graph and a split plan exist
    model.recommend(train, k=5)
    script = _Scripted([1.0, 0.9, 0.95, 0.97, 0.5])
    stop = EarlyStopping(monitor='scripted', patience=2, restore_best_weights=True)
    h = model.fit(seq, epochs=5, verbose=False, callbacks=[script, stop])
    assert len(h['loss']) == 4 and stop.stopped_epoch == 3 and stop.best_epoch == 1 and model.stop_training
    for prm, want in zip(model.parameters(), script.snapshots[1]):
        assert torch.equal(prm, want)
    assert not all(torch.equal(a, b) for a, b in zip(script.snapshots[1], script.snapshots[3]))
    fresh = _bce_model(g, 'BasicGCN', seed=99)
    set_weights_device(fresh, script.snapshots[1])
    assert np.array_equal(model.predict(pairs), fresh.predict(pairs))
    for got, want in zip(model.recommend(train, k=5), fresh.recommend(train, k=5)):
        assert np.array_equal(got, want)
    before = [p.detach().clone() for p in model.parameters()]
    h2 = model.fit(seq, epochs=1, verbose=False)                                     # trains on
    assert len(h2['loss']) == 1 and np.isfinite(h2['loss'][0]) and not model.stop_training
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_model_checkpoint_saves_what_load_weights_reads(hip, tmp_path):
    from deep_cbrs_amar_renaissance_amd.utilities.keras import ModelCheckpoint
    g, seq = _bce_sequence()
    model = _bce_model(g, 'BasicGCN')
    val, _, _ = _validation_args(g)
    ckpt = ModelCheckpoint(str(tmp_path / 'w_{epoch:02d}_{val_loss:.3f}'), monitor='val_loss', save_best_only=False)
    h = model.fit(seq, epochs=2, verbose=False, validation_data=val, callbacks=[ckpt])
    assert len(ckpt.saved) == 2 and ckpt.saved[1].endswith('w_02_{:.3f}'.format(h['val_loss'][1]))
    fresh = _bce_model(g, 'BasicGCN', seed=5)
    fresh.load_weights(ckpt.saved[1])
    for a, b in zip(model.parameters(), fresh.parameters()):
        assert torch.equal(a, b)


# ---- 6. the resident-table head -----------------------------------------------------------------------------------------------------------
def test_head_trainer_validates_and_stops(hip):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.keras import EarlyStopping
    g = helpers.tiny_graph(n_users=45, n_items=70, n_ratings=900, seed=9)
    table = np.random.default_rng(4).normal(0, 1, size=(g['n_users'] + g['n_items'], 32)).astype(np.float32)
    test = _held_out(g, np.random.default_rng(8))
    seq = UserItemEmbeddings(g['ratings'], g['users'], g['items'], table, batch_size=128, shuffle=True)
    val = UserItemEmbeddings(test, g['users'], g['items'], table, batch_size=128)
    models, hists = [], []
    for validated in (False, True):
        set_seed(7)
        model = basic.BasicRS(dense_units=[64, 32], clf_units=[64, 64])
        model.build_head(32, 32)
        model.compile(loss='binary_crossentropy', optimizer=Adam(learning_rate=1e-3), metrics=['accuracy'])
        seq_run = UserItemEmbeddings(g['ratings'], g['users'], g['items'], table, batch_size=128, shuffle=True)
        spy = _EvaluateAtEpochEnd(val)
        kwargs = dict(validation_data=val, validation_ranking={'trainset': seq, 'ratings': test, 'ks': [5]}, callbacks=[spy]) if validated else {}
        hists.append(model.fit(seq_run, epochs=3, verbose=False, **kwargs))
        models.append(model)
    assert models[1]._trainer.tables is not None                                     # the resident-table path
    assert hists[0]['loss'] == hists[1]['loss'] and len(hists[1]['val_loss']) == len(hists[1]['val_ndcg_at_5']) == 3
    for a, b in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(a, b)
    for epoch, (loss, acc) in spy.seen:
        assert hists[1]['val_loss'][epoch] == loss and hists[1]['val_accuracy'][epoch] == acc
    script = _Scripted([1.0, 0.9, 0.95, 0.97, 0.5])
    stop = EarlyStopping(monitor='scripted', patience=2, restore_best_weights=True)
    h = models[1].fit(seq, epochs=5, verbose=False, callbacks=[script, stop])
    assert len(h['loss']) == 4 and stop.best_epoch == 1
    for prm, want in zip(models[1].parameters(), script.snapshots[1]):
        assert torch.equal(prm, want)


# ---- 7. experiment ------------------------------------------------------------------------------------------------------------------------
def _run_experiment(tmp_path, name, validation, paths, epochs=4):
    import glob
    import json
    import yaml
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(paths)
    cfg['parameters']['epochs'] = epochs
    if validation:
        cfg['parameters']['validation'] = validation
    (tmp_path / (name + '.yaml')).write_text(yaml.safe_dump(cfg))
    (tmp_path / (name + '_exps.yaml')).write_text(
        "linear:\n  gcn:\n    model:\n      name: basic.BasicGCN\n      embedding_dim: 8\n      n_hiddens: [8, 8]\n"
        "      dense_units: [24, 24]\n      clf_units: [48, 48]\n    dataset:\n      load_function_name: load_user_item_graph\n")
    run_log = setup_mlflow(name, str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / (name + '.yaml')), str(tmp_path / (name + '_exps.yaml')), run_log)
    results = multi.run()
    assert all(v is not None for v in results.values())
    runs = glob.glob(str(tmp_path / 'mlruns' / name / '*'))
    assert len(runs) == 1
    return runs[0]


def _files(run):
    import os
    return sorted(os.path.relpath(os.path.join(d, f), run) for d, _, fs in os.walk(run) for f in fs)


def test_experiment_with_validation(hip, tmp_path, monkeypatch):
    import json
    import os
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:12000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:2000]
    ds.props = None
    paths = {k: v for k, v in synthetic.write_dataset(ds, str(tmp_path / 'datasets')).items() if k != 'props_triples_filepath'}
    seen = {}
    original = experiment.Experimenter.train

    def spy(self):
        seen['exp'] = self
        return original(self)

    monkeypatch.setattr(experiment.Experimenter, 'train', spy)
    monkeypatch.chdir(tmp_path)
    validation = {'fraction': 0.1, 'freq': 1, 'ranking_ks': [10],
                  'early_stopping': {'monitor': 'val_loss', 'patience': 1, 'restore_best_weights': True}}
    run_on = _run_experiment(tmp_path, 'with_validation', validation, paths)
    exp = seen.pop('exp')
    steps, final = {}, {}
    for line in open(os.path.join(run_on, 'run.jsonl')):
        rec = json.loads(line)
        if rec['event'] == 'metrics' and 'step' in rec:
            steps[rec['step']] = rec['metrics']
        elif rec['event'] == 'metrics':
            final.update(rec['metrics'])
    assert steps and sorted(steps) == list(range(len(steps))) and len(steps) <= 4
    for logged in steps.values():
        assert {'loss', 'val_loss', 'val_accuracy', 'val_ndcg_at_10', 'val_precision_at_10', 'val_recall_at_10', 'val_hit_at_10'} <= set(logged)
    assert 'stopped_epoch' in final and 'best_epoch' in final and final['best_epoch'] <= len(steps) - 1
    # the held-out rows: written, disjoint from the kept part, and no edge of the training graph
    kept = pd.read_csv(os.path.join(run_on, 'artifacts', 'validation', 'train_kept.tsv'), sep='\t', header=None).to_numpy()
    held = pd.read_csv(os.path.join(run_on, 'artifacts', 'validation', 'validation.tsv'), sep='\t', header=None).to_numpy()
    assert len(kept) + len(held) == len(ds.train) and 0.08 * len(ds.train) <= len(held) <= 0.1 * len(ds.train)
    val = exp.valset.ratings
    assert len(val) == len(held) and len(exp.trainset.ratings) == len(kept)
    adj = exp.trainset.adj_matrix.tocsr()
    assert adj[val[:, 0], val[:, 1]].sum() == 0 and adj[val[:, 1], val[:, 0]].sum() == 0
    liked = exp.trainset.ratings[exp.trainset.ratings[:, 2] == 1]              # (the unary adjacency links the liked pairs)
    assert adj[liked[:, 0], liked[:, 1]].min() > 0 and (val[:, 2] == 1).sum() > 100
    # without the key: the files of a run as it always was
    run_off = _run_experiment(tmp_path, 'without_validation', None, paths, epochs=1)
    extra = {os.path.join('artifacts', 'validation', 'train_kept.tsv'), os.path.join('artifacts', 'validation', 'validation.tsv')}
    assert set(_files(run_on)) - extra == set(_files(run_off)) and extra <= set(_files(run_on))
    assert not any('step' in json.loads(line) for line in open(os.path.join(run_off, 'run.jsonl')))

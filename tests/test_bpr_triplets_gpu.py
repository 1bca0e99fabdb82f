"""GPU: BPR triples — amar_bpr_sample_triplets_i32 against the numpy statement of its draws id for id, fit() on the
UserItemGraphTriplets Sequence replayed = eager bit for bit, samplers and graphs per Sequence, learning a per-user signal,
validation_ranking, the experiment end to end, and the refusals (pytest -m gpu)."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import bpr_triplets_cases as cases
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EINVAL = -1
PAD = 64


def _upload(seq):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (*seq.pos_csr, *seq.excl_csr)]


@pytest.mark.parametrize('exclude', ['positives', 'rated'])
@pytest.mark.parametrize('sample_by', ['user', 'interaction'])
def test_kernel_matches_restatement(hip, sample_by, exclude):
    """70 users x 50 items with a user of d = n_items - 1 and a user of one positive; h on both sides of the workgroup width; the
    outputs sit in front of canary padding."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import SAMPLE_BY, bpr_triplet_device_batch
    seq = cases.triplet_sequence(exclude=exclude, sample_by=sample_by)
    assert np.diff(seq.excl_csr[0])[cases.FULL_USER] == 49 and np.diff(seq.pos_csr[0])[cases.SINGLE_USER] == 1
    pp, pi, xp, xi = _upload(seq)
    mode = SAMPLE_BY[sample_by]
    for h, K in ((1, 1), (255, 1), (256, 1), (257, 1), (1000, 1), (1000, 4)):
        for seed in (42, 2 ** 40 + 11):
            for step in (0, 2 ** 33 + 9):
                st = torch.tensor([step], dtype=torch.int64, device=DEV)
                u = torch.full((2 * h + PAD,), -5, dtype=torch.int32, device=DEV)
                i = torch.full((2 * h + PAD,), -5, dtype=torch.int32, device=DEV)
                y = torch.full((2 * h + PAD,), -5.0, device=DEV)
                hip.bpr_sample_triplets(pp, pi, xp, xi, 70, 50, 70, seed, st, u[:2 * h], i[:2 * h], y[:2 * h], n_negatives=K, mode=mode)
                (wu, wi), wy = bpr_triplet_device_batch(seq.pos_csr, seq.excl_csr, 70, 50, 70, seed, step, h, K, sample_by)
                case = (h, K, seed, step)
                assert np.array_equal(u[:2 * h].cpu().numpy(), wu) and np.array_equal(i[:2 * h].cpu().numpy(), wi), case
                assert np.array_equal(y[:2 * h].cpu().numpy(), wy.astype(np.float32)), case
                assert bool((u[2 * h:] == -5).all()) and bool((i[2 * h:] == -5).all()) and bool((y[2 * h:] == -5.0).all()), case
                assert int(st.item()) == step + 1, case                  # the counter moved on by one batch
                hip.bpr_sample_triplets(pp, pi, xp, xi, 70, 50, 70, seed, st, u[:2 * h], i[:2 * h], None, n_negatives=K, mode=mode,
                                        advance=False)
                assert int(st.item()) == step + 1, case                  # ... and stays without `advance`
                want = bpr_triplet_device_batch(seq.pos_csr, seq.excl_csr, 70, 50, 70, seed, step + 1, h, K, sample_by)[0]
                assert np.array_equal(u[:2 * h].cpu().numpy(), want[0]) and np.array_equal(i[:2 * h].cpu().numpy(), want[1]), case
                assert bool((y[:2 * h] == torch.from_numpy(wy.astype(np.float32)).to(DEV)).all())   # y = NULL: not written
    (wu, wi), _ = bpr_triplet_device_batch(seq.pos_csr, seq.excl_csr, 70, 50, 70, 42, 0, 1000, 1, sample_by)
    full = wu[:1000] == cases.FULL_USER
    assert full.any() and np.all(wi[1000:][full] == 70 + cases.FREE_ITEM)   # (the single candidate of the d = n_items - 1 user)
    assert (wu[:1000] == cases.SINGLE_USER).any()


def test_kernel_invalid_arguments(hip):
    seq = cases.triplet_sequence()
    pp, pi, xp, xi = _upload(seq)
    h = 8
    st = torch.tensor([3], dtype=torch.int64, device=DEV)
    u = torch.full((2 * h,), -5, dtype=torch.int32, device=DEV)
    i = torch.full((2 * h,), -5, dtype=torch.int32, device=DEV)
    y = torch.full((2 * h,), -5.0, device=DEV)
    fn = hip.load().amar_bpr_sample_triplets_i32
    good = dict(pos_ptr=pp.data_ptr(), pos_ids=pi.data_ptr(), excl_ptr=xp.data_ptr(), excl_ids=xi.data_ptr(), n_users=70, n_items=50,
                item_base=70, K=1, mode=0, seed=42, step=st.data_ptr(), advance=1, h=h, u=u.data_ptr(), items=i.data_ptr(),
                y=y.data_ptr())

    def call(**change):
        a = dict(good, **change)
        code = fn(a['pos_ptr'], a['pos_ids'], a['excl_ptr'], a['excl_ids'], a['n_users'], a['n_items'], a['item_base'], a['K'], a['mode'],
                  ctypes.c_uint64(a['seed']), a['step'], a['advance'], a['h'], a['u'], a['items'], a['y'],
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return code
    for name in ('pos_ptr', 'pos_ids', 'excl_ptr', 'excl_ids', 'step', 'u', 'items'):
        assert call(**{name: None}) == EINVAL, name
    for change in (dict(n_users=0), dict(n_items=0), dict(h=0), dict(K=0), dict(n_users=-1), dict(h=-4), dict(K=-1),
                   dict(h=8, K=3), dict(h=7, K=2), dict(mode=2), dict(mode=-1)):
        assert call(**change) == EINVAL, change
    assert int(st.item()) == 3 and bool((u == -5).all()) and bool((i == -5).all()) and bool((y == -5.0).all())   # nothing ran
    assert call(y=None) == 0 and call(K=4, mode=1) == 0 and int(st.item()) == 5
    with pytest.raises(ValueError):
        hip.bpr_sample_triplets(pp, pi, xp, xi, 70, 50, 70, 42, st, u, i, y, n_negatives=3)
    with pytest.raises(ValueError):
        hip.bpr_sample_triplets(pp, pi, xp, xi, 70, 50, 70, 42, st, u, i[:8], y)


def _model(seq, cls='BasicGCN', seed=8, learning_rate=1e-3):
    from tests.test_bpr_gpu import _bpr_model
    return _bpr_model(seq, cls=cls, seed=seed, learning_rate=learning_rate)


@pytest.mark.parametrize('sample_by, n_negatives', [('user', 1), ('interaction', 4)])
def test_fit_replayed_equals_eager(hip, monkeypatch, sample_by, n_negatives):
    seq = cases.triplet_sequence(batch_size=128, sample_by=sample_by, n_negatives=n_negatives)
    models, hist = [], []
    for env in ('0', '1'):
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = _model(seq)
        hist.append(m.fit(seq, epochs=2, verbose=False)['loss'])
        models.append(m)
    assert models[1]._trainer._graphs and not models[0]._trainer._graphs
    assert hist[0] == hist[1] and np.isfinite(hist[0]).all()
    for pa, pb in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(pa, pb), tuple(pa.shape)
    assert models[0]._trainer.t == models[1]._trainer.t == 2 * len(seq)
    trainer = models[1]._trainer
    keys = [k for k in trainer._graphs if k[0] == 'sampled']
    assert len(keys) == 1 and keys[0][3] == trainer._sampler.serial
    g = trainer._graphs[keys[0]]
    last = int(trainer._sampler.step.item()) - 1
    assert last == 2 * len(seq) - 1
    (wu, wi), _ = seq.device_batch(last)
    assert np.array_equal(g['u'].cpu().numpy(), wu) and np.array_equal(g['i'].cpu().numpy(), wi)
    assert np.array_equal(wu[:64], wu[64:])                           # each pair under its own user


def test_second_sequence_gets_new_sampler_and_old_layout_still_fits(hip):
    from deep_cbrs_amar_renaissance_amd import training
    from tests.test_bpr_gpu import _sample_sequence
    first = cases.triplet_sequence(batch_size=128)
    model = _model(first)
    model.fit(first, epochs=1, verbose=False)
    trainer = model._trainer
    old = trainer._sampler
    assert isinstance(old, training.TripletSampler) and old.matches(first)
    model.fit(first, epochs=1, verbose=False)
    assert trainer._sampler is old                                    # the same Sequence keeps its lists and its graphs
    second = cases.triplet_sequence(batch_size=128, exclude='rated', n_negatives=2)
    model.fit(second, epochs=1, verbose=False)
    new = trainer._sampler
    assert new is not old and new.serial != old.serial and new.matches(second) and not new.matches(first)
    keys = [k for k in trainer._graphs if k[0] == 'sampled']
    assert keys and all(k[3] == new.serial for k in keys)
    step = int(new.step.item()) - 1
    assert step == len(second) - 1
    (wu, wi), _ = second.device_batch(step)
    g = trainer._graphs[keys[0]]
    assert np.array_equal(g['u'].cpu().numpy(), wu) and np.array_equal(g['i'].cpu().numpy(), wi)
    # the reference-layout Sequence on the same model (same 70 x 50 node space): its own sampler, its own graphs, its own layout
    legacy = _sample_sequence(batch_size=128)
    hist = model.fit(legacy, epochs=1, verbose=False)['loss']
    assert np.isfinite(hist).all() and isinstance(trainer._sampler, training.DeviceSampler) and trainer._sampler.matches(legacy)
    keys = [k for k in trainer._graphs if k[0] == 'sampled']
    assert keys and all(k[3] == trainer._sampler.serial for k in keys) and trainer._sampler.serial != new.serial
    (wu, wi), _ = legacy.device_batch(int(trainer._sampler.step.item()) - 1)
    g = trainer._graphs[keys[0]]
    assert np.array_equal(g['u'].cpu().numpy(), wu) and np.array_equal(g['i'].cpu().numpy(), wi)
    model.fit(second, epochs=1, verbose=False)                        # and back
    assert isinstance(trainer._sampler, training.TripletSampler) and trainer._sampler.matches(second)


def test_sampler_validates_the_lists_before_upload(hip):
    from deep_cbrs_amar_renaissance_amd import training
    seq = cases.triplet_sequence()
    ptr, ids = seq.pos_csr

    def broken(pos=None, excl=None):
        s = cases.triplet_sequence()
        s.pos_csr = pos if pos is not None else s.pos_csr
        s.excl_csr = excl if excl is not None else s.pos_csr
        return s
    swapped = ids.copy()
    lo = ptr[2]
    swapped[[lo, lo + 1]] = swapped[[lo + 1, lo]]
    repeated = ids.copy()
    repeated[lo + 1] = repeated[lo]
    outside = ids.copy()
    outside[-1] = 120
    below = ids.copy()
    below[ptr[2]] = 69
    everything = (np.arange(71, dtype=np.int32) * 50, np.tile(np.arange(70, 120, dtype=np.int32), 70))
    empty_row = (np.concatenate([ptr[:3], ptr[3:] - (ptr[3] - ptr[2])]).astype(np.int32), np.concatenate([ids[:ptr[2]], ids[ptr[3]:]]))
    for bad in (broken(excl=(ptr, swapped)), broken(excl=(ptr, repeated)), broken(excl=(ptr, outside)), broken(excl=(ptr, below)),
                broken(excl=everything), broken(pos=empty_row, excl=seq.pos_csr), broken(pos=(ptr, swapped), excl=seq.pos_csr),
                broken(excl=(ptr[:-1], ids))):
        with pytest.raises(ValueError):
            training.TripletSampler(bad, torch.device(DEV))
    assert training.TripletSampler(broken(pos=seq.pos_csr, excl=empty_row), torch.device(DEV)).h == 256   # d = 0 is fine


def test_learns_a_per_user_signal(hip):
    """Two user groups x two item groups, every user likes its own group only and every item is liked by the same number of users,
    so a per-item score ranks at chance; no dislikes anywhere (the reference-layout Sequence refuses such data).  24 liked items
    per user in training, 4 more held out.  Chance Recall@10 = 10 / (80 - 24) = 0.179.  Measured: 0.131 untrained,
    0.765 after 16 epochs (0.502 after 8)."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph, UserItemGraphPosNegSample, UserItemGraphTriplets
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics
    train, test, users, items = cases.two_group_data()
    n_users, n_items, seen = len(users), len(items), 24
    liked_by = np.bincount(train[:, 1] - n_users, minlength=n_items)
    assert np.all(liked_by == liked_by[0]) and np.all(train[:, 2] == 1) and np.all(np.bincount(train[:, 0]) == seen)
    assert np.all((train[:, 0] < n_users // 2) == (train[:, 1] - n_users < n_items // 2))   # own group only
    with pytest.raises(ValueError):
        UserItemGraphPosNegSample(train, users, items, build_adjacency_matrix(train, users, items, type_adjacency='binary'))
    adj = build_adjacency_matrix(train, users, items, type_adjacency='unary')
    seq = UserItemGraphTriplets(train, users, items, adj, batch_size=256, seed=42)
    trainset = UserItemGraph(train, users, items, adj)
    model = _model(seq, cls='BasicLightGCN', seed=3, learning_rate=1e-2)

    def recall():
        u, it, _ = model.recommend(trainset, k=10)
        return full_ranking_metrics(u, it, test, [10])['recall_at_10']
    before = recall()
    hist = model.fit(seq, epochs=16, verbose=False)['loss']
    after = recall()
    print('recall@10 before {:.4f} after {:.4f} loss {:.4f} -> {:.4f}'.format(before, after, hist[0], hist[-1]))
    chance = 10 / (n_items - seen)
    assert hist[-1] < hist[0]
    assert after >= 2 * chance, (before, after, chance)
    assert after > before, (before, after)


def test_fit_with_validation_ranking(hip):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    seq = cases.triplet_sequence(batch_size=128)
    rng = np.random.default_rng(2)
    held = np.stack([rng.integers(0, 70, 300), rng.integers(70, 120, 300), rng.integers(0, 2, 300)], axis=1)
    val = UserItemGraph(held, seq.users, seq.items, seq.adj_matrix, batch_size=128)
    model = _model(seq)
    h = model.fit(seq, epochs=2, verbose=False, validation_data=val, validation_ranking={'trainset': seq, 'ratings': held, 'ks': [5, 10]})
    assert len(h['loss']) == 2
    for k in (5, 10):
        assert len(h['val_recall_at_{}'.format(k)]) == 2 and all(0.0 <= v <= 1.0 for v in h['val_recall_at_{}'.format(k)])
    after = model.evaluate_ranking(seq, held, [5, 10])
    assert h['val_recall_at_10'][-1] == after['recall_at_10']
    only_ranking = model.fit(seq, epochs=1, verbose=False, validation_ranking={'trainset': seq, 'ratings': held, 'ks': [5]})
    assert len(only_ranking['val_recall_at_5']) == 1


def test_experiment_with_triplet_config(hip, tmp_path, monkeypatch):
    import yaml
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.train = ds.train[ds.train[:, 2] == 1]                          # likes only: implicit feedback, no dislike to sample from
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['parameters'].update({'epochs': 2, 'loss': 'BPRLoss', 'full_ranking_ks': [5, 10],
                              'validation': {'fraction': 0.1, 'ranking_ks': [10]}})
    cfg['model'].update({'name': 'basic.BasicLightGCN', 'embedding_dim': 8, 'n_layers': 2, 'dense_units': [24, 24],
                         'clf_units': [48, 48]})
    cfg['dataset'].update({k: v for k, v in paths.items() if k != 'props_triples_filepath'})
    cfg['dataset'].update({'load_function_name': 'load_user_item_graph_triplets', 'n_negatives': 4})
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / "exps.yaml").write_text("linear:\n  triplets:\n    model:\n      name: basic.BasicLightGCN\n")
    seen = {}
    original = experiment.Experimenter.train

    def spy(self):
        seen['exp'] = self
        return original(self)
    monkeypatch.setattr(experiment.Experimenter, 'train', spy)
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('triplets', str(tmp_path / 'mlruns'))
    results = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log).run()
    assert len(results) == 1 and all(v is not None for v in results.values())
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphTriplets
    exp = seen['exp']
    assert isinstance(exp.trainset, UserItemGraphTriplets) and exp.trainset.n_negatives == 4 and exp.trainset.batch_size == 1024
    assert isinstance(exp.model._trainer._sampler, training.TripletSampler) and exp.model._trainer.t == 2 * len(exp.trainset)
    runs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    assert len(runs) == 1
    metrics = {}
    for line in open(runs[0]):
        rec = json.loads(line)
        if rec['event'] == 'metrics':
            metrics.update(rec['metrics'])
    assert np.isfinite(metrics['test_loss']) and 'full_recall_at_10' in metrics and 'val_recall_at_10' in metrics
    art = os.path.dirname(runs[0])
    assert os.path.exists(os.path.join(art, 'artifacts', 'predictions/full_ranking/top_10.tsv'))


def test_refusals(hip):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    seq = cases.triplet_sequence(batch_size=128)
    model = _model(seq)
    with pytest.raises(ValueError, match='class_weight cannot weigh BPR training'):
        model.fit(seq, epochs=1, verbose=False, class_weight={0: 1.0, 1: 3.0})
    weighted = cases.triplet_sequence(batch_size=128)
    weighted.sample_weight = np.ones(len(weighted.ratings))
    with pytest.raises(ValueError, match='carries no sample weights'):
        model.fit(weighted, epochs=1, verbose=False)
    engine.set_seed(11)
    hyb = hybrid.HybridBertGCN(seq.adj_matrix, embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[[24, 16], [32, 24], [16, 16]],
                               clf_units=[24, 16], l2_regularizer=1e-4, feature_based=True, fusion_method='concatenate', residual=False)
    hyb.set_bert_table(np.random.default_rng(3).standard_normal((seq.adj_matrix.shape[0], 40)).astype(np.float32))
    hyb.compile(loss=BPRLoss())
    with pytest.raises(NotImplementedError, match='hybrid models do not train on it'):
        hyb.fit(seq, epochs=1, verbose=False)
    hist = model.fit(seq, epochs=1, verbose=False)['loss']            # the refusals left the model usable
    assert np.isfinite(hist).all()

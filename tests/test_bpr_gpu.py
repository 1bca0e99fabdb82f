"""GPU: BPR training — amar_bpr_grad_f32 / amar_bpr_sample_i32 against float64 and the numpy statement of the draws, the Trainer's
gradients under BPRLoss against autograd, replayed = eager fit() bit for bit, a new Sequence never replaying an old graph, learning,
the head-only BasicRS path and the experiment end to end (pytest -m gpu)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import train as otrain
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)


def _sample_sequence(n_users=70, n_items=50, n_ratings=1400, seed=3, batch_size=128, sample_seed=42):
    """A UserItemGraphPosNegSample over a random 0/1 rating set in which every user has a positive."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphPosNegSample
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    g = helpers.tiny_graph(n_users=n_users, n_items=n_items, n_ratings=n_ratings, seed=seed)
    r = g['ratings'].copy()
    first = np.unique(r[:, 0], return_index=True)[1]
    r[first, 2] = 1
    assert len(first) == n_users and len(np.unique(r[:, 1])) == n_items
    adj = build_adjacency_matrix(r, g['users'], g['items'], type_adjacency='binary')
    return UserItemGraphPosNegSample(r, g['users'], g['items'], adj, batch_size=batch_size, seed=sample_seed)


def _bpr64(p):
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    B, h = len(p), len(p) // 2
    x = p[:h] - p[h:2 * h]
    s = 1.0 / (1.0 + np.exp(-x))
    dz = np.zeros(B)
    dz[:h] = -(1 - s) * p[:h] * (1 - p[:h]) / h
    dz[h:2 * h] = (1 - s) * p[h:2 * h] * (1 - p[h:2 * h]) / h
    return float(np.mean(-np.log(s))), dz


@pytest.mark.parametrize('B', [2, 1024, 2047, 4096])
def test_bpr_grad_kernel(hip, B):
    rng = np.random.default_rng(B)
    wide = rng.uniform(0.01, 0.99, (B, 3)).astype(np.float32)
    pt = torch.from_numpy(wide).to(DEV)[:, 1:2]                      # strided [B, 1] column
    dz = torch.full((B, 1), 7.0, device=DEV)
    terms = torch.full((B,), 7.0, device=DEV)
    hip.bpr_grad(pt, dz, terms)
    loss, want_dz = _bpr64(wide[:, 1])
    t = terms.cpu().numpy().astype(np.float64)
    h = B // 2
    assert np.all(t[h:] == 0)
    x = wide[:h, 1].astype(np.float64) - wide[h:2 * h, 1]
    np.testing.assert_allclose(t[:h], (B / h) * np.log1p(np.exp(-x)), rtol=2e-6, atol=1e-7)
    assert abs(t.sum() / B - loss) <= 1e-5 * loss
    got = dz.cpu().numpy().reshape(-1).astype(np.float64)
    np.testing.assert_allclose(got, want_dz, rtol=2e-5, atol=1e-9)
    if B % 2:
        assert got[-1] == 0 and t[-1] == 0                           # the dropped trailing element
    again_dz, again_t = torch.empty_like(dz), torch.empty_like(terms)
    hip.bpr_grad(pt, again_dz, again_t)
    assert torch.equal(again_dz, dz) and torch.equal(again_t, terms)


def test_bpr_sample_kernel_matches_restatement(hip):
    seq = _sample_sequence(batch_size=1000)
    pp, pi = (torch.from_numpy(a).to(DEV) for a in seq.pos_csr)
    npt, ni = (torch.from_numpy(a).to(DEV) for a in seq.neg_csr)
    h = seq.batch_size // 2
    for seed, step in ((42, 0), (42, 1), (7, 3), (2 ** 40 + 11, 2 ** 33 + 9)):
        st = torch.tensor([step], dtype=torch.int64, device=DEV)
        u = torch.full((2 * h,), -5, dtype=torch.int32, device=DEV)
        i = torch.full((2 * h,), -5, dtype=torch.int32, device=DEV)
        y = torch.full((2 * h,), -5.0, device=DEV)
        hip.bpr_sample(pp, pi, npt, ni, len(seq.users), seed, st, u, i, y)
        from deep_cbrs_amar_renaissance_amd.data.datasets import bpr_device_batch
        (wu, wi), wy = bpr_device_batch(seq.pos_csr, seq.neg_csr, len(seq.users), seed, step, h)
        assert np.array_equal(u.cpu().numpy(), wu) and np.array_equal(i.cpu().numpy(), wi)
        assert np.array_equal(y.cpu().numpy(), wy.astype(np.float32))
        assert int(st.item()) == step + 1                             # the counter moved on by one batch
        hip.bpr_sample(pp, pi, npt, ni, len(seq.users), seed, st, u, i, advance=False)
        assert int(st.item()) == step + 1
        assert np.array_equal(i.cpu().numpy(), bpr_device_batch(seq.pos_csr, seq.neg_csr, len(seq.users), seed, step + 1, h)[0][1])


def _targets_for(p, c, eps=1e-7):
    """Targets y at which the oracle's BCE (Keras form: mean over B, epsilon inside the logs) has the data-loss cotangent
    d/dp = B^-1 * g with g = B * c, c = d(BPR)/dp: its autograd is then autograd of BPR + the same L2 terms."""
    B = len(p)
    g = B * c
    a, b = 1.0 / (p + eps), 1.0 / (1.0 - p + eps)
    return (b - g) / (a + b)


@pytest.mark.parametrize('cls', ['BasicGCN', 'BasicLightGCN', 'BasicGAT'])
def test_bpr_gradients_match_autograd(hip, cls):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests.test_training_gpu import _flatten_oracle_grads
    seq = _sample_sequence(batch_size=255)                          # h = 127 draws, 254 ids
    engine.set_seed(5)
    model = getattr(basic, cls)(seq.adj_matrix, **CFG)
    helpers.randomize_biases(model, seed=6)
    model.compile(loss=BPRLoss())
    (u, i), y = seq.device_batch(3)
    trainer = training.Trainer(model)
    loss, grads = trainer.loss_and_grads(u, i, y)
    gnn, head = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
    _, _, p = otrain.torch_model_grads(seq.adj_matrix, gnn, head, u, i, y, l2=1e-4)
    want_data, dz = _bpr64(p)
    c = dz / (p * (1 - p))                                           # d(BPR)/dp from d(BPR)/d(logit)
    bce_loss, want, _ = otrain.torch_model_grads(seq.adj_matrix, gnn, head, u, i, _targets_for(p, c), l2=1e-4)
    yt, pc = _targets_for(p, c), np.clip(p, 1e-7, 1 - 1e-7)
    l2_part = bce_loss - float(-np.mean(yt * np.log(pc + 1e-7) + (1 - yt) * np.log(1 - pc + 1e-7)))
    assert abs(loss - (want_data + l2_part)) < 1e-5
    flat = _flatten_oracle_grads(model, want)
    assert set(flat) == set(grads)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)
        # (absolute floor: the classifier's last bias gets sum(dz), in which BPR's two halves cancel — float32 rounding is relative
        # to sum |dz|, not to the small result)
        assert np.abs(got - gw).max() <= 2e-4 * np.abs(gw).max() + 2e-6 * np.abs(dz).sum(), tuple(prm.shape)


def _bpr_model(seq, cls='BasicGCN', seed=8, learning_rate=1e-3):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    engine.set_seed(seed)
    model = getattr(basic, cls)(seq.adj_matrix, **CFG)
    helpers.randomize_biases(model, seed=1)
    model.compile(loss=BPRLoss(), optimizer=Adam(learning_rate=learning_rate))
    model(seq[0][0])
    return model


def test_bpr_fit_replayed_equals_eager(hip, monkeypatch):
    seq = _sample_sequence()
    models, hist = [], []
    for env in ('0', '1'):
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = _bpr_model(seq)
        hist.append(m.fit(seq, epochs=2, verbose=False)['loss'])
        models.append(m)
    assert models[1]._trainer._graphs and not models[0]._trainer._graphs
    assert hist[0] == hist[1] and np.isfinite(hist[0]).all()
    for pa, pb in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(pa, pb), tuple(pa.shape)
    assert models[0]._trainer.t == models[1]._trainer.t == 2 * len(seq)


def test_second_fit_with_another_sequence_draws_from_its_lists(hip):
    first = _sample_sequence(sample_seed=42)
    model = _bpr_model(first)
    model.fit(first, epochs=1, verbose=False)
    trainer = model._trainer
    old = trainer._sampler
    second = _sample_sequence(sample_seed=42)
    second.pos_csr = (second.pos_csr[0], second.pos_csr[1])          # same content, another Sequence object
    keep = second.neg_csr
    second.neg_csr = (keep[0], np.roll(keep[1], 1))                 # other negative lists
    model.fit(second, epochs=1, verbose=False)
    assert trainer._sampler is not old and trainer._sampler.matches(second)
    keys = [k for k in trainer._graphs if k[0] == 'sampled']
    assert keys and all(k[3] == trainer._sampler.serial for k in keys)
    g = trainer._graphs[keys[0]]
    step = int(trainer._sampler.step.item()) - 1
    assert step == len(second) - 1
    (wu, wi), _ = second.device_batch(step)
    assert np.array_equal(g['u'].cpu().numpy(), wu) and np.array_equal(g['i'].cpu().numpy(), wi)


def test_compile_with_another_loss_captures_anew(hip):
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    seq = _sample_sequence()
    model = _bpr_model(seq)
    model.fit(seq, epochs=1, verbose=False)
    model.compile(loss='binary_crossentropy')
    model.fit(seq, epochs=1, verbose=False)
    kinds = {k[2] for k in model._trainer._graphs if k[0] == 'sampled'}
    assert kinds == {'bpr', 'bce'}
    model.compile(loss=BPRLoss())


def test_bpr_training_learns_full_ranking(hip):
    """Planted item quality: 25 good items and 95 bad ones; every user likes 12 good items and dislikes 6 bad ones in training, 6 more
    good items are its test positives.  (The signal is per item on purpose: the reference's batch layout scores pos_j against user
    batch_users[j // 2], not the user it was drawn for, which blurs per-user preferences.)  A few BPR epochs raise Recall@10 of
    recommend() well above the untrained model's."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph, UserItemGraphPosNegSample
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics
    rng = np.random.default_rng(0)
    n_users, n_items, n_good = 200, 120, 25
    good = rng.permutation(n_items)[:n_good]
    bad = np.setdiff1d(np.arange(n_items), good)
    train, test = [], []
    for u in range(n_users):
        g = rng.permutation(good)
        train += [(u, n_users + i, 1) for i in g[:12]] + [(u, n_users + i, 0) for i in rng.choice(bad, 6, replace=False)]
        test += [(u, n_users + i, 1) for i in g[12:18]]
    train, test = np.array(train), np.array(test)
    users, items = np.arange(n_users), np.arange(n_items)
    adj = build_adjacency_matrix(train, users, items, type_adjacency='binary')
    seq = UserItemGraphPosNegSample(train, users, items, adj, batch_size=256, seed=42)
    trainset = UserItemGraph(train, users, items, seq.adj_matrix)
    model = _bpr_model(seq, cls='BasicLightGCN', seed=3, learning_rate=1e-2)

    def recall():
        u, it, _ = model.recommend(trainset, k=10)
        return full_ranking_metrics(u, it, test, [10])['recall_at_10']
    before = recall()
    hist = model.fit(seq, epochs=40, verbose=False)['loss']
    after = recall()
    assert hist[-1] < hist[0]
    assert after > before + 0.15 and after > 2 * before, (before, after)


def test_head_only_basic_rs_with_bpr_loss(hip):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    engine.set_seed(4)
    rng = np.random.default_rng(6)
    n, d = 120, 16
    table = rng.standard_normal((n, d)).astype(np.float32) * 0.5
    r = np.stack([rng.integers(0, 60, 999), rng.integers(60, 120, 999), rng.integers(0, 2, 999)], axis=1)
    seq = UserItemEmbeddings(r, np.arange(60), np.arange(60), table, batch_size=200)   # last batch: 199 (odd)
    model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
    model.compile(loss=BPRLoss())
    hist = model.fit(seq, epochs=6, verbose=False)['loss']
    assert np.isfinite(hist).all() and np.all(np.diff(hist) < 0), hist
    assert ('bpr' in {k[2] for k in model._trainer._graphs})
    loss, acc = model.evaluate(seq)
    assert np.isfinite(loss) and 0 <= acc <= 1


def test_experiment_with_bpr_config(hip, tmp_path, monkeypatch):
    import yaml
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.train = ds.train[np.isin(ds.train[:, 0], ds.train[ds.train[:, 2] == 1, 0])]   # every user needs a positive to be sampled
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['parameters'].update({'epochs': 2, 'loss': 'BPRLoss', 'full_ranking_ks': [5, 10]})
    cfg['model'].update({'name': 'basic.BasicLightGCN', 'embedding_dim': 8, 'n_layers': 2, 'dense_units': [24, 24],
                         'clf_units': [48, 48]})
    cfg['dataset'].update({k: v for k, v in paths.items() if k != 'props_triples_filepath'})
    cfg['dataset'].update({'load_function_name': 'load_user_item_graph_sample', 'type_adjacency': 'binary'})
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / "exps.yaml").write_text("linear:\n  bpr:\n    model:\n      name: basic.BasicLightGCN\n")
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('bpr', str(tmp_path / 'mlruns'))
    results = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log).run()
    assert len(results) == 1 and all(v is not None for v in results.values())
    runs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    assert len(runs) == 1
    metrics = {}
    for line in open(runs[0]):
        rec = json.loads(line)
        if rec['event'] == 'metrics':
            metrics.update(rec['metrics'])
    assert np.isfinite(metrics['test_loss']) and 'full_recall_at_10' in metrics and 'precision_at_10' in metrics
    art = os.path.dirname(runs[0])
    for rel in ('predictions/top_5/predictions_1.tsv', 'predictions/top_10/results.tsv', 'predictions/full_ranking/top_10.tsv'):
        assert os.path.exists(os.path.join(art, 'artifacts', rel)), rel

"""GPU: listwise ranking losses — amar_group_loss_grad_f32 against the float64 restatement of tests/group_loss_ref.py on both kernel
forms and their segment edges, its bits' independence of a group's place in the batch, its refusals, and fit() under each loss on
the triplet Sequence: replayed = eager bit for bit, the first batch's loss, a second compile() capturing anew (pytest -m gpu)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from tests import bpr_triplets_cases as cases
from tests import group_loss_ref as ref
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EINVAL = -1
KERNEL_CASES = [(ref.SOFTMAX, 1.0), (ref.SOFTMAX, 0.05), (ref.HARDEST, 1.0), (ref.MARGIN, 1.0)]
KERNEL_IDS = ['softmax_t1', 'softmax_t0.05', 'hardest', 'margin']


def _run(hip, kind, hyper, p, K, column=False):
    """(dz, terms) of one launch as float32 numpy; column: p is the middle column of a [B, 3] array (ldp = 3)."""
    B = len(p)
    if column:
        wide = np.random.default_rng(B).uniform(0.0, 1.0, (B, 3)).astype(np.float32)
        wide[:, 1] = p
        pt = torch.from_numpy(wide).to(DEV)[:, 1:2]
    else:
        pt = torch.from_numpy(p).to(DEV)
    dz = torch.full((B, 1), 7.0, device=DEV)
    terms = torch.full((B,), 7.0, device=DEV)
    hip.group_loss_grad(kind, hyper, pt, dz, terms, n_negatives=K)
    return dz.cpu().numpy().reshape(-1), terms.cpu().numpy()


@pytest.mark.parametrize('K', ref.K_LADDER)
@pytest.mark.parametrize('kind, t', KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_against_float64(hip, kind, t, K):
    """Bounds: what tests/test_bpr_gpu.py allows amar_bpr_grad_f32 (terms rtol 2e-6 + 1e-7, dz rtol 2e-5 + 1e-9, batch loss 1e-5
    relative), for every kind.  A sequential float32 evaluation of the softmax leaves 0.27 / 0.07 of that bound (terms / dz) at
    t = 1 and 1.18 / 0.11 at t = 0.05 on these inputs (ref.F32_SEQUENTIAL, measured on the CPU: the exponent reaches 20 there, so
    one float32 rounding of it is 1e-6 of the exponential); the kernel measured 0.23 / 0.03 at most, so it needs no more."""
    hyper = ref.hyper_of(kind, t)
    bound_terms, bound_dz = ref.bounds(kind, t)
    for G, B, variant, p in ref.case_inputs(kind, hyper, K):
        loss, want_terms, want_dz = ref.group_loss(kind, hyper, p, K)
        dz0, t0 = ref.must_be_zero(B, K)
        first = None
        for column in (False, True):
            dz, terms = _run(hip, kind, hyper, p, K, column)
            case = (K, G, B, variant, column)
            assert np.all(dz[dz0] == 0) and np.all(terms[t0] == 0), case      # copies, negatives' terms, the trailing element
            e_terms = ref.scaled_error(terms, want_terms, ref.TERMS_RTOL, ref.TERMS_ATOL)
            e_dz = ref.scaled_error(dz, want_dz, ref.DZ_RTOL, ref.DZ_ATOL)
            e_loss = abs(terms.astype(np.float64).sum() / B - loss) / (1e-5 * loss) if loss else 0.0
            print(case, 'scaled error: terms {:.3f} dz {:.3f} loss {:.3f}'.format(e_terms, e_dz, e_loss))
            assert e_terms <= bound_terms and e_dz <= bound_dz and e_loss <= bound_terms, case
            if kind == ref.HARDEST:                                           # one negative per group carries the gradient
                h = B // 2
                assert np.array_equal(dz[h:2 * h] != 0, want_dz[h:2 * h] != 0), case
            if first is None:
                first = (dz, terms)
            else:                                                             # a strided column gives the same bits, and so does a rerun
                assert np.array_equal(dz, first[0]) and np.array_equal(terms, first[1]), case


@pytest.mark.parametrize('K', [1, 3, 32, 33, 200])
@pytest.mark.parametrize('kind, t', KERNEL_CASES, ids=KERNEL_IDS)
def test_bits_do_not_depend_on_where_a_group_sits(hip, kind, t, K):
    """The same group data at g = 0, in the middle and at g = G - 1 of a batch that spans several workgroups: identical dz and term
    bits (another lane segment, another wavefront, another workgroup); and a second launch repeats the first bit for bit."""
    hyper = ref.hyper_of(kind, t)
    G = 70 if K > 2 else 1000                                         # (K <= 2: 128 / 256 groups per workgroup)
    B, h = 2 * G * K + 1, G * K
    p = ref.draw(np.random.default_rng(K), B, K, kind, hyper)
    places = (0, G // 2 + 1, G - 1)
    for g in places[1:]:
        p[g * K] = p[0]
        p[h + g * K:h + (g + 1) * K] = p[h:h + K]
    dz, terms = _run(hip, kind, hyper, p, K)
    for g in places[1:]:
        assert terms[g * K] == terms[0] and dz[g * K] == dz[0], g
        assert np.array_equal(dz[h + g * K:h + (g + 1) * K], dz[h:h + K]), g
    assert terms[0] > 0 or kind == ref.MARGIN
    again = _run(hip, kind, hyper, p, K)
    assert np.array_equal(again[0], dz) and np.array_equal(again[1], terms)


def test_kernel_refusals_and_the_batch_without_a_pair(hip):
    fn = hip.load().amar_group_loss_grad_f32
    p = torch.full((24,), 0.5, device=DEV)
    dz = torch.full((24,), 7.0, device=DEV)
    terms = torch.full((24,), 7.0, device=DEV)

    def call(kind=ref.SOFTMAX, hyper=1.0, B=24, K=4, pp=p.data_ptr(), d=dz.data_ptr(), tt=terms.data_ptr(), ldp=1):
        code = fn(kind, ctypes.c_float(hyper), pp, ldp, d, tt, B, K, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return code
    for bad in (dict(K=0), dict(K=-1), dict(K=5), dict(B=22, K=4), dict(kind=3), dict(kind=-1), dict(hyper=0.0), dict(hyper=-1.0),
                dict(hyper=float('nan')), dict(kind=ref.MARGIN, hyper=-0.1), dict(kind=ref.MARGIN, hyper=float('nan')), dict(B=0),
                dict(pp=None), dict(d=None), dict(tt=None), dict(ldp=0)):
        assert call(**bad) == EINVAL, bad
    assert bool((dz == 7.0).all()) and bool((terms == 7.0).all())     # nothing ran
    assert call(kind=ref.HARDEST, hyper=-5.0) == 0                    # (the hardest-negative loss reads no hyper-parameter)
    assert call(kind=ref.MARGIN, hyper=0.0) == 0
    for kind in ref.KINDS:                                            # B = 1: no pair, zeros (as amar_bpr_grad_f32)
        dz.fill_(7.0), terms.fill_(7.0)
        assert call(kind=kind, B=1, K=4) == 0
        assert float(dz[0]) == 0 and float(terms[0]) == 0 and bool((dz[1:] == 7.0).all()) and bool((terms[1:] == 7.0).all())
    with pytest.raises(ValueError):
        hip.group_loss_grad(ref.SOFTMAX, 1.0, p, dz.reshape(-1, 1), terms, n_negatives=5)
    with pytest.raises(ValueError):
        hip.group_loss_grad(ref.SOFTMAX, 1.0, p, dz[:8].reshape(-1, 1), terms, n_negatives=4)


def test_library_exports_the_declared_entry_point(hip):
    """Header, binding and shared library agree: the symbol is exported and takes the declared arguments."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'amar_hip.h')).read()
    sym = 'amar_group_loss_grad_f32'
    decl = re.search(r'\bint\s+' + sym + r'\s*\(([^;]*)\)\s*;', header)
    assert decl and len(decl.group(1).split(',')) == len(hip.SIGNATURES[sym][1]) == 9
    lib = hip.load()
    assert getattr(lib, sym).argtypes == hip.SIGNATURES[sym][1] and getattr(lib, sym).restype is ctypes.c_int
    exported = subprocess.run(['nm', '-D', '--defined-only', lib._name], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\bT\s+' + sym + r'\b', exported)


# ---- fit() on the triplet Sequence -------------------------------------------------------------------------------------------------------
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48])


def _losses():
    from deep_cbrs_amar_renaissance_amd.utilities.losses import HardestNegativeBPRLoss, MarginRankingLoss, SampledSoftmaxLoss
    return {'softmax': lambda: SampledSoftmaxLoss(temperature=0.2), 'hardest': HardestNegativeBPRLoss,
            'margin': lambda: MarginRankingLoss(margin=0.3)}


@pytest.fixture(scope='module')
def tiny_triplets(tmp_path_factory):
    """24 users x 40 items (two groups, likes only) through load_user_item_graph_triplets: n_negatives = 4, batch 64 -> 8 groups."""
    from deep_cbrs_amar_renaissance_amd.data import loaders
    train, test, _, _ = cases.two_group_data(n_users=24, n_items=40, n_train=5, n_test=1)
    d = tmp_path_factory.mktemp('group_losses')
    paths = {}
    for name, part in (('train', train), ('test', test)):
        paths[name] = str(d / (name + '.tsv'))
        np.savetxt(paths[name], part, fmt='%d', delimiter='\t')
    seq, _ = loaders.load_user_item_graph_triplets(paths['train'], paths['test'], train_batch_size=64, n_negatives=4)
    assert seq.adj_matrix.shape == (64, 64) and seq.n_negatives == 4 and len(seq) == 15     # (8 draws a batch)
    return seq


def _model(seq, cls, loss, l2=1e-4, seed=8):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.experiment import Adam
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(seed)
    model = getattr(basic, cls)(seq.adj_matrix, l2_regularizer=l2, **CFG)
    helpers.randomize_biases(model, seed=1)
    model.compile(loss=loss, optimizer=Adam(learning_rate=1e-3))
    model(seq[0][0])
    return model


@pytest.mark.parametrize('name', ['softmax', 'hardest', 'margin'])
@pytest.mark.parametrize('cls', ['BasicLightGCN', 'BasicGCN'])
def test_fit_replayed_equals_eager_and_a_second_compile_captures_anew(hip, monkeypatch, tiny_triplets, cls, name):
    """3 epochs under the loss, then compile(BPRLoss) on the same model and one more epoch: the model that replays captured graphs
    and the model that never captures one (AMAR_TRAIN_GRAPH=0) hold the same weights bit for bit after each phase, so the BPR
    epochs ran amar_bpr_grad_f32 and not the graph captured under the first loss."""
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    seq = tiny_triplets
    models, hist, graphs = [], [], []
    for env in ('0', '1'):
        monkeypatch.setenv('AMAR_TRAIN_GRAPH', env)
        m = _model(seq, cls, _losses()[name]())
        h1 = m.fit(seq, epochs=3, verbose=False)['loss']
        snapshot = [p.detach().clone() for p in m.parameters()]
        keys = [k for k in m._trainer._graphs if k[0] == 'sampled']
        first = m._trainer._graphs[keys[0]] if keys else None
        m.compile(loss=L.BPRLoss(), optimizer=m.optimizer)
        h2 = m.fit(seq, epochs=1, verbose=False)['loss']
        models.append((m, snapshot))
        hist.append(h1 + h2)
        graphs.append((first, keys))
    assert hist[0] == hist[1] and np.isfinite(hist[0]).all()
    for (ma, sa), (mb, sb) in [models]:
        for pa, pb in zip(sa, sb):
            assert torch.equal(pa, pb), tuple(pa.shape)
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(pa, pb), tuple(pa.shape)
        assert any(not torch.equal(s, p) for s, p in zip(sb, mb.parameters()))
    eager, graphed = models[0][0]._trainer, models[1][0]._trainer
    assert not eager._graphs and graphs[0][0] is None
    first, keys = graphs[1]
    assert len(keys) == 1 and first['compiled'][0] == L.resolve_loss(_losses()[name]())[0]
    now = graphed._graphs[keys[0]]                                    # the same key: BPR's graph took the place of the first
    assert now is not first and now['compiled'][0] == L.BPR
    assert eager.t == graphed.t == 4 * len(seq) and graphed._group_k == 4


@pytest.mark.parametrize('name', ['softmax', 'hardest', 'margin'])
@pytest.mark.parametrize('cls', ['BasicLightGCN', 'BasicGCN'])
def test_first_batch_loss_is_loss_value_on_the_restated_batch(hip, tiny_triplets, cls, name):
    """No regulariser, one eager step: the reported loss is `loss_value` on the batch `bpr_triplet_device_batch` restates and the
    model's own predictions for it, within what tests/test_bpr_gpu.py allows the BPR loss against its restatement (1e-5); and
    evaluate() on the Sequence reads the same groups."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities.losses import loss_value
    seq = tiny_triplets
    loss = _losses()[name]()
    model = _model(seq, cls, loss, l2=0.0)
    (u, i), _ = seq.device_batch(0)
    cases.check_batch(seq, seq.device_batch(0), 32, 4)
    pred = model((u, i)).cpu().numpy().reshape(-1).astype(np.float64)
    want = loss_value(loss, None, pred, n_negatives=seq.n_negatives)
    assert want > 0
    whole = model.evaluate(seq)[0]
    per_batch = [loss_value(loss, None, model(seq[b][0]).cpu().numpy().reshape(-1).astype(np.float64), n_negatives=4) for b in range(len(seq))]
    assert abs(whole - np.mean(per_batch)) < 1e-9
    trainer = training.Trainer(model)
    sampler = trainer.sampler_for(seq)
    trainer.train_sampled(sampler, graph=False)
    got = trainer.pop_loss_sum() / 64
    print(cls, name, 'first batch loss', got, 'restated', want)
    assert abs(got - want) < 1e-5
    assert int(sampler.step.item()) == 1


def test_refusals_on_the_device(hip, tiny_triplets):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    from deep_cbrs_amar_renaissance_amd.utilities.losses import SampledSoftmaxLoss
    from tests.test_bpr_gpu import _sample_sequence
    seq = tiny_triplets
    model = _model(seq, 'BasicGCN', SampledSoftmaxLoss(temperature=0.2))
    with pytest.raises(ValueError, match='load_user_item_graph_triplets'):
        model.fit(_sample_sequence(batch_size=64), epochs=1, verbose=False)
    with pytest.raises(ValueError, match='class_weight cannot weigh BPR training'):
        model.fit(seq, epochs=1, verbose=False, class_weight={0: 1.0, 1: 3.0})
    with pytest.raises(ValueError, match='load_user_item_graph_triplets'):
        training.Trainer(model).loss_and_grads(*seq.device_batch(0)[0], seq.device_batch(0)[1])   # (no sampler: no group size)
    engine.set_seed(11)
    hyb = hybrid.HybridBertGCN(seq.adj_matrix, embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[[24, 16], [32, 24], [16, 16]],
                               clf_units=[24, 16], l2_regularizer=1e-4, feature_based=True, fusion_method='concatenate', residual=False)
    hyb.set_bert_table(np.random.default_rng(3).standard_normal((seq.adj_matrix.shape[0], 40)).astype(np.float32))
    hyb.compile(loss=SampledSoftmaxLoss())
    with pytest.raises(NotImplementedError, match='hybrid models do not train on it'):
        hyb.fit(seq, epochs=1, verbose=False)
    hist = model.fit(seq, epochs=1, verbose=False)['loss']            # the refusals left the model usable
    assert np.isfinite(hist).all()


def test_experiment_with_a_loss_mapping(hip, tmp_path, monkeypatch):
    """parameters.loss: {name: SampledSoftmaxLoss, temperature: 0.2} with the triplet loader trains an experiment end to end."""
    import glob
    import json
    import yaml
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities import losses as L
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)                                            # (the data of tests/test_bpr_triplets_gpu.py's experiment)
    ds.train = ds.train[:40000]
    ds.train = ds.train[ds.train[:, 2] == 1]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['parameters'].update({'epochs': 2, 'loss': {'name': 'SampledSoftmaxLoss', 'temperature': 0.2}, 'full_ranking_ks': [10]})
    cfg['model'].update({'name': 'basic.BasicLightGCN', 'embedding_dim': 8, 'n_layers': 2, 'dense_units': [24, 24], 'clf_units': [48, 48]})
    cfg['dataset'].update({k: v for k, v in paths.items() if k != 'props_triples_filepath'})
    cfg['dataset'].update({'load_function_name': 'load_user_item_graph_triplets', 'n_negatives': 4})
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / "exps.yaml").write_text("linear:\n  softmax:\n    model:\n      name: basic.BasicLightGCN\n")
    seen = {}
    original = experiment.Experimenter.train

    def spy(self):
        seen['exp'] = self
        return original(self)
    monkeypatch.setattr(experiment.Experimenter, 'train', spy)
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('softmax', str(tmp_path / 'mlruns'))
    results = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log).run()
    assert len(results) == 1 and all(v is not None for v in results.values())
    exp = seen['exp']
    spec = exp.model._trainer._loss_spec()
    assert spec[0] == L.SAMPLED_SOFTMAX and spec[1][0] == 0.2 and exp.model._trainer._group_k == 4
    assert exp.model._trainer.t == 2 * len(exp.trainset)
    runs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    metrics = {}
    for line in open(runs[0]):
        rec = json.loads(line)
        if rec['event'] == 'metrics':
            metrics.update(rec['metrics'])
    assert np.isfinite(metrics['test_loss']) and 'full_recall_at_10' in metrics

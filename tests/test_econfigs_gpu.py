"""GPU: every architecture of the reference's experiment files scored, ranked and trained for one step (pytest -m gpu).

tests/econfigs_cases.py lists the architectures of tests/golden/econfigs_reference.json.  Each is built on one tiny graph (80 users, 60
items, 1 500 ratings; the architectures of the `*-uip-*` files also on the graph with 30 property nodes) and held against the
float64 oracle: `predict` on every rating, `recommend` against the float64 grid, and the loss and gradients of one training batch
against torch autograd.  The kernel-level files pin every kernel form at synthetic shapes; this one pins what the MODELS do with them at
the widths users run: the split plan, the tape, the concatenation slices, the choice between the fused chain and the pair route
(`test_route_of_each_architecture`, the table of DESIGN.md section 8b)."""
import functools

import numpy as np
import pytest
import torch
from scipy import sparse

from oracle import models as om
from oracle import train as otrain
from tests import econfigs_cases as ec
from tests import helpers
from tests.test_recommend_gpu import MAX_NEAR_TIE_USERS, _Train, _check_lists, _excl_sets, _grid_ids
from tests.test_training_gpu import _flatten_oracle_grads

pytestmark = pytest.mark.gpu

CASES = {cid: (name, cfg) for cid, name, cfg in ec.cases()}
UIP_IDS = ec.uip_case_ids()
# (case, graph): every case on the user-item graph; the graph classes of the `*-uip-*` files also with property nodes
PARAMS = [(cid, graph) for cid in sorted(CASES) for graph in (('ui', 'uip') if cid in UIP_IDS and ec.takes_graph(CASES[cid][1]) else ('ui',))]
IDS = ['{}-{}'.format(cid, graph) for cid, graph in PARAMS]

BERT_DIM = 768
SCORE_TOL = 2e-6            # the project's bound for model scores (sigmoid outputs), as in test_recommend_gpu._compare_routes


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """The one graph of this file and the tables that go with it: [n, 768] BERT rows and [n, 768] pre-computed graph rows."""
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=9, n_props=30 if kind == 'uip' else 0, n_links=90 if kind == 'uip' else 0)
    n = g['adj'].shape[0]
    rng = np.random.default_rng(17)
    g['bert'] = (rng.standard_normal((n, BERT_DIM)) * 0.5).astype(np.float32)
    g['rows'] = (rng.standard_normal((n, BERT_DIM)) * 0.5).astype(np.float32)
    return g


def _build(cid, g, seed=5):
    """The model of a case with every weight in place: biases drawn, DGCF gates moved away from their all-ones start."""
    from deep_cbrs_amar_renaissance_amd import engine, models as models_pkg
    name, cfg = CASES[cid]
    module_name, class_name = cfg['name'].split('.')
    cls = getattr(__import__(models_pkg.__name__ + '.' + module_name, fromlist=[class_name]), class_name)
    engine.set_seed(seed)
    if ec.takes_graph(cfg):
        model = cls(g['adj'], **cfg)
        if ec.is_hybrid(cfg):
            model.set_bert_table(g['bert'])
            model.rs.build_head(model.gnn.output_dim(), BERT_DIM)
    else:
        model = cls(**cfg)
        model.build_head(BERT_DIM, BERT_DIM)
    helpers.randomize_biases(model, seed=6)
    if 'DGCF' in name:
        with torch.no_grad():
            for layer in model.gnn.gnn_layers.seq_layers:
                layer.w.add_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, tuple(layer.w.shape)).astype(np.float32)).to(layer.w.device))
    return model


def _oracle_head(model, cfg):
    rs = model.rs if ec.takes_graph(cfg) else model
    return helpers.hybrid_head_to_oracle(rs) if ec.is_hybrid(cfg) else helpers.basic_head_to_oracle(rs)


def _oracle_scores(model, cfg, g, u, i, dtype=np.float64):
    """Scores of the pairs (u, i) by the numpy oracle in `dtype` (float64: the reference; float32: what sizes a rounding bound)."""
    head = _oracle_head(model, cfg)
    if not ec.takes_graph(cfg):
        rows, bert = g['rows'].astype(dtype), g['bert'].astype(dtype)
        if ec.is_hybrid(cfg):
            return om.hybrid_cbrs(rows[u], rows[i], bert[u], bert[i], head, feature_based=cfg['feature_based'])[:, 0]
        return om.basic_rs(rows[u], rows[i], head)[:, 0]
    gnn = helpers.gnn_to_oracle(model.gnn)
    if ec.is_hybrid(cfg):
        return om.hybrid_gnn_scores(g['adj'], gnn, head, u, i, g['bert'], dtype=dtype, feature_based=cfg['feature_based'])[:, 0]
    return om.basic_gnn_scores(g['adj'], gnn, head, u, i, dtype=dtype)[:, 0]


def _sequences(cfg, g, batch_size=512):
    """(the Sequence predict() reads, the training set recommend() reads) of a case, as the experiment driver builds them."""
    from deep_cbrs_amar_renaissance_amd.data import datasets
    r, users, items = g['ratings'], g['users'], g['items']
    if not ec.takes_graph(cfg):
        if ec.is_hybrid(cfg):
            seq = datasets.HybridUserItemEmbeddings(r, users, items, g['rows'], g['bert'], batch_size=batch_size)
        else:
            seq = datasets.UserItemEmbeddings(r, users, items, g['rows'], batch_size=batch_size)
        return seq, seq
    if ec.is_hybrid(cfg):
        return datasets.UserItemGraphEmbeddings(r, users, items, g['adj'], g['bert'], batch_size=batch_size), _Train(r, g['n_users'], g['n_items'])
    return datasets.UserItemGraph(r, users, items, g['adj'], batch_size=batch_size), _Train(r, g['n_users'], g['n_items'])


@pytest.mark.parametrize('cid,graph', PARAMS, ids=IDS)
def test_scores_match_the_float64_oracle(hip, cid, graph):
    """predict() on every rating of the graph and recommend(k=10) against the float64 oracle of the same weights."""
    name, cfg = CASES[cid]
    g = _graph(graph)
    model = _build(cid, g)
    nu, ni = g['n_users'], g['n_items']
    seq, train = _sequences(cfg, g)
    u, i = _grid_ids(nu, ni)
    grid = _oracle_scores(model, cfg, g, u, i).reshape(nu, ni)
    got = model.predict(seq)
    assert got.shape == (len(g['ratings']), 1) and got.dtype == np.float32
    want = grid[g['ratings'][:, 0], g['ratings'][:, 1] - nu]
    err = float(np.abs(got[:, 0] - want).max())
    print('econfigs score {}-{} max|predict - float64| = {:.3e}'.format(cid, graph, err))
    assert err <= SCORE_TOL, (cid, graph, err)
    ru, ri, rs = model.recommend(train, k=10)
    differing = _check_lists(ru, ri, rs, grid, _excl_sets(g['ratings'], nu), 10, nu, '{}-{}'.format(cid, graph), score_tol=SCORE_TOL)
    print('econfigs lists {}-{} users differing by near-ties = {}'.format(cid, graph, differing))
    assert differing <= MAX_NEAR_TIE_USERS


def _head_only_flat(model, want):
    """{parameter: oracle gradient} of a head trained on pre-computed rows (the loop of test_training_gpu.test_head_only_training)."""
    flat = {}
    for name, val in want['head'].items():
        if name.startswith('fuse'):
            for key, arr in val.items():
                flat[getattr(getattr(model, name), key)] = arr
        else:
            for layer, (gw, gb) in zip(getattr(model, name).layers, val):
                flat[layer.kernel], flat[layer.bias] = gw, gb
    return flat


def _oracle_grads(model, cfg, g, u, i, y, dtype=np.float64):
    """(loss, gradient containers) of the batch (u, i, y) by torch autograd of the restated forward in `dtype`."""
    head = _oracle_head(model, cfg)
    hybrid = ec.is_hybrid(cfg)
    bert = (g['bert'][u], g['bert'][i]) if hybrid else None
    if not ec.takes_graph(cfg):
        # BasicRS / HybridCBRS train on rows the Sequence delivers: the rows enter the oracle as a zero-layer 'GNN' (E = the table
        # itself), which is an input and carries no L2 term; the heads have no regulariser (l2_regularizer is not read by them)
        n = g['rows'].shape[0]
        adj, gnn, l2 = sparse.coo_matrix((n, n), dtype=np.float32), {'kind': 'lightgcn', 'embeddings': g['rows'], 'layers': []}, 0.0
    else:
        adj, gnn, l2 = g['adj'], helpers.gnn_to_oracle(model.gnn), cfg['l2_regularizer']
    want_loss, want, _ = otrain.torch_model_grads(adj, gnn, head, u, i, y, l2=l2, bert=bert, feature_based=cfg['feature_based'], dtype=dtype)
    return want_loss, want


def _relu_arguments(monkeypatch, model, cfg, g, y, dtype):
    """Every argument torch.relu sees in the oracle's forward of the whole pair list, in call order (float64 copies)."""
    seen, relu = [], torch.relu
    with monkeypatch.context() as m:
        m.setattr(torch, 'relu', lambda v: (seen.append(v.detach().double().numpy().copy()), relu(v))[1])
        _oracle_grads(model, cfg, g, g['u_ids'], g['i_ids'], y, dtype=dtype)
    return seen


def _decided_pairs(monkeypatch, model, cfg, g, y):
    """Which pairs of the list have a gradient float32 can be held to.  A ReLU has no derivative at 0: where the float64 forward puts an
    argument within float32 rounding of 0, a float32 forward may land on the other side and then differentiates ANOTHER function
    (seen on the device: arguments of -2.7e-7 and -1.7e-7 in float64 came out as +3.0e-8, and the gradient of a 768 x 256 kernel moved by
    2.4 % of its largest entry).  Rounding is sized from the oracle alone: a layer's arguments in float32 and in float64 differ by at most
    d; |argument| >= 4 d counts as decided (4 x: the device sums in another order than torch).  A pair with an undecided per-pair
    argument is left out of the batch.  Returns (mask of the pairs to keep, whether every per-node argument of the graph layers is
    decided: those no batch can leave out, the caller draws other weights)."""
    z64 = _relu_arguments(monkeypatch, model, cfg, g, y, np.float64)
    z32 = _relu_arguments(monkeypatch, model, cfg, g, y, np.float32)
    assert len(z64) == len(z32)
    pairs = len(g['u_ids'])
    keep, nodes_decided = np.ones(pairs, dtype=bool), True
    for a, b in zip(z64, z32):
        undecided = np.abs(a) < 4 * np.abs(a - b).max()
        if a.shape[0] == pairs:
            keep &= ~undecided.any(axis=1)
        else:
            assert a.shape[0] == g['adj'].shape[0]
            nodes_decided = nodes_decided and not undecided.any()
    return keep, nodes_decided


def _loss_and_grads(model, cfg, g, u, i, y):
    """(trainer, loss, gradients, oracle loss, {parameter: oracle gradient}) of the batch (u, i, y)."""
    from deep_cbrs_amar_renaissance_amd import training
    want_loss, want = _oracle_grads(model, cfg, g, u, i, y)
    if not ec.takes_graph(cfg):
        blocks = (g['rows'][u], g['rows'][i]) + ((g['bert'][u], g['bert'][i]) if ec.is_hybrid(cfg) else ())
        trainer = training.HeadTrainer(model)
        loss, grads = trainer.loss_and_grads(blocks, y)
        return trainer, loss, grads, want_loss, _head_only_flat(model, want)
    trainer = training.Trainer(model)
    loss, grads = trainer.loss_and_grads(u, i, y)                    # hybrid: the BERT rows of the resident table
    return trainer, loss, grads, want_loss, _flatten_oracle_grads(model, want)


@pytest.mark.parametrize('cid,graph', PARAMS, ids=IDS)
def test_gradients_match_the_autograd_oracle(hip, monkeypatch, cid, graph):
    """Loss and every gradient of one training batch (the graph's 300 pairs with random labels, less the few whose gradient float32
    cannot decide: `_decided_pairs`) against torch autograd of the restated forward in float64, with the case's own l2_regularizer."""
    name, cfg = CASES[cid]
    g = _graph(graph)
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    for seed in (5, 6, 7):                                           # (one case of 183 needs the second seed)
        model = _build(cid, g, seed)
        keep, nodes_decided = _decided_pairs(monkeypatch, model, cfg, g, y)
        if nodes_decided:
            break
    assert nodes_decided, "a graph layer's ReLU argument within rounding of 0 under every seed"
    # an argument is undecided with probability ~ 8 d / its spread (~1e-5 for the 768-term sums): a few pairs of 300 at the most
    assert keep.sum() >= 0.9 * len(keep), int(keep.sum())
    trainer, loss, grads, want_loss, flat = _loss_and_grads(model, cfg, g, g['u_ids'][keep], g['i_ids'][keep], y[keep])
    print('econfigs loss {}-{} pairs {} |loss - float64| = {:.3e}'.format(cid, graph, int(keep.sum()), abs(loss - want_loss)))
    assert abs(loss - want_loss) < 1e-5
    assert set(flat) == set(grads)
    names = {prm: nm for nm, prm in model.named_parameters()}
    worst = (0.0, None)
    for prm, gw in flat.items():
        got = grads[prm].cpu().numpy().reshape(gw.shape).astype(np.float64)
        got += 2 * trainer._l2(prm) * prm.detach().cpu().numpy().reshape(gw.shape)      # the trainer folds the L2 term into the optimizer launch
        diff, scale = float(np.abs(got - gw).max()), float(np.abs(gw).max())
        if scale > 1e-8 and diff / scale > worst[0]:       # (not the attention vectors whose gradient vanishes: the floor below)
            worst = (diff / scale, names[prm])
        if names[prm].endswith('bias'):
            # test_training_gpu.test_randomised_gradient_sweep: "a bias gradient is a sum of +-0.5/B terms that may cancel to 1e-4 of
            # their size [...] fp32 rounding of the un-cancelled terms" — its floor, for bias gradients only
            assert diff <= 3e-4 * scale + 3e-7, (names[prm], diff, scale)
        else:
            # (absolute floor: d/d(attn_kernel_self) vanishes where a row's softmax is shift-invariant in s_i)
            assert diff <= 2e-4 * scale + 1e-10, (names[prm], diff, scale)
    print('econfigs grads {}-{} max relative gradient error = {:.3e} ({})'.format(cid, graph, worst[0], worst[1]))


# ---- the route each architecture takes ---------------------------------------------------------------------------------------------------
def _tiles(shape):
    n = shape & 7
    return '-'.join(str((shape >> (3 * (j + 1))) & 7) for j in range(n + 1))


def _chain_name(route):
    if route['kernel'] == 1:
        return 'pair-stage maxt{} {}'.format(route['maxt'], 'split' if route['split'] else 'f32')
    if route['kernel'] == 2:
        return 'towers {}{}'.format(_tiles(route['shape']), ' lastlin' if route['lastlin'] else '')
    return 'generic maxt{}'.format(route['maxt'])


class _Recorder:
    """Wraps the launchers whose choice DESIGN.md documents: every call asks the launcher's own route query on its real operands
    (host only) and then runs.  `take()` returns what was seen since the last call, as sorted 'name xN' strings."""

    def __init__(self, capi, monkeypatch):
        self.seen = []

        def wrap(name, label):
            launch = getattr(capi, name)

            def recording(*args, **kwargs):
                self.seen.append(label(*args, **kwargs))
                return launch(*args, **kwargs)
            monkeypatch.setattr(capi, name, recording)

        stack = lambda spec: '-'.join(str(d) for d in [int(spec['weights'][0].shape[0])] + [int(w.shape[1]) for w in spec['weights']])
        wrap('chain', lambda *a, **kw: 'chain ' + _chain_name(capi.chain_route(*a, **kw)))
        wrap('dual_chain', lambda *a, **kw: 'dual_chain')
        wrap('dense', lambda X, W, *a, **kw: 'dense {}x{}'.format(*((W.shape[1], W.shape[0]) if kw.get('w_transposed') else W.shape)))
        wrap('dense_split', lambda x, image, k, n, *a, **kw: 'dense_split {}x{}'.format(k, n))
        wrap('recommend', lambda *a, **kw: 'recommend fused')
        wrap('topk_segmented', lambda *a, **kw: 'recommend pairs')
        wrap('dense_stack', lambda **spec: 'stack {} rows{}'.format(stack(spec), capi.dense_stack_route(**spec)['rows']))
        wrap('dense_stack_pair', lambda s0, s1: 'stack-pair {} | {} rows{}/{}'.format(stack(s0), stack(s1), capi.dense_stack_route(**s0)['rows'],
                                                                                    capi.dense_stack_route(**s1)['rows']))
        wrap('dense_stack_bwd', lambda **spec: 'stack-bwd {} rows{}'.format(stack(spec), capi.dense_stack_bwd_route(**spec)['rows']))
        wrap('dense_stack_bwd_pair', lambda s0, s1: 'stack-bwd-pair {} | {} rows{}/{}'.format(stack(s0), stack(s1), capi.dense_stack_bwd_route(**s0)['rows'],
                                                                                             capi.dense_stack_bwd_route(**s1)['rows']))
        wrap('dense_bwd', lambda *a, **kw: 'dense_bwd')
        wrap('wgrad', lambda X, dZ, dW=None, db=None: 'wgrad {}'.format(capi.wgrad_route(X, dZ, dW, db)['kernel']))
        wrap('scatter_add_rows', lambda src, ids, dst, base=0: 'scatter_add_rows {}'.format(capi.scatter_add_rows_route(src.shape[0], src.shape[1])['kernel']))

    def take(self):
        seen, self.seen = self.seen, []
        return sorted('{} x{}'.format(label, seen.count(label)) for label in set(seen))


# case -> what predict(), recommend() and one training batch launch of the calls that choose a route ('name xN': N calls), as the
# launchers' own route queries name them; DESIGN.md 8b holds the same table in words and says why each width lands where it does
ROUTES = {
    'BasicGCN-d16-L2-dense48x48-clf64x64': {
        'predict': ['chain pair-stage maxt4 split x1', 'chain towers 3-3-3-4 lastlin x2'],
        'recommend': ['chain towers 3-3-3-4 lastlin x2', 'recommend fused x1'],
        'train': ['dense_bwd x4', 'scatter_add_rows owner x2', 'stack 96-64-64-1 rows16 x1', 'stack-bwd 96-64-64-1 rows16 x1',
                   'stack-bwd-pair 48-48-48 | 48-48-48 rows16/16 x1', 'stack-pair 48-48-48 | 48-48-48 rows16/16 x1'],
    },
    'BasicGCN-d16-L3-dense64x64-clf64x64': {
        'predict': ['chain generic maxt4 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt4 x2', 'recommend fused x1'],
        'train': ['dense_bwd x6', 'scatter_add_rows owner x2', 'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 64-64-64 | 64-64-64 rows16/16 x1', 'stack-pair 64-64-64 | 64-64-64 rows16/16 x1'],
    },
    'BasicGCN-d32-L2-dense96x48-clf64x64': {
        'predict': ['chain generic maxt8 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt8 x2', 'recommend fused x1'],
        'train': ['dense_bwd x4', 'scatter_add_rows owner x2', 'stack 96-64-64-1 rows16 x1', 'stack-bwd 96-64-64-1 rows16 x1',
                   'stack-bwd-pair 96-96-48 | 96-96-48 rows16/16 x1', 'stack-pair 96-96-48 | 96-96-48 rows16/16 x1'],
    },
    'BasicGCN-d32-L3-dense128x64-clf64x64': {
        'predict': ['chain generic maxt8 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt8 x2', 'recommend fused x1'],
        'train': ['dense_bwd x6', 'scatter_add_rows owner x2', 'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 128-128-64 | 128-128-64 rows16/16 x1', 'stack-pair 128-128-64 | 128-128-64 rows16/16 x1'],
    },
    'BasicGCN-d8-L2-dense24x24-clf48x48': {
        'predict': ['chain pair-stage maxt3 split x1', 'chain towers 2-2-2-3 lastlin x2'],
        'recommend': ['chain towers 2-2-2-3 lastlin x2', 'recommend fused x1'],
        'train': ['dense_bwd x4', 'scatter_add_rows owner x2', 'stack 48-48-48-1 rows16 x1', 'stack-bwd 48-48-48-1 rows16 x1',
                   'stack-bwd-pair 24-24-24 | 24-24-24 rows16/16 x1', 'stack-pair 24-24-24 | 24-24-24 rows16/16 x1'],
    },
    'BasicGCN-d8-L3-dense32x32-clf64x64': {
        'predict': ['chain generic maxt4 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt4 x2', 'recommend fused x1'],
        'train': ['dense_bwd x6', 'scatter_add_rows owner x2', 'stack 64-64-64-1 rows16 x1', 'stack-bwd 64-64-64-1 rows16 x1',
                   'stack-bwd-pair 32-32-32 | 32-32-32 rows16/16 x1', 'stack-pair 32-32-32 | 32-32-32 rows16/16 x1'],
    },
    'BasicLightGCN-d16-L2-dense48x48-clf64x64': {
        'predict': ['chain pair-stage maxt4 split x1', 'chain towers 1-3-3-4 lastlin x2'],
        'recommend': ['chain towers 1-3-3-4 lastlin x2', 'recommend fused x1'],
        'train': ['scatter_add_rows owner x2', 'stack 96-64-64-1 rows16 x1', 'stack-bwd 96-64-64-1 rows16 x1',
                   'stack-bwd-pair 16-48-48 | 16-48-48 rows16/16 x1', 'stack-pair 16-48-48 | 16-48-48 rows16/16 x1'],
    },
    'BasicLightGCN-d16-L3-dense64x64-clf64x64': {
        'predict': ['chain generic maxt4 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt4 x2', 'recommend fused x1'],
        'train': ['scatter_add_rows owner x2', 'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 16-64-64 | 16-64-64 rows16/16 x1', 'stack-pair 16-64-64 | 16-64-64 rows16/16 x1'],
    },
    'BasicLightGCN-d32-L2-dense96x48-clf64x64': {
        'predict': ['chain generic maxt8 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt8 x2', 'recommend fused x1'],
        'train': ['scatter_add_rows owner x2', 'stack 96-64-64-1 rows16 x1', 'stack-bwd 96-64-64-1 rows16 x1',
                   'stack-bwd-pair 32-96-48 | 32-96-48 rows16/16 x1', 'stack-pair 32-96-48 | 32-96-48 rows16/16 x1'],
    },
    'BasicLightGCN-d32-L3-dense128x64-clf64x64': {
        'predict': ['chain generic maxt8 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt8 x2', 'recommend fused x1'],
        'train': ['scatter_add_rows owner x2', 'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 32-128-64 | 32-128-64 rows16/16 x1', 'stack-pair 32-128-64 | 32-128-64 rows16/16 x1'],
    },
    'BasicLightGCN-d8-L2-dense24x24-clf48x48': {
        'predict': ['chain pair-stage maxt3 split x1', 'chain towers 1-2-2-3 lastlin x2'],
        'recommend': ['chain towers 1-2-2-3 lastlin x2', 'recommend fused x1'],
        'train': ['scatter_add_rows owner x2', 'stack 48-48-48-1 rows16 x1', 'stack-bwd 48-48-48-1 rows16 x1',
                   'stack-bwd-pair 8-24-24 | 8-24-24 rows16/16 x1', 'stack-pair 8-24-24 | 8-24-24 rows16/16 x1'],
    },
    'BasicLightGCN-d8-L3-dense32x32-clf64x64': {
        'predict': ['chain generic maxt4 x2', 'chain pair-stage maxt4 split x1'],
        'recommend': ['chain generic maxt4 x2', 'recommend fused x1'],
        'train': ['scatter_add_rows owner x2', 'stack 64-64-64-1 rows16 x1', 'stack-bwd 64-64-64-1 rows16 x1',
                   'stack-bwd-pair 8-32-32 | 8-32-32 rows16/16 x1', 'stack-pair 8-32-32 | 8-32-32 rows16/16 x1'],
    },
    'BasicRS-dense512x256x128-clf64x64': {
        'predict': ['dense 256x64 x1', 'dense 64x1 x1', 'dense 64x64 x1', 'dense_split 256x128 x2', 'dense_split 512x256 x2',
                     'dense_split 768x512 x2'],
        'recommend': ['dense 128x64 x2', 'dense_split 256x128 x2', 'dense_split 512x256 x2', 'dense_split 768x512 x2',
                       'recommend fused x1'],
        'train': ['dense 128x256 x2', 'dense 256x128 x2', 'dense 256x512 x2', 'dense 256x64 x1', 'dense 512x256 x2', 'dense 64x1 x1',
                   'dense 64x256 x1', 'dense 64x64 x1', 'dense 768x512 x2', 'dense_bwd x2', 'wgrad mfma x7'],
    },
    'HybridBertGCN-d16-L2-dense48x48+256x64+64x64-clf64x64': {
        'predict': ['chain towers 3-3-3 x2', 'dense 256x64 x2', 'dense 48x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                     'dual_chain x1'],
        'recommend': ['chain towers 3-3-3 x2', 'dense 256x64 x2', 'dense 48x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                       'dual_chain x1', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 768x256 x2', 'dense_bwd x4', 'scatter_add_rows owner x2',
                   'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1', 'stack-bwd-pair 48-48-48 | 48-48-48 rows16/16 x1',
                   'stack-bwd-pair 96-64-64 | 128-64-64 rows16/16 x1', 'stack-pair 48-48-48 | 48-48-48 rows16/16 x1',
                   'stack-pair 96-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4'],
    },
    'HybridBertGCN-d16-L2-dense48x48+256x64+64x64-clf64x64-attention': {
        'predict': ['chain generic maxt4 x1', 'chain pair-stage maxt4 split x2', 'chain towers 3-3-3 x2', 'dense 256x64 x2',
                     'dense 48x64 x2', 'dense 64x64 x4', 'dense_split 768x256 x2'],
        'recommend': ['chain generic maxt4 x1', 'chain pair-stage maxt4 split x2', 'chain towers 3-3-3 x2', 'dense 256x64 x2',
                       'dense 48x64 x2', 'dense 64x64 x4', 'dense_split 768x256 x2', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 64x64 x4', 'dense 768x256 x2', 'dense_bwd x4',
                   'scatter_add_rows owner x2', 'stack 64-64-64-1 rows16 x1', 'stack-bwd 64-64-64-1 rows16 x1',
                   'stack-bwd-pair 48-48-48 | 48-48-48 rows16/16 x1', 'stack-bwd-pair 96-64-64 | 128-64-64 rows16/16 x1',
                   'stack-pair 48-48-48 | 48-48-48 rows16/16 x1', 'stack-pair 96-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4',
                   'wgrad partial x2'],
    },
    'HybridBertGCN-d16-L2-dense48x48+256x64+64x64-clf64x64-residual': {
        'predict': ['chain generic maxt8 x1', 'chain pair-stage maxt4 split x2', 'chain towers 3-3-3 x2', 'dense 256x64 x2',
                     'dense 48x64 x2', 'dense 64x1 x1', 'dense 64x64 x2', 'dense_split 768x256 x2'],
        'recommend': ['chain generic maxt8 x1', 'chain pair-stage maxt4 split x2', 'chain towers 3-3-3 x2', 'dense 256x64 x2',
                       'dense 48x64 x2', 'dense 64x1 x1', 'dense 64x64 x2', 'dense_split 768x256 x2', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 768x256 x2', 'dense_bwd x4', 'scatter_add_rows owner x2',
                   'stack 128-64-64 rows16 x1', 'stack 64-1 rows16 x1', 'stack-bwd 128-64-64 rows16 x1', 'stack-bwd 64-1 rows16 x1',
                   'stack-bwd-pair 48-48-48 | 48-48-48 rows16/16 x1', 'stack-bwd-pair 96-64-64 | 128-64-64 rows16/16 x1',
                   'stack-pair 48-48-48 | 48-48-48 rows16/16 x1', 'stack-pair 96-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4'],
    },
    'HybridBertGCN-d16-L3-dense64x64+256x64+64x64-clf64x64': {
        'predict': ['chain generic maxt4 x2', 'dense 256x64 x2', 'dense 64x64 x4', 'dense_split 768x256 x2', 'dual_chain x1'],
        'recommend': ['chain generic maxt4 x2', 'dense 256x64 x2', 'dense 64x64 x4', 'dense_split 768x256 x2', 'dual_chain x1',
                       'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 768x256 x2', 'dense_bwd x6', 'scatter_add_rows owner x2',
                   'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 128-64-64 | 128-64-64 rows16/16 x1', 'stack-bwd-pair 64-64-64 | 64-64-64 rows16/16 x1',
                   'stack-pair 128-64-64 | 128-64-64 rows16/16 x1', 'stack-pair 64-64-64 | 64-64-64 rows16/16 x1', 'wgrad mfma x4'],
    },
    'HybridBertGCN-d32-L2-dense96x96+256x64+64x64-clf64x64': {
        'predict': ['chain generic maxt8 x2', 'dense 256x64 x2', 'dense 64x64 x2', 'dense 96x64 x2', 'dense_split 768x256 x2',
                     'dual_chain x1'],
        'recommend': ['chain generic maxt8 x2', 'dense 256x64 x2', 'dense 64x64 x2', 'dense 96x64 x2', 'dense_split 768x256 x2',
                       'dual_chain x1', 'recommend pairs x1'],
        'train': ['dense 192x64 x1', 'dense 256x64 x2', 'dense 64x192 x1', 'dense 64x256 x2', 'dense 64x64 x1', 'dense 768x256 x2',
                   'dense_bwd x5', 'scatter_add_rows owner x2', 'stack 128-64-64 rows16 x1', 'stack 128-64-64-1 rows16 x1',
                   'stack-bwd 128-64-64 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 96-96-96 | 96-96-96 rows16/16 x1', 'stack-pair 96-96-96 | 96-96-96 rows16/16 x1', 'wgrad mfma x4',
                   'wgrad partial x1'],
    },
    'HybridBertGCN-d32-L2-dense96x96+256x64+64x64-clf64x64-attention': {
        'predict': ['chain generic maxt4 x1', 'chain generic maxt8 x2', 'chain pair-stage maxt4 split x2', 'dense 256x64 x2',
                     'dense 64x64 x4', 'dense 96x64 x2', 'dense_split 768x256 x2'],
        'recommend': ['chain generic maxt4 x1', 'chain generic maxt8 x2', 'chain pair-stage maxt4 split x2', 'dense 256x64 x2',
                       'dense 64x64 x4', 'dense 96x64 x2', 'dense_split 768x256 x2', 'recommend pairs x1'],
        'train': ['dense 192x64 x1', 'dense 256x64 x2', 'dense 64x192 x1', 'dense 64x256 x2', 'dense 64x64 x5', 'dense 768x256 x2',
                   'dense_bwd x5', 'scatter_add_rows owner x2', 'stack 128-64-64 rows16 x1', 'stack 64-64-64-1 rows16 x1',
                   'stack-bwd 128-64-64 rows16 x1', 'stack-bwd 64-64-64-1 rows16 x1',
                   'stack-bwd-pair 96-96-96 | 96-96-96 rows16/16 x1', 'stack-pair 96-96-96 | 96-96-96 rows16/16 x1', 'wgrad mfma x4',
                   'wgrad partial x3'],
    },
    'HybridBertGCN-d32-L2-dense96x96+256x64+64x64-clf64x64-residual': {
        'predict': ['chain generic maxt8 x3', 'chain pair-stage maxt4 split x2', 'dense 256x64 x2', 'dense 64x1 x1', 'dense 64x64 x2',
                     'dense 96x64 x2', 'dense_split 768x256 x2'],
        'recommend': ['chain generic maxt8 x3', 'chain pair-stage maxt4 split x2', 'dense 256x64 x2', 'dense 64x1 x1',
                       'dense 64x64 x2', 'dense 96x64 x2', 'dense_split 768x256 x2', 'recommend pairs x1'],
        'train': ['dense 192x64 x1', 'dense 256x64 x2', 'dense 64x192 x1', 'dense 64x256 x2', 'dense 64x64 x1', 'dense 768x256 x2',
                   'dense_bwd x5', 'scatter_add_rows owner x2', 'stack 128-64-64 rows16 x2', 'stack 64-1 rows16 x1',
                   'stack-bwd 128-64-64 rows16 x2', 'stack-bwd 64-1 rows16 x1', 'stack-bwd-pair 96-96-96 | 96-96-96 rows16/16 x1',
                   'stack-pair 96-96-96 | 96-96-96 rows16/16 x1', 'wgrad mfma x4', 'wgrad partial x1'],
    },
    'HybridBertGCN-d32-L3-dense128x128+256x64+64x64-clf64x64': {
        'predict': ['chain generic maxt8 x2', 'dense 128x64 x2', 'dense 256x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                     'dual_chain x1'],
        'recommend': ['chain generic maxt8 x2', 'dense 128x64 x2', 'dense 256x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                       'dual_chain x1', 'recommend pairs x1'],
        'train': ['dense 256x64 x3', 'dense 64x256 x3', 'dense 64x64 x1', 'dense 768x256 x2', 'dense_bwd x7',
                   'scatter_add_rows owner x2', 'stack 128-64-64 rows16 x1', 'stack 128-64-64-1 rows16 x1',
                   'stack-bwd 128-64-64 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1',
                   'stack-bwd-pair 128-128-128 | 128-128-128 rows16/16 x1', 'stack-pair 128-128-128 | 128-128-128 rows16/16 x1',
                   'wgrad mfma x5'],
    },
    'HybridBertGCN-d8-L2-dense24x24+256x64+64x64-clf64x64': {
        'predict': ['chain towers 2-2-2 x2', 'dense 24x64 x2', 'dense 256x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                     'dual_chain x1'],
        'recommend': ['chain towers 2-2-2 x2', 'dense 24x64 x2', 'dense 256x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                       'dual_chain x1', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 768x256 x2', 'dense_bwd x4', 'scatter_add_rows owner x2',
                   'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1', 'stack-bwd-pair 24-24-24 | 24-24-24 rows16/16 x1',
                   'stack-bwd-pair 48-64-64 | 128-64-64 rows16/16 x1', 'stack-pair 24-24-24 | 24-24-24 rows16/16 x1',
                   'stack-pair 48-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4'],
    },
    'HybridBertGCN-d8-L2-dense24x24+256x64+64x64-clf64x64-attention': {
        'predict': ['chain generic maxt4 x1', 'chain pair-stage maxt4 split x2', 'chain towers 2-2-2 x2', 'dense 24x64 x2',
                     'dense 256x64 x2', 'dense 64x64 x4', 'dense_split 768x256 x2'],
        'recommend': ['chain generic maxt4 x1', 'chain pair-stage maxt4 split x2', 'chain towers 2-2-2 x2', 'dense 24x64 x2',
                       'dense 256x64 x2', 'dense 64x64 x4', 'dense_split 768x256 x2', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 64x64 x4', 'dense 768x256 x2', 'dense_bwd x4',
                   'scatter_add_rows owner x2', 'stack 64-64-64-1 rows16 x1', 'stack-bwd 64-64-64-1 rows16 x1',
                   'stack-bwd-pair 24-24-24 | 24-24-24 rows16/16 x1', 'stack-bwd-pair 48-64-64 | 128-64-64 rows16/16 x1',
                   'stack-pair 24-24-24 | 24-24-24 rows16/16 x1', 'stack-pair 48-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4',
                   'wgrad partial x2'],
    },
    'HybridBertGCN-d8-L2-dense24x24+256x64+64x64-clf64x64-residual': {
        'predict': ['chain generic maxt8 x1', 'chain pair-stage maxt4 split x2', 'chain towers 2-2-2 x2', 'dense 24x64 x2',
                     'dense 256x64 x2', 'dense 64x1 x1', 'dense 64x64 x2', 'dense_split 768x256 x2'],
        'recommend': ['chain generic maxt8 x1', 'chain pair-stage maxt4 split x2', 'chain towers 2-2-2 x2', 'dense 24x64 x2',
                       'dense 256x64 x2', 'dense 64x1 x1', 'dense 64x64 x2', 'dense_split 768x256 x2', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 768x256 x2', 'dense_bwd x4', 'scatter_add_rows owner x2',
                   'stack 128-64-64 rows16 x1', 'stack 64-1 rows16 x1', 'stack-bwd 128-64-64 rows16 x1', 'stack-bwd 64-1 rows16 x1',
                   'stack-bwd-pair 24-24-24 | 24-24-24 rows16/16 x1', 'stack-bwd-pair 48-64-64 | 128-64-64 rows16/16 x1',
                   'stack-pair 24-24-24 | 24-24-24 rows16/16 x1', 'stack-pair 48-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4'],
    },
    'HybridBertGCN-d8-L3-dense32x32+256x64+64x64-clf64x64': {
        'predict': ['chain towers 2-2-2 x2', 'dense 256x64 x2', 'dense 32x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                     'dual_chain x1'],
        'recommend': ['chain towers 2-2-2 x2', 'dense 256x64 x2', 'dense 32x64 x2', 'dense 64x64 x2', 'dense_split 768x256 x2',
                       'dual_chain x1', 'recommend pairs x1'],
        'train': ['dense 256x64 x2', 'dense 64x256 x2', 'dense 768x256 x2', 'dense_bwd x6', 'scatter_add_rows owner x2',
                   'stack 128-64-64-1 rows16 x1', 'stack-bwd 128-64-64-1 rows16 x1', 'stack-bwd-pair 32-32-32 | 32-32-32 rows16/16 x1',
                   'stack-bwd-pair 64-64-64 | 128-64-64 rows16/16 x1', 'stack-pair 32-32-32 | 32-32-32 rows16/16 x1',
                   'stack-pair 64-64-64 | 128-64-64 rows16/16 x1', 'wgrad mfma x4'],
    },
    'HybridCBRS-dense256x64+256x64+64x32-clf64x32': {
        'predict': ['chain generic maxt4 x1', 'chain generic maxt8 x2', 'dense 256x64 x4', 'dense_split 768x256 x4'],
        'recommend': ['chain generic maxt4 x3', 'dense 256x64 x4', 'dense 64x64 x4', 'dense_split 768x256 x4', 'recommend pairs x1'],
        'train': ['dense 256x64 x4', 'dense 64x256 x4', 'dense 768x256 x4', 'stack 64-64-32-1 rows16 x1',
                   'stack-bwd 64-64-32-1 rows16 x1', 'stack-bwd-pair 128-64-32 | 128-64-32 rows16/16 x1',
                   'stack-pair 128-64-32 | 128-64-32 rows16/16 x1', 'wgrad mfma x8'],
    },
    'HybridCBRS-dense256x64+256x64+64x32-clf64x32-entity': {
        'predict': ['chain generic maxt4 x1', 'chain generic maxt8 x2', 'dense 256x64 x4', 'dense_split 768x256 x4'],
        'recommend': ['chain generic maxt4 x3', 'dense 256x64 x4', 'dense 64x64 x4', 'dense_split 768x256 x4', 'recommend pairs x1'],
        'train': ['dense 256x64 x4', 'dense 64x256 x4', 'dense 768x256 x4', 'stack 64-64-32-1 rows16 x1',
                   'stack-bwd 64-64-32-1 rows16 x1', 'stack-bwd-pair 128-64-32 | 128-64-32 rows16/16 x1',
                   'stack-pair 128-64-32 | 128-64-32 rows16/16 x1', 'wgrad mfma x8'],
    },
}

ROUTE_CASES = [(cid, name, cfg) for cid, name, cfg in ec.route_representatives()]


@pytest.mark.parametrize('cid', [c[0] for c in ROUTE_CASES])
def test_route_of_each_architecture(hip, monkeypatch, cid):
    """One case per (width, dense_units, clf_units): the launches of predict(), recommend() and one training batch, each asked for its
    route on its real operands, against the table above — the fused chain / the one-launch stacks where DESIGN.md says these widths take
    them, the layer-by-layer kernels and the pair ranking only where it says so."""
    name, cfg = CASES[cid]
    g = _graph('ui')
    model = _build(cid, g)
    seq, train = _sequences(cfg, g, batch_size=2048)                # one batch: every launch of the pass once
    rec = _Recorder(hip, monkeypatch)
    if ec.takes_graph(cfg) and not ec.is_hybrid(cfg):
        model.predict(seq, graph=False)                             # (eager: a captured pass would run the launchers twice)
    else:
        model.predict(seq)
    predict = rec.take()
    route = model._recommend_route(train)
    model.recommend(train, k=10)
    recommend = rec.take()
    assert ('recommend fused x1' in recommend) == (route == 'fused') and ('recommend pairs x1' in recommend) == (route == 'pairs'), recommend
    y = np.random.default_rng(2).integers(0, 2, len(g['u_ids']))
    _loss_and_grads(model, cfg, g, g['u_ids'], g['i_ids'], y)
    train_step = rec.take()
    got = {'predict': predict, 'recommend': recommend, 'train': train_step}
    print('econfigs route {!r}: {!r},'.format(cid, got))
    assert got == ROUTES[cid]

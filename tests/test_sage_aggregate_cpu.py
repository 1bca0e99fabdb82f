"""GraphSAGE sum / max / min aggregators, host side: the test oracle (tests/sage_agg_ref.py) pinned against oracle/, the tie rule
on a hand-computed example, constructors, the C-ABI's declarations and the experiment grid."""
import os
import re

import numpy as np
import pytest

from oracle import layers as ol
from oracle import train as otrain
from tests import helpers, sage_agg_ref as ref

CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_weights(n, widths, rng):
    layers = [{'kernel': rng.uniform(-0.6, 0.6, (2 * f, c)), 'bias': rng.uniform(-0.1, 0.1, c)} for f, c in zip(widths[:-1], widths[1:])]
    return {'kind': 'sage', 'final_node': 'concatenation', 'embeddings': rng.standard_normal((n, widths[0])) * 0.5, 'layers': layers}


def _random_head(d, rng):
    net = lambda dims: [(rng.uniform(-0.4, 0.4, (a, b)), rng.uniform(-0.05, 0.05, b)) for a, b in zip(dims[:-1], dims[1:])]   # noqa: E731
    return {'unet': net([d, 12]), 'inet': net([d, 12]), 'clf': net([24, 10, 1])}


def _messy_graph(n=40, seed=0):
    """Duplicate edges, an isolated node (the last one), no diagonal; returned as the (row, col) edge list and a CSR."""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n - 1, 160), rng.integers(0, n - 1, 160)
    keep = r != c
    r, c = r[keep], c[keep]
    r, c = np.concatenate([r, r[:25]]), np.concatenate([c, c[:25]])
    return r, c


@pytest.mark.parametrize('self_loops', [True, False])
def test_numpy_layer_reproduces_the_oracle_for_mean(self_loops):
    rng = np.random.default_rng(1)
    r, c = _messy_graph()
    x, w, b = rng.standard_normal((40, 8)), rng.uniform(-0.6, 0.6, (16, 5)), rng.uniform(-0.1, 0.1, 5)
    want = ol.sage_conv(x, r, c, w, b, self_loops=self_loops)
    assert np.abs(ref.sage_conv_np(x, r, c, w, b, 'mean', self_loops) - want).max() < 1e-15


@pytest.mark.parametrize('graph', ['ui', 'uip'])
def test_torch_model_reproduces_the_oracle_for_mean(graph):
    """(b) with aggregate='mean' against oracle.train.torch_model_grads: both float64 on one CPU."""
    rng = np.random.default_rng(3)
    g = helpers.tiny_graph(n_users=30, n_items=25, n_ratings=300, seed=2, n_props=12 if graph == 'uip' else 0, n_links=40 if graph == 'uip' else 0)
    n = g['adj'].shape[0]
    gnn, head = _random_weights(n, [8, 8, 8], rng), _random_head(24, rng)
    y = rng.integers(0, 2, len(g['u_ids']))
    want_loss, want, want_p = otrain.torch_model_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, l2=1e-4)
    loss, got, p = ref.torch_model_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, 'mean', l2=1e-4)
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    assert np.abs(p - want_p).max() < 1e-14
    pairs = [(got['gnn']['embeddings'], want['gnn']['embeddings'])]
    pairs += [(a[k], b[k]) for a, b in zip(got['gnn']['layers'], want['gnn']['layers']) for k in a]
    pairs += [(x, z) for name in want['head'] for ga, gb in zip(got['head'][name], want['head'][name]) for x, z in zip(ga, gb)]
    for a, b in pairs:
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max()


@pytest.mark.parametrize('aggregate', ['sum', 'max', 'min'])
@pytest.mark.parametrize('self_loops', [True, False])
def test_numpy_forward_equals_torch_forward(aggregate, self_loops):
    """(a) against (b)'s forward on a graph with duplicate edges and an isolated node; many exact zeros in the input (ties)."""
    import torch
    rng = np.random.default_rng(5)
    r, c = _messy_graph()
    n = 40
    x = np.maximum(rng.standard_normal((n, 8)), 0)                     # a ReLU output: whole neighbourhoods tie at 0
    src, tgt = ref.with_self_loops(r, c, n, self_loops)
    agg, cnt = ref.aggregate_np(x, src, tgt, n, aggregate)
    xt = torch.tensor(x, requires_grad=True)
    agg_t = ref.torch_aggregate(xt, torch.as_tensor(src), torch.as_tensor(tgt), n, aggregate)
    assert np.array_equal(agg, agg_t.detach().numpy()) if aggregate != 'sum' else np.abs(agg - agg_t.detach().numpy()).max() < 1e-13
    assert np.all(agg[n - 1] == (x[n - 1] if self_loops else 0))       # the isolated node: itself, or the stated 0
    if aggregate != 'sum':
        # the reverse rule written out with the counts of (a) equals autograd of (b)
        d = rng.standard_normal((n, 8))
        (agg_t * torch.tensor(d)).sum().backward()
        want = np.zeros_like(x)
        share = np.where(cnt > 0, d / np.maximum(cnt, 1), 0)
        np.add.at(want, src, (x[src] == agg[tgt]) * share[tgt])
        assert np.abs(want - xt.grad.numpy()).max() < 1e-13
        deg = np.bincount(tgt, minlength=n)
        assert (cnt[deg > 0] >= 1).all() and (cnt[deg == 0] == 0).all() and np.array_equal(cnt, np.round(cnt))


def test_tie_rule_on_a_hand_computed_example():
    """4 nodes, 3 features, no self loops, target 0 receives from 1, 2, 3 and from 3 once more (a duplicated edge):
       feature 0: values 5, 5, 1 (, 1)   -> two-way tie between nodes 1 and 2: 1/2 each
       feature 1: values 0, 0, 0 (, 0)   -> every entry ties at 0; four entries: 1/4 each, node 3 holds two of them
       feature 2: values 2, 7, 7 (, 7)   -> three entries tie at 7 (node 2 once, node 3 twice): node 2 gets 1/3, node 3 2/3
    and, without the duplicate, feature 1 is the three-way tie at 0 with 1/3 each."""
    import torch
    x = np.array([[9., 9., 9.], [5., 0., 2.], [5., 0., 7.], [1., 0., 7.]])
    for dup in (False, True):
        src = np.array([1, 2, 3] + ([3] if dup else []))
        tgt = np.zeros(len(src), dtype=np.int64)
        xt = torch.tensor(x, requires_grad=True)
        agg = ref.torch_aggregate(xt, torch.as_tensor(src), torch.as_tensor(tgt), 4, 'max')
        assert agg[0].tolist() == [5., 0., 7.] and agg[1:].abs().sum() == 0
        agg[0].sum().backward()
        want = np.zeros((4, 3))
        if dup:
            want[1], want[2], want[3] = [1 / 2, 1 / 4, 0], [1 / 2, 1 / 4, 1 / 3], [0, 2 / 4, 2 / 3]
        else:
            want[1], want[2], want[3] = [1 / 2, 1 / 3, 0], [1 / 2, 1 / 3, 1 / 2], [0, 1 / 3, 1 / 2]
        assert np.allclose(xt.grad.numpy(), want, atol=1e-15)
        a_np, cnt = ref.aggregate_np(x, src, tgt, 4, 'max')
        assert np.array_equal(a_np[0], [5., 0., 7.]) and cnt[0].tolist() == ([2., 4., 3.] if dup else [2., 3., 2.])


def test_constructors_accept_the_four_names_and_refuse_the_rest():
    """Fails before the feature: every non-mean name raised NotImplementedError."""
    from deep_cbrs_amar_renaissance_amd.layers.graphsage_conv import GraphSageConv
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid, gnn, tsgnn, twgnn
    for name in ref.AGGREGATES:
        assert GraphSageConv(8, aggregate=name, activation='relu').aggregate == name
    for bad in ('prod', 'median'):
        with pytest.raises(NotImplementedError) as err:
            GraphSageConv(8, aggregate=bad, activation='relu')
        assert all(repr(name) in str(err.value) for name in ref.AGGREGATES)
    g, kg = helpers.tiny_graph(), helpers.kg_graph()
    two, three = (kg['adj_ui'], kg['adj_ip']), (kg['adj_ui'], kg['adj_ip'], kg['adj_up'])
    hcfg = dict(CFG, dense_units=[[24, 24], [16, 8], [16, 16]], clf_units=[16, 16])
    for name in ref.AGGREGATES + ('prod',):
        build = [lambda: basic.BasicGraphSage(g['adj'], aggregate=name, **CFG).gnn.gnn_layers,
                 lambda: basic.BasicTSGraphSage(kg['n_users'], kg['n_items'], two, aggregate=name, **CFG).gnn.step_two_gnn_layers,
                 lambda: basic.BasicTWGraphSage(kg['n_users'], kg['n_items'], three, aggregate=name, **CFG).gnn.step_two_gnn_layers,
                 lambda: hybrid.HybridBertGraphSage(g['adj'], aggregate=name, **hcfg).gnn.gnn_layers,
                 lambda: hybrid.HybridBertTSGraphSage(kg['n_users'], kg['n_items'], two, aggregate=name, **hcfg).gnn.step_two_gnn_layers,
                 lambda: hybrid.HybridBertTWGraphSage(kg['n_users'], kg['n_items'], three, aggregate=name, **hcfg).gnn.step_two_gnn_layers,
                 lambda: gnn.GraphSage(g['adj'], aggregate=name, **{k: CFG[k] for k in ('embedding_dim', 'n_hiddens', 'l2_regularizer')}).gnn_layers,
                 lambda: tsgnn.TwoStepGraphSage(kg['n_users'], kg['n_items'], two, aggregate=name,
                                                **{k: CFG[k] for k in ('embedding_dim', 'n_hiddens', 'l2_regularizer')}).step_two_gnn_layers,
                 lambda: twgnn.TwoWayGraphSage(kg['n_users'], kg['n_items'], three, aggregate=name,
                                               **{k: CFG[k] for k in ('embedding_dim', 'n_hiddens', 'l2_regularizer')}).step_two_gnn_layers]
        for make in build:
            if name == 'prod':
                with pytest.raises(NotImplementedError):
                    make()
            else:
                assert all(l.aggregate == name for l in make().seq_layers)


def test_entry_points_are_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_sage_layer_agg_f32', 'amar_sage_aggregate_f32', 'amar_sage_aggregate_bwd_f32'):
        assert sym in capi.SIGNATURES and re.search(r'\bint\s+' + sym + r'\s*\(', header)
    for name, code in (('SUM', 0), ('MAX', 1), ('MIN', 2)):
        assert re.search(r'#define\s+AMAR_AGG_{}\s+{}\b'.format(name, code), header) and getattr(capi, 'AGG_' + name) == code


def test_experiment_grid_over_the_aggregators_expands(tmp_path):
    import yaml
    from deep_cbrs_amar_renaissance_amd import experiment
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump({'model': {'name': 'basic.BasicGraphSage', 'aggregate': 'mean'}}))
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump({'grid': {'agg': {'model': {'name': ['basic.BasicGraphSage'],
                                                                                  'aggregate': list(ref.AGGREGATES)}}}}))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), None)
    assert len(multi.experiments) == 4
    assert sorted(e['model']['aggregate'] for e in multi.experiments.values()) == sorted(ref.AGGREGATES)

"""Multi-head GAT, host side: the test oracle (tests/gat_heads_ref.py) pinned against oracle/, the layer's weights and widths, and
everything that is refused.  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import layers as ol
from tests import helpers, gat_heads_ref as ref

CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _messy_graph(n=40, seed=0):
    """Duplicate edges, an isolated node (the last one), no diagonal."""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n - 1, 160), rng.integers(0, n - 1, 160)
    keep = r != c
    r, c = r[keep], c[keep]
    return np.concatenate([r, r[:25]]), np.concatenate([c, c[:25]])


def _layer_weights(rng, f, heads, c, concat):
    return (rng.uniform(-0.6, 0.6, (f, heads, c)), rng.uniform(-1, 1, (c, heads, 1)), rng.uniform(-1, 1, (c, heads, 1)),
            rng.uniform(-0.1, 0.1, heads * c if concat else c))


@pytest.mark.parametrize('heads,c', [(1, 8), (2, 4), (3, 8), (4, 16)])
@pytest.mark.parametrize('concat', [True, False])
@pytest.mark.parametrize('self_loops', [True, False])
def test_the_two_restatements_agree(heads, c, concat, self_loops):
    import torch
    rng = np.random.default_rng(heads * 10 + c)
    r, col = _messy_graph()
    n, f = 40, 6
    x = rng.standard_normal((n, f))
    w, a_s, a_n, b = _layer_weights(rng, f, heads, c, concat)
    want = ref.gat_heads_conv_np(x, r, col, w, a_s, a_n, b, concat, self_loops)
    src, tgt = ref.edges(r, col, n, self_loops)
    hd = (torch.tensor(x) @ torch.tensor(w).reshape(f, heads * c)).reshape(n, heads, c)
    got = ref.torch_gat_heads(hd, torch.tensor(a_s), torch.tensor(a_n), torch.tensor(b), src, tgt, concat).numpy()
    assert got.shape == want.shape == (n, heads * c if concat else c)
    assert np.abs(got - want).max() < 1e-13
    if heads == 1:                                                   # one head: the oracle's layer itself, under either joining
        oracle, _ = ol.gat_conv(x, r, col, w[:, 0, :], a_s[:, 0, 0], a_n[:, 0, 0], b, self_loops=self_loops)
        assert np.abs(want - oracle).max() < 1e-15 and np.abs(got - oracle).max() < 1e-13
    if not self_loops:                                               # the isolated node: nothing to attend to, ReLU(bias)
        assert np.array_equal(want[n - 1], np.maximum(b, 0))


def test_layer_builds_keras_shaped_weights():
    """Fails before the feature: attn_heads=2 raised NotImplementedError."""
    from deep_cbrs_amar_renaissance_amd.layers.gat_conv import GATConv
    f = 12
    for concat, bias_shape, width in ((True, (16,), 16), (False, (8,), 8)):
        layer = GATConv(8, attn_heads=2, concat_heads=concat, activation='relu')
        layer.build([(30, f), None])
        assert tuple(layer.kernel.shape) == (f, 2, 8)
        assert tuple(layer.attn_kernel_self.shape) == (8, 2, 1) and tuple(layer.attn_kernel_neighs.shape) == (8, 2, 1)
        assert tuple(layer.bias.shape) == bias_shape and layer.output_width == width
    one = GATConv(8, activation='relu')
    one.build([(30, f), None])
    assert tuple(one.kernel.shape) == (f, 1, 8) and tuple(one.attn_kernel_self.shape) == (8, 1, 1) and tuple(one.bias.shape) == (8,)
    assert one.attn_heads == 1 and one.output_width == 8


def test_unsupported_shapes_and_returned_coefficients_are_refused():
    from deep_cbrs_amar_renaissance_amd.layers.gat_conv import GATConv
    for heads, c in ((9, 8), (2, 6)):                                # H*C = 72 > 64; C = 6 is no multiple of 4
        with pytest.raises(NotImplementedError, match='64') as err:
            GATConv(c, attn_heads=heads, activation='relu')
        assert 'channels % 4' in str(err.value)
    with pytest.raises(NotImplementedError, match='return_attn_coef'):
        GATConv(8, attn_heads=2, return_attn_coef=True, activation='relu')
    with pytest.raises(NotImplementedError, match='return_attn_coef'):
        GATConv(8, return_attn_coef=True, activation='relu')
    assert GATConv(8, attn_heads=8, activation='relu').output_width == 64            # the limit itself is inside
    wide = GATConv(8, attn_heads=2, activation='relu')                                 # an input wider than the projection kernel's table
    with pytest.raises(NotImplementedError, match='64'):
        wide.build([(30, 72), None])
    GATConv(8, attn_heads=2, activation='relu').build([(30, 64), None])


def test_stack_widths_follow_the_heads():
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    g, kg = helpers.tiny_graph(), helpers.kg_graph()
    model = basic.BasicGAT(g['adj'], attn_heads=2, **CFG)
    assert model.gnn.gnn_layers.layer_widths() == [8, 16, 16] and model.gnn.output_dim() == 40
    assert all(l.attn_heads == 2 and l.concat_heads for l in model.gnn.gnn_layers.seq_layers)
    mean = basic.BasicGAT(g['adj'], attn_heads=4, concat_heads=False, **CFG)
    assert mean.gnn.gnn_layers.layer_widths() == [8, 8, 8] and mean.gnn.output_dim() == 24
    default = basic.BasicGAT(g['adj'], **CFG)
    assert default.gnn.gnn_layers.layer_widths() == [8, 8, 8] and all(l.attn_heads == 1 for l in default.gnn.gnn_layers.seq_layers)
    # TwoStep under the 'concatenation' hand-over: the user table takes the width step one really hands over
    two = basic.BasicTSGAT(kg['n_users'], kg['n_items'], (kg['adj_ui'], kg['adj_ip']), attn_heads=2, **dict(CFG, item_node='concatenation'))
    assert two.gnn.step_one_gnn_layers.layer_widths() == [8, 16, 16]
    assert two.gnn.step_two_gnn_layers.layer_widths() == [40, 48, 48]
    three = basic.BasicTWGAT(kg['n_users'], kg['n_items'], (kg['adj_ui'], kg['adj_ip'], kg['adj_up']), attn_heads=2, concat_heads=False, **CFG)
    assert all(l.attn_heads == 2 and not l.concat_heads for l in three.gnn.step_two_gnn_layers.seq_layers)
    hyb = hybrid.HybridBertGAT(g['adj'], attn_heads=2, **dict(CFG, dense_units=[[24, 24], [16, 8], [16, 16]], clf_units=[16, 16]))
    assert hyb.gnn.gnn_layers.layer_widths() == [8, 16, 16]


def test_partitioned_runner_refuses_several_heads():
    from deep_cbrs_amar_renaissance_amd import parallel
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = helpers.tiny_graph()
    for extra in (dict(attn_heads=2), dict(attn_heads=4, concat_heads=False), dict(attn_heads=2, n_hiddens=[4, 4])):
        model = basic.BasicGAT(g['adj'], **dict(CFG, **extra))       # (2 heads of 4 are 8 wide: the width check alone would let them through)
        with pytest.raises(NotImplementedError, match='attn_heads'):
            parallel.PartitionedGCNRunner(model, g['u_ids'], g['i_ids'], 0, 2)


def test_entry_points_are_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_rowwise_xw_heads_f32', 'amar_gat_heads_f32', 'amar_gat_heads_bwd_f32'):
        assert sym in capi.SIGNATURES and re.search(r'\bint\s+' + sym + r'\s*\(', header)
    assert capi.gat_heads_supported(8, 8) and capi.gat_heads_supported(16, 4) and capi.gat_heads_supported(2, 32)
    assert not capi.gat_heads_supported(9, 8) and not capi.gat_heads_supported(2, 6) and not capi.gat_heads_supported(2, 2)

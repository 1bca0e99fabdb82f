"""Directed graphs, host side: the numpy restatement of the stable CSR transpose against scipy, and the surface the feature adds."""
import os
import re

import numpy as np
import pytest
from scipy import sparse

from tests import directed_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    rng = np.random.default_rng(0)
    rect = sparse.coo_matrix((np.ones(60, np.float32), (rng.integers(0, 7, 60), rng.integers(0, 23, 60))), shape=(7, 23))
    return {'ui': dr.tiny('ui')['adj'], 'uip': dr.tiny('uip')['adj'], 'mixed': dr.mixed()['adj'],
            'empty': sparse.coo_matrix((5, 4), dtype=np.float32), 'rect': rect}


@pytest.mark.parametrize('name', ['ui', 'uip', 'mixed', 'empty', 'rect'])
def test_restatement_equals_scipy_tocsc(name):
    m = _cases()[name]
    rowptr, colidx, _ = dr.csr_of(m)
    n_cols = m.shape[1]
    t_rowptr, t_colidx, perm = dr.stable_transpose(rowptr, colidx, n_cols)
    # scipy: data tagged with the input position, so the converted data IS perm (tocsc does not sum duplicates)
    tagged = sparse.csr_matrix((np.arange(len(colidx), dtype=np.float64), colidx, rowptr), shape=m.shape)
    csc = tagged.tocsc()
    assert np.array_equal(t_rowptr, csc.indptr) and np.array_equal(t_colidx, csc.indices)
    assert np.array_equal(perm, csc.data.astype(np.int64))
    fast = dr.stable_transpose_fast(rowptr, colidx, n_cols)
    assert all(np.array_equal(a, b) for a, b in zip((t_rowptr, t_colidx, perm), fast))
    assert t_rowptr.dtype == t_colidx.dtype == perm.dtype == np.int32
    for j in range(n_cols):                                          # strictly increasing inside every output row
        seg = perm[t_rowptr[j]:t_rowptr[j + 1]]
        assert np.all(np.diff(seg) > 0)
    assert sorted(perm.tolist()) == list(range(len(colidx)))
    # sorted input columns give sorted output columns, and an entry keeps its ordinal among its duplicates
    for j in range(n_cols):
        assert np.all(np.diff(t_colidx[t_rowptr[j]:t_rowptr[j + 1]]) >= 0)
    assert np.array_equal(dr.ordinals(t_rowptr, t_colidx), dr.ordinals(rowptr, colidx)[perm])
    # transposing twice gives the input back
    back = dr.stable_transpose(t_rowptr, t_colidx, m.shape[0])
    assert np.array_equal(back[0], rowptr) and np.array_equal(back[1], colidx) and np.array_equal(perm[back[2]], np.arange(len(colidx)))


def test_graph_builders_hold_what_they_promise():
    ui = sparse.csr_matrix(dr.tiny('ui')['adj'])
    assert ui[80:].nnz == 0 and ui[:, :80].nnz == 0 and ui.nnz > 0
    rowptr, colidx, _ = dr.csr_of(dr.tiny('uip')['adj'])
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    assert ((rows[1:] == rows[:-1]) & (colidx[1:] == colidx[:-1])).any(), "the uip graph holds parallel item-property entries"
    assert dr.ordinals(*dr.csr_of(dr.mixed()['adj'])[:2]).max() >= 1


def test_new_entry_points_are_declared_and_bound():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    declared = set(re.findall(r'\b(amar_[a-z0-9_]+)\s*\(', header))
    for name in ('amar_csr_transpose_i32', 'amar_gat_bwd_directed_f32', 'amar_gat_bwd_directed_dropout_f32'):
        assert name in capi.SIGNATURES, name
        assert name in declared, name
    assert callable(capi.csr_transpose)


def test_device_csr_has_the_transposed_image_and_the_symmetry_check():
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    assert callable(DeviceCSR.transposed) and callable(DeviceCSR.is_symmetric)
    sym = DeviceCSR.from_scipy(dr.tiny('ui')['adj_sym'], device='cpu')
    assert sym.is_symmetric() and sym.transposed() is sym            # no kernel: works without a GPU
    assert not DeviceCSR.from_scipy(dr.tiny('ui')['adj'], device='cpu').is_symmetric()
    assert not DeviceCSR.from_scipy(sparse.coo_matrix((np.ones(2, np.float32), ([0, 1], [1, 2])), shape=(2, 3)), device='cpu').is_symmetric()


def test_training_no_longer_refuses_directed_graphs():
    from deep_cbrs_amar_renaissance_amd import training
    assert not hasattr(training, '_require_symmetric')
    src = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'training.py')).read()
    assert 'needs a symmetric adjacency' not in src


def test_edge_list_stacks_walk_the_transposed_list_on_a_directed_graph(monkeypatch):
    """Spektral reads an entry (r, c) as source r -> target c; the row kernels aggregate a row over its columns: on a directed graph the
    GraphSAGE / GAT stacks keep the transposed list (so that row i lists the sources of target i), a symmetric list as it comes."""
    from deep_cbrs_amar_renaissance_amd.models import gnn as gnn_mod
    from deep_cbrs_amar_renaissance_amd.layers.graphsage_conv import GraphSageConv
    from deep_cbrs_amar_renaissance_amd.layers.gcn_conv import GCNConv
    seen = []
    monkeypatch.setattr(gnn_mod, 'convert_to_tensor', lambda m, **kw: seen.append(m) or m)
    monkeypatch.setattr(gnn_mod.capi, 'check_dropout_rate', lambda *a, **k: 0.0)
    g = dr.mixed()

    import torch

    class Stub(gnn_mod.SequentialGNN):
        def __init__(self):
            torch.nn.Module.__init__(self)
    for layer_cls, adj, flipped in ((GraphSageConv, g['adj'], True), (GCNConv, g['adj'], False),
                                    (GraphSageConv, dr.tiny('ui')['adj_sym'], False)):
        seen.clear()
        stack = Stub()
        stack._init_stack(adj, [layer_cls(8, activation='relu')], 'concatenation', None, False)
        want = adj.T if flipped else adj
        assert (sparse.csr_matrix(seen[0]) != sparse.csr_matrix(want)).nnz == 0

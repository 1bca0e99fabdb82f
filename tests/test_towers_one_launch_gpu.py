"""Both entity towers in one launch (amar_chain_rows2_f32 / capi.chain2) and the 16-byte-piece X.W prologue, on the GPU.

chain2 promises the bits of two `chain` calls: every comparison here is torch.equal on the int32 views.  The stacks are the towers'
(ReLU layers, a linear last one) with random weights and non-zero biases, on tables inside NaN guard columns, outputs inside sentinel
columns.  The second group compares the one-launch tables with the GENERIC kernel (forced by an identity output index, as
tests/test_chain_forms_gpu.py does) — a kernel that issues every k-step of every tile, also those of a ragged input width (24, 40, 8) — and
with the float64 evaluation of tests/chain_ref.py inside its bound.  The model-level test takes BasicGCN's hoisted scores with and
without AMAR_TOWERS_LAUNCH=two.  The prologue's new form is compared with the one-row-per-thread kernel it replaces (AMAR_XW_FORM=rows).
"""
import os

import numpy as np
import pytest
import torch

from tests import chain_ref as cr
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN, SENTINEL, GUARD = float('nan'), 7.0, 4
TOWER_ACTS = ['relu', 'relu', None]
ROWS = [(1, 1), (15, 17), (64, 1), (129, 4097), (4097, 129)]
DIMS = [[24, 24, 24, 48], [48, 48, 48, 64]]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stack(dims, seed):
    """Random kernels and NON-ZERO biases of a tower, its packed blob on the device."""
    from deep_cbrs_amar_renaissance_amd import capi
    rng = np.random.default_rng(seed)
    ks = [(rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32) for k, n in zip(dims[:-1], dims[1:])]
    bs = [(rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n in dims[1:]]
    assert all((b != 0).all() for b in bs)
    blob, pdims = capi.chain_pack(ks, bs)
    assert pdims == dims
    return ks, bs, torch.from_numpy(blob).to(DEV)


def _table(rows, width, seed):
    """(host array, device view inside NaN guard columns)."""
    arr = np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32)
    buf = torch.full((rows, width + 2 * GUARD), NAN, dtype=torch.float32, device=DEV)
    view = buf[:, GUARD:GUARD + width]
    view.copy_(torch.from_numpy(arr).to(DEV))
    return arr, view


def _output(rows, width):
    buf = torch.full((rows, width + 2 * GUARD), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[:, GUARD:GUARD + width]
    view.fill_(NAN)
    return buf, view


def _guards_untouched(buf, width):
    return bool((buf[:, :GUARD] == SENTINEL).all()) and bool((buf[:, GUARD + width:] == SENTINEL).all())


def _problem(dims, rows, seed):
    ks, bs, blob = _stack(dims, seed)
    arr, table = _table(rows, dims[0], seed + 1000)
    return dict(dims=dims, ks=ks, bs=bs, blob=blob, arr=arr, table=table, rows=rows)


def _two_launches(hip, p, **kw):
    buf, out = _output(p['rows'], p['dims'][-1])
    hip.chain(p['table'], p['blob'], p['dims'], TOWER_ACTS, out, **kw)
    torch.cuda.synchronize()
    assert _guards_untouched(buf, p['dims'][-1])
    return out


def _one_launch(hip, pu, pi):
    bu, ou = _output(pu['rows'], pu['dims'][-1])
    bi, oi = _output(pi['rows'], pi['dims'][-1])
    first, second = (pu['table'], pu['blob'], pu['dims'], TOWER_ACTS, ou), (pi['table'], pi['blob'], pi['dims'], TOWER_ACTS, oi)
    route = hip.chain2_route(first, second)
    assert route['one_launch'] and route['blocks'][0] >= 1 and route['blocks'][1] >= 1, route
    assert route['blocks'][0] <= -(-pu['rows'] // 128) and route['blocks'][1] <= -(-pi['rows'] // 128), route
    assert hip.chain2(first, second) is True
    torch.cuda.synchronize()
    assert _guards_untouched(bu, pu['dims'][-1]) and _guards_untouched(bi, pi['dims'][-1]), 'a store outside an output'
    return ou, oi


@pytest.mark.parametrize('dims', DIMS, ids=lambda d: '-'.join(map(str, d)))
@pytest.mark.parametrize('rows', ROWS, ids=lambda r: '{}x{}'.format(*r))
def test_one_launch_equals_two_launches(hip, rows, dims):
    pu, pi = _problem(dims, rows[0], 11), _problem(dims, rows[1], 23)
    assert hip.towers_route(dims, TOWER_ACTS, rows[0], dims, TOWER_ACTS, rows[1]) == 'one'
    ou, oi = _one_launch(hip, pu, pi)
    wu, wi = _two_launches(hip, pu), _two_launches(hip, pi)
    assert hip.chain_route(pu['table'], pu['blob'], dims, TOWER_ACTS, wu)['kernel'] == hip.CHAIN_KERNEL_ROWS
    assert not bool(torch.isnan(ou).any()) and not bool(torch.isnan(oi).any())
    assert torch.equal(_bits(ou), _bits(wu)), 'user side differs'
    assert torch.equal(_bits(oi), _bits(wi)), 'item side differs'


def test_one_launch_splits_a_long_grid_by_rows(hip):
    """Past the grid cap: every workgroup walks several 128-row tiles of its own problem with its own part's stride."""
    dims = DIMS[0]
    pu, pi = _problem(dims, 2 * 768 * 128 + 45, 5), _problem(dims, 768 * 128 // 3 + 77, 6)
    r = hip.towers_route(dims, TOWER_ACTS, pu['rows'], dims, TOWER_ACTS, pi['rows'], info=True)[1]
    assert sum(r['blocks']) == 768 and abs(r['blocks'][0] / 768 - pu['rows'] / (pu['rows'] + pi['rows'])) < 2 / 768, r
    ou, oi = _one_launch(hip, pu, pi)
    assert torch.equal(_bits(ou), _bits(_two_launches(hip, pu))) and torch.equal(_bits(oi), _bits(_two_launches(hip, pi)))


def test_route_declines(hip):
    """ids on a side, unequal shapes: two launches; chain2 launches nothing and says so."""
    d1, d2 = DIMS
    assert hip.towers_route(d1, TOWER_ACTS, 100, d1, TOWER_ACTS, 100, u_ids=True) == 'two'
    assert hip.towers_route(d1, TOWER_ACTS, 100, d1, TOWER_ACTS, 100, i_ids=True) == 'two'
    assert hip.towers_route(d1, TOWER_ACTS, 100, d2, TOWER_ACTS, 100) == 'two'
    pu, pi = _problem(d1, 100, 1), _problem(d2, 100, 2)
    bu, ou = _output(100, d1[-1])
    bi, oi = _output(100, d2[-1])
    first, second = (pu['table'], pu['blob'], d1, TOWER_ACTS, ou), (pi['table'], pi['blob'], d2, TOWER_ACTS, oi)
    assert not hip.chain2_route(first, second)['one_launch']
    assert hip.chain2(first, second) is False
    torch.cuda.synchronize()
    assert bool(torch.isnan(ou).all()) and bool(torch.isnan(oi).all())                     # nothing was written
    # a stack the tower kernel does not take (all-linear): declined as well
    lin = [None, None, None]
    assert hip.towers_route(d1, lin, 100, d1, lin, 100) == 'two'


def test_basic_rs_towers_take_the_route(hip, monkeypatch):
    """BasicRS.towers: one launch on the rows themselves, two with ids — the same tables as the per-tower calls either way."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    engine.set_seed(3)
    rs = basic.BasicRS([24, 24], [48, 48])
    rs.build_head(24, 24)
    helpers.randomize_biases(rs, seed=9)
    nu, ni = 333, 1217
    emb = torch.randn((nu + ni, 24), device=DEV)
    calls = []
    real = hip.chain2
    monkeypatch.setattr(hip, 'chain2', lambda *a: calls.append(1) or real(*a))
    tu, ti, split = rs.towers(emb[:nu], emb[nu:])
    assert split and calls == [1]
    assert torch.equal(_bits(tu), _bits(rs.tower('u', emb[:nu]))) and torch.equal(_bits(ti), _bits(rs.tower('i', emb[nu:])))
    monkeypatch.setenv('AMAR_TOWERS_LAUNCH', 'two')
    tu2, ti2, _ = rs.towers(emb[:nu], emb[nu:])
    assert calls == [1] and torch.equal(_bits(tu2), _bits(tu)) and torch.equal(_bits(ti2), _bits(ti))
    monkeypatch.delenv('AMAR_TOWERS_LAUNCH')
    ids = torch.arange(nu, device=DEV, dtype=torch.int32)
    tu3, _, _ = rs.towers(emb, emb[nu:], u_ids=ids)
    assert calls == [1] and torch.equal(_bits(tu3), _bits(tu))


# ---- ragged input widths: against the kernel that issues every k-step, and against float64 ------------------------------------------------
@pytest.mark.parametrize('dims', [[24, 24, 24, 48], [40, 48, 48, 64], [8, 24, 24, 48]], ids=lambda d: '-'.join(map(str, d)))
def test_ragged_widths_against_the_generic_kernel_and_float64(hip, dims):
    """Input widths 24 and 40 (a half-filled last k-tile) and 8 (less than one tile), real weights, non-zero biases: the one-launch
    tables equal the generic kernel's bit for bit — it runs every MFMA of every tile — and stay inside the chain tolerance of the
    float64 evaluation (tests/chain_ref.py: c_K = K + 2 per layer)."""
    pu, pi = _problem(dims, 129, 31), _problem(dims, 1000, 37)
    ou, oi = _one_launch(hip, pu, pi)
    for p, got in ((pu, ou), (pi, oi)):
        index = torch.arange(p['rows'], device=DEV, dtype=torch.int32)
        buf, gen = _output(p['rows'], dims[-1])
        assert hip.chain_route(p['table'], p['blob'], dims, TOWER_ACTS, gen, out_index=index)['kernel'] == hip.CHAIN_KERNEL_GENERIC
        hip.chain(p['table'], p['blob'], dims, TOWER_ACTS, gen, out_index=index)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(gen)), 'differs from the generic kernel'
        want, bound = cr.evaluate(p['arr'], None, np.arange(p['rows']), None, False, None, p['ks'], p['bs'], TOWER_ACTS)
        cr.assert_within(got.cpu().numpy(), want, bound, 'one launch, dims {}'.format(dims))


# ---- model level ------------------------------------------------------------------------------------------------------------------------
def test_basic_gcn_hoisted_scores_do_not_depend_on_the_towers_launch(hip, ml1m_s1, monkeypatch):
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from tests.test_models_gpu import GRID1
    model = basic.BasicGCN(ml1m_s1['adj_ui'], **GRID1)
    helpers.randomize_biases(model, seed=5)
    seq = UserItemGraph(ml1m_s1['test'][:10000], ml1m_s1['users'], ml1m_s1['items'], ml1m_s1['adj_ui'], batch_size=2048, shuffle=False)
    # graph=False: eager passes — predict() otherwise keeps its captured hipGraph under a key that does not know the switch, and the
    # second call would replay the first one's launches
    calls, single = [], []
    real2, real1 = hip.chain2, hip._chain_launch
    monkeypatch.setattr(hip, 'chain2', lambda *a: calls.append(1) or real2(*a))
    monkeypatch.setattr(hip, '_chain_launch', lambda *a, **kw: single.append(kw.get('B') is None and kw.get('ids_a') is None) or real1(*a, **kw))
    one = model.predict(seq, hoist=True, graph=False)
    assert len(calls) == 1 and sum(single) == 0, (calls, single)          # both towers in the one launch, no one-table launch
    monkeypatch.setenv('AMAR_TOWERS_LAUNCH', 'two')
    two = model.predict(seq, hoist=True, graph=False)
    assert len(calls) == 1 and sum(single) == 2, (calls, single)          # a launch per tower, and no second chain2
    assert one.shape == (10000, 1) and np.array_equal(one.view(np.int32), two.view(np.int32))
    monkeypatch.delenv('AMAR_TOWERS_LAUNCH')
    faithful = model.predict(seq, hoist=False, graph=False)
    assert np.array_equal(one.view(np.int32), faithful.view(np.int32))


# ---- the X.W prologue ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def xw_inputs():
    """One table per width, made once: the cases read its first N rows."""
    n = 1000003
    g = torch.Generator(device='cpu').manual_seed(77)
    return {F: (torch.randn((n, F), generator=g).to(DEV), torch.randn((F, F), generator=g).to(DEV), (torch.rand(n, generator=g) + 0.1).to(DEV))
            for F in (8, 16)}


@pytest.mark.parametrize('copy', [False, True], ids=['nocopy', 'copy'])
@pytest.mark.parametrize('scale', [False, True], ids=['plain', 'scaled'])
@pytest.mark.parametrize('F', [8, 16])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 1000003])
def test_rowwise_xw_equals_the_row_per_thread_kernel(hip, xw_inputs, monkeypatch, N, F, scale, copy):
    x_all, w, sc_all = xw_inputs[F]
    sc = sc_all[:N].contiguous() if scale else None
    xbuf = torch.full((N, F + 2 * GUARD), NAN, dtype=torch.float32, device=DEV)       # X inside NaN guard columns: ldx = F + 8
    x = xbuf[:, GUARD:GUARD + F]
    x.copy_(x_all[:N])

    def run():
        hb = torch.full((N, F + 2 * GUARD), SENTINEL, dtype=torch.float32, device=DEV)  # H inside sentinel columns: ldh = F + 8
        cat = torch.full((N, 3 * F + 2 * GUARD), SENTINEL, dtype=torch.float32, device=DEV)
        hbuf = hb[:, GUARD:GUARD + F]
        hbuf.fill_(NAN)
        hip.rowwise_xw(x, w, hbuf, copy_to=cat[:, GUARD:GUARD + F] if copy else None, row_scale=sc)
        torch.cuda.synchronize()
        assert bool((hb[:, :GUARD] == SENTINEL).all()) and bool((hb[:, GUARD + F:] == SENTINEL).all()), 'a store outside H'
        return hbuf.contiguous(), cat, hb

    h_new, cat_new, _ = run()
    monkeypatch.setenv('AMAR_XW_FORM', 'rows')
    h_old, cat_old, _ = run()
    assert not bool(torch.isnan(h_new).any())
    assert torch.equal(_bits(h_new), _bits(h_old))
    assert torch.equal(_bits(cat_new), _bits(cat_old))
    if copy:
        assert torch.equal(cat_new[:, GUARD:GUARD + F], x) and bool((cat_new[:, GUARD + F:] == SENTINEL).all()) and bool((cat_new[:, :GUARD] == SENTINEL).all())
    else:
        assert bool((cat_new == SENTINEL).all())
    # the products themselves: k ascending fmaf from 0 is what float64 rounds to within K ulps of the absolute sum
    if N <= 65:
        want = x.double() @ w.double() * (sc.double()[:, None] if scale else 1.0)
        bound = (F + 2) * 2.0 ** -24 * (x.double().abs() @ w.double().abs()) * (sc.double()[:, None] if scale else 1.0)
        assert bool(((h_new.double() - want).abs() <= bound).all())

"""GPU, model level: the scores of a prepared pair list (models.basic.PairPlan, two-step way back forced) are the same bits whether
the second launch finishes its windows in LDS (amar_scatter_closed_f32, the default), stores score by score
(AMAR_PAIR_SCATTER=global), or the list is scored directly without a plan."""
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _routes_taken(monkeypatch, capi):
    """Record which entry point capi.scatter hands each call to."""
    lib, taken = capi.load(), []
    for name in ('amar_scatter_closed_f32', 'amar_scatter_f32'):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda fn, name: lambda *a: (taken.append(name), fn(*a))[1])(fn, name), raising=False)
    return taken


@pytest.mark.parametrize('window', [None, 40_064])
def test_basic_head_scores_same_bits_on_both_routes(hip, monkeypatch, window):
    """window None: the plan's own cut of this list (one workgroup per window); 40 064: windows of the size class that ships for
    ml1m(s=64), two workgroups each, with P just above the two-step threshold p > 2 window and a last window of 3 scores."""
    from deep_cbrs_amar_renaissance_amd import capi, engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    monkeypatch.setenv('AMAR_PAIR_WINDOW_MIN', '0')
    monkeypatch.delenv('AMAR_PAIR_SCATTER', raising=False)
    engine.set_seed(3)
    nu, ni = 5000, 3000
    rs = basic.BasicRS([24, 24], [48, 48])
    rs.build_head(24, 24)
    helpers.randomize_biases(rs, seed=4)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    emb = torch.randn((nu + ni, 24), device=DEV, generator=g)
    P = 2 * (window or 65_536) + 3
    u = torch.randint(0, nu, (P,), device=DEV, generator=g, dtype=torch.int32)
    i = (torch.randint(0, ni, (P,), device=DEV, generator=g, dtype=torch.int32) + nu).to(torch.int32)
    tw = rs.towers(emb[:nu], emb[nu:])
    direct = rs.score_towers(tw, u, i, 0, nu)
    plan = basic.PairPlan(u, i, window=window)
    assert plan.mid_index is not None and plan.max_window == plan.window and (P % plan.window) % 2 == 1
    assert window is None or (plan.n_windows == 3 and P % plan.window == 3)
    taken = _routes_taken(monkeypatch, capi)
    lds = rs.score_towers(tw, u, i, 0, nu, pair_plan=plan)
    monkeypatch.setenv('AMAR_PAIR_SCATTER', 'global')
    glob = rs.score_towers(tw, u, i, 0, nu, pair_plan=plan)
    assert taken == ['amar_scatter_closed_f32', 'amar_scatter_f32']
    assert torch.equal(lds, glob) and torch.equal(lds, direct)


def test_hybrid_head_scores_same_bits_on_both_routes(hip, ml1m_s1, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd.models import hybrid, basic
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    monkeypatch.setenv('AMAR_PAIR_WINDOW_MIN', '0')
    monkeypatch.delenv('AMAR_PAIR_SCATTER', raising=False)
    cfg = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[[24, 24], [256, 64], [64, 64]], clf_units=[64, 64],
               l2_regularizer=1e-4, final_node='concatenation', aggregate='mean', dropout_rate=0.0, activation='relu', feature_based=True)
    n_ent = len(ml1m_s1['users']) + len(ml1m_s1['items'])
    nu = len(ml1m_s1['users'])
    bert = torch.from_numpy(synthetic.entity_embeddings(n_ent, 768, 'bert')).to(DEV)
    model = hybrid.HybridBertGCN(ml1m_s1['adj_ui'], **cfg)
    model.rs.build_head(model.gnn.output_dim(), 768)
    helpers.randomize_biases(model, seed=23)
    g = torch.Generator(device=DEV)
    g.manual_seed(24)
    P = 150_001                                             # the smallest list of test_hybrid_pair_stage_on_prepared_list
    u = torch.randint(0, nu, (P,), device=DEV, generator=g, dtype=torch.int32)
    i = (torch.randint(0, n_ent - nu, (P,), device=DEV, generator=g, dtype=torch.int32) + nu).to(torch.int32)
    emb = model.gnn(None)
    rs = model.rs
    tw = rs.towers(emb[:nu], emb[nu:], bert[:nu], bert[nu:])
    assert tw[4]                                            # folded: the fused two-branch head runs
    direct = rs.score_towers(tw, u, i, 0, nu)
    plan = basic.PairPlan(u, i)
    assert plan.mid_index is not None
    taken = _routes_taken(monkeypatch, capi)
    lds = rs.score_towers(tw, u, i, 0, nu, pair_plan=plan)
    monkeypatch.setenv('AMAR_PAIR_SCATTER', 'global')
    glob = rs.score_towers(tw, u, i, 0, nu, pair_plan=plan)
    assert taken == ['amar_scatter_closed_f32', 'amar_scatter_f32']
    assert torch.equal(lds, glob) and torch.equal(lds, direct)

"""CPU: which form the way back of the scores takes (capi.scatter_route), and that models.basic.PairPlan keeps the promise the LDS
form needs — every window of its table is closed and its longest window is reported truly.  Nothing is launched here."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capacity_constant_matches_header():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    m = re.search(r'#define\s+AMAR_SCATTER_CLOSED_MAX_WINDOW\s+(\d+)', header)
    assert m and int(m.group(1)) == capi.SCATTER_CLOSED_MAX_WINDOW
    assert 'amar_scatter_closed_f32' in capi.SIGNATURES and re.search(r'\bint\s+amar_scatter_closed_f32\s*\(', header)


def test_scatter_route_edges(monkeypatch):
    from deep_cbrs_amar_renaissance_amd import capi
    monkeypatch.delenv('AMAR_PAIR_SCATTER', raising=False)
    cap = capi.SCATTER_CLOSED_MAX_WINDOW
    assert capi.scatter_route(1000, 1, 100, True) == 'lds'
    assert capi.scatter_route(1, 1, 1, True) == 'lds'
    assert capi.scatter_route(1000, 3, 100, True) == 'global'                 # a column of a wider destination
    assert capi.scatter_route(1000, 1, 100, False) == 'global'                # no promise, no LDS form
    assert capi.scatter_route(10 * cap, 1, cap, True) == 'lds'                # a window at the capacity
    assert capi.scatter_route(10 * cap, 1, cap + 1, True) == 'global'         # and one above it
    assert capi.scatter_route(0, 1, 0, True) == 'global'                      # nothing to move
    assert capi.scatter_route(1000, 1, None, True) == 'global'                # longest window unknown
    assert capi.scatter_route(1000, 1, 0, True) == 'global'
    monkeypatch.setenv('AMAR_PAIR_SCATTER', 'global')
    assert capi.scatter_route(1000, 1, 100, True) == 'global'
    monkeypatch.setenv('AMAR_PAIR_SCATTER', 'lds')                            # only 'global' is a switch
    assert capi.scatter_route(1000, 1, 100, True) == 'lds' and capi.scatter_route(1000, 1, 100, False) == 'global'


@pytest.mark.parametrize('P,window', [(3 * 4096 + 5, 4096), (3 * 40001 + 5, 40001), (200_001, None)])
def test_pair_plan_windows_are_closed(monkeypatch, P, window):
    """Lists of 3 windows + 5 pairs (two-step path forced; a window of the caller's choice) and one cut by the plan's own rule:
    final_index restricted to a window's positions sorts to exactly those positions, the last window is the short one, and
    max_window is the true maximum."""
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd.models.basic import PairPlan
    monkeypatch.setenv('AMAR_PAIR_WINDOW_MIN', '0')
    monkeypatch.delenv('AMAR_PAIR_SCATTER', raising=False)
    g = torch.Generator()
    g.manual_seed(11)
    u = torch.randint(0, 500, (P,), generator=g, dtype=torch.int32)
    i = torch.randint(500, 800, (P,), generator=g, dtype=torch.int32)
    plan = PairPlan(u, i, window=window)
    w = plan.window
    assert plan.mid_index is not None and (window is None or (w == window and plan.n_windows == 4))
    off = plan.window_off.tolist()
    assert off[0] == 0 and off[-1] == P and len(off) == plan.n_windows + 1
    lengths = [b - a for a, b in zip(off, off[1:])]
    assert lengths == [w] * (plan.n_windows - 1) + [P - (plan.n_windows - 1) * w] and 0 < lengths[-1] < w
    assert plan.max_window == max(lengths) == w
    assert capi.scatter_route(P, 1, plan.max_window, True) == 'lds'
    for lo, hi in zip(off, off[1:]):
        assert torch.equal(torch.sort(plan.final_index[lo:hi].long()).values, torch.arange(lo, hi))
    assert torch.equal(plan.final_index[plan.mid_index.long()], plan.out_index)
    win = plan.final_index.long() // plan.window
    assert bool((win[1:] >= win[:-1]).all())


def test_pair_plan_window_rule(monkeypatch):
    """Lists whose windows fit the LDS form are cut into 256 windows, a multiple of the kernel's chunk each (ml1m(s=64): 47 232
    scores); longer lists, and any list with the LDS form switched off, keep the power-of-two windows of the global form."""
    from deep_cbrs_amar_renaissance_amd.models.basic import PairPlan
    monkeypatch.delenv('AMAR_PAIR_SCATTER', raising=False)
    window_of = PairPlan.window_for
    assert window_of(12_089_292) == 47_232 and -(-12_089_292 // 47_232) == 256
    assert window_of(1 << 22) == 16_384
    assert window_of(256 * 65_536) == 65_536
    assert window_of(256 * 65_536 + 1) == 1 << 16           # 256 windows would pass the capacity: the global form's rule from here on
    assert window_of(20_000_000) == 1 << 17
    assert window_of(48_000_000) == 1 << 18                 # ml1m(s=256)'s size
    monkeypatch.setenv('AMAR_PAIR_SCATTER', 'global')
    assert window_of(12_089_292) == 1 << 16


def test_pair_plan_without_windows_reports_none(monkeypatch):
    from deep_cbrs_amar_renaissance_amd.models.basic import PairPlan
    monkeypatch.setenv('AMAR_PAIR_WINDOW_MIN', str(1 << 30))
    u = torch.arange(1000, dtype=torch.int32)
    plan = PairPlan(u, u + 1000)
    assert plan.mid_index is None and plan.n_windows == 0 and plan.max_window == 0

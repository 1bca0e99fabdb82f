"""Host side of cursor paging (no GPU): the header / binding / library agreement on amar_recommend_after_f32 and
amar_topk_segmented_after_f32 and the cursor constants the header states, the refusals of both entry points with their codes and
order (called on the host the way tests/test_rank_refusals_cpu.py calls their siblings: no case reaches a launch), the argument
errors of `recommend_after` / `recommend_deep` on models without weights, `check_after`, and tests/after_ref.py against a brute-force
sort on rows with bulk ties."""
import inspect
import os
import re

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd import recommend as rec
from tests import after_ref
from tests.test_rank_refusals_cpu import BASE, BUF, C132, EINVAL, EMPTY, EUNSUPPORTED, NO_OUT, OK, RECOMMEND, _head, _ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. header, binding, library -------------------------------------------------------------------------------------------------
def _declared(header, sym):
    decl = re.search(r'int ' + sym + r'\((.*?)\);', header, re.S)
    assert decl is not None, sym
    return [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    args = _declared(header, 'amar_recommend_after_f32')
    assert len(args) == len(capi.SIGNATURES['amar_recommend_after_f32'][1]) == 25
    assert args[16] == 'const float *after_scores' and args[17] == 'const int32_t *after_items' and args[-1] == 'amar_stream_t stream'
    assert args[:16] == _declared(header, 'amar_recommend_f32')[:16] and args[18:] == _declared(header, 'amar_recommend_f32')[16:]
    pair = _declared(header, 'amar_topk_segmented_after_f32')
    assert len(pair) == len(capi.SIGNATURES['amar_topk_segmented_after_f32'][1]) == 10
    assert pair[5] == 'const float *after_scores' and pair[6] == 'const int32_t *after_items'
    assert pair[:5] + pair[7:] == _declared(header, 'amar_topk_segmented_f32')
    # the cursor constants, stated next to the declaration
    doc = header[header.index('Top-k AFTER a position'):header.index('int amar_recommend_after_f32(')]
    for stated in ('(+inf, -1)', '(-inf, -1)', 'NaN', 'bit for bit', 'NOT by the user row', 'excluded row'):
        assert stated in doc, stated
    assert int(re.search(r'#define\s+AMAR_AFTER_NO_ITEM\s+\((-?\d+)\)', header).group(1)) == -1
    lib = capi.load()
    assert hasattr(lib, 'amar_recommend_after_f32') and hasattr(lib, 'amar_topk_segmented_after_f32')
    names = list(capi.SIGNATURES)                                                                 # ... in the header's order
    order = ('amar_topk_segmented_f32', 'amar_topk_segmented_after_f32', 'amar_recommend_slices', 'amar_recommend_among_f32',
             'amar_recommend_after_f32', 'amar_nearest_slices')
    at = [header.index(' ' + n + '(') for n in order]
    assert at == sorted(at) and [names.index(n) for n in order] == sorted(names.index(n) for n in order)
    makefile = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_rank_after.hip' in re.search(r'^SRCS\s*=(.*)$', makefile, flags=re.M).group(1).split()


def test_capi_exposes_both_wrappers():
    assert list(inspect.signature(capi.recommend_after).parameters) == [
        'Tu', 'Ti', 'wpack', 'dims', 'acts', 'in_act', 'k', 'after_items', 'after_scores', 'users', 'excl_ptr', 'excl_items', 'n_slices']
    assert list(inspect.signature(capi.topk_segmented_after).parameters) == ['seg_ptr', 'item_ids', 'scores', 'k', 'after_items', 'after_scores']
    assert rec.K_MAX == 64 and rec.DEEP_K_MAX == 1024
    assert rec.page_sizes(1) == [1] and rec.page_sizes(64) == [64] and rec.page_sizes(65) == [64, 1] and rec.page_sizes(150) == [64, 64, 22]
    assert rec.page_sizes(1024) == [64] * 16
    assert 'after' in inspect.signature(rec.pairs).parameters and callable(rec.after_fused)


# ---- 2. the refusals, on the host ----------------------------------------------------------------------------------------------------
def after(**fault):
    c = dict(dict(BASE, after_scores=BUF, after_items=BUF), **fault)
    return capi.load().amar_recommend_after_f32(*_head(c), c['users'], c['m'], c['excl_ptr'], c['excl_items'], c['after_scores'],
                                                c['after_items'], c['k'], c['n_slices'], c['ws_items'], c['ws_scores'], c['out_items'],
                                                c['out_scores'], None)


NO_SCORES, NO_ITEMS, NO_CURSOR = dict(after_scores=None), dict(after_items=None), dict(after_scores=None, after_items=None)
AFTER = RECOMMEND + [                                  # amar_recommend_f32's checks in its order, then the cursor's
    ('scores_without_items', NO_ITEMS, EINVAL),
    ('items_without_scores', NO_SCORES, EINVAL),
    ('rows_without_a_cursor', NO_CURSOR, EINVAL),
    ('k_65_and_items_without_scores', dict(NO_SCORES, k=65), EUNSUPPORTED),                # the k limit comes first
    ('k_65_and_rows_without_a_cursor', dict(NO_CURSOR, k=65), EUNSUPPORTED),
    ('m_is_not_n_users_and_rows_without_a_cursor', dict(NO_CURSOR, m=2), EINVAL),
    ('rows_without_a_cursor_and_c1_132', dict(NO_CURSOR, **C132), EINVAL),                  # the cursor comes before the tables
    ('scores_without_items_and_hidden_width_1', dict(NO_ITEMS, dims=[8, 1, 1]), EINVAL),    # ... and before the route
    ('empty_without_a_cursor', dict(EMPTY, **NO_CURSOR, **NO_OUT), OK),                     # no rows: the cursor may be NULL
    ('empty_with_half_a_cursor', dict(EMPTY, **NO_ITEMS), EINVAL),                          # ... but the two go together
]


@pytest.mark.parametrize('name,fault,code', AFTER, ids=_ids(AFTER))
def test_recommend_after_refusals(name, fault, code):
    assert fault and code in (OK, EINVAL, EUNSUPPORTED) and (code != OK or fault.get('m') == 0)      # no case is the valid base
    assert after(**fault) == code


PAIR_BASE = dict(seg_ptr=BUF, item_ids=BUF, scores=BUF, n_users=3, k=2, after_scores=BUF, after_items=BUF, out_items=BUF, out_scores=BUF)
NOTHING = dict(n_users=0, item_ids=None, scores=None, out_items=None, out_scores=None)
PAIR = [
    ('k_65', dict(k=65), EUNSUPPORTED),
    ('k_0', dict(k=0), EINVAL),
    ('negative_n_users', dict(n_users=-1), EINVAL),
    ('null_seg_ptr', dict(seg_ptr=None), EINVAL),
    ('null_seg_ptr_and_k_65', dict(seg_ptr=None, k=65), EINVAL),                            # amar_topk_segmented_f32's order
    ('scores_without_items', NO_ITEMS, EINVAL),
    ('items_without_scores', NO_SCORES, EINVAL),
    ('users_without_a_cursor', NO_CURSOR, EINVAL),
    ('k_65_and_users_without_a_cursor', dict(NO_CURSOR, k=65), EUNSUPPORTED),               # the k limit comes first
    ('no_users', dict(NOTHING, **NO_CURSOR), OK),
    ('no_users_with_half_a_cursor', dict(NOTHING, **NO_SCORES), EINVAL),
    ('null_scores', dict(scores=None), EINVAL),
    ('null_outputs', dict(out_items=None, out_scores=None), EINVAL),
]


@pytest.mark.parametrize('name,fault,code', PAIR, ids=_ids(PAIR))
def test_topk_segmented_after_refusals(name, fault, code):
    c = dict(PAIR_BASE, **fault)
    assert fault and (code != OK or c['n_users'] == 0)
    lib = capi.load()
    assert lib.amar_topk_segmented_after_f32(c['seg_ptr'], c['item_ids'], c['scores'], c['n_users'], c['k'], c['after_scores'],
                                             c['after_items'], c['out_items'], c['out_scores'], None) == code
    if 'after_scores' not in fault and 'after_items' not in fault:                          # its sibling keeps its checks and codes
        assert lib.amar_topk_segmented_f32(c['seg_ptr'], c['item_ids'], c['scores'], c['n_users'], c['k'], c['out_items'],
                                           c['out_scores'], None) == code


# ---- 3. the Python surface ---------------------------------------------------------------------------------------------------------
NU, NI = 4, 3


class _Train:
    def __init__(self, n_users, n_items):
        self.users, self.items = np.arange(n_users), np.arange(n_items)
        self.ratings = np.zeros((0, 3), dtype=np.int64)


def test_check_after():
    rows, scores = rec.check_after(([4, -1, 6], [0.5, float('-inf'), float('inf')]), 3, NU, NI)
    assert rows.dtype == np.int32 and rows.tolist() == [0, -1, 2] and scores.dtype == np.float32 and scores[0] == 0.5
    assert np.isneginf(scores[1]) and np.isposinf(scores[2])
    import torch
    rows, scores = rec.check_after((torch.tensor([5]), torch.tensor([0.25], dtype=torch.float64)), 1, NU, NI)
    assert rows.tolist() == [1] and scores.tolist() == [0.25]
    rows, scores = rec.check_after((np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)), 0, NU, NI)
    assert rows.size == 0 and scores.size == 0
    for bad in (None, 'ab', 5, ([4],), ([4], [0.5], [1]),
                ([4, 5], [0.5]), ([4], [0.5, 0.1]), ([4, 5, 6], [0.1, 0.2, 0.3]),            # lengths
                ([4.0, 5.0], [0.5, 0.5]), ([True, False], [0.5, 0.5]),                         # items that are no integers
                ([3, 4], [0.5, 0.5]), ([4, 7], [0.5, 0.5]), ([4, -2], [0.5, 0.5]),             # neither an item of the trainset nor -1
                ([4, 5], [0.5, float('nan')]), ([4, 5], ['a', 'b'])):                          # NaN, no numbers
        with pytest.raises(ValueError, match='after'):
            rec.check_after(bad, 2, NU, NI)


def test_models_reject_bad_arguments_before_any_device_work():
    """recommend_after() / recommend_deep() of every scoring class check their arguments before they touch the towers: the models
    here have no weights at all."""
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    train = _Train(NU, NI)
    ok = ([4, 5, 6, -1], [0.5, 0.5, 0.5, float('-inf')])
    for cls in (basic.BasicRS, basic.BasicGNN, hybrid.HybridCBRS, hybrid.HybridBertGNN):
        model = object.__new__(cls)
        for k in (0, 65, -1, 2.5, True, None):
            with pytest.raises(ValueError, match='k must'):
                cls.recommend_after(model, train, ok, k=k)
        for k in (0, 1025, -1, 2.5, True, None, 64.0):
            with pytest.raises(ValueError, match='k must'):
                cls.recommend_deep(model, train, k)
        for users in ([0, NU], [-1], [0.5]):
            with pytest.raises(ValueError):
                cls.recommend_after(model, train, ([4], [0.5]), k=5, users=users)
            with pytest.raises(ValueError):
                cls.recommend_deep(model, train, 100, users=users)
        for after, users in ((([4, 5, 6], [0.5] * 3), None), (([4, 5], [0.5, 0.5]), [0]), (([4], [0.5, 0.5]), [0, 1]),      # lengths
                             (([4.0], [0.5]), [0]), (([NU - 1], [0.5]), [0]), (([NU + NI], [0.5]), [0]), (([-2], [0.5]), [0]),
                             (([4], [float('nan')]), [0]), ([4], [0]), (None, [0])):
            with pytest.raises(ValueError, match='after'):
                cls.recommend_after(model, train, after, k=5, users=users)
        u, i, s = cls.recommend_after(model, train, ([], []), k=7, users=[])                  # nothing listed: nothing computed
        assert u.shape == (0,) and i.shape == (0, 7) and s.shape == (0, 7)
        with pytest.raises(ValueError):                                                      # the old calls keep their limit
            cls.recommend(model, train, k=65)
        with pytest.raises(ValueError):
            cls.recommend_among(model, train, [NU], k=65)


def test_routes(monkeypatch):
    """recommend_after / recommend_deep go where _group_route(kind='recommend') says, with the checked cursor."""
    calls = []

    class Model(rec.SimilarSearch):
        def _group_route(self, trainset, kind='group'):
            calls.append(('route', kind))
            return self.answer

    monkeypatch.setattr(rec, 'after_fused', lambda towers, plan, train, k, users, excl, cursor: calls.append(
        ('after_fused', towers, plan, k, users, excl, cursor[0].tolist(), cursor[1].tolist())) or 'fused')
    monkeypatch.setattr(rec, 'deep_fused', lambda towers, plan, train, k, users, excl: calls.append(('deep_fused', towers, plan, k, users, excl)) or 'deep fused')
    monkeypatch.setattr(rec, 'deep_pairs', lambda fn, train, k, users, excl, device=None: calls.append(('deep_pairs', fn, k, users, excl, device)) or 'deep pairs')
    model, train = Model(), _Train(NU, NI)
    model.answer = ('fused', 'towers', 'plan')
    assert model.recommend_after(train, ([6, -1], [0.5, float('-inf')]), k=3, users=[1, 0]) == 'fused'
    assert calls == [('route', 'recommend'), ('after_fused', 'towers', 'plan', 3, [1, 0], True, [2, -1], [0.5, float('-inf')])]
    del calls[:]
    assert model.recommend_deep(train, 150, exclude_seen=False) == 'deep fused'
    assert calls == [('route', 'recommend'), ('deep_fused', 'towers', 'plan', 150, None, False)]
    del calls[:]
    model.answer = ('pairs', 'score_fn', 'dev')
    assert model.recommend_deep(train, 1024, users=[2]) == 'deep pairs'
    assert calls == [('route', 'recommend'), ('deep_pairs', 'score_fn', 1024, [2], True, 'dev')]


# ---- 4. the reference against a brute-force sort -----------------------------------------------------------------------------------
def _brute(scores, k, cursor, items, excluded):
    cs, ci = cursor
    kept = [(float(s), int(i)) for s, i in zip(scores, items)
            if int(i) not in excluded and (float(s) < float(cs) or (float(s) == float(cs) and int(i) > ci))]
    kept.sort(key=lambda p: (-p[0], p[1]))
    kept = kept[:k]
    return [i for _, i in kept] + [-1] * (k - len(kept)), [s for s, _ in kept] + [float('-inf')] * (k - len(kept))


def test_after_ref_against_brute_force():
    rng = np.random.default_rng(11)
    checked = 0
    for n in (1, 5, 64, 65, 200):
        for trial in range(6):
            scores = rng.choice(np.array([0.0, 0.0, 0.0, 0.25, 0.5, 0.75], dtype=np.float32), size=n)     # bulk ties: half the rows at 0
            loose = rng.random(n) < 0.3
            scores[loose] = rng.random(int(loose.sum())).astype(np.float32)
            items = rng.permutation(3 * n)[:n] if trial % 2 else np.arange(n)
            excluded = set(rng.choice(items, size=n // 4, replace=False).tolist()) if trial % 3 else set()
            cursors = [after_ref.START, after_ref.END, (np.float32(0.0), -1), (np.float32(0.0), int(items[n // 2])),
                       (np.float32(0.0), 10 ** 9), (np.float32(0.3), 7), (np.float32(0.5), int(items[0])), (np.float32('nan'), 0),
                       (np.float32(-1.0), 0), (scores[n // 3], int(items[n // 3]))]
            for cursor in cursors:
                for k in (1, 10, 64):
                    got_i, got_s = after_ref.next_page(scores, k, cursor, items=items, excluded=excluded)
                    want_i, want_s = _brute(scores, k, cursor, items, excluded)
                    assert got_i.tolist() == want_i and got_s.tolist() == want_s, (n, trial, cursor, k)
                    checked += int((got_i >= 0).sum())
            # chained pages are the sorted list, cut
            whole = _brute(scores, n, after_ref.START, items, excluded)[0]
            chain, cursor = [], after_ref.START
            for _ in range(n // 7 + 2):
                page_i, page_s = after_ref.next_page(scores, 7, cursor, items=items, excluded=excluded)
                chain += page_i.tolist()
                cursor = (page_s[-1], int(page_i[-1]))
            assert chain[:n] == whole and all(i == -1 for i in chain[n:])
    assert checked > 1000
    assert after_ref.next_page(np.zeros(3, dtype=np.float32), 2, after_ref.END)[0].tolist() == [-1, -1]
    got = after_ref.pages(np.array([[0.5, 0.5, 0.1], [0.2, 0.9, 0.2]], dtype=np.float32), 2, (np.array([0, -1]), np.array([0.5, np.inf], dtype=np.float32)),
                          excluded=[set(), {1}])
    assert got[0].tolist() == [[1, 2], [0, 2]]

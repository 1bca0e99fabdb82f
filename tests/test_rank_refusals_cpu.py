"""The order in which the fused rankers' C entry points refuse a call (no GPU): amar_recommend_f32, amar_recommend_among_f32,
amar_recommend_group_f32, amar_rank_of_f32 and the three *_slices queries, called through the raw ctypes handle with a null stream.

Every case ends in a refusal or in the empty call's AMAR_OK, so nothing here reaches a launch or any HIP call: the host code never
dereferences a table before it launches (only `dims` and `acts` are read on the host), which lets 16-byte-aligned host buffers
stand in for the device pointers.  A case is the valid base call with one fault, or with two faults at once — a probe: the code
of the check that comes first in the launcher is the one expected.  The valid base is c1 = 8, dims = [8, 8, 1] (two layers),
ld = 8, 3 users, 5 items, k = 2; it is never called without a fault."""
import ctypes

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
RELU, SIGMOID = capi.ACT_CODES['relu'], capi.ACT_CODES['sigmoid']
WIDE = dict(c1=128, ldu=128, ldi=128, dims=[128, 128, 128, 1], acts=[RELU, RELU, SIGMOID])     # no ranker has the LDS for this head
C132 = dict(c1=132, ldu=132, ldi=132, dims=[132, 8, 1])
MANY = 1 << 35                                                           # selector rows whose blocks of 16 pass the 2^31 grid limit

_raw = np.zeros(256, dtype=np.uint8)
BUF = _raw.ctypes.data + (-_raw.ctypes.data) % 16                        # stands in for every device pointer; never dereferenced
NAN = float('nan')


def _i32(values):
    return None if values is None else (ctypes.c_int32 * len(values))(*values)


def _head(c):
    return [c['Tu'], c['ldu'], c['n_users'], c['Ti'], c['ldi'], c['n_items'], c['c1'], c['wpack'], _i32(c['dims']), _i32(c['acts']),
            c['n_layers'] if 'n_layers' in c else len(c['dims']) - 1, c['in_act']]


BASE = dict(Tu=BUF, ldu=8, n_users=3, Ti=BUF, ldi=8, n_items=5, c1=8, wpack=BUF, dims=[8, 8, 1], acts=[RELU, SIGMOID], in_act=RELU,
            users=None, m=3, excl_ptr=None, excl_items=None, k=2, n_slices=0, ws_items=None, ws_scores=None, out_items=BUF, out_scores=BUF)
NO_OUT = dict(out_items=None, out_scores=None)


def recommend(**fault):
    c = dict(BASE, **fault)
    return capi.load().amar_recommend_f32(*_head(c), c['users'], c['m'], c['excl_ptr'], c['excl_items'], c['k'], c['n_slices'],
                                          c['ws_items'], c['ws_scores'], c['out_items'], c['out_scores'], None)


def among(**fault):
    c = dict(dict(BASE, cand=BUF, n_cand=3), **fault)
    return capi.load().amar_recommend_among_f32(*_head(c), c['users'], c['m'], c['excl_ptr'], c['excl_items'], c['cand'], c['n_cand'],
                                                c['k'], c['n_slices'], c['ws_items'], c['ws_scores'], c['out_items'], c['out_scores'], None)


def group(**fault):
    c = dict(dict(BASE, grp_ptr=BUF, grp_users=BUF, n_members=4, strategy=0, min_score=float('-inf')), **fault)
    return capi.load().amar_recommend_group_f32(*_head(c), c['grp_ptr'], c['grp_users'], c['m'], c['n_members'], c['excl_ptr'],
                                                c['excl_items'], c['strategy'], c['min_score'], c['k'], c['n_slices'], c['ws_items'],
                                                c['ws_scores'], c['out_items'], c['out_scores'], None)


def rank_of(**fault):
    c = dict(dict(BASE, tgt_ptr=BUF, tgt_items=BUF, n_targets=4, max_targets=2, out=BUF), **fault)
    return capi.load().amar_rank_of_f32(*_head(c), c['users'], c['m'], c['excl_ptr'], c['excl_items'], c['tgt_ptr'], c['tgt_items'],
                                        c['n_targets'], c['max_targets'], c['n_slices'], c['out'], c['out'], c['out'], c['out'], None)


# What the four launchers check alike once their own leading checks have passed: the tables (rank_check_tables), then the route.
# (name, faults, code); `empty` = the faults that make the call an empty one (no selector row).
def _table_and_route_cases(empty):
    return [
        ('c1_not_a_multiple_of_4', dict(c1=6), EINVAL),
        ('ldu_not_a_multiple_of_4', dict(ldu=6), EINVAL),
        ('ldi_below_c1', dict(ldi=4), EINVAL),
        ('tu_unaligned', dict(Tu=BUF + 4), EINVAL),
        ('ti_unaligned', dict(Ti=BUF + 8), EINVAL),
        ('wpack_unaligned', dict(wpack=BUF + 4), EINVAL),
        ('c1_132', C132, EUNSUPPORTED),
        ('c1_132_with_ld_8', dict(c1=132, dims=[132, 8, 1]), EINVAL),           # ld < c1 is read before c1 > 128
        ('bad_in_act', dict(in_act=7), EINVAL),
        ('c1_132_and_bad_in_act', dict(C132, in_act=7), EUNSUPPORTED),
        ('one_layer', dict(dims=[8, 1], acts=[SIGMOID]), EUNSUPPORTED),
        ('ten_layers', dict(dims=[8] * 10 + [1], acts=[RELU] * 9 + [SIGMOID]), EUNSUPPORTED),
        ('bad_in_act_and_one_layer', dict(in_act=7, dims=[8, 1], acts=[SIGMOID]), EINVAL),
        ('dims0_is_not_c1', dict(dims=[16, 8, 1]), EUNSUPPORTED),
        ('last_width_is_not_1', dict(dims=[8, 8, 2]), EUNSUPPORTED),
        ('bad_act_code', dict(acts=[5, SIGMOID]), EINVAL),
        ('c1_132_and_bad_act_code', dict(C132, acts=[5, SIGMOID]), EUNSUPPORTED),      # the tables come before the route
        ('hidden_width_1', dict(dims=[8, 1, 1]), EUNSUPPORTED),
        ('hidden_width_256', dict(dims=[8, 256, 1]), EUNSUPPORTED),
        ('slices_not_the_librarys', dict(n_slices=3), EINVAL),
        ('hidden_width_1_and_slices_not_the_librarys', dict(dims=[8, 1, 1], n_slices=3), EUNSUPPORTED),      # the route comes first
        ('empty_and_bad_act_code', dict(empty, acts=[5, SIGMOID]), EINVAL),
    ]


# The tail the three top-k launchers share: slices, workspaces, the empty call, the outputs, the fit, the grid.
def _topk_tail_cases(empty, two_slices):
    return [
        ('two_slices_without_workspaces', two_slices, EINVAL),
        ('two_slices_without_score_workspace', dict(two_slices, ws_items=BUF), EINVAL),
        ('two_slices_without_workspaces_and_no_fit', dict(two_slices, **WIDE), EINVAL),
        ('empty_with_null_outputs', dict(empty, **NO_OUT), OK),
        ('empty_and_slices_not_the_librarys', dict(empty, n_slices=3), EINVAL),        # the slice checks come before the empty call
        ('empty_and_no_fit', dict(empty, **NO_OUT, **WIDE), OK),                      # the empty call comes before the fit
        ('null_outputs', NO_OUT, EINVAL),
        ('null_score_output', dict(out_scores=None), EINVAL),
        ('null_outputs_and_no_fit', dict(NO_OUT, **WIDE), EINVAL),                     # the outputs come before the fit
        ('no_fit', WIDE, EUNSUPPORTED),
        ('grid_limit', dict(users=BUF, m=MANY), EUNSUPPORTED),
        ('grid_limit_and_null_outputs', dict(users=BUF, m=MANY, **NO_OUT), EINVAL),
    ]


def _ids(cases):
    return [c[0] for c in cases]


EMPTY = dict(users=BUF, m=0)
RECOMMEND = [
    ('k_65', dict(k=65), EUNSUPPORTED),
    ('k_0', dict(k=0), EINVAL),
    ('m_is_not_n_users_without_users', dict(m=2), EINVAL),
    ('k_65_and_m_is_not_n_users', dict(k=65, m=2), EUNSUPPORTED),                    # the k limit comes first
    ('excl_ptr_without_excl_items', dict(excl_ptr=BUF), EINVAL),
    ('k_65_and_excl_ptr_without_excl_items', dict(k=65, excl_ptr=BUF), EUNSUPPORTED),
    ('null_tu', dict(Tu=None), EINVAL),
    ('null_acts', dict(acts=None, n_layers=2), EINVAL),
    ('negative_m', dict(users=BUF, m=-1), EINVAL),
    ('k_65_and_c1_6', dict(k=65, c1=6), EUNSUPPORTED),                               # the leading checks come before the tables
] + _table_and_route_cases(EMPTY) + _topk_tail_cases(EMPTY, dict(n_items=600, n_slices=2))


@pytest.mark.parametrize('name,fault,code', RECOMMEND, ids=_ids(RECOMMEND))
def test_recommend_refusals(name, fault, code):
    assert recommend(**fault) == code


AMONG = RECOMMEND[:-len(_topk_tail_cases(EMPTY, {}))] + _topk_tail_cases(EMPTY, dict(n_items=600, n_cand=600, n_slices=2)) + [
    ('negative_n_cand', dict(n_cand=-1), EINVAL),
    ('n_cand_above_n_items', dict(n_cand=6), EINVAL),
    ('candidates_without_a_list', dict(cand=None), EINVAL),
    ('no_candidates_without_a_list_and_no_rows', dict(cand=None, n_cand=0, **EMPTY, **NO_OUT), OK),
    ('n_cand_above_n_items_and_k_65', dict(n_cand=6, k=65), EINVAL),                  # the candidate check comes before the k limit
    ('k_0_and_n_cand_above_n_items', dict(k=0, n_cand=6), EINVAL),
]


@pytest.mark.parametrize('name,fault,code', AMONG, ids=_ids(AMONG))
def test_recommend_among_refusals(name, fault, code):
    assert among(**fault) == code


NO_GROUPS = dict(m=0)
GROUP = [
    ('k_65', dict(k=65), EUNSUPPORTED),
    ('k_0', dict(k=0), EINVAL),
    ('bad_strategy', dict(strategy=3), EINVAL),
    ('nan_min_score', dict(min_score=NAN), EINVAL),
    ('groups_without_grp_ptr', dict(grp_ptr=None), EINVAL),
    ('members_without_grp_users', dict(grp_users=None), EINVAL),
    ('negative_n_members', dict(n_members=-1), EINVAL),
    ('bad_strategy_and_k_65', dict(strategy=3, k=65), EINVAL),                        # here the k limit is the last leading check
    ('nan_min_score_and_k_65', dict(min_score=NAN, k=65), EINVAL),
    ('groups_without_grp_ptr_and_k_65', dict(grp_ptr=None, k=65), EINVAL),
    ('excl_ptr_without_excl_items', dict(excl_ptr=BUF), EINVAL),
    ('excl_ptr_without_excl_items_and_k_65', dict(excl_ptr=BUF, k=65), EINVAL),       # here the exclusion check precedes the k limit
    ('k_65_and_c1_6', dict(k=65, c1=6), EUNSUPPORTED),
    ('no_groups', dict(NO_GROUPS, grp_ptr=None, **NO_OUT), OK),
] + _table_and_route_cases(NO_GROUPS) + [c for c in _topk_tail_cases(NO_GROUPS, dict(n_items=600, n_slices=2)) if 'grid_limit' not in c[0]] + [
    ('grid_limit', dict(m=MANY), EUNSUPPORTED),
    ('grid_limit_and_null_outputs', dict(m=MANY, **NO_OUT), EINVAL),
]


@pytest.mark.parametrize('name,fault,code', GROUP, ids=_ids(GROUP))
def test_recommend_group_refusals(name, fault, code):
    assert group(**fault) == code


RANK_OF = [
    ('null_outputs_with_targets', dict(out=None), EINVAL),
    ('null_outputs_with_targets_and_c1_132', dict(C132, out=None), EINVAL),           # here the outputs come before the tables
    ('null_outputs_without_targets', dict(out=None, n_targets=0), OK),
    ('m_is_not_n_users_without_users', dict(m=2), EINVAL),
    ('excl_ptr_without_excl_items', dict(excl_ptr=BUF), EINVAL),
    ('entries_without_tgt_ptr', dict(tgt_ptr=None), EINVAL),
    ('targets_without_tgt_items', dict(tgt_items=None), EINVAL),
    ('negative_max_targets', dict(max_targets=-1), EINVAL),
    ('max_targets_65', dict(max_targets=65), EUNSUPPORTED),
    ('max_targets_65_and_bad_act_code', dict(max_targets=65, acts=[5, SIGMOID]), EINVAL),      # the route comes first
    ('max_targets_65_and_c1_132', dict(C132, max_targets=65), EUNSUPPORTED),
    ('max_targets_65_and_slices_not_the_librarys', dict(max_targets=65, n_slices=3), EUNSUPPORTED),
    ('no_fit', WIDE, EUNSUPPORTED),
    ('no_entries_and_no_fit', dict(EMPTY, **WIDE), EUNSUPPORTED),                     # here the fit comes before the empty call
    ('no_fit_and_slices_not_the_librarys', dict(WIDE, n_slices=3), EINVAL),
    ('no_entries', EMPTY, OK),
    ('no_entries_and_no_tgt_ptr', dict(EMPTY, tgt_ptr=None), OK),
    ('no_targets', dict(n_targets=0), OK),
    ('no_targets_and_slices_not_the_librarys', dict(n_targets=0, n_slices=3), EINVAL),
    ('grid_limit_without_targets', dict(users=BUF, m=MANY, n_targets=0), EUNSUPPORTED),        # the grid limit too precedes the empty call
] + _table_and_route_cases(EMPTY)


@pytest.mark.parametrize('name,fault,code', RANK_OF, ids=_ids(RANK_OF))
def test_rank_of_refusals(name, fault, code):
    assert rank_of(**fault) == code


def test_no_case_reaches_a_launch():
    """The valid base is a launch, so every case must differ from it; and the listed codes are refusals or the empty call."""
    for cases in (RECOMMEND, AMONG, GROUP, RANK_OF):
        assert all(fault and code in (OK, EINVAL, EUNSUPPORTED) for _, fault, code in cases)
        assert len(set(_ids(cases))) == len(cases)
        for _, fault, code in cases:
            if code == OK:                                                   # an empty call: no selector row, or (rank_of) no target
                assert fault.get('m') == 0 or fault.get('n_targets') == 0


SLICES = [
    ('negative_rows', dict(m=-1), EINVAL),
    ('negative_items', dict(n_items=-1), EINVAL),
    ('null_dims', dict(dims=None, n_layers=2), EINVAL),
    ('one_layer', dict(dims=[8, 1]), EINVAL),
    ('ten_layers', dict(dims=[8] * 10 + [1]), EINVAL),
    ('width_256', dict(dims=[8, 256, 1]), EUNSUPPORTED),
    ('negative_rows_and_width_256', dict(m=-1, dims=[8, 256, 1]), EINVAL),
]


@pytest.mark.parametrize('symbol', ['amar_recommend_slices', 'amar_rank_of_slices', 'amar_recommend_group_slices'])
@pytest.mark.parametrize('name,fault,code', SLICES, ids=_ids(SLICES))
def test_slices_refusals(symbol, name, fault, code):
    c = dict(dict(m=3, n_members=4, n_items=5, dims=[8, 8, 1], n_slices=0), **fault)
    n_layers = c['n_layers'] if 'n_layers' in c else len(c['dims']) - 1
    sizes = (c['m'], c['n_members'], c['n_items']) if symbol == 'amar_recommend_group_slices' else (c['m'], c['n_items'])
    fn = getattr(capi.load(), symbol)
    assert fn(*sizes, _i32(c['dims']), n_layers, c['n_slices']) == code
    if symbol == 'amar_recommend_group_slices':
        assert fn(3, -1, 5, _i32([8, 8, 1]), 2, 0) == EINVAL
    assert fn(*((3, 4, 5) if symbol == 'amar_recommend_group_slices' else (3, 5)), _i32([8, 8, 1]), 2, 0) == 1      # the valid base

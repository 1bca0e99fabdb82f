"""CPU: the case list of tests/econfigs_cases.py covers the golden it is made from (no GPU).

The GPU tests of tests/test_econfigs_gpu.py run `cases()`; these tests compare that list with a direct reading of
tests/golden/econfigs_reference.json, so that no filter added later can shrink it unnoticed."""
import json

from tests import econfigs_cases as ec

CLASSES = {'BasicGCN', 'BasicGraphSage', 'BasicGAT', 'BasicLightGCN', 'BasicDGCF', 'BasicRS', 'HybridBertGCN', 'HybridBertGraphSage',
           'HybridBertGAT', 'HybridBertLightGCN', 'HybridBertDGCF', 'HybridCBRS'}


def _golden_sections():
    return [m for _, m, _ in ec.expanded_sections()]


def _values(sections, key):
    return {json.dumps(m[key]) for m in sections}


def _without_l2(m):
    return json.dumps({k: v for k, v in m.items() if k != 'l2_regularizer'}, sort_keys=True)


def test_the_list_covers_the_golden():
    sections = _golden_sections()
    cases = ec.cases()
    assert len(sections) >= 223 and len(cases) == 93
    assert cases == sorted(cases)
    ids = [cid for cid, _, _ in cases]
    assert len(set(ids)) == len(ids)
    assert all(cid == ec.case_id(m) and name == ec.class_name(m) for cid, name, m in cases)
    kept = [m for _, _, m in cases]
    assert {name for _, name, _ in cases} == CLASSES == {ec.class_name(m) for m in sections}
    for key in ec.COVERED_KEYS:
        assert _values(kept, key) == _values(sections, key), key
    # every (class, n_hiddens, n_layers) with every (dense_units, clf_units) it occurs with, every (feature_based, fusion_method,
    # residual) of every hybrid class — and, as nothing is thinned, every section itself
    assert {ec.architecture_key(m) for m in kept} == {ec.architecture_key(m) for m in sections}
    tweaks = lambda ms: {(ec.class_name(m), ec.tweak_key(m)) for m in ms if ec.is_hybrid(m)}
    assert tweaks(kept) == tweaks(sections)
    assert {_without_l2(m) for m in kept} == {_without_l2(m) for m in sections}
    # the first l2_regularizer seen (files in sorted order, experiments in file order) is the one kept for training
    first = {}
    for m in sections:
        first.setdefault(ec.case_id(m), m['l2_regularizer'])
    assert all(m['l2_regularizer'] == first[cid] for cid, _, m in cases)


def test_the_property_graph_and_the_route_representatives():
    cases = ec.cases()
    uip = ec.uip_case_ids()
    # every graph class occurs in a `*-uip-*` file; the classes on pre-computed rows do not
    assert {cid for cid, _, m in cases if ec.takes_graph(m)} <= uip
    assert not any(cid in uip for cid, _, m in cases if not ec.takes_graph(m))
    reps = ec.route_representatives()
    assert {ec.route_key(m) for _, _, m in reps} == {ec.route_key(m) for _, _, m in cases}
    assert {name for _, name, _ in reps} == set(ec.ROUTE_CLASSES) and {cid for cid, _, _ in reps} <= {cid for cid, _, _ in cases}
    assert len(reps) == 27

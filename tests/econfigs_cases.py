"""The architectures of the reference's experiment files as test cases (plain module, no device work).

tests/golden/econfigs_reference.json is expanded exactly as tests/test_econfigs_cpu.py expands it (`make_grid` + `nested_dict_update` on
`base`); model sections that differ only in `l2_regularizer` are one architecture (the first value seen, files in sorted order, is kept
for training).  `cases()` is every architecture: the GPU tests of tests/test_econfigs_gpu.py take a fraction of a second each on a graph
of 140 nodes, so nothing is thinned.  tests/test_econfigs_cases_cpu.py holds the list against a direct reading of the golden — every
class, every value of every key, every (class, widths) combination, every tweak of every hybrid class — so that a filter added later
cannot shrink it unnoticed.
"""
import copy
import json
import os

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'econfigs_reference.json')
TWEAKS = ('feature_based', 'fusion_method', 'residual')
COVERED_KEYS = ('n_hiddens', 'dense_units', 'clf_units') + TWEAKS


def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def expanded_sections():
    """[(file, model section, dataset load function)] of every experiment of every file, in file order then experiment order."""
    from deep_cbrs_amar_renaissance_amd.utilities.utils import make_grid, nested_dict_update
    g = golden()
    out = []
    for path in sorted(g['econfigs']):
        cfg = g['econfigs'][path]
        experiments = dict(cfg.get('linear') or {})
        for grid in (cfg.get('grid') or {}).values():
            experiments.update({str(e): e for e in make_grid(grid)})
        for overrides in experiments.values():
            config = nested_dict_update(copy.deepcopy(g['base']), overrides) if overrides else copy.deepcopy(g['base'])
            out.append((path, dict(config['model']), config['dataset']['load_function_name']))
    return out


def class_name(model_cfg):
    return model_cfg['name'].split('.')[1]


def is_hybrid(model_cfg):
    return class_name(model_cfg).startswith('Hybrid')


def takes_graph(model_cfg):
    """BasicRS / HybridCBRS score pre-computed embedding rows; every other class propagates over the graph it is given."""
    return class_name(model_cfg) not in ('BasicRS', 'HybridCBRS')


def _units(units):
    if units and isinstance(units[0], (list, tuple)):
        return '+'.join('x'.join(str(u) for u in net) for net in units)
    return 'x'.join(str(u) for u in units)


def case_id(model_cfg):
    """BasicGAT-d16-L3-dense128x64-clf64x32; hybrid heads add what differs from the plain head: -entity (feature_based off), -attention,
    -residual.  (BasicRS / HybridCBRS ignore the graph keys, which stay at the base file's values.)"""
    name = class_name(model_cfg)
    parts = [name]
    if takes_graph(model_cfg):
        parts += ['d{}'.format(model_cfg['n_hiddens'][0]), 'L{}'.format(model_cfg['n_layers'])]
    parts += ['dense' + _units(model_cfg['dense_units']), 'clf' + _units(model_cfg['clf_units'])]
    if is_hybrid(model_cfg):
        if not model_cfg['feature_based']:
            parts.append('entity')
        if model_cfg['fusion_method'] != 'concatenate':
            parts.append(model_cfg['fusion_method'])
        if model_cfg['residual']:
            parts.append('residual')
    return '-'.join(parts)


def _key(model_cfg):
    return json.dumps({k: v for k, v in model_cfg.items() if k != 'l2_regularizer'}, sort_keys=True)


def cases():
    """Every distinct model section of the golden without `l2_regularizer` in the key, as sorted [(case_id, class_name, model_cfg)];
    model_cfg carries the first l2_regularizer seen."""
    seen = {}
    for _, model_cfg, _ in expanded_sections():
        seen.setdefault(_key(model_cfg), model_cfg)
    out = sorted((case_id(m), class_name(m), m) for m in seen.values())
    assert len({c[0] for c in out}) == len(out), "case ids must tell the architectures apart"
    return out


def architecture_key(model_cfg):
    """The class with the widths of its graph stack and of its head."""
    return (class_name(model_cfg), json.dumps(model_cfg['n_hiddens']), model_cfg['n_layers'], json.dumps(model_cfg['dense_units']),
            json.dumps(model_cfg['clf_units']))


def tweak_key(model_cfg):
    return tuple(model_cfg[k] for k in TWEAKS)


def uip_case_ids():
    """Ids of the architectures that (also) occur in a `*-uip-*` file: those run on the graph with property nodes too."""
    return {case_id(m) for path, m, _ in expanded_sections() if '-uip-' in path}


ROUTE_CLASSES = ('BasicGCN', 'BasicLightGCN', 'BasicRS', 'HybridBertGCN', 'HybridCBRS')


def route_key(model_cfg):
    """What decides the launches of a model of one class: the graph width, the head's widths and, for a hybrid head, its tweaks."""
    width = model_cfg['n_hiddens'][0] if takes_graph(model_cfg) else None
    return (width, json.dumps(model_cfg['dense_units']), json.dumps(model_cfg['clf_units'])) + (tweak_key(model_cfg) if is_hybrid(model_cfg) else ())


def route_representatives():
    """The cases whose routes are pinned: for every distinct (n_hiddens width, dense_units, clf_units) of `cases()` — and every tweak
    setting of a hybrid head it is listed with — the GCN class (concatenated layer outputs: the widest tower input) and, for the Basic
    head, the LightGCN class too (mean of the layer outputs: the narrowest); BasicRS and HybridCBRS stand for themselves."""
    return sorted(c for c in cases() if c[1] in ROUTE_CLASSES)

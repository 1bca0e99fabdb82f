#!/usr/bin/env python
"""Golden data for tests/test_econfigs_cpu.py: the model hyperparameters of the reference's experiment files.

For the base `config.yaml` and every `econfigs/*.yaml` of the reference tree, keeps only what the test reads — the `model`
sections and `dataset.load_function_name`, under `grid:` / `linear:` as written — and writes them to
tests/golden/econfigs_reference.json.  The test expands the grids with the product's own logic and builds every model.

    python tests/golden/make_econfigs_golden.py REFERENCE_TREE      (CPU only)
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from deep_cbrs_amar_renaissance_amd.experiment import load_yaml      # noqa: E402  (the product's YAML 1.2 reading: 1e-4 is a float)


def _keep(section):
    """The parts of one experiment (or grid) the test reads."""
    out = {}
    if 'model' in (section or {}):
        out['model'] = section['model']
    if 'load_function_name' in (section or {}).get('dataset', {}):
        out['dataset'] = {'load_function_name': section['dataset']['load_function_name']}
    return out


def main(tree):
    base = load_yaml(os.path.join(tree, 'config.yaml'))
    out = {'base': _keep(base), 'econfigs': {}}
    for path in sorted(glob.glob(os.path.join(tree, 'econfigs', '*.yaml'))):
        doc = load_yaml(path) or {}
        out['econfigs'][os.path.basename(path)] = {
            kind: {name: _keep(section) for name, section in (doc.get(kind) or {}).items()} for kind in ('grid', 'linear') if doc.get(kind)}
    json.dump(out, open(os.path.join(HERE, 'econfigs_reference.json'), 'w'), indent=1)
    print('wrote econfigs_reference.json:', len(out['econfigs']), 'experiment files')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

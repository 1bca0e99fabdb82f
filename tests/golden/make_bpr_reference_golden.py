#!/usr/bin/env python
"""Golden vectors for BPR training's host side, produced by the REFERENCE'S OWN code, run in the build container.

    symmetrize_matrix            /root/reference/src/utilities/math.py:6-21
    build_adjacency_matrix       /root/reference/src/data/preprocess.py:44-170       (type_adjacency='binary')
    load_train_test_ratings      /root/reference/src/data/loaders.py:11-82
    UserItemGraphPosNegSample    /root/reference/src/data/datasets.py:216-306

As in make_graph_reference_golden.py, the modules import TensorFlow at their top and cannot be imported here; this script reads
them as text, takes exactly these definitions out of the syntax tree and executes THEM, unchanged, in a namespace holding numpy,
pandas, scipy.sparse, itertools (`it`) and a `utils` whose `Sequence` is `object` (the class's Keras base adds nothing it uses).
It writes two tiny rating files — one user rates an item positively twice (todok() sums the duplicate to 2: it is in neither list),
one user has no negative rating (its candidates are drawn once from the items it has not liked) —, builds the 'binary' adjacency
and the Sequence with seed 42, draws its first batches and stores inputs and outputs in tests/golden/bpr_reference.npz.

    python tests/golden/make_bpr_reference_golden.py      (needs /root/reference; CPU only)
"""
import ast
import itertools
import os
import tempfile
import types

import numpy as np
import pandas as pd
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'
WANTED = {'utilities/math.py': ['symmetrize_matrix'],
          'data/preprocess.py': ['build_adjacency_matrix'],
          'data/loaders.py': ['load_train_test_ratings'],
          'data/datasets.py': ['UserItemGraphPosNegSample']}
BATCH_SIZE, SEED, N_BATCHES = 18, 42, 6


def reference_namespace():
    ns = {'np': np, 'pd': pd, 'sparse': sparse, 'it': itertools, 'utils': types.SimpleNamespace(Sequence=object)}
    for rel, names in WANTED.items():
        path = os.path.join(REF, rel)
        tree = ast.parse(open(path).read(), filename=path)
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
                exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), ns)
    assert all(n in ns for names in WANTED.values() for n in names)
    return ns


def rating_rows(rng):
    """Raw (user, item, rating) rows: 12 users, 15 items, every user with >= 2 positives; user 0's first positive twice; user 3
    without a negative."""
    n_users, n_items = 12, 15
    raw_u = np.sort(rng.choice(200, n_users, replace=False))
    raw_i = np.sort(rng.choice(500, n_items, replace=False))
    rows = []
    for u in range(n_users):
        items = rng.choice(n_items, 7, replace=False)
        for k, i in enumerate(items):
            r = 1 if k < 3 else int(rng.random() < 0.5)
            if u == 3:
                r = 1
            rows.append((raw_u[u], raw_i[i], r))
    train = np.array(rows, dtype=np.int64)
    dup = train[0].copy()
    assert dup[2] == 1
    train = np.concatenate([train, dup[None]])                      # the duplicated positive
    train = train[rng.permutation(len(train))]
    test = train[rng.choice(len(train), 20, replace=False)].copy()
    return train, test


def main():
    ns = reference_namespace()
    rng = np.random.default_rng(20261016)
    train, test = rating_rows(rng)
    with tempfile.TemporaryDirectory() as d:
        paths = {k: os.path.join(d, k + '.tsv') for k in ('train', 'test')}
        for k, a in (('train', train), ('test', test)):
            np.savetxt(paths[k], a, fmt='%d', delimiter='\t')
        (tr, te), (users, items), adj = ns['load_train_test_ratings'](
            paths['train'], paths['test'], return_adjacency=True, type_adjacency='binary')
    adj = adj.tocoo()
    out = {'train_raw': train, 'test_raw': test, 'train_ratings': tr, 'users': users, 'items': items,
           'binary_row': adj.row.copy(), 'binary_col': adj.col.copy(), 'binary_data': adj.data.copy(),
           'binary_shape': np.array(adj.shape), 'batch_size': np.array(BATCH_SIZE), 'seed': np.array(SEED)}
    seq = ns['UserItemGraphPosNegSample'](tr, users, items, adj, batch_size=BATCH_SIZE, seed=SEED)
    pos = seq.adj_matrix
    out.update(pos_row=pos.row, pos_col=pos.col, pos_data=pos.data, n_batches_len=np.array(len(seq)))
    for name, k in (('pos', 0), ('neg', 1)):
        lists = [np.asarray(entry[k], dtype=np.int64) for entry in seq.user_item_dict]
        out[name + '_ptr'] = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
        out[name + '_ids'] = np.concatenate(lists)
    us, its, ys = [], [], []
    for b in range(N_BATCHES):
        (u, i), y = seq[b]
        us.append(u), its.append(i), ys.append(y)
    out.update(batch_users=np.stack(us), batch_items=np.stack(its), batch_ratings=np.stack(ys))
    # the no-negatives error: the same ratings with every 0 turned into 1
    no_neg = tr.copy()
    no_neg[:, 2] = 1
    try:
        ns['UserItemGraphPosNegSample'](no_neg, users, items, ns['build_adjacency_matrix'](no_neg, users, items, type_adjacency='binary'))
        out['no_negatives_error'] = np.array('')
    except ValueError as e:
        out['no_negatives_error'] = np.array(str(e))
    np.savez_compressed(os.path.join(HERE, 'bpr_reference.npz'), **out)
    print({k: getattr(v, 'shape', v) for k, v in out.items()})


if __name__ == '__main__':
    main()

"""The fit() runs whose results tests/golden/fit_bits.npz holds bit for bit: the cases, their Sequences and the run that
tools/record_fit_bits.py records and tests/test_fit_bits_gpu.py repeats.  tests/train_bits_cases.py pins the training step; this pins
what fit() puts around it, on each of its three ways to feed a batch (ids against the graph or resident tables, the Sequence's own
blocks, batches drawn on the device), replayed (AMAR_TRAIN_GRAPH unset) and eager (=0).

Every case is `model.fit(sequence, epochs=2, verbose=False)` on the 37 nodes of train_bits_cases.symmetric_graph() with its head,
narrowed to dense_units = clf_units = [8] so that the file stays below train_step_bits.npz's 165 KB.  257 ratings in batches of 48:
five full batches and a tail of 17, so every epoch has two graph keys and the tail runs eagerly in the first epoch and is captured
in the second.  Recorded per run: every trainable parameter as uint32, history['loss'] as the uint64 bits of its float64 values,
trainer.t, and for the replayed runs trainer.capture_count and the sorted `repr` of the keys of trainer._graphs — without the two
elements of a key that hold no decision of fit(): the address of the dropout step counter and the serial of the device sampler (a
counter of the process: it depends on how many samplers the tests before this one made)."""
import os

import numpy as np

from tests import train_bits_cases as tb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fit_bits.npz')
N_USERS, N_ITEMS, BATCH, N_RATINGS, EPOCHS = tb.N_USERS, tb.N_ITEMS, tb.BATCH, 5 * tb.BATCH + 17, 2
N_NODES = N_USERS + N_ITEMS
HEAD = dict(tb.HEAD, dense_units=[8], clf_units=[8])
HYBRID_HEAD = dict(dense_units=[[8], [8], [8]], clf_units=[8], feature_based=True)
BERT_DIM, TABLE_DIM = 12, 16
ENV = ('AMAR_TRAIN_GRAPH', 'AMAR_RESIDENT_ROWS', 'AMAR_RESIDENT_BERT')

# name: (model, Sequence, settings of ENV other than AMAR_TRAIN_GRAPH, the branch of fit() it trains in: HeadTrainer, graph model, sampled)
CASES = {
    'gcn_ids': ('BasicGCN', 'UserItemGraph', {}, 'graph'),
    'gcn_dropout': ('BasicGCN-dropout', 'UserItemGraph', {}, 'graph'),          # AMAR_TRAIN_GRAPH=0: the replayed body, run eagerly
    'hybrid_gcn_blocks': ('HybridBertGCN', 'UserItemGraphEmbeddings', {'AMAR_RESIDENT_BERT': '0'}, 'graph'),
    'hybrid_gcn_resident': ('HybridBertGCN', 'UserItemGraphEmbeddings', {}, 'graph'),
    'rs_resident': ('BasicRS', 'UserItemEmbeddings', {}, 'head'),
    'rs_blocks': ('BasicRS', 'UserItemEmbeddings', {'AMAR_RESIDENT_ROWS': '0'}, 'head'),
    'cbrs_resident': ('HybridCBRS', 'HybridUserItemEmbeddings', {}, 'head'),
    'gcn_bpr_sample': ('BasicGCN-bpr', 'UserItemGraphPosNegSample', {}, 'sampled'),
    'gcn_bpr_triplets': ('BasicGCN-bpr', 'UserItemGraphTriplets', {}, 'sampled'),
    'gcn_weighted_validated': ('BasicGCN', 'UserItemGraph-weighted', {}, 'graph'),
}
GRAPH_ENVS = ('1', '0')                                              # '1': AMAR_TRAIN_GRAPH unset


def ratings():
    """257 (user, item, label) rows over the 37 nodes; every user's first row is a positive, as the BPR Sequences need."""
    rng = np.random.default_rng(4)
    keys = rng.choice(N_USERS * N_ITEMS, size=N_RATINGS, replace=False)
    r = np.stack([keys // N_ITEMS, keys % N_ITEMS + N_USERS, (rng.random(N_RATINGS) < 0.6).astype(np.int64)], axis=1).astype(np.int64)
    first = np.unique(r[:, 0], return_index=True)[1]
    r[first, 2] = 1
    assert len(first) == N_USERS and (r[:, 2] == 0).any()
    return r


def build(name):
    """(model, Sequence, keyword arguments of fit()) of a case: seeded, compiled, biases away from zero where they exist yet."""
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.data import datasets
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    from deep_cbrs_amar_renaissance_amd.utilities.keras import EarlyStopping
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests import helpers
    model_name, seq_name = CASES[name][:2]
    r, users, items = ratings(), np.arange(N_USERS), np.arange(N_USERS, N_NODES)
    adj = tb.symmetric_graph()['adj']
    rng = np.random.default_rng(9)
    table = rng.standard_normal((N_NODES, TABLE_DIM)).astype(np.float32) * 0.5
    bert = rng.standard_normal((N_NODES, BERT_DIM)).astype(np.float32) * 0.5
    fit_args = {}
    if seq_name == 'UserItemGraph':
        seq = datasets.UserItemGraph(r, users, items, adj, batch_size=BATCH, shuffle=True, seed=5)
    elif seq_name == 'UserItemGraph-weighted':
        seq = datasets.UserItemGraph(r, users, items, adj, batch_size=BATCH, shuffle=True, seed=5,
                                     sample_weight=rng.uniform(0.5, 2.0, N_RATINGS).astype(np.float32))
        held = np.stack([rng.integers(0, N_USERS, 30), rng.integers(N_USERS, N_NODES, 30), rng.integers(0, 2, 30)], axis=1).astype(np.int64)
        fit_args = dict(class_weight={0: 1.0, 1: 3.0}, validation_data=datasets.UserItemGraph(held, users, items, adj, batch_size=BATCH),
                        callbacks=[EarlyStopping(monitor='val_loss', patience=10)], initial_epoch=1, epochs=EPOCHS + 1)
    elif seq_name == 'UserItemGraphEmbeddings':
        seq = datasets.UserItemGraphEmbeddings(r, users, items, adj, bert, batch_size=BATCH, shuffle=True, seed=5)
    elif seq_name == 'UserItemEmbeddings':
        seq = datasets.UserItemEmbeddings(r, users, items, table, batch_size=BATCH, shuffle=True, seed=5)
    elif seq_name == 'HybridUserItemEmbeddings':
        seq = datasets.HybridUserItemEmbeddings(r, users, items, table, bert, batch_size=BATCH, shuffle=True, seed=5)
    elif seq_name == 'UserItemGraphPosNegSample':
        seq = datasets.UserItemGraphPosNegSample(r, users, items, build_adjacency_matrix(r, users, items, type_adjacency='binary'),
                                                 batch_size=BATCH, seed=5)
        adj = seq.adj_matrix                                         # (the positives: the graph the model propagates over)
    else:
        seq = datasets.UserItemGraphTriplets(r, users, items, adj, batch_size=BATCH, seed=5)
    engine.set_seed(11)
    if model_name.startswith('BasicGCN'):
        model = basic.BasicGCN(adj, **dict(HEAD, **(dict(dropout=0.2) if model_name.endswith('dropout') else {})))
    elif model_name == 'HybridBertGCN':
        model = hybrid.HybridBertGCN(adj, embedding_dim=8, n_hiddens=[16, 8], l2_regularizer=1e-4, **HYBRID_HEAD)
    elif model_name == 'BasicRS':
        model = basic.BasicRS(dense_units=HEAD['dense_units'], clf_units=HEAD['clf_units'])
    else:
        model = hybrid.HybridCBRS(**HYBRID_HEAD)
    if not hasattr(model, 'gnn'):
        model(seq[0][0])                                             # builds the head's weights
    helpers.randomize_biases(model, seed=6)
    if model_name.endswith('bpr'):
        model.compile(loss=BPRLoss())
    return model, seq, fit_args


def graph_key(key, trainer):
    """`repr` of a key of trainer._graphs without the dropout counter's address and the sampler's serial (see the module docstring)."""
    key, at = list(key), 4 if key[0] == 'sampled' else 3             # where the trainer's dropout_key begins
    if trainer.dropout_key:
        del key[at + 1]
    if key[0] == 'sampled':
        del key[3]
    return repr(tuple(key))


def fit_bits(name, graph_env):
    """{array name: array} of the case under AMAR_TRAIN_GRAPH unset ('1') or '0': 'params' (the trainable parameters in the trainer's
    order as uint32, one after the other: an archive member each would cost more than their words) and their 'sizes', 'loss' (uint64),
    't', and for '1' also 'captures' and 'keys'."""
    import torch
    settings = dict(CASES[name][2], **({'AMAR_TRAIN_GRAPH': '0'} if graph_env == '0' else {}))
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(settings)
        model, seq, fit_args = build(name)
        history = model.fit(seq, **dict(dict(epochs=EPOCHS, verbose=False), **fit_args))
        torch.cuda.synchronize()
        trainer = model._trainer
        flat = [p.detach().cpu().contiguous().view(-1).numpy().view(np.uint32) for p in trainer.params]
        out = {'params': np.concatenate(flat), 'sizes': np.asarray([a.size for a in flat], dtype=np.int64)}
        out['loss'] = np.asarray(history['loss'], dtype=np.float64).view(np.uint64).copy()
        out['t'] = np.asarray([trainer.t], dtype=np.int64)
        if graph_env == '1':
            out['captures'] = np.asarray([trainer.capture_count], dtype=np.int64)
            out['keys'] = np.asarray(sorted(graph_key(k, trainer) for k in getattr(trainer, '_graphs', {})), dtype=np.str_)
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in a)

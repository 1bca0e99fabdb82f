"""The training steps whose parameters tests/golden/train_step_bits.npz holds bit for bit: the cases, their inputs and the run that
tools/record_train_bits.py records and tests/test_train_bits_gpu.py repeats.  Every shape is the smallest that still reaches its
path: 37 nodes (no multiple of the 4 rows of a block), one row without entries, one duplicated edge, two layers of different widths.
The file holds 34 609 words that do not compress (138 KB: twelve cases of 1 529 to 4 201 words, a head under 'concatenation' alone is
2 400; the three directed cases run on directed_ref.mixed(), whose 160 nodes make their node tables 1 280 words each instead of 296)
and 155 archive members: 165 KB in all."""
import os

import numpy as np
from scipy import sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_step_bits.npz')
N_USERS, N_ITEMS, BATCH, STEPS = 13, 24, 48, 2
HEAD = dict(embedding_dim=8, n_hiddens=[16, 8], n_layers=2, dense_units=[24], clf_units=[16], l2_regularizer=1e-4)
SWITCHES = ('AMAR_DENSE_BWD', 'AMAR_DENSE_STACK', 'AMAR_DENSE_STACK_BWD')

# name: (model class, graph, switches ('1' / '0' / None: as the process has them), constructor arguments)
CASES = {
    'gcn_concatenation_on': ('BasicGCN', 'symmetric', '1', {}),
    'gcn_concatenation_off': ('BasicGCN', 'symmetric', '0', {}),
    'gcn_stack_dropout': ('BasicGCN', 'symmetric', None, dict(dropout=0.2)),                 # the layer-by-layer forward
    'lightgcn_mean': ('BasicLightGCN', 'symmetric', None, {}),                               # the running-sum reverse
    'lightgcn_concatenation': ('BasicLightGCN', 'symmetric', None, dict(final_node='concatenation')),    # the `cat` reverse
    'dgcf_mean': ('BasicDGCF', 'symmetric', None, {}),
    'sage_mean_on': ('BasicGraphSage', 'symmetric', '1', dict(aggregate='mean')),
    'sage_mean_off': ('BasicGraphSage', 'symmetric', '0', dict(aggregate='mean')),
    'sage_max_directed': ('BasicGraphSage', 'directed', None, dict(aggregate='max')),
    'gat_dropout_directed_on': ('BasicGAT', 'directed', '1', dict(dropout_rate=0.2, dropout=0.2)),
    'gat_dropout_directed_off': ('BasicGAT', 'directed', '0', dict(dropout_rate=0.2, dropout=0.2)),
    'gcn_w_sum': ('BasicGCN', 'symmetric', None, dict(final_node='w-sum', n_hiddens=[8, 8])),            # ('w-sum' adds equal widths)
}
# (no case with a stack width above dense_bwd_supported's 128, which would take the separate kernels by shape: the GCN forward
# refuses a width of 132, amar_rowwise_xw_f32 has no kernel for it)
ROUTES = ('eager', 'captured')


def symmetric_graph():
    """13 users x 24 items, symmetric; the last item has no entry at all and the first edge is listed twice."""
    rng = np.random.default_rng(1)
    keys = rng.choice(N_USERS * (N_ITEMS - 1), size=90, replace=False)
    u, i = keys // (N_ITEMS - 1), keys % (N_ITEMS - 1) + N_USERS
    u, i = np.append(u, u[0]), np.append(i, i[0])
    n = N_USERS + N_ITEMS
    adj = sparse.coo_matrix((np.ones(2 * len(u), dtype=np.float32), (np.concatenate([u, i]), np.concatenate([i, u]))), shape=(n, n))
    m = sparse.csr_matrix(adj)
    assert (m != m.T).nnz == 0 and m[n - 1].nnz == 0 and m.max() == 2
    pairs = rng.integers(0, N_USERS * N_ITEMS, size=STEPS * BATCH)
    return {'adj': adj, 'u_ids': pairs // N_ITEMS, 'i_ids': pairs % N_ITEMS + N_USERS}


def graph(name):
    if name == 'symmetric':
        return symmetric_graph()
    from tests import directed_ref
    return directed_ref.mixed()


def build_model(name):
    """(model, batches) of a case: seeded, biases away from zero, STEPS batches of BATCH (user, item, label) rows."""
    import torch

    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.layers.reduction import ReductionLayer
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    cls, graph_name, _, extra = CASES[name]
    g = graph(graph_name)
    engine.set_seed(11)
    model = getattr(basic, cls)(g['adj'], **dict(HEAD, **extra))
    if cls == 'BasicLightGCN' and extra.get('final_node') == 'concatenation':
        # the model class reduces by 'mean' whatever it is given (the reference's own choice); the stack itself takes any reduction,
        # and under this one it keeps every layer's output, so its reverse pass walks the layers
        seq = model.gnn.gnn_layers
        seq.final_node, seq.reduce = 'concatenation', ReductionLayer('concatenation')
        model.rs = basic.BasicRS(HEAD['dense_units'], HEAD['clf_units'])       # a head for the wider table
        model.rs.build_head(seq.output_dim(), seq.output_dim())
    helpers.randomize_biases(model, seed=6)
    if cls == 'BasicDGCF':                                           # gates away from their all-ones start
        with torch.no_grad():
            for layer in model.gnn.gnn_layers.seq_layers:
                layer.w.add_(torch.from_numpy(np.random.default_rng(3).uniform(-0.5, 0.5, tuple(layer.w.shape)).astype(np.float32)).to(layer.w.device))
    labels = np.random.default_rng(2).integers(0, 2, STEPS * BATCH)
    batches = [(g['u_ids'][k * BATCH:(k + 1) * BATCH], g['i_ids'][k * BATCH:(k + 1) * BATCH], labels[k * BATCH:(k + 1) * BATCH])
               for k in range(STEPS)]
    return model, batches


def train_bits(name, route):
    """Every trainable parameter after STEPS steps of the case, as uint32 arrays in the Trainer's parameter order.  route 'eager':
    train_batch_graphed(graph=False) at every batch; 'captured': the first batch eagerly, the second captured and replayed."""
    import torch

    from deep_cbrs_amar_renaissance_amd import training
    switches = CASES[name][2]
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            if switches is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = switches
        model, batches = build_model(name)
        trainer = training.Trainer(model)
        for u, i, y in batches:
            trainer.train_batch_graphed(u, i, y, graph=route == 'captured')
        torch.cuda.synchronize()
        assert trainer.t == STEPS and (route == 'captured') == bool(trainer._graphs)
        return [p.detach().cpu().contiguous().view(-1).numpy().view(np.uint32).copy() for p in trainer.params]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

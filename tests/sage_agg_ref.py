"""Oracle for GraphSAGE's sum / max / min aggregators.  TEST INFRASTRUCTURE ONLY; imports oracle.*, never alters it.

(a) `aggregate_np` / `sage_conv_np`: numpy, written from the formulas of include/amar_hip.h with np.add.at / np.maximum.at /
    np.minimum.at over (entries + self loops).
(b) `torch_aggregate` / `torch_stack` / `torch_model_grads`: a torch-CPU restatement (float64 unless told otherwise) of a
    GraphSAGE stack and of a whole Basic* / HybridBert* loss, the aggregate by `scatter_reduce(include_self=False)`, whose
    autograd gives every tie and every duplicate entry an equal share (TensorFlow's _UnsortedSegmentMinOrMaxGrad rule).

Edge convention of oracle/layers.py: messages flow source = row -> target = col of the edge list.  A row without entries
aggregates to 0 under every aggregator (the stated deviation from tf.math.unsorted_segment_max).
tests/test_sage_aggregate_cpu.py pins both against oracle.layers.sage_conv and oracle.train.torch_model_grads for 'mean'.
"""
import numpy as np

from oracle import graph as ograph
from oracle.train import EPS

AGGREGATES = ('mean', 'sum', 'max', 'min')


def with_self_loops(row, col, n, self_loops):
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    return ograph.add_self_loops_edges(row, col, n) if self_loops else (row, col)


def aggregate_np(x, src, tgt, n, aggregate):
    """(agg [n, F], cnt [n, F]): cnt = entries per row for mean / sum, entries that attain the extremum for max / min."""
    msgs = x[src]
    deg = np.bincount(tgt, minlength=n).astype(x.dtype)
    if aggregate in ('mean', 'sum'):
        agg = np.zeros((n, x.shape[1]), dtype=x.dtype)
        np.add.at(agg, tgt, msgs)
        if aggregate == 'mean':
            agg = agg / np.maximum(deg, 1)[:, None]
        return agg, np.repeat(deg[:, None], x.shape[1], 1)
    fill = -np.inf if aggregate == 'max' else np.inf
    agg = np.full((n, x.shape[1]), fill, dtype=x.dtype)
    (np.maximum if aggregate == 'max' else np.minimum).at(agg, tgt, msgs)
    agg[deg == 0] = 0
    cnt = np.zeros((n, x.shape[1]), dtype=x.dtype)
    np.add.at(cnt, tgt, (msgs == agg[tgt]).astype(x.dtype))
    return agg, cnt


def sage_conv_np(x, row, col, kernel, bias, aggregate='mean', self_loops=True):
    """relu(l2_normalize([x || agg] . W + b)); the counterpart of oracle.layers.sage_conv for the four aggregators."""
    n = x.shape[0]
    src, tgt = with_self_loops(row, col, n, self_loops)
    agg, _ = aggregate_np(x, src, tgt, n, aggregate)
    out = np.concatenate([x, agg], axis=1) @ kernel + bias
    sq = np.sum(out * out, axis=1, keepdims=True)
    out = out * (1.0 / np.sqrt(np.maximum(sq, np.asarray(1e-12, dtype=x.dtype))))
    return np.maximum(out, 0).astype(x.dtype)


def torch_aggregate(x, src, tgt, n, aggregate):
    import torch
    if aggregate in ('mean', 'sum'):
        agg = torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add(0, tgt, x[src])
        if aggregate == 'mean':
            agg = agg / torch.bincount(tgt, minlength=n).to(x.dtype).clamp(min=1.0)[:, None]
        return agg
    # The untouched rows start as NaN, not 0: scatter_reduce's reverse pass counts `self == result` among the ties even with
    # include_self=False (torch 2.10), so a zero-filled start would take a share wherever an extremum is exactly 0 — every
    # ReLU tie.  NaN equals nothing; rows without entries are set to the stated 0 afterwards.
    index = tgt[:, None].expand(-1, x.shape[1])
    start = torch.full((n, x.shape[1]), float('nan'), dtype=x.dtype)
    agg = start.scatter_reduce(0, index, x[src], 'amax' if aggregate == 'max' else 'amin', include_self=False)
    has = torch.bincount(tgt, minlength=n) > 0
    return torch.where(has[:, None], agg, torch.zeros_like(agg))


def torch_stack(adj, x, st, aggregate, self_loops=True, selections=None):
    """One GraphSAGE stack in differentiable torch ops (oracle.train._torch_stack's 'sage' branch with the aggregate a parameter).
    selections: a list that receives, per layer, the boolean [entries, F] mask of the entries that attain the extremum."""
    import torch
    assert st['kind'] == 'sage'
    n = x.shape[0]
    row, col, _ = ograph.reordered_coo(adj)
    row, col = with_self_loops(row, col, n, self_loops)
    src, tgt = torch.as_tensor(row, dtype=torch.long), torch.as_tensor(col, dtype=torch.long)
    hs = [x]
    for lw in st['layers']:
        agg = torch_aggregate(x, src, tgt, n, aggregate)
        if selections is not None and aggregate in ('max', 'min'):
            selections.append((x[src] == agg[tgt]).detach().numpy())
        z = torch.cat([x, agg], 1) @ lw['kernel'] + lw['bias']
        z = z * torch.rsqrt(torch.clamp((z * z).sum(1, keepdim=True), min=1e-12))
        x = torch.relu(z)
        hs.append(x)
    final_node = st.get('final_node', 'concatenation')
    if final_node == 'concatenation':
        return torch.cat(hs, 1)
    if final_node == 'last':
        return hs[-1]
    if final_node == 'w-sum':
        w = st['reduction_w'].reshape(-1)
        return sum((w[k] * w[k]) * h for k, h in enumerate(hs))
    return sum(hs) / (len(hs) if final_node == 'mean' else 1)


def torch_model_grads(adj, gnn, head, u_ids, i_ids, y, aggregate='mean', l2=0.0, self_loops=True, bert=None, n_users=None,
                      n_items=None, dtype=np.float64, selections=None):
    """(loss, grads, scores) of a GraphSAGE model: stack(s) -> reduction -> head -> BCE (Keras backend form) + L2, gradients by
    autograd.  Layouts as oracle.train.torch_model_grads: one stack, TwoStep ({'step_one', 'step_two'}) or TwoWay; the Basic head
    (unet / inet / clf) or the Hybrid head with 'concatenate' fusions, feature based, no residual (dense1a .. dense3b, clf)."""
    import torch
    T = lambda arr: torch.tensor(np.asarray(arr, dtype=dtype), requires_grad=True)   # noqa: E731
    nets = {name: [(T(w), T(b)) for w, b in head[name]] for name in head}
    assert not any(name.startswith('fuse') or name == 'residual' for name in head)
    stacks = {}

    def leaf(name, w, table_l2):
        t = {'kind': w['kind'], 'final_node': w.get('final_node', 'concatenation'),
             'layers': [{k: T(v) for k, v in lw.items()} for lw in w['layers']], 'table_l2': table_l2}
        if 'embeddings' in w:
            t['embeddings'] = T(w['embeddings'])
        if t['final_node'] == 'w-sum':
            t['reduction_w'] = T(w['reduction_w'] if w.get('reduction_w') is not None else np.ones(len(w['layers']) + 1))
        stacks[name] = t
        return t
    run_stack = lambda a, x, st: torch_stack(a, x, st, aggregate, self_loops, selections)   # noqa: E731
    if 'step_one' in gnn:
        adj_ui, adj_kg = adj
        one, two = leaf('step_one', gnn['step_one'], True), leaf('step_two', gnn['step_two'], False)
        x = run_stack(adj_kg, one['embeddings'], one)
        e_all = run_stack(adj_ui, torch.cat([two['embeddings'], x[:n_items]], 0), two)
    elif 'way_one' in gnn:
        adj_ui, adj_ip, adj_up = adj
        one, two, three = leaf('way_one', gnn['way_one'], True), leaf('way_two', gnn['way_two'], True), leaf('step_two', gnn['step_two'], False)
        users = run_stack(adj_up, one['embeddings'], one)
        items = run_stack(adj_ip, two['embeddings'], two)
        e_all = run_stack(adj_ui, torch.cat([users[:n_users], items[:n_items]], 0), three)
    else:
        only = leaf('gnn', gnn, True)
        e_all = run_stack(adj, only['embeddings'], only)

    def run(net, v, last_sigmoid=False):
        for k, (w, b) in enumerate(net):
            v = v @ w + b
            v = torch.sigmoid(v) if (last_sigmoid and k == len(net) - 1) else torch.relu(v)
        return v
    u = torch.as_tensor(np.asarray(u_ids), dtype=torch.long)
    i = torch.as_tensor(np.asarray(i_ids), dtype=torch.long)
    if 'unet' in nets:
        p = run(nets['clf'], torch.cat([run(nets['unet'], e_all[u]), run(nets['inet'], e_all[i])], 1), True)[:, 0]
    else:
        ub, ib = torch.tensor(np.asarray(bert[0], dtype=dtype)), torch.tensor(np.asarray(bert[1], dtype=dtype))
        g1, g2, b1, b2 = run(nets['dense1a'], e_all[u]), run(nets['dense1b'], e_all[i]), run(nets['dense2a'], ub), run(nets['dense2b'], ib)
        x1, x2 = run(nets['dense3a'], torch.cat([g1, g2], 1)), run(nets['dense3b'], torch.cat([b1, b2], 1))
        p = run(nets['clf'], torch.cat([x1, x2], 1), True)[:, 0]
    yv = torch.tensor(np.asarray(y, dtype=dtype))
    pc = torch.clamp(p, EPS, 1 - EPS)
    loss = -torch.mean(yv * torch.log(pc + EPS) + (1 - yv) * torch.log(1 - pc + EPS))
    for st in stacks.values():
        if st['table_l2'] and 'embeddings' in st:
            loss = loss + l2 * (st['embeddings'] ** 2).sum()
        for lw in st['layers']:
            loss = loss + l2 * ((lw['kernel'] ** 2).sum() + (lw['bias'] ** 2).sum())
    loss.backward()
    g = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))   # noqa: E731

    def export(st):
        out = {'layers': [{k: g(v) for k, v in lw.items()} for lw in st['layers']]}
        if 'embeddings' in st:
            out['embeddings'] = g(st['embeddings'])
        if 'reduction_w' in st:
            out['reduction_w'] = g(st['reduction_w'])
        return out
    grads = {'gnn': export(stacks['gnn']) if 'gnn' in stacks else {name: export(st) for name, st in stacks.items()},
             'head': {name: [(g(w), g(b)) for w, b in nets[name]] for name in nets}}
    return float(loss.detach()), grads, p.detach().numpy()


def same_selection(adj, gnn, head, u_ids, i_ids, y, aggregate, **kwargs):
    """Whether the float32 and the float64 run of (b) select identical entry sets in every layer — the condition under which a
    float32 device run can be held against the float64 oracle at all.  Trivially true for mean / sum."""
    s32, s64 = [], []
    torch_model_grads(adj, gnn, head, u_ids, i_ids, y, aggregate, dtype=np.float32, selections=s32, **kwargs)
    torch_model_grads(adj, gnn, head, u_ids, i_ids, y, aggregate, dtype=np.float64, selections=s64, **kwargs)
    return len(s32) == len(s64) and all(np.array_equal(a, b) for a, b in zip(s32, s64))


def random_basic_weights(n, seed, embedding_dim=8, n_hiddens=(8, 8), dense_units=(24, 24), clf_units=(48, 48), final_node='concatenation'):
    """(gnn, head) of a BasicGraphSage in the oracle's layout, drawn from numpy alone so that a test's weights — and with them the
    entries its max / min select — can be reproduced without a device (helpers.load_oracle_weights puts them into the model)."""
    rng = np.random.default_rng(seed)
    widths = [embedding_dim] + list(n_hiddens)
    layers = [{'kernel': rng.uniform(-0.6, 0.6, (2 * f, c)).astype(np.float32), 'bias': rng.uniform(-0.1, 0.1, c).astype(np.float32)}
              for f, c in zip(widths[:-1], widths[1:])]
    gnn = {'kind': 'sage', 'final_node': final_node, 'embeddings': (rng.standard_normal((n, embedding_dim)) * 0.5).astype(np.float32),
           'layers': layers}
    d = sum(widths) if final_node == 'concatenation' else widths[-1]
    net = lambda dims: [(rng.uniform(-0.4, 0.4, (a, b)).astype(np.float32), rng.uniform(-0.05, 0.05, b).astype(np.float32))   # noqa: E731
                        for a, b in zip(dims[:-1], dims[1:])]
    head = {'unet': net([d] + list(dense_units)), 'inet': net([d] + list(dense_units)),
            'clf': net([2 * dense_units[-1]] + list(clf_units) + [1])}
    return gnn, head

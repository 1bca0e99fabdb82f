"""Oracle for GAT with several attention heads.  TEST INFRASTRUCTURE ONLY; imports oracle.*, never alters it.

(a) `gat_heads_conv_np`: numpy.  Spektral 1.x GATConv computes every head independently (`_call_single`) and joins them in `call`
    (concatenation or mean, then bias and activation), so the multi-head forward IS the oracle's single-head `oracle.layers.gat_conv`
    called once per head on that head's slices of the weights: pinned to the oracle by construction.
(b) `torch_gat_heads` / `torch_stack` / `torch_model_grads`: a torch-CPU restatement (float64 unless told otherwise) of one layer, a
    GAT stack and a whole Basic* / HybridBert* loss; gradients by autograd.

Weight layout (Keras): kernel [F, H, C], attn_self / attn_neigh [C, H, 1], bias [H*C] (concat_heads) or [C] (mean).
Edge convention of oracle/layers.py: messages flow source = row -> target = col of the edge list.
tests/test_gat_heads_cpu.py pins (a) against (b), and both against oracle.layers.gat_conv at H = 1.
"""
import numpy as np

from oracle import graph as ograph
from oracle import layers as ol
from oracle.train import EPS


def gat_heads_conv_np(x, row, col, kernel, attn_self, attn_neigh, bias, concat=True, self_loops=True):
    """relu(join_h(out_h) + bias) with out_h = oracle.layers.gat_conv of head h without bias and activation."""
    heads, c = kernel.shape[1], kernel.shape[2]
    zero = np.zeros(c, dtype=x.dtype)
    outs = [ol.gat_conv(x, row, col, kernel[:, h, :], attn_self[:, h, 0], attn_neigh[:, h, 0], zero, activation=None, self_loops=self_loops)[0]
            for h in range(heads)]
    out = np.concatenate(outs, axis=1) if concat else sum(outs[1:], outs[0]) / heads
    return np.maximum(out + bias, 0).astype(x.dtype)


def edges(row, col, n, self_loops=True):
    """(src, tgt) index tensors of an edge list, with Spektral's self loops appended."""
    import torch
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    if self_loops:
        row, col = ograph.add_self_loops_edges(row, col, n)
    return torch.as_tensor(row, dtype=torch.long), torch.as_tensor(col, dtype=torch.long)


def torch_gat_heads(hd, attn_self, attn_neigh, bias, src, tgt, concat=True, keep=None, scalars=None):
    """One layer from its projection on: hd [n, H, C] (any leading view of [n, H*C]), attn_* [C, H, 1].  Returns the activation
    [n, H*C] or [n, C].  keep: a dict that receives the attention scalars 's' and 't' [n, H] with their gradients retained.
    scalars: (s, t) [n, H] taken as given leaves in place of hd . attn_* (the entry points take S as an input of its own)."""
    import torch
    n, heads, c = hd.shape
    if scalars is None:
        s = torch.einsum('nhc,ch->nh', hd, attn_self[:, :, 0])
        t = torch.einsum('nhc,ch->nh', hd, attn_neigh[:, :, 0])
    else:
        s, t = scalars
    if keep is not None and scalars is not None:
        keep['s'], keep['t'] = s, t
    elif keep is not None:
        s.retain_grad(), t.retain_grad()
        keep['s'], keep['t'] = s, t
    e = s[tgt] + t[src]                                              # [E, H]
    e = torch.where(e > 0, e, 0.2 * e)
    index = tgt[:, None].expand(-1, heads)
    seg_max = torch.full((n, heads), -float('inf'), dtype=hd.dtype).scatter_reduce(0, index, e.detach(), 'amax')
    ex = torch.exp(e - seg_max[tgt])
    denom = torch.zeros((n, heads), dtype=hd.dtype).index_add(0, tgt, ex) + 1e-9
    alpha = ex / denom[tgt]
    out = torch.zeros_like(hd).index_add(0, tgt, alpha[:, :, None] * hd[src])      # [n, H, C]
    out = out.reshape(n, heads * c) if concat else out.mean(1)
    return torch.relu(out + bias)


def torch_stack(adj, x, st, self_loops=True):
    """One GAT stack in differentiable torch ops; st = {'layers': [{'kernel', 'attn_self', 'attn_neigh', 'bias'}], 'concat_heads',
    'final_node'[, 'reduction_w']}."""
    import torch
    assert st['kind'] == 'gat'
    n = x.shape[0]
    row, col, _ = ograph.reordered_coo(adj)
    src, tgt = edges(row, col, n, self_loops)
    hs = [x]
    for lw in st['layers']:
        f, heads, c = lw['kernel'].shape
        hd = (x @ lw['kernel'].reshape(f, heads * c)).reshape(n, heads, c)
        x = torch_gat_heads(hd, lw['attn_self'], lw['attn_neigh'], lw['bias'], src, tgt, st['concat_heads'])
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


def torch_model_grads(adj, gnn, head, u_ids, i_ids, y, l2=0.0, self_loops=True, bert=None, n_users=None, n_items=None, dtype=np.float64):
    """(loss, grads, scores) of a multi-head GAT model: stack(s) -> reduction -> head -> BCE (Keras backend form) + L2 on the node
    table, the kernels and the biases (the attention kernels carry no regulariser), gradients by autograd.  Layouts as
    oracle.train.torch_model_grads: one stack or TwoStep ({'step_one', 'step_two'}); the Basic head (unet / inet / clf) or the
    Hybrid head with 'concatenate' fusions, feature based, no residual (dense1a .. dense3b, clf)."""
    import torch
    T = lambda arr: torch.tensor(np.asarray(arr, dtype=dtype), requires_grad=True)   # noqa: E731
    nets = {name: [(T(w), T(b)) for w, b in head[name]] for name in head}
    assert not any(name.startswith('fuse') or name == 'residual' for name in head)
    stacks = {}

    def leaf(name, w, table_l2):
        t = {'kind': w['kind'], 'final_node': w.get('final_node', 'concatenation'), 'concat_heads': w['concat_heads'],
             'layers': [{k: T(v) for k, v in lw.items()} for lw in w['layers']], 'table_l2': table_l2}
        if 'embeddings' in w:
            t['embeddings'] = T(w['embeddings'])
        stacks[name] = t
        return t
    if 'step_one' in gnn:
        adj_ui, adj_kg = adj
        one, two = leaf('step_one', gnn['step_one'], True), leaf('step_two', gnn['step_two'], False)
        x = torch_stack(adj_kg, one['embeddings'], one, self_loops)
        e_all = torch_stack(adj_ui, torch.cat([two['embeddings'], x[:n_items]], 0), two, self_loops)
    else:
        only = leaf('gnn', gnn, True)
        e_all = torch_stack(adj, only['embeddings'], only, self_loops)

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
        return out
    grads = {'gnn': export(stacks['gnn']) if 'gnn' in stacks else {name: export(st) for name, st in stacks.items()},
             'head': {name: [(g(w), g(b)) for w, b in nets[name]] for name in nets}}
    return float(loss.detach()), grads, p.detach().numpy()


# ---- product model -> the layout above -------------------------------------------------------------------------------------------
def _np(p):
    return p.detach().cpu().numpy().copy()


def seq_to_ref(seq):
    """One SequentialGNN / HalfInputSequentialGNN stack of GATConv layers -> weight dict (Keras shapes kept)."""
    layers = [{'kernel': _np(l.kernel), 'attn_self': _np(l.attn_kernel_self), 'attn_neigh': _np(l.attn_kernel_neighs), 'bias': _np(l.bias)}
              for l in seq.seq_layers]
    out = {'kind': 'gat', 'layers': layers, 'final_node': seq.final_node, 'concat_heads': bool(seq.seq_layers[0].concat_heads)}
    if getattr(seq, 'embeddings', None) is not None:
        out['embeddings'] = _np(seq.embeddings)
    return out


def gnn_to_ref(gnn):
    if hasattr(gnn, 'step_one_gnn_layers'):
        return {'step_one': seq_to_ref(gnn.step_one_gnn_layers), 'step_two': seq_to_ref(gnn.step_two_gnn_layers)}
    return seq_to_ref(gnn.gnn_layers)


def flatten_grads(model, grads):
    """Reference gradient containers -> {product parameter: ndarray}."""
    names = {'attn_self': 'attn_kernel_self', 'attn_neigh': 'attn_kernel_neighs'}
    out = {}
    if 'layers' in grads['gnn']:
        pairs = [(model.gnn.gnn_layers, grads['gnn'])]
    else:
        pairs = [(getattr(model.gnn, name + '_gnn_layers'), gs) for name, gs in grads['gnn'].items()]
    for seq, gs in pairs:
        if 'embeddings' in gs:
            out[seq.embeddings] = gs['embeddings']
        for layer, gl in zip(seq.seq_layers, gs['layers']):
            for name, arr in gl.items():
                out[getattr(layer, names.get(name, name))] = arr
    for name in grads['head']:
        for layer, (gw, gb) in zip(getattr(model.rs, name).layers, grads['head'][name]):
            out[layer.kernel], out[layer.bias] = gw, gb
    return out

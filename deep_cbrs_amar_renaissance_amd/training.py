"""Training step for the Basic GNN recommenders — what ``model.fit`` runs per batch.

Mirrors what Keras does under `Experimenter.train` (`/root/reference/src/experiment.py:155-188`):
binary cross-entropy (`config.yaml:58`) on the sigmoid scores of `BasicGNN.call` (full-graph
propagation re-run for EVERY batch, `basic.py:61-63`), plus the L2 regularisers carried by the
node table and the GCN kernels/biases (`gnn.py:45, 293-294`), differentiated and applied with
Adam (`config.yaml:52-56`; Keras defaults beta_2 = 0.999, epsilon = 1e-7).

Forward activations come from the same HIP kernels as inference; the reverse pass uses the
training kernels of `csrc/amar_train.hip` (activation backward, two-stage deterministic weight
gradients, row scatter-add for the embedding lookup, Adam) and reuses the forward SpMM, on the transposed image of the
graph (`DeviceCSR.transposed()`: the matrix itself where it is symmetric, `dataset.symmetric_adjacency: True`; else the stable
device transpose), for A_hat^T . dZ, and the forward GEMM for dX = dZ . W^T.

Implemented for GCN, GraphSAGE, GAT, LightGCN and DGCF stacks under every reduction ('concatenation', 'mean', 'sum',
'w-sum', 'last'), alone (models/gnn.py) or chained as TwoStep / TwoWay models (models/tsgnn.py, twgnn.py): `_StackTape` is the
forward-with-kept-activations + reverse pass of ONE stack, and the Trainer chains the tapes the way the model chains the
stacks (the gradient of a stack's leading rows is lifted back to its full node table).  A layer type's forward and reverse sit side by side
in its `_LayerKind`; every reverse of a linear map, the Dense tapes' included, is `_LinearReverse.linear_bwd`.  GraphSAGE trains on an unfused
forward that keeps what the reverse pass needs ([x || mean] and the normalised pre-activation); its aggregate is
(A + I) / count, so the reverse aggregate is the row scale (A's counts) followed by the value-free SpMM on A^T.  The hybrid head
(HybridCBRS: 'concatenate' / 'attention' fusion, residual classifier, both feature_based settings) trains on the same
Dense tapes; its BERT inputs are constants.  GAT (1 head; several heads: `amar_gat_heads_bwd_f32`) trains on the inference kernels plus `amar_gat_bwd_f32`, which
forms the softmax / attention-scalar gradients row-wise for both edge directions (targets on A's rows, sources on A^T's rows:
`amar_gat_bwd_directed_f32` where the two differ; no float atomics).
"""
import itertools
import os
import types

import numpy as np
import torch

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd.engine import ids_to_device, stage_ids, to_device_tensor
from deep_cbrs_amar_renaissance_amd.layers.dgcf_conv import DGCFConv
from deep_cbrs_amar_renaissance_amd.layers.gat_conv import GATConv
from deep_cbrs_amar_renaissance_amd.layers.gcn_conv import GCNConv
from deep_cbrs_amar_renaissance_amd.layers.graphsage_conv import GraphSageConv
from deep_cbrs_amar_renaissance_amd.layers.lightgcn_conv import LightGCNConv
from deep_cbrs_amar_renaissance_amd.utilities.losses import BPR, GROUP_KINDS, LOSS_NAMES, loss_kind, resolve_class_weight, resolve_loss
from deep_cbrs_amar_renaissance_amd.utilities.math import spmm_kind
from deep_cbrs_amar_renaissance_amd.utilities.metrics import metric_values, resolve_compiled
from deep_cbrs_amar_renaissance_amd.utilities.schedules import InverseTimeDecay, LearningRateSchedule, resolve as resolve_learning_rate

_NEEDS_TRIPLETS = ("{} groups each positive with the negatives drawn for the same user: it trains on the triplet Sequence of "
                   "load_user_item_graph_triplets (data/datasets.py:UserItemGraphTriplets) only")


def _spmm(a, x, out):
    """out = A_hat . x with whichever image of A_hat the forward pass uses for this width."""
    kind = spmm_kind(a, x.shape[1])
    if kind == 'xs':
        capi.spmm_xs(a.tiled_image(x.shape[1]), x, out)
    elif kind == 'sj':
        capi.spmm_sj(a.sliced(x.shape[1]), x, out)
    else:
        capi.spmm_csr(a.rowptr, a.colidx, a.vals, x, out)
    return out


def _buffer(like, rows, cols=None):
    return torch.empty(rows if cols is None else (rows, cols), dtype=torch.float32, device=like.device)


class _LinearReverse:
    """The reverse pass of a linear map Z = X . W (+ b) for the tapes: the workspaces of amar_dense_bwd_f32, the choice between that
    kernel and the separate ones, and `defer_reduce` (set by Trainer._graph_body for a captured step: the partial sums of dW / db stay in
    the workspace and the batch's ONE Adam launch adds them, see capi.DeferredGradient)."""

    def __init__(self):
        self._workspaces = {}
        self.defer_reduce = False

    def _workspace(self, key, m, kk, n, device):
        """Allocated at the first batch of a shape — an eager one — and reused by every later batch, captured ones included."""
        key = (key, int(m), int(kk), int(n))
        if key not in self._workspaces:
            self._workspaces[key] = capi.dense_bwd_workspace(m, kk, n, device)
        return self._workspaces[key]

    @staticmethod
    def fused_route(K, N, rows):
        """amar_dense_bwd_f32 (act', dX, dW, db in two launches) or the separate kernels.  A layer whose reverse is several linear_bwd calls asks
        once with its own (f, c) and passes `fused=`: its K = 1 bias and attention-vector calls must go the layer's way, not that of (1, c)."""
        return capi.dense_bwd_enabled() and capi.dense_bwd_supported(K, N) and rows > 0

    def linear_bwd(self, key, dy, *, x=None, w=None, y=None, act=None, dX=None, dZ=None, dw_like=None, db_like=None,
                   accumulate_dx=False, K=None, fused=None, column_x=False):
        """Reverse of Z = x . w (+ b), Y = act(Z), given dy = d(loss)/dY [M, N] (y None: dy already is dZ).  Returns (dW, db, dX), each
        ready for `grads` (a tensor shaped like dw_like / db_like, or what a captured step defers) or None where not asked for: dW takes
        x and dw_like, db takes db_like, dX takes w (into dX where given, else a fresh buffer; accumulate_dx: added to dX).  dZ: where to
        leave dZ itself.  key names the fused route's workspace, K its K where neither x nor w tells.  column_x: x is one column and
        dw_like holds the N values of x^T . dy, which the separate kernels form as the [N, 1] product dy^T . x."""
        m, n = dy.shape
        kk = w.shape[0] if w is not None else (x.shape[1] if x is not None else int(K or 1))
        dw, db = (torch.empty_like(p) if p is not None else None for p in (dw_like, db_like))
        if w is not None and dX is None:
            dX = _buffer(dy, m, kk)
        if self.fused_route(kk, n, m) if fused is None else fused:
            act = act if y is not None else None
            lazy = capi.dense_bwd(x, y if act is not None else None, dy, w, act, self._workspace(key, m, kk, n, dy.device), dX=dX,
                                  dW=dw.view(kk, n) if dw is not None else None, db=db, defer=self.defer_reduce, dZ=dZ, accumulate_dx=accumulate_dx, K=K)
            return (dw, db, dX) if lazy is None else (*lazy, dX)
        dz = dy
        if y is not None:
            dz = dZ if dZ is not None else torch.empty_like(y)
            capi.act_bwd(dy, y, dz, act)
        if column_x:
            capi.wgrad(dz, x, dw.view(n, 1), None)
        elif dw is not None or db is not None:
            capi.wgrad(x if dw is not None else None, dz, dw.view(kk, n) if dw is not None else None, db)
        if w is not None:
            back = _buffer(dy, m, kk) if accumulate_dx else dX
            capi.dense(dz, w, None, back, act=None, w_transposed=True)
            if accumulate_dx:
                capi.add_inplace(dX, back)
        return dw, db, dX


class _DenseTape(_LinearReverse):
    """Forward of a Dense stack that keeps every layer's input and output, and its reverse pass."""

    def __init__(self, stack):
        super().__init__()
        self.layers = list(stack.layers)
        self.inputs, self.outputs = [], []

    def _stack_spec(self, x, ids, out_last):
        """The arguments of the one-launch forward (capi.dense_stack) for this call, or None where the stack runs layer by layer."""
        m = int(ids.numel()) if ids is not None else int(x.shape[0])
        dims = [int(self.layers[0].kernel.shape[0])] + [int(l.units) for l in self.layers]
        if not (capi.dense_stack_enabled() and capi.dense_stack_supported(dims) and m > 0):
            return None
        dev = x.device
        outs = [torch.empty((m, l.units), dtype=torch.float32, device=dev) for l in self.layers]
        if out_last is not None:
            outs[-1] = out_last
        xin = torch.empty((m, dims[0]), dtype=torch.float32, device=dev) if ids is not None else None
        return dict(X=x, weights=[l.kernel.detach() for l in self.layers], biases=[l.bias.detach() for l in self.layers],
                    acts=[l.activation for l in self.layers], outs=outs, ids=ids, xcopy=xin)

    def _stack_done(self, spec):
        outs = spec['outs']
        self.inputs, self.outputs = [spec['xcopy'] if spec['ids'] is not None else spec['X']] + outs[:-1], outs
        return outs[-1]

    @staticmethod
    def forward_pair(first, first_args, second, second_args):
        """Two independent stacks (the user and the item tower) in ONE launch where both take the one-launch forward
        (capi.dense_stack_pair).  *_args = (x, ids, out_last)."""
        s0, s1 = first._stack_spec(*first_args), second._stack_spec(*second_args)
        if s0 is not None and s1 is not None:
            capi.dense_stack_pair(s0, s1)
            return first._stack_done(s0), second._stack_done(s1)
        return first.forward(*first_args), second.forward(*second_args)

    def forward(self, x, ids=None, out_last=None):
        """y = stack(x[ids]) keeping every layer's input and output.  ids: gather the input rows first; out_last: where the last
        layer's output goes (a column slice of a concatenation buffer).  Stacks of at most four layers no wider than 128 run as ONE
        launch (amar_dense_stack_f32, round 4: gather, layers and the concat store together); others layer by layer."""
        spec = self._stack_spec(x, ids, out_last)
        if spec is not None:
            capi.dense_stack(**spec)
            return self._stack_done(spec)
        m = int(ids.numel()) if ids is not None else int(x.shape[0])
        dev = x.device
        dims = [int(self.layers[0].kernel.shape[0])] + [int(l.units) for l in self.layers]
        outs = [torch.empty((m, l.units), dtype=torch.float32, device=dev) for l in self.layers]
        if out_last is not None:
            outs[-1] = out_last
        if ids is not None:
            gathered = torch.empty((m, dims[0]), dtype=torch.float32, device=dev)
            capi.copy_columns(x, gathered, ids=ids)
            x = gathered
        self.inputs, self.outputs = [], []
        for layer, y in zip(self.layers, outs):
            capi.dense(x, layer.kernel, layer.bias, y, act=layer.activation)
            self.inputs.append(x)
            self.outputs.append(y)
            x = y
        return x

    def _stack_bwd_spec(self, dy, last_is_dz, need_input_grad, dx_out):
        """The arguments of the one-launch reverse pass (capi.dense_stack_bwd) for this call, or None where it runs layer by layer."""
        m = int(dy.shape[0])
        dims = [int(self.layers[0].kernel.shape[0])] + [int(l.units) for l in self.layers]
        if not (capi.dense_bwd_enabled() and capi.dense_stack_bwd_supported(dims, m)):
            return None
        dev = dy.device
        key = ('stack', m)
        if key not in self._workspaces:
            self._workspaces[key] = capi.dense_stack_bwd_workspace(m, dims, dev)
        dws = [torch.empty_like(l.kernel) for l in self.layers]
        dbs = [torch.empty_like(l.bias) for l in self.layers]
        dx0 = (dx_out if dx_out is not None else torch.empty((m, dims[0]), dtype=torch.float32, device=dev)) if need_input_grad else None
        return dict(dYtop=dy, Ytop=None if last_is_dz else self.outputs[-1], inputs=self.inputs, weights=[l.kernel.detach() for l in self.layers],
                    acts=[l.activation for l in self.layers], workspace=self._workspaces[key], dWs=dws, dbs=dbs, dX0=dx0, defer=self.defer_reduce)

    def _stack_bwd_done(self, spec, lazy, grads):
        for k, layer in enumerate(self.layers):
            grads[layer.kernel], grads[layer.bias] = lazy[k] if lazy is not None else (spec['dWs'][k], spec['dbs'][k])
        return spec['dX0']

    @staticmethod
    def backward_pair(first, dy_first, second, dy_second, grads, need_input_grad=True, dx_out=(None, None)):
        """The reverse passes of two independent stacks in ONE launch where both take the one-launch form (capi.dense_stack_bwd_pair)."""
        s0 = first._stack_bwd_spec(dy_first, False, need_input_grad, dx_out[0])
        s1 = second._stack_bwd_spec(dy_second, False, need_input_grad, dx_out[1])
        if s0 is not None and s1 is not None:
            lazy0, lazy1 = capi.dense_stack_bwd_pair(s0, s1)
            return first._stack_bwd_done(s0, lazy0, grads), second._stack_bwd_done(s1, lazy1, grads)
        return (first.backward(dy_first, grads, need_input_grad=need_input_grad, dx_out=dx_out[0]),
                second.backward(dy_second, grads, need_input_grad=need_input_grad, dx_out=dx_out[1]))

    def backward(self, dy, grads, last_is_dz=False, need_input_grad=True, dx_out=None):
        """dy: gradient w.r.t. the stack's output (or, with last_is_dz, already w.r.t. the last pre-activation).
        Fills grads[param] for every kernel/bias; returns the gradient w.r.t. the stack's input (None when
        need_input_grad is False: constant inputs such as the BERT rows)."""
        spec = self._stack_bwd_spec(dy, last_is_dz, need_input_grad, dx_out)
        if spec is not None:
            # the whole stack's reverse pass in ONE launch (amar_dense_stack_bwd_f32): dZ walks the layers in LDS
            return self._stack_bwd_done(spec, capi.dense_stack_bwd(**spec), grads)
        last = len(self.layers) - 1
        for k in range(last, -1, -1):
            layer = self.layers[k]
            need_dx = k > 0 or need_input_grad
            grads[layer.kernel], grads[layer.bias], dy = self.linear_bwd(
                k, dy, x=self.inputs[k], w=layer.kernel.detach() if need_dx else None, y=None if (last_is_dz and k == last) else self.outputs[k],
                act=layer.activation, dX=dx_out if (k == 0 and need_dx) else None, dw_like=layer.kernel, db_like=layer.bias)
        return dy


def _concat(a, b):
    out = torch.empty((a.shape[0], a.shape[1] + b.shape[1]), dtype=torch.float32, device=a.device)
    capi.copy_columns(a, out[:, :a.shape[1]])
    capi.copy_columns(b, out[:, a.shape[1]:])
    return out


class _BasicHead:
    """BasicRS (basic.py:11-37) with saved activations: towers on E[u], E[i]; classifier on their concatenation."""

    def __init__(self, rs):
        self.unet, self.inet, self.clf = _DenseTape(rs.unet), _DenseTape(rs.inet), _DenseTape(rs.clf)

    def forward(self, gu, gi, bert, ids=None):
        """ids = (u, i): gu and gi are node tables and the towers gather their rows themselves; the towers' last layers store straight
        into the two halves of the classifier's input (no concat copies)."""
        d = int(self.unet.layers[-1].units)
        b = int(ids[0].numel()) if ids is not None else int(gu.shape[0])
        cat = torch.empty((b, 2 * d), dtype=torch.float32, device=gu.device)
        _DenseTape.forward_pair(self.unet, (gu, ids[0] if ids is not None else None, cat[:, :d]),
                                self.inet, (gi, ids[1] if ids is not None else None, cat[:, d:]))      # (both towers: one launch)
        self.d = d
        return self.clf.forward(cat)

    def backward(self, dz, grads, need_input_grad=True, dx_out=(None, None)):
        """dz = dL/d(last pre-activation). Returns (dL/dE[u], dL/dE[i]) (None, None when the inputs are constants); dx_out: where to."""
        dcat = self.clf.backward(dz, grads, last_is_dz=True)
        return _DenseTape.backward_pair(self.unet, dcat[:, :self.d], self.inet, dcat[:, self.d:], grads, need_input_grad=need_input_grad, dx_out=dx_out)


class _FusionTape:
    """FusionLayer (fusion.py:5-68) with saved operands: concatenation, or the attention mix with its two weights."""

    def __init__(self, fuse):
        self.fuse = fuse

    def plan_joined(self, rows, wa, wb, device):
        """For a concatenating fusion: (buffer, left half, right half) for the producers of its operands to store into, else
        (None, None, None) — round 4: the two column copies of every `Concatenate` of a hybrid head were 6 of a batch's 54 launches."""
        if self.fuse.method != 'concatenate':
            return None, None, None
        buf = torch.empty((rows, wa + wb), dtype=torch.float32, device=device)
        return buf, buf[:, :wa], buf[:, wa:]

    def forward(self, a, b, joined=None):
        """joined: the [rows, da + db] buffer whose two column halves a and b ALREADY are (their producers stored straight into
        it: `plan_joined`) — a concatenation then has nothing to copy."""
        f = self.fuse
        self.da, self.db = a.shape[1], b.shape[1]
        if f.method == 'concatenate':
            return joined if joined is not None else _concat(a, b)
        pa, pb = f.project(a, b)
        ta, tb = torch.empty_like(pa), torch.empty_like(pb)
        capi.dense(pa, f.att_weight, None, ta, act=None)
        capi.dense(pb, f.att_weight, None, tb, act=None)
        out = torch.empty_like(pa)
        capi.attention_mix(pa, pb, ta, tb, out)
        self.saved = (a, b, pa, pb, ta, tb)
        return out

    def backward(self, dout, grads):
        """Returns (dL/da, dL/db); fills grads for att_weight / proj_weight."""
        f = self.fuse
        if f.method == 'concatenate':
            return dout[:, :self.da], dout[:, self.da:]
        a, b, pa, pb, ta, tb = self.saved
        d_a, d_b, d_ta, d_tb = capi.attention_mix_bwd(dout, pa, pb, ta, tb)
        w = f.att_weight.detach()
        dw, dw2 = torch.empty_like(w), torch.empty_like(w)
        capi.wgrad(pa, d_ta, dw, None)
        capi.wgrad(pb, d_tb, dw2, None)
        capi.add_inplace(dw, dw2)
        grads[f.att_weight] = dw
        back = torch.empty_like(d_a)
        capi.dense(d_ta, w, None, back, act=None, w_transposed=True)
        capi.add_inplace(d_a, back)
        capi.dense(d_tb, w, None, back, act=None, w_transposed=True)
        capi.add_inplace(d_b, back)
        if f.proj_first is not None:                                 # the narrower block went through proj_weight first
            src, d_proj = (a, d_a) if f.proj_first else (b, d_b)
            dp = torch.empty_like(f.proj_weight)
            capi.wgrad(src, d_proj, dp, None)
            grads[f.proj_weight] = dp
            d_src = torch.empty((src.shape[0], src.shape[1]), dtype=torch.float32, device=src.device)
            capi.dense(d_proj, f.proj_weight.detach(), None, d_src, act=None, w_transposed=True)
            if f.proj_first:
                d_a = d_src
            else:
                d_b = d_src
        return d_a, d_b


class _HybridHead:
    """HybridCBRS (hybrid.py:13-89) with saved activations: both feature_based settings, 'concatenate' / 'attention'
    fusion, optional residual classifier.  The BERT rows are constants."""

    def __init__(self, rs):
        self.rs = rs
        self.fb = bool(rs.feature_based)
        names = ['dense1a', 'dense1b', 'dense2a', 'dense2b', 'dense3a', 'dense3b', 'clf'] + (['residual'] if rs.residual is not None else [])
        self.t = {name: _DenseTape(getattr(rs, name)) for name in names}
        self.f1a, self.f1b, self.f2 = _FusionTape(rs.fuse1a), _FusionTape(rs.fuse1b), _FusionTape(rs.fuse2)

    def forward(self, gu, gi, bert):
        ub, ib = bert
        t = self.t
        rows, dev = int(gu.shape[0]), gu.device
        w = {name: int(t[name].layers[-1].units) for name in ('dense1a', 'dense1b', 'dense2a', 'dense2b', 'dense3a', 'dense3b')}
        # feature based: (graph user, graph item) | (bert user, bert item); else per entity (hybrid.py:72-84).  Concatenating fusions
        # get their operands stored straight into the two halves of their output by the stacks that make them.
        feeds = (('dense1a', 'dense1b'), ('dense2a', 'dense2b')) if self.fb else (('dense1a', 'dense2a'), ('dense1b', 'dense2b'))
        ja, la, ra = self.f1a.plan_joined(rows, w[feeds[0][0]], w[feeds[0][1]], dev)
        jb, lb, rb = self.f1b.plan_joined(rows, w[feeds[1][0]], w[feeds[1][1]], dev)
        dest = {feeds[0][0]: la, feeds[0][1]: ra, feeds[1][0]: lb, feeds[1][1]: rb}
        g1, g2 = _DenseTape.forward_pair(t['dense1a'], (gu, None, dest['dense1a']), t['dense1b'], (gi, None, dest['dense1b']))      # (independent stacks: one launch)
        b1, b2 = _DenseTape.forward_pair(t['dense2a'], (ub, None, dest['dense2a']), t['dense2b'], (ib, None, dest['dense2b']))
        ins = ((g1, g2), (b1, b2)) if self.fb else ((g1, b1), (g2, b2))
        fa, fb = self.f1a.forward(*ins[0], joined=ja), self.f1b.forward(*ins[1], joined=jb)
        jc, lc, rc = self.f2.plan_joined(rows, w['dense3a'], w['dense3b'], dev) if 'residual' not in t else (None, None, None)
        x1, x2 = _DenseTape.forward_pair(t['dense3a'], (fa, None, lc), t['dense3b'], (fb, None, rc))
        x = self.f2.forward(x1, x2, joined=jc)
        if 'residual' in t:                                          # hybrid.py:86-89
            r = t['residual'].forward(x)
            self.s = torch.empty_like(r)
            capi.add3_act(r, x1, x2, self.s, act=self.rs.activation)
            x = self.s
        return t['clf'].forward(x)

    def backward(self, dz, grads, need_input_grad=True):
        t = self.t
        dx = t['clf'].backward(dz, grads, last_is_dz=True)
        skip = None
        if 'residual' in t:
            skip = torch.empty_like(dx)
            capi.act_bwd(dx, self.s, skip, self.rs.activation)       # d(residual(x) + x1 + x2): the same for all three terms
            dx = t['residual'].backward(skip, grads, last_is_dz=True)
        dx1, dx2 = self.f2.backward(dx, grads)
        if skip is not None:
            dx1, dx2 = dx1.contiguous().clone(), dx2.contiguous().clone()
            capi.add_inplace(dx1, skip)
            capi.add_inplace(dx2, skip)
        d3a, d3b = _DenseTape.backward_pair(t['dense3a'], dx1, t['dense3b'], dx2, grads)
        da = self.f1a.backward(d3a, grads)
        db = self.f1b.backward(d3b, grads)
        if self.fb:
            (dg1, dg2), (db1, db2) = da, db
        else:
            (dg1, db1), (dg2, db2) = da, db
        t['dense2a'].backward(db1, grads, need_input_grad=False)
        t['dense2b'].backward(db2, grads, need_input_grad=False)
        return _DenseTape.backward_pair(t['dense1a'], dg1, t['dense1b'], dg2, grads, need_input_grad=need_input_grad)


class _LayerKind:
    """What `_StackTape` asks of one layer type, forward and reverse side by side.  `tape` is the owning _StackTape: its graph, its A^T,
    its linear reverse pass.  forward_layer(k, layer, x, y) writes layer k's output into y and returns what the reverse needs (a named
    record; the default suits layers that call themselves and keep nothing); backward_layer(k, layer, saved, x, y, dx, dy, grads) adds
    d(loss)/dx into dx given dy and fills `grads` for the layer's weights.  forward_stack(x0): (output, cat) of the whole stack at once, taken
    where no stack rate is set; backward_stack(d_out): d(loss)/d(node table) at once where that left no layers to walk.  None: layer by layer."""

    saves_undropped_output = False                                   # see _StackTape.forward

    def __init__(self, tape, layers):
        self.tape, self.layers = tape, layers

    def forward_stack(self, x0):
        return None

    def backward_stack(self, d_out):
        return None

    def forward_layer(self, k, layer, x, y):
        layer([x, self.tape.seq.adj_matrix], out=y)


class _GCNLayers(_LayerKind):
    def forward_stack(self, x0):
        return self.tape.seq._propagate(x0, with_layers=True)        # the inference kernels: their outputs are all the reverse pass needs

    def backward_layer(self, k, layer, saved, x, y, dx, dy, grads):
        tape, (n, c) = self.tape, y.shape
        fused = tape.fused_route(x.shape[1], c, n)
        dz = _buffer(y, n, c)
        grads[layer.bias] = tape.linear_bwd(('b', k), dy, y=y, act='relu', dZ=dz, db_like=layer.bias, K=1, fused=fused)[1]
        dh = _spmm(tape.at, dz, _buffer(y, n, c))                    # A_hat^T . dZ
        # dW = X_k^T . dH, and dH . W^T added into the slice's gradient
        grads[layer.kernel] = tape.linear_bwd(k, dh, x=x, w=layer.kernel.detach(), dX=dx, dw_like=layer.kernel, accumulate_dx=True, fused=fused)[0]


class _LightGCNLayers(_LayerKind):
    forward_stack = _GCNLayers.forward_stack                         # (under 'mean' the running-sum kernels: no `cat`, the layers never exist)

    def backward_stack(self, d_out):
        if self.tape.cat is not None:
            return None
        # g0 = (I + A^T + (A^T)^2 + ...) d_out / (L + 1)
        g0 = torch.zeros((d_out.shape[0], self.tape.widths[0]), dtype=torch.float32, device=d_out.device)
        capi.add_inplace(g0, d_out, 1.0 / (len(self.layers) + 1))
        acc = g0.clone()
        for _ in self.layers:
            acc = _spmm(self.tape.at, acc, torch.empty_like(acc))
            capi.add_inplace(g0, acc)
        return g0

    def backward_layer(self, k, layer, saved, x, y, dx, dy, grads):
        capi.add_inplace(dx, _spmm(self.tape.at, dy, _buffer(x, *x.shape)))


class _DGCFLayers(_LayerKind):
    def backward_layer(self, k, layer, saved, x, y, dx, dy, grads):   # (every layer's input stays in `cat`: the gate's gradient needs it)
        back, dw = _spmm(self.tape.at, dy, _buffer(x, *x.shape)), _buffer(x, x.shape[0])     # A_dgcf^T . d(out)
        capi.locality_scale_bwd(back, x, layer.w.detach().view(-1), dx, dw, accumulate=True)
        grads[layer.w] = dw.view_as(layer.w)


class _SageLayers(_LayerKind):
    """An unfused forward that keeps [x || agg(x)] and the l2-normalised pre-activation.  'mean' is (A + I) / count ('sum': scale 1), so
    its reverse is the row scale, then the value-free SpMM on A^T; max / min keep how many entries attain the extremum and share among them."""

    def __init__(self, tape, layers):
        super().__init__(tape, layers)
        if len({bool(l.self_loops) for l in layers}) != 1 or len({l.aggregate for l in layers}) != 1:
            raise NotImplementedError("GraphSAGE layers with mixed self_loops / aggregate settings")
        self.self_loops, self.aggregate = bool(layers[0].self_loops), layers[0].aggregate
        # 'mean': sum / count (0 for an empty segment), 'sum': sum * 1 — the layer's cached vector; max / min keep a tie count instead
        self.inv_cnt = layers[0].row_scale(tape.seq.adj_matrix) if self.aggregate in ('mean', 'sum') else None

    def forward_layer(self, k, layer, x, y):
        a, (n, f), c = self.tape.seq.adj_matrix, x.shape, y.shape[1]
        xa, cnt = _buffer(x, n, 2 * f), None
        capi.copy_columns(x, xa[:, :f])
        if self.inv_cnt is None:                                     # max / min: the aggregate straight into xa, and how many entries attain it
            cnt = _buffer(x, n, f)
            capi.sage_aggregate(a.rowptr, a.colidx, x, xa[:, f:], self.aggregate, cnt=cnt, self_loop=self.self_loops)
        else:
            ssum = _buffer(x, n, f)
            capi.spmm_csr(a.rowptr, a.colidx, None, x, ssum)
            capi.row_affine(ssum, self.inv_cnt, xa[:, f:], b=x if self.self_loops else None)
        z, nrm, inv = _buffer(x, n, c), _buffer(x, n, c), _buffer(x, n)
        capi.dense(xa, layer.kernel, layer.bias, z, act=None)
        capi.l2norm_fwd(z, nrm, inv, y, act='relu')
        return types.SimpleNamespace(xa=xa, nrm=nrm, inv=inv, cnt=cnt)

    def backward_layer(self, k, layer, saved, x, y, dx, dy, grads):
        at, (n, f), xa = self.tape.at, x.shape, saved.xa
        dz = _buffer(x, *y.shape)
        capi.l2norm_bwd(dy, saved.nrm, saved.inv, dz, act='relu')
        grads[layer.kernel], grads[layer.bias], dxa = self.tape.linear_bwd(k, dz, x=xa, w=layer.kernel.detach(), dw_like=layer.kernel, db_like=layer.bias)
        capi.add_inplace(dx, dxa[:, :f])
        if saved.cnt is not None:
            # every entry that attains the extremum takes d_agg / cnt; row j finds its shares on the targets that list it: A^T's row j
            capi.sage_aggregate_bwd(at.rowptr, at.colidx, xa[:, :f], xa[:, f:], saved.cnt, dxa[:, f:], dx, self_loop=self.self_loops)
            return
        g, back = _buffer(x, n, f), _buffer(x, n, f)
        capi.row_affine(dxa[:, f:], self.inv_cnt, g)                 # d(mean)/d(sum) by A's row counts; 'sum': a copy
        capi.spmm_csr(at.rowptr, at.colidx, None, g, back)           # A^T . g
        capi.add_inplace(dx, back)
        if self.self_loops:
            capi.add_inplace(dx, g)


class _GATLayers(_LayerKind):
    """The inference kernels, keeping H = X . W and the two attention scalars, and amar_gat_bwd_f32 for the softmax reverse.  That reverse
    needs out_i itself (c_i = g_i . (out_i - b)): under a stack rate the undropped output stays saved and the slice gets the dropped copy.
    Layers with several heads take amar_gat_heads_f32 / amar_gat_heads_bwd_f32 (Hd [n, H*C], scalars S [n, 2H]); where the heads are
    averaged the forward also leaves their outputs on the tape, which Y no longer holds apart."""

    saves_undropped_output = True
    edge_drop = None                                                 # the attention masks, set by _StackTape.enable_dropout

    def __init__(self, tape, layers):
        super().__init__(tape, layers)
        if any(l.attn_heads > 1 and float(l.dropout_rate or 0.0) > 0.0 for l in layers):
            # the Philox counter of an edge has no field for a head index
            raise NotImplementedError("attention dropout (dropout_rate > 0) is not implemented for attn_heads > 1; train with dropout_rate=0 "
                                      "(the stack's `dropout` works with any number of heads)")

    def forward_layer(self, k, layer, x, y):
        a, n, c = self.tape.seq.adj_matrix, x.shape[0], y.shape[1]
        if layer.attn_heads > 1:
            hd, s = layer.project_heads(x)
            out = None if layer.concat_heads else _buffer(x, n, hd.shape[1])
            capi.gat_heads(a.rowptr, a.colidx, hd, layer.attn_heads, s, layer.bias, y, concat=layer.concat_heads, self_loop=layer.add_self_loops,
                           out_tape=out)
            return types.SimpleNamespace(h=hd, s=s, y=y, out=out)
        h, s_self, s_neigh = _buffer(x, n, c), _buffer(x, n), _buffer(x, n)
        capi.rowwise_xw(x, layer.kernel.view(-1, c), h, a_self=layer.attn_kernel_self.view(c), a_neigh=layer.attn_kernel_neighs.view(c), s_self=s_self, s_neigh=s_neigh)
        edge = self.edge_drop[k] if self.edge_drop is not None else None
        if edge is not None:
            capi.gat_layer_dropout(a.rowptr, a.colidx, h, s_self, s_neigh, layer.bias, y, edge, self_loop=layer.add_self_loops)
        else:
            capi.gat_layer(a.rowptr, a.colidx, h, s_self, s_neigh, layer.bias, y, self_loop=layer.add_self_loops)
        return types.SimpleNamespace(h=h, s_self=s_self, s_neigh=s_neigh, y=y)

    def _backward_heads(self, k, layer, saved, x, dx, dy, grads):
        tape, a, at, (n, f), hd = self.tape, self.tape.seq.adj_matrix, self.tape.at, x.shape, saved.h
        heads, c = layer.attn_heads, layer.channels
        dout, ds, dh = capi.gat_heads_bwd(a.rowptr, a.colidx, hd, heads, saved.s, saved.y, dy, layer.bias, layer.attn_kernel_self.detach(),
                                          layer.attn_kernel_neighs.detach(), concat=layer.concat_heads, self_loop=layer.add_self_loops,
                                          out_tape=saved.out, transposed=(at.rowptr, at.colidx) if at is not a else None)
        # d a_self[:, h] = Hd[:, h, :]^T . ds[:, h]: the diagonal blocks of the [H, H*C] product ds^T . Hd, read as [C, H] by a view (the
        # separate kernels: a captured step's deferred partial sums could not be viewed that way)
        for key, param, cols in (('s', layer.attn_kernel_self, ds[:, :heads]), ('t', layer.attn_kernel_neighs, ds[:, heads:])):
            full = tape.linear_bwd((key, k), hd, x=cols, dw_like=_buffer(x, heads, heads * c), fused=False)[0]
            grads[param] = torch.diagonal(full.view(heads, heads, c), dim1=0, dim2=1).contiguous().view_as(param)
        fused = tape.fused_route(f, heads * c, n)
        grads[layer.bias] = tape.linear_bwd(('b', k), dout, db_like=layer.bias, K=1, fused=fused)[1]
        w = layer.kernel.detach().view(f, heads * c)
        grads[layer.kernel] = tape.linear_bwd(k, dh, x=x, w=w, dX=dx, dw_like=layer.kernel, accumulate_dx=True, fused=fused)[0]

    def backward_layer(self, k, layer, saved, x, y, dx, dy, grads):
        if layer.attn_heads > 1:
            return self._backward_heads(k, layer, saved, x, dx, dy, grads)
        tape, a, at, (n, f), c, h = self.tape, self.tape.seq.adj_matrix, self.tape.at, x.shape, y.shape[1], saved.h
        edge = self.edge_drop[k] if self.edge_drop is not None else None
        gat_args = (a.rowptr, a.colidx, h, saved.s_self, saved.s_neigh, saved.y, dy, layer.bias,
                    layer.attn_kernel_self.detach().view(c), layer.attn_kernel_neighs.detach().view(c))
        # targets walk A's rows, sources A^T's (one structure where the edge multiset is symmetric)
        transposed = (at.rowptr, at.colidx) if at is not a else None
        if edge is not None:
            dout, ds, dt, dh = capi.gat_bwd_dropout(*gat_args, edge, self_loop=layer.add_self_loops, transposed=transposed)
        else:
            dout, ds, dt, dh = capi.gat_bwd(*gat_args, self_loop=layer.add_self_loops, transposed=transposed)
        fused = tape.fused_route(f, c, n)
        # H^T . ds as (ds^T . H)^T: a [1, c] weight gradient with X = ds, dZ = H
        grads[layer.attn_kernel_self] = tape.linear_bwd(('s', k), h, x=ds.view(n, 1), dw_like=layer.attn_kernel_self, fused=fused, column_x=True)[0]
        grads[layer.attn_kernel_neighs] = tape.linear_bwd(('t', k), h, x=dt.view(n, 1), dw_like=layer.attn_kernel_neighs, fused=fused, column_x=True)[0]
        grads[layer.bias] = tape.linear_bwd(('b', k), dout, db_like=layer.bias, K=1, fused=fused)[1]
        # dW = X_k^T . dH, and dH . W^T added into the slice's gradient
        w = layer.kernel.detach().view(f, c).contiguous()
        grads[layer.kernel] = tape.linear_bwd(k, dh, x=x, w=w, dX=dx, dw_like=layer.kernel, accumulate_dx=True, fused=fused)[0]


class _StackTape(_LinearReverse):
    """Forward of ONE convolution stack (SequentialGNN / HalfInput / FullInputSequentialGNN) that keeps what its reverse
    pass needs, and that reverse pass: d(loss)/d(reduced output) -> weight gradients + d(loss)/d(node table).

    Every layer's output lives in a column slice of one [N, sum(widths)] buffer `cat`; the reduction (reduction.py:9-33)
    is undone first (d_cat = d_out for 'concatenation', d_out / (L+1) per slice for 'mean', ...), then the layers run
    in reverse on the slices of (cat, d_cat).  A layer's own forward and reverse are its `_LayerKind`'s, chosen once from KINDS.
    `at` = the transposed image of the stack's graph, taken once here (before any capture; the tape keeps it and its images alive): every
    product or walk that needs A^T uses it.  For a symmetric graph (config.yaml:36) `at is a` and the reverse pass reuses the forward structure."""

    KINDS = ((GCNConv, 'gcn', _GCNLayers), (LightGCNConv, 'lightgcn', _LightGCNLayers), (GraphSageConv, 'sage', _SageLayers),
             (GATConv, 'gat', _GATLayers), (DGCFConv, 'dgcf', _DGCFLayers))
    MAX_LAYERS = 32                                                  # sites of a stack: 2 * MAX_LAYERS, three stacks at most (< 256)
    edge_drop = property(lambda self: getattr(self.impl, 'edge_drop', None))     # (the GAT layers' own)

    def __init__(self, seq):
        super().__init__()
        self.seq = seq
        layers = list(seq.seq_layers)
        self.kind, kind_cls = next(((name, impl) for cls, name, impl in self.KINDS if layers and all(isinstance(l, cls) for l in layers)), (None, None))
        if self.kind is None:
            raise NotImplementedError("training needs a stack of one layer type (GCN, GraphSAGE, GAT, LightGCN or DGCF)")
        if seq.final_node not in ('concatenation', 'mean', 'sum', 'last', 'w-sum'):
            raise NotImplementedError("no reverse pass for the '{}' reduction".format(seq.final_node))
        self.impl = kind_cls(self, layers)
        self.at = seq.adj_matrix.transposed()                        # A^T: the graph itself where it is symmetric
        self.cat = self.saved = self.node_drop = None                # node_drop: set by enable_dropout (Trainer), the stack trains without otherwise

    def dropout_rates(self):
        """(stack rate, [GAT attention rate per layer]) with 0.0 for 'none'."""
        return float(self.seq.dropout or 0.0), [float(getattr(l, 'dropout_rate', 0.0) or 0.0) for l in self.seq.seq_layers if isinstance(l, GATConv)]

    def enable_dropout(self, seed, step, stack_index):
        """The dropout sites of this stack: layer k's output has site 1 + 2 (32 stack_index + k), the attention
        coefficients of GAT layer k site 2 + 2 (32 stack_index + k); all share the Trainer's key and step counter."""
        rate, gat = self.dropout_rates()
        n_layers = len(self.seq.seq_layers)
        if n_layers > self.MAX_LAYERS or stack_index > 2:
            raise NotImplementedError("dropout sites are numbered for at most {} layers in at most 3 stacks".format(self.MAX_LAYERS))
        base = 2 * (self.MAX_LAYERS * stack_index)
        if rate > 0.0:
            self.node_drop = [capi.Dropout(seed, step, base + 2 * k + 1, rate) for k in range(n_layers)]
        if any(r > 0.0 for r in gat):
            self.impl.edge_drop = [capi.Dropout(seed, step, base + 2 * k + 2, r) if r > 0.0 else None for k, r in enumerate(gat)]

    def _slices(self, t):
        offs = self.offs
        return lambda k: t[:, offs[k]:offs[k + 1]]

    # -- forward ----------------------------------------------------------------------------------------------------
    def forward(self, x0=None):
        """Reduced node representations of the stack over the node table x0 (None: the stack's own table)."""
        seq = self.seq
        x0 = seq.embeddings if x0 is None else x0
        widths = self.widths = seq.layer_widths()
        seq._build_layers(widths)
        self.offs = [int(v) for v in np.cumsum([0] + widths)]
        self.saved = [None] * len(seq.seq_layers)
        whole = self.impl.forward_stack(x0) if self.node_drop is None else None
        if whole is not None:
            out, self.cat = whole
            return out
        cat = self.cat = _buffer(x0, seq.adj_matrix.shape[0], self.offs[-1])
        sl = self._slices(cat)
        capi.copy_columns(x0, sl(0))
        for k, layer in enumerate(seq.seq_layers):
            drop = self.node_drop[k] if self.node_drop is not None else None
            # a kind whose reverse pass needs the undropped output writes it to a buffer that stays saved; the slice takes the dropped copy
            own = drop is not None and self.impl.saves_undropped_output
            y = _buffer(x0, cat.shape[0], widths[k + 1]) if own else sl(k + 1)
            self.saved[k] = self.impl.forward_layer(k, layer, sl(k), y)
            if drop is not None:
                # before the reduction and the next layer read the slice (the reference's loop, gnn.py:76-81); in place where y is the
                # slice.  Sound for the reverse pass: it masks d(slice k + 1) first, so every `Y > 0` it then evaluates sees a kept
                # element (same sign) or meets a gradient that already is zero
                capi.dropout(y, drop, out=sl(k + 1) if own else None)
        return seq._reduce(cat, [sl(k) for k in range(len(widths))], widths)

    # -- reverse ----------------------------------------------------------------------------------------------------
    def _expand(self, d_out, grads):
        """d(loss)/d(cat) from d(loss)/d(reduced output) ('w-sum': also the gradient of the reduction weights, into `grads`)."""
        final, widths = self.seq.final_node, self.widths
        n_terms = len(widths)
        if final == 'concatenation':
            return d_out
        if final == 'w-sum':
            w = self.seq.reduce.w
            d_cat = torch.empty((d_out.shape[0], self.offs[-1]), dtype=torch.float32, device=d_out.device)
            dw = torch.empty(n_terms, dtype=torch.float32, device=d_out.device)
            capi.reduce_layers_wsum_bwd(self.cat, n_terms, widths[0], w.view(-1), d_out, d_cat, dw)
            grads[w] = dw.view_as(w)
            return d_cat
        d_cat = torch.zeros((d_out.shape[0], self.offs[-1]), dtype=torch.float32, device=d_out.device)
        sl = self._slices(d_cat)
        if final == 'last':
            capi.add_inplace(sl(n_terms - 1), d_out)
        else:
            for k in range(n_terms):
                capi.add_inplace(sl(k), d_out, 1.0 / n_terms if final == 'mean' else 1.0)
        return d_cat

    def backward(self, d_out, grads):
        """Fills `grads` for the layers' weights; returns d(loss)/d(node table) [N, widths[0]] (a fresh buffer).
        `d_out` is consumed (it may be modified in place)."""
        g0 = self.impl.backward_stack(d_out)
        if g0 is not None:
            return g0
        sl, dsl = self._slices(self.cat), self._slices(self._expand(d_out, grads))
        for k in reversed(range(len(self.saved))):
            if self.node_drop is not None:                           # the regenerated mask of layer k's output, on its gradient
                capi.dropout(dsl(k + 1), self.node_drop[k])
            self.impl.backward_layer(k, self.seq.seq_layers[k], self.saved[k], sl(k), sl(k + 1), dsl(k), dsl(k + 1), grads)
        g0 = _buffer(d_out, d_out.shape[0], self.widths[0])
        capi.copy_columns(dsl(0), g0)
        self.saved = self.cat = None
        return g0


class DeviceSampler:
    """The positive / negative lists of a UserItemGraphPosNegSample on the device, and the step counter of its draws
    (amar_bpr_sample_i32).  Uploaded once per Sequence; a captured training graph keeps this object (and so its buffers) alive, and
    `serial` (never reused) is part of the graph's key, so a graph never replays against another Sequence's lists."""

    _serials = itertools.count()

    def __init__(self, sequence, device):
        (pp, pi), (npt, ni) = sequence.pos_csr, sequence.neg_csr
        n_users, n_nodes = len(sequence.users), sequence.adj_matrix.shape[0]
        for ptr, ids, what in ((pp, pi, 'positive'), (npt, ni, 'negative-candidate')):
            ptr, ids = np.asarray(ptr), np.asarray(ids)
            # the kernel reads without bounds checks: every user row non-empty, every id a node of the graph
            if len(ptr) != n_users + 1 or ptr[0] != 0 or ptr[-1] != len(ids) or np.any(np.diff(ptr) < 1):
                raise ValueError("every user needs a non-empty {} list".format(what))
            if len(ids) and (ids.min() < 0 or ids.max() >= n_nodes):
                raise ValueError("{} list holds ids outside the graph".format(what))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)   # noqa: E731
        self.pos_ptr, self.pos_ids, self.neg_ptr, self.neg_ids = up(pp), up(pi), up(npt), up(ni)
        self.n_users, self.seed, self.h = n_users, int(sequence.seed), int(sequence.batch_size) // 2
        if self.h < 1:
            raise ValueError("a BPR batch needs batch_size >= 2")
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.serial = next(self._serials)
        self.sequence, self.arrays = sequence, (pp, pi, npt, ni)

    def matches(self, sequence):
        return self.sequence is sequence and all(a is b for a, b in zip(self.arrays, (*sequence.pos_csr, *sequence.neg_csr)))

    def sample(self, u, i, y):
        """One batch into u [2h], i [2h], y [2h]; advances the step counter on the device."""
        capi.bpr_sample(self.pos_ptr, self.pos_ids, self.neg_ptr, self.neg_ids, self.n_users, self.seed, self.step, u, i, y)


class TripletSampler:
    """DeviceSampler's sibling for a UserItemGraphTriplets (amar_bpr_sample_triplets_i32): the positive and exclusion lists on the
    device and the step counter of the draws.  Same surface (h, step, serial, matches, sample), same `serial` sequence, so a graph
    captured for one Sequence never replays against another's lists, whichever kind either is."""

    def __init__(self, sequence, device):
        from deep_cbrs_amar_renaissance_amd.data.datasets import SAMPLE_BY
        (pp, pi), (xp, xi) = sequence.pos_csr, sequence.excl_csr
        n_users, n_items, base = len(sequence.users), int(sequence.n_items), int(sequence.item_base)
        if n_users < 1 or n_items < 1:
            raise ValueError("the triplet sampler needs at least one user and one item")
        # the kernel reads without bounds checks: rows strictly ascending inside the item range, every user with a positive and
        # with a candidate left
        for ptr, ids, what in ((pp, pi, 'positive'), (xp, xi, 'exclusion')):
            ptr, ids = np.asarray(ptr, dtype=np.int64), np.asarray(ids, dtype=np.int64)
            if len(ptr) != n_users + 1 or ptr[0] != 0 or ptr[-1] != len(ids) or np.any(np.diff(ptr) < 0):
                raise ValueError("the {} lists are no CSR over {} users".format(what, n_users))
            if len(ids) and (ids.min() < base or ids.max() >= base + n_items):
                raise ValueError("{} list holds ids outside the item range [{}, {})".format(what, base, base + n_items))
            row = np.repeat(np.arange(n_users), np.diff(ptr))
            if np.any((ids[1:] <= ids[:-1]) & (row[1:] == row[:-1])):
                raise ValueError("every {} list must be strictly ascending".format(what))
        if np.any(np.diff(np.asarray(pp, dtype=np.int64)) < 1):
            raise ValueError("every user needs a non-empty positive list")
        if np.any(np.diff(np.asarray(xp, dtype=np.int64)) >= n_items):
            raise ValueError("an exclusion list covers every item: no candidate is left to draw")
        self.h, self.n_negatives = int(sequence.batch_size) // 2, int(sequence.n_negatives)
        if self.h < 1:
            raise ValueError("a BPR batch needs batch_size >= 2")
        if self.n_negatives < 1 or self.h % self.n_negatives:
            raise ValueError("batch_size // 2 = {} triples do not split into draws of n_negatives = {}".format(self.h, self.n_negatives))
        if sequence.sample_by not in SAMPLE_BY:
            raise ValueError("sample_by must be 'user' or 'interaction' (got {!r})".format(sequence.sample_by))
        self.mode = SAMPLE_BY[sequence.sample_by]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)   # noqa: E731
        self.pos_ptr, self.pos_ids, self.excl_ptr, self.excl_ids = up(pp), up(pi), up(xp), up(xi)
        self.n_users, self.n_items, self.item_base, self.seed = n_users, n_items, base, int(sequence.seed)
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.serial = next(DeviceSampler._serials)
        self.sequence, self.arrays = sequence, (pp, pi, xp, xi)
        self.settings = (sequence.batch_size, sequence.n_negatives, sequence.sample_by, sequence.seed)

    def matches(self, sequence):
        return self.sequence is sequence and all(a is b for a, b in zip(self.arrays, (*sequence.pos_csr, *sequence.excl_csr))) \
            and self.settings == (sequence.batch_size, sequence.n_negatives, sequence.sample_by, sequence.seed)

    def sample(self, u, i, y):
        """One batch of h triples into u [2h], i [2h], y [2h]; advances the step counter on the device."""
        capi.bpr_sample_triplets(self.pos_ptr, self.pos_ids, self.excl_ptr, self.excl_ids, self.n_users, self.n_items, self.item_base,
                                 self.seed, self.step, u, i, y, n_negatives=self.n_negatives, mode=self.mode)


_ADAM_HYPER = dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
# rule -> (AMAR_OPT_* name in capi, Keras' constructor defaults)
OPTIMIZER_RULES = {
    'Adam': ('OPT_ADAM', _ADAM_HYPER),
    'AMSGrad': ('OPT_AMSGRAD', _ADAM_HYPER),
    'SGD': ('OPT_SGD', dict(learning_rate=0.01, momentum=0.0, nesterov=False)),
    'RMSprop': ('OPT_RMSPROP', dict(learning_rate=1e-3, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False)),
    'Adagrad': ('OPT_ADAGRAD', dict(learning_rate=1e-3, initial_accumulator_value=0.1, epsilon=1e-7)),
    'Adamax': ('OPT_ADAMAX', _ADAM_HYPER),
    'Nadam': ('OPT_NADAM', _ADAM_HYPER),
}

# gradient clip of every Keras 2 optimizer -> AMAR_CLIP_* name in capi
CLIP_MODES = {'clipvalue': 'CLIP_VALUE', 'clipnorm': 'CLIP_NORM', 'global_clipnorm': 'CLIP_GLOBAL_NORM'}


class OptimizerSpec:
    """The update rule and hyper-parameters a trainer runs: read from an optimizer object (experiment.py: `rule` + Keras' attribute
    names; an object without a rule name means Adam) and / or keyword arguments, which win — the gradient clip (clipvalue, clipnorm or
    global_clipnorm: `clip` = (name, value) or None) in the same way.  `key` identifies it: two optimizers with equal keys train alike,
    so a cached trainer (and its state) is reused only for an equal key.

    `learning_rate` is whatever utilities/schedules.py:resolve takes: a number, or a schedule (object or mapping) that the device
    evaluates at the step counter — `schedule` then holds it, its key is part of `key` and values['learning_rate'] is its rate at
    step 0.  `decay` (Keras 2's optimizer argument) is InverseTimeDecay(learning_rate, 1, decay).  A plain number without decay:
    `schedule` is None and the key is what it was before schedules existed."""

    def __init__(self, optimizer=None, rule=None, **hyper):
        self.rule = rule or getattr(optimizer, 'rule', None) or 'Adam'
        if self.rule not in OPTIMIZER_RULES:
            raise ValueError("no update rule '{}': choose one of {}".format(self.rule, ', '.join(sorted(OPTIMIZER_RULES))))
        code, defaults = OPTIMIZER_RULES[self.rule]
        clips = {k: hyper.pop(k) if k in hyper else getattr(optimizer, k, None) for k in CLIP_MODES}
        decay = hyper.pop('decay') if 'decay' in hyper else getattr(optimizer, 'decay', None)
        unknown = set(hyper) - set(defaults)
        if unknown:
            raise TypeError("{} has no hyper-parameter {}".format(self.rule, ', '.join(sorted(unknown))))
        given = {k: hyper[k] if k in hyper else getattr(optimizer, k, d) for k, d in defaults.items()}
        self.schedule = self._checked_schedule(resolve_learning_rate(given['learning_rate']), decay)
        if self.schedule is not None:
            given['learning_rate'] = float(self.schedule(0))
        self.values = {k: type(d)(given[k]) for k, d in defaults.items()}
        self.clip = self._checked_clip(clips)
        self.key = (self.rule, tuple(sorted(self.values.items())), self.clip) + ((self.schedule.key,) if self.schedule is not None else ())
        self.code = getattr(capi, code)
        self.flags = (capi.OPT_NESTEROV if self.values.get('nesterov') else 0) | (capi.OPT_CENTERED if self.values.get('centered') else 0)
        self.hyper = capi.optim_hyper(**{k: v for k, v in self.values.items() if k in dict(capi.OptimHyper._fields_)})
        self.n_arrays = capi.optim_state_arrays(self.code, self.flags, self.values.get('momentum', 0.0))

    @property
    def adam(self):
        return self.rule == 'Adam'

    @staticmethod
    def _checked_schedule(rate, decay):
        """The schedule the device follows, or None for a fixed rate.  decay: None or 0 means off (Keras 2's default)."""
        decay = 0.0 if decay is None else float(decay)
        if not decay >= 0.0:                                         # (NaN included)
            raise ValueError("decay must not be negative (got {})".format(decay))
        if isinstance(rate, LearningRateSchedule):
            if decay:
                raise ValueError("decay together with a learning-rate schedule is refused: the schedule already says how the rate decays")
            return rate
        return InverseTimeDecay(rate, 1, decay) if decay else None

    @staticmethod
    def _checked_clip(clips):
        """None, or (name, value) of the one gradient clip that is set (Keras 2's OptimizerV2: None or absent means off)."""
        given = {}
        for name, value in clips.items():
            if value is None:
                continue
            value = float(value)
            if not value > 0.0:                                      # (NaN included)
                raise ValueError("{} must be a positive number (got {})".format(name, value))
            given[name] = value
        if 'clipnorm' in given and 'global_clipnorm' in given:
            raise ValueError("clipnorm and global_clipnorm cannot both be set (as in Keras)")
        if 'clipvalue' in given and len(given) > 1:
            raise ValueError("clipvalue together with clipnorm or global_clipnorm is refused: Keras allows the combination, but the order "
                             "in which it applies the two could not be checked against it")
        return next(iter(given.items()), None)

    @property
    def clip_mode(self):
        return getattr(capi, CLIP_MODES[self.clip[0]])

    def new_arrays(self, param):
        """The rule's state arrays for one parameter: zeros, Adagrad's accumulator at its initial value."""
        fill = self.values.get('initial_accumulator_value', 0.0)
        return [torch.full_like(param, fill) for _ in range(self.n_arrays)]


class Trainer:
    """Holds the optimizer state of a Basic* / HybridBert* model (single-graph, TwoStep or TwoWay stacks) and performs training batches."""

    def __init__(self, model, optimizer=None, bert_dim=None, **hyper):
        gnn = model.gnn
        if hasattr(gnn, 'gnn_layers'):                               # one graph (gnn.py:210-264)
            self.layout, stacks = 'single', [gnn.gnn_layers]
        elif hasattr(gnn, 'step_one_gnn_layers'):                    # TwoStep (tsgnn.py:99-101)
            self.layout, stacks = 'two_step', [gnn.step_one_gnn_layers, gnn.step_two_gnn_layers]
        elif hasattr(gnn, 'way_one_gnn_layers'):                     # TwoWay (twgnn.py:98-105)
            self.layout, stacks = 'two_way', [gnn.way_one_gnn_layers, gnn.way_two_gnn_layers, gnn.step_two_gnn_layers]
        else:
            raise NotImplementedError("no training recipe for {}".format(type(gnn).__name__))
        self.tapes = [_StackTape(seq) for seq in stacks]
        self.kind = self.tapes[-1].kind
        seq = stacks[-1]
        self.hybrid = hasattr(model.rs, 'dense1a')
        if not model.rs.built:
            if self.hybrid:
                if getattr(model, 'bert_table', None) is None and bert_dim is None:
                    raise ValueError("the hybrid head is not built yet: register the BERT table or pass bert_dim")
                model.rs.build_head(model.gnn.output_dim(), bert_dim if bert_dim is not None else model.bert_table.shape[1])
            else:
                model.rs.build_head(model.gnn.output_dim(), model.gnn.output_dim())
        self.model, self.seq = model, seq
        self.n_ids = int(seq.adj_matrix.shape[0])                    # how many ids are valid: the range check of every batch of ids
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.device = self.params[0].device
        self._init_optimizer(optimizer, hyper)
        self.head = _HybridHead(model.rs) if self.hybrid else _BasicHead(model.rs)
        self._init_dropout()

    def _init_optimizer(self, optimizer, hyper):
        """The rule (OptimizerSpec), the step count, every parameter's 0 .. 3 state arrays and the rule's device state (step counter and
        step-dependent scalars: advanced by amar_optim_advance_f32 in the eager and in the captured path alike, so the two are
        interchangeable step by step and Nadam's running product has one home; Adam uses its first two floats)."""
        self.spec = optimizer if isinstance(optimizer, OptimizerSpec) and not hyper else OptimizerSpec(optimizer, **hyper)
        self.t = 0
        self._dev_t = 0                                              # the step count the device state holds (see _sync_step)
        self.opt_arrays = {p: self.spec.new_arrays(p) for p in self.params}
        self._opt_state = torch.zeros(capi.OPTIM_STATE_FLOATS, dtype=torch.float32, device=self.device)
        self.capture_count = 0                                       # hipGraph captures so far (a set learning rate must not add one)
        # the replayed step (`_step`): captured batches by key, the keys past their first batch, the batch buffers last used, those of
        # the body run eagerly (the last key's), and the loss total of an epoch: first batches on the host, every other on the device
        self._graphs, self._seen, self._g, self._eager_g = {}, set(), None, {}
        self._eager_loss, self._loss_sum = 0.0, torch.zeros((), dtype=torch.float32, device=self.device)
        self._lr_state = None                                        # static rate: the launches are those of a trainer without schedules
        if self.spec.schedule is not None:
            self._make_rate_dynamic()

    # -- the learning rate -----------------------------------------------------------------------------------------
    @property
    def dynamic_rate(self):
        """False: the rate is an argument of the advance launch, baked into the captured graphs.  True (a schedule, a decay, or a rate
        that was set): it lives in `_lr_state` on the device and the advance launch evaluates it there."""
        return self._lr_state is not None

    def _make_rate_dynamic(self):
        """Static -> dynamic, once: the device rate state (base rate, rate of the last step) starts at the compiled rate, and whatever
        was captured with the rate baked in is dropped (every shape starts over with its eager batch).  Optimizer state and t stay."""
        if self._lr_state is not None:
            return
        base = self.spec.values['learning_rate']
        self._lr_sched = capi.lr_schedule(self.spec.schedule)
        self._lr_base = float(np.float32(base))
        self._lr_state = torch.full((capi.LR_STATE_FLOATS,), base, dtype=torch.float32, device=self.device)
        self._lr_host = torch.zeros(capi.LR_STATE_FLOATS, dtype=torch.float32).pin_memory()
        self._lr_read = None
        self._graphs.clear()
        self._seen.clear()
        self._eager_g = {}

    def set_learning_rate(self, value):
        """A new base rate from the next batch on: after the first call (which makes the rate dynamic) one write of _lr_state[0]."""
        if self.spec.schedule is not None:
            raise ValueError("the optimizer follows a learning-rate schedule ({!r}): its rate cannot be set (as in Keras)".format(self.spec.schedule))
        value = float(value)
        if not (value >= 0.0 and np.isfinite(np.float32(value))):
            raise ValueError("the learning rate must be a finite, non-negative number (got {})".format(value))
        self._make_rate_dynamic()
        self._lr_base = float(np.float32(value))
        self._lr_state[:1].fill_(value)

    def get_learning_rate(self):
        """The rate the next batch trains with, as the float32 the device holds: the base rate, or the schedule at the step count."""
        if self.spec.schedule is not None:
            return float(self.spec.schedule(self.t))
        return self._lr_base if self._lr_state is not None else float(np.float32(self.spec.values['learning_rate']))

    def pop_learning_rate(self):
        """The rate the last batch trained with (_lr_state[1]); after `pop_loss_sum` it has come over in that call's synchronisation."""
        value, self._lr_read = self._lr_read, None
        return float(self._lr_state[1].item()) if value is None else value

    def _advance_state(self):
        """The one-thread launch that opens an optimizer step: t + 1 and the step's scalars, under a dynamic rate also the rate."""
        spec = self.spec
        if self._lr_state is None:
            capi.optim_advance(self._opt_state, spec.code, spec.flags, spec.hyper)
        else:
            capi.optim_advance_lr(self._opt_state, spec.code, spec.flags, spec.hyper, self._lr_sched, self._lr_state)

    dropout_key, dropout_step = (), None                            # (HeadTrainer: the heads have no dropout, as in the reference)

    def _init_dropout(self):
        """Training-time dropout: where a stack rate or a GAT attention rate is set, one key (engine.next_dropout_seed:
        derived from the seed, one stream per Trainer that drops) and one step counter in device memory that every mask kernel reads
        and `_forward_backward` advances once per batch.  No rate set: nothing is allocated and every path is the one without dropout."""
        rates = [t.dropout_rates() for t in self.tapes]
        if not any(r > 0.0 or any(g > 0.0 for g in gat) for r, gat in rates):
            return
        from deep_cbrs_amar_renaissance_amd import engine
        device = self.device
        self.dropout_seed = engine.next_dropout_seed()
        self.dropout_step = torch.zeros(1, dtype=torch.int64, device=device)
        for index, tape in enumerate(self.tapes):
            tape.enable_dropout(self.dropout_seed, self.dropout_step, index)
        # part of a captured graph's key: the rates and the identity of the state its body reads
        self.dropout_key = (self.dropout_seed, self.dropout_step.data_ptr(), tuple((r, tuple(gat)) for r, gat in rates))

    @staticmethod
    def _l2(param):
        reg = getattr(param, 'regularizer', None)
        return float(reg.l2) if reg is not None else 0.0

    def _loss_kind(self):
        """The compiled loss (Model.compile): 'bce' (binary cross-entropy, the default) or 'bpr' (utilities/losses.py:BPRLoss)."""
        return loss_kind(getattr(self.model, 'loss', None))

    def _compiled(self):
        """(loss code, its four hyper-parameters, history names of the metrics) of Model.compile, resolved where the loss is read
        (utilities/metrics.py:resolve_compiled raises for what has no kernel) and kept until compile() hands over other objects."""
        loss, metrics = getattr(self.model, 'loss', None), getattr(self.model, 'metrics', None)
        held = getattr(self, '_compiled_held', None)
        if held is None or held[0] is not loss or held[1] is not metrics:
            held = self._compiled_held = (loss, metrics, resolve_compiled(loss, metrics))
        return held[2]

    def _loss_spec(self):
        """What a captured batch has baked in of compile(): (loss code, hyper-parameters, whether the metric counters are on).  A
        graph captured under another spec is dropped where it is looked up (`_captured`), so a second compile() captures anew."""
        code, hyper, names = self._compiled()
        return code, hyper, bool(names)

    def _captured(self, key):
        """The captured graph of `key`, or None — also when compile() has changed the loss, its hyper-parameters or the counters
        since the capture: that graph is forgotten and the shape starts over with its eager batch."""
        g = self._graphs.get(key)
        if g is not None and g.get('compiled') != self._loss_spec():
            del self._graphs[key]
            self._seen.discard(key)
            g = None
        return g

    def _metric_block(self):
        """The int64 counter block the loss kernel adds every batch to (include/amar_hip.h: amar_loss_grad_f32), allocated at the
        first counted batch — an eager one, so never inside a capture."""
        if getattr(self, '_counters', None) is None:
            self._counters = torch.zeros(capi.LOSS_COUNTERS, dtype=torch.int64, device=self.device)
            self._counters_host = torch.zeros(capi.LOSS_COUNTERS, dtype=torch.int64).pin_memory()
            self._counters_read = None
        return self._counters

    def _loss_grad(self, p, yv, dz, terms, w=None):
        """Per-pair loss terms (their sum = B x the batch's loss) and d(loss)/d(logit) of the compiled loss; with metrics compiled
        the same launch adds the batch to the counter block.  w (the batch's sample weights on the device) and the class pair of
        `set_class_weight` route to the weighted entry point; without either this is the launch it always was."""
        code, hyper, names = self._compiled()
        cw = self._class_w if self._class_weighted else None
        if code == BPR:
            if w is not None or cw is not None:
                raise ValueError("BPRLoss has no per-pair label or term: it takes no class_weight and no sample weights")
            capi.bpr_grad(p, dz, terms)
        elif code in GROUP_KINDS:                                    # the listwise losses, in bpr_grad's slot: one launch
            if w is not None or cw is not None:
                raise ValueError("{} has no per-pair label or term: it takes no class_weight and no sample weights".format(LOSS_NAMES[code]))
            if self._group_k is None:
                raise ValueError(_NEEDS_TRIPLETS.format(LOSS_NAMES[code]))
            capi.group_loss_grad(GROUP_KINDS[code], hyper[0], p, dz, terms, n_negatives=self._group_k)
        else:
            capi.loss_grad(code, hyper, p, yv, dz, terms, counters=self._metric_block() if names else None, sample_weight=w, class_weight=cw)

    # the group size of the batch being trained on (TripletSampler.n_negatives, set by `train_sampled`); None: no triplet batch yet
    _group_k = None

    # -- the weights of the loss ----------------------------------------------------------------------------------------
    _class_w, _class_weighted = None, False

    def set_class_weight(self, class_weight, labels=None):
        """Keras' fit(class_weight=...) from the next batch on: a mapping over the classes 0 and 1, 'balanced' (over `labels`), a pair
        (class 0, class 1) or None (off).  The pair lives in two floats of device memory that the loss kernel reads: the buffer is
        allocated once per trainer, so a captured graph follows new values without a new capture; only whether the pair is in use is
        part of a graph's key."""
        if isinstance(class_weight, tuple) and len(class_weight) == 2:
            class_weight = {0: class_weight[0], 1: class_weight[1]}
        pair = resolve_class_weight(class_weight, labels)
        if pair is None:
            self._class_weighted = False
            return
        if self._class_w is None:
            self._class_w = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._class_w.copy_(torch.tensor([float(pair[0]), float(pair[1])], dtype=torch.float32))
        self._class_weighted = True

    def _weights_to_device(self, w, b):
        """A batch's sample weights as a float32 device tensor [b], or None."""
        if w is None:
            return None
        wv = to_device_tensor(np.ascontiguousarray(w, dtype=np.float32).reshape(-1) if not isinstance(w, torch.Tensor) else w.reshape(-1))
        if wv.numel() != b:
            raise ValueError("the batch holds {} sample weights for {} pairs".format(wv.numel(), b))
        return wv

    def reset_metrics(self):
        """Clear the counter block (the start of a fit(): batches counted outside an epoch do not belong to it)."""
        if getattr(self, '_counters', None) is not None:
            self._counters.zero_()
            self._counters_read = None

    def pop_metrics(self):
        """{history name: value} of the compiled metrics over the batches since the last call, and the counters cleared.  After
        `pop_loss_sum` the block has already come over in that call's synchronisation; otherwise (eager epochs) it is read here."""
        names = self._compiled()[2]
        if not names:
            return {}
        block = self._metric_block()
        counts = self._counters_read
        if counts is None:
            counts = block.cpu().numpy()
            block.zero_()
        self._counters_read = None
        return metric_values(counts, names)

    # -- one batch ------------------------------------------------------------------------------------------------
    def _bert_rows(self, ids, block):
        if block is not None:
            return block if isinstance(block, torch.Tensor) and block.is_cuda else to_device_tensor(block)
        table = getattr(self.model, 'bert_table', None)
        if table is None:
            raise ValueError("no BERT block in the batch and no resident table registered")
        rows = torch.empty((ids.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
        capi.copy_columns(table, rows, ids=ids)
        return rows

    def _forward_backward(self, u, i, yv, rows, ui=None, w=None):
        """Device-only body of a batch (no host synchronisation, fixed shapes -> capturable as a hipGraph):
        returns (per-pair loss terms [B], {param: gradient}).  w: the batch's sample weights [B] on the device, or None."""
        b = u.numel()
        dev = self.device
        e = self._propagation_forward()                              # full-graph propagation, every batch (basic.py:61-63)
        f = e.shape[1]
        if isinstance(self.head, _BasicHead) and not self.hybrid:    # the towers gather E[u], E[i] themselves (one launch per stack)
            p = self.head.forward(e, e, rows, ids=(u, i))
        else:
            gu = torch.empty((b, f), dtype=torch.float32, device=dev)
            gi = torch.empty((b, f), dtype=torch.float32, device=dev)
            capi.copy_columns(e, gu, ids=u)
            capi.copy_columns(e, gi, ids=i)
            if self.hybrid:
                rows = (self._bert_rows(u, rows[0] if rows else None), self._bert_rows(i, rows[1] if rows else None))
            p = self.head.forward(gu, gi, rows)
        # ---- loss and its gradient through the final sigmoid
        dz = torch.empty((b, 1), dtype=torch.float32, device=dev)
        terms = torch.empty(b, dtype=torch.float32, device=dev)
        self._loss_grad(p, yv, dz, terms, w)
        grads = {}
        de = torch.zeros((e.shape[0], f), dtype=torch.float32, device=dev)
        both = None
        if ui is not None and isinstance(self.head, _BasicHead) and not self.hybrid and 2 * b <= 8192:
            # ui = [u ; i] (a replayed batch's id buffer): the towers leave their input gradients in the two halves of one
            # buffer and ONE launch adds them to the node table's gradient (user and item ids never meet: same sums, same order)
            both = torch.empty((2 * b, f), dtype=torch.float32, device=dev)
            self.head.backward(dz, grads, dx_out=(both[:b], both[b:]))
            capi.scatter_add_rows(both, ui, de)
        else:
            dgu, dgi = self.head.backward(dz, grads)
            capi.scatter_add_rows(dgu, u, de)
            capi.scatter_add_rows(dgi, i, de)
        self._propagation_backward(e, de, grads)
        if self.dropout_step is not None:                            # after the last reader of this batch's masks
            capi.dropout_advance(self.dropout_step)
        return terms, grads

    def loss_and_grads(self, u_ids, i_ids, y, bert=None, sample_weight=None):
        """Forward + reverse pass of one batch. Returns (data loss + regularisation loss, {param: gradient}).
        `bert` = (user block, item block) for the hybrid head (None: rows of the resident table).  `sample_weight` [B] and the pair
        of `set_class_weight` weigh the data loss: sum(w x term) / B."""
        u, i = ids_to_device(u_ids, self.n_ids), ids_to_device(i_ids, self.n_ids)
        yv = to_device_tensor(np.asarray(y, dtype=np.float32) if not isinstance(y, torch.Tensor) else y)
        wv = self._weights_to_device(sample_weight, u.numel())
        with torch.no_grad():
            terms, grads = self._forward_backward(u, i, yv, bert, w=wv)
            return self._batch_loss(terms, u.numel()), grads

    def _batch_loss(self, terms, b, with_l2=True):
        """A batch's loss on the host from its per-pair terms: sum(terms) / b, plus l2 x sum(w^2) of every regularised parameter."""
        loss = float(terms.sum().item()) / b
        for prm in self.params if with_l2 else ():
            l2 = self._l2(prm)
            if l2:
                loss += l2 * float((prm.detach().double() ** 2).sum().item())
        return loss

    # -- one batch as a hipGraph ------------------------------------------------------------------------------------
    def _graph_body(self, upload_slots=False):
        g = self._g
        tapes = self._all_tapes()
        for t in tapes:                                              # weight-gradient partials stay partial: the update launch below adds them
            t.defer_reduce = True
        try:
            terms, grads = self._forward_backward(g['u'], g['i'], g['y'], (g['ub'], g['ib']) if g['ub'] is not None else None, ui=g['ui'],
                                                  w=g.get('w'))
        finally:
            for t in tapes:
                t.defer_reduce = False
        spec = self.spec
        self._advance_state()
        # one launch updates every parameter (a table of slots, uploaded by a captured copy from pinned memory: the
        # gradient buffers of this graph have fixed addresses) and adds the regularisation loss; one more adds the data loss
        flat = [(prm.data.view(-1), capi.flat_gradient(grads[prm]), self._l2(prm)) for prm in self.params]
        if spec.clip:
            # the clip pass finishes every gradient into group 0 of its own buffer (partials added, L2 part included) and clips it
            # there: its table is over the same flat buffers, and the optimizer's table below takes group 0 with g_groups = 0, l2 = 0
            clip_host, _ = capi.clip_slot_table(flat)
            g['clip_host'][:clip_host.numel()].copy_(clip_host)
            g['clip_bytes'] = int(clip_host.numel())
            flat = [(w, capi.finished_gradient(gr, w.numel()), 0.0) for w, gr, _ in flat]
        entries = [(w, gr, [a.view(-1) for a in self.opt_arrays[prm]], l2) for prm, (w, gr, l2) in zip(self.params, flat)]
        host, blocks = capi.optim_slot_table(entries)
        g['slot_host'][:host.numel()].copy_(host)                    # pinned buffer allocated before the capture began
        g['slot_bytes'] = int(host.numel())                          # uploaded ONCE, right after the capture (`_step`), into a
        g['keep'] = entries                                          # buffer allocated BEFORE it (memory of the capture's own pool is reused
        #                                                              by the graph's temporaries): the table never changes — the slots point
        #                                                              into tensors of the graph
        if upload_slots:                                             # (the same body run eagerly: this step's own table, before its update launch)
            self._upload_slots(g)
        batch = float(g['u'].numel())
        capi.sum_into(terms, self._loss_sum)                         # sum of the per-pair terms = data loss x batch size
        reg_acc = self._loss_sum
        if spec.clip:                                                # (adds the regularisation loss itself: not a second time below)
            capi.grad_clip(spec.clip_mode, spec.clip[1], g['clip_dev'], len(entries), blocks, g['clip_ws'],
                           reg_scale=batch, loss_acc=reg_acc)
            reg_acc = None
        capi.optim_multi(spec.code, spec.flags, spec.hyper, g['slot_dev'], len(entries), blocks, self._opt_state,
                         reg_scale=batch, loss_acc=reg_acc)

    def _slot_buffers(self, g):
        """The slot tables of a batch's buffers `g`: pinned host and device memory (and the clip pass's workspace), allocated before a
        capture begins."""
        n = len(self.params)
        g['slot_host'] = torch.empty(64 * n + 64, dtype=torch.uint8).pin_memory()   # >= sizeof(amar_optim_slot) per parameter
        g['slot_dev'] = torch.empty(64 * n + 64, dtype=torch.uint8, device=self.device)
        if self.spec.clip:
            blocks = sum((prm.numel() + 1023) // 1024 for prm in self.params)
            g['clip_host'] = torch.empty(64 * n + 64, dtype=torch.uint8).pin_memory()
            g['clip_dev'] = torch.empty(64 * n + 64, dtype=torch.uint8, device=self.device)
            g['clip_ws'] = torch.zeros(capi.grad_clip_workspace_floats(n, blocks), dtype=torch.float32, device=self.device)

    @staticmethod
    def _upload_slots(g):
        g['slot_dev'][:g['slot_bytes']].copy_(g['slot_host'][:g['slot_bytes']])
        if 'clip_bytes' in g:
            g['clip_dev'][:g['clip_bytes']].copy_(g['clip_host'][:g['clip_bytes']])

    def _new_buffers(self, b, weighted=False, bert_dim=None, staged=False):
        """The static buffers `g` of the replayed body for batches of b pairs: u, i, the labels (and, weighted, the sample weights behind
        them) in ONE int32 buffer, the slot tables, with bert_dim the two BERT blocks.  staged: pinned host memory for uploaded
        batches; batches drawn on the device need none."""
        dev = self.device
        slots = 4 if weighted else 3
        uiy = torch.zeros(slots * b, dtype=torch.int32, device=dev)  # one upload per batch instead of three
        ui = uiy[:2 * b]                                             # (u and i side by side: one scatter of both towers' input gradients)
        blocks = [torch.zeros((b, bert_dim), dtype=torch.float32, device=dev) if bert_dim is not None else None for _ in range(2)]
        g = {'uiy': uiy, 'ui': ui, 'u': ui[:b], 'i': ui[b:], 'y': uiy[2 * b:3 * b].view(torch.float32),
             'w': uiy[3 * b:].view(torch.float32) if weighted else None, 'ub': blocks[0], 'ib': blocks[1]}
        self._slot_buffers(g)
        if staged:
            # pinned staging for the batch's ids and labels, four sets in turn: the uploads are asynchronous, so the host prepares
            # batch k + 1 while the device still runs batch k (a pageable copy_ made the host wait for the stream every batch:
            # 0.13 ms of a 0.52 ms batch at ml1m(s=1))
            g['stage'], g['turn'] = [], 0
            for _ in range(4):
                host = torch.empty(slots * b, dtype=torch.int32).pin_memory()
                g['stage'].append({'uiy': host, 'u': host[:b], 'i': host[b:2 * b], 'y': host[2 * b:3 * b].view(torch.float32),
                                   'w': host[3 * b:].view(torch.float32) if weighted else None, 'done': torch.cuda.Event()})
        return g

    def _step(self, key, b, buffers, fill=None, prologue=None, graph=True, first_batch=None):
        """One batch through the replayed body under `key`: lookup, first-batch policy, buffers, capture, eager body, replay, step count.
        The first batch of a key runs eagerly and warms every lazily built buffer — `first_batch()` where given (ids: train_batch,
        whose loss x b joins `_eager_loss`), else the body itself; the second is captured (graph=False: never; the body runs eagerly
        on buffers kept in `_eager_g`) and every batch from then on replayed.  buffers(): the static buffers of a new key;
        fill(g): the batch's inputs into them, ahead of the body; prologue(g): the body's first launches, captured with it."""
        g = self._captured(key)
        replay = g is not None
        if not replay:
            first = key not in self._seen
            self._seen.add(key)
            if first and first_batch is not None:
                self._eager_loss += first_batch() * b
                return
            g = self._g = self._eager_g[key] if key in self._eager_g else buffers()
            if graph and not first:
                from deep_cbrs_amar_renaissance_amd.engine import capture_graph

                def body():
                    with torch.no_grad():
                        if prologue is not None:
                            prologue(g)
                        self._graph_body()
                g['graph'], _ = capture_graph(body)
                self.capture_count += 1
                g['compiled'] = self._loss_spec()
                self._upload_slots(g)                                # the slot tables of this graph (fixed addresses): once, not per replay
                self._graphs[key], replay = g, True
                self._eager_g.pop(key, None)
            else:
                self._eager_g = {key: g}                             # (kept for the next eager step of this key)
        self._g = g
        if fill is not None:
            fill(g)
        self._sync_step()                                            # eager steps happened in between: resynchronise the counter
        if replay:
            g['graph'].replay()
        else:
            with torch.no_grad():
                if prologue is not None:
                    prologue(g)
                self._graph_body(upload_slots=True)
        self.t += 1
        self._dev_t = self.t

    def train_batch_graphed(self, u_ids, i_ids, y, bert=None, graph=True, sample_weight=None):
        """One training batch replayed from a hipGraph: the forward, the reverse pass and the Adam update are ~100
        small launches that are otherwise bound by host launch time.  The graph is captured at the second batch of a
        given size (the first one runs eagerly, through train_batch); the running loss stays on the
        device (`pop_loss_sum`).  graph=False: the same body, same buffers and uploads, run
        eagerly at every batch instead of captured and replayed (what fit() does under AMAR_TRAIN_GRAPH=0 when the model drops: the
        two then agree bit for bit, masks included).  sample_weight [b]: the batch's weights, uploaded behind the labels into the same
        static buffer; whether a batch carries them, and whether a class pair is in use, is part of the graph's key — their values
        are not."""
        b = len(y)
        with_blocks = bert is not None and bert[0] is not None
        weighted = sample_weight is not None
        if weighted and len(sample_weight) != b:
            raise ValueError("the batch holds {} sample weights for {} pairs".format(len(sample_weight), b))
        key = (b, with_blocks, self._loss_kind()) + self.dropout_key  # (a compile() with another loss captures anew; so would other dropout state)
        if weighted or self._class_weighted:                          # (an unweighted batch keeps the key it always had)
            key += (('weights', weighted, self._class_weighted),)

        def fill(g):
            """Every field from the device, from pinned staging, or — all on the host — staged and sent as ONE upload."""
            st = g['stage'][g['turn'] % len(g['stage'])]
            g['turn'] += 1
            st['done'].synchronize()                                 # (the uploads that last used this staging set have landed)
            fields = [('u', u_ids, self._stage_ids), ('i', i_ids, self._stage_ids), ('y', y, self._stage_floats)]
            if weighted:
                fields.append(('w', sample_weight, self._stage_floats))
            on_device = [isinstance(src, torch.Tensor) and src.is_cuda for _, src, _ in fields]
            mixed = any(on_device)
            for (name, src, to_host), dev_side in zip(fields, on_device):
                if dev_side:
                    g[name].copy_(src.reshape(-1))
                else:
                    to_host(st[name], src)                           # (ids: range check + int32 on the host, into pinned memory)
                    if mixed:
                        g[name].copy_(st[name], non_blocking=True)
            if not mixed:
                g['uiy'].copy_(st['uiy'], non_blocking=True)         # ids and labels of the batch: one asynchronous upload
            st['done'].record()
            if with_blocks:
                g['ub'].copy_(to_device_tensor(bert[0]))
                g['ib'].copy_(to_device_tensor(bert[1]))
        self._step(key, b, lambda: self._new_buffers(b, weighted, int(np.asarray(bert[0]).shape[1]) if with_blocks else None, staged=True),
                   fill=fill, graph=graph, first_batch=lambda: self.train_batch(u_ids, i_ids, y, bert=bert, sample_weight=sample_weight))

    def _stage_ids(self, dst_host, ids):
        stage_ids(dst_host, ids, self.n_ids)

    @staticmethod
    def _stage_floats(dst_host, values):
        dst_host.numpy()[...] = values.numpy() if isinstance(values, torch.Tensor) else np.asarray(values, dtype=np.float32)

    # -- batches drawn on the device (BPR: data/datasets.py:UserItemGraphPosNegSample, UserItemGraphTriplets) --------------------
    def sampler_for(self, sequence):
        """The DeviceSampler (or, for a UserItemGraphTriplets, TripletSampler) of `sequence`, uploaded once.  Another Sequence (or new
        lists) gets a new one, and the graphs captured for the old one are dropped with it."""
        from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphTriplets
        kind = TripletSampler if isinstance(sequence, UserItemGraphTriplets) else DeviceSampler
        sampler = getattr(self, '_sampler', None)
        if sampler is None or type(sampler) is not kind or not sampler.matches(sequence):
            self._graphs = {k: v for k, v in self._graphs.items() if k[0] != 'sampled'}
            self._seen = {k for k in self._seen if k[0] != 'sampled'}
            self._eager_g = {k: v for k, v in self._eager_g.items() if k[0] != 'sampled'}
            sampler = self._sampler = kind(sequence, self.device)
        return sampler

    def train_sampled(self, sampler, graph=True):
        """One training batch whose ids the device sampler draws (nothing is uploaded per batch).  The step is the body of a
        replayed batch — sample, forward, loss, reverse pass, one Adam launch, the loss kept on the device — either replayed from a
        hipGraph (graph=True: captured at the second batch, the first runs the same body eagerly) or run eagerly every time; both give
        the same weights and the same loss bit for bit.  The draws follow the sampler's device step counter."""
        if self.hybrid:
            raise NotImplementedError("the BPR sample Sequence carries no BERT rows: hybrid models do not train on it")
        b = 2 * sampler.h
        self._group_k = getattr(sampler, 'n_negatives', None)       # (a new group size is a new sampler: `serial` keys the graph)
        self._step(('sampled', b, self._loss_kind(), sampler.serial) + self.dropout_key, b, lambda: dict(self._new_buffers(b), sampler=sampler),
                   prologue=lambda g: sampler.sample(g['u'], g['i'], g['y']), graph=graph)

    def _sync_step(self):
        if self.spec.adam and self._dev_t != self.t:                 # host steps happened in between (apply_gradients under a static
            self._opt_state[0] = float(self.t)                       # rate): resynchronise the counter; the other rules count on the
            #                                                          device in both paths

    def _all_tapes(self):
        """Every tape of the trainer that owns a fused reverse pass (Dense stacks of the head, convolution stacks)."""
        head = getattr(self, 'head', None)
        dense = [getattr(head, name, None) for name in ('unet', 'inet', 'clf')] + list(getattr(head, 't', {}).values())
        return [t for t in list(getattr(self, 'tapes', None) or []) + dense if isinstance(t, _LinearReverse)]

    def pop_loss_sum(self):
        """Sum over the batches since the last call of (batch loss x batch size); one host synchronisation."""
        block = getattr(self, '_counters', None)
        if block is not None:                                        # the metric counters come over under the same synchronisation
            self._counters_host.copy_(block, non_blocking=True)
        if self._lr_state is not None:                               # ... and so does the rate of the last step
            self._lr_host.copy_(self._lr_state, non_blocking=True)
        total = self._eager_loss + float(self._loss_sum.item())
        if self._lr_state is not None:
            self._lr_read = float(self._lr_host[1])
        self._eager_loss = 0.0
        self._loss_sum.zero_()
        if block is not None:
            self._counters_read = self._counters_host.numpy().copy()
            block.zero_()
        return total

    def touch_parameters(self):
        """Bump the autograd version counters after graph replays (hoisting caches key on them)."""
        with torch.no_grad():
            for prm in self.params:
                prm.add_(0)

    def _propagation_forward(self):
        """E = gnn(None) with every stack's activations kept on its tape."""
        gnn, tapes = self.model.gnn, self.tapes
        if self.layout == 'single':
            return tapes[0].forward()
        if self.layout == 'two_step':
            items = tapes[0].forward()[:gnn.n_embeddings]
            users = gnn.step_two_gnn_layers.embeddings
            x0 = torch.empty((users.shape[0] + items.shape[0], users.shape[1]), dtype=torch.float32, device=self.device)
            capi.copy_columns(users.detach(), x0[:users.shape[0]])
            capi.copy_columns(items, x0[users.shape[0]:])
            return tapes[1].forward(x0)
        users, items = tapes[0].forward()[:gnn.n_users], tapes[1].forward()[:gnn.n_items]
        x0 = torch.empty((gnn.n_users + gnn.n_items, users.shape[1]), dtype=torch.float32, device=self.device)
        capi.copy_columns(users, x0[:gnn.n_users])
        capi.copy_columns(items, x0[gnn.n_users:])
        return tapes[2].forward(x0)

    def _lift(self, rows, n_nodes):
        """Gradient of a leading-rows slice: the rows, zero below (a stack hands over only its first |U| or |I| nodes)."""
        full = torch.zeros((n_nodes, rows.shape[1]), dtype=torch.float32, device=self.device)
        capi.copy_columns(rows, full[:rows.shape[0]])
        return full

    def _propagation_backward(self, e, de, grads):
        gnn, tapes = self.model.gnn, self.tapes
        if self.layout == 'single':
            grads[gnn.gnn_layers.embeddings] = tapes[0].backward(de, grads)
            return
        if self.layout == 'two_step':
            one, two = gnn.step_one_gnn_layers, gnn.step_two_gnn_layers
            dx0 = tapes[1].backward(de, grads)
            n_users = two.embeddings.shape[0]
            g_users = torch.empty_like(two.embeddings)
            capi.copy_columns(dx0[:n_users], g_users)
            grads[two.embeddings] = g_users
            grads[one.embeddings] = tapes[0].backward(self._lift(dx0[n_users:], one.adj_matrix.shape[0]), grads)
            return
        one, two = gnn.way_one_gnn_layers, gnn.way_two_gnn_layers
        dx0 = tapes[2].backward(de, grads)
        grads[one.embeddings] = tapes[0].backward(self._lift(dx0[:gnn.n_users], one.adj_matrix.shape[0]), grads)
        grads[two.embeddings] = tapes[1].backward(self._lift(dx0[gnn.n_users:], two.adj_matrix.shape[0]), grads)

    def _clipped(self, grads):
        """The eager form of the clip pass of `_graph_body`: {param: finished, clipped gradient} in buffers of the trainer's own (the
        caller's gradients stay as they are); the L2 part is in them, so the update that follows runs with l2 = 0."""
        spec = self.spec
        c = getattr(self, '_eager_clip', None)
        if c is None:
            c = self._eager_clip = {'g': {prm: torch.empty(prm.numel(), dtype=torch.float32, device=self.device) for prm in self.params}}
            host, c['blocks'] = capi.clip_slot_table([(prm.data.view(-1), c['g'][prm], self._l2(prm)) for prm in self.params])
            c['table'] = host.to(self.device)
            c['ws'] = torch.zeros(capi.grad_clip_workspace_floats(len(self.params), c['blocks']), dtype=torch.float32, device=self.device)
        for prm in self.params:
            c['g'][prm].copy_(grads[prm].reshape(-1))
        capi.grad_clip(spec.clip_mode, spec.clip[1], c['table'], len(self.params), c['blocks'], c['ws'])
        return c['g']

    def apply_gradients(self, grads):
        spec = self.spec
        host_step = spec.adam and self._lr_state is None
        if not host_step:
            self._sync_step()                                        # (steps counted on the host before the rate became dynamic)
        self.t += 1
        l2_of = self._l2
        if spec.clip:
            with torch.no_grad():
                grads, l2_of = self._clipped(grads), lambda prm: 0.0
        if host_step:
            # The one place where Adam is not a rule like the others: under a static rate the eager step forms its step size here, from
            # Python doubles (the rate not rounded to float32), and counts t on the host; _sync_step hands t to the device state before
            # the next step that reads it.  The device scalars start from the float32 rate and can differ in the last bit, so moving
            # this step onto them changes trained weights.
            v = spec.values
            lr_t = v['learning_rate'] * np.sqrt(1.0 - v['beta_2'] ** self.t) / (1.0 - v['beta_1'] ** self.t)
        with torch.no_grad():
            if not host_step:
                self._advance_state()                                # the device state the replayed batches advance: one state for both
            for prm in self.params:
                w, g, arrays = prm.data.view(-1), grads[prm].contiguous().view(-1), [a.view(-1) for a in self.opt_arrays[prm]]
                if host_step:
                    capi.adam(w, g, arrays[0], arrays[1], lr_t, v['beta_1'], v['beta_2'], v['epsilon'], l2=l2_of(prm))
                else:
                    capi.optim(spec.code, spec.flags, spec.hyper, w, g, arrays, self._opt_state, l2=l2_of(prm))
                prm.add_(0)                                          # bumps the autograd version counter (hoisting caches key on it)
        if not host_step:
            self._dev_t = self.t

    def train_batch(self, u_ids, i_ids, y, bert=None, sample_weight=None):
        loss, grads = self.loss_and_grads(u_ids, i_ids, y, bert=bert, sample_weight=sample_weight)
        self.apply_gradients(grads)
        return loss


class HeadTrainer(Trainer):
    """BasicRS / HybridCBRS on pre-computed embedding rows (econfigs/basic-kge.yaml, hybrid-kge.yaml): the batch Sequence
    delivers the rows themselves (datasets.py:43-77), so only the Dense stacks (and fusion weights) train."""

    def __init__(self, model, optimizer=None, bert_dim=None, **hyper):
        if not model.built:
            raise ValueError("build the head first (one forward call, as Experimenter.build_model does)")
        self.model = model
        self.hybrid = hasattr(model, 'dense1a')
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.device = self.params[0].device
        self._init_optimizer(optimizer, hyper)
        self.head = _HybridHead(model) if self.hybrid else _BasicHead(model)
        self.tables = self.n_ids = None                              # (n_ids: how many ids are valid, once there are tables)

    # -- batches as ids against tables kept on the device (round 4) ---------------------------------------------------------------
    def set_tables(self, tables):
        """The embedding table(s) the batch Sequence gathers its rows from ([n, D] each: one for BasicRS, graph + BERT for HybridCBRS),
        uploaded once.  Batches are then (user ids, item ids, labels): the rows are gathered on the device inside a replayed hipGraph
        (Trainer.train_batch_graphed) instead of on the host and uploaded every batch — 25 epochs of HybridCBRS at ML-1M size took
        35 s that way, more than any graph model."""
        self.tables = [to_device_tensor(np.ascontiguousarray(t, dtype=np.float32)) for t in tables]
        self.n_ids = min(int(t.shape[0]) for t in self.tables)       # (an id is a row of every table)

    def _rows_of(self, u, i):
        out = []
        for t in self.tables:
            for ids in (u, i):
                rows = torch.empty((ids.numel(), t.shape[1]), dtype=torch.float32, device=t.device)
                capi.copy_columns(t, rows, ids=ids)
                out.append(rows)
        return out                                                   # (user, item) per table: [gu, gi] or [gu, gi, bu, bi]

    def _head_step(self, r, yv, w):
        """Head forward, loss and head reverse pass on the rows r (the inputs are constants): (per-pair terms, {param: gradient})."""
        b = r[0].shape[0]
        p = self.head.forward(r[0], r[1], (r[2], r[3]) if self.hybrid else None)
        dz = torch.empty((b, 1), dtype=torch.float32, device=p.device)
        terms = torch.empty(b, dtype=torch.float32, device=p.device)
        self._loss_grad(p, yv, dz, terms, w)
        grads = {}
        self.head.backward(dz, grads, need_input_grad=False)
        return terms, grads

    def _forward_backward(self, u, i, yv, rows=None, ui=None, w=None):
        """Trainer's per-batch core for ids: gather the rows, then the head step."""
        return self._head_step(self._rows_of(u, i), yv, w)

    def loss_and_grads(self, blocks, y, sample_weight=None):
        """blocks = (user rows, item rows) or (user graph, item graph, user BERT, item BERT), each [B, D]."""
        rows = [to_device_tensor(b) for b in blocks]
        yv = to_device_tensor(np.asarray(y, dtype=np.float32) if not isinstance(y, torch.Tensor) else y)
        b = rows[0].shape[0]
        wv = self._weights_to_device(sample_weight, b)
        with torch.no_grad():
            terms, grads = self._head_step(rows, yv, wv)
            # a finding kept as it is: on blocks the reported loss leaves out the L2 term that the ids paths (below, Trainer) include
            return self._batch_loss(terms, b, with_l2=False), grads

    def train_batch(self, *args, bert=None, sample_weight=None):
        """train_batch(blocks, y): the rows themselves; train_batch(u_ids, i_ids, y): ids against `set_tables` (eager: the first
        batch of a shape before Trainer.train_batch_graphed captures)."""
        if len(args) == 3:
            loss, grads = Trainer.loss_and_grads(self, *args, sample_weight=sample_weight)
        else:
            loss, grads = self.loss_and_grads(*args, sample_weight=sample_weight)
        self.apply_gradients(grads)
        return loss


def _cached_trainer(model, spec):
    """model._trainer if it runs the currently compiled optimizer (rule and hyper-parameters equal), else None: a model compiled again
    with another optimizer trains from fresh state (t = 0, new state arrays, new captured graphs), as Keras does."""
    trainer = getattr(model, '_trainer', None)
    if trainer is not None and trainer.spec.key != spec.key:
        trainer = model._trainer = None
    return trainer


def _trainer_for(model):
    """The trainer of the compiled optimizer: the cached one, or a new one where the model can have one already (fit() creates it
    otherwise, from its first batch)."""
    spec = OptimizerSpec(getattr(model, 'optimizer', None))
    trainer = _cached_trainer(model, spec)
    if trainer is None:
        if hasattr(model, 'gnn'):
            trainer = Trainer(model, optimizer=spec)                 # (ValueError for a hybrid head that is not built yet)
        elif getattr(model, 'built', False):
            trainer = HeadTrainer(model, optimizer=spec)
        else:
            raise ValueError("the model has no trainer yet and cannot have one before its weights are built: call it once, or fit() first")
        model._trainer = trainer
    return trainer


def get_learning_rate(model):
    """The learning rate the next batch trains with (float32 as the device holds it): the compiled rate, the rate last set, or the
    schedule at the trainer's step count."""
    trainer = _cached_trainer(model, OptimizerSpec(getattr(model, 'optimizer', None)))
    if trainer is not None:
        return trainer.get_learning_rate()
    spec = OptimizerSpec(getattr(model, 'optimizer', None))
    return float(spec.schedule(0)) if spec.schedule is not None else float(np.float32(spec.values['learning_rate']))


def set_learning_rate(model, value):
    """Train with another rate from the next batch on (`backend.set_value(model.optimizer.lr, value)` of Keras 2's callbacks).  The rate
    in force is trainer state, like the moments: it holds across fit() calls until the model is compiled with another optimizer.  The
    first call drops the captured training graphs once; every later one is a write of one float on the device.  ValueError: the
    optimizer follows a schedule, or the model cannot have a trainer yet."""
    spec = OptimizerSpec(getattr(model, 'optimizer', None))
    if spec.schedule is not None:
        raise ValueError("the optimizer follows a learning-rate schedule ({!r}): its rate cannot be set (as in Keras)".format(spec.schedule))
    _trainer_for(model).set_learning_rate(value)


def make_learning_rate_dynamic(model):
    """Move the rate into device memory now, at its current value, where it would otherwise move at the first set_learning_rate: a
    callback that is going to set the rate calls this when training begins, so that the whole fit() reports `lr` and no graph is
    captured only to be dropped.  Nothing to do under a schedule: the rate is on the device already."""
    if OptimizerSpec(getattr(model, 'optimizer', None)).schedule is None:
        _trainer_for(model)._make_rate_dynamic()


class _History:
    """fit()'s return value in the making: {'loss': [...], '<metric>': [...]} with the compiled metrics in compile order under Keras'
    history names (and 'lr', the rate of the epoch's last batch, once the rate is dynamic).  Resolving them here is where fit() reads the compiled loss and metrics: what compile() refuses is refused again."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.values = {'loss': []}
        self.values.update((name, []) for name in trainer._compiled()[2])
        trainer.reset_metrics()

    def epoch(self, loss, epoch, epochs, verbose):
        """Close an epoch: its loss, and the metrics of its batches (read from the device counters, which start over)."""
        self.values['loss'].append(loss)
        for name, value in self.trainer.pop_metrics().items():
            self.values[name].append(value)
        if self.trainer.dynamic_rate:                                # the rate of the epoch's last step; a static rate adds no key
            if 'lr' not in self.values:                              # (set for the first time in mid-fit: the epochs before ran at the compiled rate)
                self.values['lr'] = [float(np.float32(self.trainer.spec.values['learning_rate']))] * (len(self.values['loss']) - 1)
            self.values['lr'].append(self.trainer.pop_learning_rate())
        if verbose:
            print("Epoch {}/{} - ".format(epoch + 1, epochs) + " - ".join("{}: {:.4f}".format(k, v[-1]) for k, v in self.values.items() if not k.startswith('val_')))


class _FitHooks:
    """What fit() does around the step when it is asked to: Keras-style callbacks (duck-typed: on_train_begin / on_train_end(logs),
    on_epoch_begin / on_epoch_end(epoch, logs), on_train_batch_begin / on_train_batch_end(batch, logs), set_model(model)), a validation
    pass every `validation_freq`-th epoch (`validation_data`: anything evaluate() accepts -> val_loss, val_<metric>;
    `validation_ranking`: {'trainset', 'ratings', 'ks', 'users'} -> val_precision_at_<k>, val_recall_at_<k>, val_ndcg_at_<k>,
    val_hit_at_<k> through evaluate_ranking; with 'rank_metrics': ['auc', 'mrr', 'map'] (any subset; 'ks' may then be empty) also
    val_auc / val_mrr / val_map from the exact rank of every held-out item) and `model.stop_training`.

    One `logs` dict per epoch goes to every callback in list order: the epoch's training entries, then its val_* entries; a callback
    may add keys for the callbacks after it.  The batch hooks are called only on callbacks that define them (a method inherited from
    utilities.keras.Callback does not count) and receive logs = {}: the batch loss stays on the device until the epoch ends, and
    reading it would put a host synchronisation into every replayed batch.

    Validation runs predict() / recommend() on the weights the epoch left: it reads neither the training Sequence nor the dropout /
    BPR step counters, leaves the model's hoist state as it found it, and the next batch replays the captured training graph."""

    _HOOKS = ('on_train_begin', 'on_train_end', 'on_epoch_begin', 'on_epoch_end', 'on_train_batch_begin', 'on_train_batch_end')

    def __init__(self, model, history, callbacks, validation_data, validation_freq, validation_ranking):
        from deep_cbrs_amar_renaissance_amd.utilities.keras import Callback
        self.model, self.history = model, history
        self.callbacks = list(callbacks or [])
        self.validation_data = validation_data
        self.freq = int(validation_freq)
        if self.freq < 1:
            raise ValueError("validation_freq must be a positive integer (got {!r})".format(validation_freq))
        self.ranking = None
        if validation_ranking is not None:
            if not hasattr(model, 'recommend'):
                raise NotImplementedError("{} has no recommend(): validation_ranking cannot rank with it".format(type(model).__name__))
            missing = [key for key in ('trainset', 'ratings', 'ks') if key not in validation_ranking]
            if missing:
                raise ValueError("validation_ranking needs the keys 'trainset', 'ratings' and 'ks' (missing {})".format(missing))
            self.ranking = dict(validation_ranking)
            if self.ranking.get('rank_metrics') is not None:
                from deep_cbrs_amar_renaissance_amd.utilities.metrics import check_rank_metrics
                self.ranking['rank_metrics'] = check_rank_metrics(self.ranking['rank_metrics'])
        names = history.trainer._compiled()[2]
        self.val_names = ['loss'] + (['accuracy'] if all(name == 'accuracy' for name in names) else list(names))   # what evaluate() returns
        self.hooks = {}
        for hook in self._HOOKS:
            self.hooks[hook] = [getattr(cb, hook) for cb in self.callbacks
                                if callable(getattr(cb, hook, None)) and getattr(type(cb), hook, None) is not getattr(Callback, hook)]
        self.batch_begin, self.batch_end = self.hooks['on_train_batch_begin'], self.hooks['on_train_batch_end']
        for cb in self.callbacks:
            if callable(getattr(cb, 'set_model', None)):
                cb.set_model(model)

    def train_begin(self):
        for hook in self.hooks['on_train_begin']:
            hook({})

    def train_end(self):
        logs = {name: values[-1] for name, values in self.history.values.items() if values}
        for hook in self.hooks['on_train_end']:
            hook(logs)

    def epoch_begin(self, epoch):
        for hook in self.hooks['on_epoch_begin']:
            hook(epoch, {})

    def on_batch_begin(self, batch):
        for hook in self.batch_begin:
            hook(batch, {})

    def on_batch_end(self, batch):
        for hook in self.batch_end:
            hook(batch, {})

    def _validate(self):
        out = {}
        if self.validation_data is not None:
            values = self.model.evaluate(self.validation_data)
            out.update(('val_' + name, float(value)) for name, value in zip(self.val_names, values))
        if self.ranking is not None:
            r = self.ranking
            found = self.model.evaluate_ranking(r['trainset'], r['ratings'], r['ks'], users=r.get('users'),
                                                exclude_seen=r.get('exclude_seen', True), rank_metrics=r.get('rank_metrics'))
            out.update(('val_' + name, float(value)) for name, value in found.items()
                       if not name.startswith('users_') and name != 'rank_metrics_users')
        return out

    def epoch_end(self, epoch, verbose):
        """After history.epoch(): validate when due, hand the epoch's logs to the callbacks; True when training is to stop."""
        values = self.history.values
        logs = {name: v[-1] for name, v in values.items() if v and not name.startswith('val_')}
        if (self.validation_data is not None or self.ranking is not None) and (epoch + 1) % self.freq == 0:
            found = self._validate()
            for name, value in found.items():
                values.setdefault(name, []).append(value)
            logs.update(found)
            if verbose:
                print("    " + " - ".join("{}: {:.4f}".format(k, v) for k, v in found.items()))
        for hook in self.hooks['on_epoch_end']:
            hook(epoch, logs)
        return bool(getattr(self.model, 'stop_training', False))


def _fit_hooks(model, history, callbacks, validation_data, validation_freq, validation_ranking):
    """The _FitHooks of a fit() call, or None when it has neither callbacks nor validation (the loop then runs as it always did)."""
    if not callbacks and validation_data is None and validation_ranking is None:
        return None
    return _FitHooks(model, history, callbacks, validation_data, validation_freq, validation_ranking)


def _split_batch(batch):
    """(inputs, y, w) of a Sequence's batch: w is the third element of a weighted Sequence's batch (Keras' sample weights), else None."""
    return batch[0], batch[1], (batch[2] if len(batch) > 2 else None)


def _ids_step(trainer, read, replayed_body, graph):
    """fit()'s step for batches of ids, against the graph or against resident tables: read(b) -> (u, i, y, w, bert).  replayed_body:
    through train_batch_graphed (the loss stays on the device), else train_batch.  A step returns (pairs, loss x pairs on the host)."""
    def step(b):
        u, i, y, w, bert = read(b)
        if replayed_body:
            trainer.train_batch_graphed(u, i, y, bert=bert, graph=graph, sample_weight=w)
            return len(y), 0.0
        return len(y), trainer.train_batch(u, i, y, bert=bert, sample_weight=w) * len(y)
    return step


def _blocks_step(trainer, sequence):
    """fit()'s step for a HeadTrainer on the Sequence's own blocks of rows (AMAR_RESIDENT_ROWS=0, or a Sequence without a table)."""
    def step(b):
        blocks, y, w = _split_batch(sequence[b])
        return len(y), trainer.train_batch(blocks, y, sample_weight=w) * len(y)
    return step


def _sampled_step(trainer, sampler, graph):
    """fit()'s step for batches drawn on the device: 2 h pairs each; the Sequence's host stream is not read."""
    pairs = 2 * sampler.h

    def step(b):
        trainer.train_sampled(sampler, graph=graph)
        return pairs, 0.0
    return step


def _run_epochs(trainer, sequence, hooks, history, step, device_loss, reshuffle, initial_epoch, epochs, verbose):
    """fit()'s one epoch loop: step(b) for every batch of every epoch, and around it the hooks, the epoch's loss (device_loss: the total
    the replayed body keeps on the device, else the sum of what the steps return), history, validation, stop.  reshuffle: the Sequence's
    on_epoch_end() after every epoch."""
    if hooks is not None:
        hooks.train_begin()
    for epoch in range(int(initial_epoch), int(epochs)):
        total, count = 0.0, 0
        if hooks is not None:
            hooks.epoch_begin(epoch)
        for b in range(len(sequence)):
            if hooks is not None and hooks.batch_begin:
                hooks.on_batch_begin(b)
            pairs, loss = step(b)
            count += pairs
            total += loss
            if hooks is not None and hooks.batch_end:
                hooks.on_batch_end(b)
        if device_loss:
            total = trainer.pop_loss_sum()
            trainer.touch_parameters()
        history.epoch(total / max(count, 1), epoch, epochs, verbose)
        stop = hooks is not None and hooks.epoch_end(epoch, verbose)
        if reshuffle and hasattr(sequence, 'on_epoch_end'):
            sequence.on_epoch_end()
        if stop:
            break
    if hooks is not None:
        hooks.train_end()
    return history.values


def fit(model, sequence, epochs=1, callbacks=None, verbose=True, validation_data=None, validation_freq=1, validation_ranking=None,
        initial_epoch=0, class_weight=None, workers=None):
    """Keras-style ``fit`` over a batch Sequence: epochs ``initial_epoch`` .. ``epochs - 1``, ``on_epoch_end`` reshuffles
    (datasets.py:205-213).  ``callbacks``, ``validation_data``, ``validation_freq``, ``validation_ranking``: _FitHooks; only validated
    epochs add a val_* entry to the returned history, as in Keras.  ``model.stop_training = True`` set by a callback's on_epoch_end
    ends training after that epoch.

    ``class_weight`` (a mapping over the classes 0 and 1, 'balanced', or the pair `resolve_class_weight` returns) and the sample weights of a
    Sequence whose batches are (inputs, y, w) weigh the data loss as Keras 2 does: w_j = sample_weight_j x class_weight[label_j],
    batch loss = sum_j w_j l_j / B, epoch loss = sum over all pairs / N; the L2 term and the compiled metrics stay unweighted, and
    validation never applies class_weight.  It holds for this call only.  BPR training refuses both.  ``workers`` (the loader
    threads of Keras' fit, passed by the experiment) is accepted and not read: batches are taken in the loop.  Any other keyword
    is a TypeError.

    What differs between models and Sequences is the step chosen here (`_ids_step`, `_blocks_step`, `_sampled_step`); the epochs
    around it are `_run_epochs`.  AMAR_TRAIN_GRAPH=0: eager batches instead of replayed ones."""
    if validation_ranking is not None and not hasattr(model, 'recommend'):
        raise NotImplementedError("{} has no recommend(): validation_ranking cannot rank with it".format(type(model).__name__))
    if class_weight is not None and not isinstance(class_weight, tuple):
        rows = getattr(sequence, 'ratings', None)                # (the Sequences of data/datasets.py: the labels the mapping must cover)
        labels = rows[:, 2] if isinstance(rows, np.ndarray) and rows.ndim == 2 and rows.shape[1] >= 3 else None
        class_weight = resolve_class_weight(class_weight, labels)
    model.stop_training = False
    from deep_cbrs_amar_renaissance_amd.data.datasets import (HybridUserItemEmbeddings, UserItemEmbeddings, UserItemGraphPosNegSample,
                                                              UserItemGraphTriplets)
    spec = OptimizerSpec(getattr(model, 'optimizer', None))
    use_graph = os.environ.get('AMAR_TRAIN_GRAPH', '1') != '0'
    sampled = hasattr(model, 'gnn') and isinstance(sequence, (UserItemGraphPosNegSample, UserItemGraphTriplets))
    group_code, _, group_name = resolve_loss(getattr(model, 'loss', None))
    if group_code in GROUP_KINDS:
        # a listwise loss reads the batch as groups of one user's positive and its n_negatives negatives: only the triplet Sequence
        # lays them out so (rows (j, h + j) of a UserItemGraphPosNegSample pair do not share a user; a rating batch has no groups)
        if not (sampled and isinstance(sequence, UserItemGraphTriplets)):
            raise ValueError(_NEEDS_TRIPLETS.format(group_name))
        resolve_compiled(model.loss, getattr(model, 'metrics', None))    # (compiled metrics are refused as under BPRLoss)
    if not hasattr(model, 'gnn'):                              # BasicRS / HybridCBRS on pre-computed rows: head-only training
        trainer = _cached_trainer(model, spec)
        if trainer is None:
            if not model.built and len(sequence):
                model(sequence[0][0])                          # one forward call builds every weight (as Keras does)
            trainer = model._trainer = HeadTrainer(model, optimizer=spec)
        # the reference's Sequences of pre-computed rows (datasets.py:55-80) gather them on the host from one (BasicRS) or two
        # (HybridCBRS) tables indexed by node id: the tables go to the device once and the batches are read as ids
        # (AMAR_RESIDENT_ROWS=0: the batches as they come, eager)
        tables = None
        if os.environ.get('AMAR_RESIDENT_ROWS', '1') != '0':
            if type(sequence) is UserItemEmbeddings and not trainer.hybrid:
                tables = [sequence.embeddings]
            elif type(sequence) is HybridUserItemEmbeddings and trainer.hybrid:
                tables = [sequence.graph_embeddings, sequence.bert_embeddings]
            if tables is not None and not all(isinstance(t, np.ndarray) and t.ndim == 2 for t in tables):
                tables = None
        if tables is not None:
            src = getattr(trainer, '_table_sources', None)
            if src is None or len(src) != len(tables) or any(a is not b for a, b in zip(src, tables)):
                trainer.set_tables(tables)
                trainer._table_sources = tables

            def read(b):
                r = sequence._batch_ratings(b)
                return r[:, 0], r[:, 1], r[:, 2], sequence._batch_weights(b), None
            step, device_loss = _ids_step(trainer, read, use_graph, True), use_graph
        else:
            step, device_loss = _blocks_step(trainer, sequence), False
    elif sampled:
        # a BPR sample Sequence: its lists go to the device once and every batch is drawn there (amar_bpr_sample_i32 /
        # amar_bpr_sample_triplets_i32), inside the replayed training graph (AMAR_TRAIN_GRAPH=0: the same steps eagerly, the same ids)
        if class_weight is not None:
            raise ValueError("class_weight cannot weigh BPR training: the batches are drawn on the device and have no per-pair label")
        if getattr(sequence, 'sample_weight', None) is not None:
            raise ValueError("the BPR sample Sequence draws its batches on the device: it carries no sample weights")
        trainer = _cached_trainer(model, spec)
        if trainer is None:
            trainer = model._trainer = Trainer(model, optimizer=spec)
    else:
        # Hybrid batches of the reference's own Sequence (datasets.py:95-123 here, 112-115 there) carry, besides the ids, the BERT rows of
        # the batch's users and items — gathered on the host from ONE table indexed by node id and uploaded every batch (6 MB at batch
        # 1 024).  That table is registered once on the device instead and the batches are read as ids only: the same rows, gathered
        # there (AMAR_RESIDENT_BERT=0: the batches as they come).  A replayed hybrid batch at ml1m(s=1): 0.41 against 0.71 ms.
        ids_only = model.resident_ids(sequence) if hasattr(model, 'resident_ids') else None
        trainer = _cached_trainer(model, spec)
        if trainer is None:
            hp = {}
            if hasattr(model.rs, 'dense1a') and not model.rs.built and len(sequence):
                first = sequence[0][0]
                if len(first) >= 4 and first[2] is not None:
                    hp['bert_dim'] = int(np.asarray(first[2]).shape[1])
            trainer = model._trainer = Trainer(model, optimizer=spec, **hp)
        if trainer._loss_kind() == 'bpr' and class_weight is not None:     # (a weighted batch under BPR is refused where it is read)
            raise ValueError("BPRLoss has no per-pair label or term: it takes no class_weight and no weighted Sequence")
        source = ids_only if ids_only is not None else sequence

        def read(b):
            inputs, y, w = _split_batch(source[b])
            # hybrid batches carry the BERT blocks (datasets.py:112-115)
            return inputs[0], inputs[1], y, w, ((inputs[2], inputs[3]) if len(inputs) >= 4 else None)
        # a model that drops runs the replayed body under AMAR_TRAIN_GRAPH=0 too, eagerly (same bits, masks included)
        device_loss = use_graph or trainer.dropout_step is not None
        step = _ids_step(trainer, read, device_loss, use_graph)
    trainer.set_class_weight(class_weight)                       # (None: off — the pair of an earlier fit() does not linger)
    if sampled:
        step, device_loss = _sampled_step(trainer, trainer.sampler_for(sequence), use_graph), True
    history = _History(trainer)
    hooks = _fit_hooks(model, history, callbacks, validation_data, validation_freq, validation_ranking)
    # (the sampled loop never calls on_epoch_end: the host stream of the BPR Sequences must not advance)
    return _run_epochs(trainer, sequence, hooks, history, step, device_loss, not sampled, initial_epoch, epochs, verbose)

"""GATConv: the Spektral layer the reference instantiates at `src/models/gnn.py:321-328`.

Spektral 1.x single-mode sparse path (``_call_single``), attn_heads=1, concat_heads=True, add_self_loops=True:

    H = X . W                                   W  [F, 1, C]
    e_ij  = LeakyReLU_0.2( H_i . a_self + H_j . a_neigh )        over A's edges (duplicates kept) + (i, i)
    alpha = exp(e - max_i) / ( sum_i exp(e - max_i) + 1e-9 )      unsorted_segment_softmax over targets
    X'_i  = act( sum_j alpha_ij H_j + b )

``dropout_rate`` drops the coefficients alpha after the softmax while training (training.py, `amar_gat_layer_dropout_f32` /
`amar_gat_bwd_dropout_f32`); calling the layer, as every scoring path does, is inference and ignores it, as Keras does outside fit().

On the device: `amar_rowwise_xw_f32` (H and the two attention scalars per node) followed by
`amar_gat_layer_f32` (two passes over the row: max of the neighbour scalars, then the weighted sum); on graphs whose
node table exceeds the per-XCD L2s, `amar_gat_xs_f32` (XCD-sliced image, exact online softmax over (max, sum, weighted
sum) triples).

``attn_heads`` = H > 1 (Spektral's ``call``: H independent heads of ``channels`` outputs each, W [F, H, C], attention kernels
[C, H, 1]; ``concat_heads`` joins them to H*C columns, otherwise they are averaged, both before bias and activation) takes
`amar_rowwise_xw_heads_f32` and `amar_gat_heads_f32` at every graph size: one wavefront per row walks it once for all heads.
channels % 4 == 0 and H * channels <= 64.  One head takes exactly the single-head path above.
"""
import os

import torch

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd.engine import Layer
from deep_cbrs_amar_renaissance_amd.utilities.math import spmm_kind


class GATConv(Layer):
    def __init__(self, channels, attn_heads=1, concat_heads=True, dropout_rate=0.5, return_attn_coef=False,
                 add_self_loops=True, activation=None, use_bias=True, kernel_regularizer=None,
                 bias_regularizer=None, attn_kernel_regularizer=None, **kwargs):
        super().__init__()
        if return_attn_coef:
            raise NotImplementedError("the HIP GAT layer does not return its attention coefficients (return_attn_coef)")
        attn_heads = int(attn_heads)
        if attn_heads < 1:
            raise ValueError("attn_heads must be at least 1 (got {})".format(attn_heads))
        if attn_heads > 1 and not capi.gat_heads_supported(attn_heads, int(channels)):
            raise NotImplementedError("the multi-head HIP GAT layer needs channels % 4 == 0 and attn_heads * channels <= {} (got attn_heads={}, "
                                      "channels={})".format(capi.GAT_HEADS_MAX_WIDTH, attn_heads, channels))
        self.attn_heads, self.concat_heads = attn_heads, bool(concat_heads)
        self.dropout_rate = capi.check_dropout_rate(dropout_rate, 'dropout_rate')      # used by training.py only
        if activation != 'relu' or not use_bias:
            raise NotImplementedError("the HIP GAT layer is built for activation='relu', use_bias=True")
        self.channels, self.add_self_loops = channels, add_self_loops
        self.kernel_regularizer, self.bias_regularizer = kernel_regularizer, bias_regularizer
        self.attn_kernel_regularizer = attn_kernel_regularizer
        self.kernel = self.attn_kernel_self = self.attn_kernel_neighs = self.bias = None

    @property
    def output_width(self):
        """Columns of the layer's output: the heads side by side under concat_heads, one head's channels where they are averaged."""
        return self.channels * self.attn_heads if self.concat_heads else self.channels

    def build(self, input_shape):
        f_in = input_shape[0][-1]
        c, heads = self.channels, self.attn_heads
        if heads > 1 and f_in > capi.GAT_HEADS_MAX_WIDTH:
            raise NotImplementedError("the multi-head HIP GAT layer takes inputs of at most {} columns (got {}: a 'concatenation' hand-over of "
                                      "several wide layers?)".format(capi.GAT_HEADS_MAX_WIDTH, f_in))
        self.kernel = self.add_weight('kernel', (f_in, heads, c), 'glorot_uniform', self.kernel_regularizer)
        self.attn_kernel_self = self.add_weight('attn_kernel_self', (c, heads, 1), 'glorot_uniform', self.attn_kernel_regularizer)
        self.attn_kernel_neighs = self.add_weight('attn_kernel_neighs', (c, heads, 1), 'glorot_uniform', self.attn_kernel_regularizer)
        self.bias = self.add_weight('bias', (self.output_width,), 'zeros', self.bias_regularizer)

    def project_heads(self, x):
        """(Hd [n, H*C], S [n, 2H]) of the multi-head path: the heads' projections and their attention scalars."""
        n, heads = x.shape[0], self.attn_heads
        hd = torch.empty((n, heads * self.channels), dtype=torch.float32, device=x.device)
        s = torch.empty((n, 2 * heads), dtype=torch.float32, device=x.device)
        capi.rowwise_xw_heads(x, self.kernel.detach(), hd, self.attn_kernel_self.detach(), self.attn_kernel_neighs.detach(), s)
        return hd, s

    def call(self, inputs, out=None, **kwargs):
        x, a = inputs
        n, c = a.shape[0], self.channels
        if self.attn_heads > 1:
            hd, s = self.project_heads(x)
            if out is None:
                out = torch.empty((n, self.output_width), dtype=torch.float32, device=x.device)
            capi.gat_heads(a.rowptr, a.colidx, hd, self.attn_heads, s, self.bias, out, concat=self.concat_heads, self_loop=self.add_self_loops)
            return out
        h = torch.empty((n, c), dtype=torch.float32, device=x.device)
        s_self = torch.empty(n, dtype=torch.float32, device=x.device)
        s_neigh = torch.empty(n, dtype=torch.float32, device=x.device)
        capi.rowwise_xw(x, self.kernel.view(-1, c), h, a_self=self.attn_kernel_self.view(c),
                        a_neigh=self.attn_kernel_neighs.view(c), s_self=s_self, s_neigh=s_neigh)
        if out is None:
            out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        # large graphs: XCD-sliced form, exact online softmax.  ml1m(s=64): C = 8 0.54 ms against 0.94 (row kernel), C = 16 0.94 / 1.08;
        # at C = 32 the XS form (4 entries per step) loses, 2.20 / 1.37, and is only used for the row blocks of a partition
        kind = spmm_kind(a, c)
        large = kind == 'xs' or (c == 32 and kind == 'csr' and not os.environ.get('AMAR_SPMM_KIND') and
                                 a.shape[0] == a.shape[1] and a.shape[1] * c * 4 >= (16 << 20))
        lt = a.tiled_gat_image(c) if c in (8, 16, 32) and large else None
        if lt is not None:
            # the LDS-tiled walk with additive softmax weights against a per-row bound (amar_gat_lt_f32)
            capi.gat_lt(lt, a, h, s_self, s_neigh, self.bias, out, self_loop=self.add_self_loops)
        elif c in (8, 16) and kind == 'xs':
            capi.gat_xs(a.xcd_sliced(), h, s_self, s_neigh, self.bias, out, self_loop=self.add_self_loops)
        else:
            capi.gat_layer(a.rowptr, a.colidx, h, s_self, s_neigh, self.bias, out, self_loop=self.add_self_loops)
        return out

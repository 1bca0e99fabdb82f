"""GraphSageConv: the Spektral layer the reference instantiates at `src/models/gnn.py:354-361`.

Spektral 1.x semantics; `aggregate` is `model.aggregate` of the reference's config (`config.yaml:17-18`, default 'mean'):

    a    <- add_self_loops(a)
    agg  =  unsorted_segment_OP( X[source], target )          OP = mean | sum | max | min; edge values ignored,
                                                              every duplicate edge an entry of its own
    X'   =  act( l2_normalize( [X || agg] . W + b ) )         W [2 F, C]; normalise BEFORE the activation

Routes on the device (utilities.math.spmm_kind decides between the row form and the tiled images):

    mean  row form, F in {4, 8, 16, 32}, C <= 64: one fused row kernel (`amar_sage_layer_f32`).  Tiled form: the LDS-tiled
          mean image with the layer's tail in the same launch (`amar_spmm_lt_f32`, AMAR_SPMM_SAGE_TAIL) where F = C in
          {8, 16, 32}, else the aggregate on the tiled image (LDS-tiled or XCD-sliced, diag = 1, row scale = 1 / count) followed
          by `amar_sage_tail_f32`.  Other widths of the row form (24 / 48, the 'concatenation' hand-over of TwoStep / TwoWay
          stacks): value-free `amar_spmm_csr_f32` + `amar_row_affine_f32`, then the tail.  Past the tail kernel's limits
          (F or C above 64 or not a multiple of 4): `amar_dense_f32` + `amar_l2norm_fwd_f32`.
    sum   the mean routes with row scale 1; the fused row kernel is `amar_sage_layer_agg_f32`.
    max / min   `amar_sage_layer_agg_f32` where F in {4, 8, 16, 32}, C <= 64, else `amar_sage_aggregate_f32` + the tail — at
          every graph size: the tiled walks are built on addition and are not ported.

Spektral is not installed here, so these points are explicit switches: the added self loop
(``self_loops``), the concat order ``[x, agg]`` and normalise-before-activation (fixed).  One stated deviation: a row
without entries (an isolated node under ``self_loops=False``) aggregates to 0 under every aggregator, as the mean does;
tf.math.unsorted_segment_max would fill it with the lowest float and make the layer's output meaningless.
"""
import torch

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd.engine import Layer
from deep_cbrs_amar_renaissance_amd.utilities.math import spmm_kind


class GraphSageConv(Layer):
    AGGREGATES = ('mean', 'sum', 'max', 'min')

    def __init__(self, channels, aggregate='mean', activation=None, use_bias=True, kernel_regularizer=None,
                 bias_regularizer=None, self_loops=True, **kwargs):
        super().__init__()
        if aggregate not in self.AGGREGATES:
            raise NotImplementedError("aggregate={!r}: the HIP GraphSAGE layer has kernels for {}".format(
                aggregate, ', '.join(repr(v) for v in self.AGGREGATES)))
        if activation != 'relu' or not use_bias:
            raise NotImplementedError("the HIP GraphSAGE layer is built for activation='relu', use_bias=True")
        self.channels, self.aggregate, self.self_loops = channels, aggregate, self_loops
        self.kernel_regularizer, self.bias_regularizer = kernel_regularizer, bias_regularizer
        self.kernel = self.bias = None

    def build(self, input_shape):
        f_in = input_shape[0][-1]
        self.kernel = self.add_weight('kernel', (2 * f_in, self.channels), 'glorot_uniform', self.kernel_regularizer)
        self.bias = self.add_weight('bias', (self.channels,), 'zeros', self.bias_regularizer)

    def _inv_count(self, a):
        """1 / (edges into the node (+1 with the self loop)); 0 for an empty segment, as unsorted_segment_mean yields."""
        cache = a.__dict__.setdefault('_sage_inv_count', {})
        if self.self_loops not in cache:
            deg = (a.rowptr[1:] - a.rowptr[:-1]).to(torch.float32)
            inv = 1.0 / (deg + 1.0) if self.self_loops else torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))
            cache[self.self_loops] = inv.contiguous()
        return cache[self.self_loops]

    def row_scale(self, a):
        """What the row's sum is multiplied by: 1 / count for 'mean', 1 for 'sum' (cached on the graph; the training tape reads it too)."""
        if self.aggregate == 'mean':
            return self._inv_count(a)
        if '_sage_ones' not in a.__dict__:
            a.__dict__['_sage_ones'] = torch.ones(a.shape[0], dtype=torch.float32, device=a.rowptr.device)
        return a.__dict__['_sage_ones']

    def _image(self, a, f):
        return a.tiled_mean_image(f, self.self_loops) if self.aggregate == 'mean' else a.tiled_sum_image(f, self.self_loops)

    def wants_dense_input(self, a, f):
        """Whether the layer gathers on the LDS-tiled image with the fused tail: its input then should be a dense [n, f] table
        (a column slice of the concatenation buffer spreads four 32-byte rows over three 128-byte lines instead of one:
        ml1m(s=64) 0.31 against 0.25 ms per layer) and `dense_out` is filled by the same launch."""
        if self.aggregate in ('max', 'min') or spmm_kind(a, f) != 'xs' or f != self.channels or f not in (8, 16, 32):
            return False
        from deep_cbrs_amar_renaissance_amd.utilities.lds_tiled import LdsTiled
        return isinstance(self._image(a, f), LdsTiled)

    def call(self, inputs, out=None, dense_out=None, **kwargs):
        """dense_out: an optional dense [n, channels] buffer that receives a second copy of the result."""
        self._dense_filled = False
        y = self._call(inputs, out, dense_out)
        if dense_out is not None and not self._dense_filled:
            capi.copy_columns(y, dense_out)
        return y

    def _call(self, inputs, out, dense_out):
        x, a = inputs
        if a.vals is not None:
            raise ValueError("GraphSageConv expects the raw edge list (DeviceCSR without values)")
        n, f = a.shape[0], x.shape[1]
        if out is None:
            out = torch.empty((n, self.channels), dtype=torch.float32, device=x.device)
        if self.aggregate in ('max', 'min'):
            return self._call_extremum(x, a, n, f, out)
        kind = spmm_kind(a, f)
        if kind != 'xs' and f in (4, 8, 16, 32) and self.channels <= 64:
            if self.aggregate == 'mean':
                capi.sage_layer(a.rowptr, a.colidx, x, self.kernel, self.bias, out, self_loop=self.self_loops)
            else:
                capi.sage_layer_agg(a.rowptr, a.colidx, x, self.kernel, self.bias, out, 'sum', self_loop=self.self_loops)
            return out
        if kind == 'xs' and f == self.channels and f in (8, 16, 32):
            from deep_cbrs_amar_renaissance_amd.utilities.lds_tiled import LdsTiled
            img = self._image(a, f)
            if isinstance(img, LdsTiled) and capi.sage_tail_on_lt_supported(x, f):     # (a span of 2^32 bytes and more: two launches)
                # mean / sum aggregate and the layer's tail in ONE launch: the tile's sums never leave the workgroup
                capi.spmm_lt(img, x, out, prescaled=True, sage_tail=(self.kernel, self.bias), Hnext=dense_out)
                self._dense_filled = dense_out is not None
                return out
        fused_tail = capi.sage_tail_supported(f, self.channels)
        xa = torch.empty((n, f if fused_tail else 2 * f), dtype=torch.float32, device=x.device)
        agg = xa if fused_tail else xa[:, f:]
        if kind == 'xs':
            capi.spmm_xs(self._image(a, f), x, agg, prescaled=True)
        else:
            # widths the fused row kernel is not instantiated for (TwoStep / TwoWay 'concatenation' hand-over, 24 / 48):
            # neighbour sum as column chunks of the value-free SpMM, then (sum + own row) / count ('sum': / 1)
            capi.spmm_csr(a.rowptr, a.colidx, None, x, agg)
            capi.row_affine(agg, self.row_scale(a), agg, b=x if self.self_loops else None)
        return self._tail(x, xa, agg, fused_tail, n, f, out)

    def _call_extremum(self, x, a, n, f, out):
        """max / min: the fused row kernel, else the aggregate kernel + tail, whatever spmm_kind says (no tiled walk for them)."""
        if capi.sage_agg_layer_supported(f, self.channels):
            capi.sage_layer_agg(a.rowptr, a.colidx, x, self.kernel, self.bias, out, self.aggregate, self_loop=self.self_loops)
            return out
        if f % 4 or f > 64:
            raise NotImplementedError("aggregate={!r} needs an input width that is a multiple of 4, at most 64 (got {})".format(self.aggregate, f))
        fused_tail = capi.sage_tail_supported(f, self.channels)
        xa = torch.empty((n, f if fused_tail else 2 * f), dtype=torch.float32, device=x.device)
        agg = xa if fused_tail else xa[:, f:]
        capi.sage_aggregate(a.rowptr, a.colidx, x, agg, self.aggregate, self_loop=self.self_loops)
        return self._tail(x, xa, agg, fused_tail, n, f, out)

    def _tail(self, x, xa, agg, fused_tail, n, f, out):
        if fused_tail:
            capi.sage_tail(x, agg, self.kernel, self.bias, out)    # [x || agg] . W + b, l2-normalise, ReLU in one pass
            return out
        capi.copy_columns(x, xa[:, :f])
        z = torch.empty((n, self.channels), dtype=torch.float32, device=x.device)
        capi.dense(xa, self.kernel, self.bias, z, act=None)
        nrm = torch.empty_like(z)
        inv = torch.empty(n, dtype=torch.float32, device=x.device)
        capi.l2norm_fwd(z, nrm, inv, out, act='relu')
        return out

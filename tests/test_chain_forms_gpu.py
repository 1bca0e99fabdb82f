"""Every kernel form of the fused scoring chain (amar_chain_f32 / amar_chain_indexed_f32 / amar_chain_segments_f32) against float64
(tests/chain_ref.py), at the smallest shapes that select each form (pytest -m gpu).

Each case first ASKS the launcher's own route function (capi.chain_route) and asserts the kernel instantiation it claims to test, then
runs the kernel, then holds every element to the bound chain_ref carries through the layers (derived from float32 summation and the
header's split-product figure; the sigmoid evaluation term comes from numpy's float32 error; nothing is measured on the kernels).
Outputs start as NaN inside a wider buffer whose guard columns (4 on each side of a [P, N] block; the two neighbours of a score column
in a [P, 3] buffer) must keep their sentinel; tables are alternately contiguous or column slices of NaN-padded wider buffers; with ids
the tables are views that start `base` rows into their buffers.  The cases and their draws live in chain_ref (the CPU suite checks the
same routes with made-up addresses and that numpy's float32 evaluation of every case satisfies its bound).

Kernel instantiation                                   reached by (each asserts the route)
  chain_kernel<M, 2, FULL, AM>  M = 3 | 4 | 8,          test_generic_forms[generic-M-{full|part}-amAM-v0 .. v3]   (18 forms x 4 calls:
      FULL = true | false, AM = 0 | 1 | 2                 with / without a 1-unit layer, ids, a second table; AM = 0 by a sigmoid hidden
                                                          layer (v1), a linear hidden layer (v2), sum_inputs with in_act none (v0) and
                                                          sigmoid (v3); P = 1 .. 129)
  chain_kernel<3, 2, false, 1>, <3, 2, false, 0>        test_generic_forms[generic-width30-*]        hidden widths 30 and 22
  chain_kernel<3, 2, false, 1>  second trip             test_generic_forms[generic-second-trip]      P = 4 096 x 128 + 45
  chain_kernel<3 | 4, 2, true, 1>  with out_index       test_pipe_forms[pipe-*-vector-indexed]       the pair-stage shape without a 1-unit
                                                                                                     layer, indexed
  chain_pipe_kernel<3, 2, false, true>                  test_pipe_forms[pipe-3-split-dot], [pipe-3-split-dot-linear], [pipe-3-split-vector]
  chain_pipe_kernel<3, 2, true,  true>                  test_pipe_forms[pipe-3-split-dot-indexed], [pipe-3-split-dot-sigmoid-indexed]
  chain_pipe_kernel<3, 2, false, false>                 test_pipe_forms[pipe-3-f32-dot], [pipe-3-f32-dot-linear], [pipe-3-f32-vector]
  chain_pipe_kernel<3, 2, true,  false>                 test_pipe_forms[pipe-3-f32-dot-indexed], [pipe-3-f32-dot-sigmoid-indexed]
  chain_pipe_kernel<4, 2, false, true>                  test_pipe_forms[pipe-4-split-dot], [pipe-4-split-dot-linear], [pipe-4-split-vector]
  chain_pipe_kernel<4, 2, true,  true>                  test_pipe_forms[pipe-4-split-dot-indexed], [pipe-4-split-dot-sigmoid-indexed]
  chain_pipe_kernel<4, 2, false, false>                 test_pipe_forms[pipe-4-f32-dot], [pipe-4-f32-dot-linear], [pipe-4-f32-vector]
  chain_pipe_kernel<4, 2, true,  false>                 test_pipe_forms[pipe-4-f32-dot-indexed], [pipe-4-f32-dot-sigmoid-indexed]
      (-dot, -dot-indexed and -vector loop: P = 1 536 x 128 + 45 and 2 x 1 536 x 128 + 77, the third trip with ids clamped two strides
      ahead; -dot-linear and -dot-sigmoid-indexed take the second trip; a sigmoid and a linear 1-unit layer each plain and indexed)
  chain_rows_kernel<S, 2, LASTLIN, false>               test_rows_forms[rows-<widths>-{relu|lin}[-ids]]  S = 24-24-24-48, 48-48-48-64,
      six shapes x LASTLIN = false | true                 24-24-24, 8-24-24-48, 16-48-48-64, 48-48-48 with full tiles and with partly
                                                          filled first / last tiles (Da 20 / 36 / 12, n_out 40 / 52 / 20 / 36 / 60); the
                                                          -ids cases with partly filled tiles loop (P = 1 024 x 128 + 45)
  chain_rows_kernel<S, 2, LASTLIN, true>                test_rows_forms[seg-8+12-24-24-40-*], [seg-16+16+16-48-48-64-*], [seg-8+8+8-24-24-*],
      six shapes x LASTLIN                                [seg-4+4-24-24-48-*], [seg-8+8-48-48-64-*], [seg-16+16+16-48-48-*]   (in the order
                                                          of S above; boundaries inside a tile and across tiles; the second table is a
                                                          row slice of a longer buffer; the -ids ones loop)
All 50 instantiations are reached.

Bit-for-bit relations the source promises (torch.equal): the f32 pipe form and the rows kernel equal the generic kernel (forced by an
identity out_index, on pre-gathered, pre-summed rows for the pair stage); an indexed call equals the plain call scattered; SEG equals the
assembled table.  The split form is bounded with c_K = K + 5 and, on the long lists, held to "no less accurate on average than the f32
evaluation" (test_pair_stage_split_products_against_f32_and_f64's relation).
"""
import numpy as np
import pytest
import torch

from tests import chain_ref as cr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
SENTINEL = 7.0
GUARD = 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(arr, padded, base, lead=0):
    """A device view of `arr` starting `base` rows in: contiguous, or (padded) columns GUARD.. of a NaN-filled buffer 2 GUARD wider
    (and `lead` rows longer at the top)."""
    rows, w = arr.shape
    if not padded:
        return _dev(arr)[base:]
    buf = torch.full((rows + lead, w + 2 * GUARD), NAN, dtype=torch.float32, device=DEV)
    view = buf[lead:, GUARD:GUARD + w]
    view.copy_(_dev(arr))
    return view[base:]


class Operands:
    """The device operands of one chain_ref case."""

    def __init__(self, hip, case):
        self.hip, self.case, self.d = hip, case, case.draw()
        d = self.d
        blob, dims = hip.chain_pack(d['ks'], d['bs'])
        assert dims == case.dims and np.array_equal(blob, cr.pack(d['ks'], d['bs']))
        self.blob = _dev(blob)
        self.A = _table(d['A'], case.padded, case.base_a)
        self.B = _table(d['B'], not case.padded, case.base_b) if case.Db else None
        if case.seg:                                                     # per-layer tables: own leading dimensions, the second a row slice
            offs = np.cumsum([0] + case.seg)
            self.assembled = self.A
            self.A = hip.ConcatTable([_table(d['A'][:, offs[j]:offs[j + 1]], j != 0, case.base_a, lead=5 if j == 1 else 0) for j in range(len(case.seg))])
        self.ia = _dev(d['ia']) if case.ids else None
        self.ib = _dev(d['ib']) if case.ids and case.Db else None
        self.Pmax = max(case.Ps)
        self.want, self.bound = {}, {}

    def reference(self, split):
        """(want, bound) for the largest P, in the order of the list; a shorter list is its first rows."""
        if split not in self.want:
            terms = []
            self.want[split], self.bound[split] = self.case.reference(self.d, self.Pmax, split=split, terms=terms)
            assert all(0 < t < cr.SIGMOID_LIMIT for t in terms), (self.case, terms)          # the sigmoid evaluation terms of THIS bound
        return self.want[split], self.bound[split]

    def perm(self, P):
        """A permutation of 0..P-1 for the output index of a list of P rows."""
        return np.argsort(self.d['perm'][:P], kind='stable').astype(np.int32)

    def output(self, P):
        """(buffer, view): a NaN [P, N] block inside sentinel guard columns, or a NaN score column between two sentinel columns."""
        n = 1 if self.case.has_dot else self.case.dims[-1]
        g = 1 if self.case.has_dot else GUARD
        buf = torch.full((P, n + 2 * g), SENTINEL, dtype=torch.float32, device=DEV)
        view = buf[:, g:g + n]
        view.fill_(NAN)
        return buf, view

    def call(self, P, expect, out_index=None, A=None, plain=False):
        """Ask the route, assert it, launch; returns (output [P, N] or [P], route).  plain: the rows in order from table A, one table."""
        c = self.case
        buf, out = self.output(P)
        if plain:
            kw = dict(out_index=out_index)
        else:
            kw = dict(ids_a=self.ia[:P] if c.ids else None, base_a=c.base_a, B=self.B, ids_b=self.ib[:P] if self.ib is not None else None,
                      base_b=c.base_b, sum_inputs=c.sum_inputs, in_act=c.in_act, out_index=out_index)
        A = self.A if A is None else A
        route = self.hip.chain_route(A, self.blob, c.dims, c.acts, out, **kw)
        assert {k: route[k] for k in expect} == expect, (c, P, route)
        self.hip.chain(A, self.blob, c.dims, c.acts, out, **kw)
        torch.cuda.synchronize()
        g = (buf.shape[1] - out.shape[1]) // 2
        assert bool((buf[:, :g] == SENTINEL).all()) and bool((buf[:, g + out.shape[1]:] == SENTINEL).all()), '{} P={}: a store outside the output'.format(c, P)
        res = out.contiguous()
        return (res.view(-1) if c.has_dot else res), route

    def check(self, got, P, split, what, perm=None):
        """Every element of the device result within its bound (row p of the list sits in row perm[p])."""
        want, bound = self.reference(split)
        got = got.cpu().numpy()
        cr.assert_within(got[perm] if perm is not None else got, want[:P], bound[:P], '{} P={} {}'.format(self.case, P, what))

    def summed_rows(self, P):
        """relu(A[ida] + B[idb]) [P, W] in float32, exactly as the pair stage forms it."""
        c = self.case
        return torch.relu(self.A[(self.ia[:P] - c.base_a).long()] + self.B[(self.ib[:P] - c.base_b).long()]).contiguous()


def _expect(case):
    """The route a case must take (the split products can be switched off for the whole process: then they are not expected)."""
    import os
    e = dict(case.expect)
    if os.environ.get('AMAR_PAIR_MFMA') == 'f32' and 'split' in e:
        e['split'] = False
    return e


@pytest.mark.parametrize('case', cr.generic_cases(), ids=repr)
def test_generic_forms(hip, case):
    ops = Operands(hip, case)
    for P in case.Ps:
        got, route = ops.call(P, _expect(case))
        assert route['blocks'] == min(-(-P // 128), 4096) and route['lds_bytes'] == 4 * cr.pack_floats(case.dims)
        ops.check(got, P, False, 'generic')


@pytest.mark.parametrize('case', cr.pipe_cases(), ids=repr)
def test_pipe_forms(hip, case):
    ops = Operands(hip, case)
    expect = _expect(case)
    generic = dict(kernel=cr.GENERIC, maxt=expect['maxt'], full=True, am=1, has_dot=case.has_dot)
    for P in case.Ps:
        perm = ops.perm(P) if case.out_index else None
        got, route = ops.call(P, expect, out_index=_dev(perm) if case.out_index else None)
        split = bool(route['split'])
        if route['kernel'] == cr.PIPE:
            assert route['blocks'] == min(-(-P // 128), 1536) and route['scatter'] == case.out_index
        ops.check(got, P, split, 'split' if split else 'f32', perm)
        listed = got[torch.from_numpy(perm).long().to(DEV)] if case.out_index else got         # back in the order of the list
        # the generic kernel on pre-gathered, pre-summed rows (an identity out_index keeps the tower kernel away): the exact f32 chain
        x = ops.summed_rows(P)
        f32, _ = ops.call(P, generic, out_index=torch.arange(P, device=DEV, dtype=torch.int32), A=x, plain=True)
        ops.check(f32, P, False, 'generic on summed rows')
        if not split:
            assert torch.equal(listed, f32), '{} P={}: the f32 form differs from the generic kernel'.format(case, P)
        elif P > 100000:
            want = torch.from_numpy(ops.reference(True)[0][:P]).to(DEV)
            e_split, e_f32 = (listed.double() - want).abs(), (f32.double() - want).abs()
            print('{} P={}: mean error split {:.3e}, f32 {:.3e}'.format(case, P, float(e_split.mean()), float(e_f32.mean())))
            assert float(e_split.mean()) < 1.5 * float(e_f32.mean()) + 1e-9
        if case.out_index and route['kernel'] == cr.PIPE:                 # the indexed call against the plain call, scattered
            plain, _ = ops.call(P, dict(expect, scatter=False))
            assert torch.equal(listed, plain), '{} P={}: the indexed call differs from the plain one'.format(case, P)


@pytest.mark.parametrize('case', cr.rows_cases(), ids=repr)
def test_rows_forms(hip, case):
    ops = Operands(hip, case)
    expect = _expect(case)
    generic = dict(kernel=cr.GENERIC, maxt=4 if max(case.dims) > 48 else 3, am=expect['am'], has_dot=False)
    for P in case.Ps:
        got, route = ops.call(P, expect)
        assert route['blocks'] == min(-(-P // 128), 1024) and route['lds_bytes'] == 4 * cr.pack_floats(case.dims)
        ops.check(got, P, False, 'rows')
        table = ops.assembled if case.seg else ops.A
        gen, _ = ops.call(P, generic, out_index=torch.arange(P, device=DEV, dtype=torch.int32), A=table)
        assert torch.equal(got, gen), '{} P={}: the tower kernel differs from the generic kernel'.format(case, P)
        if case.seg:
            whole, _ = ops.call(P, dict(expect, seg=False), A=table)
            assert torch.equal(got, whole), '{} P={}: the tables read in place differ from the assembled table'.format(case, P)

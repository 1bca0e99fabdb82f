"""Reference for the fused scoring chain (amar_chain_f32 / amar_chain_indexed_f32 / amar_chain_segments_f32).  TEST INFRASTRUCTURE ONLY.

numpy float64, written from the formula of include/amar_hip.h:
    x = [ A[ra] || B[rb] ]      or, with sum_inputs,      x = in_act( A[ra] + B[rb] )            ra / rb = ids - base, or the row itself
    x = act_l( x . W_l + b_l )  for every layer;  a trailing 1-unit layer (after at least one other layer) is the `dot`: out is [P]
on the float32 operands widened exactly, together with the per-element bound tests/test_chain_forms_gpu.py holds the kernels to.  Nothing
in `evaluate` rounds to float32.  U = 2^-24 (tests/dense_bwd_ref.py).

The bound, carried layer by layer (e = bound on |device x - float64 x|):
    input   e_0 = 0 for the concatenation (the rows are copied);  e_0 = L_act U |a + b| for the summed input (one float32 addition)
    layer   e_{l+1} = L_act ( |W|^T e_l + c_K U ( |x| |W| + |b| ) )
            L_act = 1 for none / relu (1-Lipschitz, exact), 1/4 for sigmoid (its largest slope)
            c_K = K + 2: K products and K additions (the bias among them) in float32, any order: gamma_{K+1} < (K + 2) U, as
                  tests/dense_stack_ref.py takes it.  The 1-unit layer is such a sum too (fmaf chain of K / 4 terms per lane, two cross-lane
                  additions, the bias).
            c_K = K + 5 for the layers of the split-product pair stage: csrc/amar_chain.hip derives "a term x.w is off by at most
                  3 . 2^-24 |x.w|" for the six part products it keeps, on top of the float32 accumulation.  Its 1-unit layer is float32: K + 2.
    sigmoid additionally carries the error of EVALUATING 1 / (1 + exp(-z)) in float32, which is no multiple of U (expf is accurate to an
            ulp or two, not correctly rounded).  `sigmoid_term(z)`: the worst |float32 numpy evaluation - float64 evaluation| of that
            expression over the case's own pre-activations z (rounded to float32 first, so both see the same argument), times
            SIGMOID_MARGIN = 4 because the device's expf and numpy's may differ by a few ulp.  Every term must stay below the 1e-6 the
            suite already holds sigmoid scores to (_check_scores in tests/test_entry_points_gpu.py): the CPU and the GPU tests assert it
            of every term they use.  Where the tests were written the worst float32 numpy error over the pre-activations of every case of
            `all_cases()` was 8.73e-8 (tests/test_chain_route_cpu.py measures it on the CPU), so the largest term was 3.5e-7; the figure
            depends on the numpy build's exp, which is why only the limit is asserted.
Elements whose bound is 0 must match exactly (`assert_within`).  No figure here was measured on the kernels under test;
tests/test_chain_route_cpu.py checks that the float32 numpy evaluation (`evaluate_f32`) of every GPU case stays inside its bound, so the
reference alone satisfies it.

Draws (`draw`): Glorot-uniform kernels and biases U(+-0.2), as entry_point_ref.draw_dual_head; tables N(0, 1.5^2): entries of a few units.

`pack` / `pack_floats` restate the blob layout from the comment above amar_chain_pack_f32:
    W_p[m][t][lane][r] = W[16 t + 4 (lane >> 4) + r][16 m + (lane & 15)], zero outside the matrix, then the bias padded to 16 NT;
    a trailing 1-unit layer (after at least one other): 16 KT weights (zero padded), then bias, 0, 0, 0.

`all_cases()` lists what tests/test_chain_forms_gpu.py runs: every case names the kernel instantiation it must reach (`expect`, compared
with amar_chain_route before anything is launched; the CPU test asks the same question with made-up addresses).
"""
import zlib

import numpy as np

from deep_cbrs_amar_renaissance_amd.capi import chain_shape
from tests.dense_bwd_ref import U

SIGMOID_MARGIN = 4.0
SIGMOID_LIMIT = 1e-6                                                   # _check_scores' figure: every sigmoid term must stay below it
GENERIC, PIPE, ROWS = 0, 1, 2
TABLE_ROWS = 300


def tiles16(n):
    return (n + 15) // 16


def has_dot(dims):
    return len(dims) > 2 and dims[-1] == 1


# ---- the pack layout -------------------------------------------------------------------------------------------------------------------
def pack_floats(dims):
    total = 0
    for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
        if l == len(dims) - 2 and n == 1 and l > 0:
            total += 16 * tiles16(k) + 4
        else:
            total += tiles16(n) * tiles16(k) * 256 + 16 * tiles16(n)
    return total


def pack(ks, bs):
    """The blob of amar_chain_pack_f32 for kernels ks[l] [K_l, N_l] and biases bs[l] [N_l] (float32 in, float32 out)."""
    parts = []
    for l, (w, b) in enumerate(zip(ks, bs)):
        k, n = w.shape
        kt, nt = tiles16(k), tiles16(n)
        if l == len(ks) - 1 and n == 1 and l > 0:
            v = np.zeros(16 * kt + 4, np.float32)
            v[:k] = w[:, 0]
            v[16 * kt] = b[0]
            parts.append(v)
            continue
        wp = np.zeros((16 * kt, 16 * nt), np.float32)
        wp[:k, :n] = w
        # row 16 t + 4 g + r, column 16 m + c  ->  [m][t][lane = 16 g + c][r]
        parts.append(wp.reshape(kt, 4, 4, nt, 16).transpose(3, 0, 1, 4, 2).reshape(-1))
        bp = np.zeros(16 * nt, np.float32)
        bp[:n] = b
        parts.append(bp)
    return np.concatenate(parts)


# ---- the chain in float64 with its bound, and in float32 ----------------------------------------------------------------------------------
def _act64(z, name):
    if name is None:
        return z
    if name == 'relu':
        return np.maximum(z, 0)
    if name == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-z))
    raise ValueError(name)


def _act32(z, name):
    assert z.dtype == np.float32
    one = np.float32(1)
    if name is None:
        return z
    if name == 'relu':
        return np.maximum(z, np.float32(0))
    if name == 'sigmoid':
        with np.errstate(over='ignore'):
            return one / (one + np.exp(-z))
    raise ValueError(name)


def sigmoid_f32_error(z):
    """Worst |float32 numpy sigmoid - float64 sigmoid| over the pre-activations z, both evaluated at float32(z)."""
    z32 = np.asarray(z, dtype=np.float64).astype(np.float32)
    got = _act32(z32, 'sigmoid')
    assert got.dtype == np.float32
    return float(np.abs(got.astype(np.float64) - _act64(z32.astype(np.float64), 'sigmoid')).max()) if z32.size else 0.0


def sigmoid_term(z):
    return SIGMOID_MARGIN * sigmoid_f32_error(z)


def _through(z, e, name, terms):
    """(act(z), bound behind the activation); `terms` collects the sigmoid evaluation terms used."""
    if name == 'sigmoid':
        t = sigmoid_term(z)
        terms.append(t)
        return _act64(z, name), 0.25 * e + t
    return _act64(z, name), e


def _unique_rows(ra, rb):
    """Pairs (ra, rb) -> (unique ra, unique rb, inverse): a long list over small tables is evaluated once per distinct pair."""
    if rb is None:
        u, inv = np.unique(ra, return_inverse=True)
        return u, None, inv.reshape(-1)
    key = ra.astype(np.int64) * (int(rb.max()) + 1) + rb.astype(np.int64)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    return ra[first], rb[first], inv.reshape(-1)


def evaluate(A, B, ra, rb, sum_inputs, in_act, ks, bs, acts, split=False, terms=None):
    """(want, bound) in float64: [P, N], or [P] behind a trailing 1-unit layer.  A, B: float32 tables (B None: one table); ra, rb: row
    numbers per output row; split: the MFMA layers run on the split products (c_K = K + 5)."""
    terms = [] if terms is None else terms
    ua, ub, inv = _unique_rows(np.asarray(ra), None if B is None else np.asarray(rb))
    a = np.asarray(A, dtype=np.float64)[ua]
    if B is None:
        x, e = a, np.zeros_like(a)
    elif sum_inputs:
        s = a + np.asarray(B, dtype=np.float64)[ub]
        x, e = _through(s, U * np.abs(s), in_act, terms)
    else:
        x = np.concatenate([a, np.asarray(B, dtype=np.float64)[ub]], axis=1)
        e = np.zeros_like(x)
    dims = [ks[0].shape[0]] + [k.shape[1] for k in ks]
    dot = has_dot(dims)
    for l, (w, b, name) in enumerate(zip(ks, bs, acts)):
        w64, b64 = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
        k = w64.shape[0]
        c = k + 5 if split and not (dot and l == len(ks) - 1) else k + 2
        z = x @ w64 + b64
        ez = e @ np.abs(w64) + c * U * (np.abs(x) @ np.abs(w64) + np.abs(b64))
        x, e = _through(z, ez, name, terms)
    if dot:
        x, e = x[:, 0], e[:, 0]
    return x[inv], e[inv]


def evaluate_f32(A, B, ra, rb, sum_inputs, in_act, ks, bs, acts):
    """The same chain in numpy float32."""
    a = np.asarray(A, dtype=np.float32)[ra]
    if B is None:
        x = a
    elif sum_inputs:
        x = _act32(a + np.asarray(B, dtype=np.float32)[rb], in_act)
    else:
        x = np.concatenate([a, np.asarray(B, dtype=np.float32)[rb]], axis=1)
    for w, b, name in zip(ks, bs, acts):
        x = _act32(x @ w + b, name)
    assert x.dtype == np.float32
    dims = [ks[0].shape[0]] + [k.shape[1] for k in ks]
    return x[:, 0] if has_dot(dims) else x


def assert_within(got, want, bound, what=''):
    """Every element within its bound; elements whose bound is 0 exactly equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), '{}: {} non-finite elements'.format(what, int((~np.isfinite(got)).sum()))
    zero = bound == 0
    assert np.array_equal(got[zero], want[zero]), '{}: an element with bound 0 differs'.format(what)
    err = np.abs(got - want)
    bad = err > bound
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    print('{}: worst |got - want| / bound = {:.3f} over {} elements'.format(what, float(ratio.max()) if ratio.size else 0.0, ratio.size))
    if bad.any():
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError('{}: {} of {} elements outside their bound; worst {:.3g} x bound at {} (got {!r}, want {!r}, bound {:.3g})'.format(
            what, int(bad.sum()), bad.size, float(ratio[at]), at, float(got[at]), float(want[at]), float(bound[at])))


# ---- the cases of tests/test_chain_forms_gpu.py ---------------------------------------------------------------------------------------
SMALL_P = (1, 15, 16, 17, 31, 33, 127, 129)
GENERIC_LOOP_P = 4096 * 128 + 45                                       # second trip of the generic kernel's 4 096 workgroups, ragged end
PIPE_P = (1, 16, 17, 33, 129)
PIPE_LOOP_P = (1536 * 128 + 45, 2 * 1536 * 128 + 77)                   # second and third trip of the pipe kernel's 1 536 workgroups
ROWS_P = (1, 16, 17, 129)
ROWS_LOOP_P = 1024 * 128 + 45                                          # second trip of the rows kernel's 1 024 workgroups


class Case:
    """One stack and how it is called.  expect: the fields of amar_chain_route_info it must give (for every P of `Ps`)."""

    def __init__(self, name, Da, Db, units, acts, expect, Ps, sum_inputs=False, in_act=None, ids=True, out_index=False, seg=None, padded=False):
        self.name, self.Da, self.Db, self.units, self.acts, self.expect, self.Ps = name, Da, Db, list(units), list(acts), dict(expect), tuple(Ps)
        self.sum_inputs, self.in_act, self.ids, self.out_index, self.seg, self.padded = sum_inputs, in_act, ids, out_index, seg, padded
        self.dims = [Da if sum_inputs else Da + Db] + self.units
        self.base_a, self.base_b = (7, 11) if ids else (0, 0)
        self.has_dot = has_dot(self.dims)
        assert len(self.acts) == len(self.units) and (not sum_inputs or Da == Db)

    def __repr__(self):
        return self.name

    def draw(self):
        """Seeded operands (numpy): A, B with base_* extra leading rows, kernels, biases, ids / perm for the largest P."""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        P = max(self.Ps)
        d = {'A': (rng.standard_normal((TABLE_ROWS + self.base_a, self.Da)) * 1.5).astype(np.float32),
             'B': (rng.standard_normal((TABLE_ROWS + self.base_b, self.Db)) * 1.5).astype(np.float32) if self.Db else None}
        d['ks'] = [rng.uniform(-1, 1, (k, n)).astype(np.float32) * np.float32(np.sqrt(6.0 / (k + n))) for k, n in zip(self.dims[:-1], self.dims[1:])]
        d['bs'] = [rng.uniform(-0.2, 0.2, n).astype(np.float32) for n in self.dims[1:]]
        if self.ids:
            d['ia'] = rng.integers(self.base_a, TABLE_ROWS + self.base_a, P).astype(np.int32)
            d['ib'] = rng.integers(self.base_b, TABLE_ROWS + self.base_b, P).astype(np.int32)
        else:
            assert P <= TABLE_ROWS
            d['ia'] = d['ib'] = None
        d['perm'] = rng.permutation(P).astype(np.int32) if self.out_index else None
        return d

    def rows(self, d, P):
        """(ra, rb): the table rows (of the FULL arrays d['A'], d['B']) that output rows 0..P-1 read."""
        if self.ids:
            return d['ia'][:P].astype(np.int64), d['ib'][:P].astype(np.int64)
        return np.arange(P), np.arange(P)

    def reference(self, d, P, split=None, terms=None):
        ra, rb = self.rows(d, P)
        split = bool(self.expect.get('split')) if split is None else split
        return evaluate(d['A'], d['B'], ra, rb, self.sum_inputs, self.in_act, d['ks'], d['bs'], self.acts, split=split, terms=terms)

    def reference_f32(self, d, P):
        ra, rb = self.rows(d, P)
        return evaluate_f32(d['A'], d['B'], ra, rb, self.sum_inputs, self.in_act, d['ks'], d['bs'], self.acts)


# (name, maxt, full, am, Da, Db, units, acts, how it is called): four calls per instantiation — with and without a trailing 1-unit layer
# (am = 2 has none), with and without ids, one table and two.  am = 0 through each of its causes: sum_inputs with in_act none (v0) and
# sigmoid (v3), a sigmoid hidden layer (v1), a linear layer before the last (v2).  A stack of three ReLU layers or fewer over ONE table
# without a 1-unit layer would take the tower kernel where its tile counts are a tower shape: those calls are four layers deep at 48.
GENERIC_TABLE = [
    # chain_kernel<3, 2, true, 0>
    ('generic-3-full-am0-v0', 3, True, 0, 48, 48, [48, 1], ['relu', 'sigmoid'], dict(sum_inputs=True, in_act=None)),
    ('generic-3-full-am0-v1', 3, True, 0, 48, 0, [48, 48, 1], ['sigmoid', 'relu', None], dict(ids=False, padded=True)),
    ('generic-3-full-am0-v2', 3, True, 0, 48, 0, [48, 48, 48, 48], [None, 'relu', 'relu', 'relu'], dict()),
    ('generic-3-full-am0-v3', 3, True, 0, 48, 48, [48, 48], ['relu', 'relu'], dict(sum_inputs=True, in_act='sigmoid', ids=False, padded=True)),
    # chain_kernel<3, 2, true, 1>
    ('generic-3-full-am1-v0', 3, True, 1, 24, 24, [48, 1], ['relu', 'relu'], dict()),
    ('generic-3-full-am1-v1', 3, True, 1, 48, 0, [48, 1], ['relu', 'sigmoid'], dict(ids=False, padded=True)),
    ('generic-3-full-am1-v2', 3, True, 1, 48, 0, [48, 48, 48, 48], ['relu', 'relu', 'relu', 'relu'], dict()),
    ('generic-3-full-am1-v3', 3, True, 1, 24, 24, [48, 48], ['relu', 'relu'], dict(ids=False, padded=True)),
    # chain_kernel<3, 2, true, 2>
    ('generic-3-full-am2-v0', 3, True, 2, 24, 24, [48, 48], ['relu', None], dict()),
    ('generic-3-full-am2-v1', 3, True, 2, 48, 0, [48, 48, 48, 48], ['relu', 'relu', 'relu', None], dict(padded=True)),
    ('generic-3-full-am2-v2', 3, True, 2, 48, 0, [48, 48, 48, 48], ['relu', 'relu', 'relu', None], dict(ids=False)),
    ('generic-3-full-am2-v3', 3, True, 2, 24, 24, [48, 48], ['relu', None], dict(ids=False, padded=True)),
    # chain_kernel<3, 2, false, 0>
    ('generic-3-part-am0-v0', 3, False, 0, 36, 36, [20, 48, 1], ['relu', 'relu', None], dict(sum_inputs=True, in_act=None)),
    ('generic-3-part-am0-v1', 3, False, 0, 36, 0, [20, 48, 1], ['sigmoid', 'relu', 'relu'], dict(ids=False, padded=True)),
    ('generic-3-part-am0-v2', 3, False, 0, 36, 0, [20, 48], [None, 'relu'], dict()),
    ('generic-3-part-am0-v3', 3, False, 0, 36, 36, [20, 48], ['relu', 'relu'], dict(sum_inputs=True, in_act='sigmoid', ids=False, padded=True)),
    # chain_kernel<3, 2, false, 1>
    ('generic-3-part-am1-v0', 3, False, 1, 20, 16, [20, 48, 1], ['relu', 'relu', 'sigmoid'], dict()),
    ('generic-3-part-am1-v1', 3, False, 1, 36, 0, [20, 48, 1], ['relu', 'relu', None], dict(ids=False, padded=True)),
    ('generic-3-part-am1-v2', 3, False, 1, 36, 0, [20, 48], ['relu', 'relu'], dict()),
    ('generic-3-part-am1-v3', 3, False, 1, 20, 16, [20, 48], ['relu', 'relu'], dict(ids=False, padded=True)),
    # chain_kernel<3, 2, false, 2>
    ('generic-3-part-am2-v0', 3, False, 2, 20, 16, [20, 48], ['relu', None], dict()),
    ('generic-3-part-am2-v1', 3, False, 2, 36, 0, [20, 48], ['relu', None], dict(padded=True)),
    ('generic-3-part-am2-v2', 3, False, 2, 36, 0, [20, 48], ['relu', None], dict(ids=False)),
    ('generic-3-part-am2-v3', 3, False, 2, 20, 16, [20, 48], ['relu', None], dict(ids=False, padded=True)),
    # chain_kernel<4, 2, true, 0>
    ('generic-4-full-am0-v0', 4, True, 0, 64, 64, [64, 1], ['relu', 'relu'], dict(sum_inputs=True, in_act=None)),
    ('generic-4-full-am0-v1', 4, True, 0, 64, 0, [64, 64, 1], ['sigmoid', 'relu', 'sigmoid'], dict(ids=False, padded=True)),
    ('generic-4-full-am0-v2', 4, True, 0, 64, 0, [64, 64], [None, 'relu'], dict()),
    ('generic-4-full-am0-v3', 4, True, 0, 64, 64, [64, 64], ['relu', 'relu'], dict(sum_inputs=True, in_act='sigmoid', ids=False, padded=True)),
    # chain_kernel<4, 2, true, 1>
    ('generic-4-full-am1-v0', 4, True, 1, 32, 32, [64, 1], ['relu', None], dict()),
    ('generic-4-full-am1-v1', 4, True, 1, 64, 0, [64, 1], ['relu', 'relu'], dict(ids=False, padded=True)),
    ('generic-4-full-am1-v2', 4, True, 1, 64, 0, [64, 64], ['relu', 'relu'], dict()),
    ('generic-4-full-am1-v3', 4, True, 1, 32, 32, [64, 64], ['relu', 'relu'], dict(ids=False, padded=True)),
    # chain_kernel<4, 2, true, 2>
    ('generic-4-full-am2-v0', 4, True, 2, 32, 32, [64, 64], ['relu', None], dict()),
    ('generic-4-full-am2-v1', 4, True, 2, 64, 0, [64, 64], ['relu', None], dict(padded=True)),
    ('generic-4-full-am2-v2', 4, True, 2, 64, 0, [64, 64], ['relu', None], dict(ids=False)),
    ('generic-4-full-am2-v3', 4, True, 2, 32, 32, [64, 64], ['relu', None], dict(ids=False, padded=True)),
    # chain_kernel<4, 2, false, 0>
    ('generic-4-part-am0-v0', 4, False, 0, 52, 52, [36, 64, 1], ['relu', 'relu', 'sigmoid'], dict(sum_inputs=True, in_act=None)),
    ('generic-4-part-am0-v1', 4, False, 0, 52, 0, [36, 64, 1], ['sigmoid', 'relu', None], dict(ids=False, padded=True)),
    ('generic-4-part-am0-v2', 4, False, 0, 52, 0, [36, 64], [None, 'relu'], dict()),
    ('generic-4-part-am0-v3', 4, False, 0, 52, 52, [36, 64], ['relu', 'relu'], dict(sum_inputs=True, in_act='sigmoid', ids=False, padded=True)),
    # chain_kernel<4, 2, false, 1>
    ('generic-4-part-am1-v0', 4, False, 1, 36, 16, [36, 64, 1], ['relu', 'relu', 'relu'], dict()),
    ('generic-4-part-am1-v1', 4, False, 1, 52, 0, [36, 64, 1], ['relu', 'relu', 'sigmoid'], dict(ids=False, padded=True)),
    ('generic-4-part-am1-v2', 4, False, 1, 52, 0, [36, 64], ['relu', 'relu'], dict()),
    ('generic-4-part-am1-v3', 4, False, 1, 36, 16, [36, 64], ['relu', 'relu'], dict(ids=False, padded=True)),
    # chain_kernel<4, 2, false, 2>
    ('generic-4-part-am2-v0', 4, False, 2, 36, 16, [36, 64], ['relu', None], dict()),
    ('generic-4-part-am2-v1', 4, False, 2, 52, 0, [36, 64], ['relu', None], dict(padded=True)),
    ('generic-4-part-am2-v2', 4, False, 2, 52, 0, [36, 64], ['relu', None], dict(ids=False)),
    ('generic-4-part-am2-v3', 4, False, 2, 36, 16, [36, 64], ['relu', None], dict(ids=False, padded=True)),
    # chain_kernel<8, 2, true, 0>
    ('generic-8-full-am0-v0', 8, True, 0, 128, 128, [128, 1], ['relu', None], dict(sum_inputs=True, in_act=None)),
    ('generic-8-full-am0-v1', 8, True, 0, 128, 0, [128, 128, 1], ['sigmoid', 'relu', 'relu'], dict(ids=False, padded=True)),
    ('generic-8-full-am0-v2', 8, True, 0, 128, 0, [128, 128], [None, 'relu'], dict()),
    ('generic-8-full-am0-v3', 8, True, 0, 128, 128, [128, 128], ['relu', 'relu'], dict(sum_inputs=True, in_act='sigmoid', ids=False, padded=True)),
    # chain_kernel<8, 2, true, 1>
    ('generic-8-full-am1-v0', 8, True, 1, 64, 64, [128, 1], ['relu', 'sigmoid'], dict()),
    ('generic-8-full-am1-v1', 8, True, 1, 128, 0, [128, 1], ['relu', None], dict(ids=False, padded=True)),
    ('generic-8-full-am1-v2', 8, True, 1, 128, 0, [128, 128], ['relu', 'relu'], dict()),
    ('generic-8-full-am1-v3', 8, True, 1, 64, 64, [128, 128], ['relu', 'relu'], dict(ids=False, padded=True)),
    # chain_kernel<8, 2, true, 2>
    ('generic-8-full-am2-v0', 8, True, 2, 64, 64, [128, 128], ['relu', None], dict()),
    ('generic-8-full-am2-v1', 8, True, 2, 128, 0, [128, 128], ['relu', None], dict(padded=True)),
    ('generic-8-full-am2-v2', 8, True, 2, 128, 0, [128, 128], ['relu', None], dict(ids=False)),
    ('generic-8-full-am2-v3', 8, True, 2, 64, 64, [128, 128], ['relu', None], dict(ids=False, padded=True)),
    # chain_kernel<8, 2, false, 0>
    ('generic-8-part-am0-v0', 8, False, 0, 52, 52, [36, 96, 1], ['relu', 'relu', 'relu'], dict(sum_inputs=True, in_act=None)),
    ('generic-8-part-am0-v1', 8, False, 0, 52, 0, [36, 96, 1], ['sigmoid', 'relu', 'sigmoid'], dict(ids=False, padded=True)),
    ('generic-8-part-am0-v2', 8, False, 0, 52, 0, [36, 96], [None, 'relu'], dict()),
    ('generic-8-part-am0-v3', 8, False, 0, 52, 52, [36, 96], ['relu', 'relu'], dict(sum_inputs=True, in_act='sigmoid', ids=False, padded=True)),
    # chain_kernel<8, 2, false, 1>
    ('generic-8-part-am1-v0', 8, False, 1, 36, 16, [36, 96, 1], ['relu', 'relu', None], dict()),
    ('generic-8-part-am1-v1', 8, False, 1, 52, 0, [36, 96, 1], ['relu', 'relu', 'relu'], dict(ids=False, padded=True)),
    ('generic-8-part-am1-v2', 8, False, 1, 52, 0, [36, 96], ['relu', 'relu'], dict()),
    ('generic-8-part-am1-v3', 8, False, 1, 36, 16, [36, 96], ['relu', 'relu'], dict(ids=False, padded=True)),
    # chain_kernel<8, 2, false, 2>
    ('generic-8-part-am2-v0', 8, False, 2, 36, 16, [36, 96], ['relu', None], dict()),
    ('generic-8-part-am2-v1', 8, False, 2, 52, 0, [36, 96], ['relu', None], dict(padded=True)),
    ('generic-8-part-am2-v2', 8, False, 2, 52, 0, [36, 96], ['relu', None], dict(ids=False)),
    ('generic-8-part-am2-v3', 8, False, 2, 36, 16, [36, 96], ['relu', None], dict(ids=False, padded=True)),
]


def generic_cases():
    """The 18 instantiations chain_kernel<MAXT, 2, FULL, AM> (GENERIC_TABLE) at P = 1 .. 129, hidden widths that are no multiple of 4, and
    the second trip of the capped grid."""
    cases = [Case(name, Da, Db, units, acts, dict(kernel=GENERIC, maxt=maxt, full=full, am=am, has_dot=units[-1] == 1), SMALL_P, **kw)
             for name, maxt, full, am, Da, Db, units, acts, kw in GENERIC_TABLE]
    # hidden widths that are no multiple of 4: the padded lanes of a sigmoid layer hold 0.5 and meet zero weights
    cases.append(Case('generic-width30-relu', 16, 8, [30, 1], ['relu', 'sigmoid'], dict(kernel=GENERIC, maxt=3, full=False, am=1, has_dot=True), SMALL_P))
    cases.append(Case('generic-width30-sigmoid', 16, 8, [30, 1], ['sigmoid', None], dict(kernel=GENERIC, maxt=3, full=False, am=0, has_dot=True), SMALL_P,
                      padded=True))
    cases.append(Case('generic-width30-vector', 16, 8, [30, 22, 12], ['sigmoid', 'relu', None], dict(kernel=GENERIC, maxt=3, full=False, am=0, has_dot=False),
                      SMALL_P, ids=False))
    # every workgroup of the capped grid takes a second trip; the last one is ragged
    cases.append(Case('generic-second-trip', 16, 8, [24, 24], ['relu', 'relu'],
                      dict(kernel=GENERIC, maxt=3, full=False, am=1, has_dot=False, blocks=4096), (GENERIC_LOOP_P,), padded=True))
    return cases


def pipe_cases():
    """The 8 instantiations chain_pipe_kernel<MAXT, 2, SCATTER, SPLIT>: SPLIT by depth (one layer at 64 and two at 48 split; two at 64 and
    three at 48 exceed 64 KB with their fragments), SCATTER by out_index; with a sigmoid / linear 1-unit layer and without one (without:
    the plain call only — with out_index it is the generic kernel, `kernel=GENERIC` below)."""
    cases = []
    for maxt, W, depth, split in ((3, 48, 2, True), (3, 48, 3, False), (4, 64, 1, True), (4, 64, 2, False)):
        tag = 'pipe-{}-{}'.format(maxt, 'split' if split else 'f32')
        pipe = dict(kernel=PIPE, maxt=maxt, full=True, am=1, split=split)
        kw = dict(sum_inputs=True, in_act='relu')
        relu = ['relu'] * depth
        dot, vec = dict(pipe, has_dot=True), dict(pipe, scatter=False, has_dot=False)
        # a sigmoid and a linear 1-unit layer, each plain and indexed; the first two take the second and the third trip, the others the second
        cases.append(Case(tag + '-dot', W, W, [W] * depth + [1], relu + ['sigmoid'], dict(dot, scatter=False), PIPE_P + PIPE_LOOP_P, **kw))
        cases.append(Case(tag + '-dot-indexed', W, W, [W] * depth + [1], relu + [None], dict(dot, scatter=True), PIPE_P + PIPE_LOOP_P,
                          out_index=True, padded=True, **kw))
        cases.append(Case(tag + '-dot-linear', W, W, [W] * depth + [1], relu + [None], dict(dot, scatter=False), PIPE_P + PIPE_LOOP_P[:1], padded=True, **kw))
        cases.append(Case(tag + '-dot-sigmoid-indexed', W, W, [W] * depth + [1], relu + ['sigmoid'], dict(dot, scatter=True), PIPE_P + PIPE_LOOP_P[:1],
                          out_index=True, **kw))
        cases.append(Case(tag + '-vector', W, W, [W] * depth, relu, vec, PIPE_P + PIPE_LOOP_P, padded=True, **kw))
        cases.append(Case(tag + '-vector-indexed', W, W, [W] * depth, relu, dict(kernel=GENERIC, maxt=maxt, full=True, am=1, has_dot=False), PIPE_P,
                          out_index=True, **kw))
    return cases


ROWS_SHAPES = (  # dims that fill the tiles, dims with partly filled first / last tiles
    ([24, 24, 24, 48], [20, 24, 24, 40]), ([48, 48, 48, 64], [36, 44, 48, 52]), ([24, 24, 24], [20, 20, 20]),
    ([8, 24, 24, 48], [12, 20, 24, 36]), ([16, 48, 48, 64], [16, 36, 48, 60]), ([48, 48, 48], [36, 48, 40]))
SEG_CASES = (([8, 12], [24, 24, 40]), ([8, 8, 8], [24, 24]), ([16, 16, 16], [48, 48, 64]), ([16, 16, 16], [48, 48]), ([4, 4], [24, 24, 48]),
             ([8, 8], [48, 48, 64]))


def rows_cases():
    """chain_rows_kernel<SHAPE, 2, LASTLIN, SEG>: the six shapes x LASTLIN, full and partly filled tiles, with ids (and a base) and
    without; SEG likewise for all six shapes (segment boundaries inside a 16-wide tile and across tiles)."""
    cases = []
    for k, (fulld, partd) in enumerate(ROWS_SHAPES):
        shape = chain_shape(*[tiles16(w) for w in fulld])
        assert shape == chain_shape(*[tiles16(w) for w in partd])
        for lastlin in (False, True):
            for j, dims in enumerate((fulld, partd)):
                acts = ['relu'] * (len(dims) - 2) + [None if lastlin else 'relu']
                ids = bool((k + j + lastlin) & 1)
                Ps = ROWS_P + ((ROWS_LOOP_P,) if ids and j == 1 else ())
                cases.append(Case('rows-{}-{}{}'.format('-'.join(map(str, dims)), 'lin' if lastlin else 'relu', '-ids' if ids else ''), dims[0], 0, dims[1:], acts,
                                  dict(kernel=ROWS, shape=shape, lastlin=lastlin, seg=False, am=2 if lastlin else 1, has_dot=False), Ps, ids=ids,
                                  padded=bool(j)))
    for k, (widths, units) in enumerate(SEG_CASES):
        for lastlin in (False, True):
            dims = [sum(widths)] + units
            ids = bool((k + lastlin) & 1)
            acts = ['relu'] * (len(units) - 1) + [None if lastlin else 'relu']
            Ps = ROWS_P + ((ROWS_LOOP_P,) if ids else ())
            cases.append(Case('seg-{}-{}-{}{}'.format('+'.join(map(str, widths)), '-'.join(map(str, units)), 'lin' if lastlin else 'relu', '-ids' if ids else ''),
                              dims[0], 0, units, acts,
                              dict(kernel=ROWS, shape=chain_shape(*[tiles16(w) for w in dims]), lastlin=lastlin, seg=True, am=2 if lastlin else 1, has_dot=False),
                              Ps, ids=ids, seg=list(widths)))
    return cases


def all_cases():
    return generic_cases() + pipe_cases() + rows_cases()

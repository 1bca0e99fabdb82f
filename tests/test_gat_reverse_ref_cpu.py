"""CPU: the reference of the one-head GAT reverse tests (tests/gat_reverse_ref.py) against what the project already trusts, and the
conditions under which tests/test_gat_reverse_degrees_gpu.py can tell a skipped trip of a row walk from rounding."""
import numpy as np
import pytest
import torch

from oracle import layers as olayers
from tests import gat_reverse_ref as ref
from tests.entry_point_ref import scaled_error


@pytest.mark.parametrize('directed', [False, True])
def test_degree_graph_holds_every_stride_edge(directed):
    m, tgt, src = ref.degree_graph(directed)                         # (asserts its own properties)
    assert m.shape == (ref.N, ref.N) and len(tgt) == m.nnz and 2500 < m.nnz < 4000
    assert (np.diff(tgt) >= 0).all() and ((np.diff(tgt) > 0) | (np.diff(src) >= 0)).all()       # CSR order
    for ns in (64, 32, 16, 8, 4):                                    # one below, on and one above every trip length
        assert {ns - 1, ns, ns + 1} <= set(ref.LADDER)


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('self_loop', [True, False])
def test_forward_equals_the_oracle(directed, self_loop):
    _, tgt, src = ref.degree_graph(directed)
    for C in (8, 64):
        c = ref.case(C, self_loop, directed, None)
        h, a_s, a_n, bias, _ = (np.asarray(v, dtype=np.float64) for v in c['inputs'])
        want, _ = olayers.gat_conv(h, src, tgt, np.eye(C), a_s, a_n, bias, self_loops=self_loop)      # (row = sources, col = targets)
        assert np.abs(c['want']['y'] - want).max() < 1e-12
        # the formulas behind the scales are the gradient's own
        for q in ('ds', 'dt', 'dH'):
            assert np.abs(c['want']['formula'][q] - c['want'][q]).max() < 1e-12 * max(1.0, np.abs(c['want'][q]).max()), q


@pytest.mark.parametrize('self_loop', [True, False])
@pytest.mark.parametrize('rate', [None, 0.35])
def test_gradients_equal_finite_differences_on_a_subgraph(self_loop, rate):
    """12 nodes of the directed graph (ladder rows 3 and 4 entries long among them, entries renumbered, parallel entries added):
    central differences of the float64 forward, independent of autograd."""
    rng = np.random.default_rng(3)
    n, C = 12, 8
    tgt = np.concatenate([rng.integers(0, n - 2, 40), [5, 5, 5]])    # nodes 10 and 11 stay without entries; (5, 7) three times
    src = np.concatenate([rng.integers(0, n - 2, 40), [7, 7, 7]])
    tgt, src = tgt[tgt != src], src[tgt != src]
    order = np.lexsort((src, tgt))
    tgt, src = tgt[order], src[order]
    ks = ref.edge_masks(tgt, src, n, self_loop, rate)
    T, S, _ = ref.with_self_loops(tgt, src, n, self_loop)
    h = rng.standard_normal((n, C)) * 0.7 + 0.2
    a_s, a_n, bias, dy = rng.standard_normal(C) * 0.3, rng.standard_normal(C) * 0.3, rng.uniform(-0.1, 0.3, C), rng.standard_normal((n, C))
    want = ref.gat_reverse64(h, a_s, a_n, bias, dy, T, S, n, ks)

    def loss(hh, ds=None, dt=None):
        """sum(y * dy) with the scalars s, t shifted: numpy, written out here."""
        s, t = hh @ a_s + (0 if ds is None else ds), hh @ a_n + (0 if dt is None else dt)
        pre = s[T] + t[S]
        e = np.where(pre > 0, pre, 0.2 * pre)
        mx = np.full(n, -1e30)
        np.maximum.at(mx, T, e)
        ex = np.exp(e - mx[T])
        den = np.zeros(n)
        np.add.at(den, T, ex)
        w = ex / (den + 1e-9)[T] * (1.0 if ks is None else ks)
        out = np.zeros((n, C))
        np.add.at(out, T, w[:, None] * hh[S])
        return float((np.maximum(out + bias, 0) * dy).sum())
    eps = 1e-6
    for i in range(n):
        unit = np.zeros(n)
        unit[i] = eps
        assert abs((loss(h, ds=unit) - loss(h, ds=-unit)) / (2 * eps) - want['ds'][i]) < 1e-7, ('ds', i)
        assert abs((loss(h, dt=unit) - loss(h, dt=-unit)) / (2 * eps) - want['dt'][i]) < 1e-7, ('dt', i)
        for c in range(C):
            d = np.zeros((n, C))
            d[i, c] = eps
            assert abs((loss(h + d) - loss(h - d)) / (2 * eps) - want['dH'][i, c]) < 1e-7, ('dH', i, c)


def positive_share(C, directed, seed=None):
    """The smallest share of positive outputs over the ladder rows and the 300-entry row, over both self_loop settings and both rates."""
    _, tgt, src = ref.degree_graph(directed)
    h, a_s, a_n, bias, dy = ref.draw_inputs(C, directed, seed)
    worst = 1.0
    for self_loop in (True, False):
        for rate in (None, ref.DROP_RATE):
            T, S, _ = ref.with_self_loops(tgt, src, ref.N, self_loop)
            ks = ref.edge_masks(tgt, src, ref.N, self_loop, rate)
            y = ref._reverse(torch.float64, h, a_s, a_n, bias, dy, T, S, ref.N, ks)[0].numpy()
            worst = min(worst, float((y[list(ref.LADDER_ROWS) + [ref.HUB]] > 0).mean(1).min()))
    return worst


def truncation_margins(C, directed, seed=None):
    """[(scaled error of the truncated float64 reference / bound, quantity, self_loop, 'row' | 'column', node, length, k)] for every
    truncation (ref.truncations) of every ladder row, the 300-entry row and (directed) every ladder column, rate None."""
    _, tgt, src = ref.degree_graph(directed)
    h, a_s, a_n, bias, dy = ref.draw_inputs(C, directed, seed)
    out = []
    for self_loop in (True, False):
        T, S, _ = ref.with_self_loops(tgt, src, ref.N, self_loop)
        want = ref.gat_reverse64(h, a_s, a_n, bias, dy, T, S, ref.N)
        f32 = ref.errors(ref.gat_reverse32(h, a_s, a_n, bias, dy, T, S, ref.N), want)
        nodes = [('row', v) for v in ref.LADDER_ROWS + (ref.HUB,)] + ([('column', v) for v in ref.LADDER_COLS] if directed else [])
        for kind, node in nodes:
            length = int(((src if kind == 'column' else tgt) == node).sum())
            for k in ref.truncations(length):
                keep = ref.truncated(tgt, src, node, k, by_column=kind == 'column')
                Tk, Sk, _ = ref.with_self_loops(tgt[keep], src[keep], ref.N, self_loop)
                _, dh, ds, dt, _ = ref._reverse(torch.float64, h, a_s, a_n, bias, dy, Tk, Sk, ref.N, None)
                got = {'dH': dh.numpy(), 'ds': ds.numpy(), 'dt': dt.numpy()}
                for q in ('dt' if kind == 'column' else 'ds', 'dH'):
                    bound = min(ref.FACTOR * f32[q], ref.CAP_GRADIENT)              # the GPU test's bound for this case
                    out.append((scaled_error(got[q], want[q], want['scale_' + q]) / bound, q, self_loop, kind, node, length, k))
    return out


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('C', ref.WIDTHS)
def test_truncated_walks_miss_the_bound_by_a_hundred_times(C, directed):
    """What keeps the GPU test from passing a kernel that skips a trip.  A float64 reference in which one ladder row, the 300-entry row
    or (directed) one ladder column stops after its first k entries, k the last full trip of each of the five NS and 64, misses the
    full reference by at least 100 of the GPU test's bounds, under the scales of ref's docstring: in dH for every truncation, in ds
    (rows) and dt (columns) for every row and column of more than one entry.  The one-entry row and column are left out of the ds / dt
    half only: their softmax has one logit (two with the self loop, which need not differ in sign), and with one sign in a row
    ds_i = l c_i (1 - sum_j alpha_ij) is zero whatever the row holds; their dH is asserted.  ref.draw_inputs makes the logits of
    every longer ladder row and column straddle zero for this reason, and the rows' g is non-zero: at least half of the outputs of every
    ladder row and of the 300-entry row are positive."""
    assert positive_share(C, directed) >= 0.5
    margins = truncation_margins(C, directed)
    assert len({t[3:] for t in margins}) == (108 if directed else 56)                 # distinct (kind, node, length, k)
    held = [t for t in margins if not (t[5] == 1 and t[1] in ('ds', 'dt'))]
    assert len(margins) - len(held) == (4 if directed else 2)
    worst = {q: min(t for t in held if t[1] == q) for q in {t[1] for t in held}}
    print('C', C, 'directed', directed, len(held), 'margins asserted; smallest per quantity', worst)
    assert all(t[0] >= 100.0 for t in held), min(held)


def test_float32_restatement_within_the_caps():
    """FACTOR times the float32 restatement's error, the gradients' bound, lies far inside the whole-array cap of the project's other GAT
    reverse tests; the forward's does not (torch adds a row's 300 terms one after the other: up to 5e-6 of their magnitudes), so every
    bound is min(FACTOR * figure, cap).  ref.F32_FIGURES is the record of the measurement."""
    measured = {q: 0.0 for q in ref.QUANTITIES}
    for C in ref.WIDTHS:
        for self_loop in (True, False):
            for directed in (False, True):
                for rate in (None, ref.DROP_RATE):
                    f32 = ref.case(C, self_loop, directed, rate)['f32']
                    measured = {q: max(measured[q], f32[q]) for q in ref.QUANTITIES}
    print(measured)
    assert set(measured) == set(ref.F32_FIGURES)
    for q, value in measured.items():
        assert abs(value - ref.F32_FIGURES[q]) <= 0.05 * value, (q, value)
    for q in ('dH', 'ds', 'dt'):
        assert ref.FACTOR * measured[q] < ref.CAP_GRADIENT / 10
    assert ref.FACTOR * measured['y'] < 4 * ref.CAP_FORWARD and ref.FACTOR <= 16


def test_parallel_entries_wrap_their_dropout_ordinal():
    """The 260 parallel entries of (19, 20): ordinal 255 draws the bit of ordinal 0 (edge_ordinal counts modulo 255), the mirrored
    entries of the symmetric graph agree entry by entry, and the 260 keep at the rate's share."""
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_edge_mask, edge_ordinals
    for directed in (False, True):
        _, tgt, src = ref.degree_graph(directed)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=ref.N))])
        _, ordinal = edge_ordinals(rowptr, src)
        run = np.flatnonzero((tgt == ref.HUB) & (src == ref.HUB_COL))
        assert len(run) == ref.HUB_PARALLEL and (np.diff(run) == 1).all()
        assert list(ordinal[run][:3]) == [0, 1, 2] and ordinal[run][254] == 254 and ordinal[run][255] == 0 and ordinal[run][259] == 4
        agree = 0
        for step in range(8):
            keep, loops = dropout_edge_mask(ref.DROP_SEED, step, ref.DROP_SITE, rowptr, src, True, ref.DROP_RATE)
            assert np.array_equal(keep[run][255:], keep[run][:5])
            agree += int(keep[run][255] == keep[run][0])
            share, sigma = keep[run][:255].mean(), np.sqrt(ref.DROP_RATE * (1 - ref.DROP_RATE) / 255)
            assert abs(share - (1 - ref.DROP_RATE)) < 4 * sigma        # (255 independent draws; the last 5 repeat the first)
            assert 0 < keep[run].sum() < len(run)
            if not directed:
                mirror = np.flatnonzero((tgt == ref.HUB_COL) & (src == ref.HUB))
                assert len(mirror) == ref.HUB_PARALLEL and np.array_equal(keep[mirror], keep[run])
                assert np.array_equal(keep[np.lexsort((tgt, src))], keep)       # every entry and its mirror, the whole multiset
        assert agree == 8

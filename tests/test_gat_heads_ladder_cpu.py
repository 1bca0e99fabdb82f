"""CPU: the reference of the multi-head GAT ladder tests (tests/gat_heads_ladder_ref.py), and the conditions under which
tests/test_gat_heads_ladder_gpu.py can tell a skipped trip, a head read from another head's slot or a missed maximum from rounding."""
import numpy as np
import pytest

from tests import gat_heads_ladder_ref as ref
from tests import gat_reverse_ref as one

CASES = [(h, c, concat, directed) for h, c in ref.SHAPES for concat in (True, False) for directed in (False, True)]
SPECIAL_ROWS = ref.LADDER_ROWS + (ref.HUB,)


@pytest.mark.parametrize('directed', [False, True])
def test_ladder_graph_holds_every_stride_edge(directed):
    m, tgt, src, reserved = ref.ladder_graph(directed)               # (asserts its own roles: ladder counts, parallel entries, isolated nodes,
    assert m.shape == (ref.N, ref.N) and len(tgt) == m.nnz and 3000 < m.nnz < 6000 and ref.N < 600          # the short last workgroup)
    assert (np.diff(tgt) >= 0).all() and ((np.diff(tgt) > 0) | (np.diff(src) >= 0)).all()                   # CSR order
    assert set(one.LADDER) | {23, 24, 25, 47, 48, 49} == set(ref.LADDER) and len(ref.LADDER) == 25
    table = {(2, 4): (2, 32, 1), (3, 4): (4, 16, 1), (2, 8): (4, 16, 2), (4, 4): (4, 16, 1), (3, 8): (8, 8, 2), (2, 12): (8, 8, 3), (8, 8): (16, 4, 2),
             (4, 16): (16, 4, 4), (2, 32): (16, 4, 8), (16, 4): (16, 4, 1), (2, 24): (16, 4, 6)}
    assert set(table) == set(ref.SHAPES)
    for shape, (lpn, ns, cq) in table.items():
        assert ref.walk(*shape) == (lpn, ns, cq)
        for stride in (ns, ns * cq):                                 # a row one below, on and one above the edge walk's and pass 1's trip
            assert {stride - 1, stride, stride + 1} <= set(ref.LADDER), (shape, stride)
    assert {47, 48, 49} <= set(ref.LADDER)                            # ... and the second multiple of 24
    for k, nodes in enumerate(reserved):                             # reserved[k][h]: row k's source at POSITIONS[k][h], in no other special row
        own = src[tgt == k]
        assert len(nodes) == min(ref.LADDER[k], ref.MAX_HEADS) == len(set(nodes))
        assert all(own[p] == v for p, v in zip(ref.POSITIONS[k], nodes))
    flat = [v for nodes in reserved for v in nodes]
    assert len(flat) == len(set(flat)) and not np.isin(src[tgt == ref.HUB], flat).any()
    assert len(ref.EXEMPT) == 0                                      # the one-head ladder test exempts no element either


def test_planted_maxima_cover_every_residue():
    """The dominant entry of (row, head) lies at ref.planted_position: the heads of a row differ as far as its length allows, for every
    shape every residue of its pass-1 stride NS * CQ below min(stride, longest row) is some (row, head)'s, and the last entry of every row
    of length = 1 modulo a stride is dominant for some head of every shape."""
    longest = max(ref.LADDER)
    strides = set()
    for heads, C in ref.SHAPES:
        _, ns, cq = ref.walk(heads, C)
        stride = ns * cq
        strides.add(stride)
        met = {ref.planted_position(k, h) % stride for k in range(len(ref.LADDER)) for h in range(heads)}
        assert set(range(min(stride, longest))) <= met, (heads, C, sorted(set(range(stride)) - met))
        for k, length in enumerate(ref.LADDER):
            assert len({ref.planted_position(k, h) for h in range(heads)}) == min(heads, length)
            assert ref.planted_position(k, 0) == length - 1          # every row's last entry, those of length = 1 modulo a stride among them
    assert strides == {4, 8, 16, 24, 32}
    for directed in (False, True):                                   # a +120 source serves one (row, head) only
        reserved = ref.ladder_graph(directed)[3]
        for heads in (2, 16):
            _, t = ref.planted_scalars(heads, directed, False, seed=1)
            assert (t == ref.PLANTED).sum() == heads * len(ref.LADDER) and (np.abs(t[t != ref.PLANTED]) <= 1).all()
            assert not (t[list(ref.LADDER_ROWS) + [ref.HUB]] == ref.PLANTED).any()
            for k, nodes in enumerate(reserved):
                for h in range(heads):
                    assert t[nodes[h % len(nodes)], h] == ref.PLANTED


def seed_conditions(heads, C, concat, directed, seed=None):
    """(smallest share of positive outputs of a ladder row or the 300-entry row in a head, smallest |logit| of those rows over the
    float32 evaluation's largest error of one), over both self_loop settings."""
    _, tgt, src, _ = ref.ladder_graph(directed)
    inputs = ref.draw_inputs(heads, C, concat, directed, seed)
    share, margin = 1.0, np.inf
    for self_loop in (True, False):
        T, S, _ = one.with_self_loops(tgt, src, ref.N, self_loop)
        r64 = ref.evaluate(*inputs, T, S, concat)
        r32 = ref.evaluate(*inputs, T, S, concat, dtype=np.float32)
        assert r32['pre'].dtype == np.float32
        y = r64['y'][list(SPECIAL_ROWS)]
        share = min(share, float((y.reshape(len(SPECIAL_ROWS), -1, C) > 0).mean(2).min()))
        own = np.isin(T, SPECIAL_ROWS)
        err = np.abs(r32['pre'][own].astype(np.float64) - r64['pre'][own]).max()
        margin = min(margin, float(np.abs(r64['pre'][own]).min() / err))
    return share, margin


def _moved(got, want, bound, rows, h, C, concat):
    """Largest scaled movement, in bounds, of head h's y, dH and ds at `rows`."""
    cols = slice(h * C, (h + 1) * C)
    ycols = cols if concat else slice(None)
    out = np.zeros(len(rows))
    for q, sel in (('y', ycols), ('dH', cols), ('ds', h)):
        scale = want['scale_' + q][rows][:, sel].reshape(len(rows), -1)
        diff = np.abs(got[q][rows][:, sel] - want[q][rows][:, sel]).reshape(len(rows), -1)
        out = np.maximum(out, (diff / np.where(scale > 0, scale, np.inf)).max(1) / bound[q])
    return out


def truncation_margins(heads, C, concat, directed, seed=None):
    """The smallest movement, in bounds of the GPU test, over every cut of one head's walk (gat_reverse_ref.truncations per head).
    Rows: head h's softmax of every ladder row and of the 300-entry row stops after the first k stored entries, all rows at once (what a
    row's cut moves of its own y, ds and dH no other row's cut touches: nothing points at these rows but their own sources); the other
    heads must keep their bits.  Columns (directed): the source walk of a ladder column stops after k entries: dt and dH of the column lose
    the terms of the entries past k (ref.evaluate's d pre and alpha g of the full graph), one column and head at a time."""
    _, tgt, src, _ = ref.ladder_graph(directed)
    inputs = ref.draw_inputs(heads, C, concat, directed, seed)
    a_n = inputs[2][:, :, 0].astype(np.float64)
    rows = np.array(SPECIAL_ROWS)
    lengths = {int(v): int((tgt == v).sum()) for v in rows}
    levels = [{v: ((n - 1) // ns) * ns for v, n in lengths.items()} for ns in (64, 32, 16, 8, 4)] + [{v: 64 for v, n in lengths.items() if n > 64}]
    assert all(sorted({lv[v] for lv in levels if v in lv}) == one.truncations(n) for v, n in lengths.items())
    worst = np.inf
    for self_loop in (True, False):
        T, S, _ = one.with_self_loops(tgt, src, ref.N, self_loop)
        want, f32 = ref.reference(*inputs, T, S, concat)
        bound = ref.bounds(f32)
        base = ref.evaluate(*inputs, T, S, concat)                   # (want's y, dH, ds, dt are autograd's: equal to 1e-12, not bit for bit)
        for h in range(heads):
            others = [o for o in range(heads) if o != h]
            for level in levels:
                got = ref.evaluate(*inputs, T, S, concat, keep=ref.cut_rows(T[:len(tgt)], heads, h, level, len(T)))
                cut = np.array(sorted(level))
                worst = min(worst, float(_moved(got, want, bound, cut, h, C, concat).min()))
                assert np.array_equal(got['out'][:, others], base['out'][:, others])
                if concat:
                    block = np.concatenate([np.arange(o * C, (o + 1) * C) for o in others])
                    assert all(np.array_equal(got[q][:, sel], base[q][:, sel]) for q, sel in (('y', block), ('dH', block), ('ds', others), ('dt', others)))
            for col in ref.LADDER_COLS if directed else ():
                own = np.flatnonzero(src == col)                     # CSR order restricted to the column: the stable transpose's order
                for k in one.truncations(len(own)):
                    tail = own[k:]
                    lost_dt = want['dpre'][tail, h].sum()
                    lost_dh = (want['alpha'][tail, h, None] * want['g'][T[tail], h]).sum(0) + lost_dt * a_n[:, h]
                    sc_h = want['scale_dH'][col, h * C:(h + 1) * C]
                    moved = max(abs(lost_dt) / want['scale_dt'][col, h] / bound['dt'], float((np.abs(lost_dh) / sc_h).max()) / bound['dH'])
                    worst = min(worst, float(moved))
    return worst


def mixup_margins(heads, C, concat, directed, seed=None):
    """{mix: largest movement in bounds} of ref.MIXES: head h evaluated with head h + 1's self scalar, neighbour scalar, maximum,
    denominator or c_i, and a_self / a_neigh read as [H, C]."""
    _, tgt, src, _ = ref.ladder_graph(directed)
    inputs = ref.draw_inputs(heads, C, concat, directed, seed)
    T, S, _ = one.with_self_loops(tgt, src, ref.N, True)
    want, f32 = ref.reference(*inputs, T, S, concat)
    bound = ref.bounds(f32)
    out = {}
    for mix in ref.MIXES:
        got = ref.evaluate(*inputs, T, S, concat, mix=mix)
        # (over the elements of non-zero scale; scaled_error would already fail on an element of scale 0 that moved)
        out[mix] = max(float((np.abs(got[q] - want[q]) / np.where(want['scale_' + q] > 0, want['scale_' + q], np.inf)).max()) / bound[q]
                       for q in ref.QUANTITIES)
    return out


@pytest.mark.parametrize('heads,C,concat,directed', CASES)
def test_seeds_keep_their_conditions_and_wrong_walks_miss_the_bound(heads, C, concat, directed):
    """What keeps the GPU ladder test from passing a kernel that is subtly wrong, for the tabulated seed of the case: the seed's own
    conditions; every cut of one head's walk moves float64 by at least 100 bounds and leaves the other heads' bits; every head mix-up moves
    float64 by at least 100 bounds somewhere."""
    assert (heads, C, concat, directed) in ref.INPUT_SEEDS
    share, margin = seed_conditions(heads, C, concat, directed)
    assert share >= 0.5 and margin > 1.0, (share, margin)
    cut = truncation_margins(heads, C, concat, directed)
    mixed = mixup_margins(heads, C, concat, directed)
    print(heads, C, concat, directed, 'share', share, 'logit margin', margin, 'smallest cut', cut, 'mix-ups', mixed)
    assert cut >= 100.0
    assert set(mixed) == set(ref.MIXES) and all(v >= 100.0 for v in mixed.values()), mixed


@pytest.mark.parametrize('heads,C', ref.SHAPES)
@pytest.mark.parametrize('directed', [False, True])
def test_a_missed_maximum_is_not_finite(heads, C, directed):
    """The planted cases of the GPU test in float32 with every head's maximum taken over the first k entries of a ladder row only, k the
    last full multiple of the shape's pass-1 stride NS * CQ: every (row, head) whose dominant entry lies past k comes out non-finite;
    with the whole row seen everything is finite.  Softmax is shift-invariant: no test on logits of spread 1 can see this walk."""
    _, ns, cq = ref.walk(heads, C)
    stride = ns * cq
    _, tgt, src, _ = ref.ladder_graph(directed)
    first = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=ref.N))])
    seen_stored = np.ones(len(tgt), dtype=bool)
    cut = {}
    for k, length in enumerate(ref.LADDER):
        cut[k] = ((length - 1) // stride) * stride
        seen_stored[first[k] + cut[k]:first[k + 1]] = False
    past = [(k, h) for k in cut for h in range(heads) if ref.planted_position(k, h) >= cut[k]]
    assert len(past) >= len(ref.LADDER)                               # (head 0's dominant entry is the row's last)
    for concat in (True, False):
        for self_loop in (True, False):
            c = ref.planted_case(heads, C, concat, self_loop, directed)
            T, S = c['edges']
            seen = np.concatenate([seen_stored, np.ones(len(T) - len(tgt), dtype=bool)])
            full = ref.evaluate(*c['inputs'], T, S, concat, given=c['given'], dtype=np.float32)
            assert all(np.isfinite(full[q]).all() for q in ref.QUANTITIES)
            missed = ref.evaluate(*c['inputs'], T, S, concat, given=c['given'], dtype=np.float32, max_over=seen)
            for k, h in past:
                block = missed['y'][k, h * C:(h + 1) * C] if concat else missed['y'][k]
                assert not np.isfinite(block).any(), (k, h, concat, self_loop)


def test_float32_restatement_record():
    """ref.F32_FIGURES is the record of the float32 restatement's worst scaled errors over the cases of the GPU ladder test; FACTOR times
    the gradients' figures lies inside the whole-array cap, the forward's need not (gat_reverse_ref), hence min(FACTOR * figure, cap)."""
    measured = {q: 0.0 for q in ref.QUANTITIES}
    for heads, C, concat, directed in CASES:
        for self_loop in (True, False):
            f32 = ref.case(heads, C, concat, self_loop, directed)['f32']
            measured = {q: max(measured[q], f32[q]) for q in ref.QUANTITIES}
    print(measured)
    assert set(measured) == set(ref.F32_FIGURES)
    for q, value in measured.items():
        assert abs(value - ref.F32_FIGURES[q]) <= 0.05 * value, (q, value)
    for q in ('dH', 'ds', 'dt'):
        assert ref.FACTOR * measured[q] < ref.CAP_GRADIENT / 5         # (the restatement, not the cap, decides the gradients' bounds)
    assert ref.FACTOR == 4


def test_given_scalars_leave_the_restatement_unchanged():
    """torch_gat_heads with (s, t) given as leaves: the same y, and d / d hd + ds (x) a_s + dt (x) a_n is the gradient of the composed
    layer; with the argument absent the function is what it was (tests/test_gat_heads_cpu.py pins it)."""
    import torch
    c = ref.case(2, 8, True, True, True)
    T, S = c['edges']
    s, t = c['want']['s'], c['want']['t']
    split = ref.autograd(torch.float64, *c['inputs'], T, S, True, given=(s, t))
    for q in ref.QUANTITIES:
        assert np.abs(split[q] - c['want'][q]).max() <= 1e-12 * max(1.0, np.abs(c['want'][q]).max()), q

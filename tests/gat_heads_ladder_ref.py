"""Reference of the multi-head GAT ladder tests (tests/test_gat_heads_ladder_cpu.py, tests/test_gat_heads_ladder_gpu.py).
TEST INFRASTRUCTURE ONLY: numpy and torch on the CPU, no device.

`ladder_graph` has the roles of tests/gat_reverse_ref.py:degree_graph (ladder rows, a 300-entry row with 260 parallel entries, the column
they point at, isolated nodes, Poisson rows with duplicates; directed: ladder columns, source-only and target-only nodes) on a ladder that
also holds 23, 24, 25, 47, 48, 49: the pass-1 stride of heads of 3 and 6 quads is 24 (`walk`).  Every ladder row owns min(length, 16)
RESERVED sources that no other ladder row and not the 300-entry row points at, at the CSR positions POSITIONS[row]: what the planted
maxima of `planted_case` need (a +120 neighbour scalar must dominate one (row, head) only).

The reference is float64 autograd of tests/gat_heads_ref.py:torch_gat_heads with s and t retained (`autograd`), the restatement the same
function in float32.  `evaluate` writes the same layer out in numpy with every intermediate: it gives the per-element error scales, is
asserted to reproduce autograd (`reference`), and is what the CPU tests cut and mix up.

Error scales: those of gat_reverse_ref's docstring per head h (g_ih = the head's columns of g_i, or g_i / H in the averaging form), sums of
magnitudes of terms, never of differences:
    scale_out[i, h, c] = sum_j |alpha_ijh h_jhc|
    scale_y            = head h's columns: scale_out[i, h, :] + |b|  (concat);  (1/H) sum_h scale_out[i, h, c] + |b_c|  (averaging)
    e_ijh              = alpha_ijh l_ijh (sum_c |g_ihc h_jhc| + sum_c |g_ihc| (scale_out[i, h, c] + |b|))
    scale_ds[i, h]     = sum_j e_ijh            scale_dt[j, h] = sum_i e_ijh
    scale_dH[j, h, c]  = sum_i |alpha_ijh g_ihc| + scale_ds[j, h] |a_s[c, h]| + scale_dt[j, h] |a_n[c, h]|
(in e_ijh the second sum is the magnitude of the terms of c_ih = g_ih . out_ih; with the bias of the head's columns, or b_c in the
averaging form, it is never below the one-head module's).  No element is exempt from the per-element check (EXEMPT)."""
import functools

import numpy as np
import torch
from scipy import sparse

from tests import gat_heads_ref
from tests import gat_reverse_ref as one
from tests.entry_point_ref import KERNEL_FACTOR, scaled_error

LADDER = tuple(sorted(one.LADDER + (23, 24, 25, 47, 48, 49)))
NEW_SHAPES = [(2, 8), (4, 4), (3, 4)]                                  # the LPN = 4 launches no kernel-level test reached
OLD_SHAPES = [(2, 4), (3, 8), (8, 8), (2, 32), (4, 16), (16, 4), (2, 12), (2, 24)]      # test_gat_heads_gpu.SHAPES before this module
SHAPES = OLD_SHAPES + NEW_SHAPES
MAX_HEADS = 16
HUB_ENTRIES, HUB_PARALLEL = one.HUB_ENTRIES, one.HUB_PARALLEL
# node roles (ids)
LADDER_ROWS = tuple(range(0, 25))
HUB, HUB_COL = 25, 26
LADDER_COLS = tuple(range(27, 52))                                     # directed only; ordinary nodes otherwise
ONLY_SOURCES, ONLY_TARGETS = tuple(range(52, 57)), tuple(range(57, 62))    # directed only
ISOLATED = tuple(range(62, 74))
FIRST_POOL = 74                                                        # reserved sources and shared ones, interleaved (ladder_graph)
N_SHARED = 117
N = FIRST_POOL + sum(min(length, MAX_HEADS) for length in LADDER) + N_SHARED            # 515: 128 full workgroups of 4 rows and one of 3

FACTOR = KERNEL_FACTOR
CAP_GRADIENT, CAP_FORWARD = one.CAP_GRADIENT, one.CAP_FORWARD
GRAPH_SEED = 7
QUANTITIES = ('y', 'dH', 'ds', 'dt')
EXEMPT = ()                                                            # elements left out of the per-element check: none (the one-head test: none)
PLANTED = 120.0                                                        # expf overflows float32 above 88.7: a maximum that misses it gives exp(~119)


def walk(heads, C):
    """(LPN, NS, CQ) of the launch the entry points choose for (heads, C): lanes per entry, entries per trip of the edge walk, lanes per
    head; pass 1 takes NS * CQ entries per trip."""
    quads = heads * C // 4
    lpn = 1
    while lpn < quads:
        lpn *= 2
    return lpn, 64 // lpn, C // 4


def _positions():
    """CSR positions of every ladder row's reserved sources, in the order its heads take them.  Head 0: the row's last entry (the one a
    wrong loop bound drops).  The others greedily, rows by length: the position that meets most residues not met so far, counting for
    each pass-1 stride the heads of the fewest-headed shape that has it (test_gat_heads_ladder_cpu.py asserts the coverage reached)."""
    heads_of = {}
    for heads, C in SHAPES:
        stride = walk(heads, C)[1] * walk(heads, C)[2]
        heads_of[stride] = min(heads, heads_of.get(stride, MAX_HEADS))
    met = {stride: set() for stride in heads_of}
    table = []
    for length in LADDER:
        out = []
        for j in range(min(length, MAX_HEADS)):
            counted = [stride for stride in met if j < heads_of[stride]]
            gain = lambda p: sum(p % stride not in met[stride] for stride in counted)                     # noqa: E731
            p = length - 1 if j == 0 else max((q for q in range(length) if q not in out), key=lambda q: (gain(q), q))
            out.append(p)
            for stride in counted:
                met[stride].add(p % stride)
        table.append(tuple(out))
    return tuple(table)


POSITIONS = _positions()


@functools.lru_cache(maxsize=None)
def ladder_graph(directed, seed=GRAPH_SEED):
    """(scipy coo matrix with parallel entries kept, tgt, src, reserved): tgt / src of every entry in CSR order, reserved[k][h] the source at
    position POSITIONS[k][h] of ladder row k.  The pool ids FIRST_POOL.. are numbered so that each row's reserved sources fall between the
    shared sources it draws at exactly those positions."""
    rng = np.random.default_rng(seed)
    # ---- ladder rows: shared sources drawn per row, reserved ones slotted between them
    drawn, slots = [], []                                              # slots: (number of shared ids below, row, order in the row)
    for k, length in enumerate(LADDER):
        wanted = sorted(POSITIONS[k])
        u = np.sort(rng.choice(N_SHARED, length - len(wanted), replace=False))
        drawn.append(u)
        for i, p in enumerate(wanted):
            below = p - i                                              # shared sources of this row before the reserved one
            slots.append((0 if below == 0 else int(u[below - 1]) + 1, k, i))
    keys = [(slot, 0, k, i) for slot, k, i in slots] + [(g, 1, 0, 0) for g in range(N_SHARED)]
    ids = {key: FIRST_POOL + rank for rank, key in enumerate(sorted(keys))}
    shared = np.array([ids[(g, 1, 0, 0)] for g in range(N_SHARED)])
    pool = np.arange(FIRST_POOL, N)
    special = set(LADDER_ROWS) | {HUB, HUB_COL} | set(ISOLATED)
    if directed:
        special |= set(LADDER_COLS) | set(ONLY_SOURCES) | set(ONLY_TARGETS)
    ordinary = np.array([v for v in range(N) if v not in special])
    as_rows = np.concatenate([ordinary, ONLY_TARGETS]) if directed else ordinary
    r, c = [], []
    for k, length in enumerate(LADDER):
        own = [ids[(slot, 0, kk, i)] for slot, kk, i in slots if kk == k]
        r.append(np.full(length, k)), c.append(np.concatenate([shared[drawn[k]], own]).astype(np.int64))
    r.append(np.full(HUB_ENTRIES, HUB))
    c.append(np.concatenate([np.full(HUB_PARALLEL, HUB_COL), rng.choice(shared, HUB_ENTRIES - HUB_PARALLEL, replace=False)]))
    if directed:
        for node, count in zip(LADDER_COLS, LADDER):
            r.append(rng.choice(as_rows, count, replace=False)), c.append(np.full(count, node))
        for node in ONLY_SOURCES:
            r.append(rng.choice(ordinary, 3, replace=False)), c.append(np.full(3, node))
        for node in ONLY_TARGETS:
            r.append(np.full(3, node)), c.append(rng.choice(ordinary, 3, replace=False))
    deg = rng.poisson(5 if directed else 2.5, len(ordinary))
    rows = np.repeat(ordinary, deg)
    cols = rng.choice(ordinary, len(rows))
    cols = np.where(cols == rows, ordinary[(np.searchsorted(ordinary, rows) + 1) % len(ordinary)], cols)        # no diagonal
    dup = rng.random(len(rows)) < 0.1                                  # a tenth of the ordinary entries twice
    r += [rows, rows[dup], [N - 1]]                                   # (the last node always holds an entry: the short workgroup has work)
    c += [cols, cols[dup], [shared[0]]]
    r, c = np.concatenate(r).astype(np.int64), np.concatenate(c).astype(np.int64)
    if not directed:
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
    order = np.lexsort((c, r))
    tgt, src = r[order], c[order]
    m = sparse.coo_matrix((np.ones(len(tgt), dtype=np.float32), (tgt, src)), shape=(N, N))
    # ---- what the tests rely on
    rows_n, cols_n = np.bincount(tgt, minlength=N), np.bincount(src, minlength=N)
    counts = sparse.csr_matrix(m)
    assert (tgt != src).all() and len(pool) == len(keys)
    assert tuple(rows_n[list(LADDER_ROWS)]) == LADDER and rows_n[HUB] == HUB_ENTRIES
    assert counts[HUB, HUB_COL] == HUB_PARALLEL > 255 and counts[HUB].nnz == 1 + HUB_ENTRIES - HUB_PARALLEL
    assert len(ISOLATED) >= 10 and not rows_n[list(ISOLATED)].any() and not cols_n[list(ISOLATED)].any()
    pair = tgt[tgt >= FIRST_POOL] * N + src[tgt >= FIRST_POOL]
    assert len(np.unique(pair)) < len(pair), "ordinary rows must hold duplicated entries"
    assert N % 4 == 3 and rows_n[N - 1] > 0                            # the last workgroup is short and has work
    if directed:
        assert tuple(cols_n[list(LADDER_COLS)]) == LADDER
        assert (rows_n[list(ONLY_SOURCES)] == 0).all() and (cols_n[list(ONLY_SOURCES)] > 0).all()
        assert (cols_n[list(ONLY_TARGETS)] == 0).all() and (rows_n[list(ONLY_TARGETS)] > 0).all()
        assert (counts != counts.T).nnz > 0 and not cols_n[list(LADDER_ROWS)].any()
    else:
        assert (counts != counts.T).nnz == 0 and counts[HUB_COL, HUB] == HUB_PARALLEL
    reserved = []
    special_rows = tgt <= HUB
    for k in LADDER_ROWS:
        own = src[tgt == k]
        nodes = tuple(int(own[p]) for p in POSITIONS[k])
        for v in nodes:                                                # no other ladder row and not the 300-entry row points at it
            assert ((src == v) & special_rows).sum() == 1
        reserved.append(nodes)
    tgt.setflags(write=False), src.setflags(write=False)
    return m, tgt, src, tuple(reserved)


def row_class(directed):
    names = np.array(['ordinary'] * N, dtype=object)
    names[list(LADDER_ROWS)] = 'ladder'
    if directed:
        names[list(LADDER_COLS)] = 'ladder'
    names[HUB], names[HUB_COL] = 'hub row', 'hub column'
    return names


# ---- the layer in numpy, every intermediate kept ------------------------------------------------------------------------------------------

def _segment(v, index, n):
    out = np.zeros((n,) + v.shape[1:])
    np.add.at(out, index, v)
    return out


MIXES = ('s', 't', 'max', 'den', 'c', 'layout')


def evaluate(hd, a_s, a_n, bias, dy, T, S, concat, given=None, keep=None, mix=None, dtype=np.float64, max_over=None):
    """The layer and its gradients written out (notation of the module docstring).  hd [n, H, C], a_s / a_n [C, H, 1], T / S: target and
    source of every term (self loops included by the caller).  given: (s, t) [n, H] in place of hd . a.  keep [E, H] of 0 / 1: a head's
    softmax leaves the entries marked 0 out (a walk cut short for that head only).  mix: head h evaluated with head h + 1's self
    scalar 's', neighbour scalar 't', maximum 'max', denominator 'den' or c_i 'c' where the weights alpha and d pre are formed (the
    statistics themselves are the head's own, as a kernel that reads a wrong slot of its scratch has them), or 'layout': a_s / a_n read
    as [H, C].  max_over [E] of bool: the maximum is taken over these terms only (a pass 1 that misses entries); dtype float32 evaluates
    everything in float32."""
    f = lambda v: np.asarray(v, dtype=dtype)                                                                # noqa: E731
    hd, bias, dy = f(hd), f(bias), f(dy)
    n, H, C = hd.shape
    as2, an2 = f(a_s)[:, :, 0], f(a_n)[:, :, 0]                        # [C, H]
    if mix == 'layout':
        as2, an2 = f(a_s).reshape(H, C).T, f(a_n).reshape(H, C).T
    nxt = lambda v: np.roll(v, -1, axis=1)                                                                  # noqa: E731
    s, t = (np.einsum('nhc,ch->nh', hd, as2), np.einsum('nhc,ch->nh', hd, an2)) if given is None else (f(given[0]), f(given[1]))
    pre = (nxt(s) if mix == 's' else s)[T] + (nxt(t) if mix == 't' else t)[S]
    leak = np.where(pre > 0, dtype(1.0), dtype(0.2))
    e = pre * leak
    kept = np.ones(e.shape, dtype=bool) if keep is None else np.asarray(keep) > 0
    seen = kept if max_over is None else kept & np.asarray(max_over)[:, None]
    mx = np.full((n, H), -np.inf, dtype=dtype)
    np.maximum.at(mx, T, np.where(seen, e, dtype(-np.inf)))
    mx = np.where(np.isfinite(mx), mx, dtype(0.0))                     # (a row nothing is seen of: the self loop's absence, -inf in the kernel)
    with np.errstate(over='ignore', invalid='ignore'):
        ex = np.where(kept, np.exp(e - mx[T]), dtype(0.0))
        den = _segment(ex, T, n).astype(dtype) + dtype(1e-9)
        if mix == 'max':
            alpha = np.where(kept, np.exp(e - nxt(mx)[T]), dtype(0.0)) / den[T]
        else:
            alpha = ex / (nxt(den) if mix == 'den' else den)[T]
        out = _segment(alpha[:, :, None] * hd[S], T, n).astype(dtype)                                       # [n, H, C]
        y = np.maximum((out.reshape(n, H * C) if concat else out.mean(1)) + bias, 0)
    g = dy * (y > 0)
    gh = g.reshape(n, H, C) if concat else np.broadcast_to(g[:, None, :] / dtype(H), (n, H, C))
    bh = np.abs(bias).reshape(H, C) if concat else np.broadcast_to(np.abs(bias), (H, C))
    with np.errstate(over='ignore', invalid='ignore'):
        dalpha = np.einsum('ehc,ehc->eh', gh[T], hd[S])
        ci = _segment(alpha * dalpha, T, n).astype(dtype)
        dpre = alpha * (dalpha - (nxt(ci) if mix == 'c' else ci)[T]) * leak
        ds, dt = _segment(dpre, T, n).astype(dtype), _segment(dpre, S, n).astype(dtype)
        direct = _segment(alpha[:, :, None] * gh[T], S, n).astype(dtype)
        dh = direct + ds[:, :, None] * as2.T[None] + dt[:, :, None] * an2.T[None]
    res = {'y': y, 'out': out, 'dH': dh.reshape(n, H * C), 'ds': ds, 'dt': dt, 's': s, 't': t, 'pre': pre, 'alpha': alpha, 'dpre': dpre,
           'direct': direct, 'g': gh}
    if dtype is np.float64 and mix is None and max_over is None:
        scale_out = _segment(np.abs(alpha[:, :, None] * hd[S]), T, n)
        res['scale_y'] = (scale_out.reshape(n, H * C) if concat else scale_out.mean(1)) + np.abs(bias)
        terms = alpha * leak * (np.einsum('ehc,ehc->eh', np.abs(gh[T]), np.abs(hd[S])) + np.einsum('nhc,nhc->nh', np.abs(gh), scale_out + bh)[T])
        res['scale_ds'], res['scale_dt'] = _segment(terms, T, n), _segment(terms, S, n)
        res['scale_dH'] = (_segment(np.abs(alpha[:, :, None] * gh[T]), S, n) + res['scale_ds'][:, :, None] * np.abs(as2.T)[None]
                           + res['scale_dt'][:, :, None] * np.abs(an2.T)[None]).reshape(n, H * C)
        res['scale_s'] = np.einsum('nhc,ch->nh', np.abs(hd), np.abs(as2)), np.einsum('nhc,ch->nh', np.abs(hd), np.abs(an2))
        assert (res['scale_ds'] >= _segment(np.abs(dpre), T, n)).all() and (res['scale_dt'] >= _segment(np.abs(dpre), S, n)).all()
    return res


def autograd(dtype, hd, a_s, a_n, bias, dy, T, S, concat, given=None):
    """{'y', 'dH', 'ds', 'dt'} by autograd of gat_heads_ref.torch_gat_heads in `dtype`.  given = (s, t): the three of hd, s, t are
    independent leaves and dH = d / d hd + ds (x) a_s + dt (x) a_n, as gat_heads_bwd_source_kernel composes it."""
    ten = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype)                              # noqa: E731
    n, H, C = hd.shape
    Tt, St = torch.as_tensor(np.array(T), dtype=torch.long), torch.as_tensor(np.array(S), dtype=torch.long)
    ht, ast, ant = ten(hd).requires_grad_(True), ten(a_s), ten(a_n)
    leaves = None if given is None else tuple(ten(v).requires_grad_(True) for v in given)
    kept = {}
    # one thread: with several, torch's float32 index_add adds a node's terms in an order that changes from run to run (dH of the (2, 4)
    # cases between 1e-6 and 8e-6 of its scale); one after the other is the restatement the bounds are multiples of
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        y = gat_heads_ref.torch_gat_heads(ht, ast, ant, ten(bias), St, Tt, concat, keep=kept, scalars=leaves)
        (y * ten(dy)).sum().backward()
    finally:
        torch.set_num_threads(threads)
    ds, dt = kept['s'].grad, kept['t'].grad
    ds, dt = (torch.zeros((n, H), dtype=dtype) if v is None else v for v in (ds, dt))                      # (a graph without terms)
    dh = ht.grad if ht.grad is not None else torch.zeros_like(ht)
    if given is not None:
        dh = dh + ds[:, :, None] * ast[:, :, 0].T[None] + dt[:, :, None] * ant[:, :, 0].T[None]
    out = {'y': y.detach().numpy(), 'dH': dh.reshape(n, H * C).numpy(), 'ds': ds.numpy(), 'dt': dt.numpy()}
    assert all(v.dtype == (np.float64 if dtype == torch.float64 else np.float32) for v in out.values()), "the evaluation was promoted"
    return out


UNDERFLOW_FLOOR = 1e-30


def reference(hd, a_s, a_n, bias, dy, T, S, concat, given=None, floor=0.0):
    """Float64 autograd with the scales of `evaluate`, whose formulas are asserted to reproduce it; and the float32 restatement's errors.
    floor (the planted cases: UNDERFLOW_FLOOR, as entry_point_ref.add3_scale): beside a +120 logit the other weights of a row are
    exp(-119) = 2e-52, below float32's range, and so is everything made of them alone; such elements carry absolute accuracy only.
    Elements of scale 0 stay exact."""
    want = evaluate(hd, a_s, a_n, bias, dy, T, S, concat, given)
    for q in QUANTITIES:
        want['scale_' + q] = np.where(want['scale_' + q] > 0, want['scale_' + q] + floor, 0.0)
    auto = autograd(torch.float64, hd, a_s, a_n, bias, dy, T, S, concat, given)
    for q in QUANTITIES:
        assert np.abs(want[q] - auto[q]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(auto[q]).max(initial=0.0)), q
        want[q] = auto[q]
    f32 = errors(autograd(torch.float32, hd, a_s, a_n, bias, dy, T, S, concat, given), want)
    return want, f32


def errors(got, want):
    return {q: scaled_error(got[q], want[q], want['scale_' + q]) for q in QUANTITIES}


def bounds(f32):
    return {q: min(FACTOR * f32[q], CAP_FORWARD if q == 'y' else CAP_GRADIENT) for q in QUANTITIES}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
# seeds of draw_inputs per (heads, C, concat, directed), chosen on the CPU; test_gat_heads_ladder_cpu.py holds each to its conditions: every
# ladder row and the 300-entry row keep at least half of their outputs positive in every head, and no logit of theirs lies within the float32
# restatement's error of zero, under both self_loop settings
INPUT_SEEDS = {(2, 4, True, False): 3, (2, 4, True, True): 3, (2, 4, False, False): 0, (2, 4, False, True): 0, (3, 8, True, False): 1,
               (3, 8, True, True): 1, (3, 8, False, False): 0, (3, 8, False, True): 0, (8, 8, True, False): 4, (8, 8, True, True): 4,
               (8, 8, False, False): 1, (8, 8, False, True): 0, (2, 32, True, False): 2, (2, 32, True, True): 2, (2, 32, False, False): 0,
               (2, 32, False, True): 0, (4, 16, True, False): 2, (4, 16, True, True): 2, (4, 16, False, False): 0, (4, 16, False, True): 0,
               (2, 12, True, False): 1, (2, 12, True, True): 1, (2, 12, False, False): 0, (2, 12, False, True): 0, (2, 24, True, False): 2,
               (2, 24, True, True): 2, (2, 24, False, False): 0, (2, 24, False, True): 0, (2, 8, True, False): 1, (2, 8, True, True): 1,
               (2, 8, False, False): 0, (2, 8, False, True): 0, (4, 4, True, False): 11, (4, 4, True, True): 11, (4, 4, False, False): 0,
               (4, 4, False, True): 0, (3, 4, True, False): 1, (3, 4, True, True): 1, (3, 4, False, False): 0, (3, 4, False, True): 0,
               (16, 4, True, False): 3, (16, 4, True, True): 3, (16, 4, False, False): 65, (16, 4, False, True): 10}
# worst scaled error of the float32 restatement against float64 over the cases of the GPU ladder test, as measured when the tests were
# written; test_gat_heads_ladder_cpu.py keeps the record within 5 % of a fresh measurement
F32_FIGURES = {'y': 5.645e-6, 'dH': 5.287e-6, 'ds': 1.966e-6, 'dt': 3.728e-6}


def draw_inputs(heads, C, concat, directed, seed=None):
    """(hd [N, H, C], a_s, a_n [C, H, 1], bias, dy) float32: gat_reverse_ref.draw_inputs head by head.  The heads' attention vectors are
    drawn independently; H of a ladder row, of the 300-entry row and (directed) of a ladder column moves along that head's a_s (a_n) until
    the head's logits in the row (column) straddle zero, away from LeakyReLU's kink."""
    key = (heads, C, bool(concat), bool(directed))
    rng = np.random.default_rng(INPUT_SEEDS.get(key, 0) if seed is None else seed)
    width = heads * C if concat else C
    # (sixteen heads of 4 columns, concatenated: no seed keeps half of every head positive at 0.2; averaged, 0.2 serves)
    lean = 0.8 if heads > 8 and concat else 0.2
    hd = (rng.standard_normal((N, heads, C)) * 0.7 + lean).astype(np.float32)
    a_s, a_n = ((rng.standard_normal((C, heads, 1)) * 0.7 / np.sqrt(C)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.1, 0.3, width).astype(np.float32)
    dy = rng.standard_normal((N, width)).astype(np.float32)
    _, tgt, src, _ = ladder_graph(bool(directed))
    h64, as64, an64 = hd.astype(np.float64), a_s[:, :, 0].astype(np.float64), a_n[:, :, 0].astype(np.float64)
    s, t = np.einsum('nhc,ch->nh', h64, as64), np.einsum('nhc,ch->nh', h64, an64)

    def middle(values):
        v = np.unique(values)
        return None if len(v) == 1 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    for h in range(heads):
        for node in LADDER_ROWS + (HUB,):
            mid = middle(t[src[tgt == node], h])
            if mid is not None:
                h64[node, h] += as64[:, h] * ((-mid - s[node, h]) / (as64[:, h] @ as64[:, h]))
        for node in LADDER_COLS if directed else ():
            mid = middle(s[tgt[src == node], h])
            if mid is not None:
                h64[node, h] += an64[:, h] * ((-mid - t[node, h]) / (an64[:, h] @ an64[:, h]))
    return h64.astype(np.float32), a_s, a_n, bias, dy


@functools.lru_cache(maxsize=None)
def case(heads, C, concat, self_loop, directed):
    """One case of the GPU ladder test, computed once and left unchanged by the tests that share it."""
    _, tgt, src, _ = ladder_graph(directed)
    inputs = draw_inputs(heads, C, concat, directed)
    T, S, _ = one.with_self_loops(tgt, src, N, self_loop)
    want, f32 = reference(*inputs, T, S, concat)
    return {'inputs': inputs, 'edges': (T, S), 'want': want, 'f32': f32, 'bound': bounds(f32)}


def planted_scalars(heads, directed, own, seed):
    """(s, t) [N, H] float32 built on the host: uniform in [-1, 1]; own False: for every ladder row k and head h the source at position
    POSITIONS[k][h % len] carries t = +120 for that head (the head's dominant entry); own True: the ladder rows' own t is +120 (their
    self-loop term dominates; directed only, where nothing points at a ladder row)."""
    rng = np.random.default_rng(seed)
    s, t = (rng.uniform(-1, 1, (N, heads)).astype(np.float32) for _ in range(2))
    reserved = ladder_graph(directed)[3]
    for k in LADDER_ROWS:
        for h in range(heads):
            if own:
                t[k, h] = PLANTED
            else:
                t[reserved[k][h % len(reserved[k])], h] = PLANTED
    return s, t


def planted_position(k, h):
    """CSR position in ladder row k of head h's dominant entry."""
    return POSITIONS[k][h % len(POSITIONS[k])]


@functools.lru_cache(maxsize=None)
def planted_case(heads, C, concat, self_loop, directed, own=False):
    """A case of the planted-maximum test: S is an input of its own, so hd, s and t are independent leaves of the reference."""
    assert directed or not own
    _, tgt, src, _ = ladder_graph(directed)
    hd, a_s, a_n, bias, dy = draw_inputs(heads, C, concat, directed, seed=1000 + heads * C)
    given = planted_scalars(heads, directed, own, seed=2000 + heads * C)
    T, S, _ = one.with_self_loops(tgt, src, N, self_loop)
    want, f32 = reference(hd, a_s, a_n, bias, dy, T, S, concat, given, floor=UNDERFLOW_FLOOR)
    return {'inputs': (hd, a_s, a_n, bias, dy), 'given': given, 'edges': (T, S), 'want': want, 'f32': f32, 'bound': bounds(f32)}


def cut_rows(tgt, heads, h, k_of_row, n_terms):
    """keep [n_terms, H]: head h leaves the stored entries of every row in k_of_row past its first k out (CSR order; terms past the
    stored entries, the self loops, stay)."""
    keep = np.ones((n_terms, heads))
    for node, k in k_of_row.items():
        keep[np.flatnonzero(tgt == node)[k:], h] = 0.0
    return keep

"""Graphs and float64 references for tests/test_propagate_wide_address_gpu.py: the gather-address forms of the tiled propagation
kernels.  Host-only (numpy / scipy); the device side lives in the test module."""
import numpy as np
from scipy import sparse

N = 2048                       # nodes = columns of the small graph
LD_64 = (1 << 32) // (4 * N)   # 524 288: n_cols * ld * 4 == 2^32, the first span of the 64-bit form
LD_32 = LD_64 - 4              # 524 284: 2^32 - 32 768 bytes, the last 32-bit span; the top columns' offsets lie above 2^31
LD_PAST = LD_64 + 2048       # 526 336: the byte offsets of columns 2 041 .. 2 047 no longer fit 32 bits (a truncated offset wraps into row 0's gap)
BIG_N = (1 << 24) + 2048       # rows of the dense F = 32 table above 2^31 bytes
BLOCK_ROWS, BLOCK_OFFSET = 512, 256


def wide_graph(seed=7, n=N, n_edges=20000):
    """~20 000 undirected unit edges (u < v) over n nodes: node HUB takes part in more than a quarter of all entries (its row then
    repeats inside every step of its tile: flagged repeats and, on a pairs image, implicit pairs; duplicates of (HUB, v) are
    multiplicities), a few nodes have no edge at all, and columns 0 and n - 1 are both well connected."""
    rng = np.random.default_rng(seed)
    hub = 700
    isolated = np.array([3, 64, 65, 1000, 2046])
    free = np.setdiff1d(np.arange(n), np.concatenate([isolated, [hub]]))
    n_hub = n_edges * 11 // 20                                        # 55 % of the edges touch the hub: > 1/4 of the 2 E entries in its row
    other = rng.choice(free, n_hub)
    u, v = np.minimum(hub, other), np.maximum(hub, other)
    a, b = rng.choice(free, n_edges - n_hub - 80), rng.choice(free, n_edges - n_hub - 80)
    keep = a != b
    u, v = np.concatenate([u, np.minimum(a, b)[keep]]), np.concatenate([v, np.maximum(a, b)[keep]])
    ends = rng.choice(free[(free > 0) & (free < n - 1)], 80)          # 40 edges into column 0, 40 into column n - 1
    u, v = np.concatenate([u, np.zeros(40, np.int64), ends[40:]]), np.concatenate([v, ends[:40], np.full(40, n - 1)])
    assert np.all(u < v) and not np.isin(isolated, np.concatenate([u, v])).any()
    deg_hub = int((u == hub).sum() + (v == hub).sum())
    assert 4 * deg_hub >= 2 * len(u)
    return {'u': u.astype(np.int64), 'v': v.astype(np.int64), 'n': n, 'hub': hub, 'isolated': isolated}


def edge_list(g):
    """Both directions of every edge as (row, col), duplicates kept: the edge-list adjacency GraphSAGE / GAT walk."""
    return np.concatenate([g['u'], g['v']]), np.concatenate([g['v'], g['u']])


def block_graph(n_cols, seed, blocks=('first', 'last'), n_rows=BLOCK_ROWS, offset=BLOCK_OFFSET, n_entries=12000):
    """A row block (rows = nodes offset .. offset + n_rows) of a graph with n_cols nodes whose entries lie in 1 024-column ranges at the
    first / middle / last columns only; returns (rows, cols, compact) with `compact` the same columns renumbered 0 .. 1024 len(blocks)
    (in the same order), for a reference over the referenced columns alone.  One row is heavy, a few are empty, no (i, i) entry."""
    rng = np.random.default_rng(seed)
    starts = {'first': 0, 'middle': (n_cols // 2) & ~1023, 'last': n_cols - 1024}
    base = np.array([starts[b] for b in blocks], dtype=np.int64)
    rows = rng.integers(0, n_rows, n_entries)
    rows[: n_entries // 4] = 17                                       # a heavy row
    rows[np.isin(rows, [5, 100, 511])] = 18                           # rows without entries
    compact = rng.integers(0, 1024 * len(blocks), n_entries)
    compact[:8] = [0, 1023, 1024 * len(blocks) - 1, 1024 * len(blocks) - 1024, 0, 1024 * len(blocks) - 1, 1, 2]   # the edges of every range
    cols = base[compact // 1024] + compact % 1024
    keep = cols != rows + offset
    return rows[keep], cols[keep], compact[keep], base


def referenced_rows(base):
    """The table rows a block_graph image can touch: its 1 024-column ranges (the block's own rows lie inside the first)."""
    return np.concatenate([b + np.arange(1024) for b in base])


def spmm_refs(A, t64, x0, b, w2, next_scale):
    """float64 results of the three epilogues for Y = A_eff . T (A_eff: the matrix that takes the gathered table to the product).
    plain; bias + ReLU + the next layer's product (rows scaled by next_scale or not); the running sum / mean pair."""
    y = A @ t64
    y1 = np.maximum(y + b, 0)
    hn = y1 @ w2.astype(np.float64)
    if next_scale is not None:
        hn = next_scale.astype(np.float64)[:, None] * hn
    s1 = x0.astype(np.float64) + y
    return {'plain': y, 'y1': y1, 'hn': hn, 's1': s1, 'mean': (s1 + y) / 3}


def gat_ref(rows, cols, n_rows, h64_of_col, ss_rows, sn_of_col, sn_self, h64_self, b, self_loop):
    """Dense float64 softmax of the GAT layer over an entry list: e = LeakyReLU_0.2(s_self[row] + s_neigh[col]), softmax per row
    (max-subtracted, + 1e-9 in the denominator as Spektral), out = ReLU(sum alpha h + b).  `*_of_col` are indexed by the entry's
    position (already gathered), `*_self` per row for the added self loop."""
    e = ss_rows.astype(np.float64)[rows] + sn_of_col.astype(np.float64)
    hh = h64_of_col
    r = rows
    if self_loop:
        e = np.concatenate([e, ss_rows.astype(np.float64) + sn_self.astype(np.float64)])
        hh = np.concatenate([hh, h64_self])
        r = np.concatenate([rows, np.arange(n_rows)])
    e = np.where(e > 0, e, 0.2 * e)
    mx = np.full(n_rows, -np.inf)
    np.maximum.at(mx, r, e)
    ex = np.exp(e - mx[r])
    den = np.zeros(n_rows)
    np.add.at(den, r, ex)
    num = np.zeros((n_rows, hh.shape[1]))
    np.add.at(num, r, ex[:, None] * hh)
    return np.maximum(num / (den + 1e-9)[:, None] + b, 0)


def gat_err(got, want):
    """The measure of test_gat_xcd_sliced / test_gat_lds_tiled: max |got - want| / max(1, max |want|), bound 2e-5."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(1.0, np.abs(want).max()))


def block_matrix(rows, compact, n_rows, n_ref):
    return sparse.coo_matrix((np.ones(len(rows)), (rows, compact)), shape=(n_rows, n_ref)).tocsr()

"""Reference for the directed-graph tests: the stable CSR transpose restated in numpy, and three small directed graphs.

The stable transpose of a CSR structure: output row j holds the entries of column j in the order of their input positions (by
source row; parallel entries in input order) — a counting sort that walks the input rows in order.  `perm[q]` is the input position
of the entry at output position q.  scipy's csr -> csc conversion (without summing duplicates) is the same thing.
"""
import numpy as np
from scipy import sparse


def stable_transpose(rowptr, colidx, n_cols):
    """(t_rowptr [n_cols + 1], t_colidx [nnz], perm [nnz]) as int32, by a counting sort that walks the rows in order."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    n_rows, nnz = len(rowptr) - 1, len(colidx)
    t_rowptr = np.zeros(n_cols + 1, dtype=np.int64)
    for c in colidx:
        t_rowptr[c + 1] += 1
    np.cumsum(t_rowptr, out=t_rowptr)
    cursor = t_rowptr[:-1].copy()
    t_colidx, perm = np.empty(nnz, dtype=np.int64), np.empty(nnz, dtype=np.int64)
    for i in range(n_rows):
        for p in range(rowptr[i], rowptr[i + 1]):
            q = cursor[colidx[p]]
            cursor[colidx[p]] += 1
            t_colidx[q], perm[q] = i, p
    return t_rowptr.astype(np.int32), t_colidx.astype(np.int32), perm.astype(np.int32)


def stable_transpose_fast(rowptr, colidx, n_cols):
    """The same result by a stable argsort (for graphs too large for the Python loops above; held against them in the CPU tests)."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    perm = np.argsort(colidx, kind='stable')
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=n_cols))]) if n_cols else np.zeros(1, dtype=np.int64)
    return t_rowptr.astype(np.int32), rows[perm].astype(np.int32), perm.astype(np.int32)


def ordinals(rowptr, colidx):
    """Per entry: its ordinal among the equal columns of its row, counted in position order (columns need not be sorted)."""
    out = np.zeros(len(colidx), dtype=np.int64)
    for i in range(len(rowptr) - 1):
        seen = {}
        for p in range(rowptr[i], rowptr[i + 1]):
            out[p] = seen.get(int(colidx[p]), 0)
            seen[int(colidx[p])] = out[p] + 1
    return out


def csr_of(m):
    """Row-major CSR arrays of a scipy matrix with duplicates kept, as DeviceCSR.from_scipy orders them."""
    coo = m.tocoo()
    order = np.lexsort((coo.col, coo.row))
    row, col = coo.row[order], coo.col[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m.shape[0]))]).astype(np.int32)
    return rowptr, col.astype(np.int32), coo.data[order]


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def tiny(graph, **kw):
    """helpers.tiny_graph with its adjacency rebuilt un-symmetrised: 'ui' users -> items only (every item row and every user column
    empty), 'uip' the same with item -> property links."""
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    from tests import helpers
    args = dict(n_users=80, n_items=60, n_ratings=1500, seed=9, n_props=30 if graph == 'uip' else 0, n_links=90 if graph == 'uip' else 0)
    args.update(kw)
    g = helpers.tiny_graph(**args)
    g['adj_sym'] = g['adj']
    g['adj'] = build_adjacency_matrix(g['ratings'], g['users'], g['items'], g['triples'], g['props'],
                                      type_adjacency='unary-uip' if graph == 'uip' else 'unary', symmetric_adjacency=False)
    m = sparse.csr_matrix(g['adj'])
    nu = g['n_users']
    assert m.shape[0] == m.shape[1] and (m != m.T).nnz > 0
    assert m[nu:nu + g['n_items']].nnz == (0 if graph == 'ui' else m[nu:].nnz) and m[:, :nu].nnz == 0
    if graph == 'ui':
        assert m[nu:].nnz == 0
    return g


def mixed(n_users=70, n_items=90, seed=4):
    """A random directed multigraph without diagonal entries on n_users + n_items nodes (users first, so that (user, item) pairs can
    be scored) that holds, asserted below: a reciprocal pair, a duplicate entry, a duplicate whose reverse also exists, an empty row,
    an empty column, a row of more than 64 entries and a column of more than 64 entries."""
    rng = np.random.default_rng(seed)
    n = n_users + n_items
    src = rng.integers(0, n - 2, 1400)
    dst = rng.integers(0, n - 2, 1400)
    hub_row, hub_col = 3, n_users + 5
    extra = [(hub_row, c) for c in range(10, 90)] + [(r, hub_col) for r in range(20, 110)]      # a long row, a long column
    extra += [(7, n_users + 1), (n_users + 1, 7)]                                                    # a reciprocal pair
    extra += [(9, n_users + 2), (9, n_users + 2)]                                                    # a duplicate entry
    extra += [(11, n_users + 3), (11, n_users + 3), (n_users + 3, 11)]                               # a duplicate whose reverse exists
    src = np.concatenate([src, [e[0] for e in extra]])
    dst = np.concatenate([dst, [e[1] for e in extra]])
    keep = (src != dst) & (src != n - 2) & (dst != n - 1)      # node n - 2 has no outgoing entry, node n - 1 no incoming one
    src, dst = src[keep], dst[keep]
    # ... and they get one entry the other way round each so that neither is isolated
    src, dst = np.concatenate([src, [n - 1, 5]]), np.concatenate([dst, [4, n - 2]])
    adj = sparse.coo_matrix((np.ones(len(src), dtype=np.float32), (src, dst)), shape=(n, n))
    m = sparse.csr_matrix(adj)                                  # (sums duplicates: counts per pair)
    assert m.diagonal().sum() == 0
    assert m[7, n_users + 1] >= 1 and m[n_users + 1, 7] >= 1
    assert m[9, n_users + 2] >= 2
    assert m[11, n_users + 3] >= 2 and m[n_users + 3, 11] >= 1
    assert m[n - 2].nnz == 0 and m[:, n - 1].nnz == 0
    rowptr, colidx, _ = csr_of(adj)
    assert np.diff(rowptr).max() > 64 and np.bincount(colidx, minlength=n).max() > 64
    pairs = rng.choice(n_users * n_items, size=300, replace=False)
    return {'adj': adj, 'u_ids': pairs // n_items, 'i_ids': pairs % n_items + n_users, 'n_users': n_users, 'n_items': n_items}


def graph(name):
    return mixed() if name == 'mixed' else tiny(name)

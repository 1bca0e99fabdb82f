"""Shared cases of the BPR triplet tests (CPU and GPU): a 70 x 50 rating set with the edge users, the Sequence over it, the
invariants every batch must hold, and the planted two-group data of the learning test."""
import numpy as np

N_USERS, N_ITEMS = 70, 50
FULL_USER, SINGLE_USER, FREE_ITEM = 0, 1, 17          # user 0 likes every item but item 17; user 1 has a single positive


def ratings_70x50(seed=3):
    """[R, 3] (user, item node id = item + N_USERS, label).  User 0 likes 49 of the 50 items and rates nothing else (d = n_items - 1
    under both exclusion kinds, a single candidate), user 1 likes one item and dislikes five, every other user rates 20 random
    items with at least one like."""
    rng = np.random.default_rng(seed)
    rows = [(FULL_USER, N_USERS + i, 1) for i in range(N_ITEMS) if i != FREE_ITEM]
    picked = rng.permutation(N_ITEMS)[:6]
    rows += [(SINGLE_USER, N_USERS + picked[0], 1)] + [(SINGLE_USER, N_USERS + i, 0) for i in picked[1:]]
    for u in range(2, N_USERS):
        its = rng.permutation(N_ITEMS)[:20]
        labels = (rng.random(20) < 0.6).astype(np.int64)
        labels[0] = 1
        rows += [(u, N_USERS + i, int(l)) for i, l in zip(its, labels)]
    r = np.array(rows, dtype=np.int64)
    r = r[rng.permutation(len(r))]
    return np.concatenate([r, r[:30]])                # (duplicated rows: the lists are deduplicated)


def triplet_sequence(ratings=None, **kw):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraphTriplets
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    r = ratings_70x50() if ratings is None else ratings
    users, items = np.arange(N_USERS) * 3 + 1, np.arange(N_ITEMS) * 5 + 2
    adj = build_adjacency_matrix(r, users, items, type_adjacency='unary')
    return UserItemGraphTriplets(r, users, items, adj, **kw)


def rows_of(csr):
    ptr, ids = csr
    return [set(int(x) for x in ids[ptr[k]:ptr[k + 1]]) for k in range(len(ptr) - 1)]


def check_batch(seq, batch, h, K):
    """The invariants of one batch of h triples with K negatives per draw."""
    (u, i), y = batch
    u, i, y = np.asarray(u), np.asarray(i), np.asarray(y)
    assert u.shape == (2 * h,) and i.shape == (2 * h,) and np.array_equal(y, [1] * h + [0] * h)
    assert np.array_equal(u[:h], u[h:]) and u.min() >= 0 and u.max() < len(seq.users)
    pos, excl = rows_of(seq.pos_csr), rows_of(seq.excl_csr)
    lo, hi = seq.item_base, seq.item_base + seq.n_items
    for t in range(h):
        assert int(i[t]) in pos[u[t]], t
        assert lo <= i[h + t] < hi and int(i[h + t]) not in excl[u[t]], t
    assert np.array_equal(u[:h], np.repeat(u[:h:K], K)) and np.array_equal(i[:h], np.repeat(i[:h:K], K))


def two_group_data(n_users=120, n_items=80, n_train=24, n_test=4):
    """Two user groups, two item groups of equal size; every user likes items of its own group only (n_train for training, n_test
    held out), chosen cyclically so that every item is liked by the same number of users in training: a per-item score ranks at
    chance.  No dislikes at all.  Returns (train [R, 3], test [T, 3], users, items)."""
    half_u, half_i = n_users // 2, n_items // 2
    assert (half_u * n_train) % half_i == 0 and n_train + n_test <= half_i
    train, test = [], []
    for u in range(n_users):
        g, k = divmod(u, half_u)
        own = g * half_i + (k * n_train + np.arange(n_train + n_test)) % half_i      # a cyclic window: equal item popularity
        train += [(u, n_users + i, 1) for i in own[:n_train]]
        test += [(u, n_users + i, 1) for i in own[n_train:]]
    return np.array(train, dtype=np.int64), np.array(test, dtype=np.int64), np.arange(n_users), np.arange(n_items)

"""Batch sequences fed to the models — mirrors `/root/reference/src/data/datasets.py:8-373`.

Same constructor arguments, attributes (``ratings``, ``users``, ``items``, ``adj_matrix``,
``embeddings``) and batch tuple layouts as the reference's ``keras.utils.Sequence`` classes:

    UserItemEmbeddings        ((u_emb[B,D], i_emb[B,D]), y[B])                      datasets.py:65-67
    HybridUserItemEmbeddings  ((u_graph, i_graph, u_bert, i_bert), y)               datasets.py:127-133
    UserItemGraph             ((u_ids[B], i_ids[B]), y[B])                          datasets.py:203
    UserItemGraphEmbeddings   ((u_ids, i_ids, u_emb[B,D], i_emb[B,D]), y)           datasets.py:366

Built with ``sample_weight`` (float [R], row r weighs rating row r) these four yield Keras' three-element batches
``(inputs, y, w[B])``; a shuffle permutes the weights with the ratings.  Without it nothing changes.

ids are int64 with item ids already offset by |U|; the last batch is short.  Shuffling uses
``np.random.RandomState(seed)`` re-drawn at every epoch end, like the reference.
    UserItemGraphPosNegSample ((u_ids[2h], i_ids[2h]), y[2h]), h = batch_size // 2      datasets.py:216-306

``UserItemGraphPosNegSample`` (BPR) draws its batches: on the host in ``__getitem__`` (the reference's stream) and, inside
``fit()``, on the device (``bpr_device_batch`` states that kernel's draws).

``UserItemGraphTriplets`` has no counterpart in the reference: BPR triples (user, positive, negative) in the same batch tuple, both
items under the user they were drawn for, the negative uniform over the user's unobserved items; drawn on the device inside
``fit()`` and restated by ``bpr_triplet_device_batch``.
"""
import itertools as it

import numpy as np
from scipy import sparse


def _checked_sample_weight(sample_weight, ratings):
    """None, or the per-rating weights as float32 [R] (row r weighs rating row r).  ValueError: another length or shape."""
    if sample_weight is None:
        return None
    w = np.asarray(sample_weight, dtype=np.float32)
    if w.ndim != 1 or len(w) != len(ratings):
        raise ValueError("sample_weight must hold one weight per rating row: shape {} for {} ratings".format(w.shape, len(ratings)))
    return w


class _RatingsSequence:
    def __init__(self, ratings, users, items, batch_size=512, shuffle=False, seed=42, sample_weight=None):
        self.ratings = ratings
        self.sample_weight = _checked_sample_weight(sample_weight, ratings)
        self.users = users
        self.items = items
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.seed = seed
        self.indexes = None
        self.random_state = None
        self.order_version = 0          # bumped whenever the batch order changes: lets predict() keep its uploaded id list
        self.on_epoch_end()

    def __len__(self):
        return int(np.ceil(len(self.ratings) / self.batch_size))

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    def _batch_ratings(self, idx):
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        lo = idx * self.batch_size
        hi = min(lo + self.batch_size, len(self.ratings))
        if self.shuffle:
            return self.ratings[self.indexes[lo:hi]]
        return self.ratings[lo:hi]

    def _batch_weights(self, idx):
        """The weights of the rows `_batch_ratings(idx)` returns (the shuffle permutes both alike), or None without sample_weight."""
        if self.sample_weight is None:
            return None
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        lo = idx * self.batch_size
        hi = min(lo + self.batch_size, len(self.ratings))
        if self.shuffle:
            return self.sample_weight[self.indexes[lo:hi]]
        return self.sample_weight[lo:hi]

    def _batch(self, idx, inputs, y):
        """(inputs, y), or (inputs, y, w) for a Sequence built with sample_weight (Keras' three-element batch)."""
        if self.sample_weight is None:
            return inputs, y
        return inputs, y, self._batch_weights(idx)

    def on_epoch_end(self):
        if self.shuffle:
            if self.random_state is None:
                self.random_state = np.random.RandomState(self.seed)
            self.indexes = np.arange(len(self.ratings))
            self.random_state.shuffle(self.indexes)
            self.order_version += 1


class UserItemEmbeddings(_RatingsSequence):
    """Pairs as pre-computed embedding rows (KGE or BERT), gathered on the host per batch."""

    def __init__(self, ratings, users, items, embeddings, batch_size=512, shuffle=False, seed=42, sample_weight=None):
        self.embeddings = embeddings
        super().__init__(ratings, users, items, batch_size=batch_size, shuffle=shuffle, seed=seed, sample_weight=sample_weight)

    def __getitem__(self, idx):
        r = self._batch_ratings(idx)
        return self._batch(idx, (self.embeddings[r[:, 0]], self.embeddings[r[:, 1]]), r[:, 2])


class HybridUserItemEmbeddings(_RatingsSequence):
    """Pairs as (graph, BERT) embedding rows for HybridCBRS."""

    def __init__(self, ratings, users, items, graph_embeddings, bert_embeddings, batch_size=512, shuffle=False,
                 seed=42, sample_weight=None):
        self.graph_embeddings = graph_embeddings
        self.bert_embeddings = bert_embeddings
        super().__init__(ratings, users, items, batch_size=batch_size, shuffle=shuffle, seed=seed, sample_weight=sample_weight)

    def __getitem__(self, idx):
        r = self._batch_ratings(idx)
        u, i = r[:, 0], r[:, 1]
        return self._batch(idx, (self.graph_embeddings[u], self.graph_embeddings[i],
                                 self.bert_embeddings[u], self.bert_embeddings[i]), r[:, 2])


class UserItemGraph(_RatingsSequence):
    """Pairs as node ids of the user-item(-properties) graph."""

    def __init__(self, ratings, users, items, adj_matrix, batch_size=512, shuffle=False, seed=42, sample_weight=None):
        self.adj_matrix = adj_matrix
        super().__init__(ratings, users, items, batch_size=batch_size, shuffle=shuffle, seed=seed, sample_weight=sample_weight)

    def __getitem__(self, idx):
        r = self._batch_ratings(idx)
        return self._batch(idx, (r[:, 0], r[:, 1]), r[:, 2])


class UserItemGraphEmbeddings:
    """Node ids plus the matching BERT rows (HybridBertGNN batches)."""

    def __init__(self, ratings, users, items, adj_matrix, embeddings, batch_size=512, shuffle=False, seed=42, sample_weight=None):
        self.ratings = ratings
        self.users = users
        self.items = items
        self.adj_matrix = adj_matrix
        self.graph_ids = UserItemGraph(ratings, users, items, adj_matrix,                # (the ids Sequence carries the weights)
                                       batch_size=batch_size, shuffle=shuffle, seed=seed, sample_weight=sample_weight)
        self.sample_weight = self.graph_ids.sample_weight
        self.embeddings = UserItemEmbeddings(ratings, users, items, embeddings,
                                             batch_size=batch_size, shuffle=shuffle, seed=seed)

    def __len__(self):
        return len(self.graph_ids)

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    def __getitem__(self, idx):
        (user_ids, item_ids), ratings = self.graph_ids[idx][:2]
        (user_embeddings, item_embeddings), _ = self.embeddings[idx]
        return self.graph_ids._batch(idx, (user_ids, item_ids, user_embeddings, item_embeddings), ratings)

    def on_epoch_end(self):
        self.graph_ids.on_epoch_end()
        self.embeddings.on_epoch_end()


class UserItemGraphPosNegSample:
    """Users with one positive and one negative candidate each, for the BPR loss (datasets.py:216-306 of the reference).

    `adj_matrix` is the 'binary' adjacency (preprocess.build_adjacency_matrix): 1 for a liked pair, an explicit 0 for a disliked one.
    As the reference does, the positives / negatives are the entries equal to 1 / 0 after ``todok()`` (which sums duplicates: a
    positive rated twice becomes 2 and is in neither list), ``self.adj_matrix`` keeps the positives only (the graph the model
    propagates over), and a user without an explicit negative gets `sample_size` candidates drawn once, with replacement, from the
    items it has not liked.  All draws come from one ``np.random.RandomState(seed)`` in the reference's order.

    ``__getitem__`` ignores `idx` and draws h = batch_size // 2 users, then one positive and one negative for each; it returns
    ``users = repeat(batch_users, 2)``, ``items = [pos; neg]``, ``ratings = [1]*h + [0]*h``.  So pair j of the first half is
    (batch_users[j // 2], pos_j), not (batch_users[j], pos_j): the reference's layout, kept as it is.

    ``pos_csr`` / ``neg_csr``: the per-user lists as CSR (int32 row pointers [|U|+1], int32 node ids), in the Sequence's own order —
    what ``fit()`` uploads for the device sampler.
    """

    def __init__(self, ratings, users, items, adj_matrix, batch_size=512, seed=42, sample_size=10):
        self.ratings = ratings
        self.users = users
        self.items = items
        coo = adj_matrix if sparse.isspmatrix_coo(adj_matrix) else adj_matrix.tocoo()
        coo.sum_duplicates()                              # what todok() does (in place): entries in (row, col) order = the dok's key order
        row, col, val = coo.row, coo.col, coo.data
        pos, neg = val == 1, val == 0
        if not neg.any():
            raise ValueError('Negative ratings are needed!!!')
        self.adj_matrix = sparse.coo_matrix((val[pos], (row[pos], col[pos])), shape=adj_matrix.shape, dtype=adj_matrix.dtype)

        self.contig_users = list(range(len(users)))
        self.contig_items = set(range(len(users), len(users) + len(items)))
        self.batch_size = batch_size
        self.seed = seed
        self.random_state = np.random.RandomState(seed)

        # per user: its items in key order (a stable sort by user of row-major keys keeps the columns ascending)
        n_users = len(users)

        def lists(mask):
            r, c = row[mask], col[mask]
            keep = r < n_users
            r, c = r[keep], c[keep]
            ptr = np.zeros(n_users + 1, dtype=np.int64)
            np.add.at(ptr, r + 1, 1)
            ptr = np.cumsum(ptr)
            return ptr, c.astype(np.int32)

        pos_ptr, pos_ids = lists(pos)
        neg_ptr, neg_ids = lists(neg)

        def sample_negatives(user, positives):
            if neg_ptr[user + 1] > neg_ptr[user]:
                return neg_ids[neg_ptr[user]:neg_ptr[user + 1]]
            return self.random_state.choice(list(set(self.contig_items) - set(positives)), size=sample_size)

        self.user_item_dict = []
        for user in self.contig_users:
            if pos_ptr[user + 1] == pos_ptr[user]:
                raise ValueError("user {} has no positive rating: every user needs one to be sampled".format(user))
            positives = pos_ids[pos_ptr[user]:pos_ptr[user + 1]]
            self.user_item_dict.append((positives, sample_negatives(user, positives)))
        self.pos_csr = (pos_ptr.astype(np.int32), pos_ids)
        neg_lists = [np.asarray(n, dtype=np.int32) for _, n in self.user_item_dict]
        self.neg_csr = (np.concatenate([[0], np.cumsum([len(n) for n in neg_lists])]).astype(np.int32),
                        np.concatenate(neg_lists).astype(np.int32) if neg_lists else np.zeros(0, np.int32))

    def __len__(self):
        return int(np.ceil(len(self.ratings) / self.batch_size))

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    def __getitem__(self, idx):
        h = self.batch_size // 2
        batch_users = self.random_state.choice(self.contig_users, size=h)
        pos_items = np.fromiter((self.random_state.choice(self.user_item_dict[user][0]) for user in batch_users), dtype='int32')
        neg_items = np.fromiter((self.random_state.choice(self.user_item_dict[user][1]) for user in batch_users), dtype='int32')
        items = np.concatenate([pos_items, neg_items])
        users = np.repeat(batch_users, 2)
        ratings = np.concatenate([np.full(h, 1), np.full(h, 0)])
        return (users, items), ratings

    def device_batch(self, step):
        """The batch the device sampler draws at `step` (the batches of fit()), in __getitem__'s layout."""
        return bpr_device_batch(self.pos_csr, self.neg_csr, len(self.users), self.seed, step, self.batch_size // 2)


# ---- the device sampler's draws, restated (csrc/amar_bpr.hip, include/amar_hip.h: amar_bpr_sample_i32) -----------------------
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: counter [n, 4] uint32, key (k0, k1) -> [n, 4] uint32."""
    c = np.array(counter, dtype=np.uint32).reshape(-1, 4).copy()
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    mask = np.uint64(0xFFFFFFFF)
    with np.errstate(over='ignore'):
        for r in range(10):
            if r:
                k0, k1 = k0 + _PHILOX_W0, k1 + _PHILOX_W1
            p0 = _PHILOX_M0 * c[:, 0].astype(np.uint64)
            p1 = _PHILOX_M1 * c[:, 2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & mask).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & mask).astype(np.uint32)
            c = np.stack([hi1 ^ c[:, 1] ^ k0, lo1, hi0 ^ c[:, 3] ^ k1, lo0], axis=1)
    return c


def _pick(word, n):
    return ((word.astype(np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def bpr_device_batch(pos_csr, neg_csr, n_users, seed, step, h):
    """What amar_bpr_sample_i32 writes for (seed, step): draw j uses Philox4x32-10 with key = (seed_lo, seed_hi) and counter =
    (j, step_lo, step_hi, 0); word 0 picks the user among n_users, word 1 its positive, word 2 its negative candidate, each as
    (uint64(word) * n) >> 32.  Returns ((users[2h], items[2h]), ratings[2h]) in the reference's layout (int64 ids, int64 labels)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    j = np.arange(h, dtype=np.uint64)
    counter = np.stack([j, np.full(h, step & 0xFFFFFFFF, np.uint64), np.full(h, step >> 32, np.uint64), np.zeros(h, np.uint64)], axis=1)
    w = philox4x32_10(counter.astype(np.uint32), (seed & 0xFFFFFFFF, seed >> 32))
    users = _pick(w[:, 0], n_users)
    (pp, pi), (npt, ni) = pos_csr, neg_csr
    pp, npt = np.asarray(pp, np.int64), np.asarray(npt, np.int64)
    pos = np.asarray(pi)[pp[users] + _pick(w[:, 1], pp[users + 1] - pp[users])].astype(np.int64)
    neg = np.asarray(ni)[npt[users] + _pick(w[:, 2], npt[users + 1] - npt[users])].astype(np.int64)
    return (np.repeat(users, 2), np.concatenate([pos, neg])), np.concatenate([np.ones(h, np.int64), np.zeros(h, np.int64)])


# ---- BPR triples: per-user pairs, negatives uniform over a user's unobserved items (amar_bpr_sample_triplets_i32) ----------------
SAMPLE_BY = {'user': 0, 'interaction': 1}                             # the kernel's `mode`


def _philox_words(c0, step, c3, seed):
    n = len(c0)
    counter = np.stack([np.asarray(c0, np.uint64), np.full(n, step & 0xFFFFFFFF, np.uint64), np.full(n, step >> 32, np.uint64),
                        np.full(n, c3, np.uint64)], axis=1)
    return philox4x32_10(counter.astype(np.uint32), (seed & 0xFFFFFFFF, seed >> 32))


def nth_non_excluded(excluded, r):
    """The r-th (0-based) item outside the strictly ascending list `excluded` (0-based item numbers): with e_q the q-th excluded
    item, e_q - q counts the free items below it and never decreases, so m = #{q : e_q - q <= r} is one binary search and the
    answer is r + m.  `r` may be an array."""
    excluded = np.asarray(excluded, dtype=np.int64)
    return np.asarray(r, dtype=np.int64) + np.searchsorted(excluded - np.arange(len(excluded)), r, side='right')


def bpr_triplet_device_batch(pos_csr, excl_csr, n_users, n_items, item_base, seed, step, h, n_negatives=1, sample_by='user'):
    """What amar_bpr_sample_triplets_i32 writes for (seed, step): h triples, K = n_negatives of them per draw (P = h / K draws).
    Philox4x32-10 with key = (seed_lo, seed_hi), pick(w, n) = (uint64(w) * n) >> 32.
      draw j < P, counter (j, step_lo, step_hi, 0): 'user': user = pick(w0, n_users), pos = its pick(w1, n_pos)-th positive;
        'interaction': e = pick(w0, all positives), user = the row that holds entry e, pos = pos_ids[e].
      triple t = j * K + k, counter (t, step_lo, step_hi, 1): neg = item_base + the pick(w0, n_items - d)-th item outside the user's
        exclusion row (d its length; `nth_non_excluded`): uniform over the complement, one draw, no rejection.
    Returns ((users[2h], items[2h]), ratings[2h]) with users[t] = users[h + t], items = [pos; neg], ratings = [1]*h + [0]*h (int64)."""
    if sample_by not in SAMPLE_BY:
        raise ValueError("sample_by must be 'user' or 'interaction' (got {!r})".format(sample_by))
    K, h = int(n_negatives), int(h)
    if K < 1 or h < 1 or h % K:
        raise ValueError("h = {} triples do not split into draws of n_negatives = {}".format(h, K))
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    (pp, pi), (xp, xi) = pos_csr, excl_csr
    pp, xp, pi, xi = np.asarray(pp, np.int64), np.asarray(xp, np.int64), np.asarray(pi, np.int64), np.asarray(xi, np.int64)
    w = _philox_words(np.arange(h // K), step, 0, seed)
    if SAMPLE_BY[sample_by] == 0:
        users = _pick(w[:, 0], n_users)
        pos = pi[pp[users] + _pick(w[:, 1], pp[users + 1] - pp[users])]
    else:
        e = _pick(w[:, 0], pp[n_users])
        users = np.searchsorted(pp[:n_users], e, side='right') - 1    # the largest r with pos_ptr[r] <= e
        pos = pi[e]
    users, pos = np.repeat(users, K), np.repeat(pos, K)
    d = xp[users + 1] - xp[users]
    r = _pick(_philox_words(np.arange(h), step, 1, seed)[:, 0], n_items - d)
    neg = np.empty(h, np.int64)
    for t in range(h):
        row = xi[xp[users[t]]:xp[users[t] + 1]] - item_base
        neg[t] = item_base + nth_non_excluded(row, r[t])
    return (np.concatenate([users, users]), np.concatenate([pos, neg])), np.concatenate([np.ones(h, np.int64), np.zeros(h, np.int64)])


def _user_lists(user_ids, item_ids, n_users):
    """CSR (int32 row pointers [n_users + 1], int32 ids) of the distinct (user, item) pairs, items ascending within a user."""
    pairs = np.unique(np.stack([np.asarray(user_ids, np.int64), np.asarray(item_ids, np.int64)], axis=1), axis=0) \
        if len(user_ids) else np.zeros((0, 2), np.int64)
    ptr = np.zeros(n_users + 1, dtype=np.int64)
    np.add.at(ptr, pairs[:, 0] + 1, 1)
    return np.cumsum(ptr).astype(np.int32), pairs[:, 1].astype(np.int32)


class UserItemGraphTriplets:
    """BPR triples (user, positive, negative) drawn per user: both items of a pair are scored against the user they were drawn for,
    and the negative is uniform over the items outside the user's exclusion list (Rendle et al.'s BPR; LightGCN's sampler).

    `adj_matrix` is the ordinary 'unary' training graph the model propagates over, kept as it is.  The positives are the training
    ratings with label 1, deduplicated, ascending per user.  ``exclude='positives'``: anything the user has not liked is a candidate,
    explicit dislikes included; ``exclude='rated'``: every item the user rated in training is excluded.  ``sample_by='user'`` draws
    users uniformly, ``'interaction'`` draws positive interactions uniformly.  `n_negatives` triples share one (user, positive).

    A batch holds h = batch_size // 2 triples as ``users[t] = users[h + t]``, ``items = [pos; neg]``, ``ratings = [1]*h + [0]*h``:
    BPRLoss pairs rows (t, h + t).  There is no host RNG stream: ``__getitem__(idx)`` is ``device_batch(idx)``, the batch the device
    sampler draws at step `idx`.  An epoch has ceil(#positives / (h // n_negatives)) batches, about one draw per training positive.

    ``pos_csr`` / ``excl_csr``: the per-user lists as CSR (int32 row pointers [|U|+1], int32 node ids), what ``fit()`` uploads."""

    def __init__(self, ratings, users, items, adj_matrix, batch_size=512, seed=42, n_negatives=1, sample_by='user',
                 exclude='positives'):
        if sample_by not in SAMPLE_BY:
            raise ValueError("sample_by must be 'user' or 'interaction' (got {!r})".format(sample_by))
        if exclude not in ('positives', 'rated'):
            raise ValueError("exclude must be 'positives' or 'rated' (got {!r})".format(exclude))
        h, K = int(batch_size) // 2, int(n_negatives)
        if h < 1:
            raise ValueError("a BPR batch needs batch_size >= 2")
        if K < 1 or h % K:
            raise ValueError("batch_size // 2 = {} triples do not split into draws of n_negatives = {}".format(h, n_negatives))
        self.ratings, self.users, self.items, self.adj_matrix = ratings, users, items, adj_matrix
        self.batch_size, self.seed, self.n_negatives, self.sample_by, self.exclude = int(batch_size), seed, K, sample_by, exclude
        n_users = len(users)
        self.n_items, self.item_base = len(items), n_users
        r = np.asarray(ratings)
        liked = r[:, 2] == 1
        self.pos_csr = _user_lists(r[liked, 0], r[liked, 1], n_users)
        self.excl_csr = self.pos_csr if exclude == 'positives' else _user_lists(r[:, 0], r[:, 1], n_users)
        for ids in (self.pos_csr[1], self.excl_csr[1]):
            if len(ids) and (ids.min() < self.item_base or ids.max() >= self.item_base + self.n_items):
                raise ValueError("ratings hold item ids outside [{}, {})".format(self.item_base, self.item_base + self.n_items))
        empty = np.flatnonzero(np.diff(self.pos_csr[0]) < 1)
        if len(empty):
            raise ValueError("user {} has no positive rating: every user needs one to be sampled".format(int(empty[0])))
        full = np.flatnonzero(np.diff(self.excl_csr[0]) >= self.n_items)
        if len(full):
            raise ValueError("user {} has no candidate left: its exclusion list covers every item".format(int(full[0])))

    def __len__(self):
        return int(np.ceil(len(self.pos_csr[1]) / (self.batch_size // 2 // self.n_negatives)))

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    def __getitem__(self, idx):
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        return self.device_batch(idx)

    def device_batch(self, step):
        """The batch the device sampler draws at `step` (the batches of fit())."""
        return bpr_triplet_device_batch(self.pos_csr, self.excl_csr, len(self.users), self.n_items, self.item_base, self.seed, step,
                                        self.batch_size // 2, self.n_negatives, self.sample_by)


# ---- the dropout draws, restated (csrc/amar_philox.h; include/amar_hip.h: amar_dropout_f32, amar_gat_layer_dropout_f32) -------------
def dropout_threshold(rate):
    """A 32-bit word keeps its value iff word >= T = min(2^32 - 1, floor(rate * 2^32 + 0.5)): P(keep) = 1 - T / 2^32."""
    return min(0xFFFFFFFF, int(float(rate) * 4294967296.0 + 0.5))


def dropout_scale(rate):
    """What kept values are multiplied by: the float32 nearest to 1 / (1 - rate)."""
    return np.float32(1.0 / (1.0 - float(rate)))


def dropout_stream_seed(seed, index):
    """The 64-bit key of the index-th dropout stream under `seed` (engine.set_seed restarts the count; every Trainer that drops takes
    the next one, so two models of one process do not share a stream and a re-run with the same seed repeats it): words 0 and 1 of
    Philox4x32-10 with key = (seed_lo, seed_hi) and counter = (index, 0, 0, 0x44524F50), as word0 | word1 << 32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(np.array([[int(index) & 0xFFFFFFFF, 0, 0, 0x44524F50]], dtype=np.uint32), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return int(w[0]) | (int(w[1]) << 32)


def _dropout_words(seed, step, site, c0, c3):
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    if not 1 <= int(site) <= 255:
        raise ValueError("site must lie in 1..255")
    c0, c3 = np.asarray(c0, dtype=np.uint64), np.asarray(c3, dtype=np.uint64)
    n = len(c0)
    counter = np.stack([c0, np.full(n, step & 0xFFFFFFFF, np.uint64), np.full(n, step >> 32, np.uint64),
                        (np.uint64(int(site)) << np.uint64(24)) | c3], axis=1)
    return philox4x32_10(counter.astype(np.uint32), (seed & 0xFFFFFFFF, seed >> 32))


def dropout_node_mask(seed, step, site, shape, rate):
    """The keep mask (bool [n, C]) amar_dropout_f32 applies to an [n, C] slice: call e = r * ceil(C / 4) + c // 4 has counter
    (e, step_lo, step_hi, site << 24) and its word c % 4 decides column c of row r (the surplus words of a row's last call are
    unused when C is no multiple of 4)."""
    n, c = int(shape[0]), int(shape[1])
    qpr = (c + 3) // 4
    if n * qpr >= 1 << 31:
        raise ValueError("slice too large for one counter word")
    w = _dropout_words(seed, step, site, np.arange(n * qpr, dtype=np.uint64), np.zeros(n * qpr, np.uint64))
    return (w.reshape(n, 4 * qpr)[:, :c] >= np.uint32(dropout_threshold(rate)))


def edge_ordinals(rowptr, colidx):
    """Per stored entry: its position among the entries of its row with the same column (columns sorted per row), modulo 255."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    nnz = len(colidx)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    idx = np.arange(nnz)
    first = np.ones(nnz, dtype=bool)
    first[1:] = (rows[1:] != rows[:-1]) | (colidx[1:] != colidx[:-1])
    start = np.maximum.accumulate(np.where(first, idx, 0))
    return rows, (idx - start) % 255


def dropout_edge_mask(seed, step, site, rowptr, colidx, self_loop, rate):
    """The keep bits of amar_gat_layer_dropout_f32 / amar_gat_bwd_dropout_f32: (mask [nnz] per stored entry in CSR order, mask [n] of
    the added self loops or None).  Entry (target i, source j, ordinal o): counter (min(i, j) | o << 24, step_lo, step_hi,
    site << 24 | max(i, j)), word 0; the added self loop of node i is (i, i) with ordinal slot 255.  Entry (i, j, o) and its mirror
    (j, i, o) of a symmetric multiset share the bit; parallel entries (different o) draw independently."""
    rowptr = np.asarray(rowptr, np.int64)
    n = len(rowptr) - 1
    if n > 1 << 24:
        raise ValueError("edge dropout numbers nodes in 24 bits")
    t = np.uint32(dropout_threshold(rate))
    rows, ordinal = edge_ordinals(rowptr, colidx)
    cols = np.asarray(colidx, np.int64)
    lo, hi = np.minimum(rows, cols).astype(np.uint64), np.maximum(rows, cols).astype(np.uint64)
    w = _dropout_words(seed, step, site, lo | (ordinal.astype(np.uint64) << np.uint64(24)), hi)
    loops = None
    if self_loop:
        i = np.arange(n, dtype=np.uint64)
        loops = _dropout_words(seed, step, site, i | (np.uint64(255) << np.uint64(24)), i)[:, 0] >= t
    return w[:, 0] >= t, loops


def holdout_split(ratings, fraction, seed):
    """Split rating rows into (kept, held out): about `fraction` of the rows, visited in the order of a generator seeded with `seed`,
    move to the held-out part — a row only while its user AND its item each keep at least one other row in the kept part, so every
    user and item of `ratings` still occurs in the kept part (the loaders refuse identifiers absent from training).  Both parts keep
    the input's row order; the same seed gives the same split.  Fewer than round(fraction * n) rows move only when no further row may:
    at least min(round(fraction * n), n - |users| - |items|) always do."""
    r = np.asarray(ratings)
    if not 0.0 <= float(fraction) < 1.0:
        raise ValueError("fraction must lie in [0, 1) (got {!r})".format(fraction))
    n = len(r)
    target = int(round(float(fraction) * n))
    moved = np.zeros(n, dtype=bool)
    if n == 0 or target == 0:
        return r[~moved], r[moved]
    _, u_inv = np.unique(r[:, 0], return_inverse=True)
    _, i_inv = np.unique(r[:, 1], return_inverse=True)
    u_left, i_left = np.bincount(u_inv), np.bincount(i_inv)
    done = 0
    for row in np.random.RandomState(int(seed)).permutation(n).tolist():
        u, i = u_inv[row], i_inv[row]
        if u_left[u] > 1 and i_left[i] > 1:
            moved[row] = True
            u_left[u] -= 1
            i_left[i] -= 1
            done += 1
            if done == target:
                break
    return r[~moved], r[moved]

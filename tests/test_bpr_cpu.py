"""BPR training, host side: the 'binary' adjacency, the sample Sequence and its loader against the reference's own code
(tests/golden/make_bpr_reference_golden.py), the loss lookup, and the numpy statement of the device sampler's draws."""
import os

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd.data import datasets, loaders
from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bpr_reference.npz')


@pytest.fixture(scope='module')
def ref():
    return np.load(GOLDEN)


def _write(tmp_path, ref):
    paths = {}
    for k in ('train', 'test'):
        paths[k] = str(tmp_path / (k + '.tsv'))
        np.savetxt(paths[k], ref[k + '_raw'], fmt='%d', delimiter='\t')
    return paths


def test_binary_adjacency_matches_reference(ref):
    adj = build_adjacency_matrix(ref['train_ratings'], ref['users'], ref['items'], type_adjacency='binary')
    assert adj.shape == tuple(ref['binary_shape'])
    np.testing.assert_array_equal(adj.row, ref['binary_row'])
    np.testing.assert_array_equal(adj.col, ref['binary_col'])
    np.testing.assert_array_equal(adj.data, ref['binary_data'])
    assert (adj.data == 0).any()                                     # explicit zeros are kept


def test_other_loaders_refuse_binary(tmp_path, ref):
    p = _write(tmp_path, ref)
    with pytest.raises(NotImplementedError):
        loaders.load_user_item_graph(p['train'], p['test'], type_adjacency='binary')


def test_sample_loader_and_sequence_match_reference(tmp_path, ref):
    p = _write(tmp_path, ref)
    train, test = loaders.load_user_item_graph_sample(p['train'], p['test'], train_batch_size=int(ref['batch_size']))
    assert isinstance(train, datasets.UserItemGraphPosNegSample) and isinstance(test, datasets.UserItemGraph)
    assert train.seed == int(ref['seed'])
    pos = train.adj_matrix
    np.testing.assert_array_equal(pos.row, ref['pos_row'])
    np.testing.assert_array_equal(pos.col, ref['pos_col'])
    np.testing.assert_array_equal(pos.data, ref['pos_data'])
    assert test.adj_matrix is not None and len(train) == int(ref['n_batches_len'])
    for name, csr in (('pos', train.pos_csr), ('neg', train.neg_csr)):
        assert csr[0].dtype == np.int32 and csr[1].dtype == np.int32
        np.testing.assert_array_equal(csr[0], ref[name + '_ptr'])
        np.testing.assert_array_equal(csr[1], ref[name + '_ids'])
    for k, (ul, il) in enumerate(train.user_item_dict):
        np.testing.assert_array_equal(ul, ref['pos_ids'][ref['pos_ptr'][k]:ref['pos_ptr'][k + 1]])
        np.testing.assert_array_equal(il, ref['neg_ids'][ref['neg_ptr'][k]:ref['neg_ptr'][k + 1]])
    for b in range(ref['batch_users'].shape[0]):
        (u, i), y = train[b]
        np.testing.assert_array_equal(u, ref['batch_users'][b])
        np.testing.assert_array_equal(i, ref['batch_items'][b])
        np.testing.assert_array_equal(y, ref['batch_ratings'][b])


def test_duplicated_positive_is_in_neither_list(ref):
    tr = ref['train_ratings']
    _, first, counts = np.unique(tr[:, :2], axis=0, return_index=True, return_counts=True)
    u, i = tr[first[counts > 1][0], :2]
    seq = datasets.UserItemGraphPosNegSample(tr, ref['users'], ref['items'],
                                             build_adjacency_matrix(tr, ref['users'], ref['items'], type_adjacency='binary'))
    assert i not in seq.user_item_dict[u][0] and i not in seq.user_item_dict[u][1]


def test_no_negatives_raise(ref):
    tr = ref['train_ratings'].copy()
    tr[:, 2] = 1
    adj = build_adjacency_matrix(tr, ref['users'], ref['items'], type_adjacency='binary')
    with pytest.raises(ValueError) as e:
        datasets.UserItemGraphPosNegSample(tr, ref['users'], ref['items'], adj)
    assert str(e.value) == str(ref['no_negatives_error'])


def test_user_without_positive_is_named(ref):
    tr = ref['train_ratings'].copy()
    tr[tr[:, 0] == 5, 2] = 0
    adj = build_adjacency_matrix(tr, ref['users'], ref['items'], type_adjacency='binary')
    with pytest.raises(ValueError, match='user 5 '):
        datasets.UserItemGraphPosNegSample(tr, ref['users'], ref['items'], adj)


def test_bpr_loss_resolves_by_name():
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities import losses
    assert hasattr(experiment, 'losses') and experiment.losses is losses
    assert hasattr(losses, 'BPRLoss') and not hasattr(losses, 'binary_crossentropy')
    loss = getattr(losses, 'BPRLoss')()
    assert losses.loss_kind(loss) == 'bpr' and losses.loss_kind('binary_crossentropy') == 'bce' and losses.loss_kind(None) == 'bce'
    p = np.array([0.9, 0.2, 0.4, 0.3, 0.77])                         # odd: the last one is dropped
    x = p[:2] - p[2:4]
    assert loss(None, p) == pytest.approx(-np.mean(np.log(1 / (1 + np.exp(-x)))), rel=1e-14)


def test_philox_known_answer():
    # Random123's known-answer vectors for philox4x32-10
    out = datasets.philox4x32_10([[0, 0, 0, 0]], (0, 0))
    assert [hex(int(w)) for w in out[0]] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    out = datasets.philox4x32_10([[0xffffffff] * 4], (0xffffffff, 0xffffffff))
    assert [hex(int(w)) for w in out[0]] == ['0x408f276d', '0x41c83b0e', '0xa20bc7c6', '0x6d5451fd']


def test_device_batch_restatement_is_self_consistent(ref):
    tr = ref['train_ratings']
    seq = datasets.UserItemGraphPosNegSample(tr, ref['users'], ref['items'],
                                             build_adjacency_matrix(tr, ref['users'], ref['items'], type_adjacency='binary'),
                                             batch_size=64)
    n_users = len(ref['users'])
    seen = set()
    for step in (0, 1, 2, 2 ** 32 + 5):
        (u, i), y = seq.device_batch(step)
        h = 32
        assert u.shape == (64,) and i.shape == (64,) and np.array_equal(y, [1] * h + [0] * h)
        assert np.array_equal(u[0::2], u[1::2]) and u.min() >= 0 and u.max() < n_users
        users = u[0::2]
        for j in range(h):
            assert i[j] in seq.user_item_dict[users[j]][0]
            assert i[h + j] in seq.user_item_dict[users[j]][1]
        again = seq.device_batch(step)
        assert np.array_equal(again[0][0], u) and np.array_equal(again[0][1], i)
        seen.add(tuple(i))
    assert len(seen) == 4                                            # every step draws anew
    assert not np.array_equal(datasets.bpr_device_batch(seq.pos_csr, seq.neg_csr, n_users, 43, 0, 32)[0][1],
                              seq.device_batch(0)[0][1])

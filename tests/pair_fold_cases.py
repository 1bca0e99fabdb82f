"""The cases of tests/test_pair_fold_gpu.py, their float64 reference and their launch, and — run as a program — the child process that
scores every case with AMAR_PAIR_MFMA=f32 in its environment (the switch is read once per process, csrc/amar_chain.hip, so the parent
cannot flip it): `python tests/pair_fold_cases.py OUT.npz` writes one float32 vector per case name.  Exit code 0 = scored.

The head: x = relu(A[ia - base_a] + B[ib - base_b]), y = relu(x . W1 + b1) (W wide), score = sigmoid(y . w2 + b2).  Tables of 64 users and
48 items; W = 48 is the pair-stage kernel with three f32 tiles (the last one folded over parts), 16 and 80 the other odd tile counts and 32 an
even one: the route sends those three to the generic kernel (f32 instruction in both processes), which the test asserts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

DEV = 'cuda'
N_USERS, N_ITEMS = 64, 48
WIDTHS = (16, 48, 80, 32)
PS = (1, 15, 16, 17, 31, 32, 33, 129, 4 * 128 + 5)
VARIANTS = ('plain', 'indexed', 'based')                               # based: the ids form with base_a = 7, base_b = 11 (and an out_index)
EDGES = ('last_tile_only', 'zero_last_tile', 'zero_acts', 'bias_only')
EDGE_P = 129
ACTS = ['relu', 'sigmoid']


class Case:
    def __init__(self, W, P, variant, edge=None):
        self.W, self.P, self.variant, self.edge = W, P, variant, edge
        self.name = 'w{}-p{}-{}{}'.format(W, P, variant, '-' + edge if edge else '')
        self.base_a, self.base_b = (7, 11) if variant == 'based' else (0, 0)
        self.indexed = variant != 'plain'
        self.dims = [W, W, 1]

    def __repr__(self):
        return self.name

    def draw(self):
        """Seeded float32 operands.  The tables carry base_* leading rows that no id reaches (NaN: a read before the view poisons the score)."""
        W = self.W
        rng = np.random.default_rng(1000 * W + (EDGES.index(self.edge) + 1 if self.edge else 0))
        A = (rng.standard_normal((N_USERS, W)) * 1.5).astype(np.float32)
        B = (rng.standard_normal((N_ITEMS, W)) * 1.5).astype(np.float32)
        w1 = (rng.uniform(-1, 1, (W, W)) * np.sqrt(6.0 / (2 * W))).astype(np.float32)
        b1 = rng.uniform(-0.2, 0.2, W).astype(np.float32)
        w2 = (rng.uniform(-1, 1, (W, 1)) * np.sqrt(6.0 / (W + 1))).astype(np.float32)
        b2 = rng.uniform(-0.2, 0.2, 1).astype(np.float32)
        k0 = 16 * ((W + 15) // 16 - 1)                                 # first input feature of the last f32 tile
        if self.edge == 'last_tile_only':                              # every other unit's only non-zero weights lie in the last tile
            w1[:k0, ::2] = 0
        elif self.edge == 'zero_last_tile':
            w1[k0:, :] = 0
        elif self.edge == 'zero_acts':                                 # the last tile's activations are exactly 0, and every one of each other user
            A[:, k0:], B[:, k0:] = -np.abs(A[:, k0:]), -np.abs(B[:, k0:])
            A[::2, :] = -np.abs(A[::2, :]) - 100
        elif self.edge == 'bias_only':                                 # all inputs negative: x = 0 exactly
            A, B = -np.abs(A) - 1, -np.abs(B)
        rng = np.random.default_rng(77 * W + self.P + 13 * VARIANTS.index(self.variant))
        ra, rb = rng.integers(0, N_USERS, self.P), rng.integers(0, N_ITEMS, self.P)
        perm = rng.permutation(self.P).astype(np.int32) if self.indexed else None
        return dict(A=A, B=B, ks=[w1, w2], bs=[b1, b2], ra=ra, rb=rb, perm=perm)

    def reference(self, d):
        """The scores in float64, in the order of the list."""
        x = np.maximum(d['A'].astype(np.float64)[d['ra']] + d['B'].astype(np.float64)[d['rb']], 0)
        y = np.maximum(x @ d['ks'][0].astype(np.float64) + d['bs'][0].astype(np.float64), 0)
        z = y @ d['ks'][1].astype(np.float64) + d['bs'][1].astype(np.float64)
        return (1.0 / (1.0 + np.exp(-z)))[:, 0]


def all_cases():
    return ([Case(W, P, v) for W in WIDTHS for P in PS for v in VARIANTS] +
            [Case(W, EDGE_P, 'indexed', e) for W in WIDTHS for e in EDGES])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(arr, base):
    buf = torch.full((arr.shape[0] + base, arr.shape[1]), float('nan'), dtype=torch.float32, device=DEV)
    buf[base:].copy_(_t(arr))
    return buf[base:]


class Launch:
    """The device operands of one case; `run()` launches once and returns (scores in the order of the list, as numpy; the route)."""

    def __init__(self, hip, case, d=None):
        self.hip, self.case = hip, case
        self.d = d = case.draw() if d is None else d
        blob, dims = hip.chain_pack(d['ks'], d['bs'])
        assert dims == case.dims
        self.blob = _t(blob)
        self.A, self.B = _table(d['A'], case.base_a), _table(d['B'], case.base_b)
        self.ia, self.ib = _t((d['ra'] + case.base_a).astype(np.int32)), _t((d['rb'] + case.base_b).astype(np.int32))
        self.perm = _t(d['perm']) if case.indexed else None

    def run(self, ia=None, ib=None, out_index='own'):
        c = self.case
        out_index = self.perm if isinstance(out_index, str) else out_index
        buf = torch.full((c.P, 3), 7.0, dtype=torch.float32, device=DEV)      # the score column between two sentinel columns
        out = buf[:, 1:2]
        out.fill_(float('nan'))
        kw = dict(ids_a=self.ia if ia is None else ia, base_a=c.base_a, B=self.B, ids_b=self.ib if ib is None else ib, base_b=c.base_b,
                  sum_inputs=True, in_act='relu', out_index=out_index)
        route = self.hip.chain_route(self.A, self.blob, c.dims, ACTS, out, **kw)
        self.hip.chain(self.A, self.blob, c.dims, ACTS, out, **kw)
        torch.cuda.synchronize()
        assert bool((buf[:, 0] == 7.0).all()) and bool((buf[:, 2] == 7.0).all()), '{}: a store outside the score column'.format(c)
        got = out[:, 0].contiguous()
        if out_index is not None:
            got = got[out_index.long()]
        return got.cpu().numpy(), route


def main():
    from deep_cbrs_amar_renaissance_amd import capi
    assert os.environ.get('AMAR_PAIR_MFMA') == 'f32' and torch.cuda.is_available()
    capi.load()
    scores = {}
    for case in all_cases():
        scores[case.name], route = Launch(capi, case).run()
        assert not route['split'], (case, route)
    np.savez(sys.argv[1], **scores)
    print('scored {} cases'.format(len(scores)))


if __name__ == '__main__':
    main()

"""The two-branch head's launch helper of tests/test_entry_points_gpu.py, and — run as a program — the child process that scores the common
head with AMAR_PAIR_MFMA=f32 in its environment (the switch is read once per process, csrc/amar_chain.hip, so the parent cannot flip it):
`python tests/dual_chain_worker.py OUT.npy` writes the scores of `common_case()`.  Exit code 0 = scored."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests import entry_point_ref as ref

DEV = 'cuda'
PAD = 12                                                              # guard columns of a sliced table: lda = D + PAD, the slice starts at column 4


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pack(hip, h):
    """chain_pack per branch and trunk, concatenated as models/hybrid.py:_dual_plan does."""
    blobs = []
    for layers in (h['branch'][0], h['branch'][1], h['trunk']):
        if layers:
            blob, _ = hip.chain_pack([w for w, _ in layers], [b for _, b in layers])
            blobs.append(blob)
    return _t(np.concatenate(blobs))


def device_table(table, base, sliced):
    """The table as the kernel sees it: a view that starts `base` rows into a buffer whose first rows are NaN (ids = row + base, so
    ids - base index the view), and with `sliced` a column slice of a wider buffer whose other columns are NaN too (a read before the view
    or past the slice poisons the score)."""
    rows, D = table.shape
    buf = torch.full((rows + base, D + PAD if sliced else D), float('nan'), device=DEV)
    view = buf[base:, 4:4 + D] if sliced else buf[base:]
    view.copy_(_t(table))
    return view


def run(hip, h, wpack, rows_a, rows_b, bases_a, bases_b, P, in_act, branch_acts, trunk_acts, sliced=False, strided_out=False, out_index=None):
    """One launch.  rows_*[k]: row of table k per pair (None: the table is read in place, row p); ids = rows + base travel to the device.
    Returns (scores [P] as numpy, the whole out buffer).  out starts as NaN; a strided out is column 1 of a [P, 3] buffer."""
    code = lambda n: None if n == 'none' else n                                                            # noqa: E731
    D = h['A'][0].shape[1]
    tabs_a = [device_table(h['A'][k], bases_a[k] if rows_a[k] is not None else 0, sliced) for k in range(2)]
    tabs_b = [device_table(h['B'][k], bases_b[k] if rows_b[k] is not None else 0, sliced) for k in range(2)]
    ids_a = [None if r is None else _t((r + b).astype(np.int32)) for r, b in zip(rows_a, bases_a)]
    ids_b = [None if r is None else _t((r + b).astype(np.int32)) for r, b in zip(rows_b, bases_b)]
    buf = torch.full((P, 3 if strided_out else 1), float('nan'), device=DEV)
    out = buf[:, 1:2] if strided_out else buf
    hip.dual_chain(tabs_a, tabs_b, ids_a, ids_b, bases_a, bases_b, D, code(in_act), [code(a) for a in branch_acts], h['trunk_dims'],
                   [code(a) for a in trunk_acts], wpack, out, out_index=out_index)
    torch.cuda.synchronize()
    return out[:, 0].cpu().numpy(), buf


def common_case():
    """The common head: D = W = 64, one branch layer, a three-layer trunk, ReLU throughout, all four id lists, P = 50 003."""
    h = ref.draw_dual_head(np.random.default_rng(77), 64, 64, 1, 3, 3000)
    rng = np.random.default_rng(78)
    P = 50_003
    return h, [rng.integers(0, 2900, P) for _ in range(2)], [rng.integers(0, 2900, P) for _ in range(2)], P


def score_common_case(hip):
    h, rows_a, rows_b, P = common_case()
    return run(hip, h, pack(hip, h), rows_a, rows_b, [3, 5], [7, 11], P, 'relu', ['relu'], ['relu', 'relu', 'sigmoid'])[0]


def main():
    from deep_cbrs_amar_renaissance_amd import capi
    assert os.environ.get('AMAR_PAIR_MFMA') == 'f32' and torch.cuda.is_available()
    capi.load()
    np.save(sys.argv[1], score_common_case(capi))
    print('scored')


if __name__ == '__main__':
    main()

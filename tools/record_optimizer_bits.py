#!/usr/bin/env python
"""Record tests/golden/optimizer_bits.npz: what tests/optimizer_bits_cases.py pins of the optimizer kernels, the advance entry points
and six-batch training loops (short arrays as they are, longer ones as their SHA-256).  Run it on the GPU at the commit
whose bits are to be kept (a refactor of the optimizer code records at its parent).  Every case runs twice; the file is written only
if the two runs of every case agree.
usage: python tools/record_optimizer_bits.py [output.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import optimizer_bits_cases as ob  # noqa: E402


def main(out):
    from deep_cbrs_amar_renaissance_amd import capi
    capi.load()
    specs = ob._specs()
    runs = [('multi/' + case + '/', lambda case=case: ob.multi_bits(capi, case, specs[case])) for case in specs]
    runs.append(('advance/', lambda: ob.advance_bits(capi)))
    runs += [('train/{}/{}/{}/'.format(*case), lambda case=case: ob.train_bits(*case)) for case in ob.train_cases()]
    arrays, bad = {}, []
    for name, run in runs:
        first, second = run(), run()
        same = set(first) == set(second) and all(np.array_equal(first[k], second[k]) for k in first)
        print('{:40s} {:4d} arrays: {}'.format(name, len(first), 'repeats bit for bit' if same else 'DIFFERS between its own runs'), flush=True)
        if not same:
            bad.append(name)
        arrays.update(ob.pack(name, first)[0])
    if bad:
        sys.exit("not written: {} do not repeat their own bits".format(', '.join(bad)))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print('wrote {} ({} members, {} bytes)'.format(out, len(arrays), os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else ob.GOLDEN)

#!/usr/bin/env python
"""Record tests/golden/train_step_bits.npz: every trainable parameter, as uint32, after the two training steps of each case of
tests/train_bits_cases.py.  Run it on the GPU at the commit whose bits are to be kept (a refactor of the training code records at
its parent).  Every case is trained twice from the same seed on both routes (the body run eagerly, and captured and replayed); the
file is written only if all four runs of every case agree bit for bit, so one array per parameter is all it holds.
usage: python tools/record_train_bits.py [output.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import train_bits_cases as tb  # noqa: E402


def main(out):
    arrays, bad = {}, []
    for name in tb.CASES:
        runs = [tb.train_bits(name, route) for route in tb.ROUTES for _ in range(2)]
        same = all(len(r) == len(runs[0]) and all(np.array_equal(a, b) for a, b in zip(r, runs[0])) for r in runs[1:])
        print('{:28s} {:3d} parameters, {:6d} words: {}'.format(name, len(runs[0]), sum(a.size for a in runs[0]),
                                                                 'repeats bit for bit' if same else 'DIFFERS between its own runs'))
        if not same:
            bad.append(name)
        for k, a in enumerate(runs[0]):
            arrays['{}/{:02d}'.format(name, k)] = a
    if bad:
        sys.exit("not written: {} do not repeat their own bits".format(', '.join(bad)))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print('wrote {} ({} bytes)'.format(out, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else tb.GOLDEN)

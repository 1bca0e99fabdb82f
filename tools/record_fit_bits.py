#!/usr/bin/env python
"""Record tests/golden/fit_bits.npz: what two epochs of fit() leave behind for each case of tests/fit_bits_cases.py, replayed and
under AMAR_TRAIN_GRAPH=0 (parameters as uint32, the history's loss bits, the step count, captures and graph keys).  Run it on the GPU
at the commit whose bits are to be kept (a refactor of fit() records at its parent), twice in separate processes: the second run is
given the first one's file, leaves out every case that does not repeat it and names it.  Each of fit()'s branches must keep a replayed
and an AMAR_TRAIN_GRAPH=0 case, or nothing is written.
usage: python tools/record_fit_bits.py [output.npz [recording of an earlier process.npz]]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fit_bits_cases as fb  # noqa: E402


def main(out, earlier=None):
    before = None
    if earlier is not None:
        with np.load(earlier) as z:
            before = {k: z[k] for k in z.files}
    arrays, kept = {}, set()
    for name in fb.CASES:
        for env in fb.GRAPH_ENVS:
            run = fb.fit_bits(name, env)
            prefix = '{}/{}/'.format(name, env)
            repeats = before is None or fb.same(run, {k[len(prefix):]: a for k, a in before.items() if k.startswith(prefix)})
            print('{:24s} AMAR_TRAIN_GRAPH={} t={:3d} {:6d} words, loss {}: {}'.format(
                name, env, int(run['t'][0]), run['params'].size, run['loss'].view(np.float64),
                'kept' if repeats else 'LEFT OUT: differs from the earlier recording'), flush=True)
            if repeats:
                kept.add((fb.CASES[name][3], env))
                arrays.update((prefix + k, a) for k, a in run.items())
    lost = sorted({(fb.CASES[name][3], env) for name in fb.CASES for env in fb.GRAPH_ENVS} - kept)
    if lost:
        sys.exit("not written: no case left for {}".format(lost))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print('wrote {} ({} bytes)'.format(out, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else fb.GOLDEN, sys.argv[2] if len(sys.argv) > 2 else None)

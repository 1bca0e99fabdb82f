"""GPU: two epochs of fit() give the recorded bits (pytest -m gpu).  tests/golden/fit_bits.npz was written by tools/record_fit_bits.py
before fit()'s three epoch loops became one and the Trainer's two capture-or-replay steps became one; that change moves no launch, so
every trainable parameter, the loss of every epoch, the step count, the number of captures and the graph keys must come out equal, on
each branch of fit(), replayed and under AMAR_TRAIN_GRAPH=0 (the recorder found every run equal to its repetition in another process)."""
import numpy as np
import pytest

from tests import fit_bits_cases as fb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with np.load(fb.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_file_covers_every_branch_of_fit(golden):
    runs = {tuple(k.split('/')[:2]) for k in golden}
    assert runs == {(name, env) for name in fb.CASES for env in fb.GRAPH_ENVS}
    assert {(fb.CASES[name][3], env) for name, env in runs} == {(loop, env) for loop in ('head', 'graph', 'sampled') for env in fb.GRAPH_ENVS}


@pytest.mark.parametrize('env', fb.GRAPH_ENVS)
@pytest.mark.parametrize('name', list(fb.CASES))
def test_fit_repeats_the_recorded_bits(hip, golden, name, env):
    prefix = '{}/{}/'.format(name, env)
    want = {k[len(prefix):]: a for k, a in golden.items() if k.startswith(prefix)}
    got = fb.fit_bits(name, env)
    assert set(got) == set(want)
    for k in sorted(got):
        a, b = got[k], want[k]
        differing = int((a != b).sum()) if a.shape == b.shape else -1
        print(name, env, k, a.size, 'elements,', differing, 'differ', *((a.tolist(), b.tolist()) if k not in ('params', 'loss') else ()))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, env, k, differing)

"""GPU: two training steps of every stack kind give the recorded bits (pytest -m gpu).  tests/golden/train_step_bits.npz was written
by tools/record_train_bits.py before the training tapes were split by layer kind and put on one linear reverse-pass helper; that
split changes no kernel and no launch argument, so every trainable parameter must come out equal as uint32, on the eagerly run body
and on the captured and replayed one (the recorder found the two equal, and each equal to its own repetition)."""
import numpy as np
import pytest

from tests import train_bits_cases as tb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with np.load(tb.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_file_holds_exactly_the_cases(golden):
    assert {k.split('/')[0] for k in golden} == set(tb.CASES)
    assert all(a.dtype == np.uint32 and a.ndim == 1 for a in golden.values())


@pytest.mark.parametrize('route', tb.ROUTES)
@pytest.mark.parametrize('name', list(tb.CASES))
def test_two_training_steps_repeat_the_recorded_bits(hip, golden, name, route):
    got = tb.train_bits(name, route)
    want = [golden['{}/{:02d}'.format(name, k)] for k in range(sum(k.startswith(name + '/') for k in golden))]
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        differing = int((a != b).sum()) if a.shape == b.shape else -1
        print(name, route, 'parameter', k, a.size, 'words,', differing, 'differ')
        assert a.dtype == np.uint32 and a.shape == b.shape and np.array_equal(a, b), (name, route, k, differing)

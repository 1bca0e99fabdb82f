"""GPU: amar_scatter_closed_f32 — the way back of the scores for a window table whose windows are CLOSED (each window's indices
a bijection onto the window's own range): every window finished in LDS and written to dst in whole 16-byte stores.  Pure data
movement, so every comparison is torch.equal against `dst_ref[index.long()] = src`; the destination always sits between two
rows of 64 sentinel floats that must come back untouched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
SENTINEL = -12345.0


def _table(lengths):
    off = [0]
    for l in lengths:
        off.append(off[-1] + l)
    return off


def _closed_index(off, kind, seed):
    """One closed permutation of [0, off[-1]): 'random' shuffles every window inside its own range, 'identity', 'reverse' per window."""
    g = torch.Generator()
    g.manual_seed(seed)
    parts = []
    for lo, hi in zip(off, off[1:]):
        if kind == 'random':
            parts.append(lo + torch.randperm(hi - lo, generator=g))
        elif kind == 'identity':
            parts.append(torch.arange(lo, hi))
        else:
            parts.append(torch.arange(hi - 1, lo - 1, -1))
    return torch.cat(parts).to(torch.int32).to(DEV)


def _run(capi, off, index, src, shift=0):
    """Launch on a destination `shift` floats past a 16-byte boundary, between two sentinel rows; returns (live range, guards ok)."""
    n = off[-1]
    buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, device=DEV)
    lo = GUARD + shift
    dst = buf[lo:lo + n]
    window_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    rc = capi.load().amar_scatter_closed_f32(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                                             n, ctypes.c_void_p(window_off.data_ptr()), len(off) - 1, max(b - a for a, b in zip(off, off[1:])), None)
    torch.cuda.synchronize()
    untouched = bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all())
    return rc, dst.clone(), untouched


CAP = 65536          # include/amar_hip.h: AMAR_SCATTER_CLOSED_MAX_WINDOW (tests/test_scatter_route_cpu.py holds the two together)

SHAPES = {
    'one_of_1': [1],
    'one_of_3': [3],
    'one_of_255': [255],
    'one_of_256': [256],
    'one_of_257': [257],
    'one_of_1023': [1023],                      # around the closed form's own workgroup width
    'one_of_1025': [1025],
    'one_at_half_capacity': [CAP // 2],         # the longest window one workgroup finishes alone
    'one_odd_above_half': [CAP // 2 + 1],       # two workgroups, pieces of CAP / 4 + 1 and CAP / 4 floats
    'one_odd_two_pieces': [40001],              # the two pieces differ by one
    'one_at_capacity': [CAP],
    'unequal_no_multiple_of_4': [1000, 7, 4093, 1],     # later windows start at odd word offsets: head and tail paths
    'nine_of_4096': [4096] * 9,                 # more windows than one per XCD residue, and a remainder
    'seventeen_of_4096': [4096] * 17,
    'last_window_of_1': [4096, 4096, 1],
    'empty_window_inside': [5, 0, 9],
    'two_pieces_short_last': [CAP, 40001, 3],
}


@pytest.mark.parametrize('kind', ['random', 'identity', 'reverse'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_closed_scatter_equals_indexed_assignment(hip, shape, kind):
    from deep_cbrs_amar_renaissance_amd import capi
    off = _table(SHAPES[shape])
    n = off[-1]
    index = _closed_index(off, kind, seed=len(shape) + n)
    g = torch.Generator(device=DEV)
    g.manual_seed(n)
    src = torch.randn(n, device=DEV, generator=g)
    want = torch.empty(n, device=DEV)
    want[index.long()] = src
    for shift in ((0, 1, 2, 3) if n <= 8192 else (0, 3)):            # dst 16-byte aligned and not
        rc, got, untouched = _run(capi, off, index, src, shift)
        assert rc == 0 and untouched, (shape, kind, shift, rc)
        assert torch.equal(got, want), (shape, kind, shift)


def test_closed_scatter_sources_not_aligned_alike(hip):
    """src and index at different offsets from a 16-byte boundary: the window's pairs are read one word at a time, same result."""
    from deep_cbrs_amar_renaissance_amd import capi
    off = _table([1000, 7, 4093, 1])
    n = off[-1]
    index = _closed_index(off, 'random', seed=9)
    src = torch.randn(n + 4, device=DEV)
    ibuf = torch.zeros(n + 4, dtype=torch.int32, device=DEV)
    for s_shift, i_shift in ((1, 0), (0, 2), (3, 3)):
        s, ix = src[s_shift:s_shift + n], ibuf[i_shift:i_shift + n]
        ix.copy_(index)
        want = torch.empty(n, device=DEV)
        want[index.long()] = s
        rc, got, untouched = _run(capi, off, ix, s, shift=1)
        assert rc == 0 and untouched and torch.equal(got, want), (s_shift, i_shift)


def test_closed_scatter_through_capi_and_same_bits_twice(hip, monkeypatch):
    """capi.scatter(closed=True) takes the LDS form and returns what the global form returns; the same launch twice gives the same bits."""
    from deep_cbrs_amar_renaissance_amd import capi
    monkeypatch.delenv('AMAR_PAIR_SCATTER', raising=False)
    off = _table([CAP, 40001, 4096, 3])
    n = off[-1]
    index = _closed_index(off, 'random', seed=4)
    src = torch.randn(n, device=DEV)
    window_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    want = torch.empty(n, device=DEV)
    want[index.long()] = src
    assert capi.scatter_route(n, 1, CAP, True) == 'lds'
    outs = []
    for _ in range(2):
        dst = torch.full((n, 1), float('nan'), device=DEV)
        capi.scatter(src, index, dst, window_off, len(off) - 1, closed=True, max_window=CAP)
        outs.append(dst.view(-1))
    assert torch.equal(outs[0], want) and torch.equal(outs[0], outs[1])
    glob = torch.full((n, 1), float('nan'), device=DEV)
    capi.scatter(src, index, glob, window_off, len(off) - 1)
    assert torch.equal(glob.view(-1), outs[0])
    monkeypatch.setenv('AMAR_PAIR_SCATTER', 'global')
    again = torch.full((n, 1), float('nan'), device=DEV)
    capi.scatter(src, index, again, window_off, len(off) - 1, closed=True, max_window=CAP)
    assert torch.equal(again.view(-1), want)


def test_closed_scatter_arguments(hip):
    """Every AMAR_EINVAL case of the contract; n == 0 returns AMAR_OK and writes nothing."""
    from deep_cbrs_amar_renaissance_amd import capi
    lib = capi.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n = 8
    src = torch.arange(n, dtype=torch.float32, device=DEV)
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    dst = torch.full((n,), SENTINEL, device=DEV)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    f = lib.amar_scatter_closed_f32
    assert f(None, p(idx), p(dst), n, p(off), 1, n, None) == -1
    assert f(p(src), None, p(dst), n, p(off), 1, n, None) == -1
    assert f(p(src), p(idx), None, n, p(off), 1, n, None) == -1
    assert f(p(src), p(idx), p(dst), n, None, 1, n, None) == -1                    # the closed form has no table-free variant
    assert f(p(src), p(idx), p(dst), -1, p(off), 1, n, None) == -1
    assert f(p(src), p(idx), p(dst), 1 << 31, p(off), 1 << 16, CAP, None) == -1    # n >= 2^31
    assert f(p(src), p(idx), p(dst), n, p(off), 0, n, None) == -1                  # no windows
    assert f(p(src), p(idx), p(dst), n, p(off), 1, -1, None) == -1
    assert f(p(src), p(idx), p(dst), n, p(off), 1, CAP + 1, None) == -1            # a window one longer than the capacity
    assert f(p(src), p(idx), p(dst), n, p(off), 1, n - 1, None) == -1              # one window of 7 cannot cover 8 values
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    assert f(p(src), p(idx), p(dst), 0, p(off), 1, 0, None) == 0                   # nothing to do
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    assert f(p(src), p(idx), p(dst), n, p(off), 1, CAP, None) == 0                 # a looser bound on the longest window is fine
    torch.cuda.synchronize()
    assert torch.equal(dst, src)
    with pytest.raises(ValueError):
        capi.scatter(src, idx, dst, torch.zeros(3, dtype=torch.int32, device=DEV), 1, closed=True, max_window=n)

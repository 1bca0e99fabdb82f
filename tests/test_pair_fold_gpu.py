"""The pair-stage kernel's folded last tile (csrc/amar_chain.hip, chain_pipe_kernel with SPLIT and an odd tile count) against float64
(pytest -m gpu).

With three f32 tiles (a 48-wide head) the last tile's six part products ride in three k-steps of two products each instead of a k-step
padded with zeros, and the accumulators start at the bias.  The head of every case is sum-inputs -> Dense W -> Dense 1 -> sigmoid over
tables of 64 users and 48 items (tests/pair_fold_cases.py): W = 48 is the folded kernel; 16, 80 (odd tile counts) and 32 (even) are sent to
the generic kernel by the route, which is asserted, and run the f32 instruction in either process.  P = 1 .. 33 cover the pair-tile tail
and the re-read of the last pair, 129 a second workgroup, 4 x 128 + 5 four workgroups and a ragged fifth; every P plain, with an
out_index, and in the ids form with base_a = 7, base_b = 11.

The bound is not a number fixed in advance: ONE fresh child process scores every case with AMAR_PAIR_MFMA=f32 (the f32 instruction; the
switch is read once per process), and the folded form must stay within twice that form's own max |error| against float64 over the same
width's cases, plus one f32 ulp at 1.0 (2^-23) for the sigmoid: the six-product truncation is 3 . 2^-24 per product, the size of one f32
rounding.  Edge inputs are held to the same bound against their own f32 figure.

Both measured maxima per width are printed; with AMAR_PAIR_FOLD_RECORD=<file> in the environment they are appended to that file as JSON
lines (profiles/exp_pair_fold.jsonl is such a record; the suite itself writes nothing into the tree)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import chain_ref as cr
from tests import pair_fold_cases as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP_AT_ONE = 2.0 ** -23
FOLD_P = 4 * 128 + 5


@pytest.fixture(scope='module')
def f32_scores(hip, tmp_path_factory):
    """name -> scores of the f32-instruction form, from one child process."""
    assert os.environ.get('AMAR_PAIR_MFMA') != 'f32'
    path = str(tmp_path_factory.mktemp('pair_fold') / 'f32_scores.npz')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'pair_fold_cases.py'), path], env=dict(os.environ, AMAR_PAIR_MFMA='f32'),
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return dict(np.load(path))


def _expect_route(case, route):
    """W = 48 runs the pair-stage kernel on split products (three tiles: the fold); the other widths the generic kernel."""
    if case.W == 48:
        assert route['kernel'] == cr.PIPE and route['maxt'] == 3 and route['split'] and bool(route['scatter']) == case.indexed, (case, route)
    else:
        assert route['kernel'] == cr.GENERIC and not route['split'], (case, route)


def _errors(hip, case, f32_scores):
    """(max |this process's form - float64|, max |f32 form - float64|, scores, float64 scores) of one case."""
    launch = pf.Launch(hip, case)
    got, route = launch.run()
    _expect_route(case, route)
    want = case.reference(launch.d)
    f32 = f32_scores[case.name]
    assert got.shape == f32.shape == want.shape == (case.P,) and np.isfinite(got).all() and np.isfinite(f32).all(), case
    return float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(f32.astype(np.float64) - want).max()), got, want


def _record(rec):
    print(json.dumps(rec))
    path = os.environ.get('AMAR_PAIR_FOLD_RECORD')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')


@pytest.mark.parametrize('W', pf.WIDTHS)
def test_folded_form_within_twice_the_f32_forms_error(hip, f32_scores, W):
    """Every P and call form of one width: max error of the folded form <= 2 x max error of the f32 form + 2^-23, both against float64."""
    e_fold = e_f32 = 0.0
    for P in pf.PS:
        for variant in pf.VARIANTS:
            a, b, _, _ = _errors(hip, pf.Case(W, P, variant), f32_scores)
            e_fold, e_f32 = max(e_fold, a), max(e_f32, b)
    _record(dict(what='cases', width=W, max_err_fold=e_fold, max_err_f32=e_f32, bound=2 * e_f32 + ULP_AT_ONE))
    assert e_fold <= 2 * e_f32 + ULP_AT_ONE, (W, e_fold, e_f32)


@pytest.mark.parametrize('edge', pf.EDGES)
@pytest.mark.parametrize('W', pf.WIDTHS)
def test_edge_inputs(hip, f32_scores, W, edge):
    """A weight row alive in the last tile only, an all-zero last tile, activations exactly 0 behind the ReLU, and the bias alone (every
    input negative: the score is sigmoid(dense1(relu(b))), which guards the bias' move out of the k-slot)."""
    case = pf.Case(W, pf.EDGE_P, 'indexed', edge)
    e_fold, e_f32, got, want = _errors(hip, case, f32_scores)
    _record(dict(what=edge, width=W, max_err_fold=e_fold, max_err_f32=e_f32, bound=2 * e_f32 + ULP_AT_ONE))
    assert e_fold <= 2 * e_f32 + ULP_AT_ONE, (case, e_fold, e_f32)
    if edge == 'bias_only':
        d = case.draw()
        y = np.maximum(d['bs'][0].astype(np.float64), 0)
        alone = 1.0 / (1.0 + np.exp(-(y @ d['ks'][1].astype(np.float64)[:, 0] + float(d['bs'][1][0]))))
        assert float(np.abs(want - alone).max()) < 1e-15                     # the reference itself sees x = 0
        assert float(np.abs(got.astype(np.float64) - alone).max()) <= 2 * e_f32 + ULP_AT_ONE, (case, got[:4], alone)
        assert len(set(got.tolist())) == 1                                   # every pair the same bits


@pytest.mark.parametrize('variant', pf.VARIANTS)
def test_two_calls_give_identical_bits(hip, variant):
    launch = pf.Launch(hip, pf.Case(48, FOLD_P, variant))
    first, route = launch.run()
    _expect_route(launch.case, route)
    second, _ = launch.run()
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


def test_plan_ordered_call_equals_direct_call(hip):
    """The list walked in a PairPlan's order, every score sent back through out_index, equals the direct call bit for bit (P = 4 x 128 + 5)."""
    from deep_cbrs_amar_renaissance_amd.models.basic import PairPlan
    launch = pf.Launch(hip, pf.Case(48, FOLD_P, 'plain'))
    direct, route = launch.run()
    _expect_route(launch.case, route)
    plan = PairPlan(launch.ia, launch.ib)
    assert plan.mid_index is None                                            # a short list: the direct store
    out = torch.full((FOLD_P, 1), float('nan'), dtype=torch.float32, device=pf.DEV)
    kw = dict(ids_a=plan.u_ids, base_a=0, B=launch.B, ids_b=plan.i_ids, base_b=0, sum_inputs=True, in_act='relu', out_index=plan.out_index)
    r = hip.chain_route(launch.A, launch.blob, launch.case.dims, pf.ACTS, out, **kw)
    assert r['kernel'] == cr.PIPE and r['split'] and r['scatter'] and r['maxt'] == 3, r
    hip.chain(launch.A, launch.blob, launch.case.dims, pf.ACTS, out, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(out[:, 0].cpu().numpy().view(np.uint32), direct.view(np.uint32))

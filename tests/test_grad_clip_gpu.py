"""GPU: gradient clipping — amar_grad_clip_f32 against the float64 rules and the derived float32 bounds of tests/clip_ref.py, and the
trainers that run it: a clip that cannot bind changes no bit, binding clips follow the oracle's gradients pushed through clip_ref and
optimizer_ref, replayed = eager batches, the head-only and the BPR trainer, one experiment through the public surface (pytest -m gpu).

Kernel level: every buffer a kernel must not touch starts as a sentinel and is compared as bits."""
import glob
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import train as otrain
from tests import clip_ref as cref
from tests import entry_point_ref as ref
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = np.float32(-7.25)
L2 = float(np.float32(1e-2))
CFG = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
MODE_CODES = {'clipvalue': 'CLIP_VALUE', 'clipnorm': 'CLIP_NORM', 'global_clipnorm': 'CLIP_GLOBAL_NORM'}

# (n, layout, g_groups, l2): n on both sides of the 1024-element block and of the 4-element lane, the scalar layout by n % 4 and by a
# 4-byte offset of the pointers, 17 groups = one past the sixteen the vector layout keeps in flight (five past the scalar layout's four),
# g_groups 0 and 1 both mean "g is the gradient"; 'zero' is a slot without gradient
LAYOUT = [(1, 'scalar', 0, 0.0), (3, 'scalar', 1, L2), (1023, 'scalar', 5, L2), (1024, 'vector', 17, 0.0), (1025, 'scalar', 17, L2),
          (4100, 'vector', 5, L2), (4100, 'vector', 0, 0.0), (1024, 'offset', 5, L2), (1024, 'vector', 1, L2), (1028, 'zero', 5, 0.0)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f32(x):
    return float(np.float32(x))


def fmaf32(a, b, c):
    """fmaf on float32 arrays, exactly: the product is exact in float64, TwoSum gives the rounding error of the float64 sum, and where
    that sum sits on the midpoint of two float32 values the error's sign decides (what a single rounding of the exact value does)."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    other = np.where(d > 0, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))).astype(np.float32)
    tie = (d != 0) & (s == (r.astype(np.float64) + other.astype(np.float64)) / 2)
    return np.where(tie & (err != 0) & (np.sign(err) == np.sign(d)), other, r).astype(np.float32)


def _layout():
    """(host buffer, slots): every array of every slot cut from one sentinel-filled buffer with guard floats between them."""
    rng = np.random.default_rng(21)
    GAP = 8                                                           # floats (a multiple of 4: alignment survives)
    total = sum((max(g, 1) + 1) * (n + 4 + GAP) + GAP for n, _, g, _ in LAYOUT) + 64
    host = np.full(total, SENTINEL, dtype=np.float32)
    pos, slots = GAP, []

    def take(count, offset_one):
        nonlocal pos
        start = pos + (1 if offset_one else 0)
        pos = (start + count + GAP + 3) // 4 * 4
        return slice(start, start + count)
    for n, kind, groups, l2 in LAYOUT:
        w = rng.standard_normal(n).astype(np.float32)
        parts = rng.standard_normal((max(groups, 1), n)).astype(np.float32)
        if kind == 'zero':
            parts[:] = 0
        s = {'n': n, 'kind': kind, 'groups': groups, 'l2': l2, 'w': take(n, kind == 'offset'), 'g': take(max(groups, 1) * n, kind == 'offset')}
        host[s['w']], host[s['g']] = w, parts.reshape(-1)
        s['ref'] = (w.astype(np.float64), parts.astype(np.float64), l2)
        slots.append(s)
    assert pos <= total
    return host, slots


def _run(hip, host, slots, mode, clip, with_loss=True):
    """One amar_grad_clip_f32 call on a fresh device copy of `host`: (buffer after, norms or None, loss_acc or None)."""
    buf = _t(host)
    entries = []
    for s in slots:
        g = buf[s['g']]
        entries.append((buf[s['w']], hip.DeferredGradient(g, s['groups'], (s['n'],)) if s['groups'] else g, s['l2']))
        vector = s['n'] % 4 == 0 and entries[-1][0].data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
        assert vector == (s['kind'] in ('vector', 'zero')), (s['n'], s['kind'])
    table, blocks = hip.clip_slot_table(entries)
    assert blocks == sum((s['n'] + 1023) // 1024 for s in slots)
    ws = torch.full((hip.grad_clip_workspace_floats(len(slots), blocks),), float(SENTINEL), device=DEV)
    norms = None if mode == 'clipvalue' else torch.full((len(slots) if mode == 'clipnorm' else 1,), float(SENTINEL), device=DEV)
    loss = torch.full((1,), 2.5, device=DEV) if with_loss else None
    hip.grad_clip(getattr(hip, MODE_CODES[mode]), clip, table.to(DEV), len(slots), blocks, ws, norms=norms, reg_scale=0.5, loss_acc=loss)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), None if norms is None else norms.cpu().numpy(), None if loss is None else float(loss[0])


def _binding_clip(mode, slots):
    """A clip taken from the reference's numbers: the median per-slot norm (some slots bind, some do not), half the global norm, or a
    value that cuts into the normal-distributed gradients; rounded to float32, what the kernel receives."""
    refs = [s['ref'] for s in slots]
    if mode == 'clipnorm':
        return _f32(np.median(cref.norms(mode, refs)))
    return _f32(0.5 * cref.norms(mode, refs)[0]) if mode == 'global_clipnorm' else 0.5


@pytest.mark.parametrize('mode', cref.MODES)
def test_kernels_follow_the_float64_rule_within_the_derived_bounds(hip, mode):
    """Group 0 of every slot against clip_ref.clip, per element within clip_ref.bounds (derived in that file from the roundings of the
    computation: max(G, 1) u on the magnitudes of the gradient's terms, and for the norms the n u of an n-term float32 sum carried into
    the scale); the measured norms within the bound derived there too (||e_g|| + norm (n u / 2 + u)), not the 1e-6 sqrt(n) alternative;
    guards, groups >= 1 and w keep their bits; two runs give equal bits; loss_acc against float64 at test_optimizers_gpu.py's 1e-5."""
    host, slots = _layout()
    refs = [s['ref'] for s in slots]
    clip = _binding_clip(mode, slots)
    after, norms, loss = _run(hip, host, slots, mode, clip)
    again, norms_again, loss_again = _run(hip, host, slots, mode, clip)
    assert np.array_equal(after.view(np.int32), again.view(np.int32))
    assert norms is None or np.array_equal(norms.view(np.int32), norms_again.view(np.int32))
    without, _, _ = _run(hip, host, slots, mode, clip, with_loss=False)
    assert np.array_equal(after.view(np.int32), without.view(np.int32))                           # loss_acc = NULL changes nothing else
    written = np.zeros(host.size, dtype=bool)
    for s in slots:
        written[s['g'].start:s['g'].start + s['n']] = True
    assert np.array_equal(after[~written].view(np.int32), host[~written].view(np.int32))          # guards, groups >= 1, w
    want, want_norms = cref.clip(mode, clip, refs)
    bound, norm_bound = cref.bounds(mode, clip, refs)
    worst, changed = 0.0, 0
    for s, a, b in zip(slots, want, bound):
        got = after[s['g'].start:s['g'].start + s['n']].astype(np.float64)
        assert np.isfinite(got).all()
        err = np.abs(got - a)
        live = b > 0
        assert np.array_equal(got[~live], a[~live]), (s['n'], s['kind'], s['groups'])
        if live.any():
            worst = max(worst, float((err[live] / b[live]).max()))
        assert np.all(err <= b), (s['n'], s['kind'], s['groups'], float((err[live] / b[live]).max()))
        if s['kind'] == 'zero':
            assert not got.any()                                       # a zero gradient stays zero (norm 0: scale 1)
        changed += int(not np.allclose(a, cref.finished(*s['ref']), rtol=1e-3, atol=0))
    print('{}: clip {:.6g}, max |got - float64| / bound = {:.3f}, {} of {} slots clipped'.format(mode, clip, worst, changed, len(slots)))
    assert changed >= 3                                               # (the clip binds, by the reference's numbers)
    if mode != 'clipvalue':
        err = np.abs(norms.astype(np.float64) - want_norms)
        print('norms: max |got - float64| / bound = {:.3f}'.format(float((err[norm_bound > 0] / norm_bound[norm_bound > 0]).max())))
        assert np.all(err <= norm_bound)
        assert mode != 'clipnorm' or (changed < len(slots) - 1 and norms[-1] == 0)                # some slots do not bind; the zero slot
    reg64 = sum(s['l2'] * float(np.sum(s['ref'][0] ** 2)) for s in slots)
    want_loss = 2.5 + 0.5 * reg64
    print('loss_acc {:.9g}, float64 {:.9g}'.format(loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * want_loss and abs(loss_again - want_loss) <= 1e-5 * want_loss


@pytest.mark.parametrize('mode', cref.MODES)
def test_a_clip_that_cannot_bind_leaves_the_finished_gradient_bit_for_bit(hip, mode):
    """clip = 1e30: group 0 == fmaf(2 l2, w, the partials added in the order 0 .. G-1 in float32), as bits.  The additions are torch's
    on the device, one after the other in float32; the fused multiply-add is fmaf32 above (torch has none that is promised fused)."""
    host, slots = _layout()
    after, norms, _ = _run(hip, host, slots, mode, 1e30)
    for s in slots:
        parts = _t(host[s['g']]).view(max(s['groups'], 1), s['n'])
        total = parts[0].clone()
        for k in range(1, parts.shape[0]):
            total = total + parts[k]
        total = total.cpu().numpy()
        assert np.array_equal(total, ref.sum_groups_f32(host[s['g']].reshape(-1, s['n'])))
        want = fmaf32(np.float32(2.0) * np.float32(s['l2']), host[s['w']], total)
        got = after[s['g'].start:s['g'].start + s['n']]
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (s['n'], s['kind'], s['groups'])
    if norms is not None:
        assert np.isfinite(norms).all() and norms.max() > 1


def test_argument_checks(hip):
    x, g = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    table, blocks = hip.clip_slot_table([(x, g, 0.0)])
    table = table.to(DEV)
    ws = torch.zeros(hip.grad_clip_workspace_floats(1, blocks), device=DEV)
    for mode, clip, tab, n_slots, total, work in ((0, 1.0, table, 1, 1, ws), (4, 1.0, table, 1, 1, ws), (hip.CLIP_NORM, 0.0, table, 1, 1, ws),
                                                  (hip.CLIP_VALUE, -1.0, table, 1, 1, ws), (hip.CLIP_NORM, float('nan'), table, 1, 1, ws),
                                                  (hip.CLIP_NORM, 1.0, None, 1, 1, ws), (hip.CLIP_NORM, 1.0, table, 0, 1, ws),
                                                  (hip.CLIP_NORM, 1.0, table, 1, 0, ws), (hip.CLIP_NORM, 1.0, table, 1, 2 ** 31, None),
                                                  (hip.CLIP_GLOBAL_NORM, 1.0, table, 1, 1, None)):
        with pytest.raises(ValueError):
            hip.grad_clip(mode, clip, tab, n_slots, total, work)
    with pytest.raises(ValueError):
        hip.grad_clip(hip.CLIP_NORM, 1.0, table, 1, 1, ws[:1])                                     # a workspace too small
    with pytest.raises(ValueError):
        hip.clip_slot_table([(x, torch.zeros(9, device=DEV), 0.0)])
    with pytest.raises(ValueError):
        hip.grad_clip_workspace_floats(0, 1)
    torch.cuda.synchronize()
    assert float(g.sum()) == 8                                         # nothing ran
    hip.grad_clip(hip.CLIP_VALUE, 0.5, table, 1, blocks)               # clipvalue needs no workspace
    assert float(g.sum()) == 4


# ---- trainer level ----------------------------------------------------------------------------------------------------------------------

def _gcn_pair(count=1):
    from deep_cbrs_amar_renaissance_amd import engine
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=3)
    models = []
    for _ in range(count):
        engine.set_seed(8)
        m = basic.BasicGCN(g['adj'], **CFG)
        helpers.randomize_biases(m, seed=1)
        models.append(m)
    return g, models


_ORACLE_START = {}


def _oracle_params(gnn, head, og):
    """{key: (w, finished float64 gradient)} over every parameter of the oracle's model, keyed as test_optimizers_gpu.py keys them."""
    params = {'emb': (gnn['embeddings'], og['gnn']['embeddings'])}
    for k, lw in enumerate(gnn['layers']):
        for nm in ('kernel', 'bias'):
            params[('l', k, nm)] = (lw[nm], og['gnn']['layers'][k][nm])
    for name in head:
        for k, (w, b) in enumerate(head[name]):
            params[(name, k, 'w')] = (w, og['head'][name][k][0])
            params[(name, k, 'b')] = (b, og['head'][name][k][1])
    return params


WATCHED = ('emb', ('l', 0, 'kernel'), ('clf', 2, 'w'))


def _oracle_start():
    """The 80-user / 60-item GCN of test_optimizers_gpu.py in float64, the oracle's gradient at its initial weights (the L2 part is in
    it) and what clip_ref measures on it: computed once; the learning rate and the clips below are taken from it, never from the code
    under test."""
    if not _ORACLE_START:
        g, (model,) = _gcn_pair()
        y = np.random.default_rng(4).integers(0, 2, len(g['u_ids']))
        gnn, head = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
        gnn = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in gnn.items()}
        gnn['layers'] = [{k: v.astype(np.float64) for k, v in lw.items()} for lw in gnn['layers']]
        head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in net] for k, net in head.items()}
        _, og, _ = otrain.loss_and_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, l2=1e-4)
        params = _oracle_params(gnn, head, og)
        assert all(k in params for k in WATCHED) and ('clf', 3, 'w') not in params
        slot = {k: [(np.zeros(gr.size), gr.reshape(1, -1), 0.0)] for k, (_, gr) in params.items()}
        watched = [s for k in WATCHED for s in slot[k]]
        measured = {'clipnorm': min(float(cref.norms('clipnorm', s)[0]) for s in (slot[k] for k in WATCHED)),
                    'global_clipnorm': float(cref.norms('global_clipnorm', [s[0] for s in slot.values()])[0]),
                    'clipvalue': cref.max_abs(watched)}
        _ORACLE_START.update(g=g, y=y, gnn=gnn, head=head, gmax=cref.max_abs(watched), measured=measured)
    return _ORACLE_START


RULES = {'adam': ('Adam', {}), 'sgd-momentum': ('SGD', dict(momentum=0.9)), 'rmsprop': ('RMSprop', {})}


def _state_arrays(trainer):
    return [a for prm in trainer.params for a in trainer.opt_arrays[prm]]


@pytest.mark.parametrize('case', list(RULES))
def test_a_clip_that_cannot_bind_trains_bit_for_bit_as_no_clip(hip, case):
    """Three train_batch_graphed steps (one eager, the capture, one replay) with global_clipnorm = 1e30 against three without a clip:
    the clip pass finishes the same gradients in the same order, its scale is 1.0f exactly, and the update on (g_groups = 0, l2 = 0)
    applies them unchanged — every weight and every state array equal as bits."""
    from deep_cbrs_amar_renaissance_amd import training
    g, models = _gcn_pair(2)
    y = np.random.default_rng(4).integers(0, 2, len(g['u_ids']))
    rule, hyper = RULES[case]
    plain = training.Trainer(models[0], rule=rule, **hyper)
    clipped = training.Trainer(models[1], rule=rule, global_clipnorm=1e30, **hyper)
    assert plain.spec.clip is None and clipped.spec.clip == ('global_clipnorm', 1e30)
    before = [p.detach().clone() for p in models[0].parameters()]
    for _ in range(3):
        plain.train_batch_graphed(g['u_ids'], g['i_ids'], y)
        clipped.train_batch_graphed(g['u_ids'], g['i_ids'], y)
    assert plain._graphs and clipped._graphs and plain.t == clipped.t == 3
    assert 'clip_ws' in clipped._g and 'clip_ws' not in plain._g
    for pa, pb, p0 in zip(models[0].parameters(), models[1].parameters(), before):
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), tuple(pa.shape)
        assert not torch.equal(pa, p0)
    arrays = list(zip(_state_arrays(plain), _state_arrays(clipped)))
    assert len(arrays) == plain.spec.n_arrays * len(plain.params) > 0
    for a, b in arrays:
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert abs(plain.pop_loss_sum() - clipped.pop_loss_sum()) <= 1e-6 * len(y) * 3                # (the L2 loss reaches the sum once)


@pytest.mark.parametrize('mode', cref.MODES)
def test_clipped_sgd_steps_match_the_oracle_through_the_float64_rules(hip, mode):
    """Three train_batch steps of SGD under a clip that binds by the reference's own numbers — half of what clip_ref measures on the
    oracle's gradient at the initial weights: the smallest norm of the watched tensors (clipnorm), the global norm, the largest
    magnitude on the watched tensors (clipvalue) — against the oracle's float64 gradients pushed through clip_ref and optimizer_ref.
    The bound is test_training_steps_match_the_oracle_through_the_float64_rule's: 2e-5 x (the largest single step of the float64
    reference on the watched weights / 1e-3).  The clipped reference must differ from the unclipped one by more than 10 x that bound:
    else the test could not see the clip."""
    from deep_cbrs_amar_renaissance_amd import training
    start = _oracle_start()
    g, y = start['g'], start['y']
    _, (model,) = _gcn_pair()
    lr = 1e-3 / start['gmax']                                        # SGD moves by lr g: about 1e-3 on the largest reference gradient
    c = _f32(0.5 * start['measured'][mode])
    trainer = training.Trainer(model, rule='SGD', learning_rate=lr, **{mode: c})
    assert trainer.spec.clip == (mode, c)
    weights = {}
    for clip in ((mode, c), None):
        gnn = dict(start['gnn'], layers=[dict(lw) for lw in start['gnn']['layers']])
        head = {k: list(net) for k, net in start['head'].items()}
        opt = cref.Optimizer('SGD', clip=clip, learning_rate=lr)
        largest = 0.0
        for t in range(1, 4):
            _, og, _ = otrain.loss_and_grads(g['adj'], gnn, head, g['u_ids'], g['i_ids'], y, l2=1e-4)   # (the L2 gradient is in og)
            opt.advance()
            params = _oracle_params(gnn, head, og)
            new = opt.update_all(params)
            largest = max(largest, max(float(np.abs(new[k] - params[k][0]).max()) for k in WATCHED))
            gnn['embeddings'] = new['emb']
            for k, lw in enumerate(gnn['layers']):
                for nm in ('kernel', 'bias'):
                    lw[nm] = new[('l', k, nm)]
            for name in head:
                head[name] = [(new[(name, k, 'w')], new[(name, k, 'b')]) for k in range(len(head[name]))]
        weights[clip is not None] = ([gnn['embeddings'], gnn['layers'][0]['kernel'], head['clf'][-1][0]], largest)
    for t in range(3):
        trainer.train_batch(g['u_ids'], g['i_ids'], y)
    want, largest = weights[True]
    bound = 2e-5 * largest / 1e-3
    seen = max(float(np.abs(a - b).max()) for a, b in zip(want, weights[False][0]))
    got, gh = helpers.gnn_to_oracle(model.gnn), helpers.basic_head_to_oracle(model.rs)
    errs = [float(np.abs(a - b).max()) for a, b in zip([got['embeddings'], got['layers'][0]['kernel'], gh['clf'][-1][0]], want)]
    print('{}: c {:.4g}, lr {:.3g}, largest reference step {:.3g}, bound {:.3g}, clipped - unclipped reference {:.3g}, errors {}'.format(
        mode, c, lr, largest, bound, seen, ['{:.2e}'.format(e) for e in errs]))
    assert seen > 10 * bound
    assert trainer.t == 3 and float(trainer._opt_state[0]) == 3
    assert max(errs) < bound


def test_replayed_batches_equal_eager_batches_under_a_binding_clipnorm(hip):
    """test_replayed_batches_equal_eager_batches with Adam and clipnorm = half the smallest watched norm of the oracle's start (the
    scales the replayed trainer last wrote show that it binds): train_batch_graphed == train_batch at that test's tolerances."""
    from deep_cbrs_amar_renaissance_amd import training
    c = _f32(0.5 * _oracle_start()['measured']['clipnorm'])
    g, models = _gcn_pair(2)
    rng = np.random.default_rng(4)
    batches = [(g['u_ids'][k * 64:(k + 1) * 64], g['i_ids'][k * 64:(k + 1) * 64], rng.integers(0, 2, 64)) for k in range(4)]
    eager, graphed = (training.Trainer(m, rule='Adam', clipnorm=c) for m in models)
    loss_eager = 0.0
    for epoch in range(3):
        for u, i, y in batches:
            loss_eager += eager.train_batch(u, i, y) * len(y)
            graphed.train_batch_graphed(u, i, y)
    assert graphed._graphs and graphed.t == eager.t == 12
    assert abs(graphed.pop_loss_sum() - loss_eager) < 1e-3 * abs(loss_eager)
    for ws in (graphed._g['clip_ws'], eager._eager_clip['ws']):
        scales = ws[-len(graphed.params):].cpu().numpy()
        assert np.all(scales <= 1) and np.all(scales > 0) and (scales < 1).sum() >= 3, scales
    before = _gcn_pair()[1][0]
    for pa, pb, p0 in zip(models[0].parameters(), models[1].parameters(), before.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-4, atol=1e-6), tuple(pa.shape)
        assert not torch.equal(pa, p0)


def _remeasured_global_norm(hip, trainer):
    """The global norm of the group-0 buffers the trainer's last batch left (the gradients its update applied), measured by the
    entry point itself with a clip that cannot bind (so it changes nothing)."""
    entries = [(e[0], e[1], 0.0) for e in trainer._g['keep']]
    assert all(isinstance(e[1], torch.Tensor) and e[1].numel() == e[0].numel() for e in entries)
    table, blocks = hip.clip_slot_table(entries)
    ws = torch.zeros(hip.grad_clip_workspace_floats(len(entries), blocks), device=DEV)
    norms = torch.zeros(1, device=DEV)
    hip.grad_clip(hip.CLIP_GLOBAL_NORM, 1e30, table.to(DEV), len(entries), blocks, ws, norms=norms)
    return float(norms[0])


C_SMALL = _f32(1e-4)                                                  # far below any gradient norm of these models: it binds


def _check_clipped_to(hip, trainer):
    norm = _remeasured_global_norm(hip, trainer)
    print('re-measured global norm {:.9g}, clip {:.9g}'.format(norm, C_SMALL))
    assert norm <= C_SMALL * (1 + 1e-5)
    assert norm >= C_SMALL * (1 - 1e-4)                               # (at the clip, not below it: the clip did bind)


def test_head_trainer_clips(hip):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    rng = np.random.default_rng(6)
    table = rng.standard_normal((90, 32)).astype(np.float32) * 0.5
    batches = [(rng.integers(0, 50, 64), rng.integers(50, 90, 64), rng.integers(0, 2, 64)) for _ in range(3)]
    engine.set_seed(4)
    model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
    model((table[batches[0][0]], table[batches[0][1]]))              # builds the weights
    helpers.randomize_biases(model, seed=8)
    before = [p.detach().clone() for p in model.parameters()]
    tr = training.HeadTrainer(model, rule='SGD', learning_rate=1.0, global_clipnorm=C_SMALL)
    tr.set_tables([table])
    for u, i, y in batches:
        tr.train_batch_graphed(u, i, y)
    assert tr._graphs and tr.t == 3 and 'graph' in tr._g
    _check_clipped_to(hip, tr)
    moved = np.sqrt(sum(float(((a.detach() - b) ** 2).sum()) for a, b in zip(model.parameters(), before)))
    assert 0 < moved <= 3 * C_SMALL * 1.01                           # three SGD steps of lr 1, each of norm <= c; 1 %: the weights' storage


def test_bpr_trainer_clips(hip):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPRLoss
    from tests.test_bpr_gpu import _sample_sequence
    seq = _sample_sequence()
    engine.set_seed(8)
    model = basic.BasicGCN(seq.adj_matrix, **CFG)
    helpers.randomize_biases(model, seed=1)
    model.compile(loss=BPRLoss())
    model(seq[0][0])
    tr = training.Trainer(model, rule='Adam', global_clipnorm=C_SMALL)
    sampler = tr.sampler_for(seq)
    tr.train_sampled(sampler, graph=True)                            # the body run eagerly
    _check_clipped_to(hip, tr)
    tr.train_sampled(sampler, graph=True)                            # captured and replayed
    tr.train_sampled(sampler, graph=True)
    assert tr._graphs and tr.t == 3 and 'graph' in tr._g
    _check_clipped_to(hip, tr)
    assert np.isfinite(tr.pop_loss_sum())


def test_experiment_runs_with_a_clipped_sgd(hip, tmp_path, monkeypatch):
    """test_experiment_runs_with_sgd with `optimizer: {name: SGD, ..., clipnorm: 1.0}`: the key reaches the device (the batches call the clip
    entry point in per-tensor mode with that value) and the run ends with finite metrics."""
    from deep_cbrs_amar_renaissance_amd import capi, experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    calls = []
    inner = capi.grad_clip

    def counted(mode, clip, *args, **kwargs):
        calls.append((mode, clip))
        return inner(mode, clip, *args, **kwargs)
    monkeypatch.setattr(capi, 'grad_clip', counted)
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update({k: v for k, v in paths.items() if k != 'props_triples_filepath'})
    cfg['dataset'].update({'load_function_name': 'load_user_item_graph', 'graph_filepath': 'unused.json', 'bert_user_filepath': 'unused.json',
                           'bert_item_filepath': 'unused.json'})
    cfg['model'].update({'name': 'basic.BasicGCN', 'embedding_dim': 8, 'n_hiddens': [8, 8], 'dense_units': [24, 24], 'clf_units': [48, 48]})
    cfg['parameters']['optimizer'] = {'name': 'SGD', 'learning_rate': 0.05, 'momentum': 0.9, 'clipnorm': 1.0}
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / 'exps.yaml').write_text(yaml.safe_dump({'linear': {'clipped': None}}))
    monkeypatch.chdir(tmp_path)
    run_log = setup_mlflow('clip test', str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / 'config.yaml'), str(tmp_path / 'exps.yaml'), run_log)
    results = multi.run()
    assert list(results) == ['clipped'] and results['clipped'] is not None
    assert calls and set(calls) == {(capi.CLIP_NORM, 1.0)}
    logs = glob.glob(str(tmp_path / 'mlruns' / '*' / '*' / 'run.jsonl'))
    assert len(logs) == 1
    metrics = {}
    for line in open(logs[0]):
        record = json.loads(line)
        if record['event'] == 'metrics':
            metrics.update(record['metrics'])
    assert np.isfinite(metrics['test_loss']) and metrics['test_loss'] > 0.0 and 0.0 <= metrics['test_accuracy'] <= 1.0
    assert metrics['training_time'] > 0

"""The optimizer runs whose results tests/golden/optimizer_bits.npz pins bit for bit: the cases, their seeded inputs and the runs that
tools/record_optimizer_bits.py records and tests/test_optimizer_bits_gpu.py repeats.

  multi/<case>/...    amar_optim_multi_f32 of each of the eleven rule and flag combinations, after seven advances, on SLOTS: vector and
                      scalar path (by n % 4 and by a w that starts 4 bytes off), n on both sides of a block of 1024, n = 1 and 3,
                      0 / 1 / 5 / 16 / 17 / 33 deferred groups, l2 zero and not (with loss_acc given).  Adam on slots of this kind is
                      pinned by tests/golden/adam_multi_bits.npz.
  advance/<form>/...  the state (and lr_state) after steps 1, 2, 7 and 1000 of the four advance entry points, per rule, the _lr forms
                      under the constant schedule and under ExponentialDecay.
  train/<model>/<rule>/<loop>/...   weights, state arrays and the state block of a BasicRS HeadTrainer and a BasicGCN Trainer (37 nodes)
                      after six batches of 32 under Adam and Nadam, on LOOPS.

What the file holds, per run (`pack`): `small`, the arrays of at most 64 words (every state block among them) one after the other as
uint32, in the order of their sorted names; `digests`, one row of 32 bytes per longer array, its SHA-256, in the same order.  The
arrays of the multi runs alone are 3 MB and do not compress, and the file has to stay far below that; a digest pins every bit of an
array as the array itself would, it only does not say which element moved (the test prints which array did)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optimizer_bits.npz')
DEV = 'cuda'
ADVANCE_STEPS = (1, 2, 7, 1000)
B1, B2, EPS, LR = 0.9, 0.999, 1e-7, 2e-3

# (n, vector path? / 'offset' = w starts one float off, g_groups, l2)
SLOTS = [(1, False, 0, 0.0), (3, False, 0, 1e-3), (1020, True, 0, 1e-3), (1024, True, 0, 0.0), (1028, True, 0, 1e-3), (2049, False, 0, 1e-3),
         (2048, 'offset', 0, 1e-3), (1023, False, 0, 0.0)]
for _groups in (1, 5, 16, 17, 33):
    SLOTS += [(1028, True, _groups, 1e-3 if _groups % 2 else 0.0), (1027, False, _groups, 0.0 if _groups % 2 else 1e-3)]

ADVANCE_RULES = ['SGD', 'RMSprop', 'Adagrad', 'Adamax', 'Nadam', 'AMSGrad']
LOOPS = ('captured', 'uncaptured', 'schedule', 'train_batch', 'rate_set')       # 'rate_set': Adam alone


def pin(a):
    """An array as its words (uint32)."""
    a = np.ascontiguousarray(a).reshape(-1)
    assert a.dtype.itemsize == 4
    return a.view(np.uint32).copy()


def pack(prefix, arrays):
    """What the golden file holds of the arrays of one run (see above) -> ({member name: array}, names of the small, names of the long)."""
    names = sorted(arrays)
    small, long = [k for k in names if arrays[k].size <= 64], [k for k in names if arrays[k].size > 64]
    digests = [np.frombuffer(hashlib.sha256(arrays[k].tobytes()).digest(), dtype=np.uint8) for k in long]
    members = {prefix + 'small': np.concatenate([arrays[k] for k in small] + [np.zeros(0, dtype=np.uint32)]),
               prefix + 'digests': np.stack(digests) if digests else np.zeros((0, 32), dtype=np.uint8)}
    return members, small, long


def moved(prefix, arrays, golden):
    """The names of the arrays of a run that differ from the recorded ones ('*' in front: the set of arrays itself differs)."""
    members, small, long = pack(prefix, arrays)
    want_small, want_digests = golden[prefix + 'small'], golden[prefix + 'digests']
    if members[prefix + 'small'].shape != want_small.shape or members[prefix + 'digests'].shape != want_digests.shape:
        return ['*' + prefix]
    out = [k for k, a, b in zip(long, members[prefix + 'digests'], want_digests) if not np.array_equal(a, b)]
    pos = 0
    for k in small:
        if not np.array_equal(arrays[k], want_small[pos:pos + arrays[k].size]):
            out.append(k)
        pos += arrays[k].size
    return out


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _specs():
    """id -> OptimizerSpec of the eleven rule and flag combinations (tests/test_optimizers_gpu.py: CASES)."""
    from deep_cbrs_amar_renaissance_amd import training
    from tests.test_optimizers_gpu import CASES
    return {case: training.OptimizerSpec(rule=rule, **hyper) for case, (rule, hyper) in CASES.items()}


def slot_buffer(rng, n_arrays):
    """ONE buffer with every slot of SLOTS cut from it -> (host float32 buffer, [{n, kind, groups, l2, w, s: [slices], g}]).  Weights and
    gradients N(0, 1), moments 0.1 N(0, 1) in the first array, accumulators in (0.05, 1) in the others."""
    GAP = 8
    total = sum(4 * (n + 4 + GAP) + max(g, 1) * (n + 4) + GAP for n, _, g, _ in SLOTS) + 64
    host = np.full(total, -7.25, dtype=np.float32)
    pos, slots = GAP, []

    def take(count, offset_one):
        nonlocal pos
        start = pos + (1 if offset_one else 0)
        pos = (start + count + GAP + 3) // 4 * 4
        return slice(start, start + count)
    for n, kind, groups, l2 in SLOTS:
        s = {'n': n, 'kind': kind, 'groups': groups, 'l2': l2, 'w': take(n, kind == 'offset'), 's': [take(n, False) for _ in range(n_arrays)],
             'g': take(max(groups, 1) * n, False)}
        host[s['w']] = rng.standard_normal(n)
        host[s['g']] = rng.standard_normal(max(groups, 1) * n)
        for k, sl in enumerate(s['s']):
            host[sl] = rng.standard_normal(n) * 0.1 if k == 0 else rng.uniform(0.05, 1, n)
        slots.append(s)
    assert pos <= total
    return host, slots


def optim_entries(hip, buf, slots):
    """The entries of capi.optim_slot_table over the device buffer; asserts that every slot takes the path it was laid out for."""
    entries = []
    for s in slots:
        g = buf[s['g']]
        entries.append((buf[s['w']], hip.DeferredGradient(g, s['groups'], (s['n'],)) if s['groups'] else g, [buf[k] for k in s['s']], s['l2']))
        used = [entries[-1][0], g] + entries[-1][2]
        assert (s['n'] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in used)) == (s['kind'] is True), (s['n'], s['kind'])
    return entries


def multi_bits(hip, case, spec):
    import torch
    host, slots = slot_buffer(np.random.default_rng(31), spec.n_arrays)
    state = torch.zeros(hip.OPTIM_STATE_FLOATS, device=DEV)
    for _ in range(7):
        hip.optim_advance(state, spec.code, spec.flags, spec.hyper)
    buf = _t(host)
    table, blocks = hip.optim_slot_table(optim_entries(hip, buf, slots))
    loss = torch.full((1,), 2.5, device=DEV)
    hip.optim_multi(spec.code, spec.flags, spec.hyper, table.to(DEV), len(slots), blocks, state, reg_scale=0.5, loss_acc=loss)
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    out = {'multi/{}/state'.format(case): pin(state.cpu().numpy())}
    for k, s in enumerate(slots):
        for name, sl in zip(['w', 's0', 's1', 's2'], [s['w']] + s['s']):
            out['multi/{}/{:02d}/{}'.format(case, k, name)] = pin(after[sl])
    written = np.zeros(host.size, dtype=bool)
    for s in slots:
        for sl in [s['w']] + s['s']:
            written[sl] = True
    assert np.array_equal(after[~written].view(np.uint32), host[~written].view(np.uint32))       # gaps and gradients keep their bytes
    return out


def _advance_runs(hip):
    """name -> (state size, one-step function of (state, lr_state)) for the four entry points."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    scheds = {'constant': hip.lr_schedule(None), 'exponential': hip.lr_schedule(S.ExponentialDecay(LR, 3, 0.9))}
    runs = {'adam_advance': (2, lambda st, ls: hip.adam_advance(st, LR, B1, B2))}
    for name, sc in scheds.items():
        runs['adam_advance_lr/' + name] = (2, lambda st, ls, sc=sc: hip.adam_advance_lr(st, sc, ls, B1, B2))
    for rule in ADVANCE_RULES:
        spec = training.OptimizerSpec(rule=rule, learning_rate=LR)
        runs['optim_advance/' + rule] = (hip.OPTIM_STATE_FLOATS, lambda st, ls, sp=spec: hip.optim_advance(st, sp.code, sp.flags, sp.hyper))
        for name, sc in scheds.items():
            runs['optim_advance_lr/{}/{}'.format(rule, name)] = (
                hip.OPTIM_STATE_FLOATS, lambda st, ls, sp=spec, sc=sc: hip.optim_advance_lr(st, sp.code, sp.flags, sp.hyper, sc, ls))
    return runs


def advance_bits(hip):
    import torch
    out = {}
    for name, (size, step) in _advance_runs(hip).items():
        state, lr_state = torch.zeros(size, device=DEV), torch.tensor([LR, -1.0], device=DEV)
        kept = {}
        for t in range(1, max(ADVANCE_STEPS) + 1):
            step(state, lr_state)
            if t in ADVANCE_STEPS:
                kept[t] = torch.cat([state, lr_state]).clone()
        for t, both in kept.items():
            out['advance/{}/{}'.format(name, t)] = pin(both.cpu().numpy())
    return out


def state_block(trainer):
    """The device state of the trainer's rule: Adam's two floats (t, step size), the eight of another rule."""
    return trainer._opt_state[:2] if trainer.spec.adam else trainer._opt_state


def _head_trainer(rule, learning_rate):
    from deep_cbrs_amar_renaissance_amd import engine, training
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    rng = np.random.default_rng(6)
    table = rng.standard_normal((90, 32)).astype(np.float32) * 0.5
    batches = [(rng.integers(0, 50, 32), rng.integers(50, 90, 32), rng.integers(0, 2, 32)) for _ in range(6)]
    engine.set_seed(4)
    model = basic.BasicRS(dense_units=[24, 16], clf_units=[16])
    model((table[batches[0][0]], table[batches[0][1]]))
    helpers.randomize_biases(model, seed=8)
    trainer = training.HeadTrainer(model, rule=rule, learning_rate=learning_rate)
    trainer.set_tables([table])
    return trainer, batches


def _gcn_trainer(rule, learning_rate):
    from deep_cbrs_amar_renaissance_amd import training
    from tests import train_bits_cases as tb
    model, _ = tb.build_model('gcn_concatenation_on')
    rng = np.random.default_rng(9)
    pairs = rng.integers(0, tb.N_USERS * tb.N_ITEMS, size=6 * 32)
    u, i, y = pairs // tb.N_ITEMS, pairs % tb.N_ITEMS + tb.N_USERS, rng.integers(0, 2, 6 * 32)
    batches = [(u[k * 32:(k + 1) * 32], i[k * 32:(k + 1) * 32], y[k * 32:(k + 1) * 32]) for k in range(6)]
    return training.Trainer(model, rule=rule, learning_rate=learning_rate), batches


MODELS = {'head': _head_trainer, 'gcn': _gcn_trainer}


def train_bits(model, rule, loop):
    """Six batches of one training loop -> {key: pinned array}: every weight, every state array, the state block.
    'captured': train_batch_graphed (the first batch eagerly through train_batch, the second captured, the rest replayed);
    'uncaptured': the same with graph=False; 'schedule': 'captured' under ExponentialDecay; 'train_batch': train_batch alone;
    'rate_set': 'captured' with set_learning_rate after the third batch."""
    import torch

    from deep_cbrs_amar_renaissance_amd.utilities import schedules as S
    rate = S.ExponentialDecay(LR, 2, 0.5, staircase=True) if loop == 'schedule' else LR
    trainer, batches = MODELS[model](rule, rate)
    for k, (u, i, y) in enumerate(batches):
        if loop == 'train_batch':
            trainer.train_batch(u, i, y)
        else:
            trainer.train_batch_graphed(u, i, y, graph=loop != 'uncaptured')
        if loop == 'rate_set' and k == 2:
            trainer.set_learning_rate(LR / 4)
    torch.cuda.synchronize()
    assert trainer.t == 6 and bool(trainer._graphs if hasattr(trainer, '_graphs') else False) == (loop in ('captured', 'schedule', 'rate_set'))
    base = 'train/{}/{}/{}/'.format(model, rule, loop)
    out = {}
    for k, prm in enumerate(trainer.params):
        out['{}{:02d}/w'.format(base, k)] = pin(prm.detach().cpu().numpy())
        for j, a in enumerate(trainer.opt_arrays[prm]):
            out['{}{:02d}/s{}'.format(base, k, j)] = pin(a.cpu().numpy())
    if not (trainer.spec.adam and loop == 'train_batch'):             # (a static-rate Adam stepped by train_batch alone counts on the host)
        out[base + 'state'] = pin(state_block(trainer).cpu().numpy())
    return out                                                        # (not the loss: its L2 part is one float atomic per block, in any order)


def train_cases():
    return [(model, rule, loop) for model in MODELS for rule in ('Adam', 'Nadam') for loop in LOOPS if rule == 'Adam' or loop != 'rate_set']

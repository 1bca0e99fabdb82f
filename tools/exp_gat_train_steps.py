"""A short BasicGAT training run (attention and stack dropout) for a kernel trace: with the fused reverse pass on, then off, three
eager steps and four train_batch_graphed steps.  Under `rocprofv3 --kernel-trace --stats -- python tools/exp_gat_train_steps.py` it
gave profiles/stack_tape_split_launches_{before,after}.txt: the launches of a change that must not move any."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cbrs_amar_renaissance_amd import engine, training  # noqa: E402
from deep_cbrs_amar_renaissance_amd.models import basic  # noqa: E402
from tests import helpers  # noqa: E402

CFG = dict(embedding_dim=8, n_hiddens=[16, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48], l2_regularizer=1e-4)
g = helpers.tiny_graph(n_users=80, n_items=60, n_ratings=1500, seed=3)
rng = np.random.default_rng(4)
batches = [(g['u_ids'][k * 64:(k + 1) * 64], g['i_ids'][k * 64:(k + 1) * 64], rng.integers(0, 2, 64)) for k in range(4)]
for switches in ('1', '0'):
    for k in ('AMAR_DENSE_BWD', 'AMAR_DENSE_STACK', 'AMAR_DENSE_STACK_BWD'):
        os.environ[k] = switches
    engine.set_seed(8)
    model = basic.BasicGAT(g['adj'], dropout_rate=0.2, dropout=0.2, **CFG)
    helpers.randomize_biases(model, seed=1)
    trainer = training.Trainer(model)
    for u, i, y in batches[:3]:
        trainer.train_batch(u, i, y)
    for u, i, y in batches:
        trainer.train_batch_graphed(u, i, y)
    torch.cuda.synchronize()
    print('switches', switches, 'steps', trainer.t, 'loss sum', trainer.pop_loss_sum())

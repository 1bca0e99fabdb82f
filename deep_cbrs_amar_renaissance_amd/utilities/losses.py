"""Losses named by `parameters.loss` in the configs (`/root/reference/src/utilities/losses.py:5-25`).

The experiment looks a name up here first (``hasattr(losses, name)`` -> an instance, `experiment.py:155-157` of the reference);
any other name, ``binary_crossentropy`` the default, stays a string and trains with binary cross-entropy.  ``fit()`` and
``evaluate()`` read the compiled loss through `loss_kind`.
"""
import numpy as np


class BPRLoss:
    """Bayesian Personalized Ranking on the model's sigmoid outputs: the batch holds the observed items' scores in its first half
    and the sampled negatives' in its second.  An odd batch drops its last element; with h = B // 2,
    ``loss = -mean_j log sigmoid(p[j] - p[h + j])``, j < h (on probabilities, not logits).  Keras adds the L2 losses."""

    def __init__(self, name="BPR_loss"):
        self.name = name

    def __call__(self, y_true, y_pred):
        """float64 value of the loss for one batch (y_true is not read).  A batch without a pair (B < 2) counts 0."""
        p = np.asarray(y_pred, dtype=np.float64).reshape(-1)
        h = len(p) // 2
        if h == 0:
            return 0.0
        x = p[:h] - p[h:2 * h]
        return float(np.mean(np.logaddexp(0.0, -x)))          # -log sigmoid(x)


def loss_kind(loss):
    """'bpr' for a BPRLoss (instance or name), 'bce' for anything else (the reference's default binary cross-entropy)."""
    if isinstance(loss, BPRLoss) or loss == 'BPRLoss':
        return 'bpr'
    return 'bce'

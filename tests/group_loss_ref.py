"""float64 numpy restatement of the listwise ranking losses of include/amar_hip.h (amar_group_loss_grad_f32), written group by group
from the header's formulas; no torch, no device.  Layout: B = 2h rows (an odd B drops its last), G = h / K groups, group g has the
positive p[g K] and the negatives p[h + g K + k], k < K; rows g K + 1 .. g K + K - 1 repeat the positive's pair and carry nothing.

`group_loss` returns (loss, terms [B], dz [B]); `softmax_f32` is the same softmax evaluated in float32 with a sequential sum, the
yardstick of what float32 leaves on a given input (tests/test_group_losses_cpu.py measures it against `group_loss`)."""
import numpy as np

SOFTMAX, HARDEST, MARGIN = 0, 1, 2            # include/amar_hip.h: AMAR_GROUP_*
KINDS = (SOFTMAX, HARDEST, MARGIN)

# what tests/test_bpr_gpu.py::test_bpr_grad_kernel allows amar_bpr_grad_f32 against its float64 restatement
TERMS_RTOL, TERMS_ATOL = 2e-6, 1e-7
DZ_RTOL, DZ_ATOL = 2e-5, 1e-9


def group_loss(kind, hyper, p, K):
    """(loss, terms [B], dz [B]) in float64.  hyper: the temperature (SOFTMAX) or the margin (MARGIN).  The hardest negative's
    gradient goes to the lowest k at the maximum; a hinge that is not strictly positive gives none; the positive's whole gradient
    sits on row g K, its copies and the trailing element of an odd batch hold exact zeros."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    B, h = len(p), len(p) // 2
    assert K >= 1 and h % K == 0
    G = h // K
    terms, dp = np.zeros(B), np.zeros(B)
    for g in range(G):
        a, b = p[g * K], p[h + g * K:h + (g + 1) * K]
        if kind == SOFTMAX:
            m = max(a, b.max())
            ea, eb = np.exp((a - m) / hyper), np.exp((b - m) / hyper)
            s = ea + eb.sum()
            l = -(a - m) / hyper + np.log(s)
            da, db = (ea / s - 1.0) / hyper, eb / s / hyper
        elif kind == HARDEST:
            k = int(np.flatnonzero(b == b.max())[0])                  # the lowest k at the maximum
            x = a - b[k]
            l = np.log1p(np.exp(-x))
            da, db = -1.0 / (1.0 + np.exp(x)), np.zeros(K)
            db[k] = 1.0 / (1.0 + np.exp(x))
        elif kind == MARGIN:
            v = (hyper - a) + b
            on = v > 0.0
            l = v[on].sum() / K
            da, db = -on.sum() / K, on / K
        else:
            raise ValueError(kind)
        terms[g * K] = (B / G) * l
        dp[g * K] = da / G
        dp[h + g * K:h + (g + 1) * K] = db / G
    loss = terms.sum() / B if B else 0.0
    return loss, terms, dp * p * (1.0 - p)


def softmax_f32(t, p, K):
    """(terms, dz) of the sampled softmax in float32 arithmetic, every sum taken sequentially in ascending k."""
    f = np.float32
    p = np.asarray(p, dtype=f).reshape(-1)
    t = f(t)
    B, h = len(p), len(p) // 2
    G = h // K
    terms, dz = np.zeros(B, dtype=f), np.zeros(B, dtype=f)
    scale, inv_g = f(B) / f(G), f(1) / f(G)
    for g in range(G):
        a, b = p[g * K], p[h + g * K:h + (g + 1) * K]
        m = max(a, b.max())
        eb = np.exp((b - m) / t)
        s = f(0)
        for e in eb:
            s = f(s + e)
        S = f(np.exp((a - m) / t) + s)
        l = np.log1p(s) if a >= b.max() else f((m - a) / t + np.log(S))
        terms[g * K] = scale * f(l)
        dz[g * K] = (inv_g * (-(s / S) / t)) * (a * (f(1) - a))
        dz[h + g * K:h + (g + 1) * K] = (inv_g * ((eb / S) / t)) * (b * (f(1) - b))
    return terms, dz


def scaled_error(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): 1.0 is the edge of numpy's assert_allclose(rtol, atol)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))) if want.size else 0.0


def must_be_zero(B, K):
    """Boolean masks (dz, terms) of the elements that hold exact zeros whatever the data: the positives' copies and the trailing
    element of an odd batch in dz; those and every negative row in terms."""
    h = B // 2
    dz0, t0 = np.zeros(B, dtype=bool), np.ones(B, dtype=bool)
    dz0[:h] = np.arange(h) % K != 0
    dz0[2 * h:] = True
    t0[:h] = dz0[:h]
    return dz0, t0


# ---- the inputs of tests/test_group_losses_gpu.py -------------------------------------------------------------------------------------
K_LADDER = (1, 2, 3, 5, 32, 33, 64, 65, 200)   # both kernel forms (segments up to 32 lanes, a wavefront above) and their edges
G_LADDER = (1, 7, 64)                          # G = 7 comes with an odd B
VARIANTS = ('random', 'ends', 'equal')
TEMPERATURES = (1.0, 0.05)
# sequential float32 softmax against float64 over every softmax input below, as scaled_error against the BPR kernel's bounds
# (terms, dz), measured by tests/test_group_losses_cpu.py::test_float32_sequential_softmax_figures
F32_SEQUENTIAL = {1.0: (0.267, 0.0730), 0.05: (1.176, 0.1094)}


def hyper_of(kind, t=1.0):
    """The hyper-parameter a case runs under, as the float32 the kernel receives."""
    return float(np.float32(t if kind == SOFTMAX else 0.5 if kind == MARGIN else 0.0))


def case_inputs(kind, hyper, K):
    """[(G, B, variant, p float32 [B])] of one (kind, K): every G of the ladder under every variant."""
    out = []
    for G in G_LADDER:
        B = 2 * G * K + (1 if G == 7 else 0)
        for v, variant in enumerate(VARIANTS):
            rng = np.random.default_rng(1000 * K + 10 * G + v)
            out.append((G, B, variant, draw(rng, B, K, kind, hyper, variant)))
    return out


def measure_f32_sequential(t):
    """(terms, dz): the largest scaled error of `softmax_f32` against `group_loss` over the softmax inputs at temperature t."""
    hyper = hyper_of(SOFTMAX, t)
    worst = [0.0, 0.0]
    for K in K_LADDER:
        for G, B, variant, p in case_inputs(SOFTMAX, hyper, K):
            _, terms, dz = group_loss(SOFTMAX, hyper, p, K)
            t32, dz32 = softmax_f32(hyper, p, K)
            worst[0] = max(worst[0], scaled_error(t32, terms, TERMS_RTOL, TERMS_ATOL))
            worst[1] = max(worst[1], scaled_error(dz32, dz, DZ_RTOL, DZ_ATOL))
    return tuple(worst)


def bounds(kind, t=1.0):
    """(terms, dz) bounds of the kernel in units of scaled_error: the BPR kernel's own (1.0) for every kind.  The softmax at large K
    and small temperature did not need more (the kernel's pairwise sums stay at 0.23 of it where the sequential float32 sum of
    F32_SEQUENTIAL leaves 1.18), so the 4x-sequential allowance is not taken."""
    return 1.0, 1.0


def draw(rng, B, K, kind, hyper, variant='random'):
    """float32 probabilities [B] for one case.  'random': uniform in (0, 1); 'ends': exact 0.0 and 1.0 sprinkled in; 'equal': every
    negative of a group the same value.  Under MARGIN, elements whose hinge argument float32 and float64 could sign differently
    (|m - a + b| < 1e-6 and not exactly 0) are nudged away from the kink."""
    h = B // 2
    p = rng.uniform(0.01, 0.99, B).astype(np.float32)
    if variant == 'ends':
        idx = rng.permutation(B)[:max(2, B // 4)]
        p[idx] = rng.integers(0, 2, len(idx)).astype(np.float32)
    elif variant == 'equal' and h:
        G = h // K
        p[h:2 * h] = np.repeat(rng.uniform(0.01, 0.99, G).astype(np.float32), K)
    if kind == MARGIN and h:
        a = np.repeat(p[:h:K].astype(np.float64), K)
        for _ in range(8):
            v = (float(np.float32(hyper)) - a) + p[h:2 * h].astype(np.float64)
            near = (np.abs(v) < 1e-6) & (v != 0.0)
            if not near.any():
                break
            p[h:2 * h][near] = np.float32(0.5) * p[h:2 * h][near]
    return p

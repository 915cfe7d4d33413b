"""The inputs tests/test_gpu_classification.py gives dsdgp_mixture_classification, with fixed seeds, and their CPU reference, computed
once per process.  Every case of CASES keeps, on every item, the three margins of tests/classification_reference.margins above MARGIN
(tests/test_classification_reference_cpu.py asserts it): the gap between the two largest probabilities, the distance of conf B from the
nearest integer, and the smallest |pi_c - pi_y| over c != y.  The device's probabilities are held to rtol 1e-10 / atol 1e-13, so neither
the predicted class, nor the bin, nor the rank of any row can differ and every count must match exactly, no row left out.  (The
constructed tie case of the GPU file states its own expectation and is not in this table.)

Shapes, MultiClass (n, K, S): one row | a ragged last workgroup (four waves take 1, 2 or 4 rows); K = 2 and 32, K = 3, 5, 10 (4 K lanes
of a component never fill whole rounds of 64 except at K = 16, 32); S = 1 (one wave per row), S = 2 and 3 (two waves per row, with
1 | 1 and 2 | 1 components), S >= 4 (four waves per row): S = 5 and 37 (no multiple of four: the waves' component counts differ),
S = 37 and 100 (more than one chunk of 8 components per wave: 10 | 9 | 9 | 9 and 25 each), S = 33 (9 | 8 | 8 | 8: three waves have
nothing left in the second chunk and sit it out — the only way a wave idles; no wave is ever without a component).  Bernoulli (n, D, S): n D = 4095 | 4096 | 8192 | 32768 items, each side of every lanes-per-item threshold of
mix_split_by_items, at S = 3 (where three components lower every one of them to one lane per item) and at S = 17 (16 | 8 | 4 | 1
lanes per item, the last component alone in its round), and a small odd one (16 lanes wanted, S = 5 allows 4)."""
import numpy as np

from tests import classification_reference as R

MARGIN = 1e-9

#        name                 kind          n      D   S    bins
CASES = [
    ("mc_1_2_1",          "multiclass", 1,     2,  1,   10),
    ("mc_17_3_3",         "multiclass", 17,    3,  3,   1),
    ("mc_37_10_37",       "multiclass", 37,    10, 37,  10),
    ("mc_64_32_2",        "multiclass", 64,    32, 2,   32),
    ("mc_300_10_100",     "multiclass", 300,   10, 100, 10),
    ("mc_4099_5_5",       "multiclass", 4099,  5,  5,   32),
    ("mc_37_10_37_b1",    "multiclass", 37,    10, 37,  1),
    ("mc_37_10_37_b32",   "multiclass", 37,    10, 37,  32),
    ("mc_9_4_33",         "multiclass", 9,     4,  33,  10),
    ("bern_37_3_5",       "bernoulli",  37,    3,  5,   10),
    ("bern_4095_1_3",     "bernoulli",  4095,  1,  3,   10),
    ("bern_4096_1_3",     "bernoulli",  4096,  1,  3,   1),
    ("bern_4096_2_3",     "bernoulli",  4096,  2,  3,   32),
    ("bern_16384_2_3",    "bernoulli",  16384, 2,  3,   10),
    ("bern_4095_1_17",    "bernoulli",  4095,  1,  17,  10),
    ("bern_4096_1_17",    "bernoulli",  4096,  1,  17,  10),
    ("bern_4096_2_17",    "bernoulli",  4096,  2,  17,  10),
    ("bern_16384_2_17",   "bernoulli",  16384, 2,  17,  10),
]
NAMES = [c[0] for c in CASES]
_BY_NAME = {c[0]: c for c in CASES}
_refs = {}


def make_inputs(kind, n, D, S, seed):
    """mean ~ randn (spread over the classes so that the least likely ones stay apart), var ~ U(0.01, 1.5); MultiClass labels: the class
    of the largest averaged mean for about 60 % of the rows, a uniform draw else; Bernoulli targets -1 / 1 -> (mean, var, Y)"""
    rng = np.random.RandomState(seed)
    mean = rng.randn(S, n, D) + 0.7 * rng.randn(1, n, D)
    var = rng.uniform(0.01, 1.5, size=(S, n, D))
    if kind == "bernoulli":
        Y = np.where(rng.rand(n, D) < 0.5 + 0.3 * np.tanh(mean.mean(0)), 1.0, -1.0)
    else:
        Y = np.where(rng.rand(n) < 0.6, np.argmax(mean.mean(0), axis=1), rng.randint(0, D, size=n)).astype(np.float64)[:, None]
    return mean, var, Y


def inputs(name):
    _, kind, n, D, S, bins = _BY_NAME[name]
    return (kind, bins) + make_inputs(kind, n, D, S, 7000 + 13 * n + 5 * D + S)


def reference_of(kind, mean, var, Y, bins):
    pbar = R.mixture_probs(kind, mean, var)
    return dict(pbar=pbar, rows=R.rows(kind, pbar, Y, bins), sums=R.sums(kind, pbar, Y, bins), margins=R.margins(kind, pbar, Y, bins))


def reference(name):
    """the case's inputs and reference -> dict(kind, bins, mean, var, Y, pbar, rows, sums, margins); computed once, not to be modified"""
    if name not in _refs:
        kind, bins, mean, var, Y = inputs(name)
        _refs[name] = dict(kind=kind, bins=bins, mean=mean, var=var, Y=Y, **reference_of(kind, mean, var, Y, bins))
    return _refs[name]


def clipped_variances():
    """variances at and below both clips of the MultiClass arithmetic (0 and 1e-12; the clips sit at 0.5e-10 and 1e-10), on some entries"""
    kind, bins, mean, var, Y = inputs("mc_17_3_3")
    var = var.copy()
    var[0, ::2, 0] = 0.0
    var[1, 1::3, 1] = 1e-12
    var[2, 3, :] = 0.0
    return kind, bins, mean, var, Y


def confident_and_wrong():
    """K = 3: class 0 twenty standard deviations above the others in every component, the labels 1 and 2 — pi_y sits a few 1e-5 above
    the floor eps / (K - 1)"""
    rng = np.random.RandomState(41)
    S, n = 3, 6
    mean = np.stack([20.0 + rng.randn(S, n), 0.3 * rng.randn(S, n), -1.0 + 0.3 * rng.randn(S, n)], axis=-1)
    var = rng.uniform(0.5, 1.0, size=(S, n, 3))
    Y = np.array([1.0, 2.0, 1.0, 2.0, 1.0, 0.0])[:, None]
    return "multiclass", 10, mean, var, Y

"""CPU tests of the normal-draw stream's reference (oracle/philox.py) and of the seeds the host mirror hands to the device.

The reference is checked against the published Philox4x32-10 known-answer vectors and against the layout rules of
randn_body (which words of the counter / key carry the pair index, the stream and the seed; the odd-count rule).  The seed
schedule is recorded with a stub engine: every device draw of a model uses the Philox streams 0 .. L-1 under the seed that
dgp.py passes, so a (seed, stream) pair repeats exactly when a seed repeats — across steps, across ELBO / prediction calls or
across the ranks of a data-parallel run (distributed.attach)."""
import types

import numpy as np
import pytest
import torch

from oracle.philox import philox4x32_10, randn_reference
from tests.helpers import kern_spec, product_kernel

# Random123 known-answer vectors for philox4x32-10 (kat_vectors: zero, all-ones and pi-digit counter / key)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(np.array(ctr), np.array(key))
    assert got.dtype == np.uint32
    assert tuple(int(v) for v in got) == want


def test_philox_vectorised_matches_scalar():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, size=(37, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(37, 2), dtype=np.uint64)
    batch = philox4x32_10(ctr, key)
    for j in range(37):
        assert np.array_equal(batch[j], philox4x32_10(ctr[j], key[j]))


def _pair_words(seed, stream, i):
    """The Philox block of pair i of (seed, stream), by the documented counter / key assignment."""
    ctr = np.array([i & 0xFFFFFFFF, i >> 32, stream & 0xFFFFFFFF, stream >> 32], dtype=np.uint64)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))


def test_randn_reference_layout():
    """z[2i], z[2i+1] come from the block of pair i: recompute one pair by hand from its four words."""
    seed, stream = 0x1234_5678_9ABC_DEF0, (7 << 32) | 3
    z = randn_reference(seed, stream, 10)
    for i in (0, 3, 4):
        c = [int(v) for v in _pair_words(seed, stream, i)]
        a, b = (c[1] << 32) | c[0], (c[3] << 32) | c[2]
        u1, u2 = (float(a >> 11) + 0.5) / 2.0 ** 53, (float(b >> 11) + 0.5) / 2.0 ** 53
        r = np.sqrt(-2.0 * np.log(u1))
        assert abs(z[2 * i] - r * np.cos(2 * np.pi * u2)) <= 1e-13 * max(1.0, abs(z[2 * i]))
        assert abs(z[2 * i + 1] - r * np.sin(2 * np.pi * u2)) <= 1e-13 * max(1.0, abs(z[2 * i + 1]))


def test_randn_reference_high_words_matter():
    """the high 32 bits of the seed, of the stream and of the pair index each take part"""
    base = randn_reference(5, 2, 8)
    assert not np.any(randn_reference(5 | 1 << 32, 2, 8) == base)
    assert not np.any(randn_reference(5, 2 | 1 << 32, 8) == base)
    i = 1 << 32                                               # pair 2^32 differs from pair 0 only in the counter's high word
    lo = _pair_words(5, 2, 0)
    hi = _pair_words(5, 2, i)
    assert not np.array_equal(lo, hi)
    # ... and the low words are not aliased either: seed / stream / index 1 versus 0
    assert not np.any(randn_reference(4, 2, 8) == base)
    assert not np.any(randn_reference(5, 3, 8) == base)
    assert not np.array_equal(_pair_words(5, 2, 1), lo)


def test_randn_reference_odd_count_and_prefix():
    """an odd count drops the sine value of the last pair; every count is a prefix of a longer one"""
    long = randn_reference(99, 4, 64)
    for n in (1, 2, 3, 7, 33, 64):
        z = randn_reference(99, 4, n)
        assert z.shape == (n,) and np.array_equal(z, long[:n])
    assert randn_reference(99, 4, 0).shape == (0,)
    with pytest.raises(ValueError):
        randn_reference(-1, 0, 4)
    with pytest.raises(ValueError):
        randn_reference(0, 1 << 64, 4)


def test_randn_reference_moments():
    z = randn_reference(7, 3, 1 << 18)
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 0.02
    assert np.all(np.isfinite(z))


# ---------------------------------------------------------------- seed schedule of the host mirror (dgp.py, distributed.py)
class _RecordingEngine:
    """Stands in for Engine: records the seed of every device evaluation and returns zeros of the right shapes."""

    def __init__(self, model):
        self.model = model
        self.seeds = []
        self.ctx = types.SimpleNamespace(sync=lambda: None)
        self.n_theta = 8
        self.gradbuf = torch.zeros(self.n_theta + 4, dtype=torch.float64)
        self.out4 = self.gradbuf[self.n_theta:]
        self.generation = 1

    def _rec(self, kind, seed):
        self.seeds.append((kind, int(seed)))

    def _ensure(self, n, s):
        pass

    def _upload_if_needed(self):
        pass

    def elbo(self, X, Y, S, zs=None, seed=0, **kw):
        self._rec("elbo", seed)
        return np.zeros(4)

    def train_step(self, X, Y, S, zs=None, seed=0, **kw):
        self._rec("train_step", seed)

    def train_step_minibatch(self, Xall, Yall, idx, off, n, S, seed=0, **kw):
        self._rec("train_step_minibatch", seed)

    def adam_step(self, *a, **kw):
        pass

    def propagate(self, X, S, zs=None, seed=0, want=("F", "mean", "var")):
        self._rec("propagate", seed)
        n = np.shape(X)[0]
        outs = [[torch.zeros(S, n, layer.num_outputs, dtype=torch.float64) for layer in self.model.layers] if k in want else None
                for k in ("F", "mean", "var")]
        return tuple(outs)


def _host_model(monkeypatch, minibatch_size=16):
    from doubly_stochastic_dgp.dgp import DGP, DGP_Base
    from doubly_stochastic_dgp.gpflow_compat import Gaussian
    rng = np.random.RandomState(0)
    N, D = 40, 3
    X, Y = rng.randn(N, D), rng.randn(N, 1)
    model = DGP(X, Y, X[:8].copy(), [product_kernel(kern_spec("rbf", D))] * 3, Gaussian(variance=0.1), num_samples=2,
                minibatch_size=minibatch_size)

    def next_span(self):
        idx = self._minibatch.next_indices()
        return idx, 0, idx.shape[0]

    def next_minibatch(self):
        idx = self._minibatch.next_indices()
        return self.X_data[idx], self.Y_data[idx]

    monkeypatch.setattr(DGP_Base, "_next_index_span", next_span)
    monkeypatch.setattr(DGP_Base, "next_minibatch", next_minibatch)
    eng = _RecordingEngine(model)
    object.__setattr__(model, "_eng", eng)
    object.__setattr__(model, "_dev_data", (model.X_data, model.Y_data))
    return model, eng, X, Y


def _mixed_calls(model, X, Y):
    """training steps (minibatch, full batch, asynchronous and synchronous), ELBO values / gradients and predictions, interleaved"""
    Xs = X[:5]
    for _ in range(3):
        model.train_step(0.01)
    model.compute_log_likelihood(X, Y)
    model.predict_f(Xs, 2)
    model.train_step(0.01, sync=True)
    model.predict_all_layers(Xs, 2)
    model._build_likelihood(X, Y, with_grad=True)
    model.train_step(0.01, X=X, Y=Y)
    model.propagate(Xs, S=3)
    model.train_step(0.01)
    model.predict_f(Xs, 1)
    model._build_likelihood()                                 # next minibatch
    model.train_step(0.01, X=X[:7], Y=Y[:7], sync=True)
    model.predict_all_layers(Xs, 1)
    model.train_step(0.01)


def _draw_pairs(model, eng):
    L = len(model.layers)
    return [(seed, l) for _, seed in eng.seeds for l in range(L)]


def test_seed_schedule_single_process(monkeypatch):
    model, eng, X, Y = _host_model(monkeypatch)
    _mixed_calls(model, X, Y)
    kinds = {k for k, _ in eng.seeds}
    assert kinds == {"elbo", "train_step", "train_step_minibatch", "propagate"}
    pairs = _draw_pairs(model, eng)
    assert len(pairs) == len(set(pairs)), eng.seeds
    # a single process keeps its seeds 1, 2, 3, ... (what every recorded trajectory of the suite was produced with)
    assert [s for _, s in eng.seeds] == list(range(1, len(eng.seeds) + 1))


def test_seed_schedule_two_ranks(monkeypatch):
    """distributed.attach(model, rank, 2): no (seed, stream) pair repeats within a rank (training and prediction seeds) nor across
    the ranks, whatever mix of calls each makes"""
    from doubly_stochastic_dgp import distributed
    monkeypatch.setattr(distributed, "allreduce_flat", lambda buf, world: buf)     # no process group: the sum is not the point
    per_rank = []
    for rank in range(2):
        model, eng, X, Y = _host_model(monkeypatch)
        distributed.attach(model, rank, 2)
        _mixed_calls(model, X, Y)
        if rank == 1:
            model.predict_f(X[:5], 2)                          # the ranks need not make the same number of calls
        pairs = _draw_pairs(model, eng)
        assert len(pairs) == len(set(pairs)), (rank, eng.seeds)
        assert {k for k, _ in eng.seeds} == {"elbo", "propagate"}
        per_rank.append(set(pairs))
    assert not per_rank[0] & per_rank[1], sorted(per_rank[0] & per_rank[1])


def test_engine_randn_streams_are_disjoint_from_the_model_streams():
    """Engine.randn (sample_from_conditional(z=None), the full_cov propagation) draws stream 2^32 | k under seed 0x5eed, k = 1, 2, ...
    per engine: never one of the model's streams 0 .. L-1, never twice."""
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import Engine
    calls = []

    class _Lib:
        def dsdgp_randn(self, handle, seed, stream, n, out):
            calls.append((seed.value, stream.value, n))
            return 0

    fake = types.SimpleNamespace(lib=_Lib(), ctx=types.SimpleNamespace(handle=None, sync=lambda: None,
                                                                       empty=lambda n: torch.zeros(n, dtype=torch.float64)))
    assert _lib.DSDGP_MAX_LAYERS < 1 << 32
    for shape in [(2, 3, 1), (4, 5, 2), (1, 1, 1)]:
        z = Engine.randn(fake, shape)
        assert z.shape == shape
    assert [(s, t) for s, t, _ in calls] == [(0x5eed, 1 << 32 | k) for k in (1, 2, 3)]
    assert [n for *_, n in calls] == [6, 40, 1]

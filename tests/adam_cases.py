"""The layouts and hyper-parameter sets of the direct Adam tests (tests/test_adam_reference_cpu.py, tests/test_gpu_adam_direct.py).

Small layouts: two layers, M in 5..7, D in 2..3.  Between them ARD and isotropic kernels, a white-noise kernel, a trainable Linear mean
function, a white=True model (train_step falls back to elbo + the separate launch) and frozen Parameters of every group; over the
list all nine (even entry, odd entry) mask-class pairs occur, odd and even n_theta, a class-2 and a class-0 last entry
(test_adam_reference_cpu.py::test_pair_census).  All of them sit where the sweep has a thread per pair: slot 0 of a thread's four-pair
batch only, one pass.

Large layout: one layer, M = 1024, 3 -> 5, Gaussian likelihood: n_theta = 5 251 075, odd and above 2^22 — every slot of the batch
live in the first pass and a second, partly filled pass.

Large mixed layout: the same with an ARD kernel plus white noise and a free Linear mean function: n_theta = 5 251 098, and the pairs
(white variance: class 2, A[0, 0]: class 1) and (b[4]: class 1, likelihood variance: class 2) fall into the SECOND pass of the sweep.
In a fused step the owner blocks of k_tail have updated their class-2 entries long before any sweep thread gets there, so a sweep that
stored the neighbour it had loaded would put the old theta, m and v back: the one place where that store can be observed (in the small layouts the sweep's only block is done
before the owner blocks have reduced their gradients, and in the separate launch such a store rewrites the bits it read)."""
import numpy as np

from tests.helpers import kern_spec, make_case

# (lr, beta1, beta2, eps, t)
PARAM_SETS = {
    "default_t1": dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, t=1),
    "default_t1000": dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, t=1000),
    "no_momentum_t3": dict(lr=0.02, b1=0.0, b2=0.99, eps=1e-4, t=3),
    "halves_t2": dict(lr=0.5, b1=0.5, b2=0.5, eps=1e-8, t=2),
}

# frozen: "l<layer>.<Z|q_mu|q_sqrt|kvar|kls|wvar>" or "lik"
SMALL = {
    "m5_ard_whitenoise": dict(M=5, D=3, DY=2, ard=True, wn=(False, True), white=False, linear=False, frozen=()),
    "m6_iso": dict(M=6, D=2, DY=1, ard=False, wn=(False, False), white=False, linear=False, frozen=()),
    "m5_frozen_a": dict(M=5, D=3, DY=2, ard=True, wn=(False, True), white=False, linear=False,
                        frozen=("l0.q_sqrt", "l0.kvar", "l1.Z", "l1.wvar")),
    "m7_linear_frozen_b": dict(M=7, D=3, DY=2, ard=True, wn=(False, False), white=False, linear=True,
                               frozen=("l0.q_mu", "l0.kls", "l1.q_mu", "lik")),
    "m6_frozen_c": dict(M=6, D=2, DY=1, ard=False, wn=(True, False), white=False, linear=False,
                        frozen=("l1.q_sqrt", "l0.kls", "lik")),
    # no likelihood parameter: the last entry is the Linear mean's b, class 1 at odd n_theta — the sweep's single-entry tail is live
    "m5_bernoulli_linear": dict(M=5, D=2, DY=1, ard=False, wn=(False, False), white=False, linear=True, frozen=(), bernoulli=True),
    "m6_white_model": dict(M=6, D=2, DY=2, ard=True, wn=(False, False), white=True, linear=False, frozen=("l0.kvar",)),
}

LARGE = dict(M=1024, D=3, DY=5, N=32, S=2)
LARGE_N_THETA = 1024 * 3 + 1024 * 5 + 5 * 1024 * 1024 + 1 + 1 + 1       # Z, q_mu, q_sqrt, variance, lengthscale, likelihood variance

# Z, q_mu, q_sqrt | variance, 3 lengthscales, white variance | A (3 x 5), b (5) | likelihood variance
LARGE_MIXED_N_THETA = 1024 * 3 + 1024 * 5 + 5 * 1024 * 1024 + 1 + 3 + 1 + 15 + 5 + 1
LARGE_MIXED_PAIRS = {(5251076, 5251077): (2, 1), (5251096, 5251097): (1, 2)}      # (white variance, A[0, 0]), (b[4], likelihood variance)

N_SMALL, S_SMALL, NUM_DATA = 24, 2, 100

# The sweep's launch geometry: workgroups of 256 threads, min(2048, ceil(n_theta / 512)) of them — csrc/model_schedule.hpp:870
# (dsdgp_model_adam_step) and :616 (end_rows_tail, the Adam blocks of k_tail) — and four pairs per thread and pass
# (csrc/model_kernels.hpp:1073, adam_sweep).
WG_THREADS, WG_MAX, ENTRIES_PER_WG, SLOTS = 256, 2048, 512, 4


def sweep_threads(n):
    return WG_THREADS * min(WG_MAX, -(-n // ENTRIES_PER_WG))


def slot_and_pass(i, n):
    """(slot u of the four-pair batch, pass of the grid-stride loop) that handles entry i (array or int) of n; the single entry behind
    the last pair of an odd n is handled outside the loop: (-1, -1)"""
    i = np.asarray(i, dtype=np.int64)
    nt = sweep_threads(n)
    k = i >> 1
    u, p = (k % (SLOTS * nt)) // nt, k // (SLOTS * nt)
    tail = (n & 1) * (i == n - 1)
    return np.where(tail, -1, u), np.where(tail, -1, p)


def _freeze(model, names):
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    for name in names:
        if name == "lik":
            model.likelihood.likelihood.variance.trainable = False
            continue
        l, what = name.split(".")
        layer = model.layers[int(l[1:])]
        stat, wk = split_kernel(layer.kern)
        p = {"Z": layer.feature.Z, "q_mu": layer.q_mu, "q_sqrt": layer.q_sqrt, "kvar": stat.variance, "kls": stat.lengthscales,
             "wvar": wk.variance if wk is not None else None}[what]
        p.trainable = False


def build_small(name, jitter=1e-6):
    """-> (model, X, Y, zs, S) of a small layout; the device model is not created here"""
    from doubly_stochastic_dgp.gpflow_compat import Linear
    c = SMALL[name]
    rng = np.random.RandomState(100 + sorted(SMALL).index(name))
    M, D, DY, N, S = c["M"], c["D"], c["DY"], N_SMALL, S_SMALL
    X, Y = rng.randn(N, D), rng.randn(N, DY)
    if c.get("bernoulli"):
        Y = (Y > 0).astype(np.float64)
    Z = X[:M] + 0.1 * rng.randn(M, D)
    specs = [kern_spec("rbf" if l == 0 else "matern52", D, 1.1 - 0.2 * l, (0.8 + 0.4 * rng.rand(D)) if c["ard"] else 1.2, ARD=c["ard"],
                       white_variance=0.05 if c["wn"][l] else None) for l in range(2)]
    _, _, model = make_case(X, Y, Z, specs, white=c["white"], jitter=jitter, S=S, num_data=NUM_DATA, seed=7,
                            bernoulli=bool(c.get("bernoulli")))
    if c["linear"]:                                  # a free Linear mean function on the last layer: A and b live in theta
        model.layers[-1].mean_function = Linear(0.3 * rng.randn(D, DY), 0.5 * rng.randn(DY))
    _freeze(model, c["frozen"])
    zs = [rng.randn(S, N, D), rng.randn(S, N, DY)]
    return model, X, Y, zs, S


def build_large(mixed=False):
    """-> (model, X, Y, zs, S) of the large layout (mixed: of the large mixed layout)"""
    from doubly_stochastic_dgp.gpflow_compat import Linear
    c = LARGE
    rng = np.random.RandomState(6 if mixed else 5)
    X, Y = rng.randn(c["N"], c["D"]), rng.randn(c["N"], c["DY"])
    Z = 3.0 * rng.randn(c["M"], c["D"])
    spec = kern_spec("rbf", c["D"], 1.0, [0.6, 0.7, 0.8], ARD=True, white_variance=0.05) if mixed else kern_spec("rbf", c["D"], 1.0, 0.7)
    _, _, model = make_case(X, Y, Z, [spec], S=c["S"], num_data=1000, seed=9)
    if mixed:
        model.layers[-1].mean_function = Linear(0.3 * rng.randn(c["D"], c["DY"]), 0.5 * rng.randn(c["DY"]))
    zs = [rng.randn(c["S"], c["N"], c["DY"])]
    return model, X, Y, zs, c["S"]

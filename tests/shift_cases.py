"""Inputs of the joint-shift tests (tests/shift_reference.py, tests/test_shift_reference_cpu.py, tests/test_gpu_kernel_shift.py).

A stationary kernel, Identity mean functions on the inner layers and a zero mean on the last make the model translation-invariant:
shift X and every layer's Z by one vector and the ELBO, every layer's variance, every gradient block and, after subtracting the shift,
every inner layer's mean are mathematically unchanged (init_layers_linear passes Z through the mean functions, so shifting the model's
Z shifts every layer's).  X and Z lie on the grid 2^-20 with |x| < 8 and the shifts are +- 2^6 / +- 2^10 per dimension, so X + c s and
Z + c s are exact in float64 (23 + 11 bits): the shifted problem IS the unshifted one and only the arithmetic sees the offset.

CASES: name -> dict(kind, white, D, M, N, L, S, widths, coincide, seed, force).  widths are the layers' output widths (inner layers keep D:
Identity mean), Z[:coincide] = X[:coincide] bit for bit, force is the DSDGP_FORCE value of the configuration (device side only).
ARD lengthscales in 0.7 .. 1.3, variance 1.3, jitter 1e-6, Gaussian likelihood, q_mu / q_sqrt randomised by tests.helpers.make_case.
Matern52 goes with white = True: make_case initialises a non-white q_sqrt from the UPSTREAM K(Z, Z), which at these offsets can be
the NaN that tests/test_shift_reference_cpu.py asserts.  The coordinates have standard deviation 1.2 / sqrt(D), so that a typical scaled
squared distance is about 3 at every width and the kernel matrices are neither the identity nor constant.
The seeds were chosen on the float64 reference alone, among a handful per case, for room under the conditions of
tests/test_shift_reference_cpu.py (no member of the family beyond 4 x the other three where 8 is asked, the family at 2^10 below
2.5e-7 where 1e-6 is asked): the family is rounding noise and its realisation follows the host's BLAS."""
import functools

import numpy as np

GRID = 2.0 ** -20
VARIANCE = 1.3
JITTER = 1e-6
LIK_VAR = 0.1
SHIFTS = (2.0 ** 6, 2.0 ** 10)
CASE_SEED = 7           # make_case's seed (q_mu, q_sqrt)
_SIGNS4 = ((1, 1, 1, 1), (1, -1, 1, -1), (-1, -1, 1, 1), (-1, 1, 1, -1))


def _c(kind, white, D, M, N, L, S, widths, coincide, seed, force=None):
    return dict(kind=kind, white=white, D=D, M=M, N=N, L=L, S=S, widths=widths, coincide=coincide, seed=seed, force=force)


CASES = {
    # head Ku, chain Kuf, masked k-steps (D = 4 < 16)
    "1_head_chain": _c("rbf", False, 4, 24, 48, 2, 3, (4, 2), 8, 1018),
    # direct Ku with expanded Kuf
    "2_head_off": _c("matern52", True, 4, 24, 48, 2, 3, (4, 2), 8, 1001, "head=0"),
    # the GEMM-formulated passes (direct K(Z, X) with the head launch's expanded Ku)
    "3_gemm": _c("rbf", True, 4, 24, 48, 2, 3, (4, 2), 8, 1001, "gemm_mp=16"),
    # whole groups of 16 dimensions, fused last layer
    "4_m128_d16": _c("rbf", False, 16, 128, 64, 2, 2, (16, 1), 8, 1005),
    # 8-wave instances, Ku outside the head launch
    "5_m150": _c("matern52", True, 5, 150, 48, 2, 2, (5, 2), 8, 1005),
    # 8-wave plain-row operand layout, Csave backward chain
    # (RBF at M = 300 in six dimensions has a Ku of condition ~1e6 at jitter 1e-6: the float64 family itself moves by 1e-4)
    "6_m300": _c("matern52", True, 6, 300, 40, 2, 2, (6, 1), 0, 1007),
    # the wide instances, chunked over XCH
    "7_wide_d80": _c("matern52", True, 80, 40, 48, 1, 2, (1,), 0, 1007),
}


def signs(D):
    """The four fixed sign patterns, extended periodically to D dimensions: (4, D) of +-1."""
    return np.array([[p[d % 4] for d in range(D)] for p in _SIGNS4], dtype=np.float64)


def _grid(a):
    return np.clip(np.round(a / GRID) * GRID, -8.0 + GRID, 8.0 - GRID)


def arrays(name):
    """The unshifted arrays of a case: dict(X, Y, Z, ls, zs)."""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    D, M, N, S = c["D"], c["M"], c["N"], c["S"]
    sd = 1.2 / np.sqrt(D)
    X = _grid(sd * rng.randn(N, D))
    Z = _grid(sd * rng.randn(M, D))
    Z[:c["coincide"]] = X[:c["coincide"]]
    Y = rng.randn(N, c["widths"][-1])
    ls = [0.7 + 0.6 * rng.rand(D) for _ in range(c["L"])]
    zs = [rng.randn(S, N, w) for w in c["widths"]]
    return dict(X=X, Y=Y, Z=Z, ls=ls, zs=zs)


def shift_vector(name, c, pattern):
    """c times sign pattern `pattern` (0 .. 3); c = 0 gives zeros."""
    return float(c) * signs(CASES[name]["D"])[pattern]


def kern_specs(name, arr):
    from tests.helpers import kern_spec
    c = CASES[name]
    return [kern_spec(c["kind"], c["D"], VARIANCE, arr["ls"][l], ARD=True) for l in range(c["L"])]


@functools.lru_cache(maxsize=None)
def _unshifted_q_sqrt(name):
    """What make_case gives a non-white case's q_sqrt at c = 0, from the oracle side alone (no device model is built for it):
    tests/test_shift_reference_cpu.py holds every shifted state to make_case's own unshifted one bit for bit, q_sqrt included."""
    from oracle import dgp_oracle as O
    arr = arrays(name)
    lds = O.init_layers_linear(arr["X"], arr["Y"], arr["Z"], kern_specs(name, arr), white=False, jitter=JITTER)
    rng = np.random.RandomState(CASE_SEED)
    out = []
    for l in lds:
        rng.randn(*l["q_mu"].shape)
        D, M = l["q_sqrt"].shape[:2]
        out.append(l["q_sqrt"] * 0.7 + 0.05 * np.tril(rng.randn(D, M, M)))
    return out


def build(name, c=0.0, pattern=0):
    """make_case at X + c s, Z + c s -> (spec, state, model, X + c s, arr, shift).  q_mu and q_sqrt are those of the unshifted case
    on both sides: make_case derives a non-white q_sqrt from K(Z, Z) by the upstream form, whose rounding depends on the offset, and
    the shifted problem must differ from the unshifted one in X and Z only."""
    from tests.helpers import make_case
    cs = CASES[name]
    arr = arrays(name)
    sh = shift_vector(name, c, pattern)
    kw = dict(white=cs["white"], jitter=JITTER, lik_var=LIK_VAR, S=cs["S"], num_data=4 * cs["N"], seed=CASE_SEED)
    spec, state, model = make_case(arr["X"] + sh, arr["Y"], arr["Z"] + sh, kern_specs(name, arr), **kw)
    if c != 0.0 and not cs["white"]:
        for l, (layer, q_sqrt) in enumerate(zip(model.layers, _unshifted_q_sqrt(name))):
            state[f"l{l}.q_sqrt"] = q_sqrt.copy()
            layer.q_sqrt = q_sqrt
    return spec, state, model, arr["X"] + sh, arr, sh

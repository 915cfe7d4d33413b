"""The case table of the stack of sparse sampled layers (tests/test_gpu_sgpmc_stack.py, tests/test_sgpmc_stack_reference_cpu.py,
tests/test_sgpmc_stack_plan_cpu.py): small shapes that reach every branch of csrc/sgpmc_stack.hip —
    depth L = 1, 2, 3;  rows R = S n against the workgroups of 256: 1, 255, 257, 800, and 120, 18;
    outputs DO = 1, 2, 3, 16, 17;  propagated inputs p = 0 and 2;  mean functions Zero, Identity, Linear (with and without b, a step down
    from D_in = 5 to DO = 3);  `white` on and off;  RBF and Matern52, scalar and ARD lengthscales, a White part;  M = 5 (padded) and 16;
    draws given and drawn (seed DRAW_SEED, stream = the layer: oracle/philox.py restates dsdgp_randn on the host);
    likelihoods Gaussian, Bernoulli, Poisson, StudentT (two outputs), MultiClass (K = 3);
    `zero_var` (forward only): jitter 0, M = 1, kernel variance 1 and a row of X on Z's only row — Ku = Lu = A = 1, so that row's
    conditional variance is exactly 0 at every precision and its sample is its mean.  Its reverse would divide by zero: the case is in
    no gradient test.
Conditioning: Z is standard normal with lengthscales sqrt(D) U(0.7, 1.4), and the jitter is 0.05: cond(Ku) <= (1.3 * 16 + 0.05) / 0.05
= 417, and var + jitter >= 0.05 at every sampled row, far above 1e-8 of the kernel's diagonal.  tests/test_sgpmc_stack_reference_cpu.py
holds the table to both conditions.  The long-double truth and its float64 twin are computed once per case."""
import functools

import numpy as np

from oracle import philox
from tests import sgpmc_stack_reference as KR

RBF, MATERN52 = 0, 1
VARIANCE = 1.3
JITTER = 0.05
DRAW_SEED = 20141

#  layer: (kind, ard, white_var, white, M, DO, p, mean)
CASES = {
    #           n    S  D0  layers                                                                                       lik                          zs
    "r1":      (1,   1, 2, [(RBF, 0, None, True, 5, 1, 0, "zero")],                                                       ("gaussian", 0.3, 1.0),      "given"),
    "r255":    (51,  5, 3, [(RBF, 1, None, False, 16, 3, 2, "identity"), (MATERN52, 0, 0.2, True, 5, 3, 0, "linear")],   ("multiclass", 1.0, 1.0),    "given"),
    "r257":    (257, 1, 2, [(MATERN52, 1, None, True, 16, 17, 0, "zero"), (RBF, 0, 0.1, False, 5, 16, 2, "linear_b"),
                            (RBF, 1, None, False, 16, 1, 0, "zero")],                                                     ("bernoulli", 1.0, 1.0),     "drawn"),
    "r800":    (100, 8, 5, [(RBF, 0, None, False, 5, 3, 0, "linear"), (MATERN52, 1, None, True, 16, 3, 2, "identity"),
                            (RBF, 0, 0.15, True, 5, 1, 0, "zero")],                                                       ("poisson", 1.0, 1.5),       "given"),
    "student": (40,  3, 2, [(RBF, 1, None, False, 5, 1, 2, "zero"), (MATERN52, 0, None, True, 16, 2, 0, "zero")],         ("student_t", 0.7, 3.0),     "drawn"),
}
NAMES = list(CASES)
FORWARD_ONLY = "zero_var"
CASES_FWD = {FORWARD_ONLY: (9, 2, 2, [(RBF, 0, None, True, 1, 1, 0, "zero"), (RBF, 0, 0.2, False, 5, 1, 0, "zero")], ("gaussian", 0.3, 1.0), "given")}
ZERO_ROW = 3


@functools.lru_cache(maxsize=None)
def case(name):
    n, S, D0, layers, lik, zmode = CASES.get(name) or CASES_FWD[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 13 * n + S)
    zero_var = name == FORWARD_ONLY
    X = rng.standard_normal((n, D0))
    R, D, out, zs = n * S, D0, [], []
    for l, (kind, ard, wv, white, M, DO, p, mean) in enumerate(layers):
        Z = rng.standard_normal((M, D))
        ls = np.sqrt(D) * rng.uniform(0.7, 1.4, D if ard else 1)
        last = l + 1 == len(layers)
        q_mu = rng.standard_normal((M, DO)) * (0.5 if last else 1.0)
        A = b = None
        if mean.startswith("linear"):
            A = rng.standard_normal((D, DO)) / np.sqrt(D)
            b = rng.standard_normal(DO) if mean == "linear_b" else np.zeros(DO)
        variance = VARIANCE
        if zero_var and l == 0:
            variance, X[ZERO_ROW] = 1.0, Z[0]
        out.append(dict(kind=kind, ard=bool(ard), white_var=wv, white=white, M=M, D=D, DO=DO, p=p, mean=mean.split("_")[0], A=A, b=b, Z=Z,
                        q_mu=q_mu, variance=variance, ls=ls))
        if not last:
            zs.append(rng.standard_normal((R, DO)) if zmode == "given" else philox.randn_reference(DRAW_SEED, l, R * DO).reshape(R, DO))
        D = p + DO
    DY = layers[-1][5]
    if lik[0] == "multiclass":
        Y = rng.integers(0, DY, (n, 1)).astype(np.float64)
    elif lik[0] == "bernoulli":
        Y = rng.integers(0, 2, (n, DY)).astype(np.float64)
    elif lik[0] == "poisson":
        Y = rng.integers(0, 5, (n, DY)).astype(np.float64)
    else:
        Y = rng.standard_normal((n, DY))
    return dict(name=name, layers=out, X=X, Y=Y, n=n, S=S, zs=zs, zmode=zmode, jitter=0.0 if zero_var else JITTER, data_scale=2.5, lik=lik)


def shape_args(name):
    """[L, n, S, DY, then M, D, DO, p per layer]: the arguments of the plan"""
    c = case(name)
    out = [len(c["layers"]), c["n"], c["S"], c["layers"][-1]["DO"]]
    for y in c["layers"]:
        out += [y["M"], y["D"], y["DO"], y["p"]]
    return out


@functools.lru_cache(maxsize=None)
def propagate(name, dtype=KR.LD):
    return KR.propagate(case(name), dtype)


@functools.lru_cache(maxsize=None)
def logdensity(name, dtype=KR.LD):
    return KR.logdensity(case(name), dtype)


def bar(truth, twin):
    """the project's bar of one output array, in the max norm: 8 max(the float64 twin's own error, 2^-50 of the array's largest magnitude)"""
    truth, twin = np.atleast_1d(np.asarray(truth)), np.atleast_1d(np.asarray(twin))
    return 8.0 * max(float(np.max(np.abs(twin - truth))), 2.0 ** -50 * float(np.max(np.abs(truth))))


def ratio(dev, truth, twin):
    """max |device - truth| over the bar (inf where the bar is 0 and the device is not exact)"""
    truth = np.atleast_1d(np.asarray(truth))
    dev = np.atleast_1d(np.asarray(dev)).reshape(truth.shape)
    err, b = float(np.max(np.abs(dev - truth))), bar(truth, twin)
    if not np.isfinite(err):
        return float("inf")
    return err / b if b > 0.0 else (0.0 if err == 0.0 else float("inf"))


# ---------------------------------------------------------------------------------------------- the host mirror of a case (needs the library)
class jitter:
    """settings.jitter set for a block: the host mirror reads it at every evaluation"""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from doubly_stochastic_dgp import settings
        self.old, settings.jitter = settings.jitter, self.value

    def __exit__(self, *a):
        from doubly_stochastic_dgp import settings
        settings.jitter = self.old


def zs3(c):
    """the case's draws as the model takes them: (S, n, D_out) per sampled layer"""
    return [z.reshape(c["S"], c["n"], -1) for z in c["zs"]]


def model_of(c):
    """the DGP_SGPMC of a case"""
    from doubly_stochastic_dgp import gpflow_compat as G
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_SGPMC
    layers = []
    for y in c["layers"]:
        K = (G.RBF if y["kind"] == RBF else G.Matern52)(y["D"], variance=y["variance"], lengthscales=y["ls"] if y["ard"] else float(y["ls"][0]),
                                                            ARD=y["ard"])
        if y["white_var"] is not None:
            K = K + G.White(y["D"], variance=y["white_var"])
        if y["mean"] == "linear":
            mf = G.Linear(y["A"], y["b"])
            mf.set_trainable(False)
        else:
            mf = G.Identity() if y["mean"] == "identity" else G.Zero()
        layer = SGPMC_Layer(K, y["Z"], y["DO"], mf, white=y["white"], input_prop_dim=y["p"] or None)
        layer.q_mu = y["q_mu"]
        layers.append(layer)
    name, p0, p1 = c["lik"]
    lik = {"gaussian": lambda: G.Gaussian(p0), "multiclass": lambda: G.MultiClass(c["layers"][-1]["DO"]), "bernoulli": G.Bernoulli,
           "poisson": lambda: G.Poisson(binsize=p1), "student_t": lambda: G.StudentT(scale=p0, deg_free=p1)}[name]()
    return DGP_SGPMC(c["X"], c["Y"], lik, layers, num_samples=c["S"], num_data=c["data_scale"] * c["n"])

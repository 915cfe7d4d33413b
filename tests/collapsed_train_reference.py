"""The yardstick of the tests of the collapsed model's reverse pass through its inner layers (tests/test_collapsed_train_cpu.py,
tests/test_gpu_collapsed_train.py): torch CPU float64 autograd of

    bound(mean_L, var_L; Z, v, l, s2) - sum_l KL_l

where the inner layers are the oracle's (oracle.model.build(O.TH, ...).propagate at S = 1) and the collapsed bound is restated in torch
in its direct form: Kuu with jitter, psi0 / psi1 / psi2 as tests/psi_reference.py writes them, the six terms of
tests/collapsed_reference.collapsed_from.  `cases()` builds the product models and the oracle description from the same numbers."""
import math

import numpy as np

from oracle import dgp_oracle as O
from oracle import model as OM
from tests import collapsed_reference as CR
from tests.helpers import kern_spec, make_case

JITTER = 1e-6
NOISE = 0.1


def torch_bound(mu, s, Z, variance, ls, Y, noise, jitter):
    """the bound of tests/collapsed_reference.collapsed in torch; ls has one entry or D"""
    import torch
    N, D = mu.shape
    M, DY = Z.shape[0], Y.shape[1]
    l2 = (ls.reshape(-1) * torch.ones(D, dtype=torch.float64)) ** 2
    psi0 = N * variance
    a1 = l2 + s
    d1 = mu[:, None, :] - Z[None, :, :]
    psi1 = variance * torch.sqrt(torch.prod(l2 / a1, dim=1))[:, None] * torch.exp(-0.5 * torch.sum(d1 * d1 / a1[:, None, :], dim=2))
    dz = Z[:, None, :] - Z[None, :, :]
    e0 = torch.sum(dz * dz / (4.0 * l2), dim=2)
    a2 = l2 + 2.0 * s
    pre2 = variance * variance * torch.sqrt(torch.prod(l2 / a2, dim=1))
    dm = (d1[:, :, None, :] + d1[:, None, :, :]) / 2.0
    e1 = torch.sum(dm * dm / a2[:, None, None, :], dim=3)
    psi2 = torch.sum(pre2[:, None, None] * torch.exp(-(e0[None] + e1)), dim=0)
    Kuu = variance * torch.exp(-0.5 * torch.sum(dz * dz / l2, dim=2)) + jitter * torch.eye(M, dtype=torch.float64)
    sol = lambda L, B: torch.linalg.solve_triangular(L, B, upper=False)
    L = torch.linalg.cholesky(Kuu)
    A = sol(L, psi1.T) / torch.sqrt(noise)
    AAT = sol(L, sol(L, psi2).T) / noise
    LB = torch.linalg.cholesky(AAT + torch.eye(M, dtype=torch.float64))
    c = sol(LB, A @ Y) / torch.sqrt(noise)
    return (-0.5 * N * DY * torch.log(2.0 * math.pi * noise) - DY * torch.sum(torch.log(torch.diagonal(LB))) - 0.5 * torch.sum(Y * Y) / noise
            + 0.5 * torch.sum(c * c) - 0.5 * DY * psi0 / noise + 0.5 * DY * torch.trace(AAT))


class Case:
    """One collapsed model: `dgp` (product DGP whose last layer lends its kernel and inducing inputs), X, Y, zs (per inner layer, (1, N,
    D_out)), the oracle's spec / state of the INNER layers, and the collapsed layer's constrained values `top`."""

    def __init__(self, name, N, M, widths, white=False, ard=False, seed=0, white_part=None):
        rng = np.random.default_rng(seed)
        D = widths[0]
        self.name, self.N, self.M = name, N, M
        self.X = rng.standard_normal((N, D))
        self.Y = np.sin(self.X @ rng.standard_normal((D, 1))) + 0.2 * rng.standard_normal((N, 1))
        ls = 1.1
        Z = CR.spaced_points(rng, M, D, 0.5 * ls)          # the spacing tests/collapsed_reference.py asks of inducing inputs
        specs = [kern_spec("rbf", d, 1.2, (ls + 0.2 * rng.uniform(size=d)) if ard else ls, ard, white_variance=white_part if i == 0 else None)
                 for i, d in enumerate(widths)]
        self.spec_all, self.state_all, self.dgp = make_case(self.X, self.Y, Z, specs, white=white, jitter=JITTER, lik_var=NOISE, S=1, seed=seed)
        L = len(widths)
        self.n_inner = L - 1
        self.spec = dict(self.spec_all, layers=self.spec_all["layers"][:-1])
        self.state = {k: v for k, v in self.state_all.items() if k == "lik_variance_raw" or int(k[1:k.index(".")]) < L - 1}
        last = f"l{L - 1}."
        self.top = dict(Z=np.array(self.state_all[last + "Z"]), variance=1.2, lengthscales=np.atleast_1d(np.asarray(specs[-1]["lengthscales"], dtype=np.float64)),
                        lik_variance=NOISE)
        self.zs = [rng.standard_normal((1, N, d)) for d in list(widths[1:])]

    def collapsed_model(self):
        from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
        return DGP_Collapsed.from_dgp(self.dgp)

    def evaluate(self, state=None, top=None, grad=True):
        """(bound - sum KL, {state key: gradient with respect to the RAW entry}, {top key: gradient with respect to the constrained value},
        mean_L, var_L (N, D) numpy)"""
        import torch
        t = lambda a, g: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=g)
        leaves = {k: t(v, grad) for k, v in (state or self.state).items()}
        tops = {k: t(v, grad) for k, v in (top or self.top).items()}
        m = OM.build(O.TH, self.spec, leaves)
        zs = [torch.as_tensor(z) for z in self.zs]
        _, Fm, Fv = m.propagate(O.TH, torch.as_tensor(self.X), zs, S=1)
        mu, s = Fm[-1][0], Fv[-1][0]
        val = torch_bound(mu, s, tops["Z"], tops["variance"], tops["lengthscales"], torch.as_tensor(self.Y), tops["lik_variance"], JITTER)
        val = val - sum(layer.KL(O.TH) for layer in m.layers)
        if not grad:
            return float(val), mu.numpy(), s.numpy()
        val.backward()
        g = lambda d: {k: (x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)) for k, x in d.items()}
        return float(val.detach()), g(leaves), g(tops), mu.detach().numpy(), s.detach().numpy()


def constrained_gradient(key, g_raw, raw):
    """gradient with respect to the constrained value of an oracle state entry from the one with respect to the raw entry: the raw
    kernel variances and lengthscales go through softplus + 1e-6, whose slope is the sigmoid of the raw value; q_sqrt keeps its lower
    triangle; everything else is its own free variable"""
    if key.endswith("_raw"):
        return g_raw * (1.0 + np.exp(-np.asarray(raw, dtype=np.float64)))
    return np.tril(g_raw) if key.endswith("q_sqrt") else g_raw


_CASES = {}
#                 N   M  widths      white  ard   seed  white part of layer 0's kernel
TABLE = {
    "two": (40, 6, (2, 2), False, False, 1, None),
    "three": (70, 17, (3, 3, 3), False, True, 2, None),
    "white": (40, 6, (2, 2), True, False, 3, 0.03),
}


def case(name):
    """shared: do not write to a case's arrays (a test that trains builds its own Case)"""
    if name not in _CASES:
        N, M, widths, white, ard, seed, wp = TABLE[name]
        _CASES[name] = Case(name, N, M, widths, white=white, ard=ard, seed=seed, white_part=wp)
    return _CASES[name]


def reference(name):
    key = ("ref", name)
    if key not in _CASES:
        _CASES[key] = case(name).evaluate()
    return _CASES[key]

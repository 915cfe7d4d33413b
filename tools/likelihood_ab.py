#!/usr/bin/env python
"""Bits of every path through the element-wise likelihood kernels, for a before/after comparison of two library builds.

Run once per build (DSDGP_LIB_PATH names the library), then compare the two files:

  DSDGP_LIB_PATH=$PWD/tools/bin/libdsdgp_base.so python tools/likelihood_ab.py --out /tmp/lik_base.npz
  python tools/likelihood_ab.py --out /tmp/lik_new.npz
  python tools/likelihood_ab.py --compare /tmp/lik_base.npz /tmp/lik_new.npz --md /tmp/lik_ab.md      (the table of profiles/likelihood_family_ab.md)

Per likelihood (Gaussian, Bernoulli, Poisson, Exponential, StudentT, Gamma, Beta) the file holds
  elbo / grad    out4 and the whole gradient vector of one ELBO evaluation, N = 50, D = 2, M = 19, S = 3, DY = 2, for L = 1 (the adjoints
                 stored as dmean / dvar) and L = 2 (stored transposed, MBt / VBt: S N = 150 is no multiple of 16, so the padding rows
                 are written; N DY S = 300 leaves a ragged last workgroup), without and with quadrature weights; the Gaussian also with
                 DSDGP_FORCE=lik_fuse=0 (the likelihood kernel in place of the last chain's fused epilogue)
  ve / ve_w / density / pred_mean / pred_var / mix_acc / mix_rows
                 the primitives at S = 4, N = 37, D = 3: variational_expectations_mean without and with weights,
                 predict_density_logmeanexp, predict_mean_and_var, evaluate_mixture(rows=True)
`--compare` exits non-zero unless every array of the two files is equal (np.array_equal; NaNs in the same places count as equal)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)

NAMES = ["gaussian", "bernoulli", "poisson", "exponential", "student_t", "gamma", "beta"]


def make_likelihood(name):
    from doubly_stochastic_dgp.gpflow_compat import Bernoulli, Beta, Exponential, Gamma, Gaussian, Poisson, StudentT
    return {"gaussian": lambda: Gaussian(variance=0.7), "bernoulli": Bernoulli, "poisson": lambda: Poisson(binsize=1.6),
            "exponential": Exponential, "student_t": lambda: StudentT(scale=0.7, deg_free=4.5), "gamma": lambda: Gamma(shape=1.8),
            "beta": lambda: Beta(scale=2.5)}[name]()


def targets(name, rng, N, DY):
    if name == "bernoulli":
        return np.where(rng.uniform(size=(N, DY)) < 0.5, -1.0, 1.0)
    if name == "poisson":
        return rng.poisson(2.0, size=(N, DY)).astype(np.float64)
    if name in ("exponential", "gamma"):
        return rng.exponential(1.3, size=(N, DY)) + 1e-3
    if name == "beta":
        y = rng.uniform(0.02, 0.98, size=(N, DY))
        y.ravel()[:2] = [0.0, 1.0]      # clipped by the density
        return y
    return rng.standard_t(4.0, size=(N, DY))


def elbo_case(name, L, weighted, force=None):
    """(out4, gradient vector) of one ELBO evaluation with explicit draws"""
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import Matern52, White
    N, D, M, S, DY = 50, 2, 19, 3, 2
    rng = np.random.RandomState(60 + L)
    X = rng.uniform(size=(N, D))
    Y = targets(name, rng, N, DY)
    old = os.environ.pop("DSDGP_FORCE", None)
    if force:
        os.environ["DSDGP_FORCE"] = force      # read when the device model is created
    try:
        model = DGP(X, Y, X[:M].copy(), [Matern52(D, variance=1.0, lengthscales=0.5) + White(D, variance=0.01) for _ in range(L)],
                    make_likelihood(name), num_samples=S, num_data=200)
        for layer in model.layers:
            layer.q_mu = 0.3 * rng.randn(*layer.q_mu.shape)
            q = np.asarray(layer.q_sqrt.value)
            layer.q_sqrt = q * 0.7 + 0.05 * np.tril(rng.randn(*q.shape))
        zs = [rng.randn(S, N, D) for _ in range(L - 1)] + [rng.randn(S, N, DY)]
        eng = model.engine()
    finally:
        os.environ.pop("DSDGP_FORCE", None)
        if old is not None:
            os.environ["DSDGP_FORCE"] = old
    if weighted:
        eng.set_sample_weights(eng.ctx.to_device(np.array([0.2, 0.5, 0.3])))
    out4 = eng.elbo(X, Y, S, zs=zs, data_scale=200.0 / N, with_grad=True)
    eng.ctx.sync()
    return np.array(out4), eng.grad.cpu().numpy().copy()


def primitive_case(name):
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    rng = np.random.RandomState(5)
    S, N, D = 4, 37, 3
    mu, var = 1.2 * rng.randn(S, N, D), rng.uniform(1e-6, 2.0, size=(S, N, D))
    Y = targets(name, rng, N, D)
    w = rng.uniform(size=S)
    lik = BroadcastingLikelihood(make_likelihood(name))
    pm, pv = lik.predict_mean_and_var(mu, var)
    acc, rows = lik.evaluate_mixture(mu, var, Y, rows=True)
    return {"ve": lik.variational_expectations_mean(mu, var, Y), "ve_w": lik.variational_expectations_mean(mu, var, Y, weights=w),
            "density": lik.predict_density_logmeanexp(mu, var, Y), "pred_mean": pm, "pred_var": pv, "mix_acc": acc, "mix_rows": rows}


def collect():
    out = {}
    for name in NAMES:
        for L in (1, 2):
            for weighted in (False, True):
                forces = (None, "lik_fuse=0") if name == "gaussian" else (None,)
                for force in forces:
                    key = f"{name}.L{L}{'.w' if weighted else ''}{'.unfused' if force else ''}"
                    out[key + ".elbo"], out[key + ".grad"] = elbo_case(name, L, weighted, force)
        for k, v in primitive_case(name).items():
            out[f"{name}.{k}"] = np.asarray(v)
    return out


def compare(a_path, b_path, md):
    a, b = np.load(a_path), np.load(b_path)
    lines = ["| array | shape | finite | equal bits |", "|---|---|---|---|"]
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(np.signbit(a[k]), np.signbit(b[k]))
        lines.append(f"| {k} | {a[k].shape} | {int(np.isfinite(a[k]).sum())} / {a[k].size} | {'yes' if same else 'NO'} |")
        if not same:
            bad.append(k)
    text = "\n".join(lines) + f"\n\n{len(a.files)} arrays, {len(bad)} differ" + (f": {bad}" if bad else "") + "\n"
    print(text)
    if md:
        with open(md, "w") as f:
            f.write(text)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write this build's arrays to OUT.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--md", default=None, help="with --compare: write the table here")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.md))
    arrays = collect()
    np.savez(args.out or "likelihood_ab.npz", **arrays)
    print(f"{len(arrays)} arrays -> {args.out or 'likelihood_ab.npz'} (library: {os.environ.get('DSDGP_LIB_PATH', 'in-tree')})")


if __name__ == "__main__":
    main()

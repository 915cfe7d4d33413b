#!/usr/bin/env python
"""Bits of the collapsed path — the kernel expectations, their reverse pass, SGPR_Layer, and the k-means and PCA entry points that share
the block sum — for a before/after comparison of two checkouts (library AND Python package).

Run once per checkout, then compare the two files.  The base is a parent commit's library as tools/bin/libdsdgp_base.so and its package
under tools/bin/base/ (git archive <commit> doubly-stochastic-dgp_amd/doubly_stochastic_dgp | tar -x -C tools/bin/base):

  DSDGP_LIB_PATH=$PWD/tools/bin/libdsdgp_base.so python tools/collapsed_ab.py --package-root tools/bin/base/doubly-stochastic-dgp_amd \\
      --out /tmp/col_base.npz
  python tools/collapsed_ab.py --out /tmp/col_new.npz
  python tools/collapsed_ab.py --compare /tmp/col_base.npz /tmp/col_new.npz --md /tmp/col_ab.md      (the table of profiles/collapsed_refactor_ab.md)

The file holds every output of
  psi.<case>         kernel_expectations on every case of tests/psi_cases.py, and on `n601`
  psi_grad.<case>    kernel_expectations_grad on every case of tests/psi_grad_cases.NAMES, and on `n601`
                     (n601: n = 601, M = 5, D = 2, ARD, drawn the way psi_grad_cases.OWN draws — ten row splits and three chunks of
                     k_psig_z, the last one ragged; the test cases have n <= 200 and reach one chunk)
  sgpr.<case>        SGPR_Layer on every case of tests/collapsed_reference.NAMES: bound_terms, bound_gradients, conditional_ND without
                     and with full_cov
  kmeans / pca       kmeans_inducing (with labels, counts, inertia) and pca_map (with eigenvalues, mean, Gram matrix) on the smallest
                     case of tests/kmeans_cases.py / tests/pca_cases.py
`--compare` exits non-zero unless every array of the two files is equal (np.array_equal; NaNs in the same places count as equal)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N601 = (601, 5, 2, 1, 23)          # n, M, D, ARD, seed: a row of psi_grad_cases.OWN


def n601():
    from tests import psi_grad_cases as GC
    GC.OWN["n601"] = N601
    return GC.inputs("n601")


def collect():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Zero
    from doubly_stochastic_dgp.layer_initializations import kmeans_inducing, pca_map
    from doubly_stochastic_dgp.layers import SGPR_Layer, kernel_expectations, kernel_expectations_grad
    from tests import collapsed_reference as CR, kmeans_cases as KC, pca_cases as QC, psi_cases as PC, psi_grad_cases as GC
    out = {}
    kern = lambda c: RBF(c["mu"].shape[1], variance=c["variance"], lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]), ARD=c["ard"])
    for name, c in [(n, PC.inputs(n)) for n in PC.NAMES] + [("n601", n601())]:
        for k, v in zip(("psi0", "psi1", "psi2"), kernel_expectations(kern(c), c["Z"], c["mu"], c["s"])):
            out[f"psi.{name}.{k}"] = np.asarray(v)
    for name, c in [(n, GC.inputs(n)) for n in GC.NAMES] + [("n601", n601())]:
        for k, v in kernel_expectations_grad(kern(c), c["Z"], c["mu"], c["s"], c["g0"], c["g1"], c["g2"]).items():
            out[f"psi_grad.{name}.{k}"] = np.asarray(v)
    for name in CR.NAMES:
        c = CR.inputs(name)
        layer = SGPR_Layer(RBF(c["mu"].shape[1], variance=c["variance"], lengthscales=float(c["ls"][0])), c["Z"], c["Y"].shape[1], Zero())
        layer.set_data(c["mu"], c["s"], c["Y"], c["noise"])
        out[f"sgpr.{name}.bound"], out[f"sgpr.{name}.terms"] = (np.asarray(v) for v in layer.bound_terms())
        for k, v in layer.bound_gradients().items():
            out[f"sgpr.{name}.grad.{k}"] = np.asarray(v)
        for full_cov in (False, True):
            mean, var = layer.conditional_ND(c["Xs"], full_cov=full_cov)
            out[f"sgpr.{name}.mean{'.full' if full_cov else ''}"], out[f"sgpr.{name}.var{'.full' if full_cov else ''}"] = mean, var
    name = min(KC.CASES, key=lambda k: KC.CASES[k][0] * KC.CASES[k][1])
    X, idx, iters, _ = KC.inputs(name)
    Z, info = kmeans_inducing(X, len(idx), iter=iters, init=idx, return_info=True)
    out[f"kmeans.{name}.Z"] = Z
    for k, v in info.items():
        out[f"kmeans.{name}.{k}"] = np.asarray(v, dtype=np.float64)
    name = min(QC.CASES, key=lambda k: QC.CASES[k][0] * QC.CASES[k][1])
    X, k, center = QC.inputs(name)
    T, info = pca_map(X, k, center=center, return_info=True)
    out[f"pca.{name}.T"] = T
    for k in ("eigenvalues", "mean", "gram", "sweeps"):
        out[f"pca.{name}.{k}"] = np.asarray(info[k], dtype=np.float64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write this checkout's arrays to OUT.npz")
    ap.add_argument("--package-root", default=os.path.join(ROOT, "doubly-stochastic-dgp_amd"),
                    help="the directory that holds the doubly_stochastic_dgp package to import (another checkout's, for the base)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--md", default=None, help="with --compare: write the table here")
    args = ap.parse_args()
    if args.compare:
        from likelihood_ab import compare          # tools/ is the script's directory
        sys.exit(compare(*args.compare, args.md))
    sys.path[:0] = [ROOT, os.path.abspath(args.package_root)]
    arrays = collect()
    np.savez(args.out or "collapsed_ab.npz", **arrays)
    import doubly_stochastic_dgp
    print(f"{len(arrays)} arrays -> {args.out or 'collapsed_ab.npz'} (library: {os.environ.get('DSDGP_LIB_PATH', 'in-tree')}, "
          f"package: {os.path.dirname(doubly_stochastic_dgp.__file__)})")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The step-down map of init_layers_linear — the top k right singular vectors of X — three ways:

  device   layer_initializations.pca_map (csrc/pca.hip): Gram on the fp64 MFMA pipe + round-robin Jacobi, upload and download included
  svd      np.linalg.svd(X, full_matrices=False)[2][:k] on the host: what pca="host" (and the reference) runs
  eigh     np.linalg.eigh(X.T @ X) on the host: the same reduction to D x D with LAPACK behind it

at the MNIST shape 60 000 x 784 -> 30 and at 50 000 x 8 -> 4; X = N(0, 1) with columns scaled linspace(1, 3, D), fixed seed.

Method: pca_map once warm (code objects loaded, scratch grown), then `--reps` calls on the host clock (they end with a synchronisation);
medians with min .. max.  Inside one further call the library's own HIP events (dsdgp_prof_enable) time the Gram launch and the
eigensolver (norm + every step launch + the per-sweep check, the early-returning steps after convergence included).  The Gram
launch's rate is given twice: for the n D (D + 1) flops of the lower triangle it is asked for, and for the 2 n 64^2 flops of every
64 x 64 tile it issues (edge tiles are padded), each against the 78.6 TFLOP/s fp64 matrix peak.  The host routes: one run each, host
clock, with the threads numpy finds.  No speed is promised: the table records what was measured.
Usage: python tools/pca_ab.py [--reps 5] [--out profiles/pca_ab.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)
from doubly_stochastic_dgp.engine import Context  # noqa: E402
from doubly_stochastic_dgp.layer_initializations import pca_map  # noqa: E402

SHAPES = [("mnist", 60000, 784, 30), ("narrow", 50000, 8, 4)]
PEAK_TFLOPS = 78.6


def _projector_distance(A, B):
    return float(np.linalg.norm(A @ A.T - B @ B.T, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_ab.md"))
    args = ap.parse_args()
    if args.reps < 3:
        raise SystemExit("--reps: at least 3 repetitions")
    ctx = Context.get()
    lines = ["# Device PCA: pca_map against np.linalg.svd and np.linalg.eigh(X.T @ X) on the host", "",
             f"`pca_map ms`: median of {args.reps} calls (min .. max) after a warm-up, host clock, upload of X and download of T included.",
             "`gram ms`, `solver ms`: the library's HIP events inside one call.  `% of peak`: the Gram launch's n D (D + 1) useful flops,",
             f"and in brackets the 2 n 64^2 flops per tile it issues, against {PEAK_TFLOPS} TFLOP/s.  `svd ms`, `eigh ms`: one host run each.",
             "`|P - P_svd|`: spectral distance between the projectors on the k-dimensional subspaces of the device and of the host SVD.", "",
             "| shape | pca_map ms | gram ms | % of peak | solver ms | sweeps | svd ms | eigh ms | svd / pca_map | \\|P - P_svd\\| |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for tag, n, D, k in SHAPES:
        rng = np.random.default_rng(n + D + k)
        X = rng.standard_normal((n, D)) * np.linspace(1.0, 3.0, D)
        T, info = pca_map(X, k, return_info=True)
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pca_map(X, k)
            t.append(1e3 * (time.perf_counter() - t0))
        t = np.array(t)
        ctx.prof_enable(True)
        ctx.prof_read("pca_gram")
        ctx.prof_read("pca_eig")
        pca_map(X, k)
        gram_ms, _ = ctx.prof_read("pca_gram")
        eig_ms, _ = ctx.prof_read("pca_eig")
        ctx.prof_enable(False)
        tiles = -(-D // 64)
        useful = n * D * (D + 1.0)
        issued = tiles * (tiles + 1) / 2 * 2.0 * n * 64 * 64
        share = lambda flops: 100.0 * flops / (gram_ms * 1e-3) / (PEAK_TFLOPS * 1e12)
        print(f"{tag}: svd ...", flush=True)
        t0 = time.perf_counter()
        Vs = np.linalg.svd(X, full_matrices=False)[2][:k].T
        svd_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        np.linalg.eigh(X.T @ X)
        eigh_ms = 1e3 * (time.perf_counter() - t0)
        med = float(np.median(t))
        lines.append(f"| {tag} ({n} x {D} -> {k}) | {med:.1f} ({t.min():.1f} .. {t.max():.1f}) | {gram_ms:.3f} | {share(useful):.1f} "
                     f"({share(issued):.1f}) | {eig_ms:.1f} | {info['sweeps']} | {svd_ms:.0f} | {eigh_ms:.0f} | {svd_ms / med:.1f} | "
                     f"{_projector_distance(T, Vs):.2e} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

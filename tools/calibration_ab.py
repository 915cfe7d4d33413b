#!/usr/bin/env python
"""Calibration scores and predictive quantiles two ways on config 2's model (3 layers, M = 128, D = 8; synthetic kin8nm-shaped data):
10 000 test rows, S = 100, batches of 1000 rows — the settings of demos/run_regression.py:108-123.

  calibration        DGP_Base.calibration: forward pass + PIT / CRPS reduction on the device, one read-back of (2 + P) doubles per output
  calibration host   the predict_y loop (two (S, N*, D) arrays to the host per batch), then the numpy reference of
                     tests/calibration_reference.py (rows, sums, scores)
  quantiles          DGP_Base.predict_quantiles at probs = (0.025, 0.5, 0.975): forward pass + root finding on the device
  quantiles host     the predict_y loop, then the numpy solver of tests/calibration_reference.py
  forward            the forward pass alone (Engine.propagate, last layer's mean / var wanted), no host copies

Warm-up, then the variants interleaved within every repetition; the median of the repetitions is reported, with the launches per batch.
No speed is promised: the table records what was measured.
Usage: python tools/calibration_ab.py [--rows 10000] [--S 100] [--batch 1000] [--reps 5] [--out profiles/calibration_ab.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (synthetic data + Z recipe of the benchmark)
from doubly_stochastic_dgp.dgp import DGP  # noqa: E402
from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian  # noqa: E402
from tests import calibration_reference as R  # noqa: E402

CAL_PROBS = (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)
Q_PROBS = (0.025, 0.5, 0.975)


def host_components(model, Xs, S, batch):
    """the predict_y loop of run_regression.py:109-117 -> (mu, sg), each (S, N*, D)"""
    means, vars_ = [], []
    for a in range(0, len(Xs), batch):
        m, v = model.predict_y(Xs[a:a + batch], S)
        means.append(m)
        vars_.append(v)
    return np.concatenate(means, 1), R.sigma(np.concatenate(vars_, 1))


def host_calibration(model, Xs, Ys, S, batch):
    mu, sg = host_components(model, Xs, S, batch)
    return R.scores(R.sums(R.rows(Ys, mu, sg), CAL_PROBS), CAL_PROBS)


def host_quantiles(model, Xs, S, batch):
    mu, sg = host_components(model, Xs, S, batch)
    return R.quantiles(mu, sg, Q_PROBS)


def forward_only(model, Xd, S, batch):
    eng = model.engine()
    for a in range(0, Xd.shape[0], batch):
        eng.propagate(Xd[a:a + batch], S, seed=model._draw_seed(), want=("mean", "var"))
    eng.ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--S", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_ab.md"))
    args = ap.parse_args()
    X, Y = bench.make_synthetic(7372 + args.rows, 8, seed=0)
    Xs, Ys, X, Y = X[7372:], Y[7372:], X[:7372], Y[:7372]
    Z = bench.default_Z(X, 128, seed=0)
    model = DGP(X, Y, Z, [RBF(8), RBF(8), RBF(8)], Gaussian(variance=0.1), num_samples=20, minibatch_size=1000)
    for layer in model.layers[:-1]:
        layer.q_sqrt = layer.q_sqrt.value * 1e-5
    eng = model.engine()
    ctx = eng.ctx
    Xd, Yd = ctx.to_device(Xs), ctx.to_device(Ys)
    variants = {
        "calibration": lambda: model.calibration(Xd, Yd, args.S, probs=CAL_PROBS, batch_size=args.batch),
        "calibration host": lambda: host_calibration(model, Xs, Ys, args.S, args.batch),
        "quantiles": lambda: model.predict_quantiles(Xd, args.S, probs=Q_PROBS, batch_size=args.batch),
        "quantiles host": lambda: host_quantiles(model, Xs, args.S, args.batch),
        "forward": lambda: forward_only(model, Xd, args.S, args.batch),
    }
    for fn in variants.values():      # warm-up: workspace for (batch, S), kernels loaded, scratch grown
        fn()
    nb = -(-args.rows // args.batch)
    launches = {}
    for name in ("calibration", "quantiles", "forward"):
        c0 = int(ctx.lib.dsdgp_launch_count())
        variants[name]()
        launches[name] = (int(ctx.lib.dsdgp_launch_count()) - c0) / nb
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    cal = model.calibration(Xd, Yd, args.S, probs=CAL_PROBS, batch_size=args.batch)
    lines = [f"# Calibration and quantiles, config 2's model: {args.rows} rows, S = {args.S}, batches of {args.batch}", "",
             f"median of {args.reps} interleaved repetitions after warm-up (min .. max), wall clock around the whole call incl. its one sync;",
             f"calibration at {len(CAL_PROBS)} probabilities, quantiles at {len(Q_PROBS)}", "",
             "| variant | ms | launches per batch |", "|---|---|---|"]
    for name in variants:
        t = 1e3 * np.array(times[name])
        lines.append(f"| {name} | {np.median(t):.2f} ({t.min():.2f} .. {t.max():.2f}) | {launches.get(name, '—')} |")
    med = {k: float(np.median(v)) for k, v in times.items()}
    pairs = args.S * (args.S - 1) // 2
    lines += ["", f"calibration / host = {med['calibration'] / med['calibration host']:.4f}; quantiles / host = "
              f"{med['quantiles'] / med['quantiles host']:.4f}",
              f"calibration - forward = {1e3 * (med['calibration'] - med['forward']):.2f} ms over {nb} batches "
              f"({pairs} CRPS pair terms per item, {args.batch * pairs / 1e6:.2f} M per batch); "
              f"quantiles - forward = {1e3 * (med['quantiles'] - med['forward']):.2f} ms",
              f"scores of the last call: crps {cal['crps']:.6f}, coverage "
              + ", ".join(f"{k:.2f}: {v:.4f}" for k, v in sorted(cal["coverage"].items()))]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

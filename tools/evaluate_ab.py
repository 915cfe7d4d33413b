#!/usr/bin/env python
"""Held-out evaluation three ways on config 2's model (3 layers, M = 128, D = 8; synthetic kin8nm-shaped data): 10 000 test rows, S = 100,
batches of 1000 rows, as demos/run_regression.py:108-123 evaluates every 100 iterations.

  evaluate   DGP_Base.evaluate: forward pass + mixture reduction on the device, one read-back of 3 doubles per output
  parent     the predict_y loop of run_regression.py with its numpy reduction (two (S, N*, D) arrays to the host per batch)
  forward    the forward pass alone (Engine.propagate, last layer's mean / var wanted), no host copies

Warm-up, then the variants interleaved within every repetition; the median of the repetitions is reported, with the launches per batch
and (--prof) the per-class HIP-event times of one evaluate call on a single stream (run with DSDGP_NO_OVERLAP=1).
Usage: python tools/evaluate_ab.py [--rows 10000] [--S 100] [--batch 1000] [--reps 20] [--prof] [--out FILE.md]"""
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


def parent_path(model, Xs, Ys, S, batch, Y_std=1.0):
    """demos/run_regression.py:109-123"""
    from scipy.special import logsumexp
    from scipy.stats import norm
    means, vars_ = [], []
    for a in range(0, len(Xs), batch):
        m, v = model.predict_y(Xs[a:a + batch], S)
        means.append(m)
        vars_.append(v)
    mean_SND, var_SND = np.concatenate(means, 1), np.concatenate(vars_, 1)
    mean_ND = np.average(mean_SND, 0)
    err = np.average(Y_std * np.mean((Ys - mean_ND) ** 2.0) ** 0.5)
    nll = logsumexp(norm.logpdf(Ys * Y_std, mean_SND * Y_std, var_SND ** 0.5 * Y_std), 0, b=1 / float(S))
    return err, np.average(nll)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--out", default=None)
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
        "evaluate": lambda: model.evaluate(Xd, Yd, args.S, batch_size=args.batch),
        "parent": lambda: parent_path(model, Xs, Ys, args.S, args.batch),
        "forward": lambda: forward_only(model, Xd, args.S, args.batch),
    }
    for fn in variants.values():      # warm-up: workspace for (batch, S), kernels loaded, scratch grown
        fn(); fn()
    nb = -(-args.rows // args.batch)
    launches = {}
    for name in ("evaluate", "forward"):
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
    ev = model.evaluate(Xd, Yd, args.S, batch_size=args.batch)
    lines = [f"# Held-out evaluation, config 2's model: {args.rows} rows, S = {args.S}, batches of {args.batch}", "",
             f"median of {args.reps} interleaved repetitions after warm-up (min .. max), wall clock around the whole call incl. its one sync", "",
             "| variant | ms | launches per batch |", "|---|---|---|"]
    for name in variants:
        t = 1e3 * np.array(times[name])
        lines.append(f"| {name} | {np.median(t):.2f} ({t.min():.2f} .. {t.max():.2f}) | {launches.get(name, '—')} |")
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines += ["", f"evaluate / parent = {med['evaluate'] / med['parent']:.3f}; evaluate - forward = "
              f"{1e3 * (med['evaluate'] - med['forward']):.2f} ms over {nb} batches "
              f"(the reduction reads 2 S n DY doubles = {2 * args.S * args.batch * 8 / 1e6:.1f} MB per batch)",
              f"scores of the last call: rmse {ev['rmse']:.6f}, log density {ev['log_density']:.6f}"]
    if args.prof:
        ctx.prof_enable(True)
        model.evaluate(Xd, Yd, args.S, batch_size=args.batch)
        lines += ["", f"HIP-event times of one evaluate call per kernel class (DSDGP_NO_OVERLAP={os.environ.get('DSDGP_NO_OVERLAP', '0')}):", "",
                  "| class | ms | brackets |", "|---|---|---|"]
        for cls in ("gram", "potrf", "gemm", "layer_fwd", "evaluate"):
            ms, cnt = ctx.prof_read(cls)
            lines.append(f"| {cls} | {ms:.3f} | {cnt} |")
        ctx.prof_enable(False)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

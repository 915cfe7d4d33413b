#!/usr/bin/env python
"""One gradient evaluation of a DGP_Collapsed through all its layers (compute_log_likelihood_gradients(inner=True)), timed per stage:

  propagate          the inner layers' forward-only pass whose statistics the bound is evaluated on (S = 1, the whole training set)
  set_data           the kernel expectations and the two factorisations of the collapsed layer (SGPR_Layer.set_data)
  forward_saved      dsdgp_model_forward_saved on the inner layers' engine: the same layers on the same draws, keeping what the
                     reverse pass reads
  bound_gradients    the adjoints of the bound and the reverse pass of the expectations (SGPR_Layer.bound_gradients, on the device)
  backward_adjoints  dsdgp_model_backward_adjoints seeded with the adjoints of the last layer's input mean and variance

at N = 40 000, M = 128, D = 8 with two inner layers (8 -> 8 -> 8, RBF; the collapsed layer RBF on 8 inputs, one output), and next to
them dsdgp_model_elbo(with_grad = 1) of the SAME inner engine on the same rows at S = 1: what the two new calls add over a plain
gradient evaluation (which also runs a likelihood, so the comparison flatters the pair by one launch).

Method: everything once warm, then `--reps` repetitions of the sequence; each stage between a pair of HIP events on the library's
stream; medians with min .. max.  No speed is promised: the table records what was measured.
Usage: python tools/collapsed_train_ab.py [--reps 7] [--out profiles/collapsed_train.md]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)

N, M, D = 40000, 128, 8
STAGES = ("propagate", "set_data", "forward_saved", "bound_gradients", "backward_adjoints")


def build():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, 1))) + 0.1 * rng.standard_normal((N, 1))
    Z = X[rng.permutation(N)[:M]].copy()
    dgp = DGP(X, Y, Z, [RBF(D, lengthscales=np.sqrt(D)) for _ in range(3)], Gaussian(variance=0.1), num_samples=1)
    return DGP_Collapsed.from_dgp(dgp), rng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collapsed_train.md"))
    args = ap.parse_args()
    model, rng = build()
    eng, top = model.inner_engine(), model.layers[-1]
    torch = eng.ctx.torch
    Xd, Yd = model._device_data()
    zs = [eng.ctx.to_device(rng.standard_normal((1, N, D))) for _ in range(2)]
    s2 = float(model.likelihood.likelihood.variance.value)
    Y8 = eng.ctx.to_device(np.tile(model.Y_data, (1, D)))          # targets of the inner engine's own Gaussian likelihood (8 outputs)

    def once():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        _, ms, vs = eng.propagate(Xd, 1, zs=zs, want=("mean", "var"))
        ev[1].record()
        top.set_data(ms[-1][0], vs[-1][0], Yd, s2)
        ev[2].record()
        eng.forward_saved(Xd, 1, zs=zs)
        ev[3].record()
        g = top.bound_gradients(on_device=True)
        ev[4].record()
        eng.backward_adjoints(g["X_mean"][None], g["X_var"][None], sync=False)
        ev[5].record()
        eng.ctx.sync()
        ev[6].record()
        eng.elbo(Xd, Y8, 1, zs=zs, with_grad=True, sync=False)
        ev[7].record()
        eng.ctx.sync()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(5)] + [ev[6].elapsed_time(ev[7])]

    once()
    t = np.array([once() for _ in range(args.reps)])
    med, lo, hi = np.median(t, 0), t.min(0), t.max(0)
    cell = lambda i: f"{med[i]:.2f} ({lo[i]:.2f} .. {hi[i]:.2f})"
    total = float(np.median(t[:, :5].sum(1)))
    lines = ["# One gradient evaluation of a collapsed model through all layers, per stage", "",
             f"N = {N}, M = {M}, D = {D}, two inner layers, S = 1; median of {args.reps} repetitions (min .. max) after a warm-up, HIP events,",
             "data resident.  `elbo(with_grad)`: dsdgp_model_elbo(with_grad = 1) of the same inner engine on the same rows — a plain",
             "gradient evaluation, likelihood included; `pair / elbo` is forward_saved + backward_adjoints over it.", "",
             "| stage | ms |", "|---|---|"]
    lines += [f"| {name} | {cell(i)} |" for i, name in enumerate(STAGES)]
    lines += [f"| all five | {total:.2f} |", f"| elbo(with_grad) | {cell(5)} |", f"| pair / elbo | {(med[2] + med[4]) / med[5]:.2f} |", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

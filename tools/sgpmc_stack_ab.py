#!/usr/bin/env python
"""One log-density + gradient evaluation of a DGP_SGPMC at the benchmark shape — 3 layers, M = 128, S = 20, minibatch 1000, D = 8 —
stage by stage (the library's own event brackets: the passes over A of the sparse conditional, the hops, the head), beside
  1. one training step of the SVGP engine (DGP.train_step: ELBO, gradient and Adam in one call) on the same shape — the engine and its
     kernels are the parent commit's, untouched by the stack — and
  2. torch autograd of the same stack (same kernels, factorisations, hops, Gaussian expectation) on the same device,
and a sanity run: on a one-layer Gaussian model the SGHMC sample mean of the whitened q_mu against the closed-form posterior mean
(reported, not asserted).

    python tools/sgpmc_stack_ab.py --out profiles/sgpmc_stack_ab.md

Every time is device time between two events on the library's stream after `--warmup` evaluations; the routes alternate within a
repetition; the table gives the median and the spread (min .. max) over `--reps` repetitions.  No ratio is fixed in advance: the file
states what was measured, and "not measured" where a route did not run."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "doubly-stochastic-dgp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

L, M, D, S, NB, N = 3, 128, 8, 20, 1000, 8000
SCOPES = ("gram", "potrf", "sparse_cond_fwd", "sparse_cond_adj", "gemm", "gram_grad", "stack_hop", "stack_hop_bwd", "stack_head")


def torch_stack(torch, params, X, Y, zs, jitter, s2, scale):
    Xin, prior, n_layers = X, 0.0, len(params)
    for l, (Z, q, var, ls) in enumerate(params):
        def K(A, B):
            u = (A[:, None, :] - B[None, :, :]) / ls
            return var * torch.exp(-0.5 * (u * u).sum(-1))
        Lu = torch.linalg.cholesky(K(Z, Z) + jitter * torch.eye(Z.shape[0], dtype=Z.dtype, device=Z.device))
        A = torch.linalg.solve_triangular(Lu, K(Z, Xin), upper=False)
        mean, v = A.T @ q, var - (A * A).sum(0)
        if l + 1 < n_layers:
            mean = mean + Xin
            Xin = mean + zs[l] * torch.sqrt(v + jitter)[:, None]
        prior = prior - 0.5 * (q * q).sum() - 0.5 * q.numel() * np.log(2.0 * np.pi)
    ve = -0.5 * np.log(2.0 * np.pi) - 0.5 * np.log(s2) - 0.5 * ((Y - mean) ** 2 + v[:, None]) / s2
    return scale * ve.sum() + prior


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sghmc", type=int, default=400, help="iterations of the sanity run (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from doubly_stochastic_dgp import settings, training
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.engine import Context
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Identity, Zero
    from doubly_stochastic_dgp.layers import SGPMC_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_SGPMC
    ctx = Context.get()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.tstream)
        out = fn()
        e1.record(ctx.tstream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out                    # us

    rng = np.random.default_rng(0)
    Xh = rng.standard_normal((N, D))
    Yh = np.sin(Xh[:, :1]) + 0.1 * rng.standard_normal((N, 1))
    Zh = Xh[:M].copy()
    kern = lambda: RBF(D, variance=1.0, lengthscales=float(np.sqrt(D)))
    layers = [SGPMC_Layer(kern(), Zh, D, Identity(), white=True) for _ in range(L - 1)] + [SGPMC_Layer(kern(), Zh, 1, Zero(), white=True)]
    for layer in layers:
        layer.q_mu = 0.3 * rng.standard_normal(layer.q_mu.shape)
    model = DGP_SGPMC(Xh, Yh, Gaussian(0.1), layers, minibatch_size=NB, num_samples=S)
    engine_model = DGP(Xh, Yh, Zh, [kern() for _ in range(L)], Gaussian(0.1), white=True, minibatch_size=NB, num_samples=S)
    Xb, Yb = ctx.to_device(Xh[:NB]), ctx.to_device(Yh[:NB])
    zs_h = [rng.standard_normal((S, NB, D)) for _ in range(L - 1)]
    zs_t = [ctx.to_device(z.reshape(S * NB, D)) for z in zs_h]
    Xt = Xb.repeat(S, 1)
    Yt = Yb.repeat(S, 1)

    zs3 = [z.reshape(S, NB, D) for z in zs_t]

    def ours():
        return model.log_density_device(Xb, Yb, zs=zs3, with_grad=True)

    def ours_value():
        return model.log_density_device(Xb, Yb, zs=zs3, with_grad=False)

    def engine_step():
        engine_model.train_step(0.01)

    def torch_route():
        params = []
        for layer in layers:
            Z, q = ctx.to_device(layer.feature.Z.value).requires_grad_(True), ctx.to_device(layer.q_mu.value).requires_grad_(True)
            var = torch.tensor(1.0, dtype=torch.float64, device=Xb.device, requires_grad=True)
            ls = torch.tensor(float(np.sqrt(D)), dtype=torch.float64, device=Xb.device, requires_grad=True)
            params.append((Z, q, var, ls))
        value = torch_stack(torch, params, Xt, Yt, zs_t, settings.jitter, 0.1, float(N) / NB / S)
        value.backward()
        return value.detach(), [p[1].grad for p in params], [p[0].grad for p in params]

    for _ in range(a.warmup):
        ours(); ours_value(); engine_step(); torch_route()
    ctx.sync()
    t = {k: [] for k in ("ours", "ours_value", "engine", "torch")}
    for _ in range(a.reps):
        us, res = timed(ours)
        t["ours"].append(us)
        t["ours_value"].append(timed(ours_value)[0])
        t["engine"].append(timed(engine_step)[0])
        us, ref = timed(torch_route)
        t["torch"].append(us)
    ctx.sync()
    # agreement of the two routes
    out4, grad = res
    pairs = model.split_gradient(grad.cpu().numpy())
    rel = lambda x, y: float(np.max(np.abs(x - y)) / np.max(np.abs(y)))
    agree = [("value", abs(float(out4.cpu().numpy()[0]) - float(ref[0])) / abs(float(ref[0])))]
    for l in range(L):
        agree.append(("layer %d d_q_mu" % l, rel(pairs[4 * l + 1][1], ref[1][l].cpu().numpy())))
        agree.append(("layer %d d_Z" % l, rel(pairs[4 * l][1], ref[2][l].cpu().numpy())))
    # stage by stage: the library's own event brackets around one evaluation
    ctx.prof_enable(True)
    for _ in range(a.reps):
        ours()
    ctx.sync()
    stages = {}
    for name in SCOPES:
        ms, cnt = ctx.prof_read(name)
        stages[name] = (ms * 1e3 / a.reps, cnt / a.reps)
    ctx.prof_enable(False)

    sanity = None
    if a.sghmc > 0:
        n1, M1 = 400, 16
        X1 = rng.standard_normal((n1, 1))
        Y1 = np.sin(2.0 * X1) + 0.2 * rng.standard_normal((n1, 1))
        Z1 = np.linspace(-2.5, 2.5, M1)[:, None]
        one = SGPMC_Layer(RBF(1, variance=1.0, lengthscales=0.8), Z1, 1, Zero(), white=True)
        m1 = DGP_SGPMC(X1, Y1, Gaussian(0.04), [one], minibatch_size=100, num_samples=1)
        u = (Z1[:, None, :] - Z1[None, :, :]) / 0.8
        Lu = np.linalg.cholesky(np.exp(-0.5 * (u * u).sum(-1)) + settings.jitter * np.eye(M1))
        u = (Z1[:, None, :] - X1[None, :, :]) / 0.8
        A = np.linalg.solve(Lu, np.exp(-0.5 * (u * u).sum(-1)))
        post = np.linalg.solve(np.eye(M1) + A @ A.T / 0.04, A @ Y1 / 0.04)          # mean of p(q_mu | Y): the variance term has no q_mu
        run = training.SGHMC(2e-5, 0.1).sample(m1, a.sghmc // 2, burn=a.sghmc // 2, seed=0)
        mean = run["samples"]["q_mu0"].mean(0)
        sanity = (a.sghmc, float(np.linalg.norm(post)), float(np.linalg.norm(mean - post)), float(np.linalg.norm(run["samples"]["q_mu0"][-1] - post)))

    fmt = lambda x: "%.0f (%.0f .. %.0f)" % (float(np.median(x)), float(np.min(x)), float(np.max(x)))
    med = lambda k: float(np.median(t[k]))
    lines = ["# DGP_SGPMC: one log-density + gradient evaluation at the benchmark shape (tools/sgpmc_stack_ab.py)\n",
             "%d layers, M = %d, S = %d, minibatch %d, D = %d (inner layers %d -> %d with an Identity mean, the last %d -> 1), RBF, white=True,"
             " Gaussian likelihood.  Device time in microseconds between two events on the library's stream, median (min .. max) of %d"
             " repetitions after %d warm-up evaluations; the host work between the launches of a route is inside its bracket.\n"
             % (L, M, S, NB, D, D, D, D, a.reps, a.warmup),
             "| route | one evaluation |", "|---|---|",
             "| DGP_SGPMC: dsdgp_stack_logdensity, value and gradient | %s |" % fmt(t["ours"]),
             "| DGP_SGPMC: dsdgp_stack_logdensity, value only | %s |" % fmt(t["ours_value"]),
             "| SVGP engine (DGP.train_step: ELBO, gradient and Adam), same shape; the parent commit's code, unchanged here | %s |" % fmt(t["engine"]),
             "| torch autograd of the same stack, same device | %s |" % fmt(t["torch"]),
             "", "stack / engine: %.2f;  torch / stack: %.2f.\n" % (med("ours") / med("engine"), med("torch") / med("ours")),
             "The stack runs every layer on all S n rows through dsdgp_sparse_conditional and, in the reverse, through"
             " dsdgp_sparse_conditional_grad, which repeats the layer's factorisation and solves; each of those calls reads its Cholesky"
             " status on the host, so one evaluation synchronises %d times.  The first layer's inputs are the minibatch repeated S times:"
             " its conditional is computed S times over.\n" % (3 * L),
             "Stages of one evaluation with a gradient (the library's event brackets, mean per evaluation; brackets nest — `gram`, `potrf`"
             " and `gemm` run inside the conditional's calls — so the lines do not add up to the total):\n",
             "| bracket | us per evaluation | launches per evaluation |", "|---|---|---|"]
    for name in SCOPES:
        lines.append("| %s | %.0f | %.1f |" % (name, stages[name][0], stages[name][1]))
    lines += ["", "Agreement of the two routes (relative difference, max over the entries):\n", "| quantity | relative difference |", "|---|---|"]
    lines += ["| %s | %.2g |" % kv for kv in agree]
    lines += ["", "## Sanity run: SGHMC on a one-layer Gaussian model\n"]
    if sanity is None:
        lines.append("not measured")
    else:
        lines.append("n = 400, M = 16, minibatch 100, learning rate 2e-5, friction 0.1, %d iterations, the first half discarded.  The posterior"
                     " of the whitened q_mu is Gaussian with mean (I + A A^T / s2)^-1 A Y / s2; its norm is %.3f.  Distance of the SGHMC sample"
                     " mean from it: %.3f; of the last state: %.3f; of the starting point (q_mu = 0): %.3f.  Reported, not asserted."
                     % (sanity[0], sanity[1], sanity[2], sanity[3], sanity[1]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

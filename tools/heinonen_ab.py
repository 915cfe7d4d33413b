#!/usr/bin/env python
"""One log-density + gradient evaluation of the dense collapsed layer (layers.GPR_Layer: the hot path of DGP_Heinonen under HMC) at
N = 512, 1024, 2048, D = 3, DY = 1, Matern52, stage by stage — gram, potrf, inverse (dsdgp_trsm of the identity + dsdgp_gemm),
gram_grad (with the dsdgp_gemm that forms dF/dK), bound — against torch autograd on the same device through torch.linalg.cholesky, and
dsdgp_gram_grad alone against autograd of a torch Gram matrix.

    python tools/heinonen_ab.py --out profiles/heinonen_ab.md

Every time is device time between two events on the library's stream, after `--warmup` evaluations of the same shape; the two routes
alternate within a repetition, and the table gives the median and the spread (min .. max) over `--reps` repetitions.  No ratio is fixed
in advance: the file states what was measured."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "doubly-stochastic-dgp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

D, DY, LS, VAR, NOISE = 3, 1, 0.7, 1.2, 0.1
STAGES = ("gram", "potrf", "solve", "inverse", "gram_grad", "bound")


def torch_gram(torch, X, ls, var):
    u = (X[:, None, :] - X[None, :, :]) / ls
    r = torch.sqrt((u * u).sum(-1) + 1e-12)
    s5 = 5.0 ** 0.5
    return var * (1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * torch.exp(-s5 * r)


def torch_logp(torch, X, Y, ls, var, noise):
    n = X.shape[0]
    L = torch.linalg.cholesky(torch_gram(torch, X, ls, var) + noise * torch.eye(n, dtype=X.dtype, device=X.device))
    V = torch.linalg.solve_triangular(L, Y, upper=False)
    return -0.5 * n * Y.shape[1] * np.log(2.0 * np.pi) - Y.shape[1] * torch.log(torch.diagonal(L)).sum() - 0.5 * (V * V).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from doubly_stochastic_dgp.engine import Context
    from doubly_stochastic_dgp.gpflow_compat import Matern52
    from doubly_stochastic_dgp.layers import _kernel_spec
    ctx = Context.get()
    kern = Matern52(D, variance=VAR, lengthscales=LS)
    spec, keep = _kernel_spec(kern)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.tstream)
        out = fn()
        e1.record(ctx.tstream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out                    # us

    rows, checks = [], []
    for n in (int(s) for s in a.sizes.split(",")):
        rng = np.random.default_rng(n)
        Xh, Yh = rng.uniform(size=(n, D)) * (n / 64.0) ** (1.0 / D), rng.standard_normal((n, DY))
        X, Y = ctx.to_device(Xh), ctx.to_device(Yh)
        eye0 = torch.zeros(n, n, dtype=torch.float64, device=X.device)
        K, V, alpha, Li, dK = ctx.empty(n, n), ctx.empty(n, DY), ctx.empty(n, DY), ctx.empty(n, n), ctx.empty(n, n)
        d_X, d_k, bound = ctx.empty(n, D), ctx.empty(3), ctx.empty(4)
        Gfix = ctx.to_device(rng.standard_normal((n, n)))

        def stage_gram():
            ctx.gram(spec, X, None, NOISE, K)

        def stage_potrf():
            ctx.potrf(K)

        def stage_solve():
            V.copy_(Y)
            ctx.trsm(K, V)
            alpha.copy_(V)
            ctx.trsm(K, alpha, trans=1)

        def stage_inverse():
            ctx.scale_copy(eye0, Li, diag_add=1.0)
            ctx.trsm(K, Li)
            ctx.gemm(1, 0, 1.0, Li, Li, 0.0, dK)

        def stage_gram_grad():
            ctx.gemm(0, 1, 0.5, alpha, alpha, -0.5 * DY, dK)
            ctx.gram_grad(spec, X, None, dK, d_X, None, d_k)

        def stage_bound():
            ctx.gpr_bound(K, V, bound)

        stages = dict(gram=stage_gram, potrf=stage_potrf, solve=stage_solve, inverse=stage_inverse, gram_grad=stage_gram_grad,
                      bound=stage_bound)

        def ours_all():
            for s in STAGES:
                stages[s]()

        def torch_all():
            Xt = X.detach().clone().requires_grad_(True)
            ls = torch.tensor(LS, dtype=torch.float64, device=X.device, requires_grad=True)
            var = torch.tensor(VAR, dtype=torch.float64, device=X.device, requires_grad=True)
            noise = torch.tensor(NOISE, dtype=torch.float64, device=X.device, requires_grad=True)
            f = torch_logp(torch, Xt, Y, ls, var, noise)
            f.backward()
            return f.detach(), Xt.grad, ls.grad, var.grad, noise.grad

        def ours_gg():
            ctx.gram_grad(spec, X, None, Gfix, d_X, None, d_k)

        def torch_gg():
            Xt = X.detach().clone().requires_grad_(True)
            ls = torch.tensor(LS, dtype=torch.float64, device=X.device, requires_grad=True)
            var = torch.tensor(VAR, dtype=torch.float64, device=X.device, requires_grad=True)
            (Gfix * torch_gram(torch, Xt, ls, var)).sum().backward()
            return Xt.grad, ls.grad, var.grad

        for _ in range(a.warmup):
            ours_all(); torch_all(); ours_gg(); torch_gg()
        ctx.sync()
        t = {k: [] for k in STAGES + ("ours", "torch", "gg_ours", "gg_torch")}
        for _ in range(a.reps):
            for s in STAGES:
                t[s].append(timed(stages[s])[0])
            t["ours"].append(timed(ours_all)[0])
            us, ref = timed(torch_all)
            t["torch"].append(us)
            t["gg_ours"].append(timed(ours_gg)[0])
            t["gg_torch"].append(timed(torch_gg)[0])
        # the two routes compute the same thing
        ours_all()
        ctx.sync()
        f, gX, gl, gv, gn = (x.cpu().numpy() for x in ref)
        k = d_k.cpu().numpy()
        rel = lambda x, y: float(np.max(np.abs(x - y)) / np.max(np.abs(y)))
        checks.append((n, abs(float(bound.cpu().numpy()[0]) - float(f)) / abs(float(f)), rel(d_X.cpu().numpy(), gX), abs(k[0] - gv) / abs(gv),
                       abs(k[1] - gl) / abs(gl), abs(k[2] - gn) / abs(gn)))
        rows.append((n, {k_: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k_, v in t.items()}))
        print(n, {k_: "%.1f" % np.median(v) for k_, v in t.items()}, flush=True)

    lines = ["# Dense collapsed layer: one log-density + gradient evaluation, stage by stage (tools/heinonen_ab.py)\n",
             "D = %d, DY = %d, Matern52, noise variance %g; device time in microseconds between two events on the library's stream, median"
             " (min .. max) of %d repetitions after %d warm-up evaluations; the routes alternate within a repetition.  `solve` is the two"
             " triangular solves for V and alpha; `inverse` is dsdgp_trsm of the identity and the dsdgp_gemm for K^-1; `gram_grad` includes the"
             " dsdgp_gemm that forms dF/dK.  `torch` is autograd of the same log density through torch.linalg.cholesky on the same device"
             " (forward and backward).\n" % (D, DY, NOISE, a.reps, a.warmup),
             "| N | " + " | ".join(STAGES) + " | all stages, one window | torch autograd | torch / ours |", "|---|" + "---|" * (len(STAGES) + 3)]
    fmt = lambda m: "%.1f (%.1f .. %.1f)" % m
    for n, t in rows:
        lines.append("| %d | " % n + " | ".join(fmt(t[s]) for s in STAGES) + " | %s | %s | %.2f |" % (fmt(t["ours"]), fmt(t["torch"]),
                                                                                                   t["torch"][0] / t["ours"][0]))
    lines += ["", "dsdgp_gram_grad alone (symmetric form, every output, a fixed standard-normal G) against autograd of a torch Gram matrix"
              " (forward and backward of sum(G * K)):\n", "| N | dsdgp_gram_grad | torch autograd | torch / ours |", "|---|---|---|---|"]
    for n, t in rows:
        lines.append("| %d | %s | %s | %.2f |" % (n, fmt(t["gg_ours"]), fmt(t["gg_torch"]), t["gg_torch"][0] / t["gg_ours"][0]))
    lines += ["", "Agreement of the two routes (relative difference: bound, max over d_X, d_variance, d_lengthscale, d_noise):\n",
              "| N | bound | d_X | d_variance | d_lengthscale | d_noise |", "|---|---|---|---|---|---|"]
    for c in checks:
        lines.append("| %d | %.2g | %.2g | %.2g | %.2g | %.2g |" % c)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

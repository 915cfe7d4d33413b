#!/usr/bin/env python
"""One log-density + gradient evaluation of a DGP_Collapsed over an SGPMC_Layer, stage by stage — the layer's conditional
(dsdgp_sparse_conditional), the top layer's set_data, its bound_gradients, the layer's conditional_vjp
(dsdgp_sparse_conditional_grad) — and the conditional + its reverse pass alone against torch autograd of the same conditional on the
same device.  Two shapes: N = 40 000, M = 128, D = 8 under an SGPR_Layer, and N = 2048 under a GPR_Layer (beside DGP_Heinonen at the
same N: tools/heinonen_ab.py, profiles/heinonen_ab.md).

    python tools/sgpmc_ab.py --out profiles/sgpmc_ab.md

Every time is device time between two events on the library's stream, after `--warmup` evaluations of the same shape; the routes
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

M, D, DY = 128, 8, 1
STAGES = ("conditional", "set_data", "bound_gradients", "conditional_vjp")


def torch_conditional(torch, Z, X, q, ls, var, jitter):
    def K(A, B):
        u = (A[:, None, :] - B[None, :, :]) / ls
        return var * torch.exp(-0.5 * (u * u).sum(-1))
    Lu = torch.linalg.cholesky(K(Z, Z) + jitter * torch.eye(Z.shape[0], dtype=Z.dtype, device=Z.device))
    A = torch.linalg.solve_triangular(Lu, K(Z, X), upper=False)
    return A.T @ q, var - (A * A).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="40000:sgpr,2048:gpr")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.engine import Context
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Zero
    from doubly_stochastic_dgp.layers import GPR_Layer, SGPMC_Layer, SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    ctx = Context.get()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.tstream)
        out = fn()
        e1.record(ctx.tstream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out                    # us

    rows, checks = [], []
    for shape in a.shapes.split(","):
        n, top_kind = int(shape.split(":")[0]), shape.split(":")[1]
        rng = np.random.default_rng(n)
        Xh = rng.standard_normal((n, D))
        Yh = np.sin(Xh[:, :1]) + 0.1 * rng.standard_normal((n, DY))
        low = SGPMC_Layer(RBF(D, variance=1.0, lengthscales=np.sqrt(D)), Xh[:M].copy(), D, Zero(), white=True)
        low.q_mu = 0.5 * rng.standard_normal((M, D))
        top = SGPR_Layer(RBF(D, variance=1.0, lengthscales=np.sqrt(D)), Xh[M:2 * M].copy(), DY, Zero()) if top_kind == "sgpr" else \
            GPR_Layer(RBF(D, variance=1.0, lengthscales=np.sqrt(D)), Zero(), DY)
        model = DGP_Collapsed(Xh, Yh, Gaussian(variance=0.1), [low, top])
        Xd, Yd = model._device_data()
        state = {}

        def stage_conditional():
            state["mean"], state["var"] = low.conditional_device(Xd)

        def stage_set_data():
            top.set_data(state["mean"], state["var"][:, None].expand(-1, D).contiguous(), Yd, 0.1)

        def stage_bound_gradients():
            state["g"] = top.bound_gradients(on_device=True)

        def stage_vjp():
            state["v"] = low.conditional_vjp(state["g"]["X_mean"], state["g"]["X_var"], X=Xd, on_device=True)

        stages = dict(conditional=stage_conditional, set_data=stage_set_data, bound_gradients=stage_bound_gradients, conditional_vjp=stage_vjp)

        def ours_all():
            return model.compute_log_density_gradients()

        def ours_pair():
            stage_conditional()
            stage_vjp()

        Zt0, qt0 = ctx.to_device(low.feature.Z.value), ctx.to_device(low.q_mu.value)

        def torch_pair():
            Zt, Xt, qt = (t.detach().clone().requires_grad_(True) for t in (Zt0, Xd, qt0))
            ls = torch.tensor(np.sqrt(D), dtype=torch.float64, device=Xd.device, requires_grad=True)
            var = torch.tensor(1.0, dtype=torch.float64, device=Xd.device, requires_grad=True)
            mean, v = torch_conditional(torch, Zt, Xt, qt, ls, var, settings.jitter)
            ((state["g"]["X_mean"] * mean).sum() + (state["g"]["X_var"].sum(1) * v).sum()).backward()
            return qt.grad, Zt.grad, Xt.grad, var.grad, ls.grad

        for s in STAGES:
            stages[s]()
        for _ in range(a.warmup):
            ours_all(); ours_pair(); torch_pair()
        ctx.sync()
        t = {k: [] for k in STAGES + ("ours", "pair_ours", "pair_torch")}
        for _ in range(a.reps):
            for s in STAGES:
                t[s].append(timed(stages[s])[0])
            t["ours"].append(timed(ours_all)[0])
            t["pair_ours"].append(timed(ours_pair)[0])
            us, ref = timed(torch_pair)
            t["pair_torch"].append(us)
        ctx.sync()
        v = {k: x.cpu().numpy() for k, x in state["v"].items()}
        gq, gZ, gX, gvar, gls = (x.cpu().numpy() for x in ref)
        rel = lambda x, y: float(np.max(np.abs(x - y)) / np.max(np.abs(y)))
        checks.append((n, top_kind, rel(v["q_mu"], gq), rel(v["Z"], gZ), rel(v["X"], gX), rel(v["variance"], gvar), rel(v["lengthscales"], gls)))
        rows.append((n, top_kind, {k_: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k_, x in t.items()}))
        print(n, top_kind, {k_: "%.1f" % np.median(x) for k_, x in t.items()}, flush=True)

    fmt = lambda m: "%.1f (%.1f .. %.1f)" % m
    lines = ["# DGP_Collapsed over an SGPMC_Layer: one log-density + gradient evaluation, stage by stage (tools/sgpmc_ab.py)\n",
             "M = %d, D = %d, DY = %d, RBF, white=True; device time in microseconds between two events on the library's stream, median (min .."
             " max) of %d repetitions after %d warm-up evaluations.  `conditional` and `conditional_vjp` are the SGPMC layer's two calls"
             " (dsdgp_sparse_conditional, dsdgp_sparse_conditional_grad: the reverse repeats the forward's factorisation and solves);"
             " `set_data` and `bound_gradients` are the top layer's.  `whole evaluation` is compute_log_density_gradients(), host work and"
             " the read-back of the gradients included.\n" % (M, D, DY, a.reps, a.warmup),
             "| N | top layer | " + " | ".join(STAGES) + " | whole evaluation | conditional + vjp share |", "|---|---|" + "---|" * (len(STAGES) + 2)]
    for n, k, t in rows:
        share = (t["conditional"][0] + t["conditional_vjp"][0]) / t["ours"][0]
        lines.append("| %d | %s | " % (n, k) + " | ".join(fmt(t[s]) for s in STAGES) + " | %s | %.2f |" % (fmt(t["ours"]), share))
    lines += ["", "The conditional and its reverse pass alone against torch autograd of the same conditional on the same device (forward and"
              " backward, the top layer's adjoints as seeds):\n", "| N | ours | torch autograd | torch / ours |", "|---|---|---|---|"]
    for n, k, t in rows:
        lines.append("| %d | %s | %s | %.2f |" % (n, fmt(t["pair_ours"]), fmt(t["pair_torch"]), t["pair_torch"][0] / t["pair_ours"][0]))
    lines += ["", "Agreement of the two routes (relative difference, max over the entries):\n",
              "| N | top layer | d_q_mu | d_Z | d_X | d_variance | d_lengthscales |", "|---|---|---|---|---|---|---|"]
    for c in checks:
        lines.append("| %d | %s | %.2g | %.2g | %.2g | %.2g | %.2g |" % c)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Pathwise function draws (DGP_Base.sample_functions: dsdgp_pathwise_weights at draw time, dsdgp_pathwise_eval per layer and row batch)
against a torch route on the same device for the same draws — the same basis, weights and update vectors, the features cos / sin
(rows x L each) and K(X, Z) (rows x M) materialised — and against the joint draws of predict_all_layers_full_cov.

    python tools/pathwise_ab.py --out profiles/pathwise_ab.md

Benchmark-shaped stack: 3 layers, M = 128, D = 8, S = 20 functions, L = 1024 frequencies, N* = 100 000 rows in batches of 8192.  Every
device time is between two events on the library's stream, after `--warmup` evaluations; the routes alternate within a repetition, and
the table gives the median and the spread (min .. max) over `--reps` repetitions.  The joint draws run partly on the host, so their time
is wall-clock around a synchronised call.  No time is fixed in advance: the file states what was measured."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "doubly-stochastic-dgp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

M, D, DEPTH = 128, 8, 3


def torch_layer(torch, d, Xin, S):
    """layer d of the draws at Xin — (nb, D) or (S, nb, D) — through materialised features, (S, nb, DO)"""
    Om, c = d.Omega, d.origin
    Wc, Ws, V = d.Wc.view(S, d.L, d.DO), d.Ws.view(S, d.L, d.DO), d.V.view(S, d.M, d.DO)
    X3 = Xin if Xin.dim() == 3 else Xin[None].expand(S, -1, -1)
    th = (X3 - c) @ Om                                                   # (S, nb, L)
    f = (d.variance / d.L) ** 0.5 * (torch.bmm(torch.cos(th), Wc) + torch.bmm(torch.sin(th), Ws))
    ils = 1.0 / torch.as_tensor(np.broadcast_to(d.ls_host, (d.D,)).copy(), device=Om.device)
    u = (X3[:, :, None, :] - d.Z[None, None, :, :]) * ils                # (S, nb, M, D)
    r2 = (u * u).sum(-1)
    if d.kind == "rbf":
        K = d.variance * torch.exp(-0.5 * r2)
    else:
        r = torch.sqrt(r2 + 1e-12)
        K = d.variance * (1.0 + 5.0 ** 0.5 * r + 5.0 / 3.0 * r * r) * torch.exp(-(5.0 ** 0.5) * r)
    f = f + torch.bmm(K, V)
    if d.mean == "identity":
        f = f + X3
    elif d.mean == "linear":
        f = f + X3 @ d.A + d.b
    return f


def torch_route(torch, fs, X, batch):
    S, outs = fs.num_functions, []
    for i0 in range(0, X.shape[0], batch):
        F = X[i0:i0 + batch]
        for d in fs.layers:
            F = torch_layer(torch, d, F, S)
        outs.append(F)
    return torch.cat(outs, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--functions", type=int, default=20)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--torch-batch", type=int, default=2048, help="rows per batch of the torch route (its (S, nb, M, D) differences)")
    ap.add_argument("--joint-n", type=int, default=0, help="rows of the joint draws of predict_all_layers_full_cov (0: not measured)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.engine import Context
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    ctx = Context.get()
    rng = np.random.default_rng(0)
    n, S, L = a.rows, a.functions, a.features
    Xh = rng.standard_normal((max(n, 4 * M), D))
    Yh = np.sin(Xh[:, :1]) + 0.1 * rng.standard_normal((Xh.shape[0], 1))
    model = DGP(Xh[:4096], Yh[:4096], Xh[:M].copy(), [RBF(D, lengthscales=np.sqrt(D)) for _ in range(DEPTH)], Gaussian(variance=0.1),
                num_samples=S)
    for layer in model.layers:
        layer.q_mu = 0.5 * rng.standard_normal(layer.q_mu.shape)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.tstream)
        out = fn()
        e1.record(ctx.tstream)
        e1.synchronize()
        return e0.elapsed_time(e1), out                                  # ms

    t_draw, fs = timed(lambda: model.sample_functions(num_functions=S, num_features=L, seed=0))
    Xd = ctx.to_device(Xh[:n])
    ours = lambda: fs(Xd, batch_size=a.batch, on_device=True)
    theirs = lambda: torch_route(torch, fs, Xd, a.torch_batch)
    for _ in range(a.warmup):
        ours(); theirs()
    ctx.sync()
    t = {"ours": [], "torch": []}
    for _ in range(a.reps):
        ms, F = timed(ours)
        t["ours"].append(ms)
        ms, G = timed(theirs)
        t["torch"].append(ms)
    diff = float((F - G).abs().max().cpu())
    scale = float(G.abs().max().cpu())
    ctx.prof_enable(True)
    ours()
    prof_ms, launches = ctx.prof_read("pathwise")
    ctx.prof_enable(False)
    pairs = float(S) * n * L * DEPTH
    med = lambda x: (float(np.median(x)), float(np.min(x)), float(np.max(x)))
    fmt = lambda m: "%.1f (%.1f .. %.1f)" % m
    mo, mt = med(t["ours"]), med(t["torch"])
    lines = ["# Pathwise function draws against materialised features in torch and against joint draws (tools/pathwise_ab.py)\n",
             "%d layers, M = %d, D = %d, RBF, Identity / Zero means; S = %d functions, L = %d frequencies, N* = %d rows (ours in batches of %d"
             " rows, the torch route in batches of %d: its (S, nb, M, D) differences bound the batch).  Device time in milliseconds between two"
             " events on the library's stream, median (min .. max) of %d repetitions after %d warm-up evaluations.\n"
             % (DEPTH, M, D, S, L, n, a.batch, a.torch_batch, a.reps, a.warmup),
             "| route | time, ms | sine/cosine pairs per second |", "|---|---|---|",
             "| sample_functions evaluation (dsdgp_pathwise_eval) | %s | %.3g |" % (fmt(mo), pairs / (mo[0] * 1e-3)),
             "| torch, cos / sin features and K(X, Z) materialised | %s | %.3g |" % (fmt(mt), pairs / (mt[0] * 1e-3)),
             "", "torch / ours: %.2f.  Largest difference of the two routes: %.3g at a largest value of %.3g." % (mt[0] / mo[0], diff, scale),
             "The draw itself (basis, normals, the three dsdgp_pathwise_weights calls, uploads): %.1f ms, once." % t_draw,
             "Per launch of k_pw_eval (profiling events around each): %d launches, %.3f ms each on average, %.3g pairs per second inside them."
             % (launches, prof_ms / max(launches, 1), pairs / (prof_ms * 1e-3) if prof_ms > 0 else float("nan")), ""]
    if a.joint_n > 0:
        Xj = Xh[:a.joint_n]
        model.predict_all_layers_full_cov(Xj, S)
        ctx.sync()
        w0 = time.perf_counter()
        model.predict_all_layers_full_cov(Xj, S)
        ctx.sync()
        tj = (time.perf_counter() - w0) * 1e3
        ms, _ = timed(lambda: fs(ctx.to_device(Xj), on_device=True))
        lines += ["Joint draws: predict_all_layers_full_cov at n = %d, S = %d: %.1f ms wall-clock (host and device); the same rows through the "
                  "pathwise draws: %.2f ms.  Larger n for the joint route: not measured." % (a.joint_n, S, tj, ms), ""]
    else:
        lines += ["Joint draws (predict_all_layers_full_cov): not measured.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The reverse pass of the kernel expectations — the gradients of F = g0 psi0 + <g1, psi1> + <g2, psi2> in mu, s, Z, the kernel variance
and the lengthscales — two ways:

  device   dsdgp_rbf_expectations_grad (csrc/psi_grad.hip): one call on device-resident inputs
  torch    autograd through the direct form of the expectations with torch ops on the same device, n x M x M materialised in row
           chunks (at most 2^23 doubles per chunk: autograd keeps every intermediate of a chunk), one backward per chunk

at the shapes of profiles/psi_ab.md, N = 40 000, M = 128, D = 8 and N = 45 000, M = 256, D = 9; mu, Z standard normal, s uniform on
[0, 0.5), lengthscales sqrt(D), g1, g2 standard normal, fixed seed.  No parent implementation exists: the torch route is the only
yardstick on the device, and the forward's time at the same shape (profiles/psi_ab.md) the figure to set the ratio against.

Method: both routes once warm, then `--reps` repetitions ALTERNATING between them, each timed by a pair of HIP events on the library's
stream (the stream torch runs on too); medians with min .. max.  Inside one further call the library's own events (dsdgp_prof_enable)
time the k_psi2_grad launch alone; `Gexp/s` is the n M^2 exponentials it forms over that time.  `max rel diff`: the largest difference
between the two routes' d_Z, over the largest entry.  No speed is promised: the table records what was measured.
Usage: python tools/psi_grad_ab.py [--reps 5] [--out profiles/psi_grad_ab.md]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)
from doubly_stochastic_dgp import _lib  # noqa: E402
from doubly_stochastic_dgp.engine import Context  # noqa: E402

SHAPES = [(40000, 128, 8), (45000, 256, 9)]
FORWARD_MS = {(40000, 128, 8): 0.65, (45000, 256, 9): 2.45}      # profiles/psi_ab.md
CHUNK_DOUBLES = 1 << 23


def torch_grads(torch, mu, s, Z, v, ls, g0, g1, g2):
    """(d_mu, d_s, d_Z, d_v, d_ls) by autograd through the direct form, one backward per chunk of rows"""
    leaves = [x.detach().clone().requires_grad_(True) for x in (mu, s, Z, v, ls)]
    mu, s, Z, v, ls = leaves
    n, M = mu.shape[0], Z.shape[0]
    rows = max(1, CHUNK_DOUBLES // (M * M))
    for a in range(0, n, rows):
        b = min(a + rows, n)
        l2 = ls * ls
        d1 = mu[a:b, None, :] - Z[None, :, :]
        a1 = l2 + s[a:b]
        psi1 = v * torch.sqrt(torch.prod(l2 / a1, dim=1))[:, None] * torch.exp(-0.5 * torch.sum(d1 * d1 / a1[:, None, :], dim=2))
        a2 = l2 + 2.0 * s[a:b]
        w2 = 1.0 / a2
        t = 0.25 * (w2 - 1.0 / l2)
        dz = Z[:, None, :] - Z[None, :, :]
        L = -0.5 * torch.sum(w2[:, None, :] * d1 * d1, dim=2)
        E = (t @ (dz * dz).reshape(M * M, -1).T).reshape(b - a, M, M) + L[:, :, None] + L[:, None, :]
        E = E + 0.5 * torch.log(l2 * w2).sum(1)[:, None, None]
        psi2 = v * v * torch.exp(E).sum(0)
        F = g0 * (b - a) * v + torch.sum(g1[a:b] * psi1) + torch.sum(g2 * psi2)
        F.backward()
    return [x.grad for x in leaves]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi_grad_ab.md"))
    args = ap.parse_args()
    if args.reps < 3:
        raise SystemExit("--reps: at least 3 repetitions")
    ctx = Context.get()
    torch = ctx.torch
    p = lambda x: C.c_void_p(x.data_ptr())
    lines = ["# Reverse pass of the kernel expectations: dsdgp_rbf_expectations_grad against torch autograd on the same device", "",
             f"`device ms`, `torch ms`: median of {args.reps} alternating repetitions (min .. max) after a warm-up, HIP events, inputs resident;",
             "every output of the call is asked for.  `k_psi2_grad ms`: the library's own events around the hot launch inside one call;",
             "`Gexp/s`: the n M^2 exponentials it forms over that time.  `forward ms`: dsdgp_rbf_expectations at the same shape",
             "(profiles/psi_ab.md); `device / forward` the ratio.  `max rel diff`: device against torch over the entries of d_Z, in units of",
             "the largest entry.", "",
             "| n | M | D | device ms | k_psi2_grad ms | Gexp/s | forward ms | device / forward | torch ms | torch / device | max rel diff |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, M, D in SHAPES:
        rng = np.random.default_rng(n + M + D)
        mu_h, Z_h, s_h = rng.standard_normal((n, D)), rng.standard_normal((M, D)), rng.uniform(0.0, 0.5, (n, D))
        g1_h, g2_h = rng.standard_normal((n, M)), rng.standard_normal((M, M))
        ls_h = np.full(D, np.sqrt(D))
        variance, g0 = 1.7, -0.7
        spec = _lib.KernelSpec(kind=_lib.KERN_RBF, input_dim=D, ard=1, has_white=0, variance=variance, white_variance=0.0,
                               lengthscales=ls_h.ctypes.data_as(_lib.c_double_p))
        mu, Z, s, ls, g1, g2 = (ctx.to_device(a) for a in (mu_h, Z_h, s_h, ls_h, g1_h, g2_h))
        v = ctx.to_device(np.array(variance))
        d_mu, d_s, d_Z, d_k = ctx.empty(n, D), ctx.empty(n, D), ctx.empty(M, D), ctx.empty(1 + D)

        def device():
            _lib.check(ctx.lib.dsdgp_rbf_expectations_grad(ctx.handle, C.byref(spec), p(Z), M, p(mu), p(s), n, g0, p(g1), M, p(g2), M,
                                                           p(d_mu), p(d_s), p(d_Z), p(d_k)))

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ctx.tstream)
            out = fn()
            b.record(ctx.tstream)
            b.synchronize()
            return a.elapsed_time(b), out

        route = lambda: torch_grads(torch, mu, s, Z, v, ls, g0, g1, g2)
        with torch.cuda.stream(ctx.tstream):
            device()
            ref = route()
            ctx.sync()
            td, tt = [], []
            for _ in range(args.reps):
                td.append(timed(device)[0])
                tt.append(timed(route)[0])
            ctx.prof_enable(True)
            ctx.prof_read("psi2_grad")
            device()
            k_ms, _ = ctx.prof_read("psi2_grad")
            ctx.prof_enable(False)
            diff = float(((d_Z - ref[2]).abs().max() / ref[2].abs().max()).cpu())
        td, tt = np.array(td), np.array(tt)
        gexp = n * M * M / (k_ms * 1e-3) / 1e9
        md, mt, fw = float(np.median(td)), float(np.median(tt)), FORWARD_MS[(n, M, D)]
        lines.append(f"| {n} | {M} | {D} | {md:.2f} ({td.min():.2f} .. {td.max():.2f}) | {k_ms:.2f} | {gexp:.1f} | {fw:.2f} | {md / fw:.1f} | "
                     f"{mt:.2f} ({tt.min():.2f} .. {tt.max():.2f}) | {mt / md:.2f} | {diff:.2e} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""psi2 of an RBF kernel under a diagonal Gaussian input — sum_n of an M x M matrix of exponentials — three ways:

  device   dsdgp_rbf_expectations (csrc/psi.hip): psi0, psi1 and psi2 in one call on device-resident inputs
  torch    the same exponent decomposition with torch ops on the same device, materialising n x M x M in row chunks (at most
           2^25 doubles per chunk): E = h + L_i + L_j + t @ delta^2, exp, sum over the rows
  numpy    the torch route's arithmetic on the host, one run

at N = 40 000, M = 128, D = 8 and N = 45 000, M = 256, D = 9; mu, Z standard normal, s uniform on [0, 0.5), lengthscales sqrt(D), fixed
seed.  No parent implementation exists: the torch route is the only yardstick on the device.

Method: both device routes once warm, then `--reps` repetitions ALTERNATING between them, each timed by a pair of HIP events on the
library's stream (the stream torch runs on too); medians with min .. max.  Inside one further call the library's own events
(dsdgp_prof_enable) time the k_psi2 launch alone; `Gexp/s` is n M (M + 1) / 2 exponentials — the lower triangle the call is asked
for — over that time.  `max rel diff`: the largest relative difference between the device's and the torch route's psi2.
No speed is promised: the table records what was measured.
Usage: python tools/psi_ab.py [--reps 5] [--out profiles/psi_ab.md] [--no-numpy]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)
from doubly_stochastic_dgp import _lib  # noqa: E402
from doubly_stochastic_dgp.engine import Context  # noqa: E402

SHAPES = [(40000, 128, 8), (45000, 256, 9)]
CHUNK_DOUBLES = 1 << 25


def _tables(xp, mu, s, Z, l2):
    w = 1.0 / (l2 + 2.0 * s)
    t = 0.25 * (w - 1.0 / l2)
    h = 0.5 * xp.log(l2 * w).sum(1)
    dz = Z[:, None, :] - Z[None, :, :]
    return w, t, h, (dz * dz).reshape(-1, Z.shape[1])


def psi2_chunked(xp, mu, s, Z, l2, variance):
    """the decomposition of csrc/psi.hip with array ops of module xp (torch or numpy), n x M x M materialised in row chunks"""
    n, M = mu.shape[0], Z.shape[0]
    w, t, h, dz2 = _tables(xp, mu, s, Z, l2)
    rows = max(1, CHUNK_DOUBLES // (M * M))
    out = None
    for a in range(0, n, rows):
        b = min(a + rows, n)
        d = mu[a:b, None, :] - Z[None, :, :]
        L = -0.5 * (w[a:b, None, :] * d * d).sum(2)
        E = (t[a:b] @ dz2.T).reshape(b - a, M, M) + L[:, :, None] + L[:, None, :] + h[a:b, None, None]
        part = xp.exp(E).sum(0)
        out = part if out is None else out + part
    return variance * variance * out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi_ab.md"))
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    if args.reps < 3:
        raise SystemExit("--reps: at least 3 repetitions")
    ctx = Context.get()
    torch = ctx.torch
    p = lambda x: C.c_void_p(x.data_ptr())
    lines = ["# Kernel expectations: dsdgp_rbf_expectations against a torch route on the same device and numpy on the host", "",
             f"`device ms`, `torch ms`: median of {args.reps} alternating repetitions (min .. max) after a warm-up, HIP events, inputs resident;",
             "the device call also writes psi0 and psi1.  `k_psi2 ms`: the library's own events around the psi2 launch inside one call;",
             "`Gexp/s`: n M (M + 1) / 2 exponentials over that time.  `numpy ms`: one host run of the torch route's arithmetic.",
             "`max rel diff`: device against torch, over the entries of psi2.", "",
             "| n | M | D | device ms | k_psi2 ms | Gexp/s | torch ms | torch / device | numpy ms | max rel diff |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for n, M, D in SHAPES:
        rng = np.random.default_rng(n + M + D)
        mu_h, Z_h, s_h = rng.standard_normal((n, D)), rng.standard_normal((M, D)), rng.uniform(0.0, 0.5, (n, D))
        ls_h = np.full(D, np.sqrt(D))
        variance = 1.7
        spec = _lib.KernelSpec(kind=_lib.KERN_RBF, input_dim=D, ard=1, has_white=0, variance=variance, white_variance=0.0,
                               lengthscales=ls_h.ctypes.data_as(_lib.c_double_p))
        mu, Z, s, l2 = ctx.to_device(mu_h), ctx.to_device(Z_h), ctx.to_device(s_h), ctx.to_device(ls_h ** 2)
        psi0, psi1, psi2 = ctx.empty(1), ctx.empty(n, M), ctx.empty(M, M)

        def device():
            _lib.check(ctx.lib.dsdgp_rbf_expectations(ctx.handle, C.byref(spec), p(Z), M, p(mu), p(s), n, p(psi0), p(psi1), M, p(psi2), M))

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ctx.tstream)
            out = fn()
            b.record(ctx.tstream)
            b.synchronize()
            return a.elapsed_time(b), out

        with torch.cuda.stream(ctx.tstream):
            device()
            ref = psi2_chunked(torch, mu, s, Z, l2, variance)
            ctx.sync()
            td, tt = [], []
            for _ in range(args.reps):
                td.append(timed(device)[0])
                tt.append(timed(lambda: psi2_chunked(torch, mu, s, Z, l2, variance))[0])
            ctx.prof_enable(True)
            ctx.prof_read("psi2")
            device()
            k_ms, _ = ctx.prof_read("psi2")
            ctx.prof_enable(False)
            diff = float(((psi2 - ref).abs() / ref.abs()).max().cpu())
        td, tt = np.array(td), np.array(tt)
        if args.no_numpy:
            np_ms = float("nan")
        else:
            print(f"n = {n}, M = {M}: numpy ...", flush=True)
            t0 = time.perf_counter()
            psi2_chunked(np, mu_h, s_h, Z_h, ls_h ** 2, variance)
            np_ms = 1e3 * (time.perf_counter() - t0)
        gexp = n * M * (M + 1) / 2.0 / (k_ms * 1e-3) / 1e9
        md, mt = float(np.median(td)), float(np.median(tt))
        lines.append(f"| {n} | {M} | {D} | {md:.2f} ({td.min():.2f} .. {td.max():.2f}) | {k_ms:.2f} | {gexp:.1f} | "
                     f"{mt:.2f} ({tt.min():.2f} .. {tt.max():.2f}) | {mt / md:.2f} | {np_ms:.0f} | {diff:.2e} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

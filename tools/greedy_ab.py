#!/usr/bin/env python
"""The greedy conditional-variance selection of M inducing points three ways:

  device    dsdgp_greedy_inducing (csrc/greedy.hip): M + 3 launches on the library's stream, all outputs requested
  numpy     tests/greedy_reference.greedy(..., dtype=np.float64) on the host: the same algorithm, one matrix-vector product per step
  k-means   dsdgp_kmeans, ten Lloyd iterations from M random rows: the other way the library places inducing points

at n = 50 000, D = 8, M = 128 / 512 / 1024 and at the MNIST shape n = 60 000, D = 784, M = 512; X = N(0, 1) from a fixed seed, RBF
with variance 1 and lengthscale 2 (D = 8) or 25 (D = 784), threshold 0 so that all M steps run.

Method: each device route warm (code objects loaded, scratch grown), then `--reps` calls, each between two events on the library's
stream; medians with min .. max.  numpy: one run on the host clock (`--skip-numpy TAG[,TAG]` leaves a shape's run out: its cell then
reads "not measured").  The device's bytes are counted as sum_j 8 n (D + j + 3) — the D rows of the transposed data, the j columns and
the residual read and written at step j — and reported per second against the 6.29 TB/s a streaming kernel reaches from HBM here.  A
column store M n 8 under 256 MB can stay in the Infinity Cache between steps: those shapes' rates say what the cache serves, only the
larger ones what HBM does; the table marks which is which.  No speed is promised: the table records what was measured.
Usage: python tools/greedy_ab.py [--reps 7] [--skip-numpy mnist] [--out profiles/greedy_ab.md]"""
import argparse
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)
from doubly_stochastic_dgp import _lib  # noqa: E402
from doubly_stochastic_dgp.engine import Context, ptr  # noqa: E402
from tests import greedy_reference as R  # noqa: E402

SHAPES = [("m128", 50000, 8, 128, 2.0), ("m512", 50000, 8, 512, 2.0), ("m1024", 50000, 8, 1024, 2.0), ("mnist", 60000, 784, 512, 25.0)]
HBM_TBS = 6.29
CACHE_MB = 256.0
KMEANS_ITERS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-numpy", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_ab.md"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps: at least 5 repetitions")
    skip = set(filter(None, args.skip_numpy.split(",")))
    ctx = Context.get()
    lib, torch = ctx.lib, ctx.torch
    lines = ["# Greedy inducing points: dsdgp_greedy_inducing against numpy on the host and against dsdgp_kmeans", "",
             f"ms per call: median of {args.reps} calls (min .. max) after a warm-up, each between two events on the library's stream;",
             "numpy (tests/greedy_reference.py, float64): one run, host clock.  TB/s: sum_j 8 n (D + j + 3) bytes over the device's median;",
             f"% of the {HBM_TBS} TB/s achievable from HBM.  `store`: the column store M n 8, and whether it fits the {CACHE_MB:.0f} MB Infinity Cache",
             "(a shape that fits measures the cache, not HBM).", "",
             "| shape | device ms | launches | TB/s | % of HBM rate | store | numpy ms | numpy / device | k-means ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for tag, n, D, M, ell in SHAPES:
        rng = np.random.default_rng(n + D + M)
        X = rng.standard_normal((n, D))
        ls = np.array([ell])
        spec = _lib.KernelSpec(kind=_lib.KERN_RBF, input_dim=D, ard=0, has_white=0, variance=1.0, white_variance=0.0,
                               lengthscales=ls.ctypes.data_as(_lib.c_double_p))
        Xd = ctx.to_device(X)
        idx = torch.empty(M, dtype=torch.int32, device=Xd.device)
        m_out = torch.empty(1, dtype=torch.int32, device=Xd.device)
        Z, res, tr, L = ctx.empty(M, D), ctx.empty(M), ctx.empty(M), ctx.empty(M, M)
        Z0, Zk = ctx.to_device(X[rng.permutation(n)[:M]]), ctx.empty(M, D)

        def device():
            _lib.check(lib.dsdgp_greedy_inducing(ctx.handle, C.byref(spec), ptr(Xd), n, M, -1, 0.0, ptr(idx), ptr(m_out), ptr(Z), ptr(res),
                                                 ptr(tr), ptr(L), M))

        def kmeans():
            _lib.check(lib.dsdgp_kmeans(ctx.handle, ptr(Xd), n, D, M, ptr(Z0), KMEANS_ITERS, ptr(Zk), None, None, None))

        med, spread = {}, {}
        with torch.cuda.stream(ctx.tstream):
            for name, fn in (("device", device), ("kmeans", kmeans)):
                fn()
                ctx.sync()
                c0 = int(lib.dsdgp_launch_count())
                fn()
                ctx.sync()
                launches = int(lib.dsdgp_launch_count()) - c0
                if name == "device":
                    dev_launches = launches
                t = []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(ctx.tstream)
                    fn()
                    b.record(ctx.tstream)
                    b.synchronize()
                    t.append(a.elapsed_time(b))
                t = np.array(t)
                med[name], spread[name] = float(np.median(t)), (float(t.min()), float(t.max()))
            device()
            ctx.sync()
        m = int(m_out.cpu().numpy()[0])
        dev_idx = idx.cpu().numpy()[:m]
        nbytes = sum(8.0 * n * (D + j + 3) for j in range(M))
        tbs = nbytes / (med["device"] * 1e-3) / 1e12
        store_mb = M * n * 8 / 1e6
        fits = "fits" if store_mb < CACHE_MB else "does not fit"
        if tag in skip:
            np_ms, ratio = "not measured", "not measured"
        else:
            print(f"{tag}: numpy ...", flush=True)
            t0 = time.perf_counter()
            box = {}
            th = threading.Thread(target=lambda: box.update(ref=R.greedy(X, M, "rbf", 1.0, ls, dtype=np.float64), t=time.perf_counter()))
            th.start()
            while th.is_alive():
                th.join(60.0)
                if th.is_alive():
                    print(f"{tag}: numpy still running ({time.perf_counter() - t0:.0f} s)", flush=True)
            ref, ts = box["ref"], box["t"] - t0
            np_ms, ratio = f"{1e3 * ts:.0f}", f"{1e3 * ts / med['device']:.0f}"
            same = int(np.sum(ref["indices"][:m] == dev_idx[:ref["m"]])) if ref["m"] == m else -1
            notes.append(f"{tag}: the device and the float64 numpy run agree on {same} of {m} rows (random data: no margin is guaranteed, "
                         f"see tests/greedy_cases.py for the pinned cases); trace after {m} points {float(tr[m - 1]):.6g} (device) "
                         f"against {float(ref['trace'][-1]):.6g} (numpy).")
        lines.append(f"| {tag} ({n} x {D}, M = {M}) | {med['device']:.2f} ({spread['device'][0]:.2f} .. {spread['device'][1]:.2f}) | {dev_launches} | "
                     f"{tbs:.2f} | {100.0 * tbs / HBM_TBS:.0f} | {store_mb:.0f} MB, {fits} | {np_ms} | {ratio} | "
                     f"{med['kmeans']:.2f} ({spread['kmeans'][0]:.2f} .. {spread['kmeans'][1]:.2f}) |")
        print(lines[-1], flush=True)
        if m != M:
            notes.append(f"{tag}: stopped at m = {m} of {M}")
        del Xd, Z, L, Z0, Zk
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

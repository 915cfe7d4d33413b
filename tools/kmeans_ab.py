#!/usr/bin/env python
"""Ten Lloyd iterations three ways, from the same start centres:

  fused          dsdgp_kmeans: centring, then per iteration the fp64-MFMA distance + argmin launch (nothing of size n x M written),
                 the counting sort by label and the ordered segment sums
  materialised   on the same GPU with torch: d = |x|^2 + |z|^2 - 2 X @ Z.T (n x M, through memory), argmin, index_add_ of the rows into
                 their centres, bincount, divide; an empty cluster keeps its centre
  scipy          scipy.cluster.vq.kmeans2(X, Z0, iter=10, minit='matrix') on the host (demos/run_regression.py:57)

at the headline shape (8192 x 8, M = 128) and the MNIST shape (60000 x 784, M = 512), X = N(0, 1) from a fixed seed.

Method: both device routes warm (code objects loaded, scratch grown, allocator primed), then `--reps` repetitions in which the two
alternate; one timing = one call of ten iterations between two events on the library's stream.  Medians, with min .. max as the
spread.  scipy: one run on the host clock.  The assign launch alone is timed in a further pass with the library's profiling events
(dsdgp_prof_enable; not during the A/B) and reported as 2 n M D / t against the 78.6 TFLOP/s fp64 MFMA peak at the MNIST shape and as
the bytes of X over t against 8 TB/s at the headline shape.  No speed is promised: the table records what was measured.
Usage: python tools/kmeans_ab.py [--reps 21] [--no-scipy] [--out profiles/kmeans_ab.md]"""
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
from doubly_stochastic_dgp.engine import Context, ptr  # noqa: E402

SHAPES = [("headline", 8192, 8, 128), ("MNIST", 60000, 784, 512)]
ITERS = 10
PEAK_TFLOPS, PEAK_TBS = 78.6, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_ab.md"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps: at least 20 repetitions")
    ctx = Context.get()
    lib, torch = ctx.lib, ctx.torch
    lines = ["# k-means for the inducing points: dsdgp_kmeans against a materialised route on the same GPU and scipy on the host", "",
             f"ms per call of {ITERS} iterations: median of {args.reps} repetitions (min .. max), each call between two events on the library's",
             "stream, both device routes warm, alternating within a repetition; scipy: one run, host clock", "",
             "| shape | route | ms per call | launches per call |", "|---|---|---|---|"]
    notes = []
    for tag, n, D, M in SHAPES:
        rng = np.random.default_rng(n + D + M)
        X = rng.standard_normal((n, D))
        idx = rng.permutation(n)[:M]
        Xd, Z0 = ctx.to_device(X), ctx.to_device(X[idx])
        Z = ctx.empty(M, D)
        lab = torch.empty(n, dtype=torch.int32, device=Xd.device)
        out = {}

        def fused():
            _lib.check(lib.dsdgp_kmeans(ctx.handle, ptr(Xd), n, D, M, ptr(Z0), ITERS, ptr(Z), ptr(lab), None, None))

        def materialised():
            Zt = Z0.clone()
            xn = (Xd * Xd).sum(1, keepdim=True)
            for _ in range(ITERS):
                d = xn + (Zt * Zt).sum(1)[None, :] - 2.0 * (Xd @ Zt.T)
                lt = d.argmin(1)
                sums = torch.zeros_like(Zt).index_add_(0, lt, Xd)
                cnt = torch.bincount(lt, minlength=M)
                Zt = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1)[:, None].to(sums.dtype), Zt)
            out["Z"], out["labels"] = Zt, lt

        order = [("fused", fused), ("materialised", materialised)]
        launches = {}
        with torch.cuda.stream(ctx.tstream):
            for name, fn in order:
                for _ in range(3):
                    fn()
                ctx.sync()
            c0 = int(lib.dsdgp_launch_count())
            fused()
            ctx.sync()
            launches["fused"] = str(int(lib.dsdgp_launch_count()) - c0)
            launches["materialised"] = "(torch)"
            differ = int((out["labels"].to(torch.int32) != lab).sum())
            zdiff = float((out["Z"] - Z).abs().max())
            times = {name: [] for name, _ in order}
            for _ in range(args.reps):
                for name, fn in order:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(ctx.tstream)
                    fn()
                    b.record(ctx.tstream)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b))
        med = {}
        for name, _ in order:
            t = np.array(times[name])
            med[name] = float(np.median(t))
            lines.append(f"| {tag} ({n} x {D}, M = {M}) | {name} | {med[name]:.3f} ({t.min():.3f} .. {t.max():.3f}) | {launches[name]} |")
        print("\n".join(lines[-2:]), flush=True)
        # the assign launch alone
        ctx.prof_enable(True)
        ctx.prof_read("kmeans_assign")
        ctx.prof_read("kmeans_update")
        for _ in range(3):
            fused()
        ctx.sync()
        ms_a, k_a = ctx.prof_read("kmeans_assign")
        ms_u, k_u = ctx.prof_read("kmeans_update")
        ctx.prof_enable(False)
        ta, tu = ms_a / k_a, ms_u / k_u
        tf = 2.0 * n * M * D / (ta * 1e-3) / 1e12
        tb = 8.0 * n * D / (ta * 1e-3) / 1e12
        ratio = med["fused"] / med["materialised"]
        verdict = ("fused is faster by more than 1 %" if ratio < 0.99 else "fused is SLOWER by more than 1 %" if ratio > 1.01
                   else "the two do not differ by more than 1 %")
        notes.append(f"{tag}: fused / materialised = {ratio:.3f} ({verdict}); {differ} of {n} labels differ between the two routes after "
                     f"{ITERS} iterations, centres by at most {zdiff:.2e}.  Assign launch {1e3 * ta:.1f} us (mean of {k_a}, event-bracketed): "
                     f"2 n M D / t = {tf:.2f} TFLOP/s = {100.0 * tf / PEAK_TFLOPS:.1f} % of the {PEAK_TFLOPS} TFLOP/s fp64 MFMA peak; "
                     f"bytes of X / t = {tb:.3f} TB/s = {100.0 * tb / PEAK_TBS:.1f} % of {PEAK_TBS} TB/s.  The four update launches "
                     f"(histogram, scan, scatter, segment sums) {1e3 * tu:.1f} us per iteration.")
        if not args.no_scipy:
            from scipy.cluster.vq import kmeans2
            import warnings
            print(f"{tag}: scipy ...", flush=True)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                Zs, ls = kmeans2(X, X[idx].copy(), iter=ITERS, minit="matrix")
                ts = time.perf_counter() - t0
            lines.append(f"| {tag} ({n} x {D}, M = {M}) | scipy (host) | {1e3 * ts:.1f} | |")
            notes.append(f"{tag}: scipy / fused = {1e3 * ts / med['fused']:.0f}; {int((ls != lab.cpu().numpy()).sum())} of {n} labels differ "
                         f"between scipy and fused.")
            print(lines[-1], flush=True)
        del Xd, Z0, Z, lab, out
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

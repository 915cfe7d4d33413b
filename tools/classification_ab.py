#!/usr/bin/env python
"""The MultiClass mixture probabilities two ways, on the same device arrays:

  classification   dsdgp_mixture_classification with probs_out and rows_out set: one launch for all K class integrals of all S
                   components, the report kernel, the second-stage sum
  evaluate         dsdgp_eval_mixture(MultiClass) with rows_out set: 1 + K launches of k_multiclass writing a (1 + K) x (S n) table of
                   log probabilities, the reduction that reads it back through exp, the second-stage sum

at n = 1000, K = 10, S = 100 (benchmark config 4's evaluation batch) and n = 512, K = 10, S = 10.  Both leave the n x K mixture
probabilities and the per-row log density on the device; `classification` also the report's accumulator.

Method: warm-up, then `--reps` repetitions in which the variants alternate; one timing = `inner` back-to-back calls and one
synchronisation, host clock, divided by `inner`.  `inner` is sized from the warm-up so that the fastest variant's timing lasts
`--window` seconds (a window of a few milliseconds would measure the clock and the scheduler), the same count for every variant of a
shape; `--inner N` fixes it.  `classification` is timed twice per repetition (first and last).  The spread the comparison is read
against is each variant's min .. max over the repetitions; the larger of the two classification ranges and the distance of their
medians is the figure a difference has to exceed.  No speed is promised: the table records what was measured.
Usage: python tools/classification_ab.py [--reps 9] [--window 0.5] [--inner 0] [--out profiles/classification_ab.md]"""
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

SHAPES = [(1000, 10, 100), (512, 10, 10)]
BINS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.5, help="seconds one timing should last (sizes the inner count)")
    ap.add_argument("--inner", type=int, default=0, help="calls per timing; 0: from --window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classification_ab.md"))
    args = ap.parse_args()
    ctx = Context.get()
    lib = ctx.lib
    lines = ["# MultiClass mixture probabilities: dsdgp_mixture_classification against dsdgp_eval_mixture", "",
             f"per call, ms: median of {args.reps} repetitions (min .. max), each `calls` back-to-back calls + one synchronisation on the",
             "host clock; the variants alternate within a repetition, `classification` runs first and last in it", "",
             "| n, K, S | variant | ms per call | calls per timing | launches per call |", "|---|---|---|---|---|"]
    notes = []
    for n, K, S in SHAPES:
        rng = np.random.RandomState(n + K + S)
        mean = ctx.to_device(rng.randn(S, n, K) + 0.7 * rng.randn(1, n, K))
        var = ctx.to_device(rng.uniform(0.01, 1.5, size=(S, n, K)))
        Y = ctx.to_device(rng.randint(0, K, size=(n, 1)).astype(np.float64))
        acc_c, probs, rows_c = ctx.empty(4 + 3 * BINS + K + K * K, 1), ctx.empty(n, K), ctx.empty(n, 1, 4)
        acc_e, rows_e = ctx.empty(3, K), ctx.empty(n, K, 3)

        def classification():
            _lib.check(lib.dsdgp_mixture_classification(ctx.handle, _lib.LIK_MULTICLASS, ptr(mean), ptr(var), ptr(Y), n, S, K, BINS,
                                                        ptr(probs), ptr(rows_c), ptr(acc_c), 0))

        def evaluate():
            _lib.check(lib.dsdgp_eval_mixture(ctx.handle, _lib.LIK_MULTICLASS, 1.0, 1.0, ptr(mean), ptr(var), ptr(Y), n, S, K, ptr(rows_e),
                                              ptr(acc_e), 0))

        order = [("classification", classification), ("evaluate", evaluate), ("classification (again)", classification)]
        launches, est = {}, {}
        for name, fn in order:      # warm-up: code objects loaded, scratch grown; launches counted on the second call
            fn()
            ctx.sync()
            c0 = int(lib.dsdgp_launch_count())
            fn()
            ctx.sync()
            launches[name] = int(lib.dsdgp_launch_count()) - c0
            t0 = time.perf_counter()
            for _ in range(10):
                fn()
            ctx.sync()
            est[name] = (time.perf_counter() - t0) / 10
        inner = args.inner if args.inner > 0 else int(min(100000, max(20, np.ceil(args.window / min(est.values())))))
        # same numbers from both routes
        pe, pc = rows_e.cpu().numpy()[..., 0], probs.cpu().numpy()
        le, lc = rows_e.cpu().numpy()[:, 0, 2], rows_c.cpu().numpy()[:, 0, 2]
        agree = (float(np.max(np.abs(pe - pc) / np.abs(pe))), float(np.max(np.abs(le - lc))))
        times = {name: [] for name, _ in order}
        for _ in range(args.reps):
            for name, fn in order:
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                ctx.sync()
                times[name].append((time.perf_counter() - t0) / inner)
        med, rng_ = {}, {}
        for name, _ in order:
            t = 1e3 * np.array(times[name])
            med[name], rng_[name] = float(np.median(t)), float(t.max() - t.min())
            lines.append(f"| {n}, {K}, {S} | {name} | {med[name]:.4f} ({t.min():.4f} .. {t.max():.4f}) | {inner} | {launches[name]} |")
        both = med["classification"], med["classification (again)"]
        spread = max(rng_["classification"], rng_["classification (again)"], abs(both[0] - both[1]))
        diff = max(both) - med["evaluate"]
        verdict = ("classification is slower than evaluate by more than the spread" if diff > spread else
                   "classification is faster than evaluate by more than the spread" if med["evaluate"] - max(both) > max(spread, rng_["evaluate"])
                   else "the two routes do not differ by more than the spread")
        notes.append(f"n = {n}, K = {K}, S = {S}: classification / evaluate = {both[0] / med['evaluate']:.3f} (first), "
                     f"{both[1] / med['evaluate']:.3f} (again); spread (the larger min .. max range of the two classification timings, or "
                     f"the distance of their medians) {spread:.4f} ms, evaluate's range {rng_['evaluate']:.4f} ms: {verdict}; the routes' "
                     f"probabilities differ by at most {agree[0]:.2e} (relative), the log densities by {agree[1]:.2e}")
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

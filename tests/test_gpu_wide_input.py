"""The chain kernels across input widths 9 .. 784, against the oracle (case table: tests/wide_input_cases.py, which names the branch
each case is there for; tests/test_wide_input_cases_cpu.py asserts that the table reaches them and that the oracle's own noise at these
shapes is orders of magnitude below the bars).

Per case: samples, mean and variance of every layer from model.propagate (forward-only: the whitened forward instances for a
non-white model) and the ELBO with every gradient block of every layer from the training pass (the plain instances, the backward
chain, the weight-gradient products), a second evaluation bit for bit, for two cases two optimiser steps against Adam on the oracle's
gradients, and for the D_in = 16 | 17 twins the launch counter across the head launch's threshold.

Bars — the suite's own for the same quantities on narrow inputs (test_gpu_parity.py, test_gpu_round6.py): rtol 1e-9 / atol 1e-10 on
layer outputs and the ELBO, max |delta| <= 1e-7 x max |block| per gradient block, rtol 1e-7 on the ELBO after two optimiser steps.

What a failure looks like — two changes to the wide distance code (sm_sqdist), tried together once while writing this file, neither
seen by any other test of the suite (its only inputs wider than 64 are 784-dimensional at M = 512, the GEMM-formulated passes):
(1) the masked path dropping the last column of every chunk but the first (`in[s] = j < jn - (j0 > 0)`) and (2) the 32-byte-load
path scaling x / l by 1 + 1e-6 in every chunk but the first.  All 13 cases above 64 fail and all 9 at or below 64 pass.  Under (1)
(d65, d70-*, d90, d100, d130) the first layer's outputs are off by 1e8 .. 1e9 x their bar, the ELBO by 3e-5 .. 4e-3, gradient blocks
by 0.2 .. 1.3 of their largest entry.  Under (2): d80 outputs 1.9e3 x the bar, ELBO 1.3e-8, l1.Z 1.1e-6; d128-M512 outputs 9e2 x,
ELBO 8e-8, kernel variance 2e-5; d784-pca30 — 16 of 784 columns — outputs 2.4e3 x the bar while its ELBO (1.4e-12) and every gradient
block (at most 1e-8) stay inside theirs: the per-layer outputs are the sharpest of the three checks.  Unmutated, the worst layer
output of any case sits at 8.5e-4 of its bar, the ELBOs at 4e-15 or better and the worst gradient block at 4.8e-13 of its largest
entry, five orders inside 1e-7 (profiles/wide_input_errors.md).  No case exposed a defect in the library.

DSDGP_WIDE_PROFILE=<file> writes the measured errors of every case as one table (profiles/wide_input_errors.md).
"""
import os
import time

import numpy as np
import pytest
from numpy.testing import assert_allclose

from doubly_stochastic_dgp import _lib
from oracle import dgp_oracle as O
from oracle import model as OM
from tests import wide_input_cases as W
from tests.helpers import kern_spec, make_case

pytestmark = pytest.mark.gpu

OUT_RTOL, OUT_ATOL = 1e-9, 1e-10
GRAD_BAR = 1e-7
STEP_RTOL = 1e-7

_ROWS = []
_LAUNCHES = {}


@pytest.fixture(scope="module", autouse=True)
def profile_table():
    t0 = time.time()
    yield
    path = os.environ.get("DSDGP_WIDE_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Input widths 9 .. 784 on the chain kernels against the oracle (tests/test_gpu_wide_input.py)\n\n"
                "`outputs`: the worst of max |dev - oracle| / (1e-10 + 1e-9 |oracle|) over samples, mean and variance of every layer (bar 1);\n"
                "`ELBO`: |dev - oracle| / |oracle| (bar 1e-9); `gradient`: the worst block's max |dev - oracle| / max |oracle| (bar 1e-7) and its name;\n"
                "`two steps`: the ELBO's relative error after two optimiser steps against Adam on the oracle's gradients (bar 1e-7).\n\n"
                "| case | widths | M -> Mp | kernel | white | force | outputs | ELBO | gradient | block | two steps | seconds |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| " + " | ".join(r) + " |\n")
        f.write(f"\n{len(_ROWS)} cases, {time.time() - t0:.0f} s for the module.\n")


def _set_force(monkeypatch, force):
    """DSDGP_FORCE is read when the device model is created: set (or clear) it before make_case"""
    if force:
        monkeypatch.setenv("DSDGP_FORCE", force)
    else:
        monkeypatch.delenv("DSDGP_FORCE", raising=False)


def _model(case, ref):
    inp = ref["inp"]
    spec, state, model = make_case(inp["X"], inp["Y"], inp["Z"], inp["specs"], white=case.white, jitter=1e-6, S=case.S,
                                   num_data=ref["num_data"], seed=W.MAKE_CASE_SEED)
    for k, v in ref["state"].items():             # the device model and the oracle's reference start from the same numbers
        assert np.array_equal(np.asarray(state[k]), np.asarray(v)), k
    return model


def _grads(model):
    return {k: np.asarray(v).copy() for k, v in model.engine().gradient_dict().items()}


def _scaled(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (OUT_ATOL + OUT_RTOL * np.abs(want))))


@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_wide_input_case_against_the_oracle(monkeypatch, case):
    t0 = time.time()
    ref = W.reference(case)
    inp = ref["inp"]
    X, Y, zs, S = inp["X"], inp["Y"], inp["zs"], case.S
    L = len(case.widths) - 1
    _set_force(monkeypatch, case.force)
    model = _model(case, ref)
    failures = []

    # ---- forward only: samples, mean, variance of every layer
    Fs, Fm, Fv = model.propagate(X, S=S, zs=zs)
    worst_out = 0.0
    for what, dev, orc in (("F", Fs, ref["prop"][0]), ("mean", Fm, ref["prop"][1]), ("var", Fv, ref["prop"][2])):
        for l in range(L):
            e = _scaled(dev[l], orc[l])
            worst_out = max(worst_out, e)
            if not e <= 1.0:
                failures.append(f"layer {l} {what}: {e:.3g} x the bar (rtol {OUT_RTOL:g}, atol {OUT_ATOL:g})")

    # ---- training pass: ELBO and every gradient block
    got = model._build_likelihood(X, Y, zs=zs, with_grad=True)
    elbo_err = abs(got - ref["elbo"]) / abs(ref["elbo"])
    if not abs(got - ref["elbo"]) <= OUT_ATOL + OUT_RTOL * abs(ref["elbo"]):
        failures.append(f"ELBO: {got!r} against {ref['elbo']!r} ({elbo_err:.3g})")
    g1 = _grads(model)
    assert set(ref["grad"]) <= set(g1), sorted(set(ref["grad"]) - set(g1))
    assert "lik_variance_raw" in ref["grad"]
    gerr = {}
    for k, go in ref["grad"].items():
        gerr[k] = float(np.max(np.abs(-go - g1[k])) / np.max(np.abs(go)))            # the device gradient is of the loss = -ELBO
        if not gerr[k] <= GRAD_BAR:
            failures.append(f"gradient {k}: {gerr[k]:.3g} of its largest entry (bar {GRAD_BAR:g})")
    kworst = max(gerr, key=lambda k: (np.isnan(gerr[k]), gerr[k]))

    # ---- a second evaluation returns the same bits
    got2 = model._build_likelihood(X, Y, zs=zs, with_grad=True)
    g2 = _grads(model)
    if got2 != got:
        failures.append(f"second evaluation: ELBO {got2!r} after {got!r}")
    for k in g1:
        if not np.array_equal(g1[k], g2[k]):
            failures.append(f"second evaluation: gradient {k} differs by {np.max(np.abs(g1[k] - g2[k])):.3g}")

    # ---- two optimiser steps against Adam on the oracle's gradients
    step_err = None
    if case.two_steps:
        keys = sorted(ref["state"].keys())
        th = {k: np.array(ref["state"][k], dtype=np.float64) for k in keys}
        mm = {k: np.zeros_like(th[k]) for k in keys}
        vv = {k: np.zeros_like(th[k]) for k in keys}
        for t in range(1, 3):
            gg = ref["grad"] if t == 1 else OM.elbo_and_grad(ref["spec"], th, X, Y, zs, S, num_data=ref["num_data"])[1]
            for k in keys:
                O.adam_step(th[k], -gg[k], mm[k], vv[k], t, lr=0.01)
            model.train_step(0.01, X=X, Y=Y, zs=zs)
        want = OM.elbo(ref["spec"], th, X, Y, zs, S, num_data=ref["num_data"])
        after = model.compute_log_likelihood(X, Y, zs=zs)
        step_err = abs(after - want) / abs(want)
        if not step_err <= STEP_RTOL:
            failures.append(f"ELBO after two optimiser steps: {after!r} against {want!r} ({step_err:.3g}, bar {STEP_RTOL:g})")

    # ---- the head launch's threshold in the launch counter
    if case.name in W.TWINS_HEAD:
        # Every train_step leaves Ku invalid (model_schedule.hpp, train_step_impl: kuu_valid = false), so the step after one starts with
        # the whole head of an evaluation.  prepare_async (same file): with head_ok ONE launch, k_head (factorisation, inverse and the
        # parameter transforms); without it k_prep_kuu and, below big_mp() = 192, one k_potrf_trtri launch for all layers (potrf_launch,
        # linalg.hip) — TWO launches.  Nothing else in the schedule of a step tells D_in = 16 from 17 at Mp = 32: DinP16 = 32 and the
        # fused tail (D_in <= 32) for both, no fused last layer at Mp = 32, explicit draws.  So the step costs one launch more at 17.
        from doubly_stochastic_dgp.engine import Context
        lib = Context.get().lib
        lib.dsdgp_launch_count.restype = __import__("ctypes").c_int64
        model.train_step(0.01, X=X, Y=Y, zs=zs, sync=True)
        n0 = lib.dsdgp_launch_count()
        model.train_step(0.01, X=X, Y=Y, zs=zs, sync=True)
        _LAUNCHES[case.name] = lib.dsdgp_launch_count() - n0
        print(f"launches of a train_step at {case.name}: {_LAUNCHES[case.name]}")
        if all(n in _LAUNCHES for n in W.TWINS_HEAD):
            n16, n17 = (_LAUNCHES[n] for n in W.TWINS_HEAD)
            if n17 != n16 + 1:
                failures.append(f"launches of a step: {n16} at D_in = 16, {n17} at D_in = 17 (expected one more without the head launch)")

    row = [case.name, "-".join(map(str, case.widths)), f"{case.M} -> {case.Mp}", case.kind, str(int(case.white)), case.force or "-",
           f"{worst_out:.3g}", f"{elbo_err:.3g}", f"{gerr[kworst]:.3g}", kworst, "-" if step_err is None else f"{step_err:.3g}",
           f"{time.time() - t0:.1f}"]
    print("WIDE_INPUT | " + " | ".join(row))
    _ROWS.append(row)
    assert not failures, f"{case.name} ({case.comment}):\n  " + "\n  ".join(failures) + f"\n  all gradient blocks: {gerr}"


@pytest.mark.parametrize("M,D_in,force", W.UNSUPPORTED)
def test_wide_layers_the_chains_cannot_hold_fail_loudly(monkeypatch, M, D_in, force):
    """A wide layer from Mp = 640 on runs 16 waves and would need more than 160 KiB of LDS for its activations and the dX partials of a
    64-column chunk (sm_lds; by default such layers take the GEMM-formulated passes): with `gemm_mp=0` the launch is refused with
    DSDGP_ERR_UNSUPPORTED instead of running anything"""
    assert W.sm_lds_bytes(W.pad_M(M), D_in, 1, 16) > 160 * 1024
    _set_force(monkeypatch, force)
    rng = np.random.RandomState(M)
    N = 16
    XZ = rng.randn(N + M, D_in)
    X, Y, Z = XZ[:N], rng.randn(N, 1), XZ[N:]
    with pytest.raises(_lib.DsdgpError, match=f"libdsdgp error {_lib.ERR_UNSUPPORTED}:"):
        _, _, model = make_case(X, Y, Z, [kern_spec("rbf", D_in, 1.1, float(np.sqrt(D_in)))], S=1, num_data=N)
        model._build_likelihood(X, Y, zs=[rng.randn(1, N, 1)])

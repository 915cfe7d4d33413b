"""-m gpu: SGPR_Layer's chain (set_data: gram, potrf, four solves, potrf; conditional_ND: two solves) on inducing inputs that make
Kuu + jitter I ill-conditioned — twins 1e-4 apart, data points as inducing inputs with M across the 128-row panel, a fine 1-D grid;
cond 1e7 .. 1e8 (tests/collapsed_reference.py::ILL_CASES) — where tests/test_gpu_collapsed.py stops at cond ~ 2e2 on purpose.

The yardsticks are fed the DEVICE's own statistics: Kuu from dsdgp_gram, psi0 / psi1 / psi2 from kernel_expectations, K(Z, X*) from
dsdgp_gram — separate calls on the same inputs, bit-reproducible (asserted) — so the rounding of the distance expansion, amplified by
cond, is not charged to the chain; the gram and the expectations have tests of their own.

 1. Stage residuals, order-independent, the hard assertions.  L, G, LB, c are read back from the layer; tmp1, tmp2 are recomputed with
    the device calls conditional_ND makes.  Each residual componentwise in longdouble, in units of 2^-53, scaled by the product of the
    magnitudes of its factors; each <= 8 max(the same residual of the LAPACK / scipy chain on the same statistics, the largest such
    value over the three ill-conditioned cases).  LB LB^T - (G / s2 + I) is taken on the lower triangle, the one the factorisation
    reads: G, out of two one-sided solves, is symmetric only to cond(L) roundings in every chain (collapsed_reference.stage_residuals).
    The five well-conditioned cases of test_gpu_collapsed.py get the same assertions.
 2. Assembly: the six terms of bound_terms() against the longdouble evaluation of the same formulas from the device's LB, G, c:
    8 x 2^-52 of sum |terms| — dsdgp_collapsed_bound without any conditioning.
 3. End to end against collapsed_reference.truth (the longdouble chain of collapsed_from with its ill-conditioned part carried in
    double-longdouble: at cond 1e8 the plain longdouble chain is itself 3e-13 off on the mean): bound in units of sum |terms|, mean
    in max |Y|, variance (both full_cov) in the kernel variance, <= 8 max(family, 2^-50), family = the largest error over six float64
    evaluations of the same statistics (written-out order, LAPACK, four seeded permutations of the inducing inputs); extended to at
    most 16 members if the device lands above it with every stage residual inside its bar, and the profile says so.
Set DSDGP_COLLAPSED_PROFILE=<file> for the table (profiles/collapsed_illcond.md).

Measured on an MI355X: every stage within 6 x the LAPACK chain's residual (largest 15 units of 2^-53); the device inside the family of
six on every quantity but the bound and the variance of grid1d (1.3 x and 2.5 x the family's largest member, bar 8 x): the family was
not extended.  Against dsdgp_trsm without its refinement step: L G L^T - psi2 at 168 (subset) and 206 (grid1d), L tmp1 - K(Z, X*) at
271 (subset) — the two cases fail."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import collapsed_reference as CR

pytestmark = pytest.mark.gpu

ALL_STAGES = CR.STAGES + CR.PREDICT_STAGES
_RUNS, _PROFILE = {}, {}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _inputs(name):
    return CR.ill_inputs(name) if name in CR.ILL_CASES else CR.inputs(name)


def device_statistics(layer, c):
    """dict(Kuu, psi0, psi1, psi2, Kus) as the layer's own calls form them, each call made twice: the same bits"""
    from doubly_stochastic_dgp import _lib, settings
    from doubly_stochastic_dgp.engine import ptr
    from doubly_stochastic_dgp.layers import kernel_expectations
    f = layer._factors
    ctx, M = f["ctx"], layer.num_inducing
    Xs = ctx.to_device(np.asarray(c["Xs"], dtype=np.float64))
    ns = Xs.shape[0]
    out = []
    for _ in range(2):
        Kuu, Kus = ctx.empty(M, M), ctx.empty(M, ns)
        _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(f["spec"]), ptr(f["Z"]), M, None, 0, float(settings.jitter), ptr(Kuu), M))
        _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(f["spec"]), ptr(f["Z"]), M, ptr(Xs), ns, 0.0, ptr(Kus), ns))
        psi0, psi1, psi2 = kernel_expectations(layer.kern, f["Z"], c["mu"], c["s"], on_device=True)
        ctx.sync()
        out.append(dict(Kuu=Kuu.cpu().numpy(), Kus=Kus.cpu().numpy(), psi0=float(psi0.cpu().numpy()[0]), psi1=psi1.cpu().numpy(), psi2=psi2.cpu().numpy()))
    for k in out[0]:
        assert _same_bits(out[0][k], out[1][k]), k
    assert _same_bits(out[0]["psi0"], f["psi0"].cpu().numpy()[0])
    return out[0]


def device_prediction_stages(layer, c):
    """tmp1 = L^-1 K(Z, X*), tmp2 = LB^-1 tmp1 by the calls of conditional_ND"""
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import ptr
    f = layer._factors
    ctx, M = f["ctx"], layer.num_inducing
    lib, h = ctx.lib, ctx.handle
    Xs = ctx.to_device(np.asarray(c["Xs"], dtype=np.float64))
    ns = Xs.shape[0]
    tmp1, tmp2 = ctx.empty(M, ns), ctx.empty(M, ns)
    _lib.check(lib.dsdgp_gram(h, C.byref(f["spec"]), ptr(f["Z"]), M, ptr(Xs), ns, 0.0, ptr(tmp1), ns))
    _lib.check(lib.dsdgp_trsm(h, 0, M, ns, ptr(f["L"]), M, ptr(tmp1), ns))
    _lib.check(lib.dsdgp_scale_copy(h, 0, M, ns, ptr(tmp1), ns, 1.0, 0.0, ptr(tmp2), ns))
    _lib.check(lib.dsdgp_trsm(h, 0, M, ns, ptr(f["LB"]), M, ptr(tmp2), ns))
    ctx.sync()
    return tmp1.cpu().numpy(), tmp2.cpu().numpy()


def run(name):
    """everything the device computes for a case, once per process"""
    if name not in _RUNS:
        from doubly_stochastic_dgp.gpflow_compat import RBF, Zero
        from doubly_stochastic_dgp.layers import SGPR_Layer
        c = _inputs(name)
        D, DY = c["mu"].shape[1], c["Y"].shape[1]
        layer = SGPR_Layer(RBF(D, variance=c["variance"], lengthscales=float(c["ls"][0])), c["Z"], DY, Zero())
        layer.set_data(c["mu"], c["s"], c["Y"], c["noise"])
        f = layer._factors
        f["ctx"].sync()
        fac = {k: f[k].cpu().numpy() for k in ("L", "G", "LB", "c")}
        st = device_statistics(layer, c)
        tmp1, tmp2 = device_prediction_stages(layer, c)
        bound, terms = layer.bound_terms()
        mean, var = layer.conditional_ND(c["Xs"], full_cov=False)
        mean2, cov = layer.conditional_ND(c["Xs"], full_cov=True)
        assert _same_bits(mean, mean2)
        dev = np.concatenate([CR.stage_residuals(st, c["Y"], c["noise"], fac["L"], fac["G"], fac["LB"], fac["c"]),
                              CR.predict_residuals(st["Kus"], fac["L"], fac["LB"], tmp1, tmp2)])
        _RUNS[name] = dict(c=c, st=st, fac=fac, bound=bound, terms=terms, mean=mean, var=var, cov=cov, stages=dev,
                           lapack=CR.lapack_chain_residuals(c, st), cond=float(np.linalg.cond(st["Kuu"])))
        _PROFILE.setdefault(name, {}).update(cond=_RUNS[name]["cond"], dev=dev, cpu=_RUNS[name]["lapack"])
    return _RUNS[name]


def stage_table():
    """the largest residual of the LAPACK chain, stage by stage, over the three ill-conditioned cases (on the device's statistics)"""
    return np.max(np.stack([run(n)["lapack"] for n in CR.ILL_NAMES]), axis=0)


def stage_bars(name):
    return 8.0 * np.maximum(run(name)["lapack"], stage_table())


@pytest.fixture(scope="module", autouse=True)
def profile_table():
    yield
    out = os.environ.get("DSDGP_COLLAPSED_PROFILE")
    if not out or not _PROFILE:
        return
    g = lambda v: "-" if v is None else f"{v:.3g}"
    with open(out, "w") as f:
        f.write("# SGPR_Layer's chain on ill-conditioned inducing inputs (tests/test_gpu_collapsed_illcond.py)\n\n"
                "Stage residuals: componentwise, units of 2^-53, scaled by the product of the magnitudes of the factors; `cpu` = the LAPACK / scipy chain on the\n"
                "device's own statistics.  Bar: 8 max(cpu, largest cpu over pairs / subset / grid1d).\n\n")
        hdr = ["case", "cond(Kuu)"] + [f"{s} {w}" for s in ALL_STAGES for w in ("dev", "cpu")]
        f.write("| " + " | ".join(hdr) + " |\n|" + "---|" * len(hdr) + "\n")
        for name, p in _PROFILE.items():
            if "dev" in p:
                f.write("| " + " | ".join([name, g(p["cond"])] + [g(v) for j in range(len(ALL_STAGES)) for v in (p["dev"][j], p["cpu"][j])]) + " |\n")
        f.write("\nEnd to end against the double-longdouble chain on the same statistics: bound in units of sum |terms|, mean in max |Y|, variance in the kernel variance.\n"
                "Family: float64 evaluations of the same statistics (written-out order, LAPACK, seeded permutations of the inducing inputs).  Bar: 8 max(family, 2^-50).\n\n")
        hdr = ["case", "quantity", "family members", "family smallest", "family largest", "device", "device / family largest"]
        f.write("| " + " | ".join(hdr) + " |\n|" + "---|" * len(hdr) + "\n")
        for name, p in _PROFILE.items():
            for q in p.get("end", []):
                f.write("| " + " | ".join([name, q[0], str(q[1]), g(q[2]), g(q[3]), g(q[4]), g(q[4] / q[3])]) + " |\n")
        f.write("\nAssembly of the bound from the device's LB, G, c: largest error of a term in units of sum |terms| (bar 8 x 2^-52 = 1.78e-15).\n\n| case | error |\n|---|---|\n")
        for name, p in _PROFILE.items():
            if "assembly" in p:
                f.write(f"| {name} | {g(p['assembly'])} |\n")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", CR.ILL_NAMES + CR.NAMES)
def test_stage_residuals(name):
    r = run(name)
    if name in CR.ILL_CASES:
        assert 1e6 <= r["cond"] <= 1e9
    bars = stage_bars(name)
    for j, what in enumerate(ALL_STAGES):
        print("%s  %s: device %.3g, LAPACK chain %.3g, bar %.3g (units of 2^-53)" % (name, what, r["stages"][j], r["lapack"][j], bars[j]))
    fac = r["fac"]
    assert np.all(np.isfinite(fac["L"])) and np.all(np.isfinite(fac["LB"])) and np.all(np.isfinite(fac["G"])) and np.all(np.isfinite(fac["c"]))
    assert np.all(np.triu(fac["L"], 1) == 0.0) and np.all(np.triu(fac["LB"], 1) == 0.0)
    assert np.all(r["stages"] <= bars), [(w, d, b) for w, d, b in zip(ALL_STAGES, r["stages"], bars) if d > b]


@pytest.mark.parametrize("name", CR.ILL_NAMES)
def test_assembly_of_the_bound(name):
    r = run(name)
    c, fac = r["c"], r["fac"]
    want = CR.assembly_terms(np.tril(fac["LB"]), fac["G"], fac["c"], c["Y"], r["st"]["psi0"], c["noise"])
    unit = float(np.sum(np.abs(want)))
    t = r["terms"]
    err = float(np.max(np.abs(t.astype(CR.LD) - want))) / unit
    _PROFILE.setdefault(name, {})["assembly"] = err
    print("%s: largest error of a term %.3g of sum |terms| = %.6g (bar %.3g)" % (name, err, unit, 8.0 * 2.0 ** -52))
    assert r["bound"] == ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5]
    assert err <= 8.0 * 2.0 ** -52


@pytest.mark.parametrize("name", CR.ILL_NAMES)
def test_bound_and_prediction_against_the_family(name):
    r = run(name)
    c, st = r["c"], r["st"]
    truth = CR.truth(c, st)
    assert r["mean"].shape == truth["mean"].shape and r["var"].shape == truth["var"].shape and r["cov"].shape == truth["cov"].shape
    dev = np.array(CR.errors(dict(bound=r["bound"], mean=r["mean"], var=r["var"], cov=r["cov"]), truth, c))
    members = CR.FAMILY
    fam = CR.family_errors(c, st, truth, members)
    inside = lambda: dev <= 8.0 * np.maximum(fam.max(axis=0), 2.0 ** -50)
    if not np.all(inside()) and np.all(r["stages"] <= stage_bars(name)):
        members = CR.FAMILY_MAX                       # every stage is backward stable: the six orders were lucky ones
        fam = CR.family_errors(c, st, truth, members)
    rows = []
    for j, what in enumerate(("bound", "mean", "var", "cov")):
        rows.append((what, members, fam[:, j].min(), fam[:, j].max(), dev[j]))
        print("%s %s: device %.3g; family of %d: %.3g .. %.3g; bar %.3g" % (name, what, dev[j], members, fam[:, j].min(), fam[:, j].max(),
                                                                         8.0 * max(fam[:, j].max(), 2.0 ** -50)))
    _PROFILE.setdefault(name, {})["end"] = rows
    assert np.all(inside()), list(zip(("bound", "mean", "var", "cov"), dev, 8.0 * np.maximum(fam.max(axis=0), 2.0 ** -50)))
    DY = c["Y"].shape[1]
    for d in range(1, DY):
        assert _same_bits(r["var"][..., d], r["var"][..., 0]) and _same_bits(r["cov"][..., d], r["cov"][..., 0])

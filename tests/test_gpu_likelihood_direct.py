"""The likelihood kernels of a training step driven directly: k_lik_elbo<F> (dsdgp_lik_elbo_readout) and k_multiclass with
k_scale_by_sample (dsdgp_multiclass_readout) on chosen (mean, var, target) inputs, and the public wrappers around the same formulas
(dsdgp_lik_var_exp / dsdgp_lik_predict, dsdgp_gauss_* / dsdgp_bernoulli_*, dsdgp_multiclass_var_exp), against the 20-point rule in
40-digit mpmath (tests/likelihood_reference.py) on the case table of tests/likelihood_cases.py.

Per case and quantity the measure |x - truth| / (eps scale) — scale = the sum of the magnitudes of the terms the formula adds — is at
most factor_reference.device_bar(the worse of the numpy and the torch comparator over the case) = 8 x that, never below 1.
Further: the part sums against the long-double sum of the truth; the layout (every shape gives the bits of the plain 1 x N x 1 call,
MBt is dmean transposed, padding +0.0, guard memory untouched); the quadrature-weight factor; the same bits on a second call; the model's
ELBO tied to the read-out; -inf, not NaN, where every component's density underflows.

DSDGP_LIK_PROFILE=<file> writes every measured value and bar as one table (profiles/likelihood_direct_errors.md)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from tests import likelihood_reference as LR
from tests.helpers import kern_spec, make_case
from tests.likelihood_cases import ELEMENT_CASES, LAYOUT_SHAPES, MULTICLASS_CASES, layout_inputs, targets

pytestmark = pytest.mark.gpu

EPS = LR.EPS
LDB = np.longdouble


def _code(kind):
    from doubly_stochastic_dgp import _lib
    return {"gaussian": _lib.LIK_GAUSSIAN, "bernoulli": _lib.LIK_BERNOULLI, "poisson": _lib.LIK_POISSON, "exponential": _lib.LIK_EXPONENTIAL,
            "student_t": _lib.LIK_STUDENT_T, "gamma": _lib.LIK_GAMMA, "beta": _lib.LIK_BETA}[kind]


def _ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


def readout(kind, p0, p1, mean, var, Y, **kw):
    from doubly_stochastic_dgp.utils import lik_elbo_readout
    return lik_elbo_readout(_code(kind), p0, p1, mean, var, Y, **kw)


def per_element(kind, p0, p1, mu, v, y):
    """one launch of the read-out per element (n = S = DY = 1, w = 1): its part pair is the element's own (ve, d ve / d p0), and the
    adjoints are -d ve / d mean, -d ve / d var -> dict of flat arrays ve, dp0, dmean, dvar"""
    from doubly_stochastic_dgp import _lib
    ctx = _ctx()
    n = mu.size
    m, vv, yy = ctx.to_device(mu), ctx.to_device(v), ctx.to_device(y)
    part, dm, dv = ctx.empty(2 * n), ctx.empty(n), ctx.empty(n)
    code = _code(kind)
    at = lambda t, i: C.c_void_p(t.data_ptr() + 8 * i)
    for i in range(n):
        _lib.check(ctx.lib.dsdgp_lik_elbo_readout(ctx.handle, code, p0, p1, at(m, i), at(vv, i), at(yy, i), 1, 1, 1, 1.0, None, at(part, 2 * i),
                                                  at(dm, i), at(dv, i), None, None, 16))
    ctx.sync()
    part = part.cpu().numpy().reshape(n, 2)
    return dict(ve=part[:, 0], dp0=part[:, 1], dmean=dm.cpu().numpy(), dvar=dv.cpu().numpy())


def public_calls(kind, p0, p1, mu, v, y):
    """the public wrappers on the same elements as a 1 x n x 1 problem -> ve (mode 0), ld (mode 1), pm, pv"""
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import ptr
    ctx = _ctx()
    n = mu.size
    m, vv, yy = ctx.to_device(mu), ctx.to_device(v), ctx.to_device(y)
    o0, o1, om, ov = ctx.empty(n), ctx.empty(n), ctx.empty(n), ctx.empty(n)
    h, L = ctx.handle, ctx.lib
    if kind == "gaussian":
        _lib.check(L.dsdgp_gauss_var_exp(h, ptr(m), ptr(vv), ptr(yy), n, 1, 1, p0, None, ptr(o0)))
        _lib.check(L.dsdgp_gauss_predict_density(h, ptr(m), ptr(vv), ptr(yy), n, 1, 1, p0, ptr(o1)))
        _lib.check(L.dsdgp_add_scalar(h, ptr(vv), p0, n, ptr(ov)))
        om = m
    elif kind == "bernoulli":
        _lib.check(L.dsdgp_bernoulli_var_exp(h, ptr(m), ptr(vv), ptr(yy), n, 1, 1, 0, None, ptr(o0)))
        _lib.check(L.dsdgp_bernoulli_var_exp(h, ptr(m), ptr(vv), ptr(yy), n, 1, 1, 1, None, ptr(o1)))
        _lib.check(L.dsdgp_bernoulli_predict(h, ptr(m), ptr(vv), n, ptr(om), ptr(ov)))
    else:
        code = _code(kind)
        _lib.check(L.dsdgp_lik_var_exp(h, code, p0, p1, ptr(m), ptr(vv), ptr(yy), n, 1, 1, 0, None, ptr(o0)))
        _lib.check(L.dsdgp_lik_var_exp(h, code, p0, p1, ptr(m), ptr(vv), ptr(yy), n, 1, 1, 1, None, ptr(o1)))
        _lib.check(L.dsdgp_lik_predict(h, code, p0, p1, ptr(m), ptr(vv), n, ptr(om), ptr(ov)))
    ctx.sync()
    return dict(ve=o0.cpu().numpy(), ld=o1.cpu().numpy(), pm=om.cpu().numpy(), pv=ov.cpu().numpy())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------ the profile table
_ROWS = []
_NOTES = []


@pytest.fixture(scope="module", autouse=True)
def profile_table():
    t0 = time.time()
    yield
    path = os.environ.get("DSDGP_LIK_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# The likelihood kernels of a training step against the 20-point rule in 40-digit mpmath (tests/test_gpu_likelihood_direct.py)\n\n"
                "Worst `|x - truth| / (eps scale)` per case and quantity, scale = the sum of the magnitudes of the terms the formula adds\n"
                "(tests/likelihood_reference.py).  `dev` = the device, `numpy` / `torch` = the two float64 CPU comparators of the same formulas,\n"
                "`bar` = 8 x the larger of the two, never below 1.  `route`: `elbo` = k_lik_elbo / k_multiclass through the read-out entry points\n"
                "(ve and dp0 from one-element launches, dmu / dv = the negated adjoints at w = 1), `public` = dsdgp_lik_var_exp / dsdgp_lik_predict,\n"
                "the Gaussian / Bernoulli wrappers, dsdgp_multiclass_var_exp.\n\n"
                "| case | n | route | quantity | dev | numpy | torch | bar |\n|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| " + " | ".join(r) + " |\n")
        f.write("\n## Notes\n\n")
        for n in _NOTES + STANDING_NOTES:
            f.write(f"- {n}\n")
        f.write(f"\n{len(_ROWS)} rows, {time.time() - t0:.0f} s for the module.\n")


STANDING_NOTES = [
    "dv is not measured at v = 0 (upstream's sqrt has no finite gradient there; the value is), dvar of MultiClass not at an exact tie with "
    "a clip (v_k = 1e-10, v_y = 0.5e-10).",
    f"ld (log predictive density by the rule) is measured where the truth exceeds {LR.LD_FLOOR:g}: below it float64's exp leaves the normal "
    "range inside the rule and upstream's own result is denormal-limited or -inf; there the device must give -inf or a finite value "
    "below the floor + 10, never NaN.",
    "The case nearest its bar is dp0 of gamma-shape1 (sub-case mu = 0, y = 1: dp0 = -digamma(1)): digamma_d's recurrence adds seven "
    "reciprocals (2.59) to log(8) - ... (2.02) to give -0.577, a cancellation that the scale |digamma| does not see and scipy's psi does "
    "not have; the absolute error stays inside the 1e-15 likelihood.hpp states.  With the recurrence stopped at 6 instead of 8 the same "
    "case measures 1.03e3 (gamma-shape7.9: 3 against 2.6; gamma-ordinary, beta-ordinary, beta-scale1 fail dp0 as well), and with "
    "StudentT's dv negated student_t-ordinary and student_t-small-v fail dv (both tried on a scratch build).",
    "Quadrature weights: k_lik_elbo multiplies the finished derivative by c = -w f; at w = 1 the weighted adjoints have the bits of the "
    "unweighted ones times f (asserted exactly, both forms; the Gaussian against (c (y - mu)) / p0 and (-0.5 c) / p0 in numpy).  MultiClass "
    "applies f in a second launch, after rounding: within one ulp of the float64-scaled unweighted call.",
]


def hold(name, n, route, got, T, quantities, masks=None):
    """measure every quantity of `got` against the truth, record the row, then assert the bars"""
    fails = []
    for q, x in got.items():
        if q not in quantities:
            continue
        sel = (masks or T["masks"])[q]
        val, sc = T["truth"][q]
        m = LR.measure(np.asarray(x).reshape(val.shape)[sel], (val[sel], sc[sel]))
        row = [name, str(n), route, q, f"{m:.3g}", f"{T['numpy'][q]:.3g}", f"{T['torch'][q]:.3g}", f"{T['bars'][q]:.3g}"]
        print("LIK_DIRECT | " + " | ".join(row))
        _ROWS.append(row)
        if not m <= T["bars"][q]:
            fails.append(f"{name} [{route}] {q}: {m:.3g} > bar {T['bars'][q]:.3g}")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ element-wise kinds against the truth
@pytest.mark.parametrize("case", ELEMENT_CASES, ids=lambda c: c["name"])
def test_elementwise_against_the_truth(case):
    kind, p0, p1, mu, v, y = (case[k] for k in ("kind", "p0", "p1", "mu", "v", "y"))
    n = mu.size
    T = LR.element_truth(case)
    el = per_element(kind, p0, p1, mu, v, y)
    pub = public_calls(kind, p0, p1, mu, v, y)
    # the batch launch: the same adjoint bits as the one-element launches, in both forms
    rows = readout(kind, p0, p1, mu.reshape(1, n, 1), v.reshape(1, n, 1), y.reshape(n, 1))
    tr = readout(kind, p0, p1, mu.reshape(1, n, 1), v.reshape(1, n, 1), y.reshape(n, 1), transposed=True)
    ok = case["v"] >= 0
    for a, b in ((rows["dmean"].ravel(), el["dmean"]), (rows["dvar"].ravel(), el["dvar"]), (tr["MBt"][0, :n], el["dmean"]),
                 (tr["VBt"][0, :n], el["dvar"])):
        assert same_bits(a[ok], b[ok]), case["name"]
    assert same_bits(rows["part"], tr["part"][:rows["part"].shape[0]])
    hold(case["name"], n, "elbo", dict(ve=el["ve"], dmu=-el["dmean"], dv=-el["dvar"], dp0=el["dp0"]), T, ("ve", "dmu", "dv", "dp0"))
    hold(case["name"], n, "public", pub, T, ("ve", "ld", "pm", "pv"))
    low = ~T["masks"]["ld"]
    assert not np.any(np.isnan(pub["ld"][low])) and np.all(pub["ld"][low] <= LR.LD_FLOOR + 10.0), "ld below the floor"
    # part sums: the long-double sum of the truth; allowance = the elements' bars + the summation's own count eps sum|terms|
    for col, q in ((0, "ve"), (1, "dp0")):
        val, sc = T["truth"][q]
        got = float(np.sum(rows["part"][:, col].astype(LDB)))
        allow = EPS * (T["bars"][q] * float(np.sum(sc)) + min(n, 256 + rows["part"].shape[0]) * float(np.sum(np.abs(val))))
        assert abs(LDB(got) - np.sum(val)) <= allow, (case["name"], q, got, float(np.sum(val)), allow)
        if case["kind"] not in LR.HAS_PARAM and col == 1:
            assert np.all(rows["part"][:, 1] == 0.0)


# ------------------------------------------------------------------------------------------------ MultiClass against the truth
def mc_readout(case, **kw):
    from doubly_stochastic_dgp.utils import multiclass_readout
    return multiclass_readout(case["mean"], case["var"], case["labels"], **kw)


def mc_public(case, mode):
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import ptr
    ctx = _ctx()
    S, N, K = case["mean"].shape
    # as an S = 1 problem over the S N rows (the labels tiled): per-row values, no reduction over the samples
    m, v = ctx.to_device(case["mean"].reshape(1, S * N, K)), ctx.to_device(case["var"].reshape(1, S * N, K))
    y = ctx.to_device(np.tile(case["labels"], (S, 1)))
    out = ctx.empty(S * N)
    _lib.check(ctx.lib.dsdgp_multiclass_var_exp(ctx.handle, ptr(m), ptr(v), ptr(y), S * N, 1, K, mode, None, ptr(out)))
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", MULTICLASS_CASES, ids=lambda c: c["name"])
def test_multiclass_against_the_truth(case):
    S, N, K = case["mean"].shape
    R = S * N
    T = LR.multiclass_truth(case)
    got = mc_readout(case, guard=64)
    for k in ("ve", "dmean", "dvar"):
        assert np.all(got[k + "_guard"] == got["ve_guard"][0]) and got["ve_guard"][0] < -1e70, f"{k}: memory past R K written"
    hold(case["name"], R, "elbo", dict(ve=got["ve"].ravel(), dmean=got["dmean"].reshape(R, K), dvar=got["dvar"].reshape(R, K)), T,
         ("ve", "dmean", "dvar"))
    hold(case["name"], R, "public", dict(ve=mc_public(case, 0), ld=mc_public(case, 1)), T, ("ve", "ld"))
    # the gradient gates of the clips: exactly zero on the clipped side
    var = case["var"].reshape(R, K)
    is_y = np.arange(K)[None, :] == T["labels"][:, None]
    gated = np.where(is_y, var < 0.5e-10, var < 1e-10)
    assert np.all(got["dvar"].reshape(R, K)[gated] == 0.0)
    again = mc_readout(case)
    assert all(same_bits(again[k], got[k]) for k in ("ve", "dmean", "dvar")), "a second call gives other bits"


def test_multiclass_wrapper_refuses_bad_labels_on_the_host():
    from doubly_stochastic_dgp.utils import multiclass_readout
    mean, var = np.zeros((1, 3, 4)), np.ones((1, 3, 4))
    for bad in ([[0.0], [4.0], [1.0]], [[0.0], [-1.0], [1.0]], [[0.5], [1.0], [2.0]], [[np.nan], [1.0], [2.0]]):
        with pytest.raises(ValueError, match="integer labels"):
            multiclass_readout(mean, var, np.array(bad))
    with pytest.raises(ValueError):
        multiclass_readout(mean, var, np.zeros((3, 2)))


# ------------------------------------------------------------------------------------------------ layout, exact
@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "student_t"])
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_is_exact(kind, shape):
    S, n, DY = shape
    p0, p1 = {"gaussian": (0.7, 1.0), "bernoulli": (1.0, 1.0), "student_t": (1.3, 3.0)}[kind]
    mu, v, Y, yflat = layout_inputs(kind, shape)
    total, R = S * n * DY, S * n
    ldt = -(-R // 16) * 16
    plain = readout(kind, p0, p1, mu.reshape(1, total, 1), v.reshape(1, total, 1), yflat.reshape(total, 1), w=0.375)
    rows = readout(kind, p0, p1, mu, v, Y, w=0.375, guard=40)
    tr = readout(kind, p0, p1, mu, v, Y, w=0.375, transposed=True, guard=40)
    val = readout(kind, p0, p1, mu, v, Y, w=0.375, adjoints=False)
    assert same_bits(rows["dmean"].ravel(), plain["dmean"].ravel()) and same_bits(rows["dvar"].ravel(), plain["dvar"].ravel())
    assert same_bits(rows["part"], plain["part"]) and same_bits(val["part"], plain["part"])
    assert tr["MBt"].shape == (DY, ldt)
    assert same_bits(tr["MBt"][:, :R].T, rows["dmean"].reshape(R, DY)) and same_bits(tr["VBt"][:, :R].T, rows["dvar"].reshape(R, DY))
    for k in ("MBt", "VBt"):
        assert same_bits(tr[k][:, R:], np.zeros((DY, ldt - R))), f"{k}: padding rows are not +0.0"
    nb = rows["part"].shape[0]
    assert tr["part"].shape[0] == -(-(ldt * DY) // 256) and same_bits(tr["part"][:nb], rows["part"])
    assert same_bits(tr["part"][nb:], np.zeros((tr["part"].shape[0] - nb, 2))), "a block of padding alone sums to +0.0"
    if shape == (1, 33, 20):
        assert tr["part"].shape[0] == nb + 1
    for out in (rows, tr):
        for k, g in out.items():
            if k.endswith("_guard"):
                assert g.size == 40 and np.all(g == g[0]) and g[0] < -1e70, f"{k}: memory past the output written"
    again = readout(kind, p0, p1, mu, v, Y, w=0.375, transposed=True)
    assert all(same_bits(again[k], tr[k]) for k in ("part", "MBt", "VBt")), "a second call gives other bits"


# ------------------------------------------------------------------------------------------------ quadrature weights
def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "student_t", "beta"])
def test_quadrature_weight_factor_elementwise(kind):
    """adjoints and values carry f = sw[s] S at DY = 3, exactly: the kernel multiplies the finished derivative d by c = -w f, so at
    w = 1 its adjoint is the one rounding of -f d that the unweighted adjoint -d times f is in float64.  The Gaussian's adjoints are
    rounded as (c (y - mu)) / p0 and (-0.5 c) / p0 (likelihood.hpp): the same expressions in numpy."""
    S, n, DY = 4, 23, 3
    p0, p1 = {"gaussian": (0.7, 1.0), "bernoulli": (1.0, 1.0), "student_t": (1.3, 3.0), "beta": (3.5, 1.0)}[kind]
    rng = np.random.RandomState(11)
    mu, v = 1.2 * rng.randn(S, n, DY), rng.uniform(1e-6, 2.0, size=(S, n, DY))
    Y = targets(kind, rng, n * DY).reshape(n, DY)
    base = readout(kind, p0, p1, mu, v, Y, w=1.0)
    for sw in (np.array([0.5, 0.125, 2.0, 0.25]) / S, rng.uniform(0.05, 0.6, size=S)):
        f = (sw * S)[:, None, None]
        want_m, want_v = base["dmean"] * f, base["dvar"] * f
        if kind == "gaussian":
            c = -(1.0 * f)
            want_m, want_v = (c * (Y[None] - mu)) / p0, np.broadcast_to((-0.5 * c) / p0, mu.shape)
        for form in (False, True):
            got = readout(kind, p0, p1, mu, v, Y, w=1.0, weights=sw, transposed=form)
            dm = got["MBt"][:, :S * n].T.reshape(S, n, DY) if form else got["dmean"]
            dv = got["VBt"][:, :S * n].T.reshape(S, n, DY) if form else got["dvar"]
            assert same_bits(dm, want_m) and same_bits(dv, want_v), (kind, float(np.max(_ulps(dm, want_m))), float(np.max(_ulps(dv, want_v))))
        # the block sums: sum f ve against the float64-scaled per-element values of the public call, the summation's own allowance
        pub = public_calls(kind, p0, p1, mu.ravel(), v.ravel(), np.tile(Y.ravel(), S))["ve"].reshape(S, n, DY)
        want = np.sum((pub * f).astype(LDB))
        assert abs(np.sum(got["part"][:, 0].astype(LDB)) - want) <= 3 * 256 * EPS * float(np.sum(np.abs(pub * f)))


def test_quadrature_weight_factor_multiclass():
    """K = 10: the factor is applied by a second launch, after rounding — one ulp against the unweighted call scaled in float64"""
    rng = np.random.RandomState(12)
    S, N, K = 4, 9, 10
    case = dict(mean=1.5 * rng.randn(S, N, K), var=rng.uniform(0.05, 2.0, size=(S, N, K)), labels=(np.arange(N) % K).astype(np.float64).reshape(N, 1))
    base = mc_readout(case, w=0.375)
    sw = rng.uniform(0.05, 0.6, size=S)
    got = mc_readout(case, w=0.375, weights=sw)
    f = sw * S
    assert np.max(_ulps(got["ve"], base["ve"] * f[:, None])) <= 1.0
    assert np.max(_ulps(got["dmean"], base["dmean"] * f[:, None, None])) <= 1.0
    assert np.max(_ulps(got["dvar"], base["dvar"] * f[:, None, None])) <= 1.0
    pub = ctx_multiclass_weighted(case, sw)                     # sum_s sw[s] ve_s = the read-out's sum_s f_s ve_s / S
    want = np.sum((got["ve"].astype(LDB)), axis=0) / S
    assert np.max(np.abs(pub.ravel().astype(LDB) - want)) <= 4 * S * EPS * float(np.max(np.sum(np.abs(got["ve"]), axis=0))) / S


def ctx_multiclass_weighted(case, sw):
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import ptr
    ctx = _ctx()
    S, N, K = case["mean"].shape
    m, v, y, w = ctx.to_device(case["mean"]), ctx.to_device(case["var"]), ctx.to_device(case["labels"]), ctx.to_device(sw)
    out = ctx.empty(N)
    _lib.check(ctx.lib.dsdgp_multiclass_var_exp(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, K, 0, ptr(w), ptr(out)))
    ctx.sync()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the tie to the model
@pytest.mark.parametrize("family", ["gaussian", "bernoulli", "student_t", "multiclass"])
def test_model_elbo_is_the_readout_on_its_own_predictions(family):
    """one-layer model: ELBO + sum KL = w sum(part) of the read-out on the model's own predict mean / var, w = num_data / (n S).
    Allowance: 16 eps of the sum of the magnitudes of everything that is added (the elements' terms, weighted) — the model's k_finalize
    and this test add the block sums in different orders, and the forward pass of the two calls is the same launch sequence."""
    rng = np.random.RandomState(31)
    N, D, M, S = 40, 2, 12, 3
    X = rng.randn(N, D)
    Z = X[:M].copy()
    kw = {}
    if family == "multiclass":
        K = 4
        Y = (np.arange(N) % K).astype(np.float64).reshape(N, 1)
        kw = dict(num_classes=K)
    elif family == "bernoulli":
        Y, kw = np.where(rng.uniform(size=(N, 2)) < 0.5, -1.0, 1.0), dict(bernoulli=True)
    elif family == "student_t":
        Y, kw = rng.standard_t(4.0, size=(N, 2)), dict(likelihood="student_t", lik_aux=4.5, lik_var=0.7)
    else:
        Y, kw = rng.randn(N, 2), dict(lik_var=0.3)
    spec, state, model = make_case(X, Y, Z, [kern_spec("rbf", D, 1.0, 0.8)], S=S, num_data=100, **kw)
    DY = model.layers[-1].num_outputs
    zs = [rng.randn(S, N, DY)]
    w = 100.0 / (N * S)
    eng = model.engine()
    model._build_likelihood(X, Y, zs=zs)
    out = eng.elbo(X, Y, S, zs=zs, data_scale=100.0 / N)
    mean, var = model._build_predict(X, S=S, zs=zs)
    if family == "multiclass":
        got = mc_readout(dict(mean=mean, var=var, labels=Y), w=w)
        terms = got["ve"].ravel()
        mags = np.abs(terms)
    else:
        p0, p1 = {"gaussian": (0.3, 1.0), "bernoulli": (1.0, 1.0), "student_t": (0.7, 4.5)}[family]
        p0 = float(model.likelihood.likelihood.variance.value) if family == "gaussian" else (
            float(model.likelihood.likelihood.scale.value) if family == "student_t" else p0)
        terms = readout(family, p0, p1, mean, var, Y, w=w, adjoints=False)["part"][:, 0]
        yt = np.tile(Y.ravel(), S)
        mags = LR.elementwise(LR.NPB, family, mean.ravel(), var.ravel(), yt, p0, p1, which=("ve",))["ve"][1]
    data = float(w * np.sum(terms.astype(LDB)))
    allow = 16 * EPS * (w * float(np.sum(mags)) + abs(out[2]))
    print(f"LIK_DIRECT tie {family}: model {out[0] + out[2]!r} readout {data!r} allowance {allow:.3g}")
    assert abs((out[0] + out[2]) - data) <= allow, (family, out[0] + out[2], data, allow)
    assert abs(out[1] - data) <= allow


# ------------------------------------------------------------------------------------------------ density underflow
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("kind,mu0,v0,y0", [("exponential", -8.0, 1e-4, 1.0), ("poisson", 0.0, 0.1, 400.0)])
def test_underflowed_density_is_minus_infinity(kind, mu0, v0, y0, S):
    """every component's density underflows: logsumexp gives -inf, as the oracle and scipy do, not NaN; the finite neighbour keeps the
    value it has on its own"""
    from oracle import dgp_oracle as O
    from scipy.special import logsumexp
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import ptr
    ctx = _ctx()
    mu = np.empty((S, 2, 1))
    mu[:, 0, 0], mu[:, 1, 0] = mu0, 0.3 + 0.1 * np.arange(S)
    v = np.empty((S, 2, 1))
    v[:, 0, 0], v[:, 1, 0] = v0, 0.2
    Y = np.array([[y0], [1.0]])
    ol = O.Exponential() if kind == "exponential" else O.Poisson(1.0)
    with np.errstate(all="ignore"):
        ref = logsumexp(ol.predict_density(O.NP, mu, v, Y), axis=0) - np.log(S)
    assert ref[0, 0] == -np.inf and np.isfinite(ref[1, 0])

    def run(m_, v_, y_):
        a, b, c = ctx.to_device(m_), ctx.to_device(v_), ctx.to_device(y_)
        out = ctx.empty(y_.shape[0])
        _lib.check(ctx.lib.dsdgp_lik_var_exp(ctx.handle, _code(kind), 1.0, 1.0, ptr(a), ptr(b), ptr(c), y_.shape[0], S, 1, 1, None, ptr(out)))
        ctx.sync()
        return out.cpu().numpy()

    got = run(mu, v, Y)
    alone = run(mu[:, 1:], v[:, 1:], Y[1:])
    assert got[0] == -np.inf, got
    assert same_bits(got[1:], alone) and abs(got[1] - ref[1, 0]) <= 1e-12 * abs(ref[1, 0])


def test_multiclass_density_reduction_keeps_its_bits_on_finite_input():
    """k_over_samples' guarded sum: the ordinary logsumexp over S = 3 components against scipy on the per-row device densities"""
    from scipy.special import logsumexp
    case = next(c for c in MULTICLASS_CASES if c["name"] == "mc-ordinary-K3-R33")
    S, N, K = case["mean"].shape
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import ptr
    ctx = _ctx()
    m, v, y = ctx.to_device(case["mean"]), ctx.to_device(case["var"]), ctx.to_device(case["labels"])
    out = ctx.empty(N)
    _lib.check(ctx.lib.dsdgp_multiclass_var_exp(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, K, 1, None, ptr(out)))
    ctx.sync()
    rows = mc_public(case, 1).reshape(S, N)
    assert np.max(np.abs(out.cpu().numpy() - (logsumexp(rows, axis=0) - np.log(S)))) <= 4 * EPS * np.max(np.abs(rows))

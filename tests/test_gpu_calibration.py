"""-m gpu: calibration of the predictive mixture on the device (csrc/calibration.hip; dsdgp_mixture_quantiles, dsdgp_mixture_calibration,
dsdgp_model_quantiles, dsdgp_model_calibration, DGP_Base.predict_quantiles / calibration) against tests/calibration_reference.py.

Quantiles.  A returned q is held to the normalised residual rho = |F_mp(q) - p| / (4 eps + spacing(q) f_mp(q)) with F_mp, f_mp the
mixture's distribution function and density in 40-digit mpmath: 4 eps is what a handful of rounded erfc values can move F, the second
term what one ulp of q moves it.  The bar is 8 x the worst rho the float64 CPU solver of the helper reaches on a fixed panel of the
inputs below (the issue's small shapes, the gap and the spikes case), computed once per run — the factor tests/test_gpu_natgrad_direct.py
gives a device kernel over float64 CPU versions.  The mpmath check runs on a fixed-stride subsample of (item, p) pairs per case, the
first and the last item always among them: at most 2000 pairs, and at most 6000 component evaluations (S = 100: 60 pairs; one costs
about 0.1 ms), which keeps a case to a second or two; the CPU solver's own rho per case is computed only for the profile.  Every item is also held to the CPU solver's q within 2 * 4 eps / f(q) + 2 spacing(q).
DSDGP_CALIBRATION_PROFILE=<file> writes the measured worst rho, CPU and device, per case (profiles/calibration_residuals.md).

PIT and CRPS: rtol 1e-10 / atol 1e-13 per row (the TOL of tests/test_gpu_evaluate.py), sums over n rows n times the absolute part, the
counts #(u <= p_k) and the row count exact (no reference u lies within 1e-9 of a p_k: asserted).

Shapes on both sides of every boundary of the kernel: lanes per item (1 / 4 / 8 / 16: by the item count at 4096, 8192 and 32768, lowered
by S at 4, 8 and 16, raised by S past 8 components per lane at 8 | 9, 32 | 33, 64 | 65), components staged in LDS vs read from global
memory (16 lanes x 8: 128 | 129), one vs several workgroups (16 lanes: 16 | 17 items), P = 1 and P = 16.  The kernel has no unrolled
component loop, hence no unroll remainder."""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import calibration_reference as R
from tests.helpers import kern_spec, make_case
from tests.mixture_cases import NS, _build_case, _case, run_child

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-13)
PROBS = (1e-6, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0 - 1e-6)
UNSUPPORTED, BAD_ARG = -4, -1
CANARY = -12345.25
MP_PAIRS, MP_COMPONENTS = 2000, 6000
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_CALIBRATION_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Quantiles of the Gaussian mixture: normalised residuals (tests/test_gpu_calibration.py)\n\n"
                "rho = |F_mp(q) - p| / (4 eps + spacing(q) f_mp(q)), F_mp / f_mp in 40-digit mpmath; the worst over the case's subsample of\n"
                "(item, p) pairs.  `cpu`: the float64 solver of tests/calibration_reference.py, `device`: dsdgp_mixture_quantiles, `bar`: 8 x\n"
                "the CPU solver's worst rho on the fixed panel.\n\n| case | pairs | cpu | device | bar |\n|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %d | %.3g | %.3g | %.3g |\n" % r)


def _p(a):
    return C.c_void_p(a.data_ptr() if a is not None else 0)


def _hp(probs):
    h = np.ascontiguousarray(probs, dtype=np.float64)
    return h, h.ctypes.data_as(C.POINTER(C.c_double))


def _quant(ctx, mean, var, noise, probs=PROBS):
    """dsdgp_mixture_quantiles -> ((n, DY, P) numpy or None, return code); a canary behind q_out must survive"""
    S, N, D = mean.shape
    h, hp = _hp(probs)
    m, v = ctx.to_device(mean), ctx.to_device(var)
    q = ctx.empty(N * D * h.size + 8)
    with ctx.torch.cuda.stream(ctx.tstream):
        q.fill_(CANARY)
    rc = ctx.lib.dsdgp_mixture_quantiles(ctx.handle, _p(m), _p(v), float(noise), N, S, D, hp, h.size, _p(q))
    ctx.sync()
    if rc != 0:
        return None, rc
    host = q.cpu().numpy()
    assert np.all(host[N * D * h.size:] == CANARY), "dsdgp_mixture_quantiles wrote past q_out"
    return host[:N * D * h.size].reshape(N, D, h.size), rc


def _calib(ctx, mean, var, noise, Y, probs=PROBS, acc=None, accumulate=0, want_rows=True):
    """dsdgp_mixture_calibration -> (acc (2 + P, D) device tensor, rows (N, D, 2) numpy or None, return code)"""
    S, N, D = mean.shape
    h, hp = _hp(probs)
    m, v, y = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(Y)
    if acc is None:
        acc = ctx.empty(2 + h.size, D)
    rows = ctx.empty(N * D * 2 + 8) if want_rows else None
    if want_rows:
        with ctx.torch.cuda.stream(ctx.tstream):
            rows.fill_(CANARY)
    rc = ctx.lib.dsdgp_mixture_calibration(ctx.handle, _p(m), _p(v), float(noise), _p(y), N, S, D, hp, h.size, _p(rows), _p(acc),
                                           accumulate)
    ctx.sync()
    if rc != 0 or not want_rows:
        return acc, None, rc
    host = rows.cpu().numpy()
    assert np.all(host[N * D * 2:] == CANARY), "dsdgp_mixture_calibration wrote past rows_out"
    return acc, host[:N * D * 2].reshape(N, D, 2), rc


def _inputs(n, DY, S, idx=None):
    """mean ~ scale randn, scale in {0.1, 1, 10}, every second case shifted by 100; var ~ U(0.01, 1.5); noise in {0, 0.3}; Y drawn from
    the mixture itself.  -> (mean, var, noise, Y)"""
    if idx is None:
        idx = n + DY + S
    rng = np.random.RandomState(100000 + 1000 * idx + 7 * n + 3 * DY + S)
    scale, shift, noise = (0.1, 1.0, 10.0)[idx % 3], 100.0 * (idx % 2), (0.0, 0.3)[(idx // 2) % 2]
    mean = scale * rng.randn(S, n, DY) + shift
    var = rng.uniform(0.01, 1.5, size=(S, n, DY))
    comp = rng.randint(0, S, size=(n, DY))
    ii, dd = np.meshgrid(np.arange(n), np.arange(DY), indexing="ij")
    Y = mean[comp, ii, dd] + np.sqrt(var[comp, ii, dd] + noise) * rng.randn(n, DY)
    return mean, var, noise, Y


def _gap_case():
    """two groups of four unit-variance components at -30 and +30: p = 0.5 falls into the gap, where F = 1/2 to 200 digits"""
    rng = np.random.RandomState(21)
    mean = np.concatenate([-30.0 + 0.1 * rng.randn(4, 3, 1), 30.0 + 0.1 * rng.randn(4, 3, 1)])
    return mean, np.ones_like(mean), 0.0


def _spikes_case():
    mean = np.array([-5.0, 5.0, 0.0]).reshape(3, 1, 1)
    sd = np.array([1e-3, 1e-3, 3.0]).reshape(3, 1, 1)
    return mean, sd ** 2, 0.0


def _pairs(nitems, P, S):
    """fixed-stride subsample of the flat (item, k) pairs, the first and the last item's included"""
    total = nitems * P
    want = max(3 * P, min(MP_PAIRS, MP_COMPONENTS // S))
    if total <= want:
        return [(j, k) for j in range(nitems) for k in range(P)]
    stride = -(-total // (want - 2 * P))
    if stride % P == 0:      # (a stride that is a multiple of P would visit one probability only)
        stride += 1
    flat = set(range(0, total, stride)) | set(range(P)) | set(range(total - P, total))
    return [(f // P, f % P) for f in sorted(flat)]


def _worst_rho(q, mu, sg, probs, pairs):
    """q (n, DY, P), mu / sg (S, n, DY): the worst rho over the pairs (item = flat (i, d))"""
    S = mu.shape[0]
    mu2, sg2, q2 = mu.reshape(S, -1), sg.reshape(S, -1), q.reshape(-1, len(probs))
    return max(R.residual(q2[j, k], probs[k], mu2[:, j], sg2[:, j]) for j, k in pairs)


@pytest.fixture(scope="module")
def cpu_panel_rho():
    """the float64 CPU solver's worst rho on a fixed panel: the issue's small shapes (their first items), the gap and the spikes case"""
    worst = 0.0
    panel = [_inputs(n, DY, S)[:3] for n, DY, S in [(1, 1, 1), (37, 3, 3), (37, 1, 2), (37, 1, 17), (23, 7, 20)]]
    panel += [_inputs(8, 1, S, idx)[:3] for idx, S in enumerate((1, 2, 5, 9, 30, 100))]
    panel += [_gap_case(), _spikes_case()]
    for mean, var, noise in panel:
        mu, sg = mean, R.sigma(var, noise)
        q = R.quantiles(mu, sg, PROBS)
        nitems = mu[0].size
        pairs = [(j, k) for j in range(min(nitems, 8)) for k in range(len(PROBS))]
        worst = max(worst, _worst_rho(q, mu, sg, PROBS, pairs))
    print("CPU solver, worst rho on the panel:", worst)
    assert 0.05 < worst < 4.0, worst      # (a solver that converges: a residual of the order of one rounding)
    return worst


def _check_quantiles(name, q, mean, var, noise, probs, cpu_panel_rho, monotone=True):
    mu, sg = mean, R.sigma(var, noise)
    assert np.all(np.isfinite(q))
    ref = R.quantiles(mu, sg, probs)
    # every item against the CPU solver
    with np.errstate(divide="ignore", over="ignore"):
        f = np.stack([R.pdf(ref[..., k], mu, sg) for k in range(len(probs))], axis=-1)
        tol = 2.0 * R.bar_F() / f + 2.0 * np.spacing(np.abs(ref))
    bad = np.abs(q - ref) > tol
    assert not bad.any(), (name, np.argwhere(bad)[:5], q[bad][:5], ref[bad][:5])
    # the subsample against mpmath
    pairs = _pairs(mu[0].size, len(probs), mu.shape[0])
    rho_dev = _worst_rho(q, mu, sg, probs, pairs)
    rho_cpu = _worst_rho(ref, mu, sg, probs, pairs) if os.environ.get("DSDGP_CALIBRATION_PROFILE") else float("nan")
    bar = 8.0 * cpu_panel_rho
    print(f"{name}: {len(pairs)} pairs, worst rho cpu {rho_cpu:.3g} device {rho_dev:.3g} bar {bar:.3g}")
    _ROWS.append((name, len(pairs), rho_cpu, rho_dev, bar))
    assert rho_dev <= bar, (name, rho_dev, bar)
    if monotone:
        order = np.argsort(probs)
        assert np.all(np.diff(ref[..., order], axis=-1) > 1e-9), "reference quantiles tie: the monotonicity check would be vacuous"
        assert np.all(np.diff(q[..., order], axis=-1) >= 0.0)


def _check_calibration(acc, rows, mean, var, noise, Y, probs):
    mu, sg = mean, R.sigma(var, noise)
    n = Y.shape[0]
    ref = R.rows(Y, mu, sg)
    assert np.all(np.abs(ref[..., 0][..., None] - np.asarray(probs)) > 1e-9), "a reference u within 1e-9 of a p_k: counts not pinned"
    assert_allclose(rows, ref, **TOL)
    want = R.sums(ref, probs)
    got = acc.cpu().numpy()
    assert_allclose(got[0], want[0], rtol=TOL["rtol"], atol=n * TOL["atol"])
    assert np.array_equal(got[1:], want[1:])
    return ref, want


SHAPES = [
    # the issue's shapes
    (1, 1, 1), (37, 3, 3), (37, 1, 2), (37, 1, 17), (23, 7, 20), (300, 1, 100), (4099, 2, 5),
    # components staged in LDS (16 lanes x 8) | read from global memory; one S well above the capacity
    (5, 1, 128), (5, 1, 129), (3, 2, 150),
    # lanes per item lowered by S (few items: 16 wanted): 1 | 4 | 8 | 16 at S = 4, 8, 16
    (37, 1, 4), (37, 1, 7), (37, 1, 8), (37, 1, 15), (37, 1, 16),
    # one | several workgroups at 16 lanes per item (16 items each), a ragged last one
    (16, 1, 17), (17, 1, 17),
    # lanes per item by the item count: 16 | 8 at 4096, 8 | 4 at 8192, 4 | 1 at 32768
    (4095, 1, 16), (4096, 1, 16), (8191, 1, 8), (8192, 1, 8), (32767, 1, 5), (16384, 2, 5),
    # lanes per item raised so that 8 components per lane suffice: 1 | 4 at S = 8 | 9, 4 | 8 at 32 | 33, 8 | 16 at 64 | 65
    (32768, 1, 8), (32768, 1, 9), (8192, 1, 32), (8192, 1, 33), (4096, 1, 64), (4096, 1, 65),
    # a workgroup start that is no multiple of DY
    (300, 3, 2),
]


@pytest.mark.parametrize("n,DY,S", SHAPES)
def test_primitive_shapes(ctx, cpu_panel_rho, n, DY, S):
    mean, var, noise, Y = _inputs(n, DY, S)
    q, rc = _quant(ctx, mean, var, noise)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    _check_quantiles(f"({n}, {DY}, {S})", q, mean, var, noise, PROBS, cpu_panel_rho)
    acc, rows, rc = _calib(ctx, mean, var, noise, Y)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    _check_calibration(acc, rows, mean, var, noise, Y, PROBS)


@pytest.mark.parametrize("idx", range(6))
def test_primitive_every_scale_shift_and_noise(ctx, cpu_panel_rho, idx):
    """the six combinations of scale in {0.1, 1, 10} and shift in {0, 100}, both noise values"""
    mean, var, noise, Y = _inputs(37, 2, 9, idx)
    q, rc = _quant(ctx, mean, var, noise)
    assert rc == 0
    _check_quantiles(f"scale/shift/noise {idx}", q, mean, var, noise, PROBS, cpu_panel_rho)
    acc, rows, rc = _calib(ctx, mean, var, noise, Y)
    assert rc == 0
    _check_calibration(acc, rows, mean, var, noise, Y, PROBS)


@pytest.mark.parametrize("P", [1, 16])
def test_primitive_fewest_and_most_probabilities(ctx, cpu_panel_rho, P):
    mean, var, noise, Y = _inputs(37, 3, 5)
    probs = (0.3,) if P == 1 else tuple(np.linspace(0.02, 0.98, 16)[np.random.RandomState(2).permutation(16)])      # unsorted
    q, rc = _quant(ctx, mean, var, noise, probs)
    assert rc == 0 and q.shape == (37, 3, P)
    _check_quantiles(f"P = {P}", q, mean, var, noise, probs, cpu_panel_rho)
    acc, rows, rc = _calib(ctx, mean, var, noise, Y, probs)
    assert rc == 0
    _check_calibration(acc, rows, mean, var, noise, Y, probs)


def test_primitive_gap(ctx, cpu_panel_rho):
    """p = 0.5 between two groups 60 standard deviations apart: F is flat there, any point of the gap with F = 1/2 is a root"""
    mean, var, noise = _gap_case()
    q, rc = _quant(ctx, mean, var, noise)
    assert rc == 0
    _check_quantiles("gap", q, mean, var, noise, PROBS, cpu_panel_rho)
    assert np.all(np.abs(q[..., 3]) < 25.0)
    Y = np.array([[-29.5], [0.0], [31.0]])          # (the middle target lies in the gap: u = 1/2 exactly, so p = 0.5 is left out)
    acc, rows, rc = _calib(ctx, mean, var, noise, Y, PROBS[:3] + PROBS[4:])
    assert rc == 0
    _check_calibration(acc, rows, mean, var, noise, Y, PROBS[:3] + PROBS[4:])
    assert rows[1, 0, 0] == 0.5


def test_primitive_spikes(ctx, cpu_panel_rho):
    mean, var, noise = _spikes_case()
    q, rc = _quant(ctx, mean, var, noise)
    assert rc == 0
    _check_quantiles("spikes", q, mean, var, noise, PROBS, cpu_panel_rho)
    Y = np.array([[4.9995]])
    acc, rows, rc = _calib(ctx, mean, var, noise, Y)
    assert rc == 0
    _check_calibration(acc, rows, mean, var, noise, Y, PROBS)


@pytest.mark.parametrize("S", [2, 40])
def test_primitive_far_component_stays_finite(ctx, cpu_panel_rho, S):
    """one component 10^6 standard deviations away from the others"""
    mean, var, noise, Y = _inputs(5, 1, S, 1)
    mean[S - 1] += 1e6 * np.sqrt(var[S - 1] + noise)
    Y[0, 0] = mean[S - 1, 0, 0] + 0.3
    q, rc = _quant(ctx, mean, var, noise)
    assert rc == 0
    _check_quantiles(f"far component, S = {S}", q, mean, var, noise, PROBS, cpu_panel_rho)
    acc, rows, rc = _calib(ctx, mean, var, noise, Y)
    assert rc == 0 and np.all(np.isfinite(rows)) and np.all(np.isfinite(acc.cpu().numpy()))
    _check_calibration(acc, rows, mean, var, noise, Y, PROBS)


def test_primitive_zero_variance_is_floored(ctx):
    """var + noise = 0: sig = sqrt(DBL_MIN); everything stays finite and the quantiles sit on the mean"""
    mean = np.array([1.5, -2.0]).reshape(1, 2, 1)
    q, rc = _quant(ctx, mean, np.zeros_like(mean), 0.0)
    assert rc == 0 and np.all(np.isfinite(q))
    assert_allclose(q, np.broadcast_to(mean[0][..., None], q.shape), rtol=1e-15)
    acc, rows, rc = _calib(ctx, mean, np.zeros_like(mean), 0.0, np.array([[1.0], [-2.0]]))
    assert rc == 0 and np.all(np.isfinite(rows))
    assert rows[0, 0, 0] == 0.0 and rows[1, 0, 0] == 0.5
    assert_allclose(rows[:, 0, 1], [0.5, 0.0], atol=1e-150)


@pytest.mark.parametrize("n,DY", [(1, 1), (37, 3)])
def test_primitive_single_gaussian_closed_forms(ctx, n, DY):
    """S = 1: u = Phi((y - mu) / sig), CRPS = sig [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)], q = mu + sig Phi^-1(p)"""
    from scipy.special import ndtr, ndtri
    mean, var, noise, Y = _inputs(n, DY, 1, 2)
    sg = R.sigma(var[0], noise)
    acc, rows, rc = _calib(ctx, mean, var, noise, Y)
    assert rc == 0
    assert_allclose(rows[..., 0], ndtr((Y - mean[0]) / sg), **TOL)
    assert_allclose(rows[..., 1], R.crps_single_gaussian(Y, mean[0], sg), **TOL)
    assert_allclose(acc.cpu().numpy()[0], R.crps_single_gaussian(Y, mean[0], sg).sum(0), rtol=TOL["rtol"], atol=n * TOL["atol"])
    q, rc = _quant(ctx, mean, var, noise)
    assert rc == 0
    assert_allclose(q, mean[0][..., None] + sg[..., None] * ndtri(np.asarray(PROBS)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,DY,S", [(37, 3, 3), (300, 1, 100), (4099, 2, 5)])
def test_primitive_accumulates_and_repeats_bitwise(ctx, n, DY, S):
    mean, var, noise, Y = _inputs(n, DY, S, 4)
    mu, sg = mean, R.sigma(var, noise)
    ref = R.rows(Y, mu, sg)
    assert np.all(np.abs(ref[..., 0][..., None] - np.asarray(PROBS)) > 1e-9)
    want = R.sums(ref, PROBS)
    h = n // 2 + 1
    c = np.ascontiguousarray
    acc, _, rc = _calib(ctx, c(mean[:, :h]), c(var[:, :h]), noise, Y[:h], want_rows=False)
    assert rc == 0
    acc, _, rc = _calib(ctx, c(mean[:, h:]), c(var[:, h:]), noise, Y[h:], acc=acc, accumulate=1, want_rows=False)
    assert rc == 0
    got = acc.cpu().numpy()
    assert_allclose(got[0], want[0], rtol=TOL["rtol"], atol=n * TOL["atol"])
    assert np.array_equal(got[1:], want[1:])
    a1, r1, _ = _calib(ctx, mean, var, noise, Y)
    a2, r2, _ = _calib(ctx, mean, var, noise, Y)
    assert np.array_equal(a1.cpu().numpy(), a2.cpu().numpy()) and np.array_equal(r1, r2)
    q1, _ = _quant(ctx, mean, var, noise)
    q2, _ = _quant(ctx, mean, var, noise)
    assert np.array_equal(q1, q2)


def test_primitive_rejects_bad_arguments(ctx):
    mean, var, noise, Y = _inputs(4, 2, 2)
    err = ctx.lib.dsdgp_last_error
    for probs, word in (((0.5, 0.0), b"probs[1]"), ((1.0,), b"probs[0]"), ((0.2, float("nan")), b"probs[1]"), ((-0.1,), b"probs[0]")):
        assert _quant(ctx, mean, var, noise, probs)[1] == BAD_ARG and word in err()
        assert _calib(ctx, mean, var, noise, Y, probs)[2] == BAD_ARG and word in err()
    many = tuple(np.linspace(0.1, 0.9, 17))
    assert _quant(ctx, mean, var, noise, many)[1] == BAD_ARG and b"P = 17" in err()
    assert _calib(ctx, mean, var, noise, Y, many)[2] == BAD_ARG and b"P = 17" in err()
    h, hp = _hp((0.5,))
    m, v = ctx.to_device(mean), ctx.to_device(var)
    q = ctx.empty(4 * 2)
    assert ctx.lib.dsdgp_mixture_quantiles(ctx.handle, _p(m), _p(v), 0.0, 4, 2, 2, hp, 0, _p(q)) == BAD_ARG and b"P = 0" in err()
    assert _quant(ctx, mean, var, -0.1)[1] == BAD_ARG and b"noise variance" in err()
    assert _calib(ctx, mean, var, -0.1, Y)[2] == BAD_ARG and b"noise variance" in err()
    assert _quant(ctx, mean, var, float("nan"))[1] == BAD_ARG


# ---------------------------------------------------------------- model level
_refs = {}


def _noise(model, level="y"):
    return float(model.likelihood.likelihood.variance.value) if level == "y" else 0.0


def _forward(name, S):
    """the parent path: _build_predict on all rows at once — computed once per (model, S)"""
    if (name, S) not in _refs:
        model, Xs, Ys, zs = _case(name)
        _refs[name, S] = model._build_predict(Xs, S=S, zs=[z[:S] for z in zs])
    return _refs[name, S]


def _check_model_quantiles(q, Fm, Fv, noise, probs, Y_std=1.0, Y_mean=0.0):
    mu, sg = Fm, R.sigma(Fv, noise)
    ref = R.quantiles(mu, sg, probs)
    with np.errstate(divide="ignore", over="ignore"):
        f = np.stack([R.pdf(ref[..., k], mu, sg) for k in range(len(probs))], axis=-1)
        tol = 2.0 * R.bar_F() / f + 2.0 * np.spacing(np.abs(ref))
    # (the primitive's all-items bar, carried through q -> Y_mean + Y_std q with two more roundings)
    assert np.all(np.abs(q - (Y_mean + Y_std * ref)) <= Y_std * tol + 2.0 * np.spacing(np.abs(Y_mean) + Y_std * np.abs(ref)))


def _check_scores(out, ref_rows, probs, Y_std=1.0):
    want = R.scores(R.sums(ref_rows, probs), probs, Y_std)
    n = ref_rows.shape[0]
    assert np.all(np.abs(ref_rows[..., 0][..., None] - np.asarray(probs)) > 1e-9)
    assert out["n"] == n
    if "rows" in out:
        assert_allclose(out["rows"], ref_rows, **TOL)
    assert_allclose(out["crps"], want["crps"], **TOL)
    assert_allclose(out["crps_per_output"], want["crps_per_output"], **TOL)
    assert np.array_equal(out["pit_le"], want["pit_le"])
    assert out["coverage"].keys() == want["coverage"].keys()
    for k in want["coverage"]:
        assert out["coverage"][k] == want["coverage"][k]


CAL_PROBS = (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)


@pytest.mark.parametrize("S", [1, 3, 37])
@pytest.mark.parametrize("batch_size", [16, 37, 1000])
@pytest.mark.parametrize("name", ["rbf", "matern_white"])
def test_model_matches_the_parent_path(name, batch_size, S):
    model, Xs, Ys, zs = _case(name)
    Fm, Fv = _forward(name, S)
    z = [q[:S] for q in zs]
    out = model.calibration(Xs, Ys, S, batch_size=batch_size, zs=z, return_rows=True)
    _check_scores(out, R.rows(Ys, Fm, R.sigma(Fv, _noise(model))), CAL_PROBS)
    assert len(out["coverage"]) == 3
    for level in ("y", "f"):
        q = model.predict_quantiles(Xs, S, level=level, batch_size=batch_size, zs=z)
        assert q.shape == (NS, Fm.shape[2], 3)
        _check_model_quantiles(q, Fm, Fv, _noise(model, level), (0.025, 0.5, 0.975))


def test_model_takes_device_tensors_and_broadcast_draws():
    model, Xs, Ys, zs = _case("rbf")
    ctx = model.engine().ctx
    S = 3
    zb = [zs[0][:S, :1], zs[1][:1]]                      # one draw shared by all rows / by all samples
    Fm, Fv = model._build_predict(Xs, S=S, zs=zb)
    zd = [ctx.to_device(z) for z in zb]
    out = model.calibration(ctx.to_device(Xs), ctx.to_device(Ys), S, batch_size=16, zs=zd, return_rows=True)
    _check_scores(out, R.rows(Ys, Fm, R.sigma(Fv, _noise(model))), CAL_PROBS)
    q = model.predict_quantiles(ctx.to_device(Xs), S, probs=PROBS, batch_size=16, zs=zd)
    _check_model_quantiles(q, Fm, Fv, _noise(model), PROBS)


def test_model_device_draws_use_one_seed_per_batch():
    """zs = None: batch k of a call draws under the k-th _draw_seed() after the call's start (world = 1: seed + k + 1);
    _build_predict on the same rows under the same seed is the parent path"""
    model, Xs, Ys, _ = _case("rbf")
    S, bs = 3, 16

    def parent(s0):
        Fm, Fv = [], []
        for k, a in enumerate(range(0, NS, bs)):
            model._seed = s0 + k
            m, v = model._build_predict(Xs[a:a + bs], S=S)
            Fm.append(m); Fv.append(v)
        model._seed = s0 + 3
        return np.concatenate(Fm, 1), np.concatenate(Fv, 1)

    s0 = model._seed
    out = model.calibration(Xs, Ys, S, batch_size=bs, return_rows=True)
    assert model._seed == s0 + 3
    Fm, Fv = parent(s0)
    _check_scores(out, R.rows(Ys, Fm, R.sigma(Fv, _noise(model))), CAL_PROBS)
    s0 = model._seed
    q = model.predict_quantiles(Xs, S, batch_size=bs)
    assert model._seed == s0 + 3
    Fm, Fv = parent(s0)
    _check_model_quantiles(q, Fm, Fv, _noise(model), (0.025, 0.5, 0.975))


def test_model_output_scaling():
    """predict_quantiles returns Y_mean + Y_std q; calibration scales CRPS by Y_std and nothing else"""
    model, Xs, Ys, zs = _case("matern_white")
    S, Y_std, Y_mean = 3, 2.5, -4.0
    z = [q[:S] for q in zs]
    Fm, Fv = _forward("matern_white", S)
    q1 = model.predict_quantiles(Xs, S, zs=z)
    q = model.predict_quantiles(Xs, S, zs=z, Y_std=Y_std, Y_mean=Y_mean)
    assert np.array_equal(q, Y_mean + Y_std * q1)
    _check_model_quantiles(q, Fm, Fv, _noise(model), (0.025, 0.5, 0.975), Y_std, Y_mean)
    out1 = model.calibration(Xs, Ys, S, zs=z)
    out = model.calibration(Xs, Ys, S, zs=z, Y_std=Y_std)
    _check_scores(out, R.rows(Ys, Fm, R.sigma(Fv, _noise(model))), CAL_PROBS, Y_std)
    assert "rows" not in out and np.array_equal(out["pit_le"], out1["pit_le"]) and out["coverage"] == out1["coverage"]
    assert_allclose(out["crps"], Y_std * out1["crps"], rtol=1e-15)


@pytest.mark.parametrize("name", ["bernoulli", "multiclass"])
def test_model_latent_level_on_other_likelihoods(name):
    from doubly_stochastic_dgp import _lib
    model, Xs, Ys, zs = _case(name)
    S = 3
    z = [q[:S] for q in zs]
    Fm, Fv = _forward(name, S)
    q = model.predict_quantiles(Xs, S, level="f", zs=z, batch_size=16)
    assert q.shape == (NS, 3 if name == "multiclass" else 2, 3)
    _check_model_quantiles(q, Fm, Fv, 0.0, (0.025, 0.5, 0.975))
    with pytest.raises(NotImplementedError):
        model.predict_quantiles(Xs, S, level="y", zs=z)
    with pytest.raises(NotImplementedError):
        model.predict_quantiles(Xs, S, zs=z)
    with pytest.raises(NotImplementedError):
        model.calibration(Xs, np.zeros((NS, q.shape[1])), S, zs=z)
    with pytest.raises(NotImplementedError):
        model.likelihood.mixture_quantiles(Fm, Fv, (0.5,))
    # the library refuses as well
    eng = model.engine()
    ctx = eng.ctx
    h, hp = _hp((0.5,))
    Xd, out = ctx.to_device(Xs), ctx.empty(NS, q.shape[1], 1)
    rc = ctx.lib.dsdgp_model_quantiles(eng.model, _p(Xd), NS, S, None, None, C.c_uint64(1), 1, hp, 1, _p(out))
    assert rc == UNSUPPORTED and b"not a Gaussian mixture" in ctx.lib.dsdgp_last_error()
    Yd, acc = ctx.to_device(np.zeros((NS, q.shape[1]))), ctx.empty(3, q.shape[1])
    rc = ctx.lib.dsdgp_model_calibration(eng.model, _p(Xd), _p(Yd), NS, S, None, None, C.c_uint64(1), hp, 1, None, _p(acc), 0)
    assert rc == UNSUPPORTED and b"not a Gaussian mixture" in ctx.lib.dsdgp_last_error()
    ctx.sync()


def test_model_coverage_is_the_difference_of_the_pit_fractions():
    model, Xs, Ys, zs = _case("rbf")
    S = 3
    out = model.calibration(Xs, Ys, S, zs=[q[:S] for q in zs])
    le = out["pit_le"].mean(1)      # (the outputs have equal row counts)
    assert sorted(out["coverage"]) == pytest.approx([0.5, 0.9, 0.95])
    for c, (k, l) in zip((0.95, 0.9, 0.5), ((0, 6), (1, 5), (2, 4))):
        key = min(out["coverage"], key=lambda x: abs(x - c))
        assert_allclose(out["coverage"][key], le[l] - le[k], rtol=1e-14, atol=1e-15)
    assert model.calibration(Xs, Ys, S, probs=(0.1, 0.5), zs=[q[:S] for q in zs])["coverage"] == {}


def test_model_refusals_reach_the_caller():
    from doubly_stochastic_dgp import _lib
    model, Xs, Ys, zs = _case("rbf")
    eng = model.engine()
    ctx = eng.ctx
    eng.set_sample_weights(ctx.to_device(np.full(3, 1.0 / 3.0)))
    try:
        with pytest.raises(_lib.DsdgpError, match="-4"):
            model.calibration(Xs, Ys, 3)
        assert b"sample weights" in ctx.lib.dsdgp_last_error()
        with pytest.raises(_lib.DsdgpError, match="-4"):
            model.predict_quantiles(Xs, 3, level="f")
    finally:
        eng.set_sample_weights(None)
    h, hp = _hp((0.5, 1.5))
    Xd, out = ctx.to_device(Xs), ctx.empty(NS, 2, 2)
    assert ctx.lib.dsdgp_model_quantiles(eng.model, _p(Xd), NS, 3, None, None, C.c_uint64(1), 1, hp, 2, _p(out)) == BAD_ARG
    assert b"probs[1]" in ctx.lib.dsdgp_last_error()
    assert ctx.lib.dsdgp_model_quantiles(eng.model, _p(Xd), NS, 3, None, None, C.c_uint64(1), 2, hp, 1, _p(out)) == BAD_ARG
    ctx.sync()
    assert np.isfinite(model.calibration(Xs, Ys, 3)["crps"])


_CHILD = r"""
import json, sys
sys.path[:0] = sys.argv[1:3]
from tests import test_gpu_calibration as T
print(json.dumps(T._bits_of_one_run()))
"""


def _bits_of_one_run():
    """predict_quantiles and calibration on the RBF model with explicit draws: digests of their outputs, and whether they equal, bit for
    bit, the primitive wrappers applied to this process's own _build_predict outputs (one batch)"""
    import hashlib
    model, Xs, Ys, zs = _build_case("rbf")
    S = 3
    z = [q[:S] for q in zs]
    out = model.calibration(Xs, Ys, S, batch_size=16, zs=z, return_rows=True)
    one = model.calibration(Xs, Ys, S, batch_size=1000, zs=z, return_rows=True)
    qy = model.predict_quantiles(Xs, S, probs=PROBS, zs=z)
    qf = model.predict_quantiles(Xs, S, probs=PROBS, level="f", zs=z)
    Fm, Fv = model._build_predict(Xs, S=S, zs=z)
    lik = model.likelihood
    acc, rows = lik.mixture_calibration(Fm, Fv, Ys, CAL_PROBS, rows=True)
    from doubly_stochastic_dgp.dgp import calibration_scores
    want = calibration_scores(acc, CAL_PROBS)
    same = bool(np.array_equal(rows, one["rows"]) and want["crps"] == one["crps"] and np.array_equal(want["pit_le"], one["pit_le"])
                and want["coverage"] == one["coverage"] and np.array_equal(lik.mixture_quantiles(Fm, Fv, PROBS), qy)
                and np.array_equal(lik.mixture_quantiles(Fm, Fv, PROBS, level="f"), qf))
    dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {"forward": dig(Fm) + dig(Fv), "rows": dig(out["rows"]), "qy": dig(qy), "qf": dig(qf), "crps": float(out["crps"]).hex(),
            "pit_le": dig(out["pit_le"]), "same_as_primitive": same}


def test_model_equals_the_primitive_bit_for_bit():
    """the default configuration, in this process"""
    got = _bits_of_one_run()
    assert got["same_as_primitive"]


@pytest.mark.parametrize("env", [{"DSDGP_NO_OVERLAP": "1"}, {"DSDGP_FORCE": "gemm_mp=16"}], ids=["no_overlap", "gemm"])
def test_model_bits_do_not_depend_on_the_forward_path(env):
    """Each switch in a fresh child process (both are read when the device model is created).  In every process the model-level calls
    equal the primitive on that process's own forward outputs bit for bit; two processes whose forward passes wrote the same bits report
    the same bits.  The GEMM-formulated chains sum in another order (tests/test_gpu_gemm_path.py), so their score is held to that file's
    chain-against-GEMM bound instead, rtol 1e-8."""
    base = _bits_of_one_run()
    got = run_child(_CHILD, env)
    print("default", base, "\n", env, got)
    assert base["same_as_primitive"] and got["same_as_primitive"]
    if "DSDGP_NO_OVERLAP" in env:
        assert got["forward"] == base["forward"]
    if got["forward"] == base["forward"]:
        for k in ("rows", "qy", "qf", "crps", "pit_le"):
            assert got[k] == base[k], k
    else:
        assert_allclose(float.fromhex(got["crps"]), float.fromhex(base["crps"]), rtol=1e-8)


def test_calibration_between_training_steps_leaves_their_bits():
    """two models take the same two optimiser steps; one of them scores held-out rows (another row count, another S) in between"""
    rng = np.random.RandomState(9)
    N, D, M, S = 40, 2, 16, 3
    X, Y = rng.randn(N, D), rng.randn(N, 2)
    Z = X[:M] + 0.01 * rng.randn(M, D)
    specs = [kern_spec("rbf", D, 1.2, 0.9)] * 2
    Xs, Ys = rng.randn(NS, D), rng.randn(NS, 2)
    zs = [rng.randn(S, N, 2), rng.randn(S, N, 2)]
    thetas, elbos = [], []
    for between in (False, True):
        _, _, model = make_case(X, Y, Z, specs, lik_var=0.1, S=S, seed=3)
        eng = model.engine()
        eng._ensure(N, 5)
        e = [model.train_step(X=X, Y=Y, zs=zs, sync=True)]
        if between:
            out = model.calibration(Xs, Ys, 5, batch_size=16)
            assert np.isfinite(out["crps"])
            model.predict_quantiles(Xs, 5, batch_size=16)
        e.append(model.train_step(X=X, Y=Y, zs=zs, sync=True))
        eng.ctx.sync()
        thetas.append(eng.theta.cpu().numpy().copy())
        elbos.append(e)
    assert elbos[0] == elbos[1]
    assert np.array_equal(thetas[0].view(np.uint64), thetas[1].view(np.uint64))

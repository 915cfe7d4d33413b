"""-m gpu: the PCA of the step-down mean functions on the device (csrc/pca.hip; dsdgp_pca, layer_initializations.pca_map,
init_layers_linear(pca="device"), DGP(pca="device")) against tests/pca_reference.py on the cases of tests/pca_cases.py.

Bounds.  "The truth" is the Gram matrix in long double and np.linalg.eigh of it; every bar is 8 x what the reference itself reaches.
Gram: |gram - C| <= 8 max(|Xc^T Xc (float64 numpy) - C|, n 2^-53 |Xc|^T |Xc|) elementwise — numpy's own error, or the bound of adding n
products one after another — and gram is exactly symmetric.
Eigenvalues, orthonormality, residual: 8 x R_LAM, R_ORTH, R_RES (the worst figures of the numpy Jacobi, tests/pca_reference.ratios) in
units of D 2^-52 (|C|_F); the subspace of a gapped case: 8 R_PROJ D 2^-52 |C|_F / (lam_k - lam_{k+1}).
DSDGP_PCA_PROFILE=<file> writes the measured ratio of every case, 1 = at the bar (profiles/pca_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import pca_cases as PC
from tests import pca_reference as R

pytestmark = pytest.mark.gpu

BAD_ARG = -1
CANARY = -12345.25
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_PCA_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Device PCA: measured errors (tests/test_gpu_pca.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar.  `gram`: the worst |gram - C| over 8 max(|Xc^T Xc (numpy) - C|,\n"
                "n 2^-53 |Xc|^T |Xc|).  `lam`, `orth`, `res`: eigenvalues, max|T^T T - I| and the worst residual |C t_j - lam_j t_j| over\n"
                "8 R_LAM, 8 R_ORTH, 8 R_RES x D 2^-52 (|C|_F).  `proj`: |T T^T - U_k U_k^T|_2 over 8 R_PROJ D 2^-52 |C|_F / gap, `-` where\n"
                "the case has no gap behind lam_k.  The reference's own figures: R_LAM = %.3g, R_ORTH = %.3g, R_RES = %.3g, R_PROJ = %.3g.\n\n"
                "| case | n | D | k | sweeps | gram | lam | orth | res | proj |\n|---|---|---|---|---|---|---|---|---|---|\n"
                % (R.R_LAM, R.R_ORTH, R.R_RES, R.R_PROJ))
        for r in _ROWS:
            f.write("| %s | %d | %d | %d | %d | %.3g | %.3g | %.3g | %.3g | %s |\n" % r)


def _pca(X, k, center, **kw):
    from doubly_stochastic_dgp.layer_initializations import pca_map
    return pca_map(X, k, center=center, return_info=True, **kw)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _raw(ctx, Xd, n, D, k, center, sweeps, W, ldw, evals=None, mean=None, gram=None, info=None, X_null=False):
    rc = ctx.lib.dsdgp_pca(ctx.handle, None if X_null else _p(Xd), n, D, k, center, sweeps, _p(W), ldw, _p(evals), _p(mean), _p(gram),
                           _p(info))
    ctx.sync()
    return rc


def _gram_bar(name):
    tr = PC.truth(name)
    Xc, n = tr["Xc"], tr["Xc"].shape[0]
    return 8.0 * np.maximum(np.abs(Xc.T @ Xc - tr["C"]), n * 2.0 ** -53 * (np.abs(Xc).T @ np.abs(Xc)))


@pytest.mark.parametrize("name", PC.NAMES)
def test_cases_match_the_truth(ctx, name):
    X, k, center = PC.inputs(name)
    n, D = X.shape
    tr = PC.truth(name)
    T, info = _pca(X, k, center)
    lam, gram = info["eigenvalues"], info["gram"]
    unit = D * R.EPS
    scale = unit * tr["normF"]
    gbar = _gram_bar(name)
    with np.errstate(divide="ignore", invalid="ignore"):
        g_fig = float(np.nanmax(np.where(gbar > 0, np.abs(gram - tr["C"]) / gbar, np.where(gram == tr["C"], 0.0, np.inf))))
    r_orth, r_res, _ = R.figures(tr, lam, T)
    l_fig = float(np.max(np.abs(lam - tr["lam"]))) / scale / (8.0 * R.R_LAM)
    o_fig, s_fig = r_orth / (8.0 * R.R_ORTH), r_res / (8.0 * R.R_RES)
    p_fig = R.projector_figure(tr, T, k) / (8.0 * R.R_PROJ) if PC.gapped(name) else None
    row = (name, n, D, k, info["sweeps"], g_fig, l_fig, o_fig, s_fig, "-" if p_fig is None else "%.3g" % p_fig)
    print("%s (%d x %d, k = %d): %d sweeps; gram %.3g, lam %.3g, orth %.3g, res %.3g, proj %s (x bar)" % row)
    _ROWS.append(row)
    # shape, sign rule, stopping
    assert T.shape == (D, k) and lam.shape == (D,) and gram.shape == (D, D) and info["mean"].shape == (D,)
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(lam))
    assert np.all(T[np.argmax(np.abs(T), axis=0), np.arange(k)] > 0.0)
    assert info["converged"] is True and 1 <= info["sweeps"] <= 30
    # Gram
    assert np.array_equal(gram, gram.T)
    assert np.all(np.abs(gram - tr["C"]) <= gbar)
    # eigenvalues and what is derived from them
    assert np.all(np.diff(lam) <= 0.0)
    assert np.all(np.abs(lam - tr["lam"]) <= 8.0 * R.R_LAM * scale)
    pos = np.maximum(lam, 0.0)
    assert np.array_equal(info["singular_values"], np.sqrt(pos))
    assert np.array_equal(info["explained"], np.cumsum(pos) / pos.sum() if pos.sum() > 0 else np.zeros(D))
    # orthonormality of all k columns, residual of each, subspace
    assert np.max(np.abs(T.T @ T - np.eye(k))) <= 8.0 * R.R_ORTH * unit
    assert np.all(np.linalg.norm(tr["C"] @ T - T * lam[:k], axis=0) <= 8.0 * R.R_RES * scale)
    if p_fig is not None:
        assert p_fig <= 1.0
    # mean
    if center:
        assert np.all(np.abs(info["mean"] - tr["mean"]) <= n * 2.0 ** -53 * np.abs(X).max())
    else:
        assert np.array_equal(info["mean"], np.zeros(D))
    # the raw entry gives the same bits
    Wd, ev = ctx.empty(D, k).fill_(CANARY), ctx.empty(D)
    assert _raw(ctx, ctx.to_device(X), n, D, k, int(center), 30, Wd, k, evals=ev) == 0, ctx.lib.dsdgp_last_error()
    assert _same_bits(Wd.cpu().numpy(), T) and _same_bits(ev.cpu().numpy(), lam)
    if name == "diag":
        assert info["sweeps"] == 1
        assert np.array_equal(T, np.eye(D)[:, [15, 14, 13, 12]])
        assert np.array_equal(lam, np.arange(16.0, 0.0, -1.0) ** 2)
    if name == "pair_equal":
        assert np.all(np.abs(T[:, 0] - np.sqrt(0.5)) <= 4 * np.spacing(np.sqrt(0.5)))


def test_one_sweep_of_c100_has_not_converged():
    from doubly_stochastic_dgp.layer_initializations import pca_map
    X, k, center = PC.inputs("c100")
    T, info = _pca(X, k, center, max_sweeps=1)
    assert info["converged"] is False and info["sweeps"] == 1
    assert np.max(np.abs(T.T @ T - np.eye(k))) <= 8.0 * R.R_ORTH * X.shape[1] * R.EPS
    with pytest.raises(RuntimeError):
        pca_map(X, k, center=center, max_sweeps=1)


@pytest.mark.parametrize("name", ["odd17", "c100"])
def test_a_second_call_and_a_device_tensor_give_the_same_bits(ctx, name):
    X, k, center = PC.inputs(name)
    T1, i1 = _pca(X, k, center)
    for T, i in (_pca(X, k, center), _pca(ctx.to_device(X), k, center)):
        assert _same_bits(T, T1) and _same_bits(i["eigenvalues"], i1["eigenvalues"]) and _same_bits(i["gram"], i1["gram"])


def test_raw_outputs_are_optional_and_ldw_is_respected(ctx):
    torch = ctx.torch
    X, k, center = PC.inputs("offset")
    n, D = X.shape
    Xd = ctx.to_device(X)
    ldw = k + 3
    W = ctx.empty(D, ldw).fill_(CANARY)
    ev, mean, gram = ctx.empty(D + 1).fill_(CANARY), ctx.empty(D + 1).fill_(CANARY), ctx.empty(D * D + 1).fill_(CANARY)
    info = torch.full((5,), -7, dtype=torch.int32, device=Xd.device)
    assert _raw(ctx, Xd, n, D, k, 1, 30, W, ldw, ev, mean, gram, info) == 0, ctx.lib.dsdgp_last_error()
    T, ref = _pca(X, k, center)
    Wh = W.cpu().numpy()
    assert _same_bits(np.ascontiguousarray(Wh[:, :k]), T) and np.all(Wh[:, k:] == CANARY)
    assert _same_bits(ev[:D].cpu().numpy(), ref["eigenvalues"]) and float(ev[D]) == CANARY
    assert _same_bits(mean[:D].cpu().numpy(), ref["mean"]) and float(mean[D]) == CANARY
    assert _same_bits(gram[:D * D].cpu().numpy().reshape(D, D), ref["gram"]) and float(gram[D * D]) == CANARY
    assert info.cpu().numpy().tolist() == [1, ref["sweeps"], info.cpu().numpy()[2], 0, -7]
    for drop in ("ev", "mean", "gram", "info"):
        kw = dict(evals=ev, mean=mean, gram=gram, info=info)
        kw[{"ev": "evals"}.get(drop, drop)] = None
        W2 = ctx.empty(D, k)
        assert _raw(ctx, Xd, n, D, k, 1, 30, W2, k, **kw) == 0, (drop, ctx.lib.dsdgp_last_error())
        assert _same_bits(W2.cpu().numpy(), T), drop
    W3 = ctx.empty(D, k)
    assert _raw(ctx, Xd, n, D, k, 1, 30, W3, k) == 0
    assert _same_bits(W3.cpu().numpy(), T)
    # center = 0 writes zeros to mean
    assert _raw(ctx, Xd, n, D, k, 0, 30, W3, k, mean=mean) == 0
    assert np.array_equal(mean[:D].cpu().numpy(), np.zeros(D)) and float(mean[D]) == CANARY


def test_bad_arguments_return_an_error_and_leave_w_alone(ctx):
    X, k, _ = PC.inputs("odd17")
    n, D = X.shape
    Xd = ctx.to_device(X)
    W = ctx.empty(D, k).fill_(CANARY)
    err = ctx.lib.dsdgp_last_error
    for kw in (dict(n=0), dict(n=2 ** 31), dict(D=0), dict(D=1025), dict(k=0), dict(k=D + 1), dict(center=2), dict(center=-1),
               dict(sweeps=0), dict(sweeps=65), dict(ldw=k - 1)):
        a = dict(n=n, D=D, k=k, center=0, sweeps=30, ldw=k)
        a.update(kw)
        assert _raw(ctx, Xd, a["n"], a["D"], a["k"], a["center"], a["sweeps"], W, a["ldw"]) == BAD_ARG, kw
        assert b"bad argument" in err()
    assert _raw(ctx, Xd, n, D, k, 0, 30, W, k, X_null=True) == BAD_ARG
    assert _raw(ctx, Xd, n, D, k, 0, 30, None, k) == BAD_ARG
    assert np.all(W.cpu().numpy() == CANARY)
    assert _raw(ctx, Xd, n, D, k, 0, 30, W, k) == 0
    assert np.all(np.isfinite(W.cpu().numpy()))


def test_device_pca_through_the_model():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Identity, Linear
    from doubly_stochastic_dgp.layer_initializations import init_layers_linear, pca_map
    rng = np.random.default_rng(21)
    X = rng.standard_normal((200, 8)) * np.linspace(1.0, 3.0, 8)
    Y = rng.standard_normal((200, 1))
    Z = X[:20].copy()
    T = pca_map(X, 3)
    kernels = lambda: [RBF(8), RBF(3), RBF(3)]
    layers = init_layers_linear(X, Y, Z, kernels(), pca="device")
    model = DGP(X, Y, Z, kernels(), Gaussian(), pca="device")
    for ls in (layers, model.layers):
        assert isinstance(ls[0].mean_function, Linear) and isinstance(ls[1].mean_function, Identity)
        assert _same_bits(np.ascontiguousarray(ls[0].mean_function.A.value), T)
        assert _same_bits(np.ascontiguousarray(ls[0].feature.Z.value), Z)
        assert _same_bits(np.ascontiguousarray(ls[1].feature.Z.value), Z @ T)
        assert _same_bits(np.ascontiguousarray(ls[2].feature.Z.value), Z @ T)
    # the host-built model with the device's T in its mean function and its Z (and the q_sqrt = chol Ku(Z) derived from Z) is the same model
    host = DGP(X, Y, Z, kernels(), Gaussian(), pca="host")
    host.layers[0].mean_function.A = T
    for l in (1, 2):
        host.layers[l].feature.Z = Z @ T
        host.layers[l].q_sqrt = model.layers[l].q_sqrt.value
    a, b = model.compute_log_likelihood(), host.compute_log_likelihood()
    print("ELBO with the device's PCA:", a, "host model carrying the same T:", b)
    assert np.isfinite(a)
    assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)

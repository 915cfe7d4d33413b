"""Ku's Cholesky factor Lu and the explicit inverses Lu^-1, Lu^-T, Ku^-1 read straight out of the model (dsdgp_model_layer_matrix: the
padded buffers as the kernels left them) and compared, matrix by matrix, with a CPU factorisation of the same Ku — on every
factorisation path, at every padded size of the LDS core, on well- and ill-conditioned inducing points.

What is asserted per matrix (tests/factor_reference.py; eps = 2^-52, n = M, products in longdouble, in float64 from n = 1024 on where the
bars get the product's own n eps):
 1. factor backward error  max|L L^T - Ku| / max|Ku| <= 1e-14 n                     (Lu is kept by white = True models only)
 2. inverse residuals  max|X L - I| / (n eps max(|X||L|))  and  max|L X - I| / (n eps max(|L||X|))  with the device's own Lu (white =
    True models): at most 8 x the larger value of the two CPU inverses (substitution, dtrtri) of the CPU factor on that side, and never
    required below 1.0.  Every model, also the white = False ones that keep no Lu: max|X Ku X^T - I| / (n eps max(|X||L||L^T||X^T|)),
    same rule
 3. Lu^-T == (Lu^-1)^T exactly
 4. Ku^-1:  max|Ku^-1 Ku - I| / (n eps max(|Ku^-1||Ku|)) <= 8 x the value of X^T X from the CPU inverse (floor 1.0);
    max|Ku^-1 - Ku^-1^T| / max|Ku^-1| <= n eps
 5. Mp <= 128: forward error of Lu and Lu^-1 against a 40-digit factorisation (mpmath) of the reference Ku, entrywise max relative to
    max|.|, at most 8 x LAPACK's.  LAPACK's error is taken as the larger of two runs against that same truth: on the reference Ku and on
    the Gram matrix the DEVICE forms from the same Z (dsdgp_gram).  Why: the two Ku differ by the rounding of the distance expansion
    (3.6e-15 at most on `spread`, M = 128), and on a well-conditioned matrix that alone decides the forward error.  Measured on the first
    run of this file: `spread`, rbf, M = 128 — device Lu 8.7e-13 (LDS core, one-workgroup kernel and block kernel alike: 8.7 .. 9.2e-13),
    LAPACK on the reference Ku 8.1e-14, the SAME LAPACK on a Gram matrix rounded differently by 3.6e-15 8.9e-13; Lu^-1: 5.4e-12, 9.6e-13,
    5.5e-12.  Against LAPACK on the reference Ku alone the device stood at 10 .. 24 x on fifteen well-conditioned cases and at 0.1 .. 1 x
    on the ill-conditioned ones: the input, not the factorisation.  The table also holds the ratio of both on the device-formed Gram.
    What this item did find: the one-workgroup kernel (k_potrf_trtri) formed its panels as A_ij X_jj^T with the explicit inverse of the
    diagonal block and nothing else; on `grid1d` M = 17 / 50 and `pairs` M = 50 its Lu^-1 stood at 2.5e-09 / 5.7e-09 / 2.8e-09 against
    LAPACK's 1.7e-10 / 5.9e-10 / 2.6e-10 (14 x, where the LDS core is at 1 x).  With one refinement step on the panel (linalg.hip) it is
    at 2.0e-10 / 5.6e-10 / 6.3e-10.
 6. exact structure: identity pad rows / columns, +0.0 above the diagonal of Lu and Lu^-1 and below that of Lu^-T, no NaN / Inf
The reference Ku is the oracle's kernel + jitter; the device forms its own from the same Z and hyper-parameters (test_device_gram_is_
not_the_variable bounds that difference by the rounding of the distance expansion).

Paths (chosen with the switches the library already has): the head launch's LDS core (default, Mp <= 128); the one-workgroup kernel in
LDS (DSDGP_FORCE=head=0) and in global memory (Mp = 160, or D_in = 17 which the head launch refuses); the blocked sequence's block kernel
alone (DSDGP_BIG_MP=128, read once per process: a child process); the blocked look-ahead sequence, one matrix and a uniform batch; mixed
models; the plain blocked sequence (DSDGP_CHOL_LOOKAHEAD=0); Mp = 1152, which only the GEMM-formulated layers take.

Set DSDGP_FACTOR_PROFILE=<file> to get every measured device and CPU value as one table (profiles/factor_direct_residuals.md).
135 cases, 208 matrices, about a minute on an MI355X with 16 host cores (the 40-digit factorisations run once, in worker processes)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "doubly-stochastic-dgp_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from tests import factor_reference as R      # noqa: E402
from tests.helpers import make_case          # noqa: E402

pytestmark = pytest.mark.gpu

HEAD0 = {"DSDGP_FORCE": "head=0"}
PLAIN = {"DSDGP_CHOL_LOOKAHEAD": "0"}
SINGLE = {"DSDGP_FORCE": "head=0", "DSDGP_BIG_MP": "128"}
# every padded size the LDS core exists for, with an M that is not a multiple of 16 and, for 64 and 128, the exact size
LDS_SIZES = [17, 33, 50, 64, 70, 90, 100, 127, 128]
KINDS = ["rbf", "matern52"]


def padded(M):
    from doubly_stochastic_dgp.engine import padded_M
    return padded_M(M)


# ------------------------------------------------------------------------------------------------ cases
class Layer:
    def __init__(self, family, M, kind="rbf", jitter=1e-6, D=None):
        self.family, self.M, self.kind, self.jitter = family, M, kind, jitter
        if family == "spread" and D is not None and D != 3:       # (D_in = 17: the head launch refuses it) same typical distances as D = 3
            rng = np.random.RandomState(M + D)
            self.Z = 2.0 * rng.randn(M, D)
            self.spec = dict(kind=kind, input_dim=D, variance=1.0, lengthscales=float(np.sqrt(D / 3.0)), ARD=False, white_variance=None)
        else:
            self.Z, self.spec = R.family_case(family, M, kind)
        self.D = self.Z.shape[1]
        self.name = f"{family}-{kind}-M{M}" + ("" if jitter == 1e-6 else f"-j{jitter:g}") + ("" if self.D <= 3 else f"-D{self.D}")
        self._ku = None

    def ku(self):
        if self._ku is None:
            self._ku = R.reference_ku(self.Z, self.spec, self.jitter)
        return self._ku


_REF = {}


def reference(layer):
    """the CPU reference's own measures of this matrix (once per matrix and process)"""
    if layer.name not in _REF:
        _REF[layer.name] = R.reference_measures(layer.ku())
    return _REF[layer.name]


def build_model(layers, white):
    """the product model whose layer l has inducing points layers[l].Z and kernel layers[l].spec: tests.helpers.make_case where it can
    express the model (every layer on the same Z), explicit SVGP layers (identity mean functions) for layers of different M"""
    from doubly_stochastic_dgp import settings
    jitter = layers[0].jitter
    D = layers[0].D
    assert all(l.D == D and l.jitter == jitter for l in layers)
    rng = np.random.RandomState(11)
    X, Y = rng.randn(8, D), rng.randn(8, 1)
    if all(l.Z is layers[0].Z or np.array_equal(l.Z, layers[0].Z) for l in layers):
        return make_case(X, Y, layers[0].Z, [l.spec for l in layers], white=white, jitter=jitter, S=2, seed=3)[2]
    from doubly_stochastic_dgp.dgp import DGP_Base
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Identity, Zero
    from doubly_stochastic_dgp.layers import SVGP_Layer
    from tests.helpers import product_kernel
    with settings.temp_jitter(jitter):
        svgp = [SVGP_Layer(product_kernel(l.spec), l.Z, D if i + 1 < len(layers) else 1, Identity() if i + 1 < len(layers) else Zero(),
                           white=white) for i, l in enumerate(layers)]
        return DGP_Base(X, Y, Gaussian(variance=0.1), svgp, num_samples=2)


def read_matrices(model, nlayers, white, jitter):
    """[{Linv, LinvT, Kinv (, Lu)} per layer] after dsdgp_model_prepare"""
    from doubly_stochastic_dgp import settings
    with settings.temp_jitter(jitter):
        eng = model.engine()
        eng.prepare()
        out = []
        for l in range(nlayers):
            mats = {w: eng.layer_matrix(l, w) for w in ("Linv", "LinvT", "Kinv")}
            if white:
                mats["Lu"] = eng.layer_matrix(l, "Lu")
            out.append(mats)
        return out


# ------------------------------------------------------------------------------------------------ the profile table
_ROWS = []
_ULPS = []
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def profile_table():
    yield
    path = os.environ.get("DSDGP_FACTOR_PROFILE")
    if not path or not _ROWS:
        return
    hdr = ["matrix", "path", "white", "n", "Mp", "cond(Ku)", "factor / (1e-14 n)", "X L dev", "X L cpu", "L X dev", "L X cpu", "X Ku X^T dev", "X Ku X^T cpu", "Ku^-1 dev",
           "Ku^-1 cpu", "asym / (n eps)", "fwd L dev", "fwd L lapack", "L dev / lapack on the device Gram", "fwd X dev",
           "fwd X lapack", "X dev / lapack on the device Gram"]
    with open(path, "w") as f:
        f.write("# Lu, Lu^-1, Ku^-1 read from the model against the CPU reference (tests/test_gpu_factor_direct.py)\n\n"
                "Scaled residuals as defined in tests/factor_reference.py; `cpu` = the larger of LAPACK substitution / dtrtri on the CPU factor; a device\n"
                "value may be 8 x the CPU one (never required below 1.0).  `fwd`: error against the 40-digit factorisation of the reference Ku (Mp <= 128);\n"
                "`fwd ... lapack`: the larger of LAPACK's error on the reference Ku and on the device-formed Gram matrix, both against that same truth.\n\n")
        f.write("| " + " | ".join(hdr) + " |\n|" + "---|" * len(hdr) + "\n")
        for r in _ROWS:
            f.write("| " + " | ".join(r) + " |\n")
        if _ULPS:
            f.write("\n## Largest entrywise difference of Lu^-1 between paths (ulps of the larger entry; Mp = 128)\n\n| matrix | paths | max ulps |\n|---|---|---|\n")
            for r in _ULPS:
                f.write("| " + " | ".join(r) + " |\n")
        f.write(f"\n{len(_ROWS)} matrices, {time.time() - _T0:.0f} s for the module.\n")


def _fmt(v):
    return "-" if v is None else (f"{v:.3g}")


# ------------------------------------------------------------------------------------------------ the checks
def check_structure(mats, M, Mp, tag):
    """item 6 (+ item 3): exact"""
    for name, A in mats.items():
        assert A.shape == (Mp, Mp)
        assert np.all(np.isfinite(A)), f"{tag}: NaN / Inf in {name}"
    Linv, LinvT = mats["Linv"], mats["LinvT"]
    eye_pad = np.eye(Mp)[M:]
    for name in ("Lu", "Linv", "LinvT"):
        if name in mats:
            A = mats[name]
            assert np.array_equal(A[M:], eye_pad), f"{tag}: pad rows of {name} are not those of the identity"
            assert np.array_equal(A[:, M:], eye_pad.T), f"{tag}: pad columns of {name} are not those of the identity"
    iu = np.triu_indices(Mp, 1)
    for name in ("Lu", "Linv"):
        if name in mats:
            assert not np.any(np.ascontiguousarray(mats[name][iu]).view(np.uint64)), f"{tag}: {name} is not +0.0 above the diagonal"
    assert not np.any(np.ascontiguousarray(LinvT.T[iu]).view(np.uint64)), f"{tag}: Lu^-T is not +0.0 below the diagonal"
    assert np.array_equal(LinvT, Linv.T), f"{tag}: Lu^-T is not the transpose of Lu^-1"


def check_matrix(layer, mats, path, white, with_kinv=True, with_truth=None, ku=None, ref=None, record=True):
    """items 1 - 6 for one matrix; returns the measured values"""
    M, Mp = layer.M, padded(layer.M)
    n = M
    tag = f"{layer.name} [{path}, white={white}]"
    check_structure(mats, M, Mp, tag)
    Ku = layer.ku() if ku is None else ku
    ref = reference(layer) if ref is None else ref
    X = mats["Linv"][:M, :M]
    got = dict(factor=None, left=None, right=None, kinv=None, asym=None, fwdL=None, fwdX=None, fwdL_ref=None, fwdX_ref=None, fwdL_same=None,
               fwdX_same=None)
    if "Lu" in mats:
        L = mats["Lu"][:M, :M]
        got["factor"] = R.factor_backward(L, Ku)
        got["left"], got["right"] = R.inverse_residuals(X, L)
    got["congr"] = R.congruence_residual(X, Ku, ref["L"])
    if with_kinv:
        Kinv = mats["Kinv"][:M, :M]
        got["kinv"], got["asym"] = R.kinv_residual(Kinv, Ku), R.kinv_asymmetry(Kinv)
    if with_truth is None:
        with_truth = Mp <= 128
    if with_truth:
        # item 5.  "LAPACK's error on the same matrix": the device factors the Ku IT forms, which differs from the reference Ku in the
        # rounding of the distance expansion (test_device_gram_is_not_the_variable: up to 3.6e-15), and on a well-conditioned matrix that
        # difference alone moves LAPACK's own forward error 10 to 20 x (see the module docstring).  So LAPACK is run twice against the
        # truth of the reference Ku — on the reference Ku and on the device-formed one — and the larger error is the yardstick.
        Lt, Xt = R.truth(Ku)
        Kd = device_gram(layer)
        Ld, Xd_sub, Xd_tri = R.lapack_reference(Kd)
        got["fwdX"] = R.forward_error(X, Xt)
        got["fwdX_ref"] = max(R.forward_error(A, Xt) for A in (ref["X_sub"], ref["X_tri"], Xd_sub, Xd_tri))
        got["fwdL_ref"] = max(R.forward_error(ref["L"], Lt), R.forward_error(Ld, Lt))
        # (for the record: both against the truth of the device-formed Ku — if the model's Ku is that matrix bit for bit, this is the
        # device and LAPACK on identical input)
        Ltd, Xtd = R.truth(Kd)
        got["fwdX_same"] = R.forward_error(X, Xtd) / max(R.forward_error(Xd_sub, Xtd), R.forward_error(Xd_tri, Xtd))
        if "Lu" in mats:
            got["fwdL"] = R.forward_error(L, Lt)
            got["fwdL_same"] = R.forward_error(L, Ltd) / R.forward_error(Ld, Ltd)
    row = [layer.name, path, str(int(white)), str(n), str(Mp), f"{ref['cond']:.2e}",
           _fmt(None if got["factor"] is None else got["factor"] / (1e-14 * n)), _fmt(got["left"]), _fmt(ref["left"]), _fmt(got["right"]),
           _fmt(ref["right"]), _fmt(got["congr"]), _fmt(ref["congr"]), _fmt(got["kinv"]), _fmt(ref.get("kinv")), _fmt(None if got["asym"] is None else got["asym"] / (n * R.EPS)),
           _fmt(got["fwdL"]), _fmt(got["fwdL_ref"]), _fmt(got["fwdL_same"]), _fmt(got["fwdX"]), _fmt(got["fwdX_ref"]), _fmt(got["fwdX_same"])]
    print("FACTOR_DIRECT | " + " | ".join(row))
    if record:
        _ROWS.append(row)
    if got["factor"] is not None:
        assert got["factor"] <= R.factor_bar(n), f"{tag}: factor backward error {got['factor']:.3e} > {R.factor_bar(n):.3e}"
        assert got["left"] <= R.device_bar(ref["left"], n), f"{tag}: |X L - I| scaled {got['left']:.3g}, CPU {ref['left']:.3g}"
        assert got["right"] <= R.device_bar(ref["right"], n), f"{tag}: |L X - I| scaled {got['right']:.3g}, CPU {ref['right']:.3g}"
    assert got["congr"] <= R.device_bar(ref["congr"], n), f"{tag}: |X Ku X^T - I| scaled {got['congr']:.3g}, CPU {ref['congr']:.3g}"
    if with_kinv:
        assert got["kinv"] <= R.device_bar(ref["kinv"], n), f"{tag}: |Ku^-1 Ku - I| scaled {got['kinv']:.3g}, CPU {ref['kinv']:.3g}"
        assert got["asym"] <= n * R.EPS, f"{tag}: Ku^-1 asymmetry {got['asym']:.3e} > n eps"
    if with_truth:
        assert got["fwdX"] <= R.DEVICE_FACTOR * got["fwdX_ref"], f"{tag}: forward error of Lu^-1 {got['fwdX']:.3e}, LAPACK {got['fwdX_ref']:.3e}"
        if got["fwdL"] is not None:
            assert got["fwdL"] <= R.DEVICE_FACTOR * got["fwdL_ref"], f"{tag}: forward error of Lu {got['fwdL']:.3e}, LAPACK {got['fwdL_ref']:.3e}"
    return got


_TRUTHS_DONE = []
_GRAM = {}


def device_gram(layer):
    """Ku of this layer as the DEVICE forms it (dsdgp_gram on the same Z and hyper-parameters), symmetric"""
    if layer.name not in _GRAM:
        from doubly_stochastic_dgp import _lib
        from doubly_stochastic_dgp.engine import Context
        ctx = Context.get()
        M = layer.M
        ls = np.array([layer.spec["lengthscales"]], dtype=np.float64)
        spec = _lib.KernelSpec(kind={"rbf": 0, "matern52": 1}[layer.kind], input_dim=layer.D, ard=0, has_white=0, variance=1.0,
                               white_variance=0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
        dZ, out = ctx.to_device(np.ascontiguousarray(layer.Z)), ctx.empty(M, M)
        ctx.torch.cuda.current_stream().synchronize()
        _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(spec), C.c_void_p(dZ.data_ptr()), M, None, 0, layer.jitter, C.c_void_p(out.data_ptr()), M))
        ctx.sync()
        K = out.cpu().numpy()
        assert np.array_equal(K, K.T)
        _GRAM[layer.name] = K
    return _GRAM[layer.name]


def ensure_truths():
    """the 40-digit factorisations of every Mp <= 128 matrix of this module (the reference Ku and the device-formed one), once, in
    worker processes"""
    if _TRUTHS_DONE:
        return
    _TRUTHS_DONE.append(1)
    todo = [Layer(f, M, k) for M in LDS_SIZES for f in R.FAMILIES for k in KINDS]
    todo += [Layer(f, M, jitter=j) for f, M, j in SINGLE_CASES] + [Layer("spread", 50, D=17), Layer("spread", 128, D=17)]
    R.truth_many([l.ku() for l in todo] + [device_gram(l) for l in todo])


def run_model(layers, path, env, monkeypatch, whites=(False, True)):
    for k in ("DSDGP_FORCE", "DSDGP_CHOL_LOOKAHEAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k != "DSDGP_BIG_MP"          # read once per process: the child process's
        monkeypatch.setenv(k, v)
    if any(padded(l.M) <= 128 for l in layers):
        ensure_truths()
    for white in whites:
        model = build_model(layers, white)
        for layer, mats in zip(layers, read_matrices(model, len(layers), white, layers[0].jitter)):
            check_matrix(layer, mats, path, white)


# ------------------------------------------------------------------------------------------------ the accessor itself
def test_lu_is_refused_where_no_path_keeps_it():
    from doubly_stochastic_dgp import _lib
    layer = Layer("spread", 50)
    eng = build_model([layer], False).engine()
    with pytest.raises(_lib.DsdgpError, match="keeps no Lu"):
        eng.layer_matrix(0, "Lu")
    out = np.zeros((64, 70))
    assert eng.lib.dsdgp_model_layer_matrix(eng.model, 0, _lib.MAT_LUINV, out.ctypes.data_as(C.c_void_p), 63) == -1      # ld_out < Mp
    assert eng.lib.dsdgp_model_layer_matrix(eng.model, 1, _lib.MAT_LUINV, out.ctypes.data_as(C.c_void_p), 70) == -1      # no such layer
    assert eng.lib.dsdgp_model_layer_matrix(eng.model, 0, 4, out.ctypes.data_as(C.c_void_p), 70) == -1
    out[:] = 7.0
    _lib.check(eng.lib.dsdgp_model_layer_matrix(eng.model, 0, _lib.MAT_LUINV, out.ctypes.data_as(C.c_void_p), 70))
    assert np.array_equal(out[:, :64], eng.layer_matrix(0, "Linv")) and np.all(out[:, 64:] == 7.0)


def test_device_gram_is_not_the_variable():
    """Ku as the device forms it (dsdgp_gram: the same expand-the-square distances as the head launch) against the reference Ku the other
    tests factor on the CPU.  With a_i = |z_i / l|^2 the distance r2 = a_i + a_j - 2 z_i . z_j carries (D + 2) eps (a_i + a_j + 2 |z_i . z_j|)
    <= 2 (D + 2) eps (a_i + a_j) of rounding on EACH side, and k = exp(-r2 / 2) <= 1 turns it into half of that plus the rounding of exp
    and of the jitter sum: |dK_ij| <= eps (2 (D + 2) (a_i + a_j) + 8)."""
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.engine import Context
    ctx = Context.get()
    for layer in (Layer("spread", 128), Layer("pairs", 128), Layer("grid1d", 100)):
        Z, M = layer.Z, layer.M
        ls = np.array([layer.spec["lengthscales"]], dtype=np.float64)
        spec = _lib.KernelSpec(kind=0, input_dim=layer.D, ard=0, has_white=0, variance=1.0, white_variance=0.0,
                               lengthscales=ls.ctypes.data_as(_lib.c_double_p))
        dZ, out = ctx.to_device(np.ascontiguousarray(Z)), ctx.empty(M, M)
        ctx.torch.cuda.current_stream().synchronize()
        _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(spec), C.c_void_p(dZ.data_ptr()), M, None, 0, layer.jitter, C.c_void_p(out.data_ptr()), M))
        ctx.sync()
        K = out.cpu().numpy()
        a = np.sum((Z / ls[0]) ** 2, axis=1)
        bound = R.EPS * (2 * (layer.D + 2) * (a[:, None] + a[None, :]) + 8)
        diff = np.abs(K - layer.ku())
        print(f"{layer.name}: max|Ku_dev - Ku_ref| = {diff.max():.2e} ({(diff / bound).max():.3f} of the bound)")
        assert np.array_equal(K, K.T) and np.all(diff <= bound)


# ------------------------------------------------------------------------------------------------ the LDS core, every size
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("M", LDS_SIZES)
def test_head_lds_core(monkeypatch, M, family, kind):
    """k_head / lds_chol_inverse<true>: one, two or three panel waves and every task striding of the idle waves"""
    run_model([Layer(family, M, kind)], "head", {}, monkeypatch)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("M", [17, 50, 100, 127, 128])
def test_one_workgroup_kernel_in_lds(monkeypatch, M, family):
    """k_potrf_trtri<true> (DSDGP_FORCE=head=0)"""
    run_model([Layer(family, M, "rbf" if M != 100 else "matern52")], "head=0", HEAD0, monkeypatch)


@pytest.mark.parametrize("family,M,D", [("spread", 140, None), ("pairs", 140, None), ("grid1d", 140, None), ("spread", 50, 17), ("spread", 128, 17)])
def test_one_workgroup_kernel_in_global_memory(monkeypatch, family, M, D):
    """k_potrf_trtri<false>: Mp = 160, and the D_in = 17 models the head launch refuses"""
    run_model([Layer(family, M, D=D)], "potrf-global", {}, monkeypatch)


@pytest.mark.parametrize("jitter_path", ["head", "head=0"])
def test_pairs_at_jitter_1e9_mp128(monkeypatch, jitter_path):
    """cond(Ku) about 1e10: finite results and the same bars, nothing tighter"""
    run_model([Layer("pairs", 128, jitter=1e-9)], jitter_path, HEAD0 if jitter_path == "head=0" else {}, monkeypatch)


# ------------------------------------------------------------------------------------------------ the blocked sequences
# one ill-conditioned matrix per size (the twins of `pairs` sit M / 2 apart: across the 128-row block borders); all three families at 448;
# n = 1024 is the exact size so that its products may be float64 (one matrix per path from there on)
LOOKAHEAD = [("pairs", 180), ("pairs", 250), ("pairs", 300), ("spread", 300), ("spread", 440), ("pairs", 440), ("grid1d", 440), ("grid1d", 500),
             ("pairs", 600), ("pairs", 1024)]


@pytest.mark.parametrize("family,M", LOOKAHEAD)
def test_lookahead_blocked_one_matrix(monkeypatch, family, M):
    """Mp = 192, 256, 320, 448, 512, 640, 1024: k_chol_block + k_chol_panel + wide update, the inverse by block rows (k_chol_xrow)"""
    assert padded(M) in (192, 256, 320, 448, 512, 640, 1024)
    run_model([Layer(family, M, "matern52" if M == 250 else "rbf")], "look-ahead", {}, monkeypatch)


def test_pairs_at_jitter_1e9_mp448(monkeypatch):
    run_model([Layer("pairs", 440, jitter=1e-9)], "look-ahead", {}, monkeypatch)


@pytest.mark.parametrize("Ms,family", [((300, 300), "pairs"), ((192, 192, 192), "spread")])
def test_lookahead_blocked_uniform_batch(monkeypatch, Ms, family):
    """L layers of the same M >= 192 share one batched sequence; the kernels differ per layer so that the matrices do"""
    kinds = ["rbf", "matern52", "rbf"]
    layers = [Layer(family, M, kinds[i]) for i, M in enumerate(Ms)]
    layers[-1].spec = dict(layers[-1].spec, lengthscales=1.3 * layers[-1].spec["lengthscales"])
    layers[-1].name += "-ls1.3"
    run_model(layers, f"look-ahead x{len(Ms)}", {}, monkeypatch)


@pytest.mark.parametrize("Ms", [(128, 50, 100), (300, 60)])
def test_mixed_sizes_in_one_model(monkeypatch, Ms):
    """(128, 50, 100): three factorisations of different size in ONE head launch (LDS sized by the largest);
    (300, 60): a blocked sequence and the one-workgroup kernel side by side"""
    layers = [Layer("pairs" if Ms == (300, 60) else "spread", M, KINDS[i % 2]) for i, M in enumerate(Ms)]
    run_model(layers, "mixed " + "/".join(str(m) for m in Ms), {}, monkeypatch)


@pytest.mark.parametrize("family,M", [("pairs", 300), ("grid1d", 600)])
def test_plain_blocked_sequence(monkeypatch, family, M):
    """DSDGP_CHOL_LOOKAHEAD=0 (read when a plan is built): panel and trailing update as GEMM launches, recursive doubling, k_transpose_lower"""
    run_model([Layer(family, M)], "plain blocked", PLAIN, monkeypatch)


def test_gemm_only_size(monkeypatch):
    """Mp = 1152 (M = 1100): nine diagonal blocks, the size class only the GEMM-formulated layers take"""
    run_model([Layer("pairs", 1100)], "look-ahead (GEMM layers)", {}, monkeypatch)


# ------------------------------------------------------------------------------------------------ k_chol_block alone (child process)
SINGLE_CASES = [("spread", 128, 1e-6), ("pairs", 128, 1e-6), ("grid1d", 127, 1e-6), ("pairs", 128, 1e-9)]


def _child(out_path):
    """DSDGP_BIG_MP=128 is read once per process: this process reads the matrices, the parent checks them"""
    assert os.environ.get("DSDGP_BIG_MP") == "128" and os.environ.get("DSDGP_FORCE") == "head=0"
    out = {}
    for i, (family, M, jitter) in enumerate(SINGLE_CASES):
        layer = Layer(family, M, jitter=jitter)
        for white in (False, True):
            mats = read_matrices(build_model([layer], white), 1, white, jitter)[0]
            for k, v in mats.items():
                out[f"{i}_{int(white)}_{k}"] = v
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def single_block(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("single_block") / "mats.npz")
    env = dict(os.environ, **SINGLE)
    env.pop("DSDGP_CHOL_LOOKAHEAD", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(path)


@pytest.mark.parametrize("i", range(len(SINGLE_CASES)), ids=[f"{f}-M{M}-j{j:g}" for f, M, j in SINGLE_CASES])
def test_block_kernel_as_a_single_block(single_block, i):
    """k_chol_block with one 128-block (bigchol_build accepts n = 128: the plain sequence with no panel, the inverse of the diagonal block
    is the whole inverse, Lu^-T by k_transpose_lower)"""
    family, M, jitter = SINGLE_CASES[i]
    layer = Layer(family, M, jitter=jitter)
    ensure_truths()
    for white in (False, True):
        mats = {k.split("_", 2)[2]: single_block[k] for k in single_block.files if k.startswith(f"{i}_{int(white)}_")}
        assert set(mats) == {"Linv", "LinvT", "Kinv"} | ({"Lu"} if white else set())
        check_matrix(layer, mats, "single block", white)


@pytest.mark.parametrize("i", [0, 1], ids=["spread", "pairs"])
def test_paths_agree_to_rounding_at_mp128(monkeypatch, single_block, i):
    """The same matrix through the head launch, the one-workgroup kernel and the block kernel: each meets the bars on its own (the tests
    above); here the largest entrywise difference of Lu^-1 between them goes into the profile.  No bitwise equality is asked for — only
    that each pair differs by no more than both forward errors allow (8 x LAPACK's each, as item 5)."""
    family, M, jitter = SINGLE_CASES[i]
    layer = Layer(family, M, jitter=jitter)
    ensure_truths()
    ref = reference(layer)
    Lt, Xt = R.truth(layer.ku())
    fwd_ref = max(R.forward_error(ref["X_sub"], Xt), R.forward_error(ref["X_tri"], Xt))
    got = {"single block": single_block[f"{i}_0_Linv"]}
    for path, env in (("head", {}), ("head=0", HEAD0)):
        monkeypatch.delenv("DSDGP_FORCE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got[path] = read_matrices(build_model([layer], False), 1, False, jitter)[0]["Linv"]
    names = sorted(got)
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            A, B = got[names[a]][:M, :M], got[names[b]][:M, :M]
            big = np.maximum(np.abs(A), np.abs(B))
            ulps = float(np.max(np.abs(A - B) / np.spacing(np.where(big > 0, big, 1.0))))
            rel = float(np.max(np.abs(A - B)) / np.max(np.abs(A)))
            _ULPS.append([layer.name, f"{names[a]} vs {names[b]}", f"{ulps:.3g} (max|dX| / max|X| = {rel:.2e})"])
            print("FACTOR_DIRECT_ULPS | " + " | ".join(_ULPS[-1]))
            assert rel <= 2 * R.DEVICE_FACTOR * fwd_ref


# ------------------------------------------------------------------------------------------------ the never-written halves over a run
def _current_layers(model, layers):
    """the layers with Z and the kernel's parameters as the device holds them now"""
    now = []
    for layer, pl in zip(layers, model.layers):
        from doubly_stochastic_dgp.gpflow_compat import split_kernel
        stat, _ = split_kernel(pl.kern)
        cur = Layer(layer.family, layer.M, layer.kind, layer.jitter)
        cur.Z = np.array(pl.feature.Z.value, dtype=np.float64)
        cur.spec = dict(layer.spec, variance=float(stat.variance.value), lengthscales=float(np.ravel(stat.lengthscales.value)[0]))
        now.append(cur)
    return now


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("M", [128, 300, 600])
def test_never_written_halves_stay_zero_over_a_run(monkeypatch, M, white):
    """The look-ahead sequence and the LDS core never write the upper half of Lu^-1 nor the lower half of Lu^-T: they rely on the one
    clearing of the workspace at model creation (linalg.hpp, model_layout.hpp).  Twenty Adam steps, a natural-gradient step on the last
    layer, a prediction on more rows than the training batch (which re-creates the device model), a full-covariance prediction and one more
    step: after each stage the structure is exact and the factor / inverse of the THEN-CURRENT Ku (rebuilt from the parameters read back)
    meet the bars."""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.training import NatGradOptimizer
    for k in ("DSDGP_FORCE", "DSDGP_CHOL_LOOKAHEAD"):
        monkeypatch.delenv(k, raising=False)
    layers = [Layer("spread", M, "rbf"), Layer("spread", M, "matern52")]
    rng = np.random.RandomState(M)
    N, D = 32, 3
    X, Y = rng.randn(N, D), rng.randn(N, 1)
    model = make_case(X, Y, layers[0].Z, [l.spec for l in layers], white=white, jitter=1e-6, S=2, seed=5)[2]
    Xs = rng.randn(3 * N, D)

    def stage(name):
        with settings.temp_jitter(1e-6):
            mats = read_matrices(model, 2, white, 1e-6)
            for l, cur in enumerate(_current_layers(model, layers)):
                ref = R.reference_measures(cur.ku(), with_kinv=False)
                check_matrix(cur, mats[l], f"run: {name}, layer {l}", white, with_kinv=False, with_truth=False, ref=ref, record=False)

    with settings.temp_jitter(1e-6):
        stage("created")
        for _ in range(20):
            model.train_step(0.01, X=X, Y=Y)
        stage("20 Adam steps")
        last = model.layers[-1]
        NatGradOptimizer(0.1).minimize(model, var_list=[[last.q_mu, last.q_sqrt]], maxiter=1, X=X, Y=Y)
        stage("natural-gradient step")
        model.predict_f(Xs, 2)
        stage("predict on 3 x the rows")
        model.predict_f_full_cov(Xs[:40], 2)
        stage("full-covariance predict")
        model.train_step(0.01, X=X, Y=Y, sync=True)
        stage("one more step")


# ------------------------------------------------------------------------------------------------ dsdgp_potrf: edges of the primitive
@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


def _potrf(ctx, A, n, lda=None, stride=None, batch=1):
    lda = lda or n
    stride = stride or lda * n
    dA = ctx.to_device(np.ascontiguousarray(A, dtype=np.float64))
    info = C.c_int(-1)
    ctx.torch.cuda.current_stream().synchronize()
    rc = ctx.lib.dsdgp_potrf(ctx.handle, batch, n, C.c_void_p(dA.data_ptr()), lda, stride, C.byref(info))
    ctx.sync()
    return rc, info.value, dA.cpu().numpy()


@pytest.mark.parametrize("bad", [-1.0, 0.0])
@pytest.mark.parametrize("n", [16, 128, 176, 192, 640])
def test_potrf_reports_the_failing_pivot_exactly(ctx, n, bad):
    """I with one bad diagonal entry: the first failing pivot is that position, by construction; of two bad pivots the smaller is reported"""
    from doubly_stochastic_dgp import _lib
    for p in sorted({1, 16, 17, n}):
        if p > n:
            continue
        A = np.eye(n)
        A[p - 1, p - 1] = bad
        rc, info, _ = _potrf(ctx, A, n)
        assert (rc, info) == (_lib.ERR_NOT_SPD, p), (n, p, bad, rc, info)
    if n > 17:
        A = np.eye(n)
        A[n - 1, n - 1] = bad
        A[16, 16] = -1.0
        rc, info, _ = _potrf(ctx, A, n)
        assert (rc, info) == (_lib.ERR_NOT_SPD, 17), (n, bad, rc, info)


@pytest.mark.parametrize("n", [16, 128, 176, 640])
def test_potrf_pivots_of_a_diagonal_matrix_are_rounded_square_roots(ctx, n):
    """A = diag(d): L = diag(sqrt(d)) exactly, every pivot is one hardware reciprocal-square-root seed refined by Newton steps and one
    product.  A converged step inv (1.5 - 0.5 a inv^2) evaluated with an fma carries three roundings (2.5 u with u = 2^-53, the 0.5 a inv
    product counting half), l = a inv a fourth: |l - sqrt(a)| <= 3 u |l| = 1.5 eps to first order; the bar is 2 eps.  A refinement that
    stops one step early leaves 1.5 x the square of the seed's error on top."""
    rng = np.random.RandomState(n)
    d = 10.0 ** rng.uniform(-3.0, 3.0, n)
    rc, info, L = _potrf(ctx, np.diag(d), n)
    assert (rc, info) == (0, 0)
    assert not np.any(L - np.diag(np.diag(L)))
    err = np.abs(np.asarray(np.diag(L), dtype=R.LD) - np.sqrt(np.asarray(d, dtype=R.LD))) / np.sqrt(d)
    print(f"n={n}: max |l_ii - sqrt(d_i)| / sqrt(d_i) = {float(err.max()) / R.EPS:.3f} eps")
    assert float(err.max()) <= 2 * R.EPS


@pytest.mark.parametrize("n,p", [(50, 1), (50, 23), (50, 50), (320, 1), (320, 129), (320, 200), (320, 320)])
def test_potrf_reports_a_nan_on_the_diagonal_as_that_pivot(ctx, n, p):
    """the pivot test is !(a_jj > 0): a NaN fails it"""
    from doubly_stochastic_dgp import _lib
    rng = np.random.RandomState(n)
    A = rng.randn(n, n)
    A = A @ A.T + n * np.eye(n)
    A[p - 1, p - 1] = np.nan
    rc, info, _ = _potrf(ctx, A, n)
    assert (rc, info) == (_lib.ERR_NOT_SPD, p), (rc, info)


@pytest.mark.parametrize("n", [100, 448])
def test_potrf_is_invariant_under_diagonal_scaling(ctx, n):
    """D A D with D = diag(10^linspace(-100, 100, n)): entries from 1e-200 to 1e200.  Cholesky commutes with a diagonal scaling up to
    rounding, so |L L^T - D A D|_ij <= 1e-14 n sqrt(a_ii a_jj) entrywise (LAPACK meets it: checked here on the same matrix).  A
    shortened Newton refinement of the reciprocal square root or an absolute threshold in the pivot test shows up here first."""
    Z, spec = R.family_case("spread", n)
    A = R.reference_ku(Z, spec, 1e-6)
    d = 10.0 ** np.linspace(-100.0, 100.0, n)
    DAD = A * d[:, None] * d[None, :]
    DAD = np.tril(DAD) + np.tril(DAD, -1).T
    rc, info, L = _potrf(ctx, DAD, n)
    assert (rc, info) == (0, 0)
    L = np.tril(L)
    dg = np.sqrt(np.diag(DAD))
    scale = 1e-14 * n * dg[:, None] * dg[None, :]

    def worst(Lx):
        # D^-1 L is the factor of A up to rounding: form the residual in the scaled frame, where nothing over- or underflows
        Ls = (np.asarray(Lx, dtype=R.LD) / d[:, None].astype(R.LD))
        As = np.asarray(DAD, dtype=R.LD) / d[:, None].astype(R.LD) / d[None, :].astype(R.LD)
        return float(np.max(np.abs(R.xprod(Ls, Ls.T, a_lower=True) - As) / (scale / d[:, None] / d[None, :])))

    w_ref, w_dev = worst(np.linalg.cholesky(DAD)), worst(L)
    print(f"n={n}: worst entry / bar: LAPACK {w_ref:.3g}, device {w_dev:.3g}")
    assert np.all(np.isfinite(L)) and w_ref <= 1.0 and w_dev <= 1.0


@pytest.mark.parametrize("n", [50, 128, 320])
def test_potrf_leaves_the_gaps_of_a_strided_batch_alone(ctx, n):
    """lda > n and stride > lda n: the sentinel between rows and between matrices is untouched, the factors are right"""
    rng = np.random.RandomState(n)
    batch, lda = 2, n + 3
    stride = lda * n + 7
    buf = np.full(batch * stride, 7.25)
    As = []
    for b in range(batch):
        A = rng.randn(n, n)
        A = A @ A.T + n * np.eye(n)
        As.append(A)
        view = buf[b * stride: b * stride + lda * n].reshape(n, lda)
        view[:, :n] = A
    rc, info, out = _potrf(ctx, buf, n, lda=lda, stride=stride, batch=batch)
    assert (rc, info) == (0, 0)
    mask = np.ones(batch * stride, dtype=bool)
    for b in range(batch):
        view = out[b * stride: b * stride + lda * n].reshape(n, lda)
        L = np.tril(view[:, :n])
        assert np.max(np.abs(L @ L.T - As[b])) / np.max(np.abs(As[b])) <= 1e-14 * n
        m = mask[b * stride: b * stride + lda * n].reshape(n, lda)
        m[:, :n] = False
    assert np.all(out[mask] == 7.25)


def test_potrf_rebuilds_the_context_held_plan(ctx):
    """n = 192, then 256, then 192 with batch 2, then 192 again on ONE context: every call finds another plan's key, frees that plan (one
    device block: bigchol_free) and builds its own.  The last call gives the first call's bits, and every factor meets the factor bar."""
    rng = np.random.RandomState(192)
    As = {}
    for n in (192, 256):
        A = rng.randn(2, n, n)
        As[n] = A @ A.transpose(0, 2, 1) + n * np.eye(n)
    got = []
    for n, batch in ((192, 1), (256, 1), (192, 2), (192, 1)):
        rc, info, L = _potrf(ctx, As[n][:batch], n, batch=batch)
        assert (rc, info) == (0, 0), (n, batch, rc, info)
        L = L.reshape(batch, n, n)
        for b in range(batch):
            assert not np.any(np.triu(L[b], 1))
            err = R.factor_backward(L[b], As[n][b])
            print(f"n={n} batch={batch} matrix {b}: factor backward error {err:.3e} (bar {R.factor_bar(n):.3e})")
            assert err <= R.factor_bar(n), (n, batch, b, err)
        got.append(L)
    assert np.array_equal(got[3], got[0])


if __name__ == "__main__":
    _child(sys.argv[1])

"""-m gpu: the stack of sparse sampled layers on the device (csrc/sgpmc_stack.hip; dsdgp_stack_propagate, dsdgp_stack_logdensity) against
tests/sgpmc_stack_reference.py on the cases of tests/sgpmc_stack_cases.py.

Bar, the project's, per output array in the max norm: the truth is long double; the device is within
8 max(the float64 twin's own error on that array, 2^-50 of the array's largest magnitude) of it — each layer's F, Fmean and var; the
value, the data term and the prior; each gradient block.  The bar comes from the reference alone.  Drawn z are dsdgp_randn(seed, l) bit
for bit; a second call and any subset of the optional outputs give the same bits; guard memory around every output stays untouched; a
failed factorisation in the middle layer writes nothing; a one-layer stack with S = 1 is SGPMC_Layer.conditional_device plus the
likelihood read-out, bit for bit.  DSDGP_STACK_PROFILE=<file> writes the measured ratio of every array, 1 = at the bar
(profiles/sgpmc_stack_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sgpmc_stack_cases as KC
from tests import sgpmc_stack_reference as KR

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_SPD, UNSUPPORTED = -1, -2, -4
CANARY = -12345.25
GUARD = 16
LIK = {"gaussian": 0, "multiclass": 1, "bernoulli": 2, "poisson": 3, "student_t": 5}
MEAN = {"zero": 0, "identity": 1, "linear": 2}
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_STACK_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Stack of sparse sampled layers: measured errors (tests/test_gpu_sgpmc_stack.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar: max |device - truth| over an output array, over\n"
                "8 max(the float64 twin's own error on that array, 2^-50 of the array's largest magnitude); the truth is the long-double\n"
                "evaluation of tests/sgpmc_stack_reference.py.  One line per case: the worst array of each group and its name.\n\n"
                "| case | L | R | likelihood | F | Fmean | var | value, data, prior | gradient blocks | worst array |\n|" + "---|" * 10 + "\n")
        for r in _ROWS:
            f.write("| %s | %d | %d | %s | %.3g | %.3g | %.3g | %.3g | %.3g | %s |\n" % r)


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _desc(ctx, c, jitter=None, variance_of=None):
    """(StackDesc of the case, what it points to).  variance_of: {layer: kernel variance} to override"""
    from doubly_stochastic_dgp import _lib
    keep = []
    d = _lib.StackDesc()
    d.L = len(c["layers"])
    d.lik_kind, d.lik_p0, d.lik_p1 = LIK[c["lik"][0]], c["lik"][1], c["lik"][2]
    d.lik_width = c["layers"][-1]["DO"]
    d.jitter = c["jitter"] if jitter is None else jitter
    for l, y in enumerate(c["layers"]):
        ls = np.ascontiguousarray(y["ls"], dtype=np.float64)
        t = d.layers[l]
        t.kern = _lib.KernelSpec(kind=y["kind"], input_dim=y["D"], ard=int(y["ard"]), has_white=int(y["white_var"] is not None),
                                 variance=(variance_of or {}).get(l, y["variance"]), white_variance=y["white_var"] or 0.0,
                                 lengthscales=ls.ctypes.data_as(_lib.c_double_p))
        Z, q = ctx.to_device(y["Z"]), ctx.to_device(y["q_mu"])
        t.Z, t.q_mu, t.M, t.DO, t.white, t.mean_kind, t.input_prop_dim = Z.data_ptr(), q.data_ptr(), y["M"], y["DO"], int(y["white"]), \
            MEAN[y["mean"]], y["p"]
        keep += [ls, Z, q]
        if y["mean"] == "linear":
            A, b = ctx.to_device(y["A"]), ctx.to_device(y["b"])
            t.mean_A, t.mean_b = A.data_ptr(), b.data_ptr()
            keep += [A, b]
    return d, keep


def _scratch(ctx, d, c, reverse):
    need = C.c_int64()
    assert ctx.lib.dsdgp_stack_scratch_bytes(C.byref(d), c["n"], c["S"], int(reverse), C.byref(need)) == 0, ctx.lib.dsdgp_last_error()
    return ctx.empty(need.value // 8 + 32), need.value


def _guarded(ctx, count):
    return ctx.empty(2 * GUARD + count).fill_(CANARY)


def _guards_intact(bufs):
    return all(bool((b[:GUARD] == CANARY).all()) and bool((b[-GUARD:] == CANARY).all()) for b in bufs)


def _untouched(bufs):
    return all(bool((b == CANARY).all()) for b in bufs)


def _zs(ctx, c, given):
    L = len(c["layers"])
    arr, keep = (C.c_void_p * L)(), []
    if given:
        for l, z in enumerate(c["zs"]):
            t = ctx.to_device(z)
            keep.append(t)
            arr[l] = t.data_ptr()
    return arr, keep


def _propagate(ctx, c, want=("F", "mean", "var"), given=None, jitter=None, variance_of=None, layers_wanted=None):
    """-> (rc, {key: [numpy per layer or None]}, guard buffers, info)"""
    d, keep = _desc(ctx, c, jitter, variance_of)
    L, R = len(c["layers"]), c["n"] * c["S"]
    scr, nbytes = _scratch(ctx, d, c, False)
    given = c["zmode"] == "given" if given is None else given
    zarr, zkeep = _zs(ctx, c, given)
    ptrs, bufs, views = {}, [], {}
    for k in ("F", "mean", "var"):
        ptrs[k], views[k] = (C.c_void_p * L)(), [None] * L
        for l, y in enumerate(c["layers"]):
            if k not in want or (layers_wanted is not None and l not in layers_wanted):
                continue
            w = {"F": (y["p"] + y["DO"]) if l + 1 < L else y["DO"], "mean": y["DO"], "var": 1}[k]
            b = _guarded(ctx, R * w)
            bufs.append(b)
            views[k][l] = (b[GUARD:-GUARD], (R, w) if k != "var" else (R,))
            ptrs[k][l] = b[GUARD:-GUARD].data_ptr()
    info = C.c_int(-7)
    X = ctx.to_device(c["X"])
    rc = ctx.lib.dsdgp_stack_propagate(ctx.handle, C.byref(d), _p(X), c["n"], c["S"], zarr, C.c_uint64(KC.DRAW_SEED),
                                       _p(scr), nbytes, ptrs["F"], ptrs["mean"], ptrs["var"], C.byref(info))
    ctx.sync()
    out = {k: [None if v is None else v[0].cpu().numpy().reshape(v[1]) for v in views[k]] for k in views}
    return rc, out, bufs, info.value


def _grad_count(c):
    return 1 + sum(y["M"] * y["D"] + y["M"] * y["DO"] + 2 + (y["D"] if y["ard"] else 1) for y in c["layers"])


def _split(c, grad):
    out, at = {}, 0
    for l, y in enumerate(c["layers"]):
        M, D, DO, nls = y["M"], y["D"], y["DO"], (y["D"] if y["ard"] else 1)
        out["l%d_Z" % l] = grad[at:at + M * D].reshape(M, D); at += M * D
        out["l%d_q_mu" % l] = grad[at:at + M * DO].reshape(M, DO); at += M * DO
        out["l%d_variance" % l], out["l%d_lengthscales" % l], out["l%d_diag" % l] = grad[at:at + 1], grad[at + 1:at + 1 + nls], grad[at + 1 + nls:at + 2 + nls]
        at += 2 + nls
    out["lik"] = grad[at:at + 1]
    assert at + 1 == grad.size
    return out


def _logdensity(ctx, c, with_grad=True, given=None, jitter=None, variance_of=None):
    """-> (rc, {value, data, prior, info, l<i>_<key>..., lik}, guard buffers, info)"""
    d, keep = _desc(ctx, c, jitter, variance_of)
    scr, nbytes = _scratch(ctx, d, c, with_grad)
    given = c["zmode"] == "given" if given is None else given
    zarr, zkeep = _zs(ctx, c, given)
    ob, gb = _guarded(ctx, 4), _guarded(ctx, _grad_count(c)) if with_grad else None
    info = C.c_int(-7)
    X, Y = ctx.to_device(c["X"]), ctx.to_device(c["Y"])
    rc = ctx.lib.dsdgp_stack_logdensity(ctx.handle, C.byref(d), _p(X), _p(Y), c["n"], c["S"], zarr,
                                        C.c_uint64(KC.DRAW_SEED), c["data_scale"], _p(scr), nbytes, _p(ob[GUARD:-GUARD]),
                                        _p(gb[GUARD:-GUARD]) if with_grad else None, C.byref(info))
    ctx.sync()
    o = ob[GUARD:-GUARD].cpu().numpy()
    out = dict(value=o[:1].copy(), data=o[1:2].copy(), prior=o[2:3].copy(), info=o[3:4].copy())
    if with_grad:
        out.update(_split(c, gb[GUARD:-GUARD].cpu().numpy()))
    return rc, out, [ob] + ([gb] if with_grad else []), info.value


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _device_draws(ctx, c):
    """dsdgp_randn(DRAW_SEED, stream = l, R DO_l) of every sampled layer, as (R, DO_l) numpy arrays"""
    R, zs = c["n"] * c["S"], []
    for l, y in enumerate(c["layers"][:-1]):
        t = ctx.empty(R * y["DO"])
        assert ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(KC.DRAW_SEED), C.c_uint64(l), R * y["DO"], _p(t)) == 0
        ctx.sync()
        zs.append(t.cpu().numpy().reshape(R, y["DO"]))
    return zs


_REFERENCE = {}


def _reference(ctx, name):
    """(case, truth and twin of propagate, truth and twin of logdensity as flat arrays).  A case with given draws: the table's, computed
    once per process.  A case with drawn ones: the reference on the draws the DEVICE makes (the host restatement of the generator, which
    the table's conditions were checked on, agrees with them to a few ulp but not bit for bit: its logarithm and cosine are libm's)."""
    if name not in _REFERENCE:
        c = KC.case(name)
        if c["zmode"] == "given":
            _REFERENCE[name] = (c, KC.propagate(name), KC.propagate(name, np.float64), KR.flat_arrays(KC.logdensity(name)),
                                KR.flat_arrays(KC.logdensity(name, np.float64)))
        else:
            c = dict(c, zs=_device_draws(ctx, c))
            _REFERENCE[name] = (c, KR.propagate(c), KR.propagate(c, np.float64), KR.flat_arrays(KR.logdensity(c)),
                                KR.flat_arrays(KR.logdensity(c, np.float64)))
    return _REFERENCE[name]


@pytest.mark.parametrize("name", KC.NAMES)
def test_every_output_array_is_within_the_bar_of_the_truth(ctx, name):
    c, pt, p64, lt, l64 = _reference(ctx, name)
    L, R = len(c["layers"]), c["n"] * c["S"]
    rc, fw, bufs, info = _propagate(ctx, c)
    assert rc == 0 and info == 0, ctx.lib.dsdgp_last_error()
    assert _guards_intact(bufs)
    rc, ld, bufs, info = _logdensity(ctx, c)
    assert rc == 0 and info == 0, ctx.lib.dsdgp_last_error()
    assert _guards_intact(bufs) and ld["info"][0] == 0.0
    figs = {}
    for k, rk in (("F", "F"), ("mean", "Fmean"), ("var", "var")):
        for l in range(L):
            assert np.all(np.isfinite(fw[k][l]))
            figs["%s%d" % (rk, l)] = KC.ratio(fw[k][l], pt[rk][l], p64[rk][l])
    for k in lt:
        assert np.all(np.isfinite(ld[k])), k
        figs[k] = KC.ratio(ld[k], lt[k], l64[k])
    # the last layer is not sampled: its F is its mean; the propagated columns are copies
    assert _same_bits(fw["F"][L - 1], fw["mean"][L - 1])
    Xin = np.tile(c["X"], (c["S"], 1))
    for l, y in enumerate(c["layers"][:-1]):
        assert _same_bits(fw["F"][l][:, :y["p"]], Xin[:, :y["p"]])
        Xin = fw["F"][l]
    # a second call: the same bits
    fw2, ld2 = _propagate(ctx, c)[1], _logdensity(ctx, c)[1]
    assert all(_same_bits(fw2[k][l], fw[k][l]) for k in fw for l in range(L))
    assert all(_same_bits(ld2[k], ld[k]) for k in ld)
    # the value without a gradient: the same bits
    rc, val, bufs, _ = _logdensity(ctx, c, with_grad=False)
    assert rc == 0 and _guards_intact(bufs) and all(_same_bits(val[k], ld[k]) for k in ("value", "data", "prior"))
    group = lambda pre: max((v, k) for k, v in figs.items() if k.startswith(pre))
    worst = max((v, k) for k, v in figs.items())
    grads = max((v, k) for k, v in figs.items() if k[0] == "l")
    scal = max(figs["value"], figs["data"], figs["prior"])
    for k, v in sorted(figs.items()):
        print("%s %s: %.3g (x bar)" % (name, k, v))
    _ROWS.append((name, L, R, c["lik"][0], max(v for k, v in figs.items() if k[0] == "F" and not k.startswith("Fmean")),
                  group("Fmean")[0], group("var")[0], scal, grads[0], "%s (%.3g)" % (worst[1], worst[0])))
    for k, v in figs.items():
        assert v <= 1.0, (k, v)


def test_a_row_of_exactly_zero_variance_is_its_mean(ctx):
    c = KC.case(KC.FORWARD_ONLY)
    pt, p64 = KC.propagate(KC.FORWARD_ONLY), KC.propagate(KC.FORWARD_ONLY, np.float64)
    rc, fw, bufs, info = _propagate(ctx, c)
    assert rc == 0 and info == 0 and _guards_intact(bufs), ctx.lib.dsdgp_last_error()
    rows = np.arange(KC.ZERO_ROW, c["n"] * c["S"], c["n"])
    assert np.all(fw["var"][0][rows] == 0.0) and _same_bits(fw["F"][0][rows], fw["mean"][0][rows])
    for k, rk in (("F", "F"), ("mean", "Fmean"), ("var", "var")):
        for l in range(2):
            fig = KC.ratio(fw[k][l], pt[rk][l], p64[rk][l])
            print("%s %s%d: %.3g (x bar)" % (KC.FORWARD_ONLY, rk, l, fig))
            assert fig <= 1.0, (rk, l, fig)


HOPS = [  # R, D_in, DO, p, mean
    (1, 2, 1, 0, "zero"), (255, 3, 3, 2, "identity"), (257, 5, 3, 0, "linear"), (800, 17, 16, 2, "linear_b"), (513, 2, 17, 2, "zero")]


@pytest.mark.parametrize("R,D,DO,p,mean", HOPS)
def test_the_hop_and_its_reverse_on_their_own(ctx, R, D, DO, p, mean):
    """dsdgp_stack_hop / dsdgp_stack_hop_bwd — the launches of the composed calls — on arrays of the test's own at the ragged row counts,
    entry by entry within 8 max(e64, 2^-50 mag) of the long-double formulas (e64: the float64 numpy sequence, mag: the sum of the
    magnitudes of the terms added into the entry).  One row has var + jitter = 0 exactly: its sample is its mean, bit for bit; its gv has
    no finite value and is left out of the comparison."""
    LD = np.longdouble
    rng = np.random.default_rng(R + 7 * DO)
    jitter = 0.25
    cm, Xin, z, dF = rng.standard_normal((R, DO)), rng.standard_normal((R, D)), rng.standard_normal((R, DO)), rng.standard_normal((R, p + DO))
    var = rng.uniform(0.0, 2.0, R)
    var[R // 2] = -jitter
    A = rng.standard_normal((D, DO)) if mean.startswith("linear") else None
    b = rng.standard_normal(DO) if mean == "linear_b" else None
    kind = MEAN[mean.split("_")[0]]
    dev = {k: ctx.to_device(v) for k, v in dict(cm=cm, Xin=Xin, z=z, dF=dF, var=var).items()}
    lin = None
    if A is not None:
        lin = ctx.empty(R, DO)
        ctx.gemm(0, 0, 1.0, dev["Xin"], ctx.to_device(A), 0.0, lin)
        ctx.sync()
    bd = None if b is None else ctx.to_device(b)
    bufs = {k: _guarded(ctx, n) for k, n in dict(Fmean=R * DO, F=R * (p + DO), gm=R * DO, gv=R).items()}
    o = {k: v[GUARD:-GUARD] for k, v in bufs.items()}
    assert ctx.lib.dsdgp_stack_hop(ctx.handle, _p(dev["cm"]), _p(dev["var"]), _p(dev["Xin"]), R, D, kind, _p(lin), _p(bd), p, DO, _p(dev["z"]),
                                   jitter, _p(o["Fmean"]), _p(o["F"])) == 0, ctx.lib.dsdgp_last_error()
    assert ctx.lib.dsdgp_stack_hop_bwd(ctx.handle, _p(dev["dF"]), R, p, DO, _p(dev["z"]), _p(dev["var"]), jitter, _p(o["gm"]), _p(o["gv"])) == 0
    ctx.sync()
    assert _guards_intact(bufs.values())
    Fmean, F = o["Fmean"].cpu().numpy().reshape(R, DO), o["F"].cpu().numpy().reshape(R, p + DO)
    gm, gv = o["gm"].cpu().numpy().reshape(R, DO), o["gv"].cpu().numpy()
    linh = None if lin is None else lin.cpu().numpy()          # the product is dsdgp_gemm's, with tests of its own: the hop adds it

    def formulas(dt):
        t = lambda x: np.asarray(x, dtype=dt)
        m = {0: 0.0, 1: t(Xin) if kind == 1 else 0.0, 2: (t(linh) + (t(b) if b is not None else dt(0.0))) if kind == 2 else 0.0}[kind]
        fm, fm_mag = t(cm) + m, np.abs(t(cm)) + np.abs(m)
        s = np.sqrt(t(var) + dt(jitter))[:, None]
        sample, sample_mag = fm + t(z) * s, fm_mag + np.abs(t(z)) * s
        terms = t(dF)[:, p:] * t(z)
        with np.errstate(divide="ignore", invalid="ignore"):
            g, g_mag = np.sum(terms, 1) / (dt(2.0) * s[:, 0]), np.sum(np.abs(terms), 1) / (dt(2.0) * s[:, 0])
        return dict(Fmean=(fm, fm_mag), sample=(sample, sample_mag), gv=(g, g_mag))

    tr, tw = formulas(LD), formulas(np.float64)
    keep = np.arange(R) != R // 2
    for k, got in (("Fmean", Fmean), ("sample", F[:, p:]), ("gv", gv)):
        (t, mag), (w, _) = tr[k], tw[k]
        if k == "gv":
            got, t, mag, w = got[keep], t[keep], mag[keep], w[keep]
            if got.size == 0:
                continue
        barr = 8.0 * np.maximum(np.abs(w - t).astype(np.float64), 2.0 ** -50 * mag.astype(np.float64))
        err = np.abs(got - t).astype(np.float64)
        fig = float(np.max(err / np.where(barr == 0.0, 1.0, barr))) if not np.any((barr == 0.0) & (err != 0.0)) else float("inf")
        print("hop R = %d DO = %d p = %d %s: %s %.3g (x bar)" % (R, DO, p, mean, k, fig))
        assert fig <= 1.0, (k, fig)
    assert _same_bits(F[:, :p], Xin[:, :p]) and _same_bits(gm, dF[:, p:])
    assert _same_bits(F[R // 2, p:], Fmean[R // 2])                     # var + jitter = 0: the sample is the mean
    # bad arguments launch nothing
    launches = ctx.lib.dsdgp_launch_count()
    assert ctx.lib.dsdgp_stack_hop(ctx.handle, _p(dev["cm"]), _p(dev["var"]), _p(dev["Xin"]), R, D, 1 if D != DO else 7, None, None, p, DO,
                                   _p(dev["z"]), jitter, None, _p(o["F"])) == BAD_ARG
    assert ctx.lib.dsdgp_stack_hop_bwd(ctx.handle, _p(dev["dF"]), 0, p, DO, _p(dev["z"]), _p(dev["var"]), jitter, _p(o["gm"]), _p(o["gv"])) == BAD_ARG
    assert ctx.lib.dsdgp_launch_count() == launches


@pytest.mark.parametrize("name", ("r257", "student"))
def test_drawn_z_is_dsdgp_randn_bit_for_bit(ctx, name):
    """Without zs the draws of layer l are dsdgp_randn(seed, stream = l, R DO_l): every output has the bits of a call that is GIVEN
    those draws."""
    c = KC.case(name)
    drawn = _propagate(ctx, c, given=False)[1]
    zs = _device_draws(ctx, c)
    for l, z in enumerate(zs):                                          # the host restatement: the same draws to a few ulp
        assert np.all(np.abs(z - c["zs"][l]) <= 2.0 ** -48 * np.maximum(np.abs(z), 1.0)), l
    given = _propagate(ctx, dict(c, zs=zs), given=True)[1]
    assert all(_same_bits(given[k][l], drawn[k][l]) for k in drawn for l in range(len(c["layers"])))
    a, b = _logdensity(ctx, c, given=False)[1], _logdensity(ctx, dict(c, zs=zs), given=True)[1]
    assert all(_same_bits(a[k], b[k]) for k in a)


def test_any_subset_of_the_optional_outputs_has_the_bits_of_the_full_call(ctx):
    c = KC.case("r255")
    full = _propagate(ctx, c)[1]
    for want, layers in ((("F",), None), (("mean",), None), (("var",), None), (("F", "var"), (0,)), (("mean",), (1,)), ((), None)):
        rc, part, bufs, info = _propagate(ctx, c, want=want, layers_wanted=layers)
        assert rc == 0 and info == 0 and _guards_intact(bufs)
        for k in part:
            for l, a in enumerate(part[k]):
                if a is not None:
                    assert _same_bits(a, full[k][l]), (want, layers, k, l)


def test_a_failed_factorisation_in_the_middle_layer_writes_nothing(ctx):
    """The middle layer's kernel variance is negative: its Ku = K(Z, Z) + jitter I has a negative diagonal.  The layers below and above
    are fine; nothing may be written, not even the first layer's outputs."""
    c = KC.case("r800")
    rc, _, bufs, info = _propagate(ctx, c, variance_of={1: -1.0})
    assert rc == NOT_SPD and info > 0 and _untouched(bufs)
    rc, _, bufs, info2 = _logdensity(ctx, c, variance_of={1: -1.0})
    assert rc == NOT_SPD and info2 == info and _untouched(bufs)
    rc, _, bufs, info = _logdensity(ctx, c)
    assert rc == 0 and info == 0
    # through the model: CholeskyError
    from doubly_stochastic_dgp import _lib
    model = KC_model(c)
    with _jitter(-10.0):
        with pytest.raises(_lib.CholeskyError):
            model.compute_log_density(c["X"], c["Y"], zs=_zs3(c))
        with pytest.raises(_lib.CholeskyError):
            model.propagate_device(c["X"], c["S"])


def test_refusals_launch_nothing(ctx):
    c = KC.case("r255")
    d, keep = _desc(ctx, c)
    launches = ctx.lib.dsdgp_launch_count()
    need = C.c_int64()
    t = ctx.empty(64).fill_(CANARY)
    X, Y = ctx.to_device(c["X"]), ctx.to_device(c["Y"])
    L = len(c["layers"])
    null = (C.c_void_p * L)()
    # a scratch block that is too small
    rc = ctx.lib.dsdgp_stack_logdensity(ctx.handle, C.byref(d), _p(X), _p(Y), c["n"], c["S"], null, C.c_uint64(1), 1.0, _p(t), 512, _p(t), _p(t),
                                        None)
    assert rc == BAD_ARG and bool((t == CANARY).all())
    # shapes that do not chain
    d.layers[1].input_prop_dim = 1
    assert ctx.lib.dsdgp_stack_scratch_bytes(C.byref(d), c["n"], c["S"], 0, C.byref(need)) == BAD_ARG
    d.layers[1].input_prop_dim = 0
    d.lik_width = 2
    assert ctx.lib.dsdgp_stack_scratch_bytes(C.byref(d), c["n"], c["S"], 0, C.byref(need)) == BAD_ARG
    d.lik_width = 3
    # a layer wider than the Gram reverse pass takes: the forward plans, the reverse is unsupported
    wide = KC.case("r257")
    dw, keepw = _desc(ctx, wide)
    dw.layers[2].kern.input_dim = 40
    dw.layers[1].DO = 38
    assert ctx.lib.dsdgp_stack_scratch_bytes(C.byref(dw), wide["n"], 1, 0, C.byref(need)) == 0
    assert ctx.lib.dsdgp_stack_scratch_bytes(C.byref(dw), wide["n"], 1, 1, C.byref(need)) == UNSUPPORTED
    assert b"input_dim" in ctx.lib.dsdgp_last_error()
    rc = ctx.lib.dsdgp_stack_logdensity(ctx.handle, C.byref(dw), _p(X), _p(Y), wide["n"], 1, null, C.c_uint64(1), 1.0, _p(t), 1 << 40, _p(t),
                                        _p(t), None)
    assert rc == UNSUPPORTED and bool((t == CANARY).all())
    # more than 8 GB of scratch
    assert ctx.lib.dsdgp_stack_scratch_bytes(C.byref(d), 1 << 24, 64, 0, C.byref(need)) == UNSUPPORTED
    assert ctx.lib.dsdgp_launch_count() == launches


# ---------------------------------------------------------------------------------------------------------------- through the host mirror
_jitter, _zs3, KC_model = KC.jitter, KC.zs3, KC.model_of


@pytest.mark.parametrize("name", ("r255", "student"))
def test_the_model_gives_the_raw_calls_bits(ctx, name):
    c = KC.case(name)
    model = KC_model(c)
    with _jitter(c["jitter"]):
        raw = _logdensity(ctx, c, given=True)[1]
        value, pairs = model.compute_log_density_gradients(c["X"], c["Y"], zs=_zs3(c))
        assert _same_bits(value, raw["value"][0])
        assert _same_bits(model.compute_log_likelihood(c["X"], c["Y"], zs=_zs3(c)), raw["data"][0])
        assert abs(model.compute_log_prior() - raw["prior"][0]) <= 1e-13 * abs(raw["prior"][0])
        keys = {"Z": "Z", "q_mu": "q_mu", "variance": "variance", "lengthscales": "lengthscales", "white_variance": "diag"}
        plist = model.parameter_list()
        assert len(plist) == len(pairs)
        for (p, g), (p2, l, k) in zip(pairs, plist):
            assert p is p2 and g.shape == p.shape
            assert _same_bits(g.reshape(-1), (raw["lik"] if l is None else raw["l%d_%s" % (l, keys[k])]).reshape(-1)), (l, k)
        fw = _propagate(ctx, c, given=True)[1]
        Fs, Fmeans, Fvars = model.propagate(c["X"], S=c["S"], zs=_zs3(c))
        L = len(c["layers"])
        for l, y in enumerate(c["layers"]):
            S, n, p = c["S"], c["n"], y["p"]
            assert _same_bits(Fs[l].reshape(S * n, -1), fw["F"][l])
            assert _same_bits(Fmeans[l][:, :, p:].reshape(S * n, -1), fw["mean"][l])
            assert _same_bits(Fvars[l][:, :, p:].reshape(S * n, -1), np.repeat(fw["var"][l][:, None], y["DO"], 1))
            if p:
                assert _same_bits(Fmeans[l][:, :, :p], Fs[l][:, :, :p]) and np.all(Fvars[l][:, :, :p] == 0.0)


def test_one_layer_with_one_sample_is_the_layers_conditional_plus_the_read_out(ctx):
    """L = 1, S = 1: mean and var are SGPMC_Layer.conditional_device's bits, and the value and the adjoints are those of
    dsdgp_lik_elbo_readout on them: data = w sum of its block partials in ascending order, d_q_mu = conditional_vjp(-dmean, -dvar) - q_mu."""
    c = KC.case("r1")
    big = dict(c)
    rng = np.random.default_rng(5)
    n = 300
    big.update(n=n, X=rng.standard_normal((n, 2)), Y=rng.standard_normal((n, 1)), zs=[])
    for case in (c, big):
        model = KC_model(case)
        layer = model.layers[0]
        with _jitter(case["jitter"]):
            fw = _propagate(ctx, case)[1]
            mean, var = layer.conditional_device(case["X"])
            ctx.sync()
            assert _same_bits(mean.cpu().numpy(), fw["mean"][0]) and _same_bits(var.cpu().numpy(), fw["var"][0])
            ld = _logdensity(ctx, case)[1]
            w = case["data_scale"]
            nb = -(-case["n"] // 256)
            part, dm, dv = ctx.empty(2 * nb), ctx.empty(case["n"], 1), ctx.empty(case["n"], 1)
            Y = ctx.to_device(case["Y"])
            assert ctx.lib.dsdgp_lik_elbo_readout(ctx.handle, 0, case["lik"][1], 1.0, _p(mean), _p(var), _p(Y), case["n"], 1, 1, w, None, _p(part),
                                                  _p(dm), _p(dv), None, None, 0) == 0
            ctx.sync()
            ph = part.cpu().numpy()
            data = 0.0
            for b in range(nb):
                data += ph[2 * b]
            assert _same_bits(w * data, ld["data"][0])
            g = layer.conditional_vjp(-dm, -dv[:, 0], X=case["X"])
            assert _same_bits(g["q_mu"] - case["layers"][0]["q_mu"], ld["l0_q_mu"])
            assert _same_bits(g["Z"], ld["l0_Z"]) and _same_bits(g["variance"], ld["l0_variance"][0])

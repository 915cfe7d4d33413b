"""-m gpu: dsdgp_trsm / dsdgp_trsm_batched (csrc/trsm.hip) on the Cholesky factors of ill-conditioned Gram matrices, against a
longdouble substitution on the same float64 factor.  Cases, measures and bars: tests/trsm_reference.py (its CPU test holds scipy and a
float64 restatement of the kernel's algorithm to the same bars).

  rho_dev <= 8 max(rho_cpu(case), rho_table)      componentwise backward error, units of 2^-53
  fe_dev  <= 8 max(fe_cpu(case), 2^-52)           forward error against the longdouble solution
  the project's normwise residual <= 1e-13 n |L||X| as before

Every call hands the kernel NaN above the diagonal of L (the header promises that only the lower triangle is read) and checks that L
comes back untouched.  Groups: shape edges (n across the 16-row block and the 128-row panel, nrhs across a wave's 16 and a workgroup's
64 columns) and every family; the left-looking form at its smallest, with a twin that must take the right-looking form; odd leading
dimensions with canaries in the gaps; batched solves with one shared and with three different factors; exactness properties.
Set DSDGP_TRSM_PROFILE=<file> to get every measured figure as one table (profiles/trsm_direct.md).

Measured on an MI355X: rho dev / rho cpu at most 2.14 (edge-pairs-n257-r65, trans = 1), fe dev / max(fe cpu, 2^-52) at most 6.1
(edge-grid1d-n129-r64, trans = 1); 132 solves in 7 s.  Against the kernel without its refinement step the columns-of-L cases fail
(rho 3076, fe 6.8e-12 against a bar of 1.0e-12) and the 15- to 17-point grids stand at rho 81 .. 128: profiles/trsm_refinement_ab.md."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import trsm_reference as T

pytestmark = pytest.mark.gpu

CANARY = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload: read, it poisons; written, it shows


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def path(n, nrhs, ldl, ldb, batch=1):
    """the form dsdgp_trsm_batched takes (the condition at its head; device allocations are 256-byte aligned)"""
    left = batch == 1 and n >= 256 and nrhs >= 2048 and nrhs % 8 == 0 and ldl % 2 == 0 and ldb % 2 == 0 and n % 2 == 0
    return "left" if left else "right"


def l_buffer(L, ldl):
    """n x ldl: the lower triangle of L, NaN everywhere else"""
    n = L.shape[0]
    buf = np.full((n, ldl), np.nan)
    il = np.tril_indices(n)
    buf[il] = L[il]
    return buf


def solve(ctx, L, B, trans, ldl=None, ldb=None):
    """one dsdgp_trsm call on padded buffers; asserts that L and the gaps of B come back bit for bit.  -> X (n x nrhs)"""
    from doubly_stochastic_dgp import _lib
    n, nrhs = B.shape
    ldl, ldb = ldl or n, ldb or nrhs
    Lbuf = l_buffer(L, ldl)
    Bbuf = np.full((n, ldb), CANARY)
    Bbuf[:, :nrhs] = B
    dL, dB = ctx.to_device(Lbuf), ctx.to_device(Bbuf)
    ctx.torch.cuda.current_stream().synchronize()
    _lib.check(ctx.lib.dsdgp_trsm(ctx.handle, trans, n, nrhs, _p(dL), ldl, _p(dB), ldb))
    ctx.sync()
    got = dB.cpu().numpy()
    assert np.array_equal(_bits(dL.cpu().numpy()), _bits(Lbuf)), "L was written"
    assert np.array_equal(_bits(got[:, nrhs:]), _bits(Bbuf[:, nrhs:])), "the gap of B was written"
    return np.ascontiguousarray(got[:, :nrhs])


# ------------------------------------------------------------------------------------------------ the profile table
_ROWS = []


@pytest.fixture(scope="module", autouse=True)
def profile_table():
    yield
    out = os.environ.get("DSDGP_TRSM_PROFILE")
    if not out or not _ROWS:
        return
    hdr = ["case", "trans", "path", "cond(L)", "rho dev", "rho cpu", "fe dev", "fe cpu", "normwise dev", "normwise cpu"]
    with open(out, "w") as f:
        f.write("# dsdgp_trsm on Cholesky factors of ill-conditioned Gram matrices (tests/test_gpu_trsm_direct.py)\n\n"
                "rho: componentwise backward error max |op(L) X - B| / (|op(L)||X|) in units of 2^-53; fe: max|X - X_true| / max|X_true| against the\n"
                "longdouble substitution; normwise: |op(L) X - B|_F / (n |L|_F |X|_F).  `cpu` = scipy.linalg.solve_triangular.  Bars: rho dev <= 8 max(rho cpu,\n"
                f"rho_table), rho_table = {T.rho_table():.3g} (the largest rho cpu of the table); fe dev <= 8 max(fe cpu, 2^-52); normwise <= 1e-13.\n"
                "`left` / `twin` rows: the longdouble figures are taken on 64 sampled columns.  `lrows` rows (B = L^T[:, :20]) are held to rho alone.\n\n")
        f.write("| " + " | ".join(hdr) + " |\n|" + "---|" * len(hdr) + "\n")
        for r in _ROWS:
            f.write("| " + " | ".join(r) + " |\n")
        wr, wf = max(_RATIOS), max((r[1], r[2]) for r in _RATIOS if r[3])
        f.write(f"\n{len(_ROWS)} rows.  Largest rho dev / rho cpu: {wr[0]:.3g} ({wr[2]}); largest fe dev / max(fe cpu, 2^-52): {wf[0]:.3g} ({wf[1]}).\n")


_RATIOS = []


def record(row, form):
    _ROWS.append([row["case"], str(row["trans"]), form, f"{row['cond']:.3g}", f"{row['rho']:.3g}", f"{row['rho_cpu']:.3g}", f"{row['fe']:.3g}",
                  f"{row['fe_cpu']:.3g}", f"{row['norm']:.3g}", f"{row['norm_cpu']:.3g}"])
    _RATIOS.append((row["rho"] / max(row["rho_cpu"], 1e-300), row["fe"] / max(row["fe_cpu"], 2.0 ** -52), f"{row['case']} trans={row['trans']}",
                    T.BY_NAME[row["case"]].fe_held))


def run_case(ctx, case, trans, ldl=None, ldb=None):
    """solve, record the row (before any assertion), assert the bars.  -> X"""
    ref = T.cpu_reference(case, trans)
    X = solve(ctx, case.L(), ref["B"], trans, ldl, ldb)
    form = path(case.n, case.nrhs, ldl or case.n, ldb or case.nrhs)
    T.check(case, trans, X, record=lambda row: record(row, form))
    return X


def _group(*names):
    return [c.name for c in T.CASES if c.group in names]


# ------------------------------------------------------------------------------------------------ shapes and families
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("name", _group("edge", "family"))
def test_shape_edges_and_families(ctx, name, trans):
    case = T.BY_NAME[name]
    assert path(case.n, case.nrhs, case.n, case.nrhs) == "right"
    run_case(ctx, case, trans)


# ------------------------------------------------------------------------------------------------ the left-looking form
_LEFT = {}


def _left(ctx, case, trans):
    if (case.name, trans) not in _LEFT:
        assert path(case.n, case.nrhs, case.n, case.nrhs) == "left"
        X = run_case(ctx, case, trans)
        _LEFT[(case.name, trans)] = X
        ref = T.cpu_reference(case, trans)
        rho64 = T.float64_rho(case.L(), X, ref["B"], trans)            # every column
        bar = T.bars(case, trans)[0] + T.float64_slack(case.n)
        print("  all %d columns, float64 product: rho %.3g (bar %.3g)" % (case.nrhs, rho64, bar))
        assert rho64 <= bar
    return _LEFT[(case.name, trans)]


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("name", _group("left"))
def test_left_looking_form(ctx, name, trans):
    """pgemm_accum over the rows solved so far and, for trans, the transposed copy LT, at shapes where the panel borders at 128, 256 and
    384 split the near-duplicate twins (n / 2 apart) and the last panel has 2 rows"""
    _left(ctx, T.BY_NAME[name], trans)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("name", _group("twin"))
def test_twin_takes_the_right_looking_form_and_agrees(ctx, name, trans):
    """nrhs = 2052 is no multiple of 8: the same factor and the same first 2052 columns through the right-looking form.  The two results
    agree, on all shared columns, within the forward bar (here with the truth and scipy's error taken on all 2052 columns)."""
    twin = T.BY_NAME[name]
    left = T.BY_NAME[name.replace("twin", "left").replace("r2052", "r2056")]
    assert path(twin.n, twin.nrhs, twin.n, twin.nrhs) == "right"
    Xr = run_case(ctx, twin, trans)
    Xl = _left(ctx, left, trans)[:, :twin.nrhs]
    ref = T.cpu_reference(twin, trans)
    X_true = T.solve_truth(twin.L(), ref["B"], trans)
    unit = float(np.max(np.abs(X_true)))
    fe_cpu = float(np.max(np.abs(ref["X_cpu"] - X_true))) / unit
    diff = float(np.max(np.abs(Xr - Xl))) / unit
    bar = T.DEVICE_FACTOR * max(fe_cpu, 2.0 ** -52)
    print("%s trans=%d: right- against left-looking on %d columns: %.3g (scipy's forward error %.3g, bar %.3g)" % (name, trans, twin.nrhs, diff, fe_cpu, bar))
    assert diff <= bar


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("name", _group("layout"))
def test_odd_leading_dimensions_and_gaps(ctx, name, trans):
    """ldl = n + 3, ldb = nrhs + 1 (both odd: no 16-byte alignment of any row but the first); NaN above the diagonal and in the pad of L,
    a canary in the pad column of B that must survive bit for bit (solve() asserts both)"""
    case = T.BY_NAME[name]
    run_case(ctx, case, trans, ldl=case.n + 3, ldb=case.nrhs + 1)


# ------------------------------------------------------------------------------------------------ batched
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("group", ["shared", "batched"])
def test_batched(ctx, group, trans):
    """batch = 3, n = 130, nrhs = 17: one L for all (strideL = 0, the Lu_tiled use) or three different factors (strideL = n ldl); the B
    matrices sit strideB = n ldb + 5 apart with canaries between them.  Every entry is held to the bars of its own single solve."""
    from doubly_stochastic_dgp import _lib
    cases = [c for c in T.CASES if c.group == group]
    n, nrhs, batch = 130, 17, 3
    assert len(cases) == batch and all(c.n == n and c.nrhs == nrhs for c in cases)
    shared = group == "shared"
    assert not shared or all(c.L() is cases[0].L() for c in cases)
    ldl, ldb, gap = n + 1, nrhs, 5
    strideB = n * ldb + gap
    Lbuf = np.stack([l_buffer(c.L(), ldl) for c in (cases[:1] if shared else cases)])
    Bbuf = np.full(batch * strideB, CANARY)
    for b, c in enumerate(cases):
        Bbuf[b * strideB:b * strideB + n * ldb] = T.cpu_reference(c, trans)["B"].ravel()
    dL, dB = ctx.to_device(Lbuf), ctx.to_device(Bbuf)
    ctx.torch.cuda.current_stream().synchronize()
    _lib.check(ctx.lib.dsdgp_trsm_batched(ctx.handle, trans, n, nrhs, batch, _p(dL), ldl, 0 if shared else n * ldl, _p(dB), ldb, strideB))
    ctx.sync()
    got = dB.cpu().numpy()
    assert np.array_equal(_bits(dL.cpu().numpy()), _bits(Lbuf))
    failures = []
    for b, c in enumerate(cases):
        assert np.array_equal(_bits(got[b * strideB + n * ldb:(b + 1) * strideB]), _bits(np.full(gap, CANARY))), "the gap behind B_%d was written" % b
        X = got[b * strideB:b * strideB + n * ldb].reshape(n, ldb)
        try:
            T.check(c, trans, X, record=lambda row: record(row, "right, batch of 3" + (", one L" if shared else "")))
        except AssertionError as e:          # measure every entry before failing
            failures.append(e)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("family", ["pairs", "subset1d"])
def test_power_of_two_column_scaling_is_exact(ctx, family, trans):
    """columns of B scaled by 2^-30 .. 2^30 give the same columns of X scaled by the same powers, bit for bit: no column's arithmetic sees
    another column.  And a second call gives the bits of the first."""
    plain, scaled = T.BY_NAME[f"exact-{family}-n129-r61"], T.BY_NAME[f"exact-{family}-n129-r61-pow2"]
    s = T.pow2_scales(61)
    assert s[0] == 2.0 ** -30 and s[-1] == 2.0 ** 30 and len(set(s)) == 61
    assert np.array_equal(scaled.B(trans), plain.B(trans) * s[None, :])
    X1 = run_case(ctx, plain, trans)
    Xs = run_case(ctx, scaled, trans)
    assert np.array_equal(_bits(Xs), _bits(X1 * s[None, :]))
    X2 = solve(ctx, plain.L(), plain.B(trans), trans)
    assert np.array_equal(_bits(X2), _bits(X1))


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("family", ["pairs", "subset1d"])
def test_a_zero_column_stays_zero(ctx, family, trans):
    case = T.BY_NAME[f"exact-{family}-n129-r20-zerocol"]
    X = run_case(ctx, case, trans)
    assert np.all(case.B(trans)[:, 1] == 0.0) and np.all(X[:, 1] == 0.0)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("family", ["pairs", "subset1d"])
def test_columns_of_L_give_the_identity(ctx, family, trans):
    """B = L[:, :20]: at trans = 0, X = [I_20; 0] within the forward bar, the rows below 20 included, in units of max|X_true| = 1; at
    trans = 1 it is one more right-hand side under both bars.  The transposed twin B = L^T[:, :20] (X = [I; 0] at trans = 1) is held to
    rho and its forward error recorded: tests/trsm_reference.py::Case says why substitution's exact [I; 0] is no bar for a blocked solve."""
    case = T.BY_NAME[f"exact-{family}-n150-r20-lcols"]
    ref = T.cpu_reference(case, trans)
    if trans == 0:
        assert float(np.max(np.abs(ref["X_true"] - np.eye(150, 20)))) <= 2.0 ** -40
    run_case(ctx, case, trans)
    if trans == 1:
        twin = T.BY_NAME[f"exact-{family}-n150-r20-lrows"]
        assert float(np.max(np.abs(T.cpu_reference(twin, 1)["X_true"] - np.eye(150, 20)))) <= 2.0 ** -40
        run_case(ctx, twin, 1)

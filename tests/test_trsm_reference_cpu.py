"""-m "not gpu": the yardstick of tests/test_gpu_trsm_direct.py held to its own bars (tests/trsm_reference.py).

scipy's solve must be a backward-stable substitution on every case of the table; rho_table — the one number every device bar may fall
back to — is computed here and printed; and blocked_emulation, the float64 restatement of the device kernel's algorithm (explicit
16 x 16 diagonal inverses applied as block products), must meet both device bars on every case: no bar asks for more than the design
can give.  Run with -s to read the figures."""
import numpy as np
import pytest

from tests import trsm_reference as T


def test_the_table_covers_what_it_promises():
    groups = {}
    for c in T.CASES:
        groups.setdefault(c.group, []).append(c)
    edges = groups["edge"]
    assert {c.n for c in edges} == set(T.N_EDGES) and {c.nrhs for c in edges} == set(T.NRHS_EDGES)
    for fam in ("pairs", "grid1d"):
        for n in T.N_EDGES:
            assert len([c for c in edges if c.family == fam and c.n == n]) == 2
        for r in T.NRHS_EDGES:
            assert len([c for c in edges if c.family == fam and c.nrhs == r]) >= 2
    assert {(c.family, c.jitter) for c in groups["family"]} == {(f, 1e-6) for f in T.FAMILIES} | {("pairs", 1e-9)}
    assert {(c.n, c.nrhs) for c in groups["left"]} == {(256, 2048), (386, 2056)} and {(c.n, c.nrhs) for c in groups["twin"]} == {(386, 2052)}
    for c in groups["left"] + groups["twin"]:
        cols = c.columns()
        assert len(cols) == 64 and len(set(cols)) == 64 and cols.max() < 2052
    Z, _ = T.family_case("dups", 130)
    assert np.array_equal(Z[65:], Z[:65])
    Z, _ = T.family_case("subset1d", 130)
    assert Z.shape == (130, 1) and np.all(np.diff(Z[:, 0]) > 0)


def test_the_factors_are_ill_conditioned():
    """the point of the table: cond(Ku) = cond(L)^2 up to 1e8 and beyond, diagonal blocks whose explicit inverse is itself badly scaled"""
    worst_block = 0.0
    for fam, n, jit in [("pairs", 330, 1e-6), ("grid1d", 330, 1e-6), ("subset1d", 386, 1e-6), ("dups", 200, 1e-6), ("pairs", 200, 1e-9)]:
        L, cond = T.factor(fam, n, jit)
        blocks = [L[i:i + 16, i:i + 16] for i in range(0, n, 16)]
        kb = max(float(np.max(np.abs(np.linalg.inv(D)) @ np.abs(D))) for D in blocks)
        worst_block = max(worst_block, kb)
        print("%s n=%d jitter %g: cond(L) %.3g, cond(Ku) ~ %.3g, largest | |D^-1||D| | over the 16 x 16 diagonal blocks %.3g" % (fam, n, jit, cond, cond * cond, kb))
        assert cond * cond >= 1e6
    assert worst_block >= 1e3


@pytest.mark.parametrize("trans", [0, 1])
def test_reference_and_blocked_emulation_meet_every_device_bar(trans):
    table = T.rho_table()
    print("rho_table = %.3g units of 2^-53 (the largest componentwise backward error of scipy's solve over %d cases x 2)" % (table, len(T.CASES)))
    assert table >= 0.5
    worst_rho, worst_fe = (0.0, None), (0.0, None)
    for c in T.CASES:
        ref = T.cpu_reference(c, trans)
        assert ref["rho"] <= min(table, c.n + 1.0) and ref["norm"] <= 1e-13          # substitution's bound is gamma_n: at most n + 1 units
        X = T.blocked_emulation(c.L(), ref["B"], trans)
        row = T.check(c, trans, X, what="blocked emulation")
        r1 = row["rho"] / max(row["rho_cpu"], 1e-300)
        r2 = row["fe"] / max(row["fe_cpu"], 2.0 ** -52)
        worst_rho, worst_fe = max(worst_rho, (r1, c.name)), max(worst_fe, (r2, c.name))
        if c.sample is not None:         # the float64 residual the device test takes on all columns
            assert T.float64_rho(c.L(), X, ref["B"], trans) <= row["rho_bar"] + T.float64_slack(c.n)
    print("trans=%d: largest emulation / scipy ratio: rho %.3g on %s, fe %.3g on %s" % ((trans,) + worst_rho + worst_fe))


def test_without_the_refinement_step_the_design_misses_the_bars():
    """what the bars found: explicit diagonal inverses alone (refine = 0, the kernel before this table existed) leave a componentwise
    residual of |D^-1||D| roundings.  On the factor of a 15-point 1-D grid, trans = 1, that is 182 units of 2^-53 in float64 numpy and was
    85 .. 128 on an MI355X, against 1.3 for substitution and a bar of 8 rho_table; one refinement step per block brings it to 1."""
    c = T.BY_NAME["edge-grid1d-n15-r15"]
    ref = T.cpu_reference(c, 1)
    before = T.measures(c.L(), T.blocked_emulation(c.L(), ref["B"], 1, refine=0), ref["B"], 1, ref["X_true"])["rho"]
    after = T.measures(c.L(), T.blocked_emulation(c.L(), ref["B"], 1, refine=1), ref["B"], 1, ref["X_true"])["rho"]
    print("rho without / with the refinement step: %.3g / %.3g (scipy %.3g, bar %.3g)" % (before, after, ref["rho"], T.bars(c, 1)[0]))
    assert before > T.bars(c, 1)[0] >= 8.0 * after


@pytest.mark.parametrize("trans", [0, 1])
def test_truth_is_a_truth(trans):
    """the longdouble substitution leaves a residual at its own rounding level, 2^-11 of a float64 unit"""
    c = T.BY_NAME["edge-pairs-n330-r17"]
    ref = T.cpu_reference(c, trans)
    L = np.asarray(c.L(), dtype=T.LD)
    Lo = L.T if trans else L
    res = np.abs(Lo @ ref["X_true"] - ref["B"]) / (np.abs(Lo) @ np.abs(ref["X_true"]))
    assert float(np.max(res)) / T.U <= 2.0 ** -6


def test_exactness_cases_hold_for_the_reference_order():
    """the properties the device test asserts bit for bit are properties of any fixed-order solve in binary arithmetic"""
    for fam in ("pairs", "subset1d"):
        a, b = T.BY_NAME[f"exact-{fam}-n129-r61-pow2"], T.BY_NAME[f"exact-{fam}-n129-r61"]
        for trans in (0, 1):
            s = T.pow2_scales(61)
            assert np.array_equal(a.B(trans), b.B(trans) * s[None, :])
            Xa, Xb = T.blocked_emulation(a.L(), a.B(trans), trans), T.blocked_emulation(b.L(), b.B(trans), trans)
            assert np.array_equal(Xa[:, :1], Xb[:, :1] * s[0])          # BLAS may block columns differently: one column at a time
            z = T.BY_NAME[f"exact-{fam}-n129-r20-zerocol"]
            assert np.all(T.blocked_emulation(z.L(), z.B(trans), trans)[:, 1] == 0.0)
            e = T.BY_NAME[f"exact-{fam}-n150-r20-" + ("lrows" if trans else "lcols")]
            Xt = T.cpu_reference(e, trans)["X_true"]
            assert float(np.max(np.abs(Xt - np.eye(150, 20)))) <= 2.0 ** -40

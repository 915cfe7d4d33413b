"""tests/model_reuse_plan.py without a GPU: the call sequences of tests/test_gpu_model_reuse.py contain the transitions they are there
for and stay within their extents, the schedule switches claimed in the tables follow from the mirrored selection rules, the two data
pools differ, and the bit comparison tells apart what a tolerance would let through."""
import numpy as np
import pytest

from tests import model_reuse_plan as plan

SHAPED = ("G", "V", "P", "Q", "E", "Gd")


@pytest.mark.parametrize("name", list(plan.CONFIGS))
def test_sequence_contains_the_required_transitions(name):
    cfg = plan.CONFIGS[name]
    seq = cfg.seq
    n_max, s_max = cfg.extents
    assert 10 <= len(seq) <= 16
    for kind, n, S in seq:
        assert kind in SHAPED + ("C", "Cw")
        if kind in SHAPED:
            assert 1 <= n <= n_max and 1 <= S <= s_max, (kind, n, S)
        elif kind == "C":
            assert 1 <= n <= n_max and S == 1                # Engine.layer_conditional keeps the model for these
        else:
            assert n > n_max * s_max
    assert seq[0] == ("G", n_max, s_max) and seq[-1] == ("G", n_max, s_max)
    shaped = [(c[1], c[2]) for c in seq if c[0] in SHAPED]
    assert set(cfg.shapes) <= set(shaped)                                     # every shape of the configuration is visited ...
    assert set(cfg.shapes) <= {(c[1], c[2]) for c in seq if c[0] == "G"}      # ... by a full gradient call
    pairs = list(zip(seq[:-1], seq[1:]))
    both = [(a, b) for a, b in pairs if a[0] in SHAPED and b[0] in SHAPED]
    assert any(b[1] * b[2] < a[1] * a[2] for a, b in both)                    # a shrink
    assert any(b[1] > a[1] for a, b in both[1:])                              # a growth back
    assert any(a[1] == b[1] and a[2] != b[2] for a, b in both)                # a change of S alone
    assert any(a[0] == "Q" and b[0] == "G" and a[1:] != b[1:] for a, b in pairs)
    assert any(a[0] in ("V", "P") and b[0] == "G" and a[1:] == b[1:] for a, b in pairs)
    kinds = [c[0] for c in seq]
    assert kinds.count("Gd") >= 1 and kinds.count("E") >= 1 and kinds.count("C") + kinds.count("Cw") >= 1
    assert ("Cw" in kinds) == (name == "D")
    if name in "ABC":
        kind, n, S = seq[cfg.anchor]
        assert kind == "G" and n <= 100 and S <= 3 and plan.pool_of(cfg.anchor) == "a"
        later = [c for c in seq[cfg.anchor + 1:] if c[0] == "G" and c[1] <= 100 and c[2] <= 3]
        assert not later                                                      # the LAST small gradient call of the used model
    else:
        assert cfg.anchor is None


def test_schedule_switches_of_the_tables():
    a = plan.CONFIGS["A"]
    Mp = plan.padded_M(a.M)
    assert Mp == 128
    want = {(1000, 13): (813, 4, 4, 1, True), (330, 8): (165, 4, 8, 3, True), (100, 8): (50, 8, 8, 4, False),
            (100, 3): (19, 8, 8, 4, False), (37, 1): (3, 8, 8, 4, False), (1, 1): (1, 8, 8, 4, False)}
    for (n, S), row in want.items():
        nb = plan.row_blocks(n, S)
        got = (nb, plan.chain_waves(Mp, nb, False), plan.chain_waves(Mp, nb, True), plan.chain_d_split(nb, 8), plan.two_streams(n, S, Mp))
        assert got == row, ((n, S), got)
    assert 37 % 16 == 5
    # B / C / D: padded orders, weight-gradient tile rows and one stream throughout
    assert [plan.padded_M(m) for m in (100, 40, 300, 32)] == [112, 48, 320, 32]
    for cfg in (plan.CONFIGS["B"], plan.CONFIGS["C"], plan.CONFIGS["D"], plan.CONFIGS["F"]):
        for kind, n, S in cfg.seq:
            if kind in SHAPED:
                assert not plan.two_streams(n, S, plan.padded_M(cfg.M))
    b = plan.CONFIGS["B"]
    for n, S in b.shapes:
        nb = plan.row_blocks(n, S)
        assert [plan.chain_d_split(nb, d) for d in (3, 3, 2)] == [3, 3, 2]
        assert plan.chain_waves(112, nb, True) == 4
    pads = {s: -(s[0] * s[1]) % 16 for s in b.shapes + [(17, 4)]}
    assert pads == {(300, 4): 0, (96, 3): 0, (40, 3): 8, (37, 1): 11, (17, 2): 14, (1, 1): 15, (17, 4): 12}
    e = plan.CONFIGS["E"]
    assert plan.padded_M(e.M) == 320
    want = {(600, 8): (300, 1), (330, 8): (165, 3), (330, 4): (83, 4), (200, 4): (50, 4), (37, 1): (3, 4)}
    for (n, S), row in want.items():
        nb = plan.row_blocks(n, S)
        assert (nb, plan.chain_d_split(nb, 6)) == row
        assert plan.chain_waves(320, nb, False) == plan.chain_waves(320, nb, True) == 8


@pytest.mark.parametrize("name", list(plan.CONFIGS))
def test_pools_differ_and_no_two_calls_share_inputs(name):
    cfg = plan.CONFIGS[name]
    K = cfg.DY if name == "F" else None
    pools = {w: plan.make_pool(cfg, w, num_classes=K) for w in "ab"}
    a, b = pools["a"], pools["b"]
    assert a["X"].shape == b["X"].shape == (cfg.pool_rows, cfg.widths[0])
    for k in ("X", "Y"):
        assert np.all(np.isfinite(a[k])) and np.all(np.isfinite(b[k]))
        assert not np.array_equal(a[k], b[k])
    assert not np.any(a["X"] == b["X"])
    assert [z.shape for z in a["zs"]] == [(cfg.extents[1], cfg.pool_rows, d) for d in cfg.widths[1:] + [cfg.DY]]
    assert all(not np.any(za == zb) for za, zb in zip(a["zs"], b["zs"]))
    if K is None:
        assert np.std(b["Y"]) > 100 * np.std(a["Y"])
    assert np.std(b["X"]) > 1.5 * np.std(a["X"])
    seen = []
    for i, (kind, n, S) in enumerate(cfg.seq):
        if kind in ("C", "Cw"):
            Xs = plan.conditional_inputs(pools, i, n)
            assert [x.shape for x in Xs] == [(n, d) for d in cfg.widths]
            X = Xs[0]
        else:
            X, Y, zs = plan.call_inputs(pools, i, n, S)
            assert X.shape == (n, cfg.widths[0]) and Y.shape[0] == n
            assert [z.shape for z in zs] == [(S, n, d) for d in cfg.widths[1:] + [cfg.DY]]
        assert all(not np.array_equal(X[0], x0) for x0 in seen)
        seen.append(X[0].copy())
    # neighbours come from different pools
    assert all(plan.pool_of(i) != plan.pool_of(i + 1) for i in range(len(cfg.seq) - 1))


def test_p2_plan_stays_within_the_extents():
    for name, case in plan.P2_CASES.items():
        cfg = plan.CONFIGS[name]
        n_max, s_max = cfg.extents
        n, S = case["step"]
        assert n <= n_max and S <= s_max
        assert max(plan.P2_MINIBATCH_STEPS) * n + n <= n_max and len(plan.P2_MINIBATCH_STEPS) == 2
        assert len(case["between"]) == plan.P2_STEPS - 1
        calls = [c for group in case["between"] for c in group]
        assert sorted(c[0] for c in calls) == sorted(["P", "V", "G", "Q", "E", "C"])
        for kind, nn, SS in calls:
            assert nn <= n_max and SS <= s_max
            assert kind == "C" or (nn, SS) != (n, S)                          # the OTHER shapes of the configuration
        last = max(plan.ROW_STEP * 2 * (k + j) + c[1] for k, group in enumerate(case["between"]) for j, c in enumerate(group))
        assert max(last, plan.ROW_STEP * (2 * plan.P2_STEPS - 1) + n) <= cfg.pool_rows


def test_bit_comparison():
    x = np.array([1.0, -2.5, 0.0, np.nan, np.inf])
    assert plan.bits_diff(x, x.copy()) is None
    one_ulp = x.copy()
    one_ulp[1] = np.nextafter(one_ulp[1], 0.0)
    assert np.allclose(one_ulp, x, rtol=1e-15, atol=0.0, equal_nan=True)
    msg = plan.bits_diff(one_ulp, x)
    assert msg is not None and "1 of 5" in msg and "(1,)" in msg
    neg_zero = x.copy()
    neg_zero[2] = -0.0
    assert np.array_equal(neg_zero[:3], x[:3])                               # ... which is why array_equal is not used
    assert plan.bits_diff(neg_zero, x) is not None
    # NaN against the same NaN is equal, against a NaN of another payload it is not
    other_nan = x.copy()
    other_nan.view(np.uint64)[3] ^= 1
    assert np.isnan(other_nan[3]) and plan.bits_diff(other_nan, x) is not None
    assert plan.bits_diff(np.float64(np.nan), np.float64(np.nan)) is None
    assert plan.bits_diff(np.zeros((2, 3)), np.zeros((3, 2))) is not None     # shapes count
    assert plan.bits_diff(np.zeros(0), np.zeros(0)) is None
    with pytest.raises(AssertionError, match="grad"):
        plan.assert_same_bits({"elbo": x, "grad": one_ulp}, {"elbo": x, "grad": x}, "case")
    with pytest.raises(AssertionError):
        plan.assert_same_bits({"elbo": x}, {"elbo": x, "grad": x}, "case")
    plan.assert_same_bits({"elbo": x, "grad": x}, {"elbo": x.copy(), "grad": x.copy()}, "case")

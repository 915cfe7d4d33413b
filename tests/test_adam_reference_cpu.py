"""The long-double Adam reference, its bounds and the cases of tests/test_gpu_adam_direct.py, checked without a device: the reference
against the oracle's step, plain float64 within HALF the asserted bars on the generator's inputs, the mask-class census of the small
layouts, and which slots and passes of the sweep each layout reaches."""
import numpy as np
import pytest

from oracle import dgp_oracle as O
from tests import adam_cases as AC
from tests import adam_reference as R

SETS = list(AC.PARAM_SETS)


def _all_live_inputs(n, seed, b1):
    mask = np.ones(n, dtype=np.int8)
    return R.make_inputs(mask, seed, b1) + (mask != 0,)


@pytest.mark.parametrize("pset", SETS)
def test_reference_agrees_with_the_oracle_step(pset):
    h = AC.PARAM_SETS[pset]
    th, g, m, v, zero, on = _all_live_inputs(20_000, 11, h["b1"])
    on = on & (np.arange(on.size) % 7 != 3)                       # some entries off: they must come back as they went in
    ref = R.adam_ld(th, g, m, v, on, h["lr"], h["b1"], h["b2"], h["eps"], h["t"])
    th_o, m_o, v_o = th.copy(), m.copy(), v.copy()
    O.adam_step(th_o, g, m_o, v_o, h["t"], lr=h["lr"], b1=h["b1"], b2=h["b2"], eps=h["eps"])
    for key, got, start in (("theta", th_o, th), ("m", m_o, m), ("v", v_o, v)):
        r = R.ratios(got, ref[key], ref["B_" + key], on)
        assert float(r.max()) <= R.BAR, (key, float(r.max()), int(np.argmax(r)))
        assert np.array_equal(ref[key][~on].astype(np.float64), start[~on]) and np.all(ref["B_" + key][~on] == 0)


@pytest.mark.parametrize("pset", SETS)
def test_float64_stays_within_half_the_asserted_bars(pset):
    h = AC.PARAM_SETS[pset]
    th, g, m, v, zero, on = _all_live_inputs(200_000, 12, h["b1"])
    assert np.all(np.abs(g[g != 0]) >= 1e-12) and np.all(g * g <= 1e12) and np.all((v == 0) | (v >= 1e-24))     # no subnormals, no overflow
    ref = R.adam_ld(th, g, m, v, on, h["lr"], h["b1"], h["b2"], h["eps"], h["t"])
    got = dict(zip(("theta", "m", "v"), R.adam_f64(th, g, m, v, on, h["lr"], h["b1"], h["b2"], h["eps"], h["t"])))
    for key in ("theta", "m", "v"):
        r = R.ratios(got[key], ref[key], ref["B_" + key], on)
        print("%s %-5s float64 / B = %.3f" % (pset, key, float(r.max())))
        assert float(r.max()) <= R.BAR / 2, (key, float(r.max()), int(np.argmax(r)))
    # the cancelling tenth is there and does cancel; the zero tenth comes back bit-equal, moments +0
    if h["b1"] != 0.0:
        small = np.abs(ref["m"].astype(np.float64)) <= 1e-8 * np.abs((1.0 - h["b1"]) * g)
        assert 0.09 * on.size <= np.count_nonzero(small & ~zero) <= 0.11 * on.size
    assert 0.09 * on.size <= np.count_nonzero(zero) <= 0.11 * on.size
    assert np.array_equal(got["theta"][zero], th[zero])
    for key in ("m", "v"):
        assert np.all(got[key][zero] == 0.0) and not np.any(np.signbit(got[key][zero]))


def test_poison_on_dead_entries():
    mask = np.array([1, 0, 2, 0, 0, 1, 1, 0] * 50, dtype=np.int8)
    th, g, m, v, zero = R.make_inputs(mask, 3, 0.9)
    dead = mask == 0
    for a in (g, m, v, th):
        assert np.all(np.isfinite(a)) and np.all(a[dead] != 0.0) and np.unique(a[dead]).size == np.count_nonzero(dead)
    assert not np.any(zero & dead)


def test_pair_census():
    """over the small layouts: all nine (even, odd) mask-class pairs, odd and even n_theta, a class-2 and a class-0 last entry — and
    over the layouts that take the fused tail alone as well (there classes 1 and 2 have different writers)"""
    for names in (list(AC.SMALL), [k for k, c in AC.SMALL.items() if not c["white"]]):
        pairs, parities, last = set(), set(), set()
        for name in names:
            model = AC.build_small(name)[0]
            entries, n = R.host_entries(model)
            mask = R.mask_from_model(model, entries)
            assert mask.size == n
            p, odd, la = R.pair_census(mask)
            print(name, n, sorted(p), "odd" if odd else "even", "last", la)
            pairs |= p
            parities.add(odd)
            last.add(la)
        assert pairs == {(a, b) for a in range(3) for b in range(3)}, sorted(pairs)
        assert parities == {True, False}
        assert {0, 2} <= last
    assert any(c["white"] for c in AC.SMALL.values()) and sum(bool(c["frozen"]) for c in AC.SMALL.values()) >= 2


def test_mask_classes_of_one_layout_by_hand():
    """m6_frozen_c, entry by entry: Z 12, q_mu 12, q_sqrt 2 x 6 x 6 | variance, lengthscale (frozen), white variance | Z 12, q_mu 6,
    q_sqrt 1 x 6 x 6 (frozen) | variance, lengthscale | likelihood variance (frozen)"""
    model = AC.build_small("m6_frozen_c")[0]
    entries, n = R.host_entries(model)
    mask = R.mask_from_model(model, entries)
    tri = np.tril(np.ones((6, 6), dtype=np.int8)).ravel()
    want = np.concatenate([np.ones(24, np.int8), tri, tri, [2, 0, 2], np.ones(18, np.int8), np.zeros(36, np.int8), [2, 2], [0]])
    assert n == 156 and np.array_equal(mask, want)


def test_slots_and_passes_each_layout_reaches():
    # copied from csrc/model_schedule.hpp:870 (dsdgp_model_adam_step) and :616 (end_rows_tail): min(2048, ceil_div(n, 512)) workgroups
    # of 256; csrc/model_kernels.hpp:1073: four pairs per thread and pass
    wg_max, per_wg, wg, slots = 2048, 512, 256, 4
    assert (AC.WG_MAX, AC.ENTRIES_PER_WG, AC.WG_THREADS, AC.SLOTS) == (wg_max, per_wg, wg, slots)
    one_slot_limit = wg_max * per_wg                    # 2^20 entries: up to here a thread per pair
    one_pass_limit = slots * wg_max * wg * 2            # 2^22 entries: up to here one pass
    assert (one_slot_limit, one_pass_limit) == (1 << 20, 1 << 22)
    for name in AC.SMALL:
        n = R.host_entries(AC.build_small(name)[0])[1]
        u, p = AC.slot_and_pass(np.arange(n), n)
        assert n <= one_slot_limit and set(np.unique(u)) <= {0, -1} and set(np.unique(p)) <= {0, -1}, name
        assert AC.sweep_threads(n) >= n // 2
    n = AC.LARGE_N_THETA
    assert n == 5_251_075 and n % 2 == 1 and n > one_pass_limit
    nt = AC.sweep_threads(n)
    assert nt == wg_max * wg
    u, p = AC.slot_and_pass(np.arange(n), n)
    assert u[-1] == -1 and p[-1] == -1                  # the entry behind the last pair
    count = {(a, b): int(np.count_nonzero((u == a) & (p == b))) for a in range(slots) for b in range(2)}
    assert int(p.max()) == 1 and sum(count.values()) == n - 1
    assert all(count[(a, 0)] == 2 * nt for a in range(slots))             # first pass: every slot of every thread live
    npair2 = n // 2 - slots * nt                                         # second pass: slot 0 full, slot 1 partly, slots 2 and 3 clamped
    assert [count[(a, 1)] for a in range(slots)] == [2 * max(0, min(nt, npair2 - a * nt)) for a in range(slots)]
    assert count[(0, 1)] == 2 * nt and 0 < count[(1, 1)] < 2 * nt and count[(2, 1)] == count[(3, 1)] == 0
    # the large mixed layout: its (class 2, class 1) and (class 1, class 2) pairs are handled in the second pass
    n2 = AC.LARGE_MIXED_N_THETA
    assert n2 == 5_251_098 and AC.sweep_threads(n2) == nt
    for a, b in AC.LARGE_MIXED_PAIRS:
        assert a % 2 == 0 and b == a + 1
        assert [int(x) for x in AC.slot_and_pass(a, n2)] == [int(x) for x in AC.slot_and_pass(b, n2)] == [1, 1]

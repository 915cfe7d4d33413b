"""The case table of tests/test_gpu_wide_input.py (tests/wide_input_cases.py) without a GPU: every branch in the input width that the
table names is reached by at least one case — the conditions restated in Python from D_in and Mp —, each padded inducing count is the
one the case says, and the oracle alone stays far inside the bars of the GPU test: finite values, cond(Ku) < 1e8 in every layer, and for
the single-layer cases the ELBO and every gradient block on column-permuted inputs, un-permuted, 100 x closer to the original than the
GPU bars (ELBO rtol 1e-11, gradient blocks 1e-9 of their largest entry): the bars are not hiding reference noise."""
import numpy as np
import pytest

from oracle import dgp_oracle as O
from oracle import model as OM
from tests import wide_input_cases as W

CASES = W.CASES


def _layers(pred=lambda c: True):
    """(case, layer index, D_in, D_out) of every layer of the table"""
    return [(c, l, din, dout) for c in CASES if pred(c) for l, (din, dout) in enumerate(W.layer_dims(c))]


def _bwd_blocks(c, l):
    return W.blocks(c.N if l == 0 else c.S * c.N)


def test_names_are_unique_and_every_case_says_what_it_is_for():
    assert len(W.BY_NAME) == len(CASES)
    for c in CASES:
        assert c.comment.strip(), c.name
        assert c.name.startswith("d%d-" % c.widths[0]), c.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_padded_inducing_count_is_the_one_named(case):
    assert W.pad_M(case.M) == case.Mp
    if "Mp%d" % case.Mp not in case.name and "M%d" % case.M not in case.name:
        assert case.Mp == 48 and case.widths[0] == 70      # the d70-L* rows name their Mp in the table only


def test_default_shape_has_three_row_blocks_the_last_one_ragged():
    for c in CASES:
        assert W.blocks(c.N) >= 2 and c.N % 16 != 0, c.name
        assert (c.N, c.S) == (35, 2) or c.name in ("d12-Mp128-last-fused", "d128-M512-chains")


def test_head_launch_branches():
    """Din <= 8 | > 8 inside the head launch, the launch itself on | off at HEAD_MAX_DIN = 16"""
    on = [c for c in CASES if W.head_on(c)]
    assert any(8 < din <= 16 for c in on for din, _ in W.layer_dims(c))
    a, b = (W.BY_NAME[n] for n in W.TWINS_HEAD)
    assert a.widths[0] == W.HEAD_MAX_DIN and b.widths[0] == W.HEAD_MAX_DIN + 1
    assert W.head_on(a) and not W.head_on(b)
    assert a._replace(name="", widths=(), comment="") == b._replace(name="", widths=(), comment="")      # twins: the width alone differs
    assert len(a.widths) == len(b.widths) == 3 and a.widths[-1] == b.widths[-1]
    assert a.Mp <= W.HEAD_MAX_N and not a.white


def test_fused_last_layer_is_taken_at_a_width_between_8_and_16():
    """layer_last_built: Mp = 128 | 256, D_out = 1, D_in <= 16; taken where dl/dKu is assembled algebraically (4 D_out Mp <= S N), the
    model is not whitened and has at least two layers; off one width past 16 whatever the rest"""
    def taken(c):
        din, dout = W.layer_dims(c)[-1]
        return (len(c.widths) >= 3 and not c.white and c.Mp in (128, 256) and dout == 1 and din <= 16 and 4 * dout * c.Mp <= c.S * c.N
                and "last_fuse" not in c.force)
    hit = [c for c in CASES if taken(c)]
    assert any(8 < W.layer_dims(c)[-1][0] <= 16 for c in hit)
    assert not taken(W.BY_NAME["d17-Mp32"]) and not taken(W.BY_NAME["d64-Mp128"])


def test_dinp16_steps():
    got = {W.din_p16(din) for _, _, din, _ in _layers()}
    assert {16, 32, 48, 80, 96} <= got
    assert W.din_p16(15) == 16 and W.din_p16(16) == 32 and W.din_p16(17) == 32
    for n in ("d15-Mp32", "d16-Mp32", "d17-Mp32"):
        assert n in W.BY_NAME


def test_wide_din_twins():
    a, b = W.BY_NAME["d32-Mp32-ard"], W.BY_NAME["d33-Mp32-ard"]
    assert a.widths[0] == W.WIDE_DIN and b.widths[0] == W.WIDE_DIN + 1 and not a.white and not b.white      # (white = True has no fused tail)
    assert a._replace(name="", widths=(), comment="") == b._replace(name="", widths=(), comment="")


def test_xch_twins_take_the_8_wave_and_the_4_wave_instances():
    a, b = W.BY_NAME["d64-Mp128"], W.BY_NAME["d65-Mp128"]
    assert a.widths[0] == W.XCH and b.widths[0] == W.XCH + 1
    assert a._replace(name="", widths=(), comment="") == b._replace(name="", widths=(), comment="")
    for l in range(2):
        nb = _bwd_blocks(a, l)
        for bwd in (False, True):
            assert W.sm_small(a.Mp, nb, W.XCH, bwd) and W.sm_nw(a.Mp, nb, W.XCH, bwd) == 8
            assert not W.sm_small(b.Mp, nb, W.XCH + 1, bwd) and W.sm_nw(b.Mp, nb, W.XCH + 1, bwd) == 4
    # the adjoint prologue of the first layer: on at 64, off at 65
    assert W.sm_adj_fusable(a.Mp, W.blocks(a.N), 64, 64) and not W.sm_adj_fusable(b.Mp, W.blocks(b.N), 65, 65)


def test_wide_instances_by_wave_count():
    """a wide layer runs 4 waves up to Mp = 256 and 8 waves from 320 to 512, in both directions"""
    nw = {}
    for c, l, din, dout in _layers():
        if din > W.XCH:
            for bwd in (False, True):
                nw.setdefault((W.sm_nw(c.Mp, _bwd_blocks(c, l), din, bwd), bwd), set()).add(c.Mp)
    for bwd in (False, True):
        assert {128, 256} <= nw[(4, bwd)] and {320, 512} <= nw[(8, bwd)]
        assert (16, bwd) not in nw
    # every padded count of the first two compiled ranges has at least one representative below 128 and one in 128 .. 256
    assert nw[(4, True)] & {32, 48, 64, 112}


def test_distance_paths_per_chunk():
    wide = [(c, din) for c, _, din, _ in _layers() if din > W.XCH]
    kinds = {}
    for c, din in wide:
        ch = W.chunks(din)
        kinds.setdefault(tuple(W.fast_path(din, jn) for _, jn in ch), []).append((c.name, din))
    assert any(len(k) == 2 and all(k) for k in kinds)                       # fast path in both chunks (jn = 64, 16)
    assert any(len(k) == 13 and all(k) for k in kinds)                      # 784 = 12 x 64 + 16
    assert (True, False) in kinds                                           # D_in % 4 == 0 with a ragged last chunk (jn = 36)
    assert (False, False, False) in kinds                                   # D_in & 3 != 0: full chunks on the masked path, 2-column tail
    assert any(din == 65 for _, din in wide) and W.chunks(65) == [(0, 64), (64, 1)]
    assert W.chunks(100)[1][1] == 36 and W.chunks(130)[2][1] == 2 and W.chunks(80) == [(0, 64), (64, 16)]


def test_ragged_tail_groups_of_the_masked_path():
    """ns = (jn - kk + 3) >> 2 < 4 in the last group of a chunk: 1, 2 and 3 k-steps on the narrow instance and on the wide one"""
    narrow, widec = set(), set()
    for c, _, din, _ in _layers():
        for _, jn in W.chunks(din):
            if W.fast_path(din, jn):
                continue
            (widec if din > W.XCH else narrow).add(W.tail_steps(jn))
    assert {1, 2, 3, 4} <= narrow, narrow
    assert {1, 2, 3, 4} <= widec, widec
    assert W.tail_steps(33) == 1 and W.tail_steps(17) == 1 and W.tail_steps(9) == 3 and W.tail_steps(70 - 64) == 2 and W.tail_steps(64) == 4


def test_single_item_epilogue_both_ways():
    """16 jn <= 64 NW per chunk of every backward launch: true and false on the narrow instance, on 4 waves and on 8"""
    seen = set()
    for c, l, din, dout in _layers():
        NW = W.sm_nw(c.Mp, _bwd_blocks(c, l), din, True)
        for _, jn in W.chunks(din):
            seen.add((din > W.XCH, NW, W.single_item(jn, NW)))
    for key in [(False, 4, True), (False, 4, False), (False, 8, False), (True, 4, True), (True, 4, False), (True, 8, True), (True, 8, False)]:
        assert key in seen, key
    assert W.single_item(16, 4) and not W.single_item(17, 4)


def test_lds_of_the_wide_chains():
    """Mp = 512 wide: above the 64 KB default, inside the 160 KB of the chip (the attribute path); wide layers from Mp = 640 on do not
    fit and have to be refused"""
    c = W.BY_NAME["d128-M512-chains"]
    din, dout = W.layer_dims(c)[0]
    assert "gemm_mp=0" in c.force
    for bwd in (False, True):
        NW = W.sm_nw(c.Mp, W.blocks(c.N), din, bwd)
        assert NW == 8
        assert 64 * 1024 < W.sm_lds_bytes(c.Mp, din, dout, NW) <= 160 * 1024
    for M, din, force in W.UNSUPPORTED:
        Mp = W.pad_M(M)
        assert W.sm_nw(Mp, 1, din, False) == 16 and W.sm_lds_bytes(Mp, din, 1, 16) > 160 * 1024 and force == "gemm_mp=0"
    for c2, l, din, dout in _layers():
        if c2 is not c:
            NW = W.sm_nw(c2.Mp, _bwd_blocks(c2, l), din, True)
            assert W.sm_lds_bytes(c2.Mp, din, dout, NW, 2 if "save_c=2" in c2.force else 1) <= 160 * 1024


def test_epilogue_instances_of_the_wide_chains():
    wide_last = [c for c in CASES if len(c.widths) >= 3 and W.layer_dims(c)[-1][0] > W.XCH]
    assert {1, 3} <= {c.widths[-1] for c in wide_last}                                 # WIDE && LIK, one and three outputs
    assert any(c.white for c in CASES if c.widths[0] > W.XCH) and any(c.kind == "matern52" and not c.white for c in wide_last)
    cs = [c for c in CASES if "save_c=2" in c.force]
    assert cs and all(c.widths[0] > W.XCH and c.Mp in (32, 64, 128, 256) for c in cs)   # sm_cs_built
    ds = [c for c in CASES if "bwd_split=2" in c.force]
    assert ds and all(len(c.widths) >= 3 and W.layer_dims(c)[-1][0] > W.XCH and c.widths[-1] >= 2 for c in ds)
    pca = [c for c in CASES if len(c.widths) >= 3 and c.widths[0] > W.XCH and c.widths[1] < c.widths[0]]
    assert {len(W.chunks(c.widths[0])) for c in pca} == {2, 13}
    assert sum(c.two_steps for c in CASES) == 2 and W.BY_NAME["d90-M100-ard"].two_steps and W.BY_NAME["d130-Mp320"].two_steps
    ref = W.BY_NAME["d90-M100-ard"]
    assert ref.widths == (90, 90, 1) and ref.M == 100 and ref.ard


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_is_finite_and_well_conditioned(case):
    r = W.reference(case)
    assert np.isfinite(r["elbo"])
    for k, g in r["grad"].items():
        assert np.all(np.isfinite(g)), k
        assert np.max(np.abs(g)) > 0.0, k               # every block carries signal: a relative bar means something
    for F in r["prop"]:
        for a in F:
            assert np.all(np.isfinite(a))
    om = OM.build(O.NP, r["spec"], r["state"])
    for l, layer in enumerate(om.layers):
        Ku, _ = layer.build_cholesky(O.NP)
        assert np.linalg.cond(Ku) < 1e8, l


@pytest.mark.parametrize("case", [c for c in CASES if len(c.widths) == 2], ids=[c.name for c in CASES if len(c.widths) == 2])
def test_oracle_on_permuted_columns_agrees_100x_inside_the_gpu_bars(case):
    """The same model on relabelled input dimensions: other summation orders in every distance, the same mathematics.  (Single-layer
    cases only: an identity mean ties the columns of an inner layer to the outputs of the one below.)"""
    r = W.reference(case)
    D = case.widths[0]
    perm = np.random.RandomState(D).permutation(D)
    inp = W.case_inputs(case, perm=perm)
    spec, state = W.oracle_state(case, inp)
    e2, g2 = OM.elbo_and_grad(spec, state, inp["X"], inp["Y"], inp["zs"], case.S, num_data=r["num_data"])
    print("ELBO: rel %.2e" % (abs(e2 - r["elbo"]) / abs(r["elbo"])))
    assert abs(e2 - r["elbo"]) <= 1e-11 * abs(r["elbo"]) + 1e-12
    inv = np.argsort(perm)
    for k, a in r["grad"].items():
        b = g2[k]
        if k == "l0.Z":
            b = b[:, inv]
        elif k == "l0.kern_lengthscales_raw" and case.ard:
            b = b[inv]
        err = np.max(np.abs(a - b)) / np.max(np.abs(a))
        print("%s: %.2e of the largest entry" % (k, err))
        assert err <= 1e-9, (k, err)

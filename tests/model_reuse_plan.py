"""Call sequences, data pools and the bit comparison of tests/test_gpu_model_reuse.py (numpy only: tests/test_model_reuse_plan_cpu.py
checks this file on a machine without a GPU).

A device model is re-created only when a call outgrows its extents (Engine._ensure); every smaller call runs on the workspace the
earlier calls left behind, re-strided for its own shape.  The sequences below walk one model through the shapes at which the launch
schedule changes and through every kind of call, so that each call meets pads, partial sums and flags of a different predecessor.

Call kinds (what is compared is listed in test_gpu_model_reuse.py::_run_call):
  G   ELBO + full gradient, explicit draws        V   forward-only ELBO and E_log_p_Y       P   propagate
  Q   (q_mu, q_sqrt)-only reverse pass from layer 1                                          E   evaluate, ragged second batch
  Gd  ELBO + full gradient, device Philox draws under an explicit seed
  C   conditional_ND of every layer on `n` rows  Cw  the same through the C-ABI on more rows than n_max * s_max (chunked walk of the
                                                      GEMM-formulated pass; the host mirror would re-create the model first)

Inputs.  Position i of a sequence takes its rows from pool "b" (i even) or "a" (i odd) at a row offset of its own, so no two calls of a
sequence see the same inputs and direct neighbours differ in magnitude as well (pool b: X = 1.7 x + 0.3, Y = 1e3 y, other generator
streams): content that a call left in the workspace is never what a later call should have written there.
"""
import numpy as np

ROW_STEP = 7      # row offset between the inputs of consecutive positions


class Config:
    def __init__(self, name, extents, shapes, seq, anchor, M, widths, DY):
        self.name, self.extents, self.shapes, self.seq, self.anchor = name, extents, shapes, seq, anchor
        self.M, self.widths, self.DY = M, widths, DY

    @property
    def pool_rows(self):
        rows = max([self.extents[0]] + [c[1] for c in self.seq if c[0] in ("C", "Cw")])
        return rows + ROW_STEP * len(self.seq)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. headline path: M = 128 (Mp = 128), widths 8 -> 8 -> 8 -> 1, Gaussian, white = False: head launch, fused last layer, fused tail.
#    Layers >= 1 run on n S rows = ceil(n S / 16) row blocks (layer 0 on n rows).
#
#    (n, S)       row blocks   forward chain   backward chain   d_split (D_out 8)   streams   P_d tasks
#    (1000, 13)   813          4-wave (> 160)  4-wave (> 768)   1 (>= 512)          two       grouped
#    (330, 8)     165          4-wave (> 160)  8-wave           3 (512 / 165)       two       grouped
#    (100, 8)     50           8-wave          8-wave           4                   one       ungrouped
#    (100, 3)     19           8-wave          8-wave           4                   one       ungrouped
#    (37, 1)      3 (2.16 + 5 rows: ragged last block)           4                   one       ungrouped
#    (1, 1)       1                                               4                   one       ungrouped
#    two streams: n S Mp >= 2^18 (overlap_on); grouped P_d: two streams, D_out >= 3, Mw = 128 (ensure_plan)
A1, A2, A3, A4, A5, A3S = (1000, 13), (330, 8), (100, 3), (37, 1), (1, 1), (100, 8)
CONFIG_A = Config("A", A1, [A1, A2, A3, A4, A5], [
    ("G", *A1),        # the largest shape first
    ("G", *A4),        # shrink: every pad of the 37-row strides lies on the 13 000-row call's data
    ("P", *A2),        # growth back, forward only
    ("G", *A2),        # forward-only prepare, then a gradient prepare at unchanged parameters
    ("Q", *A3),        # pruned reverse pass: the partial sums of layer 0 stay stale by design
    ("G", *A5),        # ... and a full pass of another shape right behind it
    ("V", *A1),
    ("G", *A3),
    ("G", *A3S),       # S alone: layer 0 keeps its 100 rows, the layers above go from 300 to 800
    ("Gd", *A2),
    ("E", *A2),
    ("G", *A4),        # oracle anchor
    ("C", 777, 1),
    ("G", *A1),
], anchor=11, M=128, widths=[8, 8, 8], DY=1)

# B. M = 100: Mp = 112 on Mw = 128-row weight-gradient tiles (rows 112 .. 127 are pad); Matern52 + White below ARD RBF; widths
#    5 -> 3 -> 3, DY = 2: the 5 -> 3 step-down carries a fixed Linear mean, the last layer runs as two chains (d_split 2) with the
#    likelihood epilogue.  Mp < 128: every chain is the 4-wave instance.
#    (n, S)     row blocks   d_split (D_out 3 / 3 / 2)   ld = round_up(n S, 16) - n S pad columns
#    (300, 4)   75           3 / 3 / 2                   0
#    (96, 3)    18           3 / 3 / 2                   0      (layer 0: 96 rows, 0)
#    (40, 3)    8            3 / 3 / 2                   8      (layer 0: 40 rows, 8)
#    (37, 1)    3            3 / 3 / 2                   11
#    (17, 2)    3            3 / 3 / 2                   14     (layer 0: 17 rows, 15)
#    (17, 4)    5            3 / 3 / 2                   12
#    (1, 1)     1            3 / 3 / 2                   15
#    n S Mp < 2^18 throughout: one stream
B1, B2, B3, B4, B5, B6, B5S = (300, 4), (96, 3), (40, 3), (37, 1), (17, 2), (1, 1), (17, 4)
_SEQ_B = [
    ("G", *B1),
    ("G", *B4),        # shrink
    ("P", *B2),        # growth back
    ("G", *B2),        # forward-only prepare, then a gradient prepare
    ("Q", *B3),
    ("G", *B5),        # full pass of another shape behind the pruned one
    ("G", *B5S),       # S alone
    ("V", *B1),
    ("G", *B6),
    ("Gd", *B2),
    ("E", *B1),
    ("G", *B3),        # oracle anchor
    ("C", 211, 1),
    ("G", *B1),
]
CONFIG_B = Config("B", B1, [B1, B2, B3, B4, B5, B6], _SEQ_B, anchor=11, M=100, widths=[5, 3, 3], DY=2)

# C. white = True, M = 40: Mp = 48 (ragged wave ownership of the 16-row blocks of the factor), Mw = 64; two layers 3 -> 3, DY = 2;
#    the Cholesky adjoint, Lu kept.  Shapes and switches as B.
CONFIG_C = Config("C", B1, [B1, B2, B3, B4, B5, B6], _SEQ_B, anchor=11, M=40, widths=[3, 3], DY=2)

# D. DSDGP_FORCE=gemm_mp=16: every layer through the GEMM-formulated passes (T1 / T2 / Pb / colsq / MUT / ZZ / OUTt scratch).  M = 40, two
#    layers; shapes as B plus conditional_ND on 1300 > 300 * 4 rows, which the GEMM pass walks in chunks of its scratch.
CONFIG_D = Config("D", B1, [B1, B2, B3, B4, B5, B6], _SEQ_B[:-1] + [("Cw", 1300, 1), _SEQ_B[-1]], anchor=None, M=40, widths=[4, 4], DY=2)

# E. M = 300: Mp = 320 (8-wave chains at every size), Csave backward chain, backward d-split with the ticketed hand-over
#    (bpart / bcnt), look-ahead Cholesky.  Widths 6 -> 6, DY = 2.
#    (n, S)      row blocks   d_split (layer 0, D_out 6)
#    (600, 8)    300          1   (256 .. 511 blocks: min(1024 / 300, 6 / 5))
#    (330, 8)    165          3
#    (330, 4)    83           4
#    (200, 4)    50           4
#    (37, 1)     3            4
E1, E2, E3, E4, E2S = (600, 8), (330, 8), (200, 4), (37, 1), (330, 4)
CONFIG_E = Config("E", E1, [E3, E2, E1, E4], [
    ("G", *E1),
    ("G", *E4),        # shrink
    ("P", *E3),        # growth back
    ("G", *E3),        # forward-only prepare, then a gradient prepare
    ("Q", *E2),
    ("G", *E2S),       # full pass of another shape behind the pruned one
    ("G", *E2),        # S alone
    ("V", *E1),
    ("Gd", *E3),
    ("E", *E2),
    ("C", 500, 1),
    ("G", *E4),
    ("G", *E1),
], anchor=None, M=300, widths=[6, 6], DY=2)

# F. D_in = 70 > XCH = 64: layer 0 takes the WIDE chain instances; M = 32, widths 70 -> 5, MultiClass(3) (k_adj_prep writes MB, VB and
#    [X^T;1] of the last layer).  One stream, 4-wave chains.
#    (n, S)     row blocks   pad columns of the layers >= 1 / of layer 0
#    (96, 3)    18           0 / 0
#    (40, 3)    8            8 / 8
#    (40, 2)    5            0 / 8
#    (37, 1)    3            11 / 11
#    (1, 1)     1            15 / 15
F1, F2, F3, F4, F2S = (96, 3), (40, 2), (37, 1), (1, 1), (40, 3)
CONFIG_F = Config("F", F1, [F1, F2, F3, F4], [
    ("G", *F1),
    ("G", *F3),        # shrink
    ("P", *F2),        # growth back
    ("G", *F2),        # forward-only prepare, then a gradient prepare
    ("Q", *F3),
    ("G", *F2S),       # full pass of another shape behind the pruned one
    ("G", *F2),        # S alone
    ("V", *F1),
    ("G", *F4),
    ("Gd", *F2),
    ("E", *F1),
    ("C", 77, 1),
    ("G", *F1),
], anchor=None, M=32, widths=[70, 5], DY=3)

CONFIGS = {c.name: c for c in (CONFIG_A, CONFIG_B, CONFIG_C, CONFIG_D, CONFIG_E, CONFIG_F)}

# read-only calls that model U of the P2 test makes between the optimiser steps of (config, step shape): one after each of the first
# five steps (two after the fifth), at the OTHER shapes of the configuration
P2_CASES = {
    "A": dict(step=A3, between=[[("P", *A2)], [("V", *A1)], [("G", *A4)], [("Q", *A2)], [("E", *A1), ("C", 777, 1)]]),
    "C": dict(step=B3, between=[[("P", *B2)], [("V", *B1)], [("G", *B4)], [("Q", *B5)], [("E", *B1), ("C", 211, 1)]]),
}
P2_STEPS = 6
P2_MINIBATCH_STEPS = (2, 4)      # these go through train_step_minibatch: gather and device draws inside the step


# ---------------------------------------------------------------------------------------------------------------------------------
def pool_of(position):
    return "b" if position % 2 == 0 else "a"


def make_pool(cfg, which, num_classes=None):
    """{"X": (rows, D_in), "Y": (rows, DY) or (rows, 1) labels, "zs": [(s_max, rows, D_out_l)]} — all finite"""
    rng = np.random.RandomState({"a": 1234, "b": 98765}[which] + len(cfg.name) + ord(cfg.name[0]))
    rows, s_max = cfg.pool_rows, cfg.extents[1]
    X = rng.randn(rows, cfg.widths[0])
    if num_classes:
        Y = rng.choice(np.arange(num_classes, dtype=np.float64), rows).reshape(rows, 1)
    else:
        Y = rng.randn(rows, cfg.DY)
    zs = [rng.randn(s_max, rows, d) for d in cfg.widths[1:] + [cfg.DY]]
    if which == "b":
        X = 1.7 * X + 0.3
        if not num_classes:
            Y = 1e3 * Y
        zs = [1.5 * z for z in zs]
    return dict(X=X, Y=Y, zs=zs)


def call_inputs(pools, position, n, S):
    """(X, Y, zs) of the call at `position` on n rows and S samples: contiguous copies"""
    p = pools[pool_of(position)]
    a = ROW_STEP * position
    assert a + n <= p["X"].shape[0]
    return (np.ascontiguousarray(p["X"][a:a + n]), np.ascontiguousarray(p["Y"][a:a + n]),
            [np.ascontiguousarray(z[:S, a:a + n]) for z in p["zs"]])


def conditional_inputs(pools, position, n):
    """one (n, D_in_l) input per layer for the C / Cw call at `position`: layer 0 from X, layer l from the draws of width D_in_l"""
    p = pools[pool_of(position)]
    a = ROW_STEP * position
    assert a + n <= p["X"].shape[0]
    return [np.ascontiguousarray(p["X"][a:a + n])] + [np.ascontiguousarray(z[0, a:a + n]) for z in p["zs"][:-1]]


# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.atleast_1d(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).view(np.uint64)


def bits_diff(got, want):
    """None when the two float64 arrays have one shape and one bit pattern (NaN equals the same NaN, -0.0 differs from 0.0), else a
    one-line description of the difference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    ne = _bits(got) != _bits(want)
    if not ne.any():
        return None
    g, w = np.atleast_1d(got), np.atleast_1d(want)
    first = tuple(int(i) for i in np.argwhere(ne.reshape(g.shape))[0])
    with np.errstate(invalid="ignore"):
        d = np.abs(g - w)[ne.reshape(g.shape)]
    return (f"{int(ne.sum())} of {ne.size} entries differ, first at {first}: {g[first]!r} against {w[first]!r}"
            f" (max |diff| {np.nanmax(d) if np.isfinite(d).any() else float('nan'):.3e})")


def assert_same_bits(got, want, what):
    """got, want: dicts of float64 arrays with the same keys"""
    assert list(got.keys()) == list(want.keys()), (what, list(got.keys()), list(want.keys()))
    bad = {k: d for k, d in ((k, bits_diff(got[k], want[k])) for k in want) if d is not None}
    assert not bad, f"{what}: " + "; ".join(f"{k}: {d}" for k, d in bad.items())


# ---------------------------------------------------------------------------------------------------------------------------------
# Mirrors of the shape-dependent switches (csrc/chain_policy.hpp: sm_small / sm_nw, chain_d_split; model_schedule.hpp:
# overlap_on with the default overlap_min) for the tables above.
def padded_M(M):
    if M <= 32:
        return 32
    q = 16 if M <= 128 else 32 if M <= 256 else 64 if M <= 512 else 128
    return -(-M // q) * q


def row_blocks(n, S):
    return -(-(n * S) // 16)


def chain_waves(Mp, nblk, bwd):
    if Mp > 256:
        return 16 if Mp > 512 else 8
    lim = (1 << 40) if Mp > 128 else (768 if bwd else 160)
    return 8 if 128 <= Mp <= 256 and nblk <= lim else 4


def chain_d_split(nblk, D_out):
    ds = 1
    if nblk < 256:
        ds = min(4, max(1, 512 // nblk))
    elif nblk < 512:
        ds = min(1024 // nblk, D_out // 5)
    return max(1, min(ds, D_out))


def two_streams(n, S, Mp):
    return n * S * Mp >= 1 << 18

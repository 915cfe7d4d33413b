"""The case table of tests/test_gpu_wide_input.py, shared with tests/test_wide_input_cases_cpu.py (which asserts that the table reaches
every branch in the input width it names and that the oracle alone stays inside the bars).  CPU only, no product code.

The split-M chain kernels (csrc/layer_sm_impl.hpp) branch on the input width D_in of a layer in many places; the host side mirrors
of those conditions are the functions below (`chunks`, `fast_path`, `tail_steps`, `single_item`, ...), restated from the sources so
that the CPU test can say which case runs which branch:

    D_in <= 8 | > 8          head launch: two or four k-steps of the Ku Gram block          (head_impl.hpp, head_factor)
    D_in <= 16 | > 16        head launch on / off (HEAD_MAX_DIN), fused last layer built    (model.hip head_ok, chain_policy.hpp layer_last_built)
    D_in + 1 <= 16 | > 16    DinP16 = round_up(D_in + 1, 16): 16 -> 32 between 15 and 16    (model_layout.hpp; thinz / WZ / XT1 products)
    D_in <= 32 | > 32        fused tail and folded Ku-side adjoints on / off (WIDE_DIN)     (model.hip tail_ok, model_kernels.hpp)
    D_in <= 64 | > 64        narrow | WIDE chain instances (XCH), 8-wave instances and the
                             adjoint prologue off above                                     (chain_policy.hpp sm_small / sm_nw / sm_adj_fusable)
    per 64-column chunk      whole groups of 16 with D_in % 4 == 0: the 32-byte-load path,
                             else the masked path; a last group of fewer than 16 dimensions
                             issues ns = 1 .. 3 k-steps                                     (sm_sqdist, sqdist_chunk_masked)
    16 jn <= 64 NW           one epilogue item per thread: operands requested early         (backward chain, `single`)

Common recipe (so that the oracle is well conditioned and cheap at any width): X ~ randn(N + M, D_in); Z = the M held-out rows of X
plus 0.02 randn; lengthscales sqrt(D) U(0.8, 1.2) for a layer of input width D (per dimension where the case is ARD), which keeps r^2
of order 1; kernel variance 1.1; (q_mu, q_sqrt) randomised as tests.helpers.make_case does; num_data = 4 N; N = 35 (three row blocks,
the last one ragged) and S = 2 unless the case says otherwise.  `widths` = the input width of every layer followed by the width of Y:
equal neighbours give an identity mean (the reference's construction: every inner layer as wide as the data), a narrower successor the
PCA Linear mean.

Differences from the table the cases were asked with, each from reading the sources:
  * DinP16 = round_up(D_in + 1, 16) steps from 16 to 32 between D_in = 15 and 16, not between 16 and 17: `d15` joins the 16 | 17 twins.
  * WIDE_DIN = 32 (fused tail, Ku-side Z / lengthscale adjoints as GEMMs above it) is a threshold in D_in of its own: `d32` | `d33` twins.
  * the forward chain's likelihood epilogue (LIK) runs on the LAST layer of a model of at least two layers (model_schedule.hpp,
    elbo_impl: fused_last needs L > 1), so WIDE && LIK needs a wide last layer: every `(…, D, D, 1)` case above 64 has one, and
    `d70-L2-D3` runs it with three outputs next to the single-layer pair that was asked for.
"""
from collections import namedtuple

import numpy as np

from oracle import dgp_oracle as O
from oracle import model as OM
from tests.helpers import kern_spec

XCH = 64            # layer_sm_impl.hpp: columns of x / l staged per chunk
HEAD_MAX_DIN = 16   # head_impl.hpp
HEAD_MAX_N = 128    # head_impl.hpp
WIDE_DIN = 32       # model_types.hpp
SM_SMALL_BLOCKS = 160       # chain_policy.hpp
SM_BWD_RESIDENT_8W = 768    # chain_policy.hpp

Case = namedtuple("Case", "name widths M Mp N S kind white ard force two_steps comment")


def _c(name, widths, M, Mp, comment, N=35, S=2, kind="rbf", white=False, ard=False, force="", two_steps=False):
    return Case(name, tuple(widths), M, Mp, N, S, kind, white, ard, force, two_steps, comment)


CASES = [
    # ------------------------------------------------------------ narrow instance (D_in <= 64): ragged k-steps
    _c("d9-Mp112", (9, 9, 1), 100, 112, "head launch's Din > 8 branch; ns = 3 tail group"),
    _c("d12-Mp128-last-fused", (12, 12, 1), 128, 128, "fused last layer (layer_last.hip) at 8 < D_in <= 16: 4 Mp <= S N", N=130, S=4),
    _c("d15-Mp32", (15, 15, 1), 20, 32, "DinP16 = 16: the last width below the 16 -> 32 step of the thinz products"),
    _c("d16-Mp32", (16, 16, 1), 20, 32, "HEAD_MAX_DIN and layer_last_built exactly met: head launch on; DinP16 = 32; one whole k-group"),
    _c("d17-Mp32", (17, 17, 1), 20, 32, "head launch off (k_prep_kuu + k_potrf_trtri); one-dimension second group, ns = 1; single off"),
    _c("d32-Mp32-ard", (32, 32, 1), 30, 32, "WIDE_DIN exactly met: fused tail and folded Ku-side adjoints still on", ard=True),
    _c("d33-Mp32-ard", (33, 33, 1), 30, 32, "past WIDE_DIN: k_asm_kbar + the GEMM form of the Z / lengthscale adjoints", ard=True),
    _c("d33-Mp64-matern-white-ard", (33, 33, 1), 60, 64, "one-dimension tail group, ns = 1, in the Matern WHITE instances", kind="matern52",
       white=True, ard=True),
    _c("d64-Mp128", (64, 64, 1), 120, 128, "exactly XCH: last width on the narrow 8-wave instance (sm_small true)"),
    # ------------------------------------------------------------ wide instance (D_in > 64)
    _c("d65-Mp128", (65, 65, 1), 120, 128, "one-column second chunk; 4-wave instance because sm_small is false; adjoint prologue off"),
    _c("d80-Mp112", (80, 80, 1), 100, 112, "sm_sqdist fast path in both chunks (jn = 64, 16)"),
    _c("d90-M100-ard", (90, 90, 1), 100, 112, "the reference benchmark's shape: wide inner layer, identity mean, dX, adjoints not fused",
       ard=True, two_steps=True),
    _c("d100-Mp256-matern-white", (100, 2), 250, 256, "jn = 36 masked chunk while D_in % 4 == 0 (first chunk on the fast path); 4-wave Mp = 256",
       kind="matern52", white=True),
    _c("d130-Mp320", (130, 130, 1), 270, 320, "8-wave wide instance; two full masked chunks (D_in & 3 != 0) and a 2-column tail",
       kind="matern52", two_steps=True),
    _c("d128-M512-chains", (128, 3), 512, 512, "wide chain at Mp = 512 (8 waves both ways): LDS above 64 KB, the attribute path", N=20,
       force="gemm_mp=0"),
    _c("d70-L1-D1", (70, 1), 40, 48, "wide single layer (rep = S epilogue), one output"),
    _c("d70-L1-D3", (70, 3), 40, 48, "wide single layer (rep = S epilogue), three outputs, ARD", ard=True),
    _c("d70-L2-D3", (70, 70, 3), 40, 48, "WIDE && LIK forward epilogue with three outputs (last layer of two)"),
    _c("d70-pca5-Mp32", (70, 5, 1), 30, 32, "PCA Linear mean under a wide layer (mean_A in the forward epilogue); two chunks"),
    _c("d784-pca30-Mp32", (784, 30, 1), 30, 32, "PCA Linear mean under a wide layer; 13 chunks, all on the fast path"),
    _c("d70-Mp128-csave", (70, 70, 3), 128, 128, "WIDE && CS backward chain (c_d kept by the wide forward chain)",
       force="save_c=2,cs_min_blocks=0,cs_min_dout=1"),
    _c("d70-Mp64-dsplit", (70, 70, 5), 60, 64, "d-split hand-over of the backward chain with chunked dX", force="bwd_split=2"),
]
BY_NAME = {c.name: c for c in CASES}
TWINS_HEAD = ("d16-Mp32", "d17-Mp32")
# a wide layer whose chains cannot hold their staging in the LDS must be refused: (M, D_in, force)
UNSUPPORTED = [(600, 70, "gemm_mp=0"), (1024, 70, "gemm_mp=0")]


# ---------------------------------------------------------------------------------------------- the conditions, restated
def pad_M(M):
    """common.hpp pad_M"""
    def up(a, b):
        return (a + b - 1) // b * b
    if M <= 32:
        return 32
    if M <= 128:
        return up(M, 16)
    if M <= 256:
        return up(M, 32)
    if M <= 512:
        return up(M, 64)
    return up(M, 128)


def layer_dims(case):
    """[(D_in, D_out)] of every layer"""
    w = case.widths
    return [(w[i], w[i + 1]) for i in range(len(w) - 1)]


def din_p16(D_in):
    return (D_in + 1 + 15) // 16 * 16


def chunks(D_in):
    """[(j0, jn)] of the 64-column chunks of a wide layer (one chunk of D_in columns on the narrow instance)"""
    return [(j0, min(XCH, D_in - j0)) for j0 in range(0, D_in, XCH)]


def fast_path(D_in, jn):
    """sm_sqdist: whole groups of 16 dimensions read with one 32-byte load (wide instances only)"""
    return D_in > XCH and (jn & 15) == 0 and (D_in & 3) == 0


def tail_steps(jn):
    """k-steps ns of the last group of 16 of a chunk on the masked path (4 = a whole group)"""
    r = jn % 16
    return 4 if r == 0 else (r + 3) >> 2


def sm_small(Mp, nblk, D_in, bwd):
    lim = (1 << 40) if Mp > 128 else (SM_BWD_RESIDENT_8W if bwd else SM_SMALL_BLOCKS)
    return 128 <= Mp <= 256 and nblk <= lim and D_in <= XCH


def sm_nw(Mp, nblk, D_in, bwd):
    if Mp > 512 or (Mp == 512 and D_in <= XCH and not bwd):
        return 16
    if Mp > 256:
        return 8
    return 8 if sm_small(Mp, nblk, D_in, bwd) else 4


def sm_adj_fusable(Mp, nblk, D_in, D_out):
    if D_in > XCH:
        return False
    return sm_nw(Mp, nblk, D_in, True) * 16 * min(D_in, XCH) >= 2 * 16 * D_out


def single_item(jn, NW):
    return 16 * jn <= NW * 64


def sm_lds_bytes(Mp, D_in, D_out, NW, nbuf=1):
    """layer_sm_impl.hpp sm_lds"""
    wide = D_in > XCH
    xch = min(D_in, XCH)
    o = 16 * (xch + 1)
    o += o & 1
    o += Mp * 16
    db = 8 if NW == 4 else (4 if NW == 8 else 1)
    mu_early = NW == 4 and not wide
    red = max(NW * 16 + 2 * db * NW * 16 + (NW * 16 * D_out if mu_early else 2 * db * NW * 16), NW * 16 * xch)
    if nbuf == 2:
        red = max(red, Mp * 16)
    return 8 * (o + red)


def head_on(case):
    return all(d <= HEAD_MAX_DIN for d, _ in layer_dims(case)) and case.Mp <= HEAD_MAX_N


def blocks(rows):
    return -(-rows // 16)


# ---------------------------------------------------------------------------------------------- inputs and the oracle's side
def _seed(case):
    return sum(map(ord, case.name))


def case_inputs(case, perm=None):
    """-> dict(X, Y, Z, specs, zs): seeded, the same arrays in every process.  `perm`: the columns of X and Z and the ARD lengthscales
    of the first layer permuted (the same model on relabelled input dimensions)."""
    rng = np.random.RandomState(_seed(case))
    dims = layer_dims(case)
    D, DY = dims[0][0], case.widths[-1]
    XZ = rng.randn(case.N + case.M, D)
    Y = rng.randn(case.N, DY)
    Z = XZ[case.N:] + 0.02 * rng.randn(case.M, D)
    X = XZ[:case.N].copy()
    specs = []
    for d_in, _ in dims:
        u = 0.8 + 0.4 * rng.rand(d_in)
        ls = np.sqrt(d_in) * (u if case.ard else float(u[0]))
        specs.append(kern_spec(case.kind, d_in, 1.1, ls, case.ard))
    zs = [rng.randn(case.S, case.N, d_out) for _, d_out in dims]
    if perm is not None:
        X, Z = X[:, perm], Z[:, perm]
        if case.ard:
            specs[0] = dict(specs[0], lengthscales=specs[0]["lengthscales"][perm])
    return dict(X=X, Y=Y, Z=Z, specs=specs, zs=zs)


MAKE_CASE_SEED = 3


def oracle_state(case, inp=None):
    """(spec, state) exactly as tests.helpers.make_case(..., seed = MAKE_CASE_SEED) builds them, without the device model"""
    inp = inp or case_inputs(case)
    rng = np.random.RandomState(MAKE_CASE_SEED)
    lds = O.init_layers_linear(inp["X"], inp["Y"], inp["Z"], inp["specs"], white=case.white, jitter=1e-6, num_outputs=None)
    for l in lds:
        l["q_mu"] = 0.3 * rng.randn(*l["q_mu"].shape)
        D, M = l["q_sqrt"].shape[0], l["q_sqrt"].shape[1]
        l["q_sqrt"] = l["q_sqrt"] * 0.7 + 0.05 * np.tril(rng.randn(D, M, M))
    sl, state = OM.state_from_layers(lds, lik_variance=0.1, likelihood="gaussian")
    spec = dict(jitter=1e-6, white=case.white, likelihood="gaussian", layers=sl, num_classes=None, lik_aux=None)
    return spec, state


_REF = {}


def reference(case):
    """inputs and the oracle's results of one case, computed once per process and left unchanged"""
    if case.name not in _REF:
        inp = case_inputs(case)
        spec, state = oracle_state(case, inp)
        num_data = 4 * case.N
        elbo, grad = OM.elbo_and_grad(spec, state, inp["X"], inp["Y"], inp["zs"], case.S, num_data=num_data)
        prop = OM.propagate(spec, state, inp["X"], inp["zs"], case.S)
        _REF[case.name] = dict(inp=inp, spec=spec, state=state, num_data=num_data, elbo=elbo, grad=grad, prop=prop)
    return _REF[case.name]

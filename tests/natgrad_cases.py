"""The case table of tests/test_gpu_natgrad_direct.py, shared with tests/test_natgrad_reference_cpu.py (which asserts the conditions
the GPU cases rely on at every M of the table).  CPU only, no product code.

path                          M -> Mp                       D_out
LDS one-workgroup             9 -> 32, 20 -> 32, 100 -> 112, 128     1, 3 (10 at M = 20)
global-memory one-workgroup   150 -> 160, 200 -> 224        2        (Mp in (128, 256) that is no multiple of 64: k_trtri_only + potrf in global memory)
look-ahead BigChol            180 -> 192, 256, 300 -> 320   2        (+ M = 300 with DSDGP_CHOL_LOOKAHEAD=0: the plain blocked sequence)
big tiles                     570 -> 640                    1        (dense, init_prior)
GEMM-formulated layer         1100 -> 1152                  1        (dense; float64 products in the measures)
Every row: T families dense and init_prior, both gradient families at gamma = 0.1, white = False.  One M per path (`full`) also gets
init_white / init_inner / dense_scaled, quad at gamma = 1, two white = True cases and the evaluation after the step; the two largest
paths get quad at gamma = 1, one white = True case and the evaluation after the step on `dense`."""
from collections import namedtuple

from tests import natgrad_reference as NG

Case = namedtuple("Case", "path M D_out t_family g_family gamma white plain eval_after")

PATHS = [
    # (path, [(M, D_outs)], M of the full set, D_out of the full set)
    ("lds", [(9, (1, 3)), (20, (1, 3, 10)), (100, (1, 3)), (128, (1, 3))], 100, 3),
    ("potrf-global", [(150, (2,)), (200, (2,))], 150, 2),
    ("look-ahead", [(180, (2,)), (256, (2,)), (300, (2,))], 180, 2),
    ("big tiles", [(570, (1,))], None, 1),
    ("gemm layers", [(1100, (1,))], None, 1),
]


def _cases():
    out = []
    for path, sizes, full_M, full_D in PATHS:
        for M, D_outs in sizes:
            for D in D_outs:
                tfs = ("dense",) if M == 1100 else ("dense", "init_prior")
                for tf in tfs:
                    for gf in NG.G_FAMILIES:
                        # the evaluation after the step: one case per path (the two largest paths have no `full` M)
                        ev = (M == full_M and D == full_D or full_M is None) and tf == "dense" and gf == "quad"
                        out.append(Case(path, M, D, tf, gf, 0.1, False, False, ev))
                if M == full_M and D == full_D:
                    for tf in ("init_white", "init_inner", "dense_scaled"):
                        for gf in NG.G_FAMILIES:
                            out.append(Case(path, M, D, tf, gf, 0.1, False, False, False))
                    out.append(Case(path, M, D, "dense", "quad", 1.0, False, False, False))
                    out.append(Case(path, M, D, "dense", "generic", 0.1, True, False, False))
                    out.append(Case(path, M, D, "init_prior", "quad", 0.1, True, False, False))
        if full_M is None:
            # the two largest paths: dense only for the extras (quad at gamma = 1, one white = True case)
            M, D = sizes[0][0], full_D
            out.append(Case(path, M, D, "dense", "quad", 1.0, False, False, False))
            out.append(Case(path, M, D, "dense", "generic", 0.1, True, False, False))
        if path == "look-ahead":
            for tf in ("dense", "init_prior"):
                for gf in NG.G_FAMILIES:
                    out.append(Case("plain blocked", 300, 2, tf, gf, 0.1, False, True, tf == "dense" and gf == "quad"))
    return out


CASES = _cases()
REFUSED_M = (20, 300)
TWO_STEP_M = (150, 300)
UNIFORM_BIG_M = 192


def case_id(c):
    return (f"{c.path.replace(' ', '_')}-M{c.M}-D{c.D_out}-{c.t_family}-{c.g_family}-g{c.gamma:g}" + ("-white" if c.white else "")
            + ("-plain" if c.plain else ""))


def case_inputs(t_family, M, D_out, g_family, seed=0, w_scale=1.0):
    """-> (q_mu, q_sqrt, g_mu, g_sqrt) of one case (seeded: the same arrays in every process)"""
    q_mu, q_sqrt = NG.t_family(t_family, M, D_out, seed)
    g_mu, g_sqrt = NG.g_family(g_family, q_mu, q_sqrt, seed, w_scale)
    return q_mu, q_sqrt, g_mu, g_sqrt

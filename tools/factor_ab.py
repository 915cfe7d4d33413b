#!/usr/bin/env python
"""Bits of everything the blocked Cholesky + triangular inverse (csrc/chol_plan.hpp, linalg.hip: bigchol_build / bigchol_run) produces,
for a before/after comparison of two builds of the library.

Run once per build, then compare the two files.  The base is a parent commit's library as tools/bin/libdsdgp_base.so:

  DSDGP_LIB_PATH=$PWD/tools/bin/libdsdgp_base.so python tools/factor_ab.py --out /tmp/factor_base.npz
  python tools/factor_ab.py --out /tmp/factor_new.npz
  python tools/factor_ab.py --compare /tmp/factor_base.npz /tmp/factor_new.npz --md /tmp/factor_ab.md     (the table of profiles/chol_plan_ab.md)

The file holds
  model.<route>.l<layer>.<matrix>   Lu (white = True models only: the others keep none), Lu^-1, Lu^-T, Ku^-1 read as the kernels left them
                                    (dsdgp_model_layer_matrix, as tests/test_gpu_factor_direct.py reads them) and the layer's KL term, which
                                    carries the factorisation's log-determinant (the library has no accessor for the number itself), on
                                    one small model per route of that file: look-ahead at Mp = 192, 320, 640; a uniform batch of two at 192;
                                    a mixed model (300, 60); look-ahead off at 320; DSDGP_BIG_MP=128 (read once per process: a child
                                    process); white = True (the factor is kept: need_factor); Mp = 1152
  natgrad.M<M>.{q_mu,q_sqrt}        after one dsdgp_model_natgrad_step at M = 192 and 300 (Mp = 192, 320; D_out = 2: both factorisations of
                                    the step in their batched, blocked form) on the `dense` / `quad` inputs of tests/natgrad_cases.py
  potrf.n<n>.b<batch>.{L,info}      dsdgp_potrf at n = 176, 177, 192, 256, 448 with batch 1 and 3
  potrf.fail.{info,rc}              the status of a matrix of order 448 that fails in its third block (pivot 300)
`--compare` exits non-zero unless every array of the two files is equal (np.array_equal, signs of zeros included)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "doubly-stochastic-dgp_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# route -> ([(family, M, kind)], white, environment)
ROUTES = {
    "lookahead192": ([("pairs", 180, "rbf")], False, {}),
    "lookahead320": ([("pairs", 300, "rbf")], False, {}),
    "lookahead640": ([("pairs", 600, "rbf")], False, {}),
    "uniform192x2": ([("spread", 192, "rbf"), ("spread", 192, "matern52")], False, {}),
    "mixed300_60": ([("pairs", 300, "rbf"), ("pairs", 60, "matern52")], False, {}),
    "plain320": ([("pairs", 300, "rbf")], False, {"DSDGP_CHOL_LOOKAHEAD": "0"}),
    "white320": ([("pairs", 300, "rbf")], True, {}),
    "gemm1152": ([("pairs", 1100, "rbf")], False, {}),
}
CHILD_ROUTE = ("single128", ([("pairs", 128, "rbf")], False, {"DSDGP_FORCE": "head=0", "DSDGP_BIG_MP": "128"}))


def model_route(name, layers, white, out):
    from tests import test_gpu_factor_direct as F
    ls = [F.Layer(f, M, k) for f, M, k in layers]
    model = F.build_model(ls, white)
    mats = F.read_matrices(model, len(ls), white, ls[0].jitter)
    eng = model.engine()
    for l, m in enumerate(mats):
        for k, v in m.items():
            out[f"model.{name}.l{l}.{k}"] = v
        out[f"model.{name}.l{l}.kl"] = np.array(eng.layer_kl(l))


def collect_models(out):
    for name, (layers, white, env) in ROUTES.items():
        for k in ("DSDGP_FORCE", "DSDGP_CHOL_LOOKAHEAD"):      # (read when a model is created)
            os.environ.pop(k, None)
        os.environ.update(env)
        model_route(name, layers, white, out)
    for k in ("DSDGP_FORCE", "DSDGP_CHOL_LOOKAHEAD"):
        os.environ.pop(k, None)


def collect_natgrad(out):
    from tests.helpers import kern_spec, make_case
    from tests.natgrad_cases import case_inputs
    N, D_in, D_out = 16, 3, 2
    for M in (192, 300):
        rng = np.random.RandomState(M)
        X, Y, Z = rng.randn(N, D_in), rng.randn(N, D_out), 2.0 * rng.randn(M, D_in)
        model = make_case(X, Y, Z, [kern_spec("rbf", D_in, 1.0, 1.0)], white=False, S=1, seed=M)[2]
        q_mu, q_sqrt, g_mu, g_sqrt = case_inputs("dense", M, D_out, "quad")
        layer = model.layers[0]
        layer.q_mu, layer.q_sqrt = q_mu, q_sqrt
        model._build_likelihood(X, Y, zs=[rng.randn(1, N, D_out)], with_grad=True)
        eng = model.engine()
        torch = eng.ctx.torch
        eng.ctx.sync()
        for p, val in ((layer.q_mu, g_mu), (layer.q_sqrt, g_sqrt)):      # the synthetic gradient, as tests/test_gpu_natgrad_direct.py injects it
            off, cnt = next((o, c) for q, o, c, _ in eng.entries if q is p)
            eng.grad[off:off + cnt].copy_(torch.as_tensor(np.ascontiguousarray(val, dtype=np.float64).ravel()))
        torch.cuda.synchronize()
        eng.natgrad_step(0, 0.1, check=True)
        eng.sync_to_host()
        out[f"natgrad.M{M}.q_mu"], out[f"natgrad.M{M}.q_sqrt"] = np.array(layer.q_mu.value), np.array(layer.q_sqrt.value)


def collect_potrf(out):
    import ctypes as C
    from doubly_stochastic_dgp.engine import Context
    ctx = Context.get()

    def potrf(A, n, batch):
        dA = ctx.to_device(np.ascontiguousarray(A, dtype=np.float64))
        info = C.c_int(-1)
        ctx.torch.cuda.current_stream().synchronize()
        rc = ctx.lib.dsdgp_potrf(ctx.handle, batch, n, C.c_void_p(dA.data_ptr()), n, n * n, C.byref(info))
        ctx.sync()
        return rc, info.value, dA.cpu().numpy()

    for n in (176, 177, 192, 256, 448):
        for batch in (1, 3):
            rng = np.random.RandomState(n + batch)
            A = rng.randn(batch, n, n)
            A = A @ A.transpose(0, 2, 1) + n * np.eye(n)
            rc, info, L = potrf(A, n, batch)
            assert rc == 0, (n, batch, rc, info)
            out[f"potrf.n{n}.b{batch}.L"], out[f"potrf.n{n}.b{batch}.info"] = L, np.array(info)
    rng = np.random.RandomState(448)
    A = rng.randn(448, 448)
    A = A @ A.T + 448 * np.eye(448)
    A[299, 299] = -1.0                      # rows 256 .. 383 are the third 128-block
    rc, info, _ = potrf(A, 448, 1)
    out["potrf.fail.info"], out["potrf.fail.rc"] = np.array(info), np.array(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write this build's arrays to OUT.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--md", default=None, help="with --compare: write the table here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.compare:
        from likelihood_ab import compare          # tools/ is the script's directory
        sys.exit(compare(*args.compare, args.md))
    out = {}
    if args.child:
        name, (layers, white, _) = CHILD_ROUTE
        model_route(name, layers, white, out)
        np.savez(args.child, **out)
        return
    path = args.out or "factor_ab.npz"
    child_path = path + ".child.npz"
    env = dict(os.environ, **CHILD_ROUTE[1][2])
    env.pop("DSDGP_CHOL_LOOKAHEAD", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child_path], cwd=ROOT, env=env, check=True, timeout=600)
    with np.load(child_path) as child:
        out.update({k: child[k] for k in child.files})
    os.remove(child_path)
    collect_models(out)
    collect_natgrad(out)
    collect_potrf(out)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path} (library: {os.environ.get('DSDGP_LIB_PATH', 'in-tree')})")


if __name__ == "__main__":
    main()

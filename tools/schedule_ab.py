#!/usr/bin/env python
"""Bits, launch counts and workspace sizes of the training step on every schedule of the reverse pass, for a before/after comparison of
two library builds (a change of the host-side schedule / split-K plan must leave all of them as they were).

Run once per build (DSDGP_LIB_PATH names the library), then compare the two files:

  DSDGP_LIB_PATH=$PWD/tools/bin/libdsdgp_base.so python tools/schedule_ab.py --out /tmp/sched_base.npz
  python tools/schedule_ab.py --out /tmp/sched_new.npz
  python tools/schedule_ab.py --compare /tmp/sched_base.npz /tmp/sched_new.npz --md /tmp/sched_ab.md

Every case of CASES runs under every setting of SETTINGS (DSDGP_FORCE is read when the device model is created, DSDGP_NO_OVERLAP per
step).  Per (case, setting) the file holds
  out4 / grad        the four result scalars and the whole gradient of one ELBO evaluation with explicit draws
  theta              the parameter vector after three train_steps (cases with a pruned reverse pass: none, train_step refuses them)
  launches           dsdgp_launch_count of the evaluation and of each step
  workspace          dsdgp_model_workspace_bytes of the model
  buckets            (bucket case) the (bucket, offset, count) triples the callback was handed
The cases with draws from a seed or input propagation also hold the arrays of one propagate (prop_*) and, last in `launches`, its count.
The walk and vjp cases hold, per call of their sequence (cNN_<call>_<what>), the result scalars, gradient, theta or propagated arrays, and in
`launches` the launch count of every call: which launches each state of the model leads to.
`--compare` exits non-zero unless every array of the two files is equal (np.array_equal; NaNs in the same places count as equal)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "doubly-stochastic-dgp_amd"))
sys.path.insert(0, ROOT)

# name: (N, D, M, S, L) + options.  n S Mp of "L3.M128.overlap" and "L5.M128.overlap" is 2^18: the default two-stream schedule
CASES = {
    "L2.M20": dict(N=64, D=3, M=20, S=4, L=2),
    "L3.M20": dict(N=100, D=3, M=20, S=3, L=3),
    "L2.M50": dict(N=100, D=4, M=50, S=3, L=2),
    "L3.M50": dict(N=130, D=5, M=50, S=2, L=3),
    "L2.M128": dict(N=200, D=5, M=128, S=2, L=2),
    "L3.M128.overlap": dict(N=512, D=5, M=128, S=4, L=3),
    "L2.Mp192": dict(N=128, D=3, M=180, S=2, L=2),
    "L5.M20": dict(N=96, D=3, M=20, S=2, L=5),
    "L5.M128.overlap": dict(N=512, D=3, M=128, S=4, L=5),
    "L2.wide": dict(N=80, D=40, M=30, S=2, L=2),
    "L2.white": dict(N=64, D=3, M=20, S=4, L=2, white=True),
    "L2.linear_mean": dict(N=90, D=3, M=24, S=3, L=2, DY=2, linear_mean=True),
    "L2.multiclass": dict(N=70, D=3, M=20, S=3, L=2, classes=3),
    "L3.grad_first1": dict(N=100, D=3, M=20, S=3, L=3, grad_first=1),
    "L3.grad_q_only": dict(N=100, D=3, M=20, S=3, L=3, grad_first=1, q_only=True),
    "L3.M50.buckets": dict(N=130, D=5, M=50, S=2, L=3, buckets=True),
    # chain instances the cases above do not reach: the 8-wave fused last layer (S N >= 4 Mp: algebraic assembly), the WIDE instances
    # (D > 64; "L2.wide" is a narrow one) at 4 and 8 waves, and the 32-byte operand order of Mp > 256
    "L2.M256.fused": dict(N=300, D=5, M=256, S=4, L=2),
    "L2.wide65": dict(N=80, D=65, M=30, S=2, L=2),
    "L2.wide65.M128": dict(N=80, D=65, M=128, S=2, L=2),
    "L2.Mp320": dict(N=128, D=3, M=310, S=2, L=2),
    # what a prepare keeps (csrc/prepare_plan.hpp): the walk of tests/test_gpu_prepare_walk.py, bits and launch count of every call
    "L3.M20.walk": dict(N=40, D=3, M=20, S=2, L=3, walk=True),
    # forward-side decisions (csrc/forward_plan.hpp) the cases above leave where they are: input propagation (the concat launch between
    # the layers); draws of every inner layer from a fixed seed (head launch; at M = 180 the side stream, once the streams overlap) or
    # of some layers only (layer 1's from the seed); a saved forward pass and its reverse pass from the caller's adjoints (a second
    # pair at a smaller shape behind the first)
    "L3.prop": dict(N=90, D=2, M=14, S=3, L=3, prop=True),
    "L3.M20.seed": dict(N=100, D=3, M=20, S=3, L=3, draws="seed"),
    "L3.Mp192.seed": dict(N=256, D=3, M=180, S=8, L=3, draws="seed"),
    "L3.M20.some": dict(N=100, D=3, M=20, S=3, L=3, draws="some"),
    "L3.M20.vjp": dict(N=100, D=3, M=20, S=3, L=3, vjp=True),
    "L2.M128.vjp": dict(N=512, D=5, M=128, S=4, L=2, vjp=True, draws="seed"),
}
SETTINGS = {
    "default": {},
    "no_overlap": {"DSDGP_NO_OVERLAP": "1"},
    "overlap_min=0": {"DSDGP_FORCE": "overlap_min=0"},
    "pipe_tail=1": {"DSDGP_FORCE": "overlap_min=0,pipe_tail=1"},
    "wg_red=0": {"DSDGP_FORCE": "wg_red=0"},
    "wg_red=2": {"DSDGP_FORCE": "wg_red=2"},
    "wg_group=0": {"DSDGP_FORCE": "overlap_min=0,wg_group=0"},
    "wg_group=2": {"DSDGP_FORCE": "wg_group=2"},
    "wg_defer=0": {"DSDGP_FORCE": "overlap_min=0,wg_defer=0"},
    "wg_defer=2": {"DSDGP_FORCE": "overlap_min=0,wg_defer=2"},
    "red_ahead=0": {"DSDGP_FORCE": "overlap_min=0,red_ahead=0"},
    "adj_fuse=0": {"DSDGP_FORCE": "adj_fuse=0"},
    "last_fuse=0": {"DSDGP_FORCE": "last_fuse=0"},
    "tail=0": {"DSDGP_FORCE": "tail=0"},
    "head=0": {"DSDGP_FORCE": "head=0"},
    "gemm_mp=16": {"DSDGP_FORCE": "gemm_mp=16"},
    "bwd_split+save_c": {"DSDGP_FORCE": "bwd_split=2,save_c=2,cs_min_blocks=0,cs_min_dout=1"},
    "white_fwd=0": {"DSDGP_FORCE": "white_fwd=0"},
    "lik_fuse=0": {"DSDGP_FORCE": "lik_fuse=0"},
}


def run_walk(eng, X, Y, zs, S):
    """V, G, natgrad(last), G, natgrad(0), V, pruned G from layer 1 (q only), G, propagate, Adam step, V, G at explicit draws"""
    count = eng.lib.dsdgp_launch_count
    res, launches = {}, []
    L = len(eng.layers)

    def call(what, fn):
        i, n0 = len(launches), count()
        got = fn()
        eng.ctx.sync()
        launches.append(count() - n0)
        for k, v in got.items():
            res[f"c{i:02d}_{what}_{k}"] = v

    def ev(with_grad, first=0, q_only=False):
        out4 = eng.elbo(X, Y, S, zs=zs, data_scale=1.0, with_grad=with_grad, grad_from_layer=first, grad_q_only=q_only)
        return {"out4": np.array(out4), **({"grad": eng.grad.cpu().numpy().copy()} if with_grad else {})}

    def theta_after(fn):
        fn()
        eng.ctx.sync()
        return {"theta": eng.theta.cpu().numpy().copy()}

    def prop():
        eng.ctx.sync()
        return {f"{k}{l}": t.cpu().numpy().copy() for k, ts in zip(("F", "mean", "var"), eng.propagate(X, S, zs=zs)) for l, t in enumerate(ts)}

    for what, fn in (("V", lambda: ev(False)), ("G", lambda: ev(True)), ("natgrad_last", lambda: theta_after(lambda: eng.natgrad_step(L - 1, 0.005))),
                     ("G", lambda: ev(True)), ("natgrad_0", lambda: theta_after(lambda: eng.natgrad_step(0, 0.005))), ("V", lambda: ev(False)),
                     ("Gq1", lambda: ev(True, 1, True)), ("G", lambda: ev(True)), ("propagate", prop),
                     ("adam", lambda: theta_after(lambda: eng.adam_step(lr=0.01))), ("V", lambda: ev(False)), ("G", lambda: ev(True))):
        call(what, fn)
    res["launches"] = np.array(launches, dtype=np.int64)
    res["workspace"] = np.array([eng.workspace.numel() - 256])
    return res


def run_vjp(eng, X, Y, zs, S, seed):
    """a gradient evaluation; a saved forward pass and its reverse pass from the caller's adjoints; the pair again on the first
    half of the rows and one sample less, draws from the seed; a gradient evaluation: results and launch count of every call"""
    count = eng.lib.dsdgp_launch_count
    rng = np.random.RandomState(3)
    res, launches = {}, []
    DY = Y.shape[1]

    def call(what, fn):
        i, n0 = len(launches), count()
        got = fn()
        eng.ctx.sync()
        launches.append(count() - n0)
        for k, v in got.items():
            res[f"c{i:02d}_{what}_{k}"] = v

    def grad():
        out4 = eng.elbo(X, Y, S, zs=zs, seed=seed, data_scale=5.0, with_grad=True)
        return {"out4": np.array(out4), "grad": eng.grad.cpu().numpy().copy()}

    def pair(Xp, Sp, zp):
        got = {}

        def fwd():
            got["mean"], got["var"] = eng.forward_saved(Xp, Sp, zs=zp, seed=seed)
            return {k: v.cpu().numpy().copy() for k, v in got.items()}

        def bwd():
            out4 = eng.backward_adjoints(rng.randn(Sp, Xp.shape[0], DY), rng.randn(Sp, Xp.shape[0], DY))
            return {"out4": np.array(out4), "grad": eng.grad.cpu().numpy().copy()}

        return fwd, bwd

    h = X.shape[0] // 2
    f1, b1 = pair(X, S, zs)
    f2, b2 = pair(X[:h], S - 1, None)
    for what, fn in (("G", grad), ("saved", f1), ("adjoints", b1), ("saved_small", f2), ("adjoints_small", b2), ("G", grad)):
        call(what, fn)
    res["launches"] = np.array(launches, dtype=np.int64)
    res["workspace"] = np.array([eng.workspace.numel() - 256])
    return res


def run_case(c):
    """arrays of one case under the environment as it stands"""
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Linear, Matern52, MultiClass
    N, D, M, S, L = c["N"], c["D"], c["M"], c["S"], c["L"]
    DY = c.get("DY", 1)
    rng = np.random.RandomState(11)
    X = rng.randn(N, D)
    Z = X[:M] + 0.01 * rng.randn(M, D) if M <= N else rng.randn(M, D)
    classes = c.get("classes")
    Y = rng.randint(0, classes, size=(N, 1)).astype(np.float64) if classes else rng.randn(N, DY)
    kernels = [(RBF if l % 2 == 0 else Matern52)(D, variance=1.0 + 0.1 * l, lengthscales=0.9) for l in range(L)]
    kw = {}
    if c.get("linear_mean"):
        kw["mean_function"] = Linear(0.3 * rng.randn(D, DY), 0.5 * rng.randn(DY))
    if c.get("prop"):      # every inner layer forwards the D inputs beside its own outputs (widths D + 3, D + 2)
        from doubly_stochastic_dgp.dgp import DGP_Base
        from doubly_stochastic_dgp.layer_initializations import init_layers_input_prop
        kernels = [RBF(D, variance=1.3, lengthscales=0.9), Matern52(D + 3, variance=0.8, lengthscales=1.4), RBF(D + 2, variance=1.1, lengthscales=1.2)]
        np.random.seed(5)      # the inducing inputs of the propagated columns come from numpy's global generator
        model = DGP_Base(X, Y, Gaussian(variance=0.2), init_layers_input_prop(X, Y, Z, kernels), num_samples=S, num_data=5 * N)
    else:
        model = DGP(X, Y, Z, kernels, MultiClass(classes) if classes else Gaussian(variance=0.2), white=bool(c.get("white")),
                    num_outputs=classes, num_samples=S, num_data=5 * N, **kw)
    for layer in model.layers:
        layer.q_mu = 0.3 * rng.randn(*layer.q_mu.shape)
        q = np.asarray(layer.q_sqrt.value)
        layer.q_sqrt = q * 0.7 + 0.05 * np.tril(rng.randn(*q.shape))
        if c.get("walk"):      # well-conditioned, so that the natural-gradient step on an inner layer is not refused
            layer.q_sqrt = 0.7 * np.tile(np.eye(q.shape[1]), (q.shape[0], 1, 1)) + np.tril(rng.randn(*q.shape)) / q.shape[1]
    zs = [rng.randn(S, N, layer.num_outputs) for layer in model.layers]
    if c.get("draws") == "seed":
        zs = None
    elif c.get("draws") == "some":
        zs[1] = None
    seed = 4242      # fixed: what zs leaves open is drawn from it, the same numbers in both builds
    eng = model.engine()
    if c.get("walk"):
        return run_walk(eng, X, Y, zs, S)
    if c.get("vjp"):
        return run_vjp(eng, X, Y, zs, S, seed)
    handed = []
    if c.get("buckets"):
        def on_bucket(user, bucket, ptr, count, stream):      # no exchange: the step's own results must not depend on the callback
            handed.append((bucket, (ptr - eng.gradbuf.data_ptr()) // 8, count))
        cb = _lib.BUCKET_FN(on_bucket)
        eng._bucket_cb = cb      # keep the thunk alive
        eng._post_create = [lambda e: _lib.check(e.lib.dsdgp_model_set_bucket_callback(e.model, C.cast(cb, C.c_void_p), None))]
        eng._post_create[0](eng)      # the device model exists since Engine(): install now, the hook re-installs after a re-creation
    count = eng.lib.dsdgp_launch_count
    launches = [count()]
    out4 = eng.elbo(X, Y, S, zs=zs, seed=seed, data_scale=5.0, with_grad=True, grad_from_layer=c.get("grad_first", 0),
                    grad_q_only=bool(c.get("q_only")))
    launches.append(count())
    res = {"out4": np.array(out4), "grad": eng.grad.cpu().numpy().copy(), "workspace": np.array([eng.workspace.numel() - 256])}
    if c.get("buckets"):
        res["buckets"] = np.array(handed, dtype=np.int64)
    if not c.get("grad_first"):
        for _ in range(3):
            eng.train_step(X, Y, S, zs=zs, seed=seed, data_scale=5.0, lr=0.01)
            eng.ctx.sync()
            launches.append(count())
        res["theta"] = eng.theta.cpu().numpy().copy()
        res["out4_step3"] = eng.out4.cpu().numpy().copy()
    res["launches"] = np.diff(np.array(launches, dtype=np.int64))
    if c.get("prop") or c.get("draws"):      # the forward-only plan of the same model: every layer's sample, mean and variance
        n0 = count()
        for k, ts in zip(("F", "mean", "var"), eng.propagate(X, S, zs=zs, seed=seed)):
            for l, t in enumerate(ts):
                res[f"prop_{k}{l}"] = t.cpu().numpy().copy()
        res["launches"] = np.append(res["launches"], count() - n0)
    return res


def collect(only):
    out = {}
    for sname, env in SETTINGS.items():
        for cname, c in CASES.items():
            if only and only not in f"{cname}@{sname}":
                continue
            saved = {k: os.environ.pop(k, None) for k in ("DSDGP_FORCE", "DSDGP_NO_OVERLAP")}
            os.environ.update(env)
            t0 = time.time()
            try:
                for k, v in run_case(c).items():
                    out[f"{cname}@{sname}.{k}"] = v
            except Exception as err:      # a refusal (a forced variant that a shape has no instance for) must be the same refusal in both builds
                if "hip" in str(err).lower():      # a device error is no refusal: stop here, start nothing more on the GPU
                    raise
                out[f"{cname}@{sname}.error"] = np.array(f"{type(err).__name__}: {err}")
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            print(f"{cname}@{sname}: {time.time() - t0:.2f} s", flush=True)
    return out


def compare(a_path, b_path, md):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    rows = {}
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and (
            np.array_equal(a[k], b[k]) if a[k].dtype.kind != "f" else
            np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(np.signbit(a[k]), np.signbit(b[k])))
        case, kind = k.rsplit(".", 1)
        rows.setdefault(case, []).append((kind, same, a[k]))
        if not same:
            bad.append(k)
    lines = ["| case @ setting | arrays | launches (evaluation, steps) | workspace bytes | all finite | equal bits |", "|---|---|---|---|---|---|"]
    for case, items in rows.items():
        d = {kind: arr for kind, _, arr in items}
        finite = all(np.isfinite(arr).all() for kind, _, arr in items if arr.dtype.kind == "f")
        if "error" in d:
            lines.append(f"| {case} | refused: {str(d['error'])[:80]} | | | | {'yes' if all(s for _, s, _ in items) else 'NO'} |")
            continue
        lines.append(f"| {case} | {len(items)} | {' '.join(map(str, d['launches']))} | {int(d['workspace'][0])} | {'yes' if finite else 'NO'} | "
                     f"{'yes' if all(s for _, s, _ in items) else 'NO'} |")
    text = "\n".join(lines) + f"\n\n{len(a.files)} arrays in {len(rows)} (case, setting) pairs, {len(bad)} differ" + (f": {bad}" if bad else "") + "\n"
    print(text)
    if md:
        with open(md, "w") as f:
            f.write(text)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write this build's arrays to OUT.npz")
    ap.add_argument("--only", default=None, help="run only the (case@setting) pairs whose name contains this")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--md", default=None, help="with --compare: write the table here")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.md))
    arrays = collect(args.only)
    np.savez(args.out or "schedule_ab.npz", **arrays)
    print(f"{len(arrays)} arrays -> {args.out or 'schedule_ab.npz'} (library: {os.environ.get('DSDGP_LIB_PATH', 'in-tree')})")


if __name__ == "__main__":
    main()

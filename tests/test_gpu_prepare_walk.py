"""What a prepare keeps (csrc/prepare_plan.hpp: the reuse rules under dsdgp_model_track_theta) must not change a bit of any result.
Two identical models run the same walk through every kind of state the rules tell apart — forward-only and gradient evaluations at
unchanged parameters, natural-gradient steps on one layer and then on a second, a pruned (q_mu, q_sqrt)-only reverse pass followed by
a full one, propagate, an Adam step — with explicit draws.  One of the two reports a (fictitious) write to theta before every call and
therefore recomputes everything every time: every call's results must be bitwise equal between the two.

Shapes: the smallest that reach each factorisation route (N = 40, D = 3, S = 2, L = 3): the head launch, the one-workgroup batch
(DSDGP_FORCE=head=0), the batched blocked factorisation (M = 180, Mp = 192) and a white = True model."""
import numpy as np
import pytest

from tests.helpers import kern_spec, make_case

pytestmark = pytest.mark.gpu

N, D, S, L = 40, 3, 2, 3
GAMMA, LR = 0.005, 0.01


def _walk(model, X, Y, zs, refactor, white):
    """the results of every call, in order: (what, arrays...)"""
    from doubly_stochastic_dgp import _lib
    eng = model.engine()
    q_entries = [(off, cnt) for l, layer in enumerate(model.layers) if l >= 1
                 for p, off, cnt, _ in eng.entries if p is layer.q_mu or p is layer.q_sqrt]
    seen = []

    def before():
        if refactor:
            eng._upload_if_needed()
            _lib.check(eng.lib.dsdgp_model_theta_changed(eng.model))

    def theta():
        eng.ctx.sync()
        return eng.theta.cpu().numpy().copy()

    def V():
        before()
        seen.append(("V", eng.elbo(X, Y, S, zs=zs, data_scale=1.0).copy()))

    def G(first=0, q_only=False):
        before()
        out4 = eng.elbo(X, Y, S, zs=zs, data_scale=1.0, with_grad=True, grad_from_layer=first, grad_q_only=q_only).copy()
        g = eng.grad.cpu().numpy().copy()
        if (first or q_only) and not white:      # a pruned pass produces the (q_mu, q_sqrt) entries of the layers >= first and nothing
            # else (white = True: the restriction does not apply, the pass is a full one)
            g = np.concatenate([g[off:off + cnt] for off, cnt in q_entries])
        seen.append(("G", out4, g))

    def natgrad(l):
        before()
        eng.natgrad_step(l, GAMMA)
        seen.append(("natgrad", theta()))

    def propagate():
        before()
        Fs, means, vars_ = eng.propagate(X, S, zs=zs)
        eng.ctx.sync()
        seen.append(("propagate", *[t.cpu().numpy().copy() for t in (*Fs, *means, *vars_)]))

    def adam():
        before()
        eng.adam_step(lr=LR)
        seen.append(("adam", theta()))

    V(); G(); natgrad(L - 1); G(); natgrad(0); V(); G(first=1, q_only=True); G(); propagate(); adam(); V(); G()
    return seen


@pytest.mark.parametrize("M,force,white", [(20, None, False), (20, "head=0", False), (180, None, False), (20, None, True)],
                         ids=["head", "one_workgroup_batch", "batched_blocked", "white"])
def test_walk_is_bitwise_equal_to_recomputing_everything(M, force, white, monkeypatch):
    if force:      # DSDGP_FORCE is read when the device model is created
        monkeypatch.setenv("DSDGP_FORCE", force)
    else:
        monkeypatch.delenv("DSDGP_FORCE", raising=False)
    rng = np.random.RandomState(31)
    X, Y = rng.randn(N, D), rng.randn(N, 2)
    Z = X[:M] + 0.01 * rng.randn(M, D) if M <= N else 3.0 * rng.randn(M, D)
    specs = [kern_spec("rbf", D, 1.1, 0.9), kern_spec("matern52", D, 0.8, 1.2), kern_spec("rbf", D, 0.9, 1.0)]
    zs = [rng.randn(S, N, D), rng.randn(S, N, D), rng.randn(S, N, 2)]
    # A natural-gradient step on an INNER layer is refused unless A = S^-1 + 2 gamma Sbar stays positive definite, and the data term is
    # not convex in that layer's S: a well-conditioned q_sqrt (0.7 I + noise / M), unit likelihood variance and data scale keep the
    # smallest eigenvalue of A above 1 at this gamma on every layer (oracle, float64: 1.1 .. 1.7 at M = 20 and M = 180)
    q = [(0.3 * rng.randn(M, d), 0.7 * np.tile(np.eye(M), (d, 1, 1)) + np.tril(rng.randn(d, M, M)) / M) for d in (D, D, 2)]
    walks = []
    for refactor in (False, True):
        _, _, model = make_case(X, Y, Z, specs, white=white, S=S, lik_var=1.0)
        for layer, (q_mu, q_sqrt) in zip(model.layers, q):
            layer.q_mu, layer.q_sqrt = q_mu, q_sqrt
        walks.append(_walk(model, X, Y, zs, refactor, white))
    kept, redone = walks
    assert [c[0] for c in kept] == [c[0] for c in redone] and len(kept) == 12
    for i, (a, b) in enumerate(zip(kept, redone)):
        for x, y in zip(a[1:], b[1:]):
            assert np.all(np.isfinite(x)), (i, a[0])
            assert np.array_equal(x, y), (i, a[0], float(np.max(np.abs(x - y))))

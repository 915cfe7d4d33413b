"""-m gpu: grouped weight-gradient tasks (WgradJob::ng, wgrad.hip).  A layer's D_out symmetric products P_d = sum_r vbar_d,r a_r a_r^T
share the operand A; grouped tasks form up to four of them per 32 x 32 tile from one load of each A fragment.  Every element must be
summed exactly as by the one-result 64 x 64 tasks (same K splits, same quarter of a split per wave, same k order, same LDS tree, same
partials), so DSDGP_FORCE=wg_group=0 (one-result tasks only), the default (grouped at Mp <= 128 from D_out = 3) and wg_group=2 (grouped at every
D_out, D_out = 1 included) must give the same bits for the ELBO terms, the gradient and the parameters after Adam steps — under each
split-K reduction form (wg_red=0: k_reduce_grouped; 2: the ticketed in-launch reduction, whose jobs keep one-result tasks; default).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, D = hidden width = D_out of the hidden layers, M, S, minibatch): the last layer has D_out = 1
SHAPES = {
    "cfg2": (7372, 8, 128, 20, 1000),            # the headline shape: 20 000 rows per hidden layer, Mp = 128, 23 K splits
    "dout3": (3000, 3, 128, 20, 1000),            # D_out = 3: one group of three
    "ragged_mp256": (2500, 8, 256, 7, 777),       # 5 439 rows (not a multiple of 16), Mp = 256 (4 x 4 64-tiles)
}


def _run(monkeypatch, shape, force, steps=3):
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    if force:
        monkeypatch.setenv("DSDGP_FORCE", force)      # read when the device model is created
    else:
        monkeypatch.delenv("DSDGP_FORCE", raising=False)
    n, D, M, S, mb = SHAPES[shape]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, D))
    Y = rng.standard_normal((n, 1))
    Z = X[rng.permutation(n)[:M]] + 0.01 * rng.standard_normal((M, D))
    model = DGP(X, Y, Z, [RBF(D) for _ in range(3)], Gaussian(), num_samples=S, minibatch_size=mb)
    for layer in model.layers[:-1]:
        layer.q_sqrt = layer.q_sqrt.value * 1e-5
    for _ in range(steps):
        model.train_step(0.01)
    model.train_step(0.01, sync=True)
    eng = model.engine()
    eng.ctx.sync()
    return [t.detach().cpu().numpy().astype(np.float64).copy() for t in (eng.out4, eng.grad, eng.theta)]


@pytest.mark.parametrize("red", ["", "wg_red=0", "wg_red=2"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_grouped_wgrad_tasks_are_bitwise_neutral(monkeypatch, shape, red):
    join = lambda *a: ",".join(x for x in a if x)
    ref = _run(monkeypatch, shape, join("wg_group=0", red))
    assert all(np.all(np.isfinite(a)) for a in ref)
    for force in (red, join("wg_group=2", red)):
        got = _run(monkeypatch, shape, force)
        for name, a, b in zip(("elbo_terms", "grad", "theta"), ref, got):
            assert np.array_equal(a, b), (shape, force, name, float(np.max(np.abs(a - b))))

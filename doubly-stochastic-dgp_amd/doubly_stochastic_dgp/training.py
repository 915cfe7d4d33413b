"""[UPSTREAM] gpflow.training.AdamOptimizer mirror: `AdamOptimizer(0.01).minimize(model, maxiter=K)`
(demos/demo_regression_UCI.ipynb:324).  The step itself (gradient + Adam update) runs in libdsdgp."""


class AdamOptimizer:
    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta1, beta2, epsilon

    def minimize(self, model, maxiter=1000):
        if not getattr(model, "supports_gradients", True):
            raise NotImplementedError(f"{type(model).__name__} builds no reverse pass: there is no gradient to step along")
        n = int(maxiter)
        for it in range(n):
            # steps are asynchronous; the last one synchronises and surfaces a failed Kuu factorisation (CholeskyError)
            model.train_step(self.lr, self.b1, self.b2, self.eps, sync=(it == n - 1))


class NatGradOptimizer:
    """[UPSTREAM] gpflow.training.NatGradOptimizer(gamma): natural-gradient steps on chosen layers' (q_mu, q_sqrt)
    (demos/demo_regression_UCI.ipynb:360-366, using_natural_gradients.ipynb:139-145, tests/test_collapsed.py:100).
    `var_list` is a list of [q_mu, q_sqrt] Parameter pairs, as in the reference."""

    def __init__(self, gamma):
        self.gamma = float(gamma)

    def _layer_indices(self, model, var_list):
        idx = []
        for pair in var_list:
            ids = {id(p) for p in pair}
            hit = [i for i, layer in enumerate(model.layers) if {id(layer.q_mu), id(layer.q_sqrt)} == ids]
            if len(hit) != 1:
                raise ValueError("each var_list entry must be the [q_mu, q_sqrt] pair of one layer of the model")
            idx.append(hit[0])
        return idx

    def minimize(self, model, var_list, maxiter=1, X=None, Y=None, zs=None):
        if not getattr(model, "supports_gradients", True):
            raise NotImplementedError(f"{type(model).__name__} builds no reverse pass: there is no gradient to step along")
        layers = self._layer_indices(model, var_list)
        eng = model.engine()
        for _ in range(int(maxiter)):
            # tf.gradients w.r.t. var_list only: the reverse pass stops below the lowest layer in it, and — var_list holding nothing
            # but (q_mu, q_sqrt) pairs — it never visits that layer's Kuf / Kuu adjoints (they feed Z and the kernel hyper-parameters)
            model._build_likelihood(X, Y, zs=zs, with_grad=True, grad_from_layer=min(layers), grad_q_only=True)
            for l in layers:
                eng.natgrad_step(l, self.gamma)
        eng.ctx.sync()


class ScipyOptimizer:
    """[UPSTREAM] gpflow.training.ScipyOptimizer mirror: `ScipyOptimizer().minimize(m)` as the reference's tests and demos fit their
    collapsed baselines (tests/test_collapsed.py:10, tests/test_dgp.py:150).  For a `DGP_Collapsed` it MAXIMISES the bound over the trainable ones among the
    parameters the collapsed last layer owns — `feature.Z`, `kern.variance`, `kern.lengthscales` — and the likelihood's `variance`,
    with the gradients of `DGP_Collapsed.compute_log_likelihood_gradients` (device) and scipy.optimize.minimize on the host.  The inner
    layers are held fixed.  The search runs in unconstrained space: a positive parameter theta = softplus(x) + 1e-6 (gpflow_compat),
    d theta / dx = 1 - exp(-(theta - 1e-6)).  Values go back through `Parameter.assign`, so models that share layers stay coherent.
    A factorisation that fails inside the line search (CholeskyError) is a step back, not an exception: that trial point reports an
    objective well above the last one that succeeded, `f + 10 (|f| + 1)`, with a zero gradient.  (Not +inf: the interpolation of
    scipy's L-BFGS-B line search turns an infinite or a huge trial value into a step of zero length and then reports convergence at
    the point it started from; tests/test_psi_grad_reference_cpu.py shows the finite value recovering.)  A failure at the starting
    point itself is raised: there is nothing to step back to.
    Any other model: NotImplementedError.  `options`: further entries of scipy's options dict (`maxiter` is minimize's argument)."""

    def __init__(self, method="L-BFGS-B", tol=None, options=None):
        self.method, self.tol, self.options = method, tol, dict(options or {})

    def minimize(self, model, maxiter=1000, zs=None):
        """returns scipy's OptimizeResult (`fun` = minus the bound); zs: fixed draws for the inner layers, as compute_log_likelihood"""
        import numpy as np
        import scipy.optimize
        from ._lib import CholeskyError
        from .gpflow_compat import SOFTPLUS_LOWER, positive_backward, positive_forward, split_kernel
        from .model_zoo import DGP_Collapsed
        if not isinstance(model, DGP_Collapsed):
            raise NotImplementedError(f"ScipyOptimizer fits the collapsed last layer of a DGP_Collapsed; {type(model).__name__} is "
                                      "trained by AdamOptimizer / NatGradOptimizer")
        top = model.layers[-1]
        params = [top.feature.Z, split_kernel(top.kern)[0].variance, split_kernel(top.kern)[0].lengthscales,
                  model.likelihood.likelihood.variance]
        train = [p for p in params if p.trainable]
        if not train:
            raise ValueError("ScipyOptimizer: none of the collapsed layer's parameters is trainable")
        sizes = [int(np.prod(p.shape)) for p in train]

        def pack(values):
            return np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in values])

        def assign(x):
            at = 0
            for p, k in zip(train, sizes):
                v = x[at:at + k].reshape(p.shape)
                p.assign(positive_forward(v) if p.transform == "positive" else v)
                at += k

        last = [None]                                 # the last objective that succeeded

        def objective(x):
            assign(x)
            try:
                bound, pairs, _ = model.compute_log_likelihood_gradients(zs=zs)
            except CholeskyError:
                if last[0] is None:
                    raise
                return last[0] + 10.0 * (abs(last[0]) + 1.0), np.zeros_like(x)
            last[0] = -float(bound)
            grads = {id(p): g for p, g in pairs}
            out = []
            for p in train:
                g = grads[id(p)]
                if p.transform == "positive":
                    g = g * -np.expm1(-(p.value - SOFTPLUS_LOWER))
                out.append(-g)
            return -float(bound), pack(out)

        x0 = pack([positive_backward(p.value) if p.transform == "positive" else p.value for p in train])
        options = dict(self.options)
        options["maxiter"] = int(maxiter)
        res = scipy.optimize.minimize(objective, x0, jac=True, method=self.method, tol=self.tol, options=options)
        assign(res.x)
        return res

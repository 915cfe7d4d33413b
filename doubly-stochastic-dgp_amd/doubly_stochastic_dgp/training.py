"""[UPSTREAM] gpflow.training.AdamOptimizer mirror: `AdamOptimizer(0.01).minimize(model, maxiter=K)`
(demos/demo_regression_UCI.ipynb:324).  The step itself (gradient + Adam update) runs in libdsdgp."""
import numpy as np

from .gpflow_compat import positive_backward, positive_forward, positive_slope

_NO_SAMPLED_GRADIENT = ("{} takes no minibatch step of a sampled bound: there is no reverse pass of one to step along (a DGP_Collapsed "
                        "trains on its own bound: ScipyOptimizer(inner=True), CollapsedAdamOptimizer)")


class Variables:
    """A list of Parameters seen as unconstrained variables, in list order: a positive Parameter theta = softplus(x) + 1e-6
    (gpflow_compat) moves as x with d theta / dx = 1 - exp(-(theta - 1e-6)), any other as itself.  masks: per Parameter a boolean array
    of the entries that are variables (the lower triangle of a `tril` q_sqrt) or None for all of them; a masked Parameter's values
    travel as the 1-d array of its masked entries, and the others are set to zero.  who: the trainer named in the errors."""

    def __init__(self, params, masks=None, who="Variables"):
        self.params, self.who = list(params), who
        self.masks = list(masks) if masks is not None else [None] * len(self.params)

    def values(self):
        """the current unconstrained values, one array per Parameter"""
        xs = [positive_backward(p.value) if p.transform == "positive" else p.value for p in self.params]
        return [x if m is None else x[m] for m, x in zip(self.masks, xs)]

    def constrained(self, xs):
        """the Parameters' values at the unconstrained values xs (fresh arrays)"""
        out = []
        for p, m, x in zip(self.params, self.masks, xs):
            if m is not None:
                x, masked = np.zeros(p.shape), x
                x[m] = masked
            out.append(positive_forward(x) if p.transform == "positive" else np.array(x, dtype=np.float64))
        return out

    def assign(self, xs):
        for p, v in zip(self.params, self.constrained(xs)):
            p.assign(v)

    def chain(self, pairs):
        """the gradients [(Parameter, dF / d theta), ...] as dF / dx per variable, at the Parameters' current values"""
        grads = {id(p): g for p, g in pairs}
        out = []
        for p, m in zip(self.params, self.masks):
            if id(p) not in grads:
                raise ValueError(f"{self.who}: a Parameter of var_list has no gradient of the model's log density")
            g = np.asarray(grads[id(p)], dtype=np.float64).reshape(p.shape)
            g = g * positive_slope(p.value) if p.transform == "positive" else g
            out.append(g if m is None else g[m])
        return out

    @staticmethod
    def flat(xs):
        return np.concatenate([np.ravel(x) for x in xs])

    def cut(self, flat):
        """a flat vector (numpy or a device tensor) in variable order as one piece per Parameter"""
        out, at = [], 0
        for p, m in zip(self.params, self.masks):
            k = int(np.prod(p.shape) if m is None else np.count_nonzero(m))
            out.append(flat[at:at + k].reshape(p.shape) if m is None else flat[at:at + k])
            at += k
        return out


class AdamOptimizer:
    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta1, beta2, epsilon

    def minimize(self, model, maxiter=1000):
        if not getattr(model, "supports_gradients", True):
            raise NotImplementedError(_NO_SAMPLED_GRADIENT.format(type(model).__name__))
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
            raise NotImplementedError(_NO_SAMPLED_GRADIENT.format(type(model).__name__))
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
    A GPR_Layer on top has no inducing inputs: its variables are the kernel's `variance` and `lengthscales`, a White part's `variance`
    and the likelihood's `variance` (`DGP_Collapsed.top_parameters`).  For a `DGP_Heinonen` the objective is `compute_log_density` (MAP:
    the prior of the inner layer's latents included), with `layers[0].q_mu` among the variables.
    Any other model: NotImplementedError.  `options`: further entries of scipy's options dict (`maxiter` is minimize's argument)."""

    def __init__(self, method="L-BFGS-B", tol=None, options=None):
        self.method, self.tol, self.options = method, tol, dict(options or {})

    def minimize(self, model, maxiter=1000, zs=None, inner=False):
        """returns scipy's OptimizeResult (`fun` = minus the bound); zs: fixed draws for the inner layers, as compute_log_likelihood.
        inner=True: the search is over the trainable parameters of ALL layers — the four above, then `DGP_Collapsed.inner_parameters()`
        — with the gradients of `compute_log_likelihood_gradients(inner=True)`; of a `q_sqrt` only the lower triangle is a variable."""
        import scipy.optimize
        from ._lib import CholeskyError
        from .model_zoo import DGP_Collapsed
        if not isinstance(model, DGP_Collapsed):
            raise NotImplementedError(f"ScipyOptimizer fits the collapsed last layer of a DGP_Collapsed; {type(model).__name__} is "
                                      "trained by AdamOptimizer / NatGradOptimizer")
        from .model_zoo import DGP_Heinonen
        variables = Variables(*_collapsed_variables(model, inner), who="ScipyOptimizer")
        if not variables.params:
            raise ValueError("ScipyOptimizer: none of the collapsed layer's parameters is trainable" if not inner else
                             "ScipyOptimizer: none of the model's parameters is trainable")
        kw = {"inner": True} if inner else {}
        if isinstance(model, DGP_Heinonen) or (inner and getattr(model, "_sgpmc", False)):
            # MAP: the log density (the prior of q_mu included), q_mu among the variables
            gradients = lambda: model.compute_log_density_gradients() + (None,)
        else:
            gradients = lambda: model.compute_log_likelihood_gradients(zs=zs, **kw)

        last = [None]                                 # the last objective that succeeded

        def objective(x):
            variables.assign(variables.cut(x))
            try:
                bound, pairs, _ = gradients()
            except CholeskyError:
                if last[0] is None:
                    raise
                return last[0] + 10.0 * (abs(last[0]) + 1.0), np.zeros_like(x)
            last[0] = -float(bound)
            return -float(bound), -variables.flat(variables.chain(pairs))

        x0 = variables.flat(variables.values())
        options = dict(self.options)
        options["maxiter"] = int(maxiter)
        res = scipy.optimize.minimize(objective, x0, jac=True, method=self.method, tol=self.tol, options=options)
        variables.assign(variables.cut(res.x))
        return res


def _collapsed_variables(model, inner):
    """(the trainable Parameters a collapsed model is fitted over, a boolean mask per Parameter of the entries that are variables):
    the collapsed layer's `feature.Z`, kernel `variance` and `lengthscales` and the likelihood's `variance`; with `inner` the inner
    layers' as well.  Every entry is a variable, except above the diagonal of a `q_sqrt` (transform "tril").  What training.Variables takes."""
    from .model_zoo import DGP_Heinonen
    # DGP_Collapsed.top_parameters: an SGPR_Layer's four as above; a GPR_Layer has no inducing inputs and may have a White variance
    params = [p for p, _ in model.top_parameters()]
    if isinstance(model, DGP_Heinonen):
        params = [model.layers[0].q_mu] + params         # the inner layer's latents: always among the variables
    elif inner:
        params += model.inner_parameters()
    train = [p for p in params if p.trainable]
    free = [np.broadcast_to(np.tril(np.ones(p.shape[-2:], dtype=bool)), p.shape) if p.transform == "tril" else np.ones(p.shape, dtype=bool)
            for p in train]
    return train, free


class CollapsedAdamOptimizer:
    """Full-batch Adam ascent on the bound of a `DGP_Collapsed` over the trainable parameters of all its layers, with the gradient of
    `compute_log_likelihood_gradients(inner=True)` — tf.train.AdamOptimizer's rule (m, v, the bias-corrected step size
    lr sqrt(1 - beta2^t) / (1 - beta1^t), the step lr_t m / (sqrt(v) + epsilon)) in unconstrained space.
    The inner layers' parameters are stepped on the device, by dsdgp_model_adam_step on the inner engine's own parameter vector, moments
    and the gradient the reverse pass left there.  The collapsed layer's four — `feature.Z`, kernel `variance` and `lengthscales`, the
    likelihood's `variance` — are stepped by the same rule on the host and assigned through `Parameter.assign`.  The likelihood's
    variance is the host's: its entry of the inner engine's gradient is zero, so the device does not move its copy, which is
    overwritten from the host with the next upload.
    What moves per step: the adjoints stay on the device; the four host gradients and the bound come down (a few hundred bytes plus
    Z's M x D); the engine's parameter vector comes down once (`sync_to_host`, because the host assignment below reads the current
    values) and goes up once (`mark_host_dirty` by the likelihood variance's assignment, which the inner engine also owns) — n_theta
    doubles each way.  That is the existing coherence machinery, unchanged; it is small beside the N x M work of a step."""

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta1, beta2, epsilon

    def minimize(self, model, maxiter=1000, zs=None):
        """returns the bound at the last evaluated point (before the last step); zs as for compute_log_likelihood"""
        from .model_zoo import DGP_Collapsed, DGP_Heinonen
        if not isinstance(model, DGP_Collapsed):
            raise NotImplementedError(f"CollapsedAdamOptimizer trains a DGP_Collapsed; {type(model).__name__} is trained by AdamOptimizer")
        if getattr(model, "_sgpmc", False):
            raise NotImplementedError("CollapsedAdamOptimizer steps the inner layers through their engine, which a model over an "
                                      "SGPMC_Layer does not have: sample it with HMC or fit it with ScipyOptimizer(inner=True) (MAP)")
        if isinstance(model, DGP_Heinonen):
            raise NotImplementedError("CollapsedAdamOptimizer steps the inner layers through their engine, which a DGP_Heinonen does not "
                                      "have: sample it with HMC or fit it with ScipyOptimizer (MAP)")
        top4 = Variables(_collapsed_variables(model, False)[0], who="CollapsedAdamOptimizer")
        deep = len(model.layers) > 1
        # moments and step count of the four live with the model, as the engine's do with the engine: a second call goes on (TF's slots)
        state = getattr(model, "_collapsed_adam", None)
        if state is None:
            state = {"t": 0}
            object.__setattr__(model, "_collapsed_adam", state)
        bound = None
        for _ in range(int(maxiter)):
            bound, pairs, _adj = model.compute_log_likelihood_gradients(zs=zs, inner=True)
            if deep:
                model.inner_engine().adam_step(self.lr, self.b1, self.b2, self.eps)
            state["t"] += 1
            lr_t = self.lr * np.sqrt(1.0 - self.b2 ** state["t"]) / (1.0 - self.b1 ** state["t"])
            xs = []
            for p, g, x in zip(top4.params, top4.chain(pairs), top4.values()):
                g = -g                                                                  # d(-bound)/dx
                m, v = state.setdefault(id(p), (np.zeros(p.shape), np.zeros(p.shape)))
                m[...] = self.b1 * m + (1.0 - self.b1) * g
                v[...] = self.b2 * v + (1.0 - self.b2) * g * g
                xs.append(x - lr_t * m / (np.sqrt(v) + self.eps))
            top4.assign(xs)
        if deep and bound is not None:
            model.inner_engine().prepare()      # the last host step reaches the device; a failed factorisation there is raised here
        return bound


class HMC:
    """[UPSTREAM] gpflow.train.HMC mirror: Hamiltonian Monte Carlo on `model.compute_log_density()` of a `DGP_Heinonen`, the way the
    reference's model is built to be used (model_zoo.py:60-88).  The variables are `var_list`, by default `[model.layers[0].q_mu]`; any
    Parameter among the pairs of `compute_log_likelihood_gradients` may be added (the top kernel's, the likelihood's variance).  A
    positive parameter moves in unconstrained space, theta = softplus(x) + 1e-6 (gpflow_compat).  Only `q_mu` has a prior (standard
    normal, part of compute_log_density); a parameter without a prior has a FLAT density in the space it moves in — unconstrained space
    for a positive one: no prior and no Jacobian term is added for it.
    Leapfrog integration with unit mass: positions and momenta are device tensors updated by torch operations, and every step costs one
    `compute_log_likelihood_gradients` (the model's Parameters are assigned at every position, which is how the gradient sees it).
    Randomness, so that a run can be replayed: the momenta of iteration i are `dsdgp_randn(seed, stream = i)` (one draw of the total
    size, cut in var_list order); the path lengths and the acceptance uniforms come from `np.random.default_rng(seed)`, one
    `integers(lmin, lmax + 1)` and one `uniform()` per iteration, in that order.  A CholeskyError inside a trajectory is a rejection."""

    @staticmethod
    def _variables(model, var_list):
        var_list = [model.layers[0].q_mu] if var_list is None else list(var_list)
        if not var_list:
            raise ValueError("HMC: var_list is empty")
        return Variables(var_list, who="HMC")

    @staticmethod
    def _assign(variables, q):
        variables.assign([x.cpu().numpy() for x in q])

    @staticmethod
    def _logp_and_grad(model, variables):
        """(log density, its gradient in the unconstrained variables as device tensors) at the model's current parameters"""
        ctx = model._context()
        logp, pairs = model.compute_log_density_gradients()
        return float(logp), [ctx.to_device(g) for g in variables.chain(pairs)]

    @classmethod
    def _leapfrog(cls, model, variables, q, p, grad, epsilon, steps):
        """`steps` leapfrog steps from (q, p) with the gradient `grad` at q -> (q, p, log density at q, gradient at q); q, p: lists of
        device tensors, not modified"""
        eps = float(epsilon)
        q = [x.clone() for x in q]
        p = [m + (0.5 * eps) * g for m, g in zip(p, grad)]
        logp = None
        for s in range(int(steps)):
            for x, m in zip(q, p):
                x += eps * m
            cls._assign(variables, q)
            logp, grad = cls._logp_and_grad(model, variables)
            w = eps if s + 1 < int(steps) else 0.5 * eps
            p = [m + w * g for m, g in zip(p, grad)]
        return q, p, logp, grad

    @classmethod
    def leapfrog(cls, model, q, p, epsilon, steps, var_list=None):
        """`steps` leapfrog steps of size epsilon from position q and momentum p (arrays shaped like the variables — unconstrained
        values — or lists of them, one per entry of var_list) -> (q, p, log density at the new q) as numpy arrays (lists if lists were
        given).  The model's Parameters are left at the new position."""
        variables = cls._variables(model, var_list)
        ctx = model._context()
        single = not isinstance(q, (list, tuple))
        qd = [ctx.to_device(x) for x in ([q] if single else q)]
        pd = [ctx.to_device(x) for x in ([p] if single else p)]
        if len(qd) != len(variables.params) or any(tuple(x.shape) != v.shape or tuple(m.shape) != v.shape
                                                   for x, m, v in zip(qd, pd, variables.params)):
            raise ValueError("HMC.leapfrog: q and p must have the shapes of var_list")
        cls._assign(variables, qd)
        _, grad = cls._logp_and_grad(model, variables)
        qd, pd, logp, _ = cls._leapfrog(model, variables, qd, pd, grad, epsilon, steps)
        qn, pn = [x.cpu().numpy() for x in qd], [m.cpu().numpy() for m in pd]
        return (qn[0], pn[0], logp) if single else (qn, pn, logp)

    @classmethod
    def momenta(cls, model, var_list, seed, iteration):
        """the momenta of one iteration: dsdgp_randn(seed, stream = iteration), cut in var_list order (device tensors)"""
        import ctypes as C
        from . import _lib
        ctx = model._context()
        flat = ctx.empty(sum(int(np.prod(p.shape)) for p in var_list))
        _lib.check(ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(int(seed)), C.c_uint64(int(iteration)), flat.numel(), C.c_void_p(flat.data_ptr())))
        return Variables(var_list).cut(flat)

    def sample(self, model, num_samples, epsilon, lmin=1, lmax=1, thin=1, burn=0, var_list=None, seed=0):
        """-> dict(samples={name: (num_samples, *shape)} of the CONSTRAINED values — names "q_mu", then "var<i>" by position in var_list
        for any other Parameter —, logprobs (num_samples,), accepted (one flag per iteration, burn-in included), accept_rate).
        burn + num_samples thin iterations; every thin-th state after the burn-in is kept.  The model is left at the last state."""
        from ._lib import CholeskyError
        from .model_zoo import DGP_Heinonen
        if not isinstance(model, DGP_Heinonen) and not getattr(model, "_sgpmc", False):
            raise NotImplementedError(f"HMC samples a DGP_Heinonen; {type(model).__name__} has no log density to sample from")
        if int(num_samples) < 1 or int(thin) < 1 or int(burn) < 0 or int(lmin) < 1 or int(lmax) < int(lmin) or not float(epsilon) > 0.0:
            raise ValueError("HMC.sample: num_samples, thin >= 1, burn >= 0, 1 <= lmin <= lmax, epsilon > 0")
        variables = self._variables(model, var_list)
        var_list = variables.params
        names = ["q_mu" if p is model.layers[0].q_mu else f"var{i}" for i, p in enumerate(var_list)]
        rng = np.random.default_rng(seed)
        q = [model._context().to_device(x) for x in variables.values()]
        logp, grad = self._logp_and_grad(model, variables)
        kept, logps, accepted = {n: [] for n in names}, [], []
        for it in range(int(burn) + int(num_samples) * int(thin)):
            steps, u = int(rng.integers(int(lmin), int(lmax) + 1)), float(rng.uniform())
            p0 = self.momenta(model, var_list, seed, it)
            H0 = -logp + 0.5 * sum(float((m * m).sum()) for m in p0)
            try:
                q1, p1, logp1, grad1 = self._leapfrog(model, variables, q, p0, grad, epsilon, steps)
                H1 = -logp1 + 0.5 * sum(float((m * m).sum()) for m in p1)
                ok = bool(np.log(u) < H0 - H1)
            except CholeskyError:
                ok = False
            if ok:
                q, logp, grad = q1, logp1, grad1
            accepted.append(ok)
            if it >= int(burn) and (it - int(burn) + 1) % int(thin) == 0:
                for n, x in zip(names, variables.constrained([x.cpu().numpy() for x in q])):
                    kept[n].append(x)
                logps.append(logp)
        self._assign(variables, q)
        accepted = np.array(accepted, dtype=bool)
        return dict(samples={n: np.stack(v) for n, v in kept.items()}, logprobs=np.array(logps), accepted=accepted,
                    accept_rate=float(np.mean(accepted)))


class SGHMC:
    """Stochastic-gradient Hamiltonian Monte Carlo (Chen, Fox and Guestrin 2014, eq. 15, with the gradient-noise estimate at 0) on the
    log density of a `model_zoo.DGP_SGPMC`: per iteration ONE minibatch gradient (`compute_log_density_gradients`) and ONE
    dsdgp_sghmc_step over the flat vector of the variables,
        theta += v;   v = (1 - friction) v + learning_rate g + sqrt(2 friction learning_rate) xi,
    g the gradient of the log density at the position the iteration started from, xi = dsdgp_randn(seed, stream = iteration): a run
    replays from its seed (together with the model's minibatch and draw sequences; `model.fix_draws` pins the latter).  No
    accept / reject step: the sampler is biased at the order of the learning rate.
    The variables are `var_list`, by default every layer's `q_mu`; any Parameter among the pairs of `compute_log_density_gradients`
    may be added.  A positive parameter moves in unconstrained space, theta = softplus(x) + 1e-6, with a FLAT density there, exactly as
    `training.HMC` documents: only the q_mu have priors, no Jacobian term is added.  Position and momentum are device tensors; the
    model's Parameters are assigned at every position, which is how the gradient sees it.  A CholeskyError at a new position restores
    the previous position and momentum and draws the next minibatch."""

    def __init__(self, learning_rate=1e-4, friction=0.05):
        self.eta, self.alpha = float(learning_rate), float(friction)
        if not self.eta > 0.0 or not 0.0 <= self.alpha <= 1.0:
            raise ValueError("SGHMC: learning_rate > 0 and 0 <= friction <= 1")

    @staticmethod
    def _check(model):
        from .model_zoo import DGP_SGPMC
        if not isinstance(model, DGP_SGPMC):
            raise NotImplementedError(f"SGHMC samples a DGP_SGPMC; {type(model).__name__} is trained by its own optimisers "
                                      "(a DGP_Heinonen is sampled by HMC)")

    @staticmethod
    def _names(model, var_list):
        qs = {id(layer.q_mu): l for l, layer in enumerate(model.layers)}
        return ["q_mu%d" % qs[id(p)] if id(p) in qs else f"var{i}" for i, p in enumerate(var_list)]

    @staticmethod
    def _gradient(model, variables, ctx):
        """(log density, its gradient in the unconstrained variables as one flat device tensor) at the model's Parameters, on the next
        minibatch"""
        logp, pairs = model.compute_log_density_gradients()
        return logp, ctx.to_device(variables.flat(variables.chain(pairs)))

    def step(self, ctx, theta, v, g, xi):
        """one dsdgp_sghmc_step on flat device tensors, in place"""
        import ctypes as C
        from . import _lib
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _lib.check(ctx.lib.dsdgp_sghmc_step(ctx.handle, theta.numel(), p(theta), p(v), p(g), p(xi), self.alpha, self.eta))

    def sample(self, model, num_samples, thin=1, burn=0, var_list=None, seed=0):
        """-> dict(samples={name: (num_samples, *shape)} of the CONSTRAINED values — names "q_mu<layer>", then "var<i>" by position in
        var_list for any other Parameter —, logprobs (num_samples,): the minibatch log density at each kept state, names, variables (the
        Parameters, in the order of names: what DGP_SGPMC's scoring methods take as `run`)).  burn + num_samples thin iterations;
        every thin-th state after the burn-in is kept.  The model is left at the last state."""
        import ctypes as C
        from . import _lib
        self._check(model)
        if int(num_samples) < 1 or int(thin) < 1 or int(burn) < 0:
            raise ValueError("SGHMC.sample: num_samples, thin >= 1, burn >= 0")
        var_list = [layer.q_mu for layer in model.layers] if var_list is None else list(var_list)
        if not var_list:
            raise ValueError("SGHMC: var_list is empty")
        names = self._names(model, var_list)
        ctx = model._context()
        variables = Variables(var_list, who="SGHMC")
        assign = lambda theta: variables.assign(variables.cut(theta.cpu().numpy()))
        theta = ctx.to_device(variables.flat(variables.values()))
        v = ctx.torch.zeros_like(theta)
        xi = ctx.empty(theta.numel())
        logp, g = self._gradient(model, variables, ctx)
        kept, logps = {n: [] for n in names}, []
        for it in range(int(burn) + int(num_samples) * int(thin)):
            _lib.check(ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(int(seed)), C.c_uint64(it), theta.numel(), C.c_void_p(xi.data_ptr())))
            theta0, v0 = theta.clone(), v.clone()
            self.step(ctx, theta, v, g, xi)
            assign(theta)
            try:
                logp, g = self._gradient(model, variables, ctx)
            except _lib.CholeskyError:
                theta, v = theta0, v0                       # the previous state, and the gradient there on the next minibatch
                assign(theta)
                logp, g = self._gradient(model, variables, ctx)
            if it >= int(burn) and (it - int(burn) + 1) % int(thin) == 0:
                for n, x in zip(names, variables.constrained(variables.cut(theta.cpu().numpy()))):
                    kept[n].append(x)
                logps.append(logp)
        assign(theta)
        return dict(samples={n: np.stack(x) for n, x in kept.items()}, logprobs=np.array(logps), names=names, variables=var_list)

"""The one small model of the HMC tests (tests/test_hmc_reference_cpu.py, tests/test_gpu_hmc.py): the reference's shapes for the dense
two-layer model (tests/test_zoo_models.py: N = 6, D_X = 3, D_Y = 2, Matern52 kernels with lengthscale 0.5), an Identity mean under the
inner layer whose kernel has variance 0.1 (as in test_vs_single_layer there), a Zero mean and noise variance 0.1 on top.  Everything from default_rng(7)."""
import functools

import numpy as np

from tests import dense_reference as DR
from tests import gram_grad_reference as GR

N, D_X, D_Y = 6, 3, 2
LS, VAR0, VAR1, NOISE, JITTER = 0.5, 0.1, 1.0, 0.1, 1e-6
EPS_REPLAY, LMIN, LMAX, ITERS, SEED = 0.5, 1, 4, 5, 11      # two of the five iterations reject, three accept


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(7)
    X, Y = rng.uniform(size=(N, D_X)), rng.standard_normal((N, D_Y))
    q0, p0 = 0.5 * rng.standard_normal((N, D_X)), rng.standard_normal((N, D_X))
    for a in (X, Y, q0, p0):
        a.setflags(write=False)
    return dict(X=X, Y=Y, q0=q0, p0=p0)


def logp_grad(dtype, fail_when=None):
    """q -> (log density, gradient) of the model at precision dtype (tests/dense_reference.py: log_density); fail_when(q): raise
    LinAlgError there, as a failed factorisation would"""
    d = data()
    ls = np.array([LS])
    Lu = DR.gpmc(GR.MATERN52, d["X"], d["q0"], VAR0, ls, None, JITTER, dtype=dtype)[0]["Lu"]

    def f(q):
        if fail_when is not None and fail_when(q):
            raise np.linalg.LinAlgError("not positive definite")
        v, g, _ = DR.log_density((GR.MATERN52, GR.MATERN52), d["X"], d["Y"], q, VAR0, ls, JITTER, VAR1, ls, False, NOISE,
                                 mean0="identity", mean1=None, dtype=dtype, Lu=Lu)
        return v, g
    return f


def build_model():
    """the same model on the device (needs a GPU)"""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Identity, Matern52, Zero
    from doubly_stochastic_dgp.layers import GPMC_Layer, GPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Heinonen
    d = data()
    with settings.temp_jitter(JITTER):
        layer0 = GPMC_Layer(Matern52(D_X, lengthscales=LS, variance=VAR0), d["X"].copy(), D_X, Identity())
    layer1 = GPR_Layer(Matern52(D_X, lengthscales=LS, variance=VAR1), Zero(), D_Y)
    model = DGP_Heinonen(d["X"], d["Y"], Gaussian(variance=NOISE), [layer0, layer1])
    model.layers[0].q_mu = d["q0"]
    return model

"""CPU side of tests/test_gpu_evaluate.py: the held-out scores of the reference's experiment script restated in numpy / scipy, from
demos/run_regression.py:108-123 (the loop over predict_y batches, the mixture mean, the RMSE, logsumexp of norm.logpdf) and
dgp.py:116-126 (predict_y, predict_density).  No product kernel is involved in the reduction itself; tests/test_evaluate_reference_cpu.py
pins it against direct draws from the mixture.

Components: (logp, E, V), each (S, N, D) — the log density of the target under component s and the component's predictive mean and
variance (what predict_mean_and_var returns for it).  Per (i, d):
  mhat = mean_s E_s ;  mixture variance = mean_s (V_s + E_s^2) - mhat^2 (law of total variance) ;  l = logsumexp_s logp_s - log S
rows = (N, D, 3) of these; sums = (3, D): [sum_i (Y - mhat)^2, sum_i l, N] per output.
MultiClass: logp is (S, N, 1) for the label, E = P (S, N, K) the class probabilities; the squared error gives way to the indicator that
numpy.argmax_k mhat_k differs from the label, and only output 0 carries sums."""
import numpy as np
from scipy.special import logsumexp
from scipy.stats import norm


def gaussian_components(mean, var, Y, lik_var):
    """Gaussian likelihood in closed form: component s is N(mean_s, var_s + lik_var) (dgp.py:116-119 adds the noise variance)."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    V = var + lik_var
    return norm.logpdf(np.asarray(Y)[None], mean, np.sqrt(V)), mean, V


def host_components(lik, mean, var, Y):
    """Any other likelihood: the moments from the host likelihood class (BroadcastingLikelihood.predict_mean_and_var), the log
    densities from its predict_density applied to every component on its own (a mixture of one: logsumexp over one entry - log 1)."""
    mean = np.asarray(mean, dtype=np.float64)
    var = np.broadcast_to(np.asarray(var, dtype=np.float64), mean.shape)
    S, N, D = mean.shape
    E, V = lik.predict_mean_and_var(mean, var)
    Yt = np.tile(np.asarray(Y, dtype=np.float64), (S, 1))
    logp = lik.predict_density_logmeanexp(mean.reshape(1, S * N, D), var.reshape(1, S * N, D), Yt)
    return logp.reshape(S, N, -1), E, V


def mixture_rows(logp, E, V):
    S = E.shape[0]
    mhat = E.mean(0)
    mixvar = (V + E ** 2).mean(0) - mhat ** 2
    ell = logsumexp(logp, axis=0) - np.log(S)
    return np.stack([mhat, mixvar, np.broadcast_to(ell, mhat.shape)], axis=-1)


def sums(rows, Y):
    """(3, D) for the element-wise likelihoods"""
    Y = np.asarray(Y, dtype=np.float64)
    return np.stack([((Y - rows[..., 0]) ** 2).sum(0), rows[..., 2].sum(0), np.full(Y.shape[1], float(Y.shape[0]))])


def multiclass_sums(rows, Y):
    """(3, K): misclassifications, sum of l and the row count in column 0, zeros elsewhere"""
    N, K, _ = rows.shape
    out = np.zeros((3, K))
    out[0, 0] = float(np.sum(np.argmax(rows[..., 0], axis=1) != np.asarray(Y)[:, 0].astype(int)))
    out[1, 0] = rows[:, 0, 2].sum()
    out[2, 0] = float(N)
    return out


def scores(s, Y_std=1.0, gaussian=True, multiclass=False):
    """the dict DGP_Base.evaluate returns, from the (3, D) sums"""
    if multiclass:
        return {"error_rate": s[0, 0] / s[2, 0], "log_density": s[1, 0] / s[2, 0]}
    cnt = s[2].sum()
    return {"rmse": Y_std * np.sqrt(s[0].sum() / cnt), "rmse_per_output": Y_std * np.sqrt(s[0] / s[2]),
            "log_density": s[1].sum() / cnt - (np.log(Y_std) if gaussian else 0.0)}


def run_regression_scores(mean_SND, var_SND, Ys, Y_std):
    """demos/run_regression.py:119-123, literally (predict_y outputs of all batches concatenated along N)"""
    S = mean_SND.shape[0]
    mean_ND = np.average(mean_SND, 0)
    test_err = np.average(Y_std * np.mean((Ys - mean_ND) ** 2.0) ** 0.5)
    test_nll_ND = logsumexp(norm.logpdf(Ys * Y_std, mean_SND * Y_std, var_SND ** 0.5 * Y_std), 0, b=1 / float(S))
    return test_err, np.average(test_nll_ND)

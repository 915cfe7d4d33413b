// The element-wise likelihoods behind BroadcastingLikelihood (utils.py:54-121 wraps ANY likelihood): the formulas, one family tag that
// the kernels are instantiated on, and the host helpers every launch site dispatches through.  A further element-wise likelihood is
// one more case in this file.  MultiClass is not element-wise and has kernels of its own (multiclass.hip).
#pragma once
#include <type_traits>

#include "common.hpp"

// Family of a likelihood kind = the template parameter of k_lik_elbo / k_lik_over_samples / k_lik_predict / k_eval_mix: the Gaussian's
// and the Bernoulli's closed forms are compile-time instances, LIKF_QUAD takes the kind at run time (closed forms with the exp link,
// the 20-point Gauss-Hermite rule otherwise).
enum { LIKF_NONE = -1, LIKF_GAUSS = 0, LIKF_BERN = 1, LIKF_QUAD = 2 };
// the family of DSDGP_LIK_*, LIKF_NONE for MultiClass and for anything that is no likelihood kind
static inline int lik_family(int kind) {
  switch (kind) {
    case DSDGP_LIK_GAUSSIAN: return LIKF_GAUSS;
    case DSDGP_LIK_BERNOULLI: return LIKF_BERN;
    case DSDGP_LIK_POISSON: case DSDGP_LIK_EXPONENTIAL: case DSDGP_LIK_STUDENT_T: case DSDGP_LIK_GAMMA: case DSDGP_LIK_BETA: return LIKF_QUAD;
    default: return LIKF_NONE;
  }
}
// the likelihood owns one positive parameter p0 (Gaussian.variance / StudentT.scale / Gamma.shape / Beta.scale; in a model:
// desc.off_lik_var in theta, lik_const[0] on the device).  A bit test, not a chain of comparisons: k_lik_elbo<LIKF_QUAD> sits at the
// register limit, and one more scalar comparison there costs it a spill slot.
__host__ __device__ static inline bool lik_has_param(int kind) {
  constexpr unsigned with_param = 1u << DSDGP_LIK_GAUSSIAN | 1u << DSDGP_LIK_STUDENT_T | 1u << DSDGP_LIK_GAMMA | 1u << DSDGP_LIK_BETA;
  return (unsigned)kind < 32u && ((with_param >> kind) & 1u);
}
// p0 as above, p1 = Poisson.binsize / StudentT.deg_free: the values an element-wise kind accepts
static inline bool lik_params_ok(int kind, double p0, double p1) {
  if (lik_family(kind) == LIKF_NONE) return false;
  if (lik_has_param(kind) && !(p0 > 0.0)) return false;
  return (kind != DSDGP_LIK_POISSON && kind != DSDGP_LIK_STUDENT_T) || p1 > 0.0;
}
// f(std::integral_constant<int, LIKF_*>) for the family of a run-time kind; false (and no call) for LIKF_NONE
template <class Fn>
static inline bool lik_dispatch(int kind, Fn f) {
  switch (lik_family(kind)) {
    case LIKF_GAUSS: f(std::integral_constant<int, LIKF_GAUSS>()); return true;
    case LIKF_BERN: f(std::integral_constant<int, LIKF_BERN>()); return true;
    case LIKF_QUAD: f(std::integral_constant<int, LIKF_QUAD>()); return true;
    default: return false;
  }
}

#ifdef __HIPCC__
// node k (0..19, ascending) of np.polynomial.hermite.hermgauss(20) and its weight / sqrt(pi): the base Likelihood's rule
__device__ __forceinline__ void lik_gh20(int k, double& x, double& w) {
  constexpr double GX[10] = {0.24534070830090124, 0.7374737285453944, 1.234076215395323, 1.7385377121165861, 2.2549740020892757,
                             2.7888060584281305, 3.3478545673832163, 3.944764040115625, 4.603682449550744, 5.387480890011233};
  constexpr double GW[10] = {0.2607930634495549, 0.16173933398399998, 0.0615063720639769, 0.013997837447101022,
                             0.00183010313108049, 0.00012882627996192928, 4.402121090230851e-06, 6.127490259982928e-08,
                             2.4820623623151755e-10, 1.2578006724379234e-13};
  x = (k < 10) ? -GX[9 - k] : GX[k - 10];
  w = (k < 10) ? GW[9 - k] : GW[k - 10];
}

// ---- [UPSTREAM] Bernoulli likelihood, probit link (upstream's tests/test_dgp.py:48-54 builds it; its variational expectations are
// the base Likelihood's 20-point Gauss-Hermite rule, its predictions the probit closed form)
// probit(x) = Phi(x) (1 - 2e-3) + 1e-3
__device__ __forceinline__ double bern_probit(double x) { return 0.5 * (1.0 + erf(x * 0.70710678118654752440)) * (1.0 - 2e-3) + 1e-3; }
// log Bernoulli(y | p): y == 1 selects p, every other target 1 - p
__device__ __forceinline__ double bern_logp(double p, double y) { return log(y == 1.0 ? p : 1.0 - p); }
// variational expectation int log p(y | f) N(f | mu, v) df; dmu / dv = its derivatives.  No clamp on v: a negative variance gives
// NaN, as upstream's sqrt does.
__device__ __forceinline__ double bern_var_exp(double mu, double v, double y, double* dmu, double* dv) {
  const double sd = sqrt(2.0 * v);
  const double sgn = (y == 1.0) ? 1.0 : -1.0;
  double ve = 0.0, gm = 0.0, gv = 0.0;
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    double x, w;
    lik_gh20(k, x, w);
    const double f = mu + sd * x;
    const double p = bern_probit(f);
    const double q = (y == 1.0) ? p : 1.0 - p;
    ve += w * log(q);
    const double dl = sgn * (1.0 - 2e-3) * 0.39894228040143267794 * exp(-0.5 * f * f) / q;      // d log q / d f
    gm += w * dl;
    gv += w * dl * x;
  }
  *dmu = gm;
  *dv = gv / sd;
  return ve;
}

// ---- [UPSTREAM] further GPflow 1.1.1 likelihoods: Poisson and Exponential / Gamma with the exp link, StudentT, Beta.
// kind = DSDGP_LIK_*; p0 = StudentT.scale / Gamma.shape / Beta.scale, p1 = Poisson.binsize / StudentT.deg_free.
// digamma(x), x > 0: recurrence up to x >= 8, then the asymptotic series (error < 1e-15 there)
__device__ __forceinline__ double digamma_d(double x) {
  double r = 0.0;
  while (x < 8.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double i = 1.0 / x, i2 = i * i;
  return r + log(x) - 0.5 * i -
         i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0 - i2 / 12.0))))));
}
// log p(y | f).  Gamma (exp link): p0 = shape.  Beta (the Bernoulli's probit link): p0 = scale, y clipped to [1e-6, 1 - 1e-6].
__device__ __forceinline__ double lik_logp(int kind, double f, double y, double p0, double p1) {
  if (kind == DSDGP_LIK_GAMMA) return -p0 * f - lgamma(p0) + (p0 - 1.0) * log(y) - y * exp(-f);
  if (kind == DSDGP_LIK_BETA) {
    const double mean = bern_probit(f), al = mean * p0, be = p0 - al, yc = fmin(fmax(y, 1e-6), 1.0 - 1e-6);
    return (al - 1.0) * log(yc) + (be - 1.0) * log(1.0 - yc) + lgamma(al + be) - lgamma(al) - lgamma(be);
  }
  if (kind == DSDGP_LIK_POISSON) return y * (f + log(p1)) - exp(f) * p1 - lgamma(y + 1.0);      // y log(lam) - lam - lgamma(y + 1), lam = exp(f) binsize
  if (kind == DSDGP_LIK_EXPONENTIAL) return -y * exp(-f) - f;                                 // -y / scale - log(scale), scale = exp(f)
  const double nu = p1, z = (y - f) / p0;                                                     // StudentT
  return lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * (log(nu) + 1.1447298858494001741) - log(p0) -
         0.5 * (nu + 1.0) * log(1.0 + z * z / nu);
}
// conditional mean / variance of y given f
__device__ __forceinline__ void lik_cond(int kind, double f, double p0, double p1, double* cm, double* cv) {
  if (kind == DSDGP_LIK_POISSON) { *cm = *cv = exp(f) * p1; return; }
  if (kind == DSDGP_LIK_EXPONENTIAL) { const double e = exp(f); *cm = e; *cv = e * e; return; }
  if (kind == DSDGP_LIK_GAMMA) { const double e = exp(f); *cm = p0 * e; *cv = p0 * e * e; return; }
  if (kind == DSDGP_LIK_BETA) { const double m = bern_probit(f); *cm = m; *cv = (m - m * m) / (p0 + 1.0); return; }
  *cm = f;
  *cv = p0 * p0 * (p1 / (p1 - 2.0));
}
// variational expectation int log p(y | f) N(f | mu, v) df and its derivatives w.r.t. mu, v and p0: the closed forms GPflow uses with
// the exp link (Poisson, Exponential, Gamma), the Gauss-Hermite rule for Beta and StudentT
__device__ __forceinline__ double lik_var_exp(int kind, double mu, double v, double y, double p0, double p1, double* dmu, double* dv,
                                              double* dp0) {
  *dp0 = 0.0;
  if (kind == DSDGP_LIK_POISSON) {
    const double e = exp(mu + 0.5 * v) * p1;
    *dmu = y - e;
    *dv = -0.5 * e;
    return y * mu - e - lgamma(y + 1.0) + y * log(p1);
  }
  if (kind == DSDGP_LIK_EXPONENTIAL) {
    const double e = exp(-mu + 0.5 * v) * y;
    *dmu = e - 1.0;
    *dv = -0.5 * e;
    return -e - mu;
  }
  if (kind == DSDGP_LIK_GAMMA) {      // -shape mu - lgamma(shape) + (shape - 1) log y - y exp(-mu + v / 2)
    const double e = exp(-mu + 0.5 * v) * y;
    *dmu = e - p0;
    *dv = -0.5 * e;
    *dp0 = -mu - digamma_d(p0) + log(y);
    return -p0 * mu - lgamma(p0) + (p0 - 1.0) * log(y) - e;
  }
  if (kind == DSDGP_LIK_BETA) {      // quadrature of the log density, its derivatives through alpha = probit(f) scale, beta = scale - alpha
    const double sd = sqrt(2.0 * v), yc = fmin(fmax(y, 1e-6), 1.0 - 1e-6), ly = log(yc), l1y = log(1.0 - yc);
    const double lgs = lgamma(p0), dgs = digamma_d(p0);
    double ve = 0.0, gm = 0.0, gv = 0.0, gp = 0.0;
#pragma unroll 1
    for (int k = 0; k < 20; ++k) {
      double x, w;
      lik_gh20(k, x, w);
      const double f = mu + sd * x;
      const double mean = bern_probit(f), al = mean * p0, be = p0 - al;
      ve += w * ((al - 1.0) * ly + (be - 1.0) * l1y + lgs - lgamma(al) - lgamma(be));
      const double da = digamma_d(al), db = digamma_d(be);
      const double dl = (1.0 - 2e-3) * 0.39894228040143267794 * exp(-0.5 * f * f) * p0 * (ly - l1y - da + db);      // d log p / d f
      gm += w * dl;
      gv += w * dl * x;
      gp += w * (mean * ly + (1.0 - mean) * l1y + dgs - mean * da - (1.0 - mean) * db);
    }
    *dmu = gm;
    *dv = gv / sd;
    *dp0 = gp;
    return ve;
  }
  const double sd = sqrt(2.0 * v), nu = p1;      // StudentT
  const double c0 = lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * (log(nu) + 1.1447298858494001741) - log(p0);
  double ve = 0.0, gm = 0.0, gv = 0.0, gp = 0.0;
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    double x, w;
    lik_gh20(k, x, w);
    const double r = y - (mu + sd * x), den = nu * p0 * p0 + r * r;
    ve += w * (c0 - 0.5 * (nu + 1.0) * log(den / (nu * p0 * p0)));
    const double dl = (nu + 1.0) * r / den;                       // d log p / d f
    gm += w * dl;
    gv += w * dl * x;
    gp += w * (-1.0 / p0 + (nu + 1.0) * r * r / (p0 * den));      // d log p / d scale
  }
  *dmu = gm;
  *dv = gv / sd;
  *dp0 = gp;
  return ve;
}
// log int p(y | f) N(f | mu, v) df (predict_density) by the same rule
__device__ __forceinline__ double lik_log_density(int kind, double mu, double v, double y, double p0, double p1) {
  const double sd = sqrt(2.0 * v);
  double s = 0.0;
#pragma unroll 1
  for (int k = 0; k < 20; ++k) {
    double x, w;
    lik_gh20(k, x, w);
    s += w * exp(lik_logp(kind, mu + sd * x, y, p0, p1));
  }
  return log(s);
}
// predict_mean_and_var: E_y = sum w cm(f_k), V_y = sum w (cv(f_k) + cm(f_k)^2) - E_y^2
__device__ __forceinline__ void lik_predict(int kind, double mu, double v, double p0, double p1, double* ey, double* vy) {
  const double sd = sqrt(2.0 * v);
  double e = 0.0, q = 0.0;
#pragma unroll 1
  for (int k = 0; k < 20; ++k) {
    double x, w;
    lik_gh20(k, x, w);
    double cm, cv;
    lik_cond(kind, mu + sd * x, p0, p1, &cm, &cv);
    e += w * cm;
    q += w * (cv + cm * cm);
  }
  *ey = e;
  *vy = q - e * e;
}

// ---- the three things a kernel asks of a likelihood, per family F (kind is read by LIKF_QUAD only)
// Variational expectation `ve` of one component; am / av = c times its derivatives w.r.t. mu / v, for the caller's scale c; dp = its
// derivative w.r.t. p0.  The scale goes in because the Gaussian's adjoints are rounded as c (y - mu) / s2 and -0.5 c / s2.
template <int F>
__device__ __forceinline__ void lik_ve(int kind, double mu, double v, double y, double p0, double p1, double c, double& ve, double& am,
                                       double& av, double& dp) {
  if (F == LIKF_GAUSS) {      // [UPSTREAM] Gaussian.variational_expectations (dgp.py:89-90); p0 = variance
    const double q = (y - mu) * (y - mu) + v;
    ve = -0.91893853320467274178 - 0.5 * log(p0) - 0.5 * q / p0;
    dp = -0.5 / p0 + 0.5 * q / (p0 * p0);
    am = c * (y - mu) / p0;
    av = -0.5 * c / p0;
  } else {
    double dm, dv;
    if (F == LIKF_BERN) {
      ve = bern_var_exp(mu, v, y, &dm, &dv);
      dp = 0.0;
    } else {
      ve = lik_var_exp(kind, mu, v, y, p0, p1, &dm, &dv, &dp);
    }
    am = c * dm;
    av = c * dv;
  }
}
// log predictive density of one component
template <int F>
__device__ __forceinline__ double lik_density(int kind, double mu, double v, double y, double p0, double p1) {
  if (F == LIKF_GAUSS) {
    const double vv = v + p0, r = y - mu;
    return -0.91893853320467274178 - 0.5 * log(vv) - 0.5 * r * r / vv;
  }
  if (F == LIKF_BERN) return bern_logp(bern_probit(mu / sqrt(1.0 + v)), y);
  return lik_log_density(kind, mu, v, y, p0, p1);
}
// predict_mean_and_var of one component
template <int F>
__device__ __forceinline__ void lik_moments(int kind, double mu, double v, double p0, double p1, double& E, double& V) {
  if (F == LIKF_GAUSS) {
    E = mu;
    V = v + p0;
  } else if (F == LIKF_BERN) {
    const double p = bern_probit(mu / sqrt(1.0 + v));
    E = p;
    V = p - p * p;
  } else {
    lik_predict(kind, mu, v, p0, p1, &E, &V);
  }
}
#endif

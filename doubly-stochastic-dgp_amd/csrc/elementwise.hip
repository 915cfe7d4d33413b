// Thin elementwise / gather entry points around the hot path (minibatch gather, the element-wise likelihoods' wrappers).
#include "likelihood.hpp"

__global__ void k_gather_rows(const double* __restrict__ src, int64_t cols, const int64_t* __restrict__ idx, int64_t n,
                              double* __restrict__ dst) {
  const int64_t total = n * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols, c = i % cols;
    dst[i] = src[idx[r] * cols + c];
  }
}

extern "C" int dsdgp_gather_rows(dsdgp_ctx* ctx, const double* src, int64_t cols, const int64_t* idx, int64_t n,
                                 int64_t idx_offset, double* dst) {
  DS_CHECK_ARG(ctx && src && idx && dst && n > 0 && cols > 0);
  const int nb = (int)std::min<int64_t>(4096, ceil_div(n * cols, 256));
  DS_LAUNCH(k_gather_rows, dim3(nb), dim3(256), 0, ctx->stream, src, cols, idx + idx_offset, n, dst);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// X and Y rows of one minibatch in one launch (Minibatch(X), Minibatch(Y) share their seed, dgp.py:51-52)
__global__ void k_gather_rows2(const double* __restrict__ a, int64_t ca, double* __restrict__ da, const double* __restrict__ b,
                               int64_t cb, double* __restrict__ db, const int64_t* __restrict__ idx, int64_t n) {
  const int64_t ct = ca + cb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * ct; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ct, j = i % ct;
    if (j < ca)
      da[r * ca + j] = a[idx[r] * ca + j];
    else
      db[r * cb + (j - ca)] = b[idx[r] * cb + (j - ca)];
  }
}
extern "C" int dsdgp_gather_rows2(dsdgp_ctx* ctx, const double* srcX, int64_t colsX, double* dstX, const double* srcY,
                                  int64_t colsY, double* dstY, const int64_t* idx, int64_t n, int64_t idx_offset) {
  DS_CHECK_ARG(ctx && srcX && srcY && dstX && dstY && idx && n > 0 && colsX > 0 && colsY > 0);
  const int nb = (int)std::min<int64_t>(4096, ceil_div(n * (colsX + colsY), 256));
  DS_LAUNCH(k_gather_rows2, dim3(nb), dim3(256), 0, ctx->stream, srcX, colsX, dstX, srcY, colsY, dstY, idx + idx_offset, n);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// ---- the element-wise likelihoods through BroadcastingLikelihood, one instance per family (likelihood.hpp).
// mode 0: mean_s variational expectation, or with quadrature weights sw their weighted sum (DGP_Quad.E_log_p_Y, dgp.py:160-166; the MC
// mean is dgp.py:90) ; mode 1: logsumexp_s predictive log density - log S, in two passes (maximum, then sum)
template <int F>
__global__ __launch_bounds__(256) void k_lik_over_samples(int kind, double p0, double p1, const double* __restrict__ mean, const double* __restrict__ var,
                                   const double* __restrict__ Y, int64_t n, int S, int DY, int mode, const double* __restrict__ sw,
                                   double* __restrict__ out) {
  const int64_t total = n * DY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const double y = Y[i];
    if (mode == 0) {
      double acc = 0.0;
      for (int s = 0; s < S; ++s) {
        double ve, am, av, dp;
        lik_ve<F>(kind, mean[(int64_t)s * total + i], var[(int64_t)s * total + i], y, p0, p1, 0.0, ve, am, av, dp);
        acc += sw ? sw[s] * ve : ve;
      }
      out[i] = sw ? acc : acc / S;
    } else {
      double mx = -1.0 / 0.0;
      for (int s = 0; s < S; ++s) {
        const double l = lik_density<F>(kind, mean[(int64_t)s * total + i], var[(int64_t)s * total + i], y, p0, p1);
        mx = l > mx ? l : mx;
      }
      double acc = 0.0;
      for (int s = 0; s < S; ++s) {
        const double l = lik_density<F>(kind, mean[(int64_t)s * total + i], var[(int64_t)s * total + i], y, p0, p1);
        acc += (l == mx) ? 1.0 : exp(l - mx);      // (every component -inf: no NaN, the result stays -inf — evaluate.hip's lse_add)
      }
      out[i] = mx + log(acc) - log((double)S);
    }
  }
}
static int lik_over_samples(dsdgp_ctx* ctx, int kind, double p0, double p1, const double* mean, const double* var, const double* Y,
                            int64_t n, int S, int DY, int mode, const double* sw, double* out) {
  DS_CHECK_ARG(ctx && mean && var && Y && out && n > 0 && S > 0 && DY > 0 && (mode == 0 || mode == 1));
  DS_CHECK_ARG(mode == 0 || !sw);
  DS_CHECK_ARG(lik_params_ok(kind, p0, p1));
  const int nb = (int)std::min<int64_t>(4096, ceil_div(n * DY, 256));
  lik_dispatch(kind, [&](auto fam) {
    DS_LAUNCH(k_lik_over_samples<decltype(fam)::value>, dim3(nb), dim3(256), 0, ctx->stream, kind, p0, p1, mean, var, Y, n, S, DY, mode, sw, out);
  });
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}
// predict_mean_and_var of every component
template <int F>
__global__ __launch_bounds__(256) void k_lik_predict(int kind, double p0, double p1, const double* __restrict__ mean, const double* __restrict__ var,
                              int64_t count, double* __restrict__ om, double* __restrict__ ov) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    double e, q;
    lik_moments<F>(kind, mean[i], var[i], p0, p1, e, q);
    om[i] = e;
    ov[i] = q;
  }
}
static int lik_predict_all(dsdgp_ctx* ctx, int kind, double p0, double p1, const double* mean, const double* var, int64_t count,
                           double* out_mean, double* out_var) {
  DS_CHECK_ARG(ctx && mean && var && out_mean && out_var && count > 0);
  DS_CHECK_ARG(lik_params_ok(kind, p0, p1));
  const int nb = (int)std::min<int64_t>(4096, ceil_div(count, 256));
  lik_dispatch(kind, [&](auto fam) {
    DS_LAUNCH(k_lik_predict<decltype(fam)::value>, dim3(nb), dim3(256), 0, ctx->stream, kind, p0, p1, mean, var, count, out_mean, out_var);
  });
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_gauss_var_exp(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n,
                                   int32_t S, int32_t DY, double lik_var, const double* sample_w, double* out) {
  return lik_over_samples(ctx, DSDGP_LIK_GAUSSIAN, lik_var, 1.0, mean, var, Y, n, S, DY, 0, sample_w, out);
}
extern "C" int dsdgp_gauss_predict_density(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y,
                                           int64_t n, int32_t S, int32_t DY, double lik_var, double* out) {
  return lik_over_samples(ctx, DSDGP_LIK_GAUSSIAN, lik_var, 1.0, mean, var, Y, n, S, DY, 1, nullptr, out);
}
extern "C" int dsdgp_bernoulli_var_exp(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n,
                                       int32_t S, int32_t DY, int mode, const double* sample_w, double* out) {
  return lik_over_samples(ctx, DSDGP_LIK_BERNOULLI, 1.0, 1.0, mean, var, Y, n, S, DY, mode, sample_w, out);
}
extern "C" int dsdgp_bernoulli_predict(dsdgp_ctx* ctx, const double* mean, const double* var, int64_t count, double* out_mean,
                                       double* out_var) {
  return lik_predict_all(ctx, DSDGP_LIK_BERNOULLI, 1.0, 1.0, mean, var, count, out_mean, out_var);
}
// Poisson / Exponential / Gamma (exp link), StudentT and Beta only: the Gaussian and the Bernoulli have the entry points above
extern "C" int dsdgp_lik_var_exp(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var,
                                 const double* Y, int64_t n, int32_t S, int32_t DY, int mode, const double* sample_w, double* out) {
  DS_CHECK_ARG(lik_family(kind) == LIKF_QUAD);
  return lik_over_samples(ctx, kind, p0, p1, mean, var, Y, n, S, DY, mode, sample_w, out);
}
extern "C" int dsdgp_lik_predict(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var,
                                 int64_t count, double* out_mean, double* out_var) {
  DS_CHECK_ARG(lik_family(kind) == LIKF_QUAD);
  return lik_predict_all(ctx, kind, p0, p1, mean, var, count, out_mean, out_var);
}

__global__ void k_add_scalar(const double* __restrict__ in, double v, int64_t count, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[i] + v;
}
extern "C" int dsdgp_add_scalar(dsdgp_ctx* ctx, const double* in, double value, int64_t count, double* out) {
  DS_CHECK_ARG(ctx && in && out && count > 0);
  const int nb = (int)std::min<int64_t>(4096, ceil_div(count, 256));
  DS_LAUNCH(k_add_scalar, dim3(nb), dim3(256), 0, ctx->stream, in, value, count, out);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

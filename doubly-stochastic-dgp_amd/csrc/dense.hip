// The two small reductions of the dense collapsed layer (the reference's GPR_Layer, layers.py:310-342) that dsdgp_gram / dsdgp_potrf /
// dsdgp_trsm / dsdgp_gemm lack.  The host mirror composes them:  K = k(F, F) + s2 I (dsdgp_gram with the noise variance as its diagonal
// add);  L = chol(K);  V = L^-1 (Y - m(F));  the bound from L and V (dsdgp_gpr_bound);  at test inputs A = L^-1 K(F, X*),
// mean = A^T V + m(X*), var = Kdiag - colsum(A^2) (dsdgp_gpr_var).
// Every sum runs in a fixed order (a thread adds its entries in ascending order, then a fixed tree): the same inputs give the same bits.
#include <math.h>

#include "common.hpp"

#define DN_T 256

// one workgroup.  out[0] = the bound = sum over the outputs of log N(Y_d | m_d, L L^T) (multivariate_normal of layers.py:342), out[1 .. 3]
// its terms  -1/2 n DY log(2 pi),  -DY sum log L_ii,  -1/2 sum V^2
__global__ __launch_bounds__(DN_T) void k_gpr_bound(int64_t n, int DY, const double* __restrict__ L, int64_t ldl, const double* __restrict__ V,
                                                    int64_t ldv, double* __restrict__ out) {
  __shared__ double red[DN_T];
  const int tid = threadIdx.x;
  double ld = 0.0, vv = 0.0;
  for (int64_t i = tid; i < n; i += DN_T) ld += log(L[i * ldl + i]);
  for (int64_t e = tid; e < n * DY; e += DN_T) {
    const int64_t i = e / DY;
    const double v = V[i * ldv + (e - i * DY)];
    vv = fma(v, v, vv);
  }
  ld = block_sum<DN_T>(ld, red);
  vv = block_sum<DN_T>(vv, red);
  if (tid != 0) return;
  const double Dy = (double)DY;
  const double t1 = -0.5 * (double)n * Dy * log(2.0 * M_PI), t2 = -Dy * ld, t3 = -0.5 * vv;
  out[1] = t1;
  out[2] = t2;
  out[3] = t3;
  out[0] = (t1 + t2) + t3;
}

// var[r][d] = kdiag - sum_i A[i][r]^2 for every output d (layers.py:333-334), i ascending
__global__ __launch_bounds__(DN_T) void k_gpr_var(int64_t n, int64_t ns, int DY, const double* __restrict__ A, int64_t lda, double kdiag,
                                                  double* __restrict__ var) {
  const int64_t r = (int64_t)blockIdx.x * DN_T + threadIdx.x;
  if (r >= ns) return;
  double a = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double x = A[i * lda + r];
    a = fma(x, x, a);
  }
  const double v = kdiag - a;
  for (int d = 0; d < DY; ++d) var[r * DY + d] = v;
}

extern "C" int dsdgp_gpr_bound(dsdgp_ctx* ctx, int64_t n, int32_t DY, const double* L, int64_t ldl, const double* V, int64_t ldv,
                               double* out) {
  DS_CHECK_ARG(ctx && L && V && out);
  DS_CHECK_ARG(n >= 1 && DY >= 1 && ldl >= n && ldv >= DY);
  DS_LAUNCH(k_gpr_bound, dim3(1), dim3(DN_T), 0, ctx->stream, n, (int)DY, L, ldl, V, ldv, out);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_gpr_var(dsdgp_ctx* ctx, int64_t n, int64_t ns, int32_t DY, const double* A, int64_t lda, double kdiag, double* var) {
  DS_CHECK_ARG(ctx && A && var);
  DS_CHECK_ARG(n >= 1 && ns >= 1 && DY >= 1 && lda >= ns);
  DS_LAUNCH(k_gpr_var, dim3(ceil_div(ns, DN_T)), dim3(DN_T), 0, ctx->stream, n, ns, (int)DY, A, lda, kdiag, var);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

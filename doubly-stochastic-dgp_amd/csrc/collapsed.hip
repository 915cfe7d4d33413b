// The small reductions of the collapsed bound and its prediction (the reference's gplvm_build_likelihood / gplvm_build_predict, psi
// branch, layers.py:405-450, 483-525) that dsdgp_gram / dsdgp_potrf / dsdgp_trsm / dsdgp_gemm lack.  The host mirror (SGPR_Layer)
// composes them:  L = chol(Kuu);  T = L^-1 psi2;  G = L^-1 T^T  (dsdgp_scale_copy transposes);  B = G / s2 + I  (dsdgp_scale_copy);
// LB = chol(B);  c = LB^-1 L^-1 psi1^T Y / s2;  the bound's terms from LB, G, c, Y and psi0 (dsdgp_collapsed_bound);  at test inputs
// tmp1 = L^-1 K(Z, X*), tmp2 = LB^-1 tmp1, mean = tmp2^T c, var = Kdiag + colsum(tmp2^2) - colsum(tmp1^2) (dsdgp_collapsed_var).
// For the gradients of the bound (SGPR_Layer.bound_gradients) the same primitives give Sigma^-1, Kuu^-1, Kuu^-1 psi2 Kuu^-1 and alpha, and
// dsdgp_collapsed_adjoints turns them into the adjoints of psi2, of Kuu and of the noise variance.
// Every sum runs in a fixed order (a thread adds its entries in ascending order, then a fixed tree): the same inputs give the same bits.
#include <math.h>

#include "common.hpp"

#define CL_T 256

// B[i][j] = op(A)[i][j] / div + (i == j ? diag_add : 0), op(A) = A or A^T, m x n entries of B
__global__ __launch_bounds__(CL_T) void k_scale_copy(int trans, int m, int n, const double* __restrict__ A, int64_t lda, double div,
                                                     double diag_add, double* __restrict__ B, int64_t ldb) {
  const int64_t e = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  if (e >= (int64_t)m * n) return;
  const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
  const double a = trans ? A[(int64_t)j * lda + i] : A[(int64_t)i * lda + j];
  B[(int64_t)i * ldb + j] = a / div + (i == j ? diag_add : 0.0);
}

// one workgroup.  out[0] = the bound, out[1 .. 6] its terms (layers.py:443-448):
//   -1/2 N D log(2 pi s2),  -D sum log diag(LB),  -1/2 sum Y^2 / s2,  1/2 sum c^2,  -1/2 D psi0 / s2,  1/2 D tr(G) / s2
__global__ __launch_bounds__(CL_T) void k_collapsed_bound(int M, int64_t n, int DY, const double* __restrict__ LB, int64_t ldb,
                                                          const double* __restrict__ G, int64_t ldg, const double* __restrict__ c,
                                                          const double* __restrict__ Y, const double* __restrict__ psi0, double s2,
                                                          double* __restrict__ out) {
  __shared__ double red[CL_T];
  const int tid = threadIdx.x;
  double ld = 0.0, tr = 0.0, cc = 0.0, yy = 0.0;
  for (int i = tid; i < M; i += CL_T) {
    ld += log(LB[(int64_t)i * ldb + i]);
    tr += G[(int64_t)i * ldg + i];
  }
  for (int e = tid; e < M * DY; e += CL_T) cc = fma(c[e], c[e], cc);
  for (int64_t e = tid; e < n * DY; e += CL_T) yy = fma(Y[e], Y[e], yy);
  ld = block_sum<CL_T>(ld, red);
  tr = block_sum<CL_T>(tr, red);
  cc = block_sum<CL_T>(cc, red);
  yy = block_sum<CL_T>(yy, red);
  if (tid != 0) return;
  const double Dy = (double)DY, ND = (double)n * Dy;
  const double t1 = -0.5 * ND * log(2.0 * M_PI * s2), t2 = -Dy * ld, t3 = -0.5 * yy / s2, t4 = 0.5 * cc;
  const double t5 = -0.5 * Dy * (psi0[0] / s2), t6 = 0.5 * Dy * (tr / s2);
  out[1] = t1;
  out[2] = t2;
  out[3] = t3;
  out[4] = t4;
  out[5] = t5;
  out[6] = t6;
  out[0] = ((((t1 + t2) + t3) + t4) + t5) + t6;
}

// var[r][d] = kdiag + sum_m tmp2[m][r]^2 - sum_m tmp1[m][r]^2 for every output d (layers.py:521-524)
__global__ __launch_bounds__(CL_T) void k_collapsed_var(int M, int64_t ns, int DY, const double* __restrict__ tmp1, int64_t ld1,
                                                        const double* __restrict__ tmp2, int64_t ld2, double kdiag,
                                                        double* __restrict__ var) {
  const int64_t r = (int64_t)blockIdx.x * CL_T + threadIdx.x;
  if (r >= ns) return;
  double a1 = 0.0, a2 = 0.0;
  for (int m = 0; m < M; ++m) {
    const double x1 = tmp1[(int64_t)m * ld1 + r], x2 = tmp2[(int64_t)m * ld2 + r];
    a1 = fma(x1, x1, a1);
    a2 = fma(x2, x2, a2);
  }
  const double v = (kdiag + a2) - a1;
  for (int d = 0; d < DY; ++d) var[r * DY + d] = v;
}

// one workgroup.  The adjoints of the bound F(Kuu, psi0, psi1, psi2, s2) that are M x M, and the one of the noise variance:
//   dS = -1/2 D Si - 1/2 alpha alpha^T  (Si = Sigma^-1, Sigma = Kuu + psi2 / s2, alpha = Sigma^-1 psi1^T Y / s2)
//   g_psi2 = dS / s2 + 1/2 D Ki / s2,   d_Kuu = dS + 1/2 D Ki - 1/2 D KpK / s2   (Ki = Kuu^-1, KpK = Ki psi2 Ki)
//   out[0] = dF/ds2 = -1/2 N D / s2 + 1/2 sum Y^2 / s2^2 - sum c^2 / s2 + 1/2 D psi0 / s2^2 - 1/2 D tr(Ki psi2) / s2^2 - tr(dS psi2) / s2^2
//   (sum c^2 = b^T Sigma^-1 b / s2^2, b = psi1^T Y),  out[1 .. 6] its terms in this order,  out[7] = g_psi0 = -1/2 D / s2
__global__ __launch_bounds__(CL_T) void k_collapsed_adjoints(int M, int64_t n, int DY, const double* __restrict__ Si,
                                                             const double* __restrict__ Ki, const double* __restrict__ KpK,
                                                             const double* __restrict__ psi2, const double* __restrict__ alpha,
                                                             const double* __restrict__ c, const double* __restrict__ Y,
                                                             const double* __restrict__ psi0, double s2, double* __restrict__ g_psi2,
                                                             double* __restrict__ d_Kuu, double* __restrict__ out) {
  __shared__ double red[CL_T];
  const int tid = threadIdx.x;
  const double Dy = (double)DY;
  double tk = 0.0, ts = 0.0, cc = 0.0, yy = 0.0;
  for (int e = tid; e < M * M; e += CL_T) {
    const int i = e / M, j = e - i * M;
    double aa = 0.0;
    for (int d = 0; d < DY; ++d) aa = fma(alpha[i * DY + d], alpha[j * DY + d], aa);
    const double ki = 0.5 * Dy * Ki[e], dS = -0.5 * Dy * Si[e] - 0.5 * aa, p = psi2[e];
    g_psi2[e] = (dS + ki) / s2;
    d_Kuu[e] = (dS + ki) - 0.5 * Dy * (KpK[e] / s2);
    tk = fma(Ki[e], p, tk);
    ts = fma(dS, p, ts);
  }
  for (int e = tid; e < M * DY; e += CL_T) cc = fma(c[e], c[e], cc);
  for (int64_t e = tid; e < n * DY; e += CL_T) yy = fma(Y[e], Y[e], yy);
  tk = block_sum<CL_T>(tk, red);
  ts = block_sum<CL_T>(ts, red);
  cc = block_sum<CL_T>(cc, red);
  yy = block_sum<CL_T>(yy, red);
  if (tid != 0) return;
  const double s4 = s2 * s2;
  const double t1 = -0.5 * (double)n * Dy / s2, t2 = 0.5 * yy / s4, t3 = -cc / s2, t4 = 0.5 * Dy * (psi0[0] / s4);
  const double t5 = -0.5 * Dy * (tk / s4), t6 = -ts / s4;
  out[1] = t1;
  out[2] = t2;
  out[3] = t3;
  out[4] = t4;
  out[5] = t5;
  out[6] = t6;
  out[0] = ((((t1 + t2) + t3) + t4) + t5) + t6;
  out[7] = -0.5 * Dy / s2;
}

extern "C" int dsdgp_collapsed_adjoints(dsdgp_ctx* ctx, int32_t M, int64_t n, int32_t DY, const double* Si, const double* Ki,
                                        const double* KpK, const double* psi2, const double* alpha, const double* c, const double* Y,
                                        const double* psi0, double noise_var, double* g_psi2, double* d_Kuu, double* out) {
  DS_CHECK_ARG(ctx && Si && Ki && KpK && psi2 && alpha && c && Y && psi0 && g_psi2 && d_Kuu && out);
  DS_CHECK_ARG(M >= 1 && M <= DSDGP_MAX_MP && n >= 1 && DY >= 1);
  DS_LAUNCH(k_collapsed_adjoints, dim3(1), dim3(CL_T), 0, ctx->stream, (int)M, n, (int)DY, Si, Ki, KpK, psi2, alpha, c, Y, psi0, noise_var,
            g_psi2, d_Kuu, out);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_scale_copy(dsdgp_ctx* ctx, int trans, int m, int n, const double* A, int64_t lda, double div, double diag_add,
                                double* B, int64_t ldb) {
  DS_CHECK_ARG(ctx && A && B && A != B);
  DS_CHECK_ARG(m >= 1 && n >= 1 && ldb >= n && lda >= (trans ? m : n));
  DS_LAUNCH(k_scale_copy, dim3(ceil_div((int64_t)m * n, CL_T)), dim3(CL_T), 0, ctx->stream, trans ? 1 : 0, m, n, A, lda, div, diag_add, B,
            ldb);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_collapsed_bound(dsdgp_ctx* ctx, int32_t M, int64_t n, int32_t DY, const double* LB, int64_t ldb, const double* G,
                                     int64_t ldg, const double* c, const double* Y, const double* psi0, double noise_var, double* out) {
  DS_CHECK_ARG(ctx && LB && G && c && Y && psi0 && out);
  DS_CHECK_ARG(M >= 1 && n >= 1 && DY >= 1 && ldb >= M && ldg >= M);
  DS_LAUNCH(k_collapsed_bound, dim3(1), dim3(CL_T), 0, ctx->stream, (int)M, n, (int)DY, LB, ldb, G, ldg, c, Y, psi0, noise_var, out);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_collapsed_var(dsdgp_ctx* ctx, int32_t M, int64_t ns, int32_t DY, const double* tmp1, int64_t ld1, const double* tmp2,
                                   int64_t ld2, double kdiag, double* var) {
  DS_CHECK_ARG(ctx && tmp1 && tmp2 && var);
  DS_CHECK_ARG(M >= 1 && ns >= 1 && DY >= 1 && ld1 >= ns && ld2 >= ns);
  DS_LAUNCH(k_collapsed_var, dim3(ceil_div(ns, CL_T)), dim3(CL_T), 0, ctx->stream, (int)M, ns, (int)DY, tmp1, ld1, tmp2, ld2, kdiag, var);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// The per-row tables of the RBF kernel expectations, shared by the forward (psi.hip) and its reverse pass (psi_grad.hip):
// k_psi_rows writes w1 = 1 / (l^2 + s), w2 = 1 / (l^2 + 2 s), t = (w2 - l^-2) / 4 and the log-prefactors h1, h2 of every row,
// k_psi_cross the n x M table L_ri = -1/2 sum_d w2_rd (mu_rd - z_id)^2 together with psi1.  The notation is that of psi.hip's header.
#pragma once
#include <math.h>

#include "common.hpp"

#define PS_MAX_M 2048
#define PS_MAX_D 1024
#define PS_T 256
#define PS_TILE 16          // tile edge of psi2
#define PS_KC 32            // input dimensions per chunk of the delta^2 operand (8 MFMA k-steps)
#define PS_TARGET_WG 4096
#define PS_MIN_ROWS 64      // fewest rows worth a split
#define PS_SCRATCH_CAP ((size_t)8 << 30)

// one thread per row: w1 = 1 / (l^2 + s), w2 = 1 / (l^2 + 2 s), t = (w2 - l^-2) / 4 (columns D .. Dq - 1 zero), h1, h2
static __global__ __launch_bounds__(PS_T) void k_psi_rows(const double* __restrict__ s, const double* __restrict__ ls2, int64_t n, int D,
                                                          int Dq, double variance, double* __restrict__ W1, double* __restrict__ W2,
                                                          double* __restrict__ T, double* __restrict__ H1, double* __restrict__ H2,
                                                          double* __restrict__ psi0) {
  const int64_t r = (int64_t)blockIdx.x * PS_T + threadIdx.x;
  if (r == 0 && psi0) psi0[0] = (double)n * variance;
  if (r >= n) return;
  double h1 = 0.0, h2 = 0.0;
  for (int d = 0; d < D; ++d) {
    const double l2 = ls2[d], sv = s ? s[r * D + d] : 0.0;
    const double w1 = 1.0 / (l2 + sv), w2 = 1.0 / (l2 + 2.0 * sv);
    W1[r * D + d] = w1;
    W2[r * D + d] = w2;
    T[r * Dq + d] = 0.25 * (w2 - 1.0 / l2);
    h1 += log(l2 * w1);
    h2 += log(l2 * w2);
  }
  for (int d = D; d < Dq; ++d) T[r * Dq + d] = 0.0;
  H1[r] = 0.5 * h1;
  H2[r] = 0.5 * h2;
}

// entry (r, i): psi1 = v exp(h1_r - 1/2 sum_d w1_rd (mu_rd - z_id)^2),  L = -1/2 sum_d w2_rd (mu_rd - z_id)^2
static __global__ __launch_bounds__(PS_T) void k_psi_cross(const double* __restrict__ mu, const double* __restrict__ Z,
                                                           const double* __restrict__ W1, const double* __restrict__ W2,
                                                           const double* __restrict__ H1, int64_t n, int M, int D, double variance,
                                                           double* __restrict__ psi1, int64_t ld1, double* __restrict__ Ltab) {
  const int64_t total = n * M, stride = (int64_t)gridDim.x * PS_T;
  for (int64_t e = (int64_t)blockIdx.x * PS_T + threadIdx.x; e < total; e += stride) {
    const int64_t r = e / M;
    const int i = (int)(e - r * M);
    const double *pm = mu + r * D, *pz = Z + (int64_t)i * D, *p1 = W1 + r * D, *p2 = W2 + r * D;
    double a1 = 0.0, a2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = pm[d] - pz[d], q = df * df;
      a1 = fma(p1[d], q, a1);
      a2 = fma(p2[d], q, a2);
    }
    if (psi1) psi1[r * ld1 + i] = variance * exp(H1[r] - 0.5 * a1);
    if (Ltab) Ltab[e] = -0.5 * a2;
  }
}

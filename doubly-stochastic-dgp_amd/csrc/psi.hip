// Expectations of the RBF kernel under a diagonal Gaussian input (the psi statistics): GPflow 1.1.1's
// expectation(DiagonalGaussian, (RBF, InducingPoints)[, (RBF, InducingPoints)]) as the reference's collapsed layers call it
// (layers.py:415-417, 494-495).  mu, s: n x D means and variances (s == NULL: zero), Z: M x D, kernel variance v, lengthscales l_d.
//   psi0       = n v
//   psi1[r, i] = v prod_d (l_d^2 / (l_d^2 + s_rd))^1/2 exp(-1/2 sum_d (mu_rd - z_id)^2 / (l_d^2 + s_rd))
//   psi2[i, j] = sum_r v^2 prod_d (l_d^2 / (l_d^2 + 2 s_rd))^1/2 exp(-sum_d [(z_id - z_jd)^2 / (4 l_d^2) + (mu_rd - (z_id + z_jd) / 2)^2 / (l_d^2 + 2 s_rd)])
//
// Every exponent is formed from differences, never from an expanded square.  With w_rd = 1 / (l_d^2 + 2 s_rd) the exponent of psi2 is
//   E_rij = h_r + L_ri + L_rj + sum_d t_rd (z_id - z_jd)^2,    h_r = 1/2 sum_d log(l_d^2 w_rd),  L_ri = -1/2 sum_d w_rd (mu_rd - z_id)^2,
//   t_rd = (w_rd - l_d^-2) / 4
// (for s >= 0 every term is <= 0: nothing overflows, a far pair underflows to +0).  k_psi_rows writes the per-row tables (w, t, h),
// k_psi_cross the n x M table L together with psi1 (same form with w = 1 / (l^2 + s)) — both launched by psi_front, the front end this
// call shares with its reverse pass (psi_tables.hpp) — and k_psi2 — the hot path, n M (M + 1) / 2 exponentials — sums exp(E) over the
// rows.  The row splits and the scratch layout are psi_plan.hpp's.
//
// k_psi2.  Only the 16 x 16 tiles (I, J), I >= J, on or below the diagonal are formed.  A workgroup of four waves owns a tile and a split
// of the rows; wave w owns the tile rows i = w, w + 4, w + 8, w + 12 and all 16 columns j.  sum_d t_rd delta_ijd^2 is a small-K product
// (16 rows of t) x (delta^2 of 16 pairs) on v_mfma_f64_16x16x4_f64: lane (g, c) holds delta^2 of pair (i, j = c) for the input
// dimensions k0 + 4 ks + g of a chunk of PS_KC = 32 dimensions in registers — for D <= 32 they are computed once per workgroup, for a
// wider input once per chunk and block of 16 rows — the A operand is read from the t table (row stride D rounded up to 4, zero pad),
// and result register u of the accumulator is row g + 4 u of the block, column j = c.  The vector pipe is left for the exponentials.
// Rows past the end of a split are loaded from a clamped address and their terms replaced by zero: no branch around a load, and a NaN
// row (l^2 + 2 s < 0, as upstream's sqrt gives it) reaches exactly the entries it feeds.  A lane adds its rows in ascending order, the
// four 16-lane groups are combined by sum_groups; a split writes its partial tile, k_psi2_reduce adds the partials in ascending split
// order, scales by v^2 and writes the entry and its mirror image (a diagonal tile is mirrored from its lower half: psi2 is exactly
// symmetric).  No floating-point atomics: the summation order depends on (n, M, D) alone.
#include "psi_tables.hpp"      // the front end and the plan, shared with psi_grad.hip

// one thread per row: w1 = 1 / (l^2 + s), w2 = 1 / (l^2 + 2 s), t = (w2 - l^-2) / 4 (columns D .. Dq - 1 zero), h1, h2
__global__ __launch_bounds__(PS_T) void k_psi_rows(const double* __restrict__ s, const double* __restrict__ ls2, int64_t n, int D, int Dq,
                                                   double variance, double* __restrict__ W1, double* __restrict__ W2,
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
__global__ __launch_bounds__(PS_T) void k_psi_cross(const double* __restrict__ mu, const double* __restrict__ Z,
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

// tile t of the lower triangle -> (I, J), I >= J
__device__ __forceinline__ void ps_tile(int t, int& I, int& J) {
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  J = t - I * (I + 1) / 2;
}

// part[(split * ntiles + tile) * 256 + il * 16 + jl] = sum over the split's rows of exp(E_rij), i = I 16 + il, j = J 16 + jl
__global__ __launch_bounds__(PS_T) void k_psi2(const double* __restrict__ Z, const double* __restrict__ T, const double* __restrict__ H2,
                                               const double* __restrict__ Ltab, int64_t n, int M, int D, int Dq, int64_t rows_per_split,
                                               double* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, w = DS_WAVE_ID(tid);
  const int g = lane >> 4, c = lane & 15;
  int I, J;
  ps_tile(blockIdx.x, I, J);
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < n ? r0 + rows_per_split : n;
  // entries past M compute a copy of row / column M - 1; the reduction never reads them
  const int jc = J * PS_TILE + c < M ? J * PS_TILE + c : M - 1;
  int ic[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) ic[q] = I * PS_TILE + w + 4 * q < M ? I * PS_TILE + w + 4 * q : M - 1;
  const int nch = (Dq + PS_KC - 1) / PS_KC;
  double b[4][PS_KC / 4];
  // delta^2 of the pairs (ic[q], jc) for the dimensions k0 + 4 ks + g; zero past D
  auto load_b = [&](int k0) {
#pragma unroll
    for (int ks = 0; ks < PS_KC / 4; ++ks) {
      const int d = k0 + 4 * ks + g, dc = d < D ? d : D - 1;
      const double zj = Z[(int64_t)jc * D + dc];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double df = Z[(int64_t)ic[q] * D + dc] - zj;
        b[q][ks] = d < D ? df * df : 0.0;
      }
    }
  };
  if (nch == 1) load_b(0);
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t n0 = r0; n0 < r1; n0 += 16) {
    d4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    const int64_t ra = n0 + c < n ? n0 + c : n - 1;      // A operand: row n0 + c of t, dimension k0 + 4 ks + g
    const double* ta = T + ra * Dq + g;
    for (int ch = 0; ch < nch; ++ch) {
      const int k0 = ch * PS_KC;
      if (nch > 1) load_b(k0);
#pragma unroll
      for (int ks = 0; ks < PS_KC / 4; ++ks) {
        if (k0 + 4 * ks < Dq) {
          const double a = ta[k0 + 4 * ks];
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] = mfma_f64(a, b[q][ks], acc[q]);
        }
      }
    }
    // accumulator q, register u: row n0 + g + 4 u, pair (ic[q], jc)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t row = n0 + g + 4 * u;
      const bool in = row < r1;
      const int64_t rc = row < n ? row : n - 1;
      const double* lr = Ltab + rc * M;
      const double hj = H2[rc] + lr[jc];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double v = exp(hj + lr[ic[q]] + acc[q][u]);
        sum[q] += in ? v : 0.0;
      }
    }
  }
  double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PS_TILE * PS_TILE);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double tot = sum_groups(sum[q]);
    if (g == 0) out[(w + 4 * q) * PS_TILE + c] = tot;
  }
}

// psi2[i][j] = psi2[j][i] = v^2 x (the partials in ascending split order), for the entries i >= j of the lower tiles
__global__ __launch_bounds__(PS_T) void k_psi2_reduce(const double* __restrict__ part, int nsplit, int ntiles, int M, double var2,
                                                      double* __restrict__ psi2, int64_t ld2) {
  int I, J;
  ps_tile(blockIdx.x, I, J);
  const int e = threadIdx.x;
  const int i = I * PS_TILE + e / PS_TILE, j = J * PS_TILE + e % PS_TILE;
  if (i >= M || j > i) return;
  const double* p = part + (int64_t)blockIdx.x * (PS_TILE * PS_TILE) + e;
  double s = 0.0;
  for (int b = 0; b < nsplit; ++b) s += p[(int64_t)b * ntiles * (PS_TILE * PS_TILE)];
  const double v = var2 * s;
  psi2[(int64_t)i * ld2 + j] = v;
  psi2[(int64_t)j * ld2 + i] = v;
}

int psi_front(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* mu, const double* s, int64_t n,
              bool reverse, bool want1, bool want2, bool want_dZ, const std::function<int()>& own_checks, const char* scope,
              double* psi0, double* psi1, int64_t ld1, PsiFront& F) {
  DS_CHECK_ARG(ctx && kern && Z && mu);
  if (kern->kind != DSDGP_KERN_RBF || kern->has_white) {
    dsdgp_set_error("%s:%d: the kernel expectations have a closed form for a plain RBF kernel only (kind %d, has_white %d)", __FILE__,
                    __LINE__, kern->kind, kern->has_white);
    return DSDGP_ERR_UNSUPPORTED;
  }
  DS_CHECK_ARG(M >= 1 && M <= PS_MAX_M);
  DS_CHECK_ARG(n >= 1 && n <= 0x7fffffff);
  DS_CHECK_ARG(kern->input_dim >= 1 && kern->input_dim <= PS_MAX_D && kern->lengthscales);
  DS_TRY(own_checks());
  const int D = kern->input_dim, nl = reverse ? 2 : 1;
  const PsiPlan& P = F.plan = reverse ? psi_plan_reverse(n, M, D, want1, want2, want_dZ) : psi_plan_forward(n, M, D, want2);
  if (P.total > PS_SCRATCH_CAP) {
    dsdgp_set_error("%s:%d: the row tables of n = %lld, M = %d, D = %d need %zu bytes of scratch, above the cap of %zu: pass the rows in "
                    "batches and add the results", __FILE__, __LINE__, (long long)n, M, D, P.total, PS_SCRATCH_CAP);
    return DSDGP_ERR_UNSUPPORTED;
  }
  DS_TRY(ctx_scratch(ctx, P.total, (void**)&F.base));
  F.ls2 = F.at(P.ls), F.W1 = F.at(P.W1), F.W2 = F.at(P.W2), F.T = F.at(P.T), F.H1 = F.at(P.H1), F.H2 = F.at(P.H2), F.Ltab = F.at(P.L);
  if (reverse) psi1 = F.at(P.A), ld1 = M;
  std::vector<double> l2(nl * D);
  for (int d = 0; d < D; ++d) {
    const double l = kern->lengthscales[kern->ard ? d : 0];
    l2[d] = l * l;
    if (reverse) l2[D + d] = l;
  }
  DS_TRY(ctx_upload(ctx, F.ls2, l2.data(), (size_t)nl * D * 8));
  const double v = kern->variance;
  F.prof.emplace(ctx, scope);
  DS_LAUNCH(k_psi_rows, dim3(ceil_div(n, PS_T)), dim3(PS_T), 0, ctx->stream, s, F.ls2, n, D, P.Dq, v, F.W1, F.W2, F.T, F.H1, F.H2, psi0);
  if (want1 || want2) {
    const int64_t blocks = std::min<int64_t>(((int64_t)n * M + PS_T - 1) / PS_T, 1 << 20);
    DS_LAUNCH(k_psi_cross, dim3((unsigned)blocks), dim3(PS_T), 0, ctx->stream, mu, Z, F.W1, F.W2, F.H1, n, (int)M, D, v, psi1, ld1, F.Ltab);
  }
  return DSDGP_OK;
}

extern "C" int dsdgp_rbf_expectations(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* mu,
                                      const double* s, int64_t n, double* psi0, double* psi1, int64_t ld1, double* psi2, int64_t ld2) {
  PsiFront F;
  auto own_checks = [&]() -> int {
    DS_CHECK_ARG(!psi1 || ld1 >= M);
    DS_CHECK_ARG(!psi2 || ld2 >= M);
    return DSDGP_OK;
  };
  DS_TRY(psi_front(ctx, kern, Z, M, mu, s, n, false, psi1, psi2, false, own_checks, "psi", psi0, psi1, ld1, F));
  if (psi2) {
    const PsiPlan& P = F.plan;
    const double v = kern->variance;
    double* part = F.at(P.part);
    {
      ProfScope p2(ctx, "psi2");
      DS_LAUNCH(k_psi2, dim3(P.ntiles, P.nsplit), dim3(PS_T), 0, ctx->stream, Z, F.T, F.H2, F.Ltab, n, (int)M, kern->input_dim, P.Dq,
                P.rows_per_split, part);
    }
    DS_LAUNCH(k_psi2_reduce, dim3(P.ntiles), dim3(PS_T), 0, ctx->stream, part, P.nsplit, P.ntiles, (int)M, v * v, psi2, ld2);
  }
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

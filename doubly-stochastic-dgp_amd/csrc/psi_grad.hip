// Reverse pass of the RBF kernel expectations (psi.hip): given the adjoints g_psi0, g_psi1 (n x M), g_psi2 (M x M) of
//   psi0 = n v,  psi1[r, i],  psi2[i, j] = sum_r v^2 exp(E_rij)
// the adjoints of mu, s (n x D), Z (M x D), the kernel variance v and the lengthscales l_d.  Notation of psi.hip:
//   l2 = l^2,  w1 = 1 / (l2 + s),  w2 = 1 / (l2 + 2 s),  t = (w2 - 1 / l2) / 4,  delta_rid = mu_rd - z_id,  Delta_ijd = z_id - z_jd,
//   E_rij = h_r + L_ri + L_rj + sum_d t_rd Delta_ijd^2  (the forward's exponent, from the forward's own row tables: psi_front, psi.hip).
// psi1 part, A_ri = g_psi1_ri psi1_ri, a1_r = sum_i A_ri;  psi2 part, Gs = (g_psi2 + g_psi2^T) / 2, Q_rij = Gs_ij v^2 exp(E_rij),
//   q_ri = sum_j Q_rij,  a_r = sum_i q_ri,  P_rd = sum_ij Q_rij Delta_ijd^2,  S_id = sum_j Delta_ijd sum_r Q_rij t_rd:
//   d_mu_rd = -w1 sum_i A delta - 2 w2 sum_i q delta
//   d_Z_id  = sum_r A w1 delta + 2 sum_r q w2 delta + 4 S_id
//   dW1_rd  = a1 / (2 w1) - 1/2 sum_i A delta^2,     dW2_rd = a / (2 w2) - sum_i q delta^2 + P / 4
//   d_s_rd  = -w1^2 dW1 - 2 w2^2 dW2
//   d_l2_d  = sum_r (-w1^2 dW1 + a1 / (2 l2)) + sum_r (-w2^2 dW2 + a / (2 l2) + P / (4 l2^2)),   d_l_d = 2 l_d d_l2_d
//   d_v     = n g_psi0 + sum_r (a1_r + 2 a_r) / v
// Every difference is formed as a difference of the inputs, never from an expanded square.
//
// k_psi2_grad — the hot path, n M^2 fp64 exponentials.  A workgroup of four waves owns a tile ROW I (16 inducing inputs i) and a split
// of the rows r, and walks EVERY tile column J: twice the exponentials of the forward's lower triangle, and in return q_ri is complete
// when the walk of a block of 16 rows ends (no partial q per tile column, 8 n M^2 / 16 bytes, is written and read back), and the
// i side of every pair is the only side a workgroup feeds.  Wave w owns i = I 16 + w + 4 q, q < 4.  The exponent's product runs with
// the forward's operands SWAPPED, delta^2 of the pair as the A operand and the row of t as the B operand, so that the result register u
// of lane (g, c) is pair (i_q, j = J 16 + g + 4 u) of row n0 + c: Q in that layout IS the B operand (k = the 16 columns j, n = the row)
// of the two small-K products that follow, without a round trip through the LDS:
//   P^T[d][row]   += Delta^2[(i_q, j)][d] Q[(i_q, j)][row]      summed over the wave's 64 pairs and over J      (one accumulator)
//   V_q^T[d][row] += Delta  [(i_q, j)][d] Q[(i_q, j)][row]      summed over j and over J                        (one per q)
// with d = 16 db + c of the A operand, db < NDB = 1 (D <= 16) or 2 (D <= 32).  When the walk of a row block ends, q_ri = the sum of
// Q over u and J in the lane, then over the four 16-lane groups (sum_groups), is written; P^T is added over the four waves through the
// LDS in ascending wave order and written as the partial of tile row I; S_id += V_q^T[d][row] t[row][d] stays in registers across
// the row blocks and is added over the 16 lanes of a row by a fixed butterfly at the end of the split.  Rows past the end of a split
// and entries past M are loaded from a clamped address and their Q replaced by zero (no branch around a load; a NaN row — l^2 + 2 s < 0
// — reaches its own column of the products only, so its own rows of q and P and every sum over rows).  k_psig_row adds the partials
// of P in ascending I and forms d_mu, d_s and each row's term of d_l2 and d_v (one thread per (r, d), i ascending); k_psig_z forms the
// O(n M D) part of d_Z over chunks of rows (r ascending); k_psig_zsum adds the chunks, then the splits of S, in ascending order;
// k_psig_kern (one workgroup) sums the rows' terms of d_v and d_l2 (a thread its rows in ascending order, then a fixed tree).  No
// floating-point atomics: every summation order depends on (n, M, D) alone.
#include "psi_tables.hpp"      // psi_front: the checks, the plan (psi_plan.hpp) and the forward's row tables

// Gs[i][j] = v^2 (g[i][j] + g[j][i]) / 2
__global__ __launch_bounds__(PS_T) void k_psig_sym(const double* __restrict__ g, int64_t ldg, int M, double var2, double* __restrict__ Gs) {
  const int e = blockIdx.x * PS_T + threadIdx.x;
  if (e >= M * M) return;
  const int i = e / M, j = e - i * M;
  Gs[e] = var2 * (0.5 * (g[(int64_t)i * ldg + j] + g[(int64_t)j * ldg + i]));
}

template <int NDB>
__global__ __launch_bounds__(PS_T) void k_psi2_grad(const double* __restrict__ Z, const double* __restrict__ T, const double* __restrict__ H2,
                                                    const double* __restrict__ Ltab, const double* __restrict__ Gs, int64_t n, int M, int D,
                                                    int Dq, int64_t rows_per_split, double* __restrict__ qout, double* __restrict__ Ppart,
                                                    double* __restrict__ Spart) {
  __shared__ double pl[4][NDB * 4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = DS_WAVE_ID(tid);
  const int g = lane >> 4, c = lane & 15;
  const int I = blockIdx.x, nt1 = gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < n ? r0 + rows_per_split : n;
  int ic[4];
  bool iv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = I * PS_TILE + w + 4 * q;
    iv[q] = i < M;
    ic[q] = iv[q] ? i : M - 1;
  }
  // z_i at the dimensions d = 16 db + c of the A operand of the P and V products
  int dpc[NDB];
  bool dpv[NDB];
  double zi[4][NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    const int d = 16 * db + c;
    dpv[db] = d < D;
    dpc[db] = dpv[db] ? d : D - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) zi[q][db] = Z[(int64_t)ic[q] * D + dpc[db]];
  }
  d4 Sacc[4][NDB];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int db = 0; db < NDB; ++db) Sacc[q][db] = d4{0.0, 0.0, 0.0, 0.0};

  for (int64_t n0 = r0; n0 < r1; n0 += 16) {
    const int64_t row = n0 + c;
    const bool in = row < r1;
    const int64_t rc = row < n ? row : n - 1;
    const double* lr = Ltab + rc * M;
    const double* tr = T + rc * Dq;
    const double hrow = H2[rc];
    double hi[4], qacc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hi[q] = hrow + lr[ic[q]];
      qacc[q] = 0.0;
    }
    d4 Pacc[NDB], Vacc[4][NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      Pacc[db] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) Vacc[q][db] = d4{0.0, 0.0, 0.0, 0.0};
    }
    for (int J = 0; J < nt1; ++J) {
      // sum_d t_rd Delta_ijd^2: A = Delta^2 of pair (i_q, j = J 16 + c) at d = 4 ks + g, B = row n0 + c of t at d = 4 ks + g
      d4 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
      const int ja = J * PS_TILE + c < M ? J * PS_TILE + c : M - 1;
#pragma unroll
      for (int ks = 0; ks < PG_MAX_D / 4; ++ks) {
        if (4 * ks < Dq) {
          const int d = 4 * ks + g, dc = d < D ? d : D - 1;
          const double tb = tr[d];
          const double zj = Z[(int64_t)ja * D + dc];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double df = Z[(int64_t)ic[q] * D + dc] - zj;
            acc[q] = mfma_f64(d < D ? df * df : 0.0, tb, acc[q]);
          }
        }
      }
      // Q of pair (i_q, j = J 16 + g + 4 u), row n0 + c; then the two products with Q as the B operand of k-step (q, u)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = J * PS_TILE + g + 4 * u;
        const bool jv = j < M;
        const int jc = jv ? j : M - 1;
        const double lj = lr[jc];
        double zj[NDB];
#pragma unroll
        for (int db = 0; db < NDB; ++db) zj[db] = Z[(int64_t)jc * D + dpc[db]];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double ex = exp(hi[q] + lj + acc[q][u]);
          const double gs = Gs[(int64_t)ic[q] * M + jc];
          const double Q = in && iv[q] && jv ? gs * ex : 0.0;
          qacc[q] += Q;
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const double df = dpv[db] ? zi[q][db] - zj[db] : 0.0;
            Pacc[db] = mfma_f64(df * df, Q, Pacc[db]);
            Vacc[q][db] = mfma_f64(df, Q, Vacc[q][db]);
          }
        }
      }
    }
    // q_ri: the lane's sum over u and J, then over the four groups g
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double tot = sum_groups(qacc[q]);
      if (g == 0 && in && iv[q]) qout[row * M + ic[q]] = tot;
    }
    // result register u of P^T and V^T: d = 16 db + g + 4 u, row n0 + c
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int d = 16 * db + g + 4 * u;
        const double tv = in && d < D ? tr[d < Dq ? d : 0] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) Sacc[q][db][u] = fma(Vacc[q][db][u], tv, Sacc[q][db][u]);
        pl[w][db * 4 + u][lane] = Pacc[db][u];
      }
    __syncthreads();
    // entry (db, u) of lane `lane`, the four waves in ascending order: thread tid takes u = w
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int k = db * 4 + w, d = 16 * db + g + 4 * w;
      const double tot = ((pl[0][k][lane] + pl[1][k][lane]) + pl[2][k][lane]) + pl[3][k][lane];
      if (in && d < D) Ppart[((int64_t)I * n + row) * D + d] = tot;
    }
    __syncthreads();
  }
  if (!Spart) return;
  // S_id, i = i_q, d = 16 db + g + 4 u: the sum over the 16 lanes (rows) of a group by a fixed butterfly
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double x = Sacc[q][db][u];
        x += __shfl_xor(x, 1, 16);
        x += __shfl_xor(x, 2, 16);
        x += __shfl_xor(x, 4, 16);
        x += __shfl_xor(x, 8, 16);
        const int d = 16 * db + g + 4 * u;
        if (c == 0 && iv[q] && d < D) Spart[((int64_t)blockIdx.y * M + ic[q]) * D + d] = x;
      }
}

// one thread per (r, d): the sums over i (ascending), the partials of P (ascending I), d_mu, d_s, the row's term C of d_l2_d and AV of d_v
__global__ __launch_bounds__(PS_T) void k_psig_row(const double* __restrict__ mu, const double* __restrict__ Z, const double* __restrict__ W1,
                                                   const double* __restrict__ W2, const double* __restrict__ ls2,
                                                   const double* __restrict__ psi1, const double* __restrict__ g1, int64_t ldg1,
                                                   const double* __restrict__ qv, const double* __restrict__ Ppart, int nt1, int64_t n,
                                                   int M, int D, double* __restrict__ d_mu, double* __restrict__ d_s,
                                                   double* __restrict__ Crow, double* __restrict__ AV) {
  const int64_t e = (int64_t)blockIdx.x * PS_T + threadIdx.x;
  if (e >= n * D) return;
  const int64_t r = e / D;
  const int d = (int)(e - r * D);
  const double m = mu[e], w1 = W1[e], w2 = W2[e], l2 = ls2[d];
  double a1 = 0.0, s1 = 0.0, s1q = 0.0, a2 = 0.0, s2 = 0.0, s2q = 0.0, P = 0.0;
  if (psi1) {
    const double *pa = psi1 + r * M, *pg = g1 + r * ldg1;
    for (int i = 0; i < M; ++i) {
      const double df = m - Z[(int64_t)i * D + d], A = pg[i] * pa[i];
      a1 += A;
      s1 = fma(A, df, s1);
      s1q = fma(A, df * df, s1q);
    }
  }
  if (qv) {
    const double* pq = qv + r * M;
    for (int i = 0; i < M; ++i) {
      const double df = m - Z[(int64_t)i * D + d], q = pq[i];
      a2 += q;
      s2 = fma(q, df, s2);
      s2q = fma(q, df * df, s2q);
    }
    for (int I = 0; I < nt1; ++I) P += Ppart[((int64_t)I * n + r) * D + d];
  }
  const double dW1 = a1 / (2.0 * w1) - 0.5 * s1q;
  const double dW2 = (a2 / (2.0 * w2) - s2q) + 0.25 * P;
  const double u1 = -(w1 * w1) * dW1, u2 = -(w2 * w2) * dW2;
  if (d_mu) d_mu[e] = -(w1 * s1) - 2.0 * (w2 * s2);
  if (d_s) d_s[e] = u1 + 2.0 * u2;
  Crow[e] = (u1 + a1 / (2.0 * l2)) + ((u2 + a2 / (2.0 * l2)) + P / (4.0 * l2 * l2));
  if (d == 0) AV[r] = a1 + 2.0 * a2;
}

// Zpart[chunk][i][d] = sum over the chunk's rows (ascending) of A_ri w1_rd delta_rid + 2 q_ri w2_rd delta_rid; thread (d, i), i fastest
__global__ __launch_bounds__(PS_T) void k_psig_z(const double* __restrict__ mu, const double* __restrict__ Z, const double* __restrict__ W1,
                                                 const double* __restrict__ W2, const double* __restrict__ psi1,
                                                 const double* __restrict__ g1, int64_t ldg1, const double* __restrict__ qv, int64_t n, int M,
                                                 int D, int64_t rows_per_chunk, double* __restrict__ Zpart) {
  const int e = blockIdx.x * PS_T + threadIdx.x;
  if (e >= M * D) return;
  const int d = e / M, i = e - d * M;
  const int64_t ra = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t rb = ra + rows_per_chunk < n ? ra + rows_per_chunk : n;
  const double z = Z[(int64_t)i * D + d];
  double x1 = 0.0, x2 = 0.0;
  for (int64_t r = ra; r < rb; ++r) {
    const double df = mu[r * D + d] - z;
    if (psi1) x1 = fma(g1[r * ldg1 + i] * psi1[r * M + i], W1[r * D + d] * df, x1);
    if (qv) x2 = fma(qv[r * M + i], W2[r * D + d] * df, x2);
  }
  Zpart[((int64_t)blockIdx.y * M + i) * D + d] = x1 + 2.0 * x2;
}

// d_Z[i][d] = (the chunks in ascending order) + 4 (the splits of S in ascending order)
__global__ __launch_bounds__(PS_T) void k_psig_zsum(const double* __restrict__ Zpart, int nchunk, const double* __restrict__ Spart, int nsplit,
                                                    int M, int D, double* __restrict__ d_Z) {
  const int e = blockIdx.x * PS_T + threadIdx.x;
  if (e >= M * D) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nchunk; ++k) a += Zpart[(int64_t)k * M * D + e];
  if (Spart)
    for (int k = 0; k < nsplit; ++k) b += Spart[(int64_t)k * M * D + e];
  d_Z[e] = a + 4.0 * b;
}

// one workgroup: d_kern[0] = n g_psi0 + sum_r AV_r / v;  d_kern[1 + d] = 2 l_d sum_r C_rd (added over d, ascending, without ARD)
__global__ __launch_bounds__(PS_T) void k_psig_kern(const double* __restrict__ Crow, const double* __restrict__ AV,
                                                    const double* __restrict__ ls, int64_t n, int D, int ard, double variance, double g0,
                                                    double* __restrict__ d_kern) {
  __shared__ double red[PS_T];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t r = tid; r < n; r += PS_T) a += AV[r];
  a = block_sum<PS_T>(a, red);
  if (tid == 0) d_kern[0] = (double)n * g0 + a / variance;
  double tot = 0.0;
  for (int d = 0; d < D; ++d) {
    double x = 0.0;
    for (int64_t r = tid; r < n; r += PS_T) x += Crow[r * D + d];
    x = block_sum<PS_T>(x, red);
    const double dl = 2.0 * ls[d] * x;
    if (ard) {
      if (tid == 0) d_kern[1 + d] = dl;
    } else {
      tot += dl;
    }
  }
  if (!ard && tid == 0) d_kern[1] = tot;
}

extern "C" int dsdgp_rbf_expectations_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* mu,
                                           const double* s, int64_t n, double g_psi0, const double* g_psi1, int64_t ldg1,
                                           const double* g_psi2, int64_t ldg2, double* d_mu, double* d_s, double* d_Z, double* d_kern) {
  PsiFront F;
  auto own_checks = [&]() -> int {
    DS_CHECK_ARG(!g_psi1 || ldg1 >= M);
    DS_CHECK_ARG(!g_psi2 || ldg2 >= M);
    if (kern->input_dim > PG_MAX_D) {
      dsdgp_set_error("%s:%d: the reverse pass of the kernel expectations takes input_dim <= %d (one chunk of the forward's operand), "
                      "not %d", __FILE__, __LINE__, PG_MAX_D, kern->input_dim);
      return DSDGP_ERR_UNSUPPORTED;
    }
    return DSDGP_OK;
  };
  DS_TRY(psi_front(ctx, kern, Z, M, mu, s, n, true, g_psi1, g_psi2, d_Z, own_checks, "psi_grad", nullptr, nullptr, 0, F));
  hipStream_t st = ctx->stream;
  const PsiPlan& P = F.plan;
  const int D = kern->input_dim, nt1 = P.nt1;
  const double v = kern->variance;
  double *ls = F.ls2 + D, *A = F.at(P.A), *qv = F.at(P.q), *Gs = F.at(P.Gs), *Ppart = F.at(P.Ppart), *Spart = F.at(P.Spart);
  double *Zpart = F.at(P.Zpart), *Crow = F.at(P.Crow), *AV = F.at(P.AV);
  if (g_psi2) {
    DS_LAUNCH(k_psig_sym, dim3(ceil_div(M * M, PS_T)), dim3(PS_T), 0, st, g_psi2, ldg2, (int)M, v * v, Gs);
    ProfScope p2(ctx, "psi2_grad");
    if (D <= 16)
      DS_LAUNCH(k_psi2_grad<1>, dim3(nt1, P.g_nsplit), dim3(PS_T), 0, st, Z, F.T, F.H2, F.Ltab, Gs, n, (int)M, D, P.Dq, P.g_rows_per_split, qv,
                Ppart, Spart);
    else
      DS_LAUNCH(k_psi2_grad<2>, dim3(nt1, P.g_nsplit), dim3(PS_T), 0, st, Z, F.T, F.H2, F.Ltab, Gs, n, (int)M, D, P.Dq, P.g_rows_per_split, qv,
                Ppart, Spart);
  }
  if (d_mu || d_s || d_kern)
    DS_LAUNCH(k_psig_row, dim3(ceil_div(n * D, PS_T)), dim3(PS_T), 0, st, mu, Z, F.W1, F.W2, F.ls2, A, g_psi1, ldg1, qv, Ppart, nt1, n, (int)M, D,
              d_mu, d_s, Crow, AV);
  if (d_Z) {
    DS_LAUNCH(k_psig_z, dim3(ceil_div(M * D, PS_T), P.nchunk), dim3(PS_T), 0, st, mu, Z, F.W1, F.W2, A, g_psi1, ldg1, qv, n, (int)M, D,
              P.rows_per_chunk, Zpart);
    DS_LAUNCH(k_psig_zsum, dim3(ceil_div(M * D, PS_T)), dim3(PS_T), 0, st, Zpart, P.nchunk, Spart, P.g_nsplit, (int)M, D, d_Z);
  }
  if (d_kern) DS_LAUNCH(k_psig_kern, dim3(1), dim3(PS_T), 0, st, Crow, AV, ls, n, D, kern->ard ? 1 : 0, v, g_psi0, d_kern);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

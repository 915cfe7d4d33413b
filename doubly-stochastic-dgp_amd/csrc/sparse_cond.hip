// The sparse conditional without q_sqrt and its reverse pass: the reference's SVGP conditional (layers.py:178-219) on the branch
// `q_sqrt is None` (layers.py:200), which is all of its SGPMC_Layer (layers.py:249-260).  With
//   Ku = K(Z, Z) + jitter I (the White part on the diagonal),  Lu = chol(Ku),  A = Lu^-1 K(Z, X) (M x n),
//   W = q_mu (white) or Lu^-1 q_mu,  kd = variance + White variance:
//   mean = A^T W (n x DO),   var_r = kd - sum_i A_ir^2 (n; the same for every output).
// Reverse, given gm = dJ/dmean (n x DO) and gv = dJ/dvar summed over the outputs (n):
//   A_bar = W gm^T - 2 A diag(gv),  W_bar = A gm,  K1_bar = Lu^-T A_bar,
//   Lu_bar = -tril(K1_bar A^T) [- tril((Lu^-T W_bar) W^T) when not white],  q_mu_bar = W_bar (white) or Lu^-T W_bar,
//   Ku_bar = Lu^-T 1/2 (P + P^T) Lu^-1 with P = Phi(Lu^T Lu_bar), Phi the lower triangle with a halved diagonal,  kd_bar = sum_r gv_r,
// and K1_bar, Ku_bar reach Z, X and the kernel through dsdgp_gram_grad (cross form with G = K1_bar, symmetric form with G = Ku_bar).
//
// Composed from the library's own calls: dsdgp_gram, dsdgp_potrf, dsdgp_trsm, dsdgp_gemm, dsdgp_scale_copy, dsdgp_gram_grad.  They use the
// context's scratch from its first byte, each of them, so this call's own intermediates live in a block the CALLER holds.  The two Gram
// calls see Z and X moved to Z's first row as origin (k_sc_center): the kernels depend on differences only.  New here are the
// passes over the M x n matrix A, which dominate the traffic (41 MB at M = 128, n = 40 000):
// k_sc_fwd: a workgroup owns a tile of SC_CT columns of A and walks its rows in blocks of SC_KC, staged coalesced in the LDS (clamped
//   addresses, +0.0 outside the matrix).  One read gives both results: wave w forms the 16 rows of `mean` of its 16 columns on the fp64
//   MFMA pipe (D rows = data rows, D columns = outputs in chunks of 16, k = the rows of A in ascending order), and the threads of wave 0
//   add A^2 down their column in ascending i.
// k_sc_adj: workgroup (s, c) walks the tiles of row split s for the rows of chunk c.  From one staged block of A it writes the block of
//   A_bar (MFMA over the outputs, four at a time in ascending order, then - 2 A gv) and adds the block's A gm into its partial of W_bar
//   (MFMA, k = the data rows in ascending order).  k_sc_wsum adds the partials in ascending split order.
// k_sc_tril (Lu_bar = -tril(T)), k_sc_phi (S_ij = 1/2 Q[max(i, j)][min(i, j)]: Phi and the symmetrisation at once) and k_sc_final (the
//   two Gram reverse passes' results added, kd_bar by a fixed tree) are element-wise.
// No floating-point atomics; every summation order follows from sparse_cond_plan.hpp, that is from (n, M, D, DO) alone.
#include "common.hpp"
#include "gram_grad_plan.hpp"
#include "sparse_cond_plan.hpp"

// the block A[i0 .. i0 + SC_KC)[r0 .. r0 + SC_CT) into the LDS, row stride SC_LD: clamped addresses, +0.0 outside the matrix
__device__ __forceinline__ void sc_stage(const double* __restrict__ A, int64_t lda, int M, int64_t n, int i0, int64_t r0, double* blk) {
  const int tid = threadIdx.x, col = tid & (SC_CT - 1), row0 = tid / SC_CT;
  const int64_t r = r0 + col, rc = r < n ? r : n - 1;
#pragma unroll
  for (int q = 0; q < SC_KC * SC_CT / SC_T; ++q) {
    const int row = q * (SC_T / SC_CT) + row0, i = i0 + row, ic = i < M ? i : M - 1;
    const double x = A[(int64_t)ic * lda + rc];
    blk[row * SC_LD + col] = (i < M && r < n) ? x : 0.0;
  }
}

// W[i][o] (M x DO) from a clamped address, +0.0 outside
__device__ __forceinline__ double sc_small(const double* __restrict__ W, int M, int DO, int i, int o) {
  const double x = W[(int64_t)(i < M ? i : M - 1) * DO + (o < DO ? o : DO - 1)];
  return (i < M && o < DO) ? x : 0.0;
}
// gm[r][o] (n x DO) likewise
__device__ __forceinline__ double sc_rowval(const double* __restrict__ gm, int64_t n, int DO, int64_t r, int o) {
  const double x = gm[(r < n ? r : n - 1) * DO + (o < DO ? o : DO - 1)];
  return (r < n && o < DO) ? x : 0.0;
}

__global__ __launch_bounds__(SC_T) void k_sc_fwd(const double* __restrict__ A, int64_t lda, int M, int64_t n, const double* __restrict__ W,
                                                 int DO, int out_groups, double kd, double* __restrict__ mean, double* __restrict__ var) {
  __shared__ double blk[SC_KC * SC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = DS_WAVE_ID(tid), g = lane >> 4, c = lane & 15;
  const int64_t r0 = (int64_t)blockIdx.x * SC_CT;
  double a2 = 0.0;
  for (int og = 0; og < out_groups; ++og) {
    const int o0 = og * SC_DOC * SC_DOG;
    d4 acc[SC_DOG];
#pragma unroll
    for (int q = 0; q < SC_DOG; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < M; i0 += SC_KC) {
      __syncthreads();                     // the previous block is consumed
      sc_stage(A, lda, M, n, i0, r0, blk);
      __syncthreads();
      if (og == 0 && tid < SC_CT) {        // the column's sum of squares, ascending i (rows past M are +0.0)
#pragma unroll 8
        for (int i = 0; i < SC_KC; ++i) {
          const double x = blk[i * SC_LD + tid];
          a2 = fma(x, x, a2);
        }
      }
#pragma unroll 4
      for (int k = 0; k < SC_KC; k += 4) {
        const double a = blk[(k + g) * SC_LD + wave * 16 + c];      // A operand: [data row c][k = g]
#pragma unroll
        for (int q = 0; q < SC_DOG; ++q)
          if (o0 + q * SC_DOC < DO) acc[q] = mfma_f64(a, sc_small(W, M, DO, i0 + k + g, o0 + q * SC_DOC + c), acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < SC_DOG; ++q) {
      const int o = o0 + q * SC_DOC + c;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t r = r0 + wave * 16 + g + 4 * t;
        if (mean && r < n && o < DO) mean[r * DO + o] = acc[q][t];
      }
    }
  }
  if (var && tid < SC_CT && r0 + tid < n) var[r0 + tid] = kd - a2;
}

__global__ __launch_bounds__(SC_T) void k_sc_adj(const double* __restrict__ A, int64_t lda, int M, int64_t n, const double* __restrict__ W,
                                                 int DO, int out_groups, const double* __restrict__ gm, const double* __restrict__ gv,
                                                 int64_t tiles, int64_t tiles_per_split, double* __restrict__ Abar,
                                                 double* __restrict__ PW) {
  __shared__ double blk[SC_KC * SC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = DS_WAVE_ID(tid), g = lane >> 4, c = lane & 15;
  const int i0 = (int)blockIdx.y * SC_KC, iw = i0 + wave * 16;      // the wave's 16 rows of A
  const int64_t t_lo = (int64_t)blockIdx.x * tiles_per_split;
  const int64_t t_hi = t_lo + tiles_per_split < tiles ? t_lo + tiles_per_split : tiles;
  for (int og = 0; og < out_groups; ++og) {
    const int o0 = og * SC_DOC * SC_DOG;
    d4 wb[SC_DOG];
#pragma unroll
    for (int q = 0; q < SC_DOG; ++q) wb[q] = d4{0.0, 0.0, 0.0, 0.0};
    for (int64_t tile = t_lo; tile < t_hi; ++tile) {
      const int64_t r0 = tile * SC_CT;
      __syncthreads();
      sc_stage(A, lda, M, n, i0, r0, blk);
      __syncthreads();
      if (og == 0) {                       // A_bar[i][r] = sum_o W[i][o] gm[r][o] - 2 A[i][r] gv[r]
        d4 ab[SC_CT / 16];
#pragma unroll
        for (int b = 0; b < SC_CT / 16; ++b) ab[b] = d4{0.0, 0.0, 0.0, 0.0};
        for (int o = 0; o < DO; o += 4) {
          const double w = sc_small(W, M, DO, iw + c, o + g);       // A operand: [row c][k = g]
#pragma unroll
          for (int b = 0; b < SC_CT / 16; ++b) ab[b] = mfma_f64(w, sc_rowval(gm, n, DO, r0 + b * 16 + c, o + g), ab[b]);
        }
#pragma unroll
        for (int b = 0; b < SC_CT / 16; ++b) {
          const int64_t r = r0 + b * 16 + c;
          const double v2 = 2.0 * gv[r < n ? r : n - 1];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int il = wave * 16 + g + 4 * t;
            if (i0 + il < M && r < n) Abar[(int64_t)(i0 + il) * lda + r] = ab[b][t] - v2 * blk[il * SC_LD + b * 16 + c];
          }
        }
      }
      // W_bar[i][o] += sum_r A[i][r] gm[r][o]
#pragma unroll 4
      for (int k = 0; k < SC_CT; k += 4) {
        const double a = blk[(wave * 16 + c) * SC_LD + k + g];      // A operand: [row c][k = g]
#pragma unroll
        for (int q = 0; q < SC_DOG; ++q)
          if (o0 + q * SC_DOC < DO) wb[q] = mfma_f64(a, sc_rowval(gm, n, DO, r0 + k + g, o0 + q * SC_DOC + c), wb[q]);
      }
    }
    double* __restrict__ P = PW + (int64_t)blockIdx.x * M * DO;
#pragma unroll
    for (int q = 0; q < SC_DOG; ++q) {
      const int o = o0 + q * SC_DOC + c;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = iw + g + 4 * t;
        if (i < M && o < DO) P[(int64_t)i * DO + o] = wb[q][t];
      }
    }
  }
}

// Zc = Z - Z[0], Xc = X - Z[0]: the kernels depend on differences only, and dsdgp_gram expands |x|^2 + |z|^2 - 2 x.z for D <= 32, which
// costs nothing around the origin only.  (The subtraction is exact for data within a factor of two of the origin it is moved to.)
__global__ __launch_bounds__(256) void k_sc_center(const double* __restrict__ Z, int64_t zcount, const double* __restrict__ X, int64_t xcount,
                                                   int D, double* __restrict__ Zc, double* __restrict__ Xc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= zcount + xcount) return;
  if (e < zcount) Zc[e] = Z[e] - Z[e % D];
  else Xc[e - zcount] = X[e - zcount] - Z[(e - zcount) % D];
}

// W_bar = the splits' partials in ascending order
__global__ __launch_bounds__(256) void k_sc_wsum(const double* __restrict__ PW, int nsplit, int64_t count, double* __restrict__ Wbar) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double a = 0.0;
  for (int s = 0; s < nsplit; ++s) a += PW[(int64_t)s * count + e];
  Wbar[e] = a;
}

// in place: Lu_bar = -tril(T)
__global__ __launch_bounds__(256) void k_sc_tril(double* __restrict__ T, int M) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M * M) return;
  const int i = (int)(e / M), j = (int)(e - (int64_t)i * M);
  T[e] = j <= i ? -T[e] : 0.0;
}

// S = 1/2 (P + P^T) with P = Phi(Q): S_ij = 1/2 Q[max(i, j)][min(i, j)]
__global__ __launch_bounds__(256) void k_sc_phi(const double* __restrict__ Q, int M, double* __restrict__ S) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M * M) return;
  const int i = (int)(e / M), j = (int)(e - (int64_t)i * M);
  S[e] = 0.5 * Q[(int64_t)(i > j ? i : j) * M + (i > j ? j : i)];
}

// one workgroup: kd_bar = sum_r gv_r (a thread its entries in ascending order, then a fixed tree); d_Z = dZ1 + dZ2; d_kern = dk1 + dk2,
// kd_bar added to the variance and, with a White part, to the last entry
__global__ __launch_bounds__(256) void k_sc_final(const double* __restrict__ gv, int64_t n, const double* __restrict__ dZ1,
                                                  const double* __restrict__ dZ2, int64_t zcount, const double* __restrict__ dk1,
                                                  const double* __restrict__ dk2, int nls, int has_white, double* __restrict__ d_Z,
                                                  double* __restrict__ d_kern) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  if (d_Z)
    for (int64_t e = tid; e < zcount; e += 256) d_Z[e] = dZ1[e] + dZ2[e];
  if (!d_kern) return;
  double a = 0.0;
  for (int64_t r = tid; r < n; r += 256) a += gv[r];
  a = block_sum<256>(a, red);
  if (tid <= 1 + nls) {
    double x = dk1[tid] + dk2[tid];
    if (tid == 0 || (tid == 1 + nls && has_white)) x += a;
    d_kern[tid] = x;
  }
}

static int sc_check(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* X, int64_t n, const double* q_mu,
                    int32_t DO, void* scratch) {
  DS_CHECK_ARG(ctx && kern && Z && X && q_mu && scratch);
  DS_CHECK_ARG(kern->kind == DSDGP_KERN_RBF || kern->kind == DSDGP_KERN_MATERN52);
  DS_CHECK_ARG(kern->input_dim > 0 && kern->lengthscales);
  DS_CHECK_ARG(M >= 1 && M <= SC_MAX_M && n >= 1 && n < SC_MAX_ROWS && DO >= 1);
  return DSDGP_OK;
}

static int sc_too_large(size_t bytes, int64_t n, int M) {
  dsdgp_set_error("%s:%d: the conditional of %lld rows on %d inducing points would take %zu bytes of scratch (more than 8 GB): pass the "
                  "rows in batches", __FILE__, __LINE__, (long long)n, M, bytes);
  return DSDGP_ERR_UNSUPPORTED;
}

// Lu, A and W into their regions of the scratch; DSDGP_ERR_NOT_SPD (and *info) from the factorisation
static int sc_factors(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const SCPlan& P, char* scr, const double* Z, const double* X,
                      const double* q_mu, int white, double jitter, int* info) {
  const int M = P.M;
  double *Lu = (double*)(scr + P.Ku.off), *A = (double*)(scr + P.A.off), *W = (double*)(scr + P.W.off);
  double *Zc = (double*)(scr + P.Zc.off), *Xc = (double*)(scr + P.Xc.off);
  const int64_t zc = (int64_t)M * P.D, xc = P.n * P.D;
  int status = 0;
  DS_LAUNCH(k_sc_center, dim3(ceil_div(zc + xc, 256)), dim3(256), 0, ctx->stream, Z, zc, X, xc, P.D, Zc, Xc);
  DS_TRY(dsdgp_gram(ctx, kern, Zc, M, nullptr, 0, jitter, Lu, M));
  const int rc = dsdgp_potrf(ctx, 1, M, Lu, M, 0, &status);
  if (info) *info = status;
  DS_TRY(rc);
  DS_TRY(dsdgp_gram(ctx, kern, Zc, M, Xc, P.n, 0.0, A, P.n));
  DS_TRY(dsdgp_trsm(ctx, 0, M, P.n, Lu, M, A, P.n));
  DS_HIP(hipMemcpyAsync(W, q_mu, (size_t)M * P.DO * 8, hipMemcpyDeviceToDevice, ctx->stream));
  if (!white) DS_TRY(dsdgp_trsm(ctx, 0, M, P.DO, Lu, M, W, P.DO));
  return DSDGP_OK;
}

extern "C" int dsdgp_sparse_conditional_scratch_bytes(int64_t n, int32_t M, int32_t D, int32_t DO, int32_t reverse, int64_t* bytes) {
  DS_CHECK_ARG(bytes && M >= 1 && M <= SC_MAX_M && n >= 1 && n < SC_MAX_ROWS && D >= 1 && DO >= 1);
  const SCPlan P = sparse_cond_plan(n, M, D, DO);
  *bytes = (int64_t)(reverse ? P.total : P.fwd_total);
  return DSDGP_OK;
}

extern "C" int dsdgp_sparse_conditional(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* X, int64_t n,
                                        const double* q_mu, int32_t DO, int32_t white, double jitter, void* scratch, int64_t scratch_bytes,
                                        double* mean, double* var, int* info) {
  DS_TRY(sc_check(ctx, kern, Z, M, X, n, q_mu, DO, scratch));
  const SCPlan P = sparse_cond_plan(n, M, kern->input_dim, DO);
  if (P.fwd_total > SC_SCRATCH_CAP) return sc_too_large(P.fwd_total, n, M);
  DS_CHECK_ARG(scratch_bytes >= 0 && (size_t)scratch_bytes >= P.fwd_total);
  char* scr = (char*)scratch;
  DS_TRY(sc_factors(ctx, kern, P, scr, Z, X, q_mu, white, jitter, info));
  if (!mean && !var) return DSDGP_OK;
  ProfScope ps(ctx, "sparse_cond_fwd");
  // both results are always formed (one read of A); a NULL output is only not stored
  const double kd = kern->variance + (kern->has_white ? kern->white_variance : 0.0);
  DS_LAUNCH(k_sc_fwd, dim3((unsigned)P.tiles), dim3(SC_T), 0, ctx->stream, (const double*)(scr + P.A.off), n, M, n,
            (const double*)(scr + P.W.off), (int)DO, P.out_groups, kd, mean, var);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_sparse_conditional_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* X, int64_t n,
                                             const double* q_mu, int32_t DO, int32_t white, double jitter, const double* gm,
                                             const double* gv, void* scratch, int64_t scratch_bytes, double* d_q_mu, double* d_Z,
                                             double* d_X, double* d_kern, int* info) {
  DS_TRY(sc_check(ctx, kern, Z, M, X, n, q_mu, DO, scratch));
  DS_CHECK_ARG(gm && gv);
  const int D = kern->input_dim;
  if (D > SC_MAX_D_GRAD) {
    dsdgp_set_error("%s:%d: the reverse pass of the sparse conditional goes through the reverse pass of the Gram matrix, which takes "
                    "input_dim <= %d, not %d", __FILE__, __LINE__, SC_MAX_D_GRAD, D);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const SCPlan P = sparse_cond_plan(n, M, D, DO);
  const size_t inner = std::max(gram_grad_plan(M, n, D, false).total, gram_grad_plan(M, M, D, true).total);
  if (P.total > SC_SCRATCH_CAP || inner > GG_SCRATCH_CAP) return sc_too_large(std::max(P.total, inner), n, M);
  DS_CHECK_ARG(scratch_bytes >= 0 && (size_t)scratch_bytes >= P.total);
  char* scr = (char*)scratch;
  auto at = [&](const SCRegion& r) { return (double*)(scr + r.off); };
  DS_TRY(sc_factors(ctx, kern, P, scr, Z, X, q_mu, white, jitter, info));
  hipStream_t st = ctx->stream;
  double *Lu = at(P.Ku), *A = at(P.A), *W = at(P.W), *Abar = at(P.Abar), *Wbar = at(P.Wbar), *V = at(P.V), *T = at(P.T), *Q = at(P.Q),
         *S = at(P.S), *St = at(P.St);
  const int mm_blocks = ceil_div((int64_t)M * M, 256);
  {
    ProfScope ps(ctx, "sparse_cond_adj");
    DS_LAUNCH(k_sc_adj, dim3((unsigned)P.nsplit, (unsigned)P.row_chunks), dim3(SC_T), 0, st, A, n, M, n, W, (int)DO, P.out_groups, gm, gv,
              P.tiles, P.tiles_per_split, Abar, at(P.PW));
    DS_LAUNCH(k_sc_wsum, dim3(ceil_div((int64_t)M * DO, 256)), dim3(256), 0, st, at(P.PW), P.nsplit, (int64_t)M * DO, Wbar);
  }
  DS_TRY(dsdgp_trsm(ctx, 1, M, n, Lu, M, Abar, n));                                  // K1_bar = Lu^-T A_bar
  DS_TRY(dsdgp_gemm(ctx, 0, 1, M, M, (int)n, 1.0, Abar, n, A, n, 0.0, T, M));        // T = K1_bar A^T
  if (!white) {
    DS_HIP(hipMemcpyAsync(V, Wbar, (size_t)M * DO * 8, hipMemcpyDeviceToDevice, st));
    DS_TRY(dsdgp_trsm(ctx, 1, M, DO, Lu, M, V, DO));                                 // V = Lu^-T W_bar = q_mu_bar
    DS_TRY(dsdgp_gemm(ctx, 0, 1, M, M, DO, 1.0, V, DO, W, DO, 1.0, T, M));           // T += V W^T
  }
  DS_LAUNCH(k_sc_tril, dim3(mm_blocks), dim3(256), 0, st, T, (int)M);                // Lu_bar
  DS_TRY(dsdgp_gemm(ctx, 1, 0, M, M, M, 1.0, Lu, M, T, M, 0.0, Q, M));               // Q = Lu^T Lu_bar
  DS_LAUNCH(k_sc_phi, dim3(mm_blocks), dim3(256), 0, st, Q, (int)M, S);
  DS_TRY(dsdgp_trsm(ctx, 1, M, M, Lu, M, S, M));                                     // Lu^-T S
  DS_TRY(dsdgp_scale_copy(ctx, 1, M, M, S, M, 1.0, 0.0, St, M));
  DS_TRY(dsdgp_trsm(ctx, 1, M, M, Lu, M, St, M));                                    // Lu^-T (Lu^-T S)^T = Ku_bar^T
  if (d_q_mu) DS_HIP(hipMemcpyAsync(d_q_mu, white ? Wbar : V, (size_t)M * DO * 8, hipMemcpyDeviceToDevice, st));
  if (d_Z || d_X || d_kern) {
    // the symmetric form adds G_ij + G_ji, so Ku_bar^T serves as Ku_bar; d_Z and d_kern are always formed, whichever is asked for
    DS_TRY(dsdgp_gram_grad(ctx, kern, Z, M, X, n, Abar, n, at(P.dZ1), d_X, at(P.dk1)));
    DS_TRY(dsdgp_gram_grad(ctx, kern, Z, M, nullptr, 0, St, M, at(P.dZ2), nullptr, at(P.dk2)));
    if (d_Z || d_kern)
      DS_LAUNCH(k_sc_final, dim3(1), dim3(256), 0, st, gv, n, at(P.dZ1), at(P.dZ2), (int64_t)M * D, at(P.dk1), at(P.dk2), kern->ard ? D : 1,
                kern->has_white ? 1 : 0, d_Z, d_kern);
  }
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// Reverse pass of the Gram matrix (gram.hip): given the adjoint G (n x n2) of K = dsdgp_gram(kern, X, X2) for a scalar F, the adjoints of
// X, X2 and of the kernel's hyper-parameters — what tf.gradients builds through kern.K of the dense layers (layers.py:278-279, 320-342).
// With u_d = (x_d - y_d) / l_d, r2 = sum_d u_d^2, k = v k1(r2), dk1 = d k1 / d r2 (kern_val_grad of common.hpp with variance 1):
//   dk/dx_d = 2 v dk1 u_d / l_d,   dk/dy_d = -dk/dx_d,   dk/dl_d = -2 v dk1 u_d^2 / l_d,   dk/dv = k1.
// A pair (row i, column j) has the weight w = G_ij (cross form), or G_ij + G_ji (symmetric form: K_ij and K_ji are the same function of
// the same two rows, so row i collects both adjoints), and t = 2 v w dk1.  Thread i of a pass accumulates over the columns j of its
// split, in ascending j,
//   sx_d += t u_d,   sl_d += (t u_d) u_d,   sv += w k1
// and the results are  d_X[i, d] = sum(sx_d) / l_d,  d_l_d = -f sum_i sum(sl_d) / l_d,  d_v = f sum_i sum(sv), with f = 1/2 in the
// symmetric form (every pair is met from both sides) and 1 in the cross form.  Every x_d - y_d is the difference of the two INPUTS,
// scaled afterwards: data at a large offset lose nothing.  Coincident rows have u = 0 and add nothing to d_X and d_l; a pair whose
// exponential underflows has k1 = dk1 = +0.
//
// k_gg_pass: a workgroup of GG_T threads owns GG_T rows (one per thread: the row's D values and its 2 D + 1 accumulators in registers)
// and one column split (gram_grad_plan.hpp), walked in tiles of GG_CT columns: the tile's rows of the column side are staged coalesced in
// the LDS and read as broadcasts, the tile of G through the LDS as well (read along its rows, used along its columns); the transposed
// weights (G_ji; the whole weight in pass b, where the roles of X and X2 are swapped) are coalesced as they are.  Two passes over d per
// pair: r2, then the weighted differences.  Loads are from clamped addresses and the weight of a column past the end is replaced by zero.
// k_gg_rows adds the partials of a row in ascending split order; k_gg_kern (one workgroup) adds the rows (a thread its rows in ascending
// order, then a fixed tree) and the diagonal of G.  No floating-point atomics: every summation order depends on (n, n2, D, form) alone.
#include "common.hpp"
#include "gram_grad_plan.hpp"

struct GGHyp {
  double il[GG_MAX_D];      // 1 / lengthscale of every dimension (the scalar one repeated)
  double variance;
};

enum { GG_W_DIRECT = 0, GG_W_TRANSPOSED = 1, GG_W_BOTH = 2 };      // the weight of (row r, column c): G[r][c], G[c][r], their sum
#define GG_LDG (GG_T + 1)

template <int KIND, int DMAX, bool KERN>
__global__ __launch_bounds__(GG_T) void k_gg_pass(const double* __restrict__ R, int64_t nrows, const double* __restrict__ Cm, int64_t ncols,
                                                  int D, const GGHyp hyp, const double* __restrict__ G, int64_t ldg, int wmode,
                                                  int64_t cols_per_split, double* __restrict__ PX, double* __restrict__ PL,
                                                  double* __restrict__ PV) {
  __shared__ double ys[GG_CT * DMAX];
  __shared__ double gt[GG_CT * GG_LDG];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * GG_T, row = r0 + tid, rc = row < nrows ? row : nrows - 1;
  const int64_t c_lo = (int64_t)blockIdx.y * cols_per_split;
  const int64_t c_hi = c_lo + cols_per_split < ncols ? c_lo + cols_per_split : ncols;
  double x[DMAX], sx[DMAX], sl[KERN ? DMAX : 1], sv = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    x[d] = R[rc * D + (d < D ? d : D - 1)];
    sx[d] = 0.0;
    if constexpr (KERN) sl[d] = 0.0;
  }
  const double v2 = 2.0 * hyp.variance;
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += GG_CT) {
    __syncthreads();                       // the previous tile is consumed
    // the tile's rows of the column side: GG_CT x D contiguous doubles (clamped at the end of the matrix)
    for (int e = tid; e < GG_CT * D; e += GG_T) {
      const int64_t idx = c0 * D + e, last = ncols * D - 1;
      ys[e] = Cm[idx < last ? idx : last];
    }
    if (wmode != GG_W_TRANSPOSED) {        // G[r0 + rr][c0 + cc], read along the rows, parked as gt[cc][rr]
#pragma unroll
      for (int q = 0; q < GG_CT; ++q) {
        const int e = q * GG_T + tid, rr = e / GG_CT, cc = e % GG_CT;
        const int64_t gr = r0 + rr < nrows ? r0 + rr : nrows - 1, gc = c0 + cc < ncols ? c0 + cc : ncols - 1;
        gt[cc * GG_LDG + rr] = G[gr * ldg + gc];
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int cc = 0; cc < GG_CT; ++cc) {
      const int64_t c = c0 + cc, ccl = c < ncols ? c : ncols - 1;
      double w = wmode != GG_W_TRANSPOSED ? gt[cc * GG_LDG + tid] : 0.0;
      if (wmode != GG_W_DIRECT) w += G[ccl * ldg + rc];
      if (c >= c_hi) w = 0.0;
      // a column past the end of the matrix was staged from a clamped address: finite values, weight zero
      const double* __restrict__ y = ys + (c < ncols ? cc : (int)(ncols - 1 - c0)) * D;
      double r2 = 0.0;
#pragma unroll
      for (int d = 0; d < DMAX; ++d)
        if (d < D) {
          const double u = (x[d] - y[d]) * hyp.il[d];
          r2 = fma(u, u, r2);
        }
      double k1, dk1;
      kern_val_grad<KIND>(r2, 1.0, k1, dk1);
      const double t = v2 * (w * dk1);
      if constexpr (KERN) sv = fma(w, k1, sv);
#pragma unroll
      for (int d = 0; d < DMAX; ++d)
        if (d < D) {
          const double u = (x[d] - y[d]) * hyp.il[d];
          const double tu = t * u;
          sx[d] += tu;
          if constexpr (KERN) sl[d] = fma(tu, u, sl[d]);
        }
    }
  }
  if (row >= nrows) return;
  const int64_t o = ((int64_t)blockIdx.y * nrows + row) * D;
#pragma unroll
  for (int d = 0; d < DMAX; ++d)
    if (d < D) {
      PX[o + d] = sx[d];
      if constexpr (KERN) PL[o + d] = sl[d];
    }
  if constexpr (KERN) PV[(int64_t)blockIdx.y * nrows + row] = sv;
}

// one thread per (row, d): the splits in ascending order; d_X = sum / l_d, and (KERN side) the row's sums for k_gg_kern
__global__ __launch_bounds__(256) void k_gg_rows(const double* __restrict__ PX, const double* __restrict__ PL, const double* __restrict__ PV,
                                                 int nsplit, int64_t nrows, int D, const GGHyp hyp, double* __restrict__ d_X,
                                                 double* __restrict__ Lrow, double* __restrict__ Vrow) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nrows * D) return;
  const int64_t r = e / D;
  const int d = (int)(e - r * D);
  if (d_X) {
    double a = 0.0;
    for (int s = 0; s < nsplit; ++s) a += PX[(int64_t)s * nrows * D + e];
    d_X[e] = a * hyp.il[d];
  }
  if (Lrow) {
    double b = 0.0;
    for (int s = 0; s < nsplit; ++s) b += PL[(int64_t)s * nrows * D + e];
    Lrow[e] = b;
    if (d == 0) {
      double c = 0.0;
      for (int s = 0; s < nsplit; ++s) c += PV[(int64_t)s * nrows + r];
      Vrow[r] = c;
    }
  }
}

// one workgroup: d_kern[0] = f sum_r Vrow_r;  d_kern[1 + d] = -f sum_r Lrow_rd / l_d (added over d, ascending, without ARD);  the last
// entry = sum_i G_ii in the symmetric form (G != NULL), 0 in the cross form
__global__ __launch_bounds__(256) void k_gg_kern(const double* __restrict__ Lrow, const double* __restrict__ Vrow, int64_t n, int D, int ard,
                                                 const GGHyp hyp, double f, const double* __restrict__ G, int64_t ldg,
                                                 double* __restrict__ d_kern) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t r = tid; r < n; r += 256) a += Vrow[r];
  a = block_sum<256>(a, red);
  if (tid == 0) d_kern[0] = f * a;
  double tot = 0.0;
  for (int d = 0; d < D; ++d) {
    double x = 0.0;
    for (int64_t r = tid; r < n; r += 256) x += Lrow[r * D + d];
    x = block_sum<256>(x, red);
    const double dl = -f * (x * hyp.il[d]);
    if (ard) {
      if (tid == 0) d_kern[1 + d] = dl;
    } else {
      tot += dl;
    }
  }
  if (!ard && tid == 0) d_kern[1] = tot;
  double g = 0.0;
  if (G) {
    for (int64_t r = tid; r < n; r += 256) g += G[r * ldg + r];
    g = block_sum<256>(g, red);
  }
  if (tid == 0) d_kern[1 + (ard ? D : 1)] = g;
}

template <int KIND, bool KERN>
static void gg_pass_go(hipStream_t st, const GGPass& p, const double* R, const double* Cm, int D, const GGHyp& hyp, const double* G, int64_t ldg,
                       int wmode, double* PX, double* PL, double* PV) {
  const dim3 grid((unsigned)p.row_blocks, (unsigned)p.nsplit), block(GG_T);
  if (D <= 4)
    DS_LAUNCH((k_gg_pass<KIND, 4, KERN>), grid, block, 0, st, R, p.rows, Cm, p.cols, D, hyp, G, ldg, wmode, p.cols_per_split, PX, PL, PV);
  else if (D <= 8)
    DS_LAUNCH((k_gg_pass<KIND, 8, KERN>), grid, block, 0, st, R, p.rows, Cm, p.cols, D, hyp, G, ldg, wmode, p.cols_per_split, PX, PL, PV);
  else if (D <= 16)
    DS_LAUNCH((k_gg_pass<KIND, 16, KERN>), grid, block, 0, st, R, p.rows, Cm, p.cols, D, hyp, G, ldg, wmode, p.cols_per_split, PX, PL, PV);
  else
    DS_LAUNCH((k_gg_pass<KIND, 32, KERN>), grid, block, 0, st, R, p.rows, Cm, p.cols, D, hyp, G, ldg, wmode, p.cols_per_split, PX, PL, PV);
}

extern "C" int dsdgp_gram_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, const double* X2, int64_t n2,
                               const double* G, int64_t ldg, double* d_X, double* d_X2, double* d_kern) {
  DS_CHECK_ARG(ctx && kern && X && G);
  DS_CHECK_ARG(kern->kind == DSDGP_KERN_RBF || kern->kind == DSDGP_KERN_MATERN52);
  DS_CHECK_ARG(kern->input_dim > 0 && kern->lengthscales);
  DS_CHECK_ARG(n > 0 && n < GG_MAX_ROWS);
  const bool symmetric = X2 == nullptr;
  if (symmetric) {
    DS_CHECK_ARG(d_X2 == nullptr);
    n2 = n;
  }
  DS_CHECK_ARG(n2 > 0 && n2 < GG_MAX_ROWS && ldg >= n2);
  const int D = kern->input_dim;
  if (D > GG_MAX_D) {
    dsdgp_set_error("%s:%d: the reverse pass of the Gram matrix takes input_dim <= %d (a thread holds its row in registers), not %d",
                    __FILE__, __LINE__, GG_MAX_D, D);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const GGPlan P = gram_grad_plan(n, n2, D, symmetric);
  if (P.total > GG_SCRATCH_CAP) {
    dsdgp_set_error("%s:%d: the partial sums of %lld x %lld rows would take %zu bytes of scratch (more than 8 GB): pass the rows in batches",
                    __FILE__, __LINE__, (long long)n, (long long)n2, P.total);
    return DSDGP_ERR_UNSUPPORTED;
  }
  GGHyp hyp;
  for (int d = 0; d < GG_MAX_D; ++d) hyp.il[d] = d < D ? 1.0 / kern->lengthscales[kern->ard ? d : 0] : 0.0;
  hyp.variance = kern->variance;
  void* scr;
  DS_TRY(ctx_scratch(ctx, P.total, &scr));
  auto at = [&](const GGRegion& r) { return (double*)((char*)scr + r.off); };
  hipStream_t st = ctx->stream;
  ProfScope ps(ctx, "gram_grad");
  const bool rbf = kern->kind == DSDGP_KERN_RBF;
  if (d_X || d_kern) {
    const int wmode = symmetric ? GG_W_BOTH : GG_W_DIRECT;
    const double* Cm = symmetric ? X : X2;
    if (rbf) gg_pass_go<DSDGP_KERN_RBF, true>(st, P.a, X, Cm, D, hyp, G, ldg, wmode, at(P.a.PX), at(P.PL), at(P.PV));
    else gg_pass_go<DSDGP_KERN_MATERN52, true>(st, P.a, X, Cm, D, hyp, G, ldg, wmode, at(P.a.PX), at(P.PL), at(P.PV));
    DS_LAUNCH(k_gg_rows, dim3(ceil_div(n * D, 256)), dim3(256), 0, st, at(P.a.PX), at(P.PL), at(P.PV), P.a.nsplit, n, D, hyp, d_X,
              d_kern ? at(P.Lrow) : nullptr, at(P.Vrow));
    if (d_kern)
      DS_LAUNCH(k_gg_kern, dim3(1), dim3(256), 0, st, at(P.Lrow), at(P.Vrow), n, D, kern->ard ? 1 : 0, hyp, symmetric ? 0.5 : 1.0,
                symmetric ? G : nullptr, ldg, d_kern);
  }
  if (d_X2) {
    if (rbf) gg_pass_go<DSDGP_KERN_RBF, false>(st, P.b, X2, X, D, hyp, G, ldg, GG_W_TRANSPOSED, at(P.b.PX), nullptr, nullptr);
    else gg_pass_go<DSDGP_KERN_MATERN52, false>(st, P.b, X2, X, D, hyp, G, ldg, GG_W_TRANSPOSED, at(P.b.PX), nullptr, nullptr);
    DS_LAUNCH(k_gg_rows, dim3(ceil_div(n2 * D, 256)), dim3(256), 0, st, at(P.b.PX), nullptr, nullptr, P.b.nsplit, n2, D, hyp, d_X2, nullptr,
              nullptr);
  }
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// Greedy conditional-variance selection of the inducing points on the device: the pivoted Cholesky factorisation of K(X, X) that
// Burt, Rasmussen and van der Wilk (2020) call "ConditionalVariance".  Step j takes the row p_j whose variance conditioned on the rows
// already chosen is largest, appends the column c_j = (k(., x_p) - sum_{t<j} c_t c_t[p]) / sqrt(d_p) and lowers every d_i by c_j[i]^2.
// All M steps are enqueued on the context's stream; the chosen row never visits the host.
//
// Layout.  The columns live t-major in scratch, C[t][i] with a row stride of np = n rounded up to GR_ROWS, and so does a transposed
// copy of the data, Xt[d][i] (written once by k_gr_transpose, zero in the padding).  Step j is then two sweeps of the same shape over
// contiguous length-np rows: D rows of Xt for r^2 = sum_d ((x_i - x_p)_d / l_d)^2 — differences first, never |x|^2 + |z|^2 - 2 x.z —
// and j rows of C for sum_t c_t[i] c_t[p].  A lane owns two neighbouring data rows (one 16-byte load per stream row), a one-wave
// workgroup GR_ROWS = 128 of them per chunk; GR_U = 16 stream rows are loaded into one register buffer while the previous 16 are
// consumed from the other, so 16 .. 32 rows x n x 8 bytes are in flight over the device.  The ragged end of either sweep is loaded
// from the last valid stream row and meets a zero coefficient: no branch around a load.  Bytes of step j: 8 n (D + j + 3).
//
// One launch per step (k_gr_step).  Every workgroup first folds the previous launch's per-workgroup partials — (largest d, its row)
// by the order larger value, then lower row; the partial sums of d in a fixed tree — which gives p_j, d_p and trace_{j-1} without any
// coordination inside a launch: the kernel boundary is the only synchronisation.  It fetches the pivot's x_p and the strided
// c_t[p], t < j, into LDS once (workgroup 0 writes them out as row j of Z and of L), sweeps its chunks, and leaves its own partials
// in the other half of a double buffer.  After the stop rule fires (d_p <= threshold) the later launches see stopped[j] and return.
//
// Determinism.  No floating-point atomics; sum_d and sum_t are single fma chains in ascending order, the same instructions for both
// rows of a lane and for every lane, so a row's arithmetic does not depend on where the row sits: two bit-identical rows of X carry
// bit-identical d, and their tie goes to the lower row.  The partial sums depend on n alone.  A NaN never wins the arg-max.
#include <math.h>

#include "common.hpp"

#define GR_T 64
#define GR_ROWS 128       // data rows of a chunk: two per lane
#define GR_U 16           // stream rows per register buffer
#define GR_MAX_M 2048
#define GR_MAX_D 1024
#define GR_MAX_NB 2048    // most workgroups (= partials folded by every workgroup of the next launch)
#define GR_NONE 0x7fffffff

struct GrArgs {
  const double* X;        // n x D, row-major
  const double* Xt;       // D x np
  const double* ils;      // D reciprocal lengthscales
  double* C;              // M x np
  double* d;              // np
  double* pmax;           // 2 x nb
  double* psum;           // 2 x nb
  int* pidx;              // 2 x nb
  int* stopped;           // M + 2
  int32_t* idx;
  int32_t* m_out;
  double *Z, *residual, *trace, *L;
  int64_t n, np, ldl;
  int D, M, nb, cpw;      // cpw: chunks per workgroup
  double variance, threshold;
};

// X (n x D) -> Xt (D x np), zero for the rows n .. np
__global__ __launch_bounds__(256) void k_gr_transpose(const double* __restrict__ X, int64_t n, int D, int64_t np, double* __restrict__ Xt) {
  __shared__ double tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * 64;
  const int d0 = blockIdx.y * 64;
  for (int r = ty; r < 64; r += 4) {
    const int64_t i = i0 + r;
    const int dd = d0 + tx;
    tile[r][tx] = (i < n && dd < D) ? X[i * D + dd] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int dd = d0 + r;
    if (dd < D) Xt[(int64_t)dd * np + i0 + tx] = tile[tx][r];
  }
}

// d_i = kdiag (0 in the padding); the partials launch 0 folds: (kdiag, p0) in slot 0, so p_0 = p0; the sums add up to tr K(X, X)
__global__ __launch_bounds__(256) void k_gr_init(GrArgs a, double kdiag, int p0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.np) a.d[i] = i < a.n ? kdiag : 0.0;
  if (i < a.nb) {
    const int64_t r0 = i * a.cpw * GR_ROWS;
    int64_t r1 = r0 + (int64_t)a.cpw * GR_ROWS;
    if (r1 > a.n) r1 = a.n;
    a.pmax[i] = i == 0 ? kdiag : -INFINITY;
    a.pidx[i] = i == 0 ? p0 : GR_NONE;
    a.psum[i] = r1 > r0 ? (double)(r1 - r0) * kdiag : 0.0;
  }
}

__device__ __forceinline__ void gr_better(double& bv, int& bi, double v, int i) {      // larger value, then lower row; a NaN never wins
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// (value, row, sum) over the wave: xor butterfly, every lane ends with the same bits
__device__ __forceinline__ void gr_wave_fold(double& bv, int& bi, double& sum) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    gr_better(bv, bi, ov, oi);
    sum += __shfl_xor(sum, off);
  }
}

// the partials of the previous launch: lane l takes the slots l, l + 64, ... in order
__device__ __forceinline__ void gr_fold_partials(const GrArgs& a, int half, int lane, double& bv, int& bi, double& sum) {
  const double* pm = a.pmax + (int64_t)half * a.nb;
  const double* ps = a.psum + (int64_t)half * a.nb;
  const int* pi = a.pidx + (int64_t)half * a.nb;
  bv = -INFINITY;
  bi = GR_NONE;
  sum = 0.0;
  for (int q = lane; q < a.nb; q += GR_T) {
    gr_better(bv, bi, pm[q], pi[q]);
    sum += ps[q];
  }
  gr_wave_fold(bv, bi, sum);
}

template <int KIND>
__global__ __launch_bounds__(GR_T) void k_gr_step(GrArgs a, int j) {
  __shared__ double cp[GR_MAX_M + GR_U];      // c_t[p], t < j, zeros up to a whole buffer
  __shared__ double xp[GR_MAX_D + GR_U];      // x_p
  __shared__ double il[GR_MAX_D + GR_U];      // 1 / lengthscale, zeros up to a whole buffer
  const int lane = threadIdx.x, b = blockIdx.x;
  if (a.stopped[j]) {
    if (b == 0 && lane == 0) a.stopped[j + 1] = 1;
    return;
  }
  double res, tr;
  int p;
  gr_fold_partials(a, j & 1, lane, res, p, tr);
  if (!(res > a.threshold) || p < 0 || (int64_t)p >= a.n) {      // the stop rule: m = j points; trace_{m-1} fills the rest
    if (b == 0) {
      if (lane == 0) a.stopped[j + 1] = 1;
      if (a.trace)
        for (int t = (j > 0 ? j - 1 : 0) + lane; t < a.M; t += GR_T) a.trace[t] = tr;
    }
    return;
  }
  const double sq = sqrt(res);
  const int jpad = (j + GR_U - 1) / GR_U * GR_U, dpad = (a.D + GR_U - 1) / GR_U * GR_U;
  for (int t = lane; t < jpad; t += GR_T) cp[t] = t < j ? a.C[(int64_t)t * a.np + p] : 0.0;
  for (int dd = lane; dd < dpad; dd += GR_T) {
    xp[dd] = dd < a.D ? a.X[(int64_t)p * a.D + dd] : 0.0;
    il[dd] = dd < a.D ? a.ils[dd] : 0.0;
  }
  __syncthreads();
  if (b == 0) {
    if (lane == 0) {
      a.idx[j] = p;
      a.m_out[0] = j + 1;
      if (a.residual) a.residual[j] = res;
      if (a.trace && j > 0) a.trace[j - 1] = tr;
      if (a.L) a.L[(int64_t)j * a.ldl + j] = sq;
    }
    if (a.L)
      for (int t = lane; t < j; t += GR_T) a.L[(int64_t)j * a.ldl + t] = cp[t];
    if (a.Z)
      for (int dd = lane; dd < a.D; dd += GR_T) a.Z[(int64_t)j * a.D + dd] = xp[dd];
  }
  const int64_t nchunks = a.np / GR_ROWS;
  const int64_t c0 = (int64_t)b * a.cpw;
  const int64_t c1 = c0 + a.cpw < nchunks ? c0 + a.cpw : nchunks;
  const int64_t s2 = a.np / 2;      // stream row stride in double2
  double bv = -INFINITY, sum = 0.0;
  int bi = GR_NONE;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t i0 = c * GR_ROWS + 2 * lane;
    // ---- r^2 over the D rows of Xt
    double r0 = 0.0, r1 = 0.0;
    {
      const double2* src = (const double2*)(a.Xt + i0);
      const int last = a.D - 1;
      double2 cur[GR_U], nxt[GR_U];
#pragma unroll
      for (int u = 0; u < GR_U; ++u) cur[u] = src[(int64_t)(u < last ? u : last) * s2];
      for (int t0 = 0; t0 < dpad; t0 += GR_U) {
        const int t1 = t0 + GR_U;
        if (t1 < dpad) {
#pragma unroll
          for (int u = 0; u < GR_U; ++u) nxt[u] = src[(int64_t)(t1 + u < last ? t1 + u : last) * s2];
        }
#pragma unroll
        for (int u = 0; u < GR_U; ++u) {
          const double x = xp[t0 + u], s = il[t0 + u];
          const double e0 = (cur[u].x - x) * s, e1 = (cur[u].y - x) * s;
          r0 = fma(e0, e0, r0);
          r1 = fma(e1, e1, r1);
        }
#pragma unroll
        for (int u = 0; u < GR_U; ++u) cur[u] = nxt[u];
      }
    }
    // ---- sum_t c_t[i] c_t[p] over the j rows of C, ascending t
    double a0 = 0.0, a1 = 0.0;
    if (j > 0) {
      const double2* src = (const double2*)(a.C + i0);
      const int last = j - 1;
      double2 cur[GR_U], nxt[GR_U];
#pragma unroll
      for (int u = 0; u < GR_U; ++u) cur[u] = src[(int64_t)(u < last ? u : last) * s2];
      for (int t0 = 0; t0 < jpad; t0 += GR_U) {
        const int t1 = t0 + GR_U;
        if (t1 < jpad) {
#pragma unroll
          for (int u = 0; u < GR_U; ++u) nxt[u] = src[(int64_t)(t1 + u < last ? t1 + u : last) * s2];
        }
#pragma unroll
        for (int u = 0; u < GR_U; ++u) {
          const double w = cp[t0 + u];
          a0 = fma(cur[u].x, w, a0);
          a1 = fma(cur[u].y, w, a1);
        }
#pragma unroll
        for (int u = 0; u < GR_U; ++u) cur[u] = nxt[u];
      }
    }
    const double k0 = kern_val<KIND>(r0, a.variance), k1 = kern_val<KIND>(r1, a.variance);
    double2 cj;
    cj.x = (k0 - a0) / sq;
    cj.y = (k1 - a1) / sq;
    *(double2*)(a.C + (int64_t)j * a.np + i0) = cj;
    double2 dv = *(const double2*)(a.d + i0);
    const double n0 = fma(-cj.x, cj.x, dv.x), n1 = fma(-cj.y, cj.y, dv.y);
    dv.x = (n0 > 0.0 && i0 != p) ? n0 : 0.0;
    dv.y = (n1 > 0.0 && i0 + 1 != p) ? n1 : 0.0;
    *(double2*)(a.d + i0) = dv;
    if (i0 < a.n) gr_better(bv, bi, dv.x, (int)i0);
    if (i0 + 1 < a.n) gr_better(bv, bi, dv.y, (int)(i0 + 1));
    sum += dv.x;
    sum += dv.y;
  }
  gr_wave_fold(bv, bi, sum);
  if (lane == 0) {
    const int64_t o = (int64_t)((j + 1) & 1) * a.nb + b;
    a.pmax[o] = bv;
    a.pidx[o] = bi;
    a.psum[o] = sum;
  }
}

// after the last step: trace_{M-1}
__global__ __launch_bounds__(GR_T) void k_gr_finish(GrArgs a) {
  if (a.stopped[a.M]) return;
  double res, tr;
  int p;
  gr_fold_partials(a, a.M & 1, threadIdx.x, res, p, tr);
  if (threadIdx.x == 0) a.trace[a.M - 1] = tr;
}

extern "C" int dsdgp_greedy_inducing(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, int32_t M, int64_t first,
                                     double threshold, int32_t* idx, int32_t* m_out, double* Z, double* residual, double* trace,
                                     double* L, int64_t ldl) {
  DS_CHECK_ARG(ctx && kern && X && idx && m_out);
  DS_CHECK_ARG(kern->kind == DSDGP_KERN_RBF || kern->kind == DSDGP_KERN_MATERN52);
  DS_CHECK_ARG(kern->input_dim >= 1 && kern->input_dim <= GR_MAX_D && kern->lengthscales);
  DS_CHECK_ARG(M >= 2 && M <= GR_MAX_M);
  DS_CHECK_ARG(n >= M && n <= 0x7fffffff);
  DS_CHECK_ARG(first >= -1 && first < n);
  DS_CHECK_ARG(threshold >= 0.0);      // false for a NaN
  DS_CHECK_ARG(!L || ldl >= M);
  const int D = kern->input_dim;
  const int64_t np = round_up(n, GR_ROWS);
  const int64_t cap = (int64_t)1 << 30;      // doubles: 8 GB of scratch per array
  if ((int64_t)M * n > cap || (int64_t)D * np > cap) {
    dsdgp_set_error("dsdgp_greedy_inducing: the %d x %lld column store or the %d x %lld transposed data exceed 2^30 doubles: pass a subset of the rows",
                    (int)M, (long long)n, D, (long long)np);
    return DSDGP_ERR_UNSUPPORTED;
  }
  hipStream_t st = ctx->stream;
  const int64_t nchunks = np / GR_ROWS;
  const int cpw = ceil_div(nchunks, GR_MAX_NB);
  const int nb = ceil_div(nchunks, cpw);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (size_t)round_up((int64_t)bytes, 256); return at; };
  const size_t o_ils = take((size_t)D * 8), o_xt = take((size_t)D * np * 8), o_c = take((size_t)M * np * 8), o_d = take((size_t)np * 8);
  const size_t o_pmax = take((size_t)2 * nb * 8), o_psum = take((size_t)2 * nb * 8), o_pidx = take((size_t)2 * nb * 4);
  const size_t o_stop = take((size_t)(M + 2) * 4);
  void* scr;
  DS_TRY(ctx_scratch(ctx, off, &scr));
  char* base = (char*)scr;
  std::vector<double> ils(D);
  for (int q = 0; q < D; ++q) ils[q] = 1.0 / kern->lengthscales[kern->ard ? q : 0];
  DS_TRY(ctx_upload(ctx, base + o_ils, ils.data(), (size_t)D * 8));
  GrArgs a;
  a.X = X;
  a.Xt = (const double*)(base + o_xt);
  a.ils = (const double*)(base + o_ils);
  a.C = (double*)(base + o_c);
  a.d = (double*)(base + o_d);
  a.pmax = (double*)(base + o_pmax);
  a.psum = (double*)(base + o_psum);
  a.pidx = (int*)(base + o_pidx);
  a.stopped = (int*)(base + o_stop);
  a.idx = idx;
  a.m_out = m_out;
  a.Z = Z;
  a.residual = residual;
  a.trace = trace;
  a.L = L;
  a.n = n;
  a.np = np;
  a.ldl = ldl;
  a.D = D;
  a.M = M;
  a.nb = nb;
  a.cpw = cpw;
  a.variance = kern->variance;
  a.threshold = threshold;
  const double kdiag = kern->variance + (kern->has_white ? kern->white_variance : 0.0);
  ProfScope prof(ctx, "greedy");
  // what the entries j >= m keep: idx -1, residual 0, zero rows of Z and L (the trace is filled by the launch that stops)
  DS_HIP(hipMemsetAsync(a.stopped, 0, (size_t)(M + 2) * 4, st));
  DS_HIP(hipMemsetAsync(idx, 0xff, (size_t)M * 4, st));
  DS_HIP(hipMemsetAsync(m_out, 0, 4, st));
  if (Z) DS_HIP(hipMemsetAsync(Z, 0, (size_t)M * D * 8, st));
  if (residual) DS_HIP(hipMemsetAsync(residual, 0, (size_t)M * 8, st));
  if (L) DS_HIP(hipMemset2DAsync(L, (size_t)ldl * 8, 0, (size_t)M * 8, (size_t)M, st));
  DS_LAUNCH(k_gr_transpose, dim3((unsigned)(np / 64), (unsigned)ceil_div(D, 64)), dim3(256), 0, st, X, n, D, np, (double*)(base + o_xt));
  DS_LAUNCH(k_gr_init, dim3((unsigned)ceil_div(np, 256)), dim3(256), 0, st, a, kdiag, (int)(first >= 0 ? first : 0));
  for (int j = 0; j < M; ++j) {
    if (kern->kind == DSDGP_KERN_RBF)
      DS_LAUNCH(k_gr_step<DSDGP_KERN_RBF>, dim3(nb), dim3(GR_T), 0, st, a, j);
    else
      DS_LAUNCH(k_gr_step<DSDGP_KERN_MATERN52>, dim3(nb), dim3(GR_T), 0, st, a, j);
  }
  if (trace) DS_LAUNCH(k_gr_finish, dim3(1), dim3(GR_T), 0, st, a);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// Pathwise (Matheron) draws of a sparse GP posterior function (Wilson, Borovitskiy, Terenin, Mostowsky and Deisenroth, ICML 2020); the
// calls have no counterpart in the reference.  With k = s2 kappa(. / l), a random Fourier basis Omega (D x L, already divided by l row
// by row), an origin c and standard normal weights a = Wc, b = Ws (S x L x DO):
//   theta_j(x) = sum_d (x_d - c_d) Omega_dj                                   (the difference first, then the product)
//   f0(x)_o    = sqrt(s2 / L) sum_j [a_jo cos theta_j(x) + b_jo sin theta_j(x)]        (Var f0(x) = s2 exactly)
//   f(x)_o     = f0(x)_o + sum_m k(x, z_m) v_mo + add(x)_o,    v = Ku^-1 (u - f0(Z)),  Ku = K(Z, Z) + (White variance + jitter) I,
//   u_o = q_mu_o + q_sqrt_o eps_o, with white Lu (q_mu_o + q_sqrt_o eps_o), Lu = chol(Ku).
//
// k_pw_eval, one launch for all draws: workgroup (tile, s) owns PW_RT rows of draw s, each of its four waves 16 of them, as COLUMNS of the
// fp64 MFMA products, so that a product's result is the next product's B operand without a transpose:
//   theta^T (16 frequencies x 16 rows) = Omega^T (x - c)^T      k over the input dimensions, four per MFMA, the last group ragged;
//   sincos per element: D register t of lane (g, c) is frequency g + 4t of row c, which is B[k = g][row c] of k-step t;
//   out^T (16 outputs x 16 rows) += Wc^T cos(theta^T) + Ws^T sin(theta^T)      k over the chunk's frequencies in ascending order;
//   out^T += V^T K(Z, x)      k over the inducing rows, lane (g, c) forming k(x_c, z_{m0 + 4u + g}) from the differences x_d - z_d.
// X, the origin, Omega, [Wc; Ws], Z, V and 1 / l are staged in the LDS chunk by chunk (pathwise_plan.hpp); nothing of size rows x L or
// rows x M reaches memory.  A row is a column of every product and a lane's own distances: a NaN or an infinity in it stays in its outputs.
// No atomics; an entry's summation order follows from (L, M, D, DO) alone, never from n, S or the row's place in the call.
//
// Sine and cosine: |theta| < PW_FAST_MAX = 4096 reduces by n = rint(theta 2 / pi) with pi / 2 in two doubles (theta - n P1 is exact in an
// fma for |n| < 2^12, the tail n P2 costs under 1e-28) and evaluates the two minimax polynomials on [-pi / 4, pi / 4]; everything else,
// NaN and the infinities included, goes through the device library's sincos, which is correct for every finite argument.
//
// dsdgp_pathwise_weights composes dsdgp_gram, dsdgp_potrf, k_pw_eval at X = Z, M = 0, dsdgp_gemm and dsdgp_trsm in a block the caller holds.
#include "common.hpp"
#include "pathwise_plan.hpp"

struct PWArgs {
  const double *X, *Om, *org, *Wc, *Ws, *Z, *V, *ils, *add;
  double* out;
  int64_t n, x_stride, ld_add, add_stride, ld_out, out_stride;
  int D, L, M, DO, kind;
  double amp, s2;
};

// sin and cos of a reduced argument |r| <= pi / 4 (+ an ulp): the minimax polynomials of fdlibm's k_sin.c / k_cos.c
__device__ __forceinline__ void pw_sincos_small(double r, double& sn, double& cs) {
  const double z = r * r;
  const double ps = fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                               -1.98412698298579493134e-04), 8.33333333332248946124e-03);
  sn = fma(z * r, fma(z, ps, -1.66666666666666324348e-01), r);
  const double pc = z * fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                                 -2.75573143513906633035e-07), 2.48015872894767294178e-05), -1.38888888888741095749e-03),
                            4.16666666666666019037e-02);
  const double hz = 0.5 * z, w = 1.0 - hz;
  cs = w + (((1.0 - w) - hz) + z * pc);
}

// the safe route, out of line: one copy of the library routine, not one per unrolled element
__device__ __attribute__((noinline)) void pw_sincos_any(double th, double& sn, double& cs) { sincos(th, &sn, &cs); }

__device__ __forceinline__ void pw_sincos(double th, double& sn, double& cs) {
  if (fabs(th) < PW_FAST_MAX) {
    const double fn = rint(th * 6.36619772367581382433e-01);      // 2 / pi
    const double r = fma(-fn, 6.12323399573676603587e-17, fma(-fn, 1.57079632679489655800e+00, th));
    double s0, c0;
    pw_sincos_small(r, s0, c0);
    const int q = (int)fn;
    const double sa = (q & 1) ? c0 : s0, ca = (q & 1) ? s0 : c0;
    sn = (q & 2) ? -sa : sa;
    cs = ((q + 1) & 2) ? -ca : ca;
  } else {
    pw_sincos_any(th, sn, cs);
  }
}

__global__ __launch_bounds__(PW_T) void k_pw_eval(const PWArgs a) {
  __shared__ double xs[PW_RT * PW_XLD], orgs[PW_DC], oms[PW_DC * PW_OLD], wsm[(2 * PW_LC > PW_ZT ? 2 * PW_LC : PW_ZT) * PW_WLD],
      zs[PW_ZT * PW_XLD], ilss[PW_DC];
  const int tid = threadIdx.x, lane = tid & 63, wave = DS_WAVE_ID(tid), g = lane >> 4, c = lane & 15;
  const int D = a.D, L = a.L, M = a.M, DO = a.DO;
  const int64_t n = a.n, s = blockIdx.y, r0 = (int64_t)blockIdx.x * PW_RT;
  const double* __restrict__ X = a.X + s * a.x_stride;
  const double* __restrict__ Wc = a.Wc + s * (int64_t)L * DO;
  const double* __restrict__ Ws = a.Ws + s * (int64_t)L * DO;
  const double* __restrict__ V = M > 0 ? a.V + s * (int64_t)M * DO : nullptr;
  const int xrow = (wave * 16 + c) * PW_XLD;
  int xs_d0 = -1;                            // the chunk of input dimensions xs and orgs hold
  // X[r0 .. r0 + PW_RT)[d0 .. d0 + PW_DC) and the origin's chunk: clamped addresses, +0.0 outside
  auto stage_x = [&](int d0) {
    if (xs_d0 == d0) return;
    xs_d0 = d0;
#pragma unroll
    for (int q = 0; q < PW_RT * PW_DC / PW_T; ++q) {
      const int e = q * PW_T + tid, row = e / PW_DC, dd = e % PW_DC, d = d0 + dd;
      const int64_t r = r0 + row;
      const double x = X[(r < n ? r : n - 1) * D + (d < D ? d : D - 1)];
      xs[row * PW_XLD + dd] = (r < n && d < D) ? x : 0.0;
    }
    if (tid < PW_DC) orgs[tid] = d0 + tid < D ? a.org[d0 + tid] : 0.0;
  };

  for (int o0 = 0; o0 < DO; o0 += PW_OC * PW_OG) {
    d4 af[PW_OG], ak[PW_OG];
#pragma unroll
    for (int q = 0; q < PW_OG; ++q) af[q] = d4{0.0, 0.0, 0.0, 0.0}, ak[q] = d4{0.0, 0.0, 0.0, 0.0};

    // ---- the prior part: the frequencies in chunks of PW_LC
    for (int j0 = 0; j0 < L; j0 += PW_LC) {
      d4 th[PW_LC / 16];
#pragma unroll
      for (int jt = 0; jt < PW_LC / 16; ++jt) th[jt] = d4{0.0, 0.0, 0.0, 0.0};
      for (int d0 = 0; d0 < D; d0 += PW_DC) {
        __syncthreads();                     // the previous chunk's operands are consumed
        stage_x(d0);
#pragma unroll
        for (int q = 0; q < PW_DC * PW_LC / PW_T; ++q) {
          const int e = q * PW_T + tid, dd = e / PW_LC, jj = e % PW_LC, d = d0 + dd, j = j0 + jj;
          const double w = a.Om[(int64_t)(d < D ? d : D - 1) * L + (j < L ? j : L - 1)];
          oms[dd * PW_OLD + jj] = (d < D && j < L) ? w : 0.0;
        }
        if (d0 == 0) {                       // [Wc; Ws] of the chunk, outputs o0 .. o0 + 32
#pragma unroll
          for (int q = 0; q < 2 * PW_LC * PW_OC * PW_OG / PW_T; ++q) {
            const int e = q * PW_T + tid, half = e / (PW_LC * PW_OC * PW_OG), f = e % (PW_LC * PW_OC * PW_OG);
            const int jj = f / (PW_OC * PW_OG), oo = f % (PW_OC * PW_OG), j = j0 + jj, o = o0 + oo;
            const double w = (half ? Ws : Wc)[(int64_t)(j < L ? j : L - 1) * DO + (o < DO ? o : DO - 1)];
            wsm[(half * PW_LC + jj) * PW_WLD + oo] = (j < L && o < DO) ? w : 0.0;
          }
        }
        __syncthreads();
        const int kmax = D - d0 < PW_DC ? D - d0 : PW_DC;
        for (int k = 0; k < kmax; k += 4) {  // a ragged group reads the +0.0 rows of oms
          const double b = xs[xrow + k + g] - orgs[k + g];
#pragma unroll
          for (int jt = 0; jt < PW_LC / 16; ++jt) th[jt] = mfma_f64(oms[(k + g) * PW_OLD + jt * 16 + c], b, th[jt]);
        }
      }
#pragma unroll
      for (int jt = 0; jt < PW_LC / 16; ++jt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          double sn, cs;
          pw_sincos(th[jt][t], sn, cs);
          const int jj = jt * 16 + 4 * t + g;
#pragma unroll
          for (int q = 0; q < PW_OG; ++q)
            if (o0 + q * PW_OC < DO) {
              af[q] = mfma_f64(wsm[jj * PW_WLD + q * PW_OC + c], cs, af[q]);
              af[q] = mfma_f64(wsm[(PW_LC + jj) * PW_WLD + q * PW_OC + c], sn, af[q]);
            }
        }
      }
    }

    // ---- the update: the inducing rows in tiles of PW_ZT, lane (g, c) the rows m0 + 4u + g against data row c
    for (int m0 = 0; m0 < M; m0 += PW_ZT) {
      double r2[PW_ZT / 4];
#pragma unroll
      for (int u = 0; u < PW_ZT / 4; ++u) r2[u] = 0.0;
      for (int d0 = 0; d0 < D; d0 += PW_DC) {
        __syncthreads();
        stage_x(d0);
#pragma unroll
        for (int q = 0; q < PW_ZT * PW_DC / PW_T; ++q) {
          const int e = q * PW_T + tid, mm = e / PW_DC, dd = e % PW_DC, d = d0 + dd, m = m0 + mm;
          const double z = a.Z[(int64_t)(m < M ? m : M - 1) * D + (d < D ? d : D - 1)];
          zs[mm * PW_XLD + dd] = (m < M && d < D) ? z : 0.0;
        }
        if (tid < PW_DC) ilss[tid] = d0 + tid < D ? a.ils[d0 + tid] : 0.0;
        if (d0 == 0) {                       // V of the tile, outputs o0 .. o0 + 32
#pragma unroll
          for (int q = 0; q < PW_ZT * PW_OC * PW_OG / PW_T; ++q) {
            const int e = q * PW_T + tid, mm = e / (PW_OC * PW_OG), oo = e % (PW_OC * PW_OG), m = m0 + mm, o = o0 + oo;
            const double v = V[(int64_t)(m < M ? m : M - 1) * DO + (o < DO ? o : DO - 1)];
            wsm[mm * PW_WLD + oo] = (m < M && o < DO) ? v : 0.0;
          }
        }
        __syncthreads();
        const int kmax = D - d0 < PW_DC ? D - d0 : PW_DC;
        for (int dd = 0; dd < kmax; ++dd) {
          const double xv = xs[xrow + dd], il = ilss[dd];
#pragma unroll
          for (int u = 0; u < PW_ZT / 4; ++u) {
            const double t = (xv - zs[(4 * u + g) * PW_XLD + dd]) * il;
            r2[u] = fma(t, t, r2[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PW_ZT / 4; ++u) {
        const double kv = kern_val_rt(a.kind, r2[u], a.s2);
#pragma unroll
        for (int q = 0; q < PW_OG; ++q)
          if (o0 + q * PW_OC < DO) ak[q] = mfma_f64(wsm[(4 * u + g) * PW_WLD + q * PW_OC + c], kv, ak[q]);
      }
    }

    // ---- out^T: D register t of lane (g, c) is output o0 + 16 q + g + 4t of row c
    const int64_t r = r0 + wave * 16 + c;
    if (r < n) {
#pragma unroll
      for (int q = 0; q < PW_OG; ++q) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int o = o0 + q * PW_OC + g + 4 * t;
          if (o < DO) {
            double v = fma(a.amp, af[q][t], ak[q][t]);
            if (a.add) v += a.add[s * a.add_stride + r * a.ld_add + o];
            a.out[s * a.out_stride + r * a.ld_out + o] = v;
          }
        }
      }
    }
  }
}

// U[m][s DO + o] = q_mu[m][o] + sum_{k <= m} q_sqrt[o][m][k] eps[s][k][o], ascending k; q_sqrt NULL: q_mu
__global__ __launch_bounds__(256) void k_pw_u(const double* __restrict__ q_mu, const double* __restrict__ q_sqrt, const double* __restrict__ eps,
                                              int M, int DO, int S, double* __restrict__ U) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, wide = (int64_t)S * DO;
  if (e >= (int64_t)M * wide) return;
  const int m = (int)(e / wide), col = (int)(e - (int64_t)m * wide), s = col / DO, o = col - s * DO;
  double acc = 0.0;
  if (q_sqrt)
    for (int k = 0; k <= m; ++k) acc = fma(q_sqrt[((int64_t)o * M + m) * M + k], eps[((int64_t)s * M + k) * DO + o], acc);
  U[e] = q_mu[(int64_t)m * DO + o] + acc;
}

// in place: T = U - F0
__global__ __launch_bounds__(256) void k_pw_sub(const double* __restrict__ U, int64_t count, double* __restrict__ F0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < count) F0[e] = U[e] - F0[e];
}

// V[s][m][o] = T[m][s DO + o]
__global__ __launch_bounds__(256) void k_pw_unwide(const double* __restrict__ T, int M, int DO, int S, double* __restrict__ V) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, wide = (int64_t)S * DO;
  if (e >= (int64_t)M * wide) return;
  const int m = (int)(e / wide), col = (int)(e - (int64_t)m * wide), s = col / DO, o = col - s * DO;
  V[((int64_t)s * M + m) * DO + o] = T[e];
}

// Zc = Z - Z[0]: dsdgp_gram expands |x|^2 + |z|^2 - 2 x.z for D <= 32, which costs nothing around the origin only
__global__ __launch_bounds__(256) void k_pw_center(const double* __restrict__ Z, int64_t count, int D, double* __restrict__ Zc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < count) Zc[e] = Z[e] - Z[e % D];
}

static int pw_check_kernel(const dsdgp_kernel* kern) {
  DS_CHECK_ARG(kern && kern->input_dim > 0 && kern->lengthscales && kern->variance >= 0.0);
  if (kern->kind != DSDGP_KERN_RBF && kern->kind != DSDGP_KERN_MATERN52) {
    dsdgp_set_error("%s:%d: the pathwise draws know the spectral density of the RBF and the Matern52 kernel, not of kind %d", __FILE__,
                    __LINE__, kern->kind);
    return DSDGP_ERR_UNSUPPORTED;
  }
  return DSDGP_OK;
}

static int pw_check_eval(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, int64_t x_stride, int32_t S,
                         const double* Omega, const double* origin, int32_t L, const double* Wc, const double* Ws, const double* Z, int32_t M,
                         const double* V, int32_t DO, const double* add, int64_t ld_add, int64_t add_stride, double* out, int64_t ld_out) {
  DS_CHECK_ARG(ctx && X && Omega && origin && Wc && Ws && out);
  DS_TRY(pw_check_kernel(kern));
  DS_CHECK_ARG(n >= 1 && S >= 1 && L >= 1 && M >= 0 && DO >= 1 && ld_out >= DO);
  DS_CHECK_ARG(M == 0 || (Z && V));
  DS_CHECK_ARG(x_stride == 0 || x_stride == n * (int64_t)kern->input_dim);
  DS_CHECK_ARG(!add || (ld_add >= DO && add_stride >= 0));
  if (L > PW_MAX_L || M > PW_MAX_M || S > PW_MAX_S || n >= PW_MAX_ROWS || n * (int64_t)S >= PW_MAX_ROWS) {
    dsdgp_set_error("%s:%d: a pathwise evaluation takes L <= %d frequencies, M <= %d inducing rows, S <= %d draws and fewer than 2^31 rows "
                    "in all, not L = %d, M = %d, S = %d, n = %lld", __FILE__, __LINE__, PW_MAX_L, PW_MAX_M, PW_MAX_S, L, M, S, (long long)n);
    return DSDGP_ERR_UNSUPPORTED;
  }
  return DSDGP_OK;
}

// the launch; out_stride: doubles between the draws of `out` (dsdgp_pathwise_eval: n ld_out)
static int pw_launch(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, int64_t x_stride, int S, const double* Omega,
                     const double* origin, int L, const double* Wc, const double* Ws, const double* Z, int M, const double* V, int DO,
                     const double* add, int64_t ld_add, int64_t add_stride, double* out, int64_t ld_out, int64_t out_stride) {
  const int D = kern->input_dim;
  std::vector<double> ils(D);
  for (int d = 0; d < D; ++d) ils[d] = 1.0 / kern->lengthscales[kern->ard ? d : 0];
  void* dev = nullptr;
  DS_TRY(ctx_scratch(ctx, (size_t)D * 8, &dev));
  DS_TRY(ctx_upload(ctx, dev, ils.data(), (size_t)D * 8));
  PWArgs a{};
  a.X = X, a.Om = Omega, a.org = origin, a.Wc = Wc, a.Ws = Ws, a.Z = Z, a.V = V, a.ils = (const double*)dev, a.add = add, a.out = out;
  a.n = n, a.x_stride = x_stride, a.ld_add = ld_add, a.add_stride = add_stride, a.ld_out = ld_out, a.out_stride = out_stride;
  a.D = D, a.L = L, a.M = M, a.DO = DO, a.kind = kern->kind;
  a.amp = sqrt(kern->variance / (double)L), a.s2 = kern->variance;
  ProfScope ps(ctx, "pathwise");
  DS_LAUNCH(k_pw_eval, dim3((unsigned)((n + PW_RT - 1) / PW_RT), (unsigned)S), dim3(PW_T), 0, ctx->stream, a);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_pathwise_eval(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, int64_t x_stride, int32_t S,
                                   const double* Omega, const double* origin, int32_t L, const double* Wc, const double* Ws, const double* Z,
                                   int32_t M, const double* V, int32_t DO, const double* add, int64_t ld_add, int64_t add_stride, double* out,
                                   int64_t ld_out) {
  DS_TRY(pw_check_eval(ctx, kern, X, n, x_stride, S, Omega, origin, L, Wc, Ws, Z, M, V, DO, add, ld_add, add_stride, out, ld_out));
  return pw_launch(ctx, kern, X, n, x_stride, S, Omega, origin, L, Wc, Ws, Z, M, V, DO, add, ld_add, add_stride, out, ld_out, n * ld_out);
}

extern "C" int dsdgp_pathwise_scratch_bytes(int32_t M, int32_t D, int32_t DO, int32_t S, int64_t* bytes) {
  DS_CHECK_ARG(bytes && M >= 1 && M <= PW_MAX_M && D >= 1 && DO >= 1 && S >= 1 && S <= PW_MAX_S);
  *bytes = (int64_t)pathwise_scratch(M, D, DO, S).total;
  return DSDGP_OK;
}

extern "C" int dsdgp_pathwise_weights(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* Omega,
                                      const double* origin, int32_t L, const double* Wc, const double* Ws, int32_t S, const double* q_mu,
                                      const double* q_sqrt, const double* eps, int32_t DO, int32_t white, double jitter, void* scratch,
                                      int64_t scratch_bytes, double* V, int* info) {
  DS_CHECK_ARG(ctx && Z && Omega && origin && Wc && Ws && q_mu && scratch && V && (eps || !q_sqrt));
  DS_TRY(pw_check_kernel(kern));
  DS_CHECK_ARG(M >= 1 && M <= PW_MAX_M && L >= 1 && DO >= 1 && S >= 1);
  const int D = kern->input_dim;
  const int64_t wide = (int64_t)S * DO;
  if (L > PW_MAX_L || S > PW_MAX_S || wide > (1 << 30)) {
    dsdgp_set_error("%s:%d: the pathwise weights take L <= %d frequencies, S <= %d draws and S DO <= 2^30, not L = %d, S = %d, DO = %d",
                    __FILE__, __LINE__, PW_MAX_L, PW_MAX_S, L, S, DO);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const PWScratch P = pathwise_scratch(M, D, DO, S);
  if (P.total > PW_SCRATCH_CAP) {
    dsdgp_set_error("%s:%d: the weights of %d draws of %d outputs on %d inducing points would take %zu bytes of scratch (more than 8 GB): "
                    "draw fewer functions at a time", __FILE__, __LINE__, S, DO, M, P.total);
    return DSDGP_ERR_UNSUPPORTED;
  }
  DS_CHECK_ARG(scratch_bytes >= 0 && (size_t)scratch_bytes >= P.total);
  char* scr = (char*)scratch;
  double *Zc = (double*)(scr + P.Zc.off), *Lu = (double*)(scr + P.Ku.off), *U = (double*)(scr + P.U.off), *LU = (double*)(scr + P.LU.off),
         *F0 = (double*)(scr + P.F0.off);
  hipStream_t st = ctx->stream;
  int status = 0;
  DS_LAUNCH(k_pw_center, dim3(ceil_div((int64_t)M * D, 256)), dim3(256), 0, st, Z, (int64_t)M * D, D, Zc);
  DS_TRY(dsdgp_gram(ctx, kern, Zc, M, nullptr, 0, jitter, Lu, M));
  const int rc = dsdgp_potrf(ctx, 1, M, Lu, M, 0, &status);
  if (info) *info = status;
  DS_TRY(rc);
  const int blocks = ceil_div((int64_t)M * wide, 256);
  DS_LAUNCH(k_pw_u, dim3(blocks), dim3(256), 0, st, q_mu, q_sqrt, eps, (int)M, (int)DO, (int)S, U);
  if (white) DS_TRY(dsdgp_gemm(ctx, 0, 0, M, (int)wide, M, 1.0, Lu, M, U, wide, 0.0, LU, wide));
  // f0(Z): column s DO + o of row m, so ld_out = S DO and the draws DO apart
  DS_TRY(pw_launch(ctx, kern, Z, M, 0, S, Omega, origin, L, Wc, Ws, nullptr, 0, nullptr, DO, nullptr, 0, 0, F0, wide, DO));
  DS_LAUNCH(k_pw_sub, dim3(blocks), dim3(256), 0, st, white ? LU : U, (int64_t)M * wide, F0);
  DS_TRY(dsdgp_trsm(ctx, 0, M, wide, Lu, M, F0, wide));
  DS_TRY(dsdgp_trsm(ctx, 1, M, wide, Lu, M, F0, wide));
  DS_LAUNCH(k_pw_unwide, dim3(blocks), dim3(256), 0, st, F0, (int)M, (int)DO, (int)S, V);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// A stack of sparse sampled layers and its reverse pass: the reference's DGP_Base (dgp.py:42-98) over SGPMC_Layer (layers.py:249-260) at
// every depth — the SVGP conditional without q_sqrt (layers.py:178-219, line 200), a draw between the layers (layers.py:76-119,
// utils.py:40-41), the last layer not sampled (dgp.py:78-90) — with the log density
//   data_scale / S * sum_{s, i, d} E_q[log p(y | f)]  +  sum_l ( -1/2 sum q_mu_l^2 - 1/2 M_l DO_l log 2 pi )
// and its gradient in Z, q_mu and the kernel of every layer and in the likelihood's parameter.  Row r = s n + i, R = S n.
//
// Composed from the library's own calls — dsdgp_sparse_conditional[_grad], dsdgp_randn, dsdgp_gemm, dsdgp_lik_elbo_readout /
// dsdgp_multiclass_readout, dsdgp_gram, dsdgp_potrf — which use the context's scratch, so everything that lives from one call to the next
// is in a block the CALLER holds, carved by sgpmc_stack_plan.hpp.  New here, all element-wise or one fixed-order reduction:
// k_stack_tile: Xin[0] = X repeated S times.
// k_stack_hop: Fmean = cm + m(Xin), F = [Xin[:, :p] | Fmean + z sqrt(var + jitter)], one thread per entry of F, written into the next
//   layer's input.  A Linear mean's Xin A comes from dsdgp_gemm ahead of the kernel; the kernel adds b.
// k_stack_hop_bwd: from dF, one thread per row: gm = dF[:, p:], gv = sum_o dF[r, p + o] z[r, o] / (2 sqrt(var_r + jitter)), ascending o.
// k_stack_dx_shares: after the layer's reverse pass has overwritten d_X, the Identity mean's share gm and the propagated columns' share
//   dF[:, :p] added into it (a Linear mean's gm A^T is a dsdgp_gemm with beta = 1 ahead of the kernel).
// k_stack_head_bcast: the one variance column repeated over the DY columns the read-outs take.
// k_stack_head: gm = -dmean, gv_r = -sum_d dvar[r, d] in ascending d (the read-outs return the adjoints of MINUS the data term).
// k_stack_prior: one workgroup per layer: -1/2 sum q_mu^2 - 1/2 M DO log 2 pi (a thread its entries in ascending order, then a fixed
//   tree), and -q_mu added into d_q_mu.
// k_stack_final: one workgroup: the read-out's block partials in ascending block order (thread 0 the data term, thread 1 d / d p0), the
//   priors in ascending layer order, the four result scalars and the likelihood parameter's entry of the gradient.
// k_sghmc_step: theta += v, then v = (1 - alpha) v + eta g + sqrt(2 alpha eta) xi (Chen, Fox and Guestrin 2014, eq. 15, noise estimate 0).
// No floating-point atomics; every summation order follows from sgpmc_stack_plan.hpp, that is from the shapes alone.
#include "common.hpp"
#include "sgpmc_stack_plan.hpp"

__global__ __launch_bounds__(STK_T) void k_stack_tile(const double* __restrict__ X, int64_t count, int64_t total, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (e < total) out[e] = X[e % count];
}

__global__ __launch_bounds__(STK_T) void k_stack_center(const double* __restrict__ Z, int64_t count, int D, double* __restrict__ Zc) {
  const int64_t e = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (e < count) Zc[e] = Z[e] - Z[e % D];
}

// m(Xin)[r][o]: Zero, Identity (D_in == DO), Linear (lin = Xin A, b may be NULL)
__device__ __forceinline__ double stack_mean(int kind, const double* __restrict__ Xin, int D, const double* __restrict__ lin,
                                             const double* __restrict__ b, int DO, int64_t r, int o) {
  if (kind == DSDGP_MEAN_IDENTITY) return Xin[r * D + o];
  if (kind == DSDGP_MEAN_LINEAR) return b ? lin[r * DO + o] + b[o] : lin[r * DO + o];
  return 0.0;
}

// one thread per entry (r, j) of F (R x (p + DO)); z == NULL: no sample (the last layer), only Fmean is formed
__global__ __launch_bounds__(STK_T) void k_stack_hop(const double* __restrict__ cm, const double* __restrict__ var,
                                                     const double* __restrict__ Xin, int D, int mean_kind, const double* __restrict__ lin,
                                                     const double* __restrict__ b, int p, int DO, const double* __restrict__ z,
                                                     double jitter, int64_t R, double* __restrict__ Fmean, double* __restrict__ F,
                                                     double* __restrict__ F_out) {
  const int W = p + DO;
  const int64_t e = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (e >= R * W) return;
  const int64_t r = e / W;
  const int j = (int)(e - r * W);
  double f;
  if (j < p) {
    f = Xin[r * D + j];
  } else {
    const int o = j - p;
    const double m = mean_kind == DSDGP_MEAN_ZERO ? cm[r * DO + o] : cm[r * DO + o] + stack_mean(mean_kind, Xin, D, lin, b, DO, r, o);
    if (Fmean) Fmean[r * DO + o] = m;
    if (!z) return;
    f = m + z[r * DO + o] * sqrt(var[r] + jitter);
  }
  if (F) F[e] = f;
  if (F_out) F_out[e] = f;
}

// one thread per row
__global__ __launch_bounds__(STK_T) void k_stack_hop_bwd(const double* __restrict__ dF, int p, int DO, const double* __restrict__ z,
                                                         const double* __restrict__ var, double jitter, int64_t R,
                                                         double* __restrict__ gm, double* __restrict__ gv) {
  const int64_t r = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (r >= R) return;
  const double* d = dF + r * (p + DO) + p;
  double a = 0.0;
  for (int o = 0; o < DO; ++o) {
    const double g = d[o];
    gm[r * DO + o] = g;
    a += g * z[r * DO + o];
  }
  gv[r] = a / (2.0 * sqrt(var[r] + jitter));
}

// one thread per entry of d_X (R x D): += gm (Identity, D == DO), then += dF[:, :p] in the first p columns
__global__ __launch_bounds__(STK_T) void k_stack_dx_shares(double* __restrict__ dX, int D, int identity, const double* __restrict__ gm,
                                                           const double* __restrict__ dF, int p, int W, int64_t R) {
  const int64_t e = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (e >= R * D) return;
  const int64_t r = e / D;
  const int j = (int)(e - r * D);
  double x = dX[e];
  if (identity) x += gm[e];
  if (dF && j < p) x += dF[r * W + j];
  dX[e] = x;
}

__global__ __launch_bounds__(STK_T) void k_stack_head_bcast(const double* __restrict__ var, int DY, int64_t R, double* __restrict__ varb) {
  const int64_t e = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (e < R * DY) varb[e] = var[e / DY];
}

// one thread per row
__global__ __launch_bounds__(STK_T) void k_stack_head(const double* __restrict__ dmean, const double* __restrict__ dvar, int DY, int64_t R,
                                                      double* __restrict__ gm, double* __restrict__ gv) {
  const int64_t r = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (r >= R) return;
  double a = 0.0;
  for (int d = 0; d < DY; ++d) {
    gm[r * DY + d] = -dmean[r * DY + d];
    a += dvar[r * DY + d];
  }
  gv[r] = -a;
}

__global__ __launch_bounds__(STK_T) void k_stack_prior(const double* __restrict__ q_mu, int64_t count, double* __restrict__ d_q_mu,
                                                       double* __restrict__ prior) {
  __shared__ double red[STK_T];
  double a = 0.0;
  for (int64_t e = threadIdx.x; e < count; e += STK_T) {
    const double q = q_mu[e];
    a = fma(q, q, a);
    if (d_q_mu) d_q_mu[e] -= q;
  }
  a = block_sum<STK_T>(a, red);
  if (threadIdx.x == 0) *prior = -0.5 * a - 0.5 * (double)count * 1.8378770664093454835606594728112;      // log 2 pi
}

// part: the read-out's [blocks][2] partials, or with ve != NULL the per-row values of MultiClass (a thread its rows in ascending order,
// then a fixed tree)
__global__ __launch_bounds__(STK_T) void k_stack_final(const double* __restrict__ part, int blocks, const double* __restrict__ ve,
                                                       int64_t R, const double* __restrict__ prior, int L, double w,
                                                       double* __restrict__ grad_lik, double* __restrict__ out) {
  __shared__ double red[STK_T];
  __shared__ double s[2];
  const int tid = threadIdx.x;
  if (ve) {
    double a = 0.0;
    for (int64_t r = tid; r < R; r += STK_T) a += ve[r];
    a = block_sum<STK_T>(a, red);
    if (tid == 0) s[0] = a, s[1] = 0.0;
  } else if (tid < 2) {
    double a = 0.0;
    for (int b = 0; b < blocks; ++b) a += part[2 * b + tid];
    s[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    double pr = 0.0;
    for (int l = 0; l < L; ++l) pr += prior[l];
    const double data = w * s[0];
    out[0] = data + pr;
    out[1] = data;
    out[2] = pr;
    out[3] = 0.0;
    if (grad_lik) *grad_lik = w * s[1];
  }
}

__global__ __launch_bounds__(STK_T) void k_sghmc_step(int64_t count, double* __restrict__ theta, double* __restrict__ v,
                                                      const double* __restrict__ g, const double* __restrict__ xi, double alpha, double eta,
                                                      double noise) {
  const int64_t e = (int64_t)blockIdx.x * STK_T + threadIdx.x;
  if (e >= count) return;
  const double v0 = v[e];
  theta[e] += v0;
  double v1 = (1.0 - alpha) * v0 + eta * g[e];
  if (alpha != 0.0) v1 += noise * xi[e];
  v[e] = v1;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
static bool lik_known(int kind) { return kind >= DSDGP_LIK_GAUSSIAN && kind <= DSDGP_LIK_BETA; }

static int stack_shape(const dsdgp_stack_desc* d, int64_t n, int32_t S, StackShape* s) {
  DS_CHECK_ARG(d && d->L >= 1 && d->L <= STK_MAX_L && n >= 1 && S >= 1 && d->lik_width >= 1);
  s->L = d->L, s->n = n, s->S = S, s->DY = d->lik_width;
  for (int l = 0; l < d->L; ++l) {
    const dsdgp_stack_layer& y = d->layers[l];
    s->M[l] = y.M, s->D[l] = y.kern.input_dim, s->DO[l] = y.DO, s->p[l] = y.input_prop_dim;
  }
  return DSDGP_OK;
}

// everything that can be refused before a launch
static int stack_check(const dsdgp_stack_desc* d, const StackPlan& P, bool reverse) {
  if (!P.ok) {
    dsdgp_set_error("%s:%d: the stack's shapes do not chain: 1 <= M <= %d, input_dim[l + 1] = input_prop_dim[l] + DO[l], the last layer "
                    "with input_prop_dim 0 and DO = the likelihood's width, S n < 2^31", __FILE__, __LINE__, SC_MAX_M);
    return DSDGP_ERR_BAD_ARG;
  }
  DS_CHECK_ARG(lik_known(d->lik_kind));
  DS_CHECK_ARG(d->lik_kind != DSDGP_LIK_MULTICLASS || (d->lik_width >= 2 && d->lik_width <= 32));
  for (int l = 0; l < d->L; ++l) {
    const dsdgp_stack_layer& y = d->layers[l];
    DS_CHECK_ARG(y.Z && y.q_mu && y.kern.lengthscales);
    DS_CHECK_ARG(y.kern.kind == DSDGP_KERN_RBF || y.kern.kind == DSDGP_KERN_MATERN52);
    DS_CHECK_ARG(y.mean_kind == DSDGP_MEAN_ZERO || y.mean_kind == DSDGP_MEAN_IDENTITY || y.mean_kind == DSDGP_MEAN_LINEAR);
    DS_CHECK_ARG(y.mean_kind != DSDGP_MEAN_IDENTITY || y.kern.input_dim == y.DO);
    DS_CHECK_ARG(y.mean_kind != DSDGP_MEAN_LINEAR || y.mean_A);
    if (reverse && y.kern.input_dim > SC_MAX_D_GRAD) {
      dsdgp_set_error("%s:%d: the reverse pass of the stack goes through the reverse pass of the Gram matrix, which takes input_dim <= %d; "
                      "layer %d has %d", __FILE__, __LINE__, SC_MAX_D_GRAD, l, y.kern.input_dim);
      return DSDGP_ERR_UNSUPPORTED;
    }
  }
  if (P.total > SC_SCRATCH_CAP) {
    dsdgp_set_error("%s:%d: the stack of %d layers on %lld rows would take %zu bytes of scratch (more than 8 GB): pass the rows in batches",
                    __FILE__, __LINE__, d->L, (long long)P.R, P.total);
    return DSDGP_ERR_UNSUPPORTED;
  }
  return DSDGP_OK;
}

// every layer's Ku factorised as dsdgp_sparse_conditional will factorise it (the same calls on the same numbers): a failure is known
// before anything is written
static int stack_factor_check(dsdgp_ctx* ctx, const dsdgp_stack_desc* d, const StackPlan& P, char* scr, int* info) {
  double *Zc = (double*)(scr + P.Zc.off), *Ku = (double*)(scr + P.Ku.off);
  if (info) *info = 0;
  for (int l = 0; l < d->L; ++l) {
    const dsdgp_stack_layer& y = d->layers[l];
    const int M = y.M, D = y.kern.input_dim;
    int status = 0;
    DS_LAUNCH(k_stack_center, dim3(ceil_div((int64_t)M * D, STK_T)), dim3(STK_T), 0, ctx->stream, y.Z, (int64_t)M * D, D, Zc);
    DS_TRY(dsdgp_gram(ctx, &y.kern, Zc, M, nullptr, 0, d->jitter, Ku, M));
    const int rc = dsdgp_potrf(ctx, 1, M, Ku, M, 0, &status);
    if (info && status) *info = status;
    DS_TRY(rc);
  }
  return DSDGP_OK;
}

struct StackRun {
  dsdgp_ctx* ctx;
  const dsdgp_stack_desc* d;
  StackPlan P;
  char* scr;
  const double* zs[STK_MAX_L];      // the draws in use: the caller's or the scratch's
  double* at(const SCRegion& r) const { return (double*)(scr + r.off); }
};

// the forward pass into the scratch; F_out / mean_out / var_out: the caller's optional copies
static int stack_forward(StackRun& run, const double* X, const double* const* zs, uint64_t seed, double* const* F_out,
                         double* const* mean_out, double* const* var_out) {
  dsdgp_ctx* ctx = run.ctx;
  const dsdgp_stack_desc* d = run.d;
  const StackPlan& P = run.P;
  hipStream_t st = ctx->stream;
  const int64_t R = P.R;
  const int L = d->L;
  {
    const int64_t total = R * d->layers[0].kern.input_dim;
    DS_LAUNCH(k_stack_tile, dim3(ceil_div(total, STK_T)), dim3(STK_T), 0, st, X, P.n * d->layers[0].kern.input_dim, total, run.at(P.Xin[0]));
  }
  for (int l = 0; l < L; ++l) {
    const dsdgp_stack_layer& y = d->layers[l];
    const int D = y.kern.input_dim, DO = y.DO, p = y.input_prop_dim;
    const bool last = l + 1 == L;
    double *Xin = run.at(P.Xin[l]), *cm = run.at(P.cm[l]), *var = run.at(P.var[l]);
    int status = 0;
    DS_TRY(dsdgp_sparse_conditional(ctx, &y.kern, y.Z, y.M, Xin, R, y.q_mu, DO, y.white, d->jitter, run.at(P.sc), (int64_t)P.sc_bytes, cm,
                                    var, &status));
    const double* lin = nullptr;
    if (y.mean_kind == DSDGP_MEAN_LINEAR) {
      DS_TRY(dsdgp_gemm(ctx, 0, 0, (int)R, DO, D, 1.0, Xin, D, y.mean_A, DO, 0.0, run.at(P.lin), DO));
      lin = run.at(P.lin);
    }
    const double* z = nullptr;
    if (!last) {
      z = zs && zs[l] ? zs[l] : nullptr;
      if (!z) {
        DS_TRY(dsdgp_randn(ctx, seed, (uint64_t)l, R * DO, run.at(P.z[l])));
        z = run.at(P.z[l]);
      }
    }
    run.zs[l] = z;
    ProfScope ps(ctx, "stack_hop");
    double* Fmean = last ? run.at(P.fmean) : (mean_out ? mean_out[l] : nullptr);
    DS_LAUNCH(k_stack_hop, dim3((unsigned)P.hop_blocks[l]), dim3(STK_T), 0, st, cm, var, Xin, D, (int)y.mean_kind, lin, y.mean_b, p, DO, z,
              d->jitter, R, Fmean, last ? nullptr : run.at(P.Xin[l + 1]), last || !F_out ? nullptr : F_out[l]);
    if (last && mean_out && mean_out[l])
      DS_HIP(hipMemcpyAsync(mean_out[l], Fmean, (size_t)R * DO * 8, hipMemcpyDeviceToDevice, st));
    if (var_out && var_out[l]) DS_HIP(hipMemcpyAsync(var_out[l], var, (size_t)R * 8, hipMemcpyDeviceToDevice, st));
  }
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

static int stack_begin(dsdgp_ctx* ctx, const dsdgp_stack_desc* desc, const double* X, int64_t n, int32_t S, void* scratch,
                       int64_t scratch_bytes, bool reverse, int* info, StackRun* run) {
  DS_CHECK_ARG(ctx && desc && X && scratch);
  StackShape s{};
  DS_TRY(stack_shape(desc, n, S, &s));
  run->ctx = ctx, run->d = desc, run->scr = (char*)scratch;
  run->P = sgpmc_stack_plan(s, reverse);
  DS_TRY(stack_check(desc, run->P, reverse));
  DS_CHECK_ARG(scratch_bytes >= 0 && (size_t)scratch_bytes >= run->P.total);
  return stack_factor_check(ctx, desc, run->P, run->scr, info);
}

extern "C" int dsdgp_sizeof_stack_desc(void) { return (int)sizeof(dsdgp_stack_desc); }

extern "C" int dsdgp_stack_scratch_bytes(const dsdgp_stack_desc* desc, int64_t n, int32_t S, int32_t reverse, int64_t* bytes) {
  DS_CHECK_ARG(bytes);
  StackShape s{};
  DS_TRY(stack_shape(desc, n, S, &s));
  const StackPlan P = sgpmc_stack_plan(s, reverse != 0);
  DS_TRY(stack_check(desc, P, reverse != 0));
  *bytes = (int64_t)P.total;
  return DSDGP_OK;
}

extern "C" int dsdgp_stack_propagate(dsdgp_ctx* ctx, const dsdgp_stack_desc* desc, const double* X, int64_t n, int32_t S,
                                     const double* const* zs, uint64_t seed, void* scratch, int64_t scratch_bytes, double* const* F_out,
                                     double* const* mean_out, double* const* var_out, int* info) {
  StackRun run{};
  DS_TRY(stack_begin(ctx, desc, X, n, S, scratch, scratch_bytes, false, info, &run));
  DS_TRY(stack_forward(run, X, zs, seed, F_out, mean_out, var_out));
  // the last layer is not sampled (dgp.py:78-90): its F is its mean
  const int l = desc->L - 1;
  if (F_out && F_out[l])
    DS_HIP(hipMemcpyAsync(F_out[l], run.at(run.P.fmean), (size_t)run.P.R * desc->layers[l].DO * 8, hipMemcpyDeviceToDevice, ctx->stream));
  return DSDGP_OK;
}

extern "C" int dsdgp_stack_logdensity(dsdgp_ctx* ctx, const dsdgp_stack_desc* desc, const double* X, const double* Y, int64_t n, int32_t S,
                                      const double* const* zs, uint64_t seed, double data_scale, void* scratch, int64_t scratch_bytes,
                                      double* out, double* grad, int* info) {
  DS_CHECK_ARG(Y && out);
  StackRun run{};
  DS_TRY(stack_begin(ctx, desc, X, n, S, scratch, scratch_bytes, grad != nullptr, info, &run));
  DS_TRY(stack_forward(run, X, zs, seed, nullptr, nullptr, nullptr));
  const StackPlan& P = run.P;
  hipStream_t st = ctx->stream;
  const int L = desc->L, DY = P.DY;
  const int64_t R = P.R;
  const double w = data_scale / (double)S;
  const bool mc = desc->lik_kind == DSDGP_LIK_MULTICLASS;
  // head: the likelihood on the last layer's mean and its one variance column
  {
    ProfScope ps(ctx, "stack_head");
    DS_LAUNCH(k_stack_head_bcast, dim3((unsigned)P.head_blocks), dim3(STK_T), 0, st, run.at(P.var[L - 1]), DY, R, run.at(P.varb));
    if (mc)
      DS_TRY(dsdgp_multiclass_readout(ctx, run.at(P.fmean), run.at(P.varb), Y, n, S, DY, w, nullptr, run.at(P.ve), run.at(P.dmean),
                                      run.at(P.dvar)));
    else
      DS_TRY(dsdgp_lik_elbo_readout(ctx, desc->lik_kind, desc->lik_p0, desc->lik_p1, run.at(P.fmean), run.at(P.varb), Y, n, S, DY, w, nullptr,
                                    run.at(P.part), run.at(P.dmean), run.at(P.dvar), nullptr, nullptr, 0));
  }
  // the gradient's layout: per layer d_Z (M x D), d_q_mu (M x DO), d_kern (2 + lengthscale entries), then the likelihood parameter's entry
  double* g = grad;
  double *gZ[STK_MAX_L], *gq[STK_MAX_L], *gk[STK_MAX_L];
  for (int l = 0; l < L && grad; ++l) {
    const dsdgp_stack_layer& y = desc->layers[l];
    const int D = y.kern.input_dim;
    gZ[l] = g, g += (int64_t)y.M * D;
    gq[l] = g, g += (int64_t)y.M * y.DO;
    gk[l] = g, g += 2 + (y.kern.ard ? D : 1);
  }
  if (grad) {
    double *gm = run.at(P.gm), *gv = run.at(P.gv);
    DS_LAUNCH(k_stack_head, dim3((unsigned)P.row_blocks), dim3(STK_T), 0, st, run.at(P.dmean), run.at(P.dvar), DY, R, gm, gv);
    for (int l = L - 1; l >= 0; --l) {
      const dsdgp_stack_layer& y = desc->layers[l];
      const int D = y.kern.input_dim, DO = y.DO, p = y.input_prop_dim;
      double* dX = l > 0 ? run.at(P.dX[l & 1]) : nullptr;                 // the model's inputs have no gradient
      const double* dF = l + 1 < L ? run.at(P.dX[(l + 1) & 1]) : nullptr; // the adjoint of this layer's F = the next layer's input
      if (dF) {
        ProfScope ps(ctx, "stack_hop_bwd");
        DS_LAUNCH(k_stack_hop_bwd, dim3((unsigned)P.row_blocks), dim3(STK_T), 0, st, dF, p, DO, run.zs[l], run.at(P.var[l]), desc->jitter, R,
                  gm, gv);
      }
      int status = 0;
      DS_TRY(dsdgp_sparse_conditional_grad(ctx, &y.kern, y.Z, y.M, run.at(P.Xin[l]), R, y.q_mu, DO, y.white, desc->jitter, gm, gv,
                                           run.at(P.sc), (int64_t)P.sc_bytes, gq[l], gZ[l], dX, gk[l], &status));
      if (dX) {
        if (y.mean_kind == DSDGP_MEAN_LINEAR) DS_TRY(dsdgp_gemm(ctx, 0, 1, (int)R, D, DO, 1.0, gm, DO, y.mean_A, DO, 1.0, dX, D));
        if (y.mean_kind == DSDGP_MEAN_IDENTITY || (dF && p > 0))
          DS_LAUNCH(k_stack_dx_shares, dim3(ceil_div(R * D, STK_T)), dim3(STK_T), 0, st, dX, D, y.mean_kind == DSDGP_MEAN_IDENTITY ? 1 : 0,
                    (const double*)gm, dF, p, p + DO, R);
      }
    }
  }
  for (int l = 0; l < L; ++l) {
    const dsdgp_stack_layer& y = desc->layers[l];
    DS_LAUNCH(k_stack_prior, dim3(1), dim3(STK_T), 0, st, y.q_mu, (int64_t)y.M * y.DO, grad ? gq[l] : nullptr, run.at(P.prior) + l);
  }
  DS_LAUNCH(k_stack_final, dim3(1), dim3(STK_T), 0, st, (const double*)run.at(P.part), P.head_blocks, mc ? (const double*)run.at(P.ve) : nullptr,
            R, (const double*)run.at(P.prior), L, w, grad ? g : nullptr, out);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// the hop and its reverse as calls of their own: the launches of the composed calls, on the caller's arrays
extern "C" int dsdgp_stack_hop(dsdgp_ctx* ctx, const double* cm, const double* var, const double* Xin, int64_t R, int32_t D_in,
                               int32_t mean_kind, const double* lin, const double* b, int32_t p, int32_t DO, const double* z, double jitter,
                               double* Fmean, double* F) {
  DS_CHECK_ARG(ctx && cm && var && Xin && z && F && R >= 1 && R < SC_MAX_ROWS && D_in >= 1 && DO >= 1 && p >= 0 && p <= D_in);
  DS_CHECK_ARG(mean_kind == DSDGP_MEAN_ZERO || (mean_kind == DSDGP_MEAN_IDENTITY && D_in == DO) || (mean_kind == DSDGP_MEAN_LINEAR && lin));
  DS_LAUNCH(k_stack_hop, dim3((unsigned)ceil_div(R * (p + DO), STK_T)), dim3(STK_T), 0, ctx->stream, cm, var, Xin, (int)D_in, (int)mean_kind,
            lin, b, (int)p, (int)DO, z, jitter, R, Fmean, F, (double*)nullptr);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_stack_hop_bwd(dsdgp_ctx* ctx, const double* dF, int64_t R, int32_t p, int32_t DO, const double* z, const double* var,
                                   double jitter, double* gm, double* gv) {
  DS_CHECK_ARG(ctx && dF && z && var && gm && gv && R >= 1 && R < SC_MAX_ROWS && DO >= 1 && p >= 0);
  DS_LAUNCH(k_stack_hop_bwd, dim3((unsigned)ceil_div(R, STK_T)), dim3(STK_T), 0, ctx->stream, dF, (int)p, (int)DO, z, var, jitter, R, gm, gv);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_sghmc_step(dsdgp_ctx* ctx, int64_t count, double* theta, double* v, const double* g, const double* xi, double alpha,
                                double eta) {
  DS_CHECK_ARG(ctx && theta && v && g && count >= 1);
  DS_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0 && eta > 0.0);
  DS_CHECK_ARG(alpha == 0.0 || xi);
  DS_LAUNCH(k_sghmc_step, dim3(ceil_div(count, STK_T)), dim3(STK_T), 0, ctx->stream, count, theta, v, g, xi, alpha, eta,
            sqrt(2.0 * alpha * eta));
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

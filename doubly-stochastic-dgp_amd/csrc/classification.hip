// Classification report of the predictive mixture on the device: the class probabilities averaged over the S mixture components, and
// from them calibration (reliability bins, expected calibration error), the Brier score, the rank of the label and the confusion counts —
// what a user of the MultiClass / Bernoulli models would otherwise compute on the host from predict_y outputs (dgp.py:116-126).
//   MultiClass(K), RobustMax(eps = 1e-3), 20-point Gauss–Hermite, per component (s, i) and class k (multiclass.hip's arithmetic):
//     X_h = mu_k + x_h sqrt(2 max(v_k, 0.5e-10)) ;  cdf_jh = (1 + erf((X_h - mu_j) rsqrt(2 max(v_j, 1e-10)))) / 2 (1 - 2e-4) + 1e-4
//     pt = sum_h w_h prod_{j != k} cdf_jh ;  p_k = pt (1 - eps) + (1 - pt) eps / (K - 1) ;  pbar[i, k] = (1/S) sum_s p_{s,i,k}
//   Bernoulli (probit): p[i, d] = (1/S) sum_s bern_probit(mu / sqrt(1 + v)); every output its own two-class problem, pi = (1 - p, p)
//   per row (Bernoulli: per (i, d)), label y:  c^ = argmax_c pi_c (ties: the lowest c), conf = pi_c^, err = [c^ != y], l = log pi_y,
//     brier = sum_c (pi_c - [c = y])^2, rank = #{c : pi_c > pi_y} + #{c < y : pi_c == pi_y}, bin = min(B - 1, floor(conf B))
// k_cls_probs is bound by fp64 erf: 20 K (K - 1) per (s, i), each row's K (mu, sqrt(2 v), rsqrt(2 v)) formed once and shared through LDS.
// Every reduction runs in a fixed order: the same inputs and n give the same bits.
#include <math.h>

#include "gauss_hermite.hpp"
#include "likelihood.hpp"
#include "mixture_common.hpp"

#define CLS_KMAX 32       // MC_KMAX of multiclass.hip
#define CLS_BMAX 32       // reliability bins
#define CLS_HG 4          // node groups of a class integral, GH20_H / CLS_HG nodes each (k_multiclass's split and order of the node sum)
#define CLS_HN (GH20_H / CLS_HG)
#define CLS_WAVES (MIX_T / 64)
#define CLS_CH 8          // components a wave stages in LDS at a time
#define CLS_EPS 1e-3

__constant__ double c_cls_x[GH20_H];
__constant__ double c_cls_w[GH20_H];   // w_h / sqrt(pi)
static bool g_cls_gh_ready = false;

static int cls_ensure_gh(hipStream_t st) {
  if (g_cls_gh_ready) return DSDGP_OK;
  double x[GH20_H], w[GH20_H];
  gh20_nodes(x, w);
  DS_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_cls_x), x, sizeof(x), 0, hipMemcpyHostToDevice, st));
  DS_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_cls_w), w, sizeof(w), 0, hipMemcpyHostToDevice, st));
  DS_HIP(hipStreamSynchronize(st));
  g_cls_gh_ready = true;
  return DSDGP_OK;
}

// doubles of LDS a workgroup of k_cls_probs asks for: per wave CLS_CH components x K x (mu, sqrt(2 v), rsqrt(2 v), p), then the waves' sums
static inline size_t cls_probs_lds(int K) { return (size_t)(CLS_WAVES * 4 * CLS_CH * K + CLS_WAVES * K) * sizeof(double); }

// pbar (n x K) from mean / var ((S n) x K, row s n + i).  A workgroup of four waves takes 4 / wpr rows; the wpr waves of a row take the
// components s = sw, sw + wpr, ... CLS_CH at a time.  Within a chunk the (component, class, node group) units are flattened over the 64
// lanes: unit u -> c = u / 4K, k = (u % 4K) / 4, g = u % 4, so the four node groups of a class integral sit in adjacent lanes and a full
// chunk at K = 10 is exactly five rounds of 64.  A unit walks the other K - 1 classes once, five nodes (five independent erf) per class.
// Sums: five nodes by fma in node order, the four groups in group order, a wave's components in ascending s, the waves in wave order.
__global__ __launch_bounds__(MIX_T) void k_cls_probs(const double* __restrict__ mean, const double* __restrict__ var, int64_t n, int S,
                                                     int K, int wpr, double* __restrict__ pbar) {
  extern __shared__ double cls_lds[];
  __shared__ double gx[GH20_H], gw[GH20_H];
  const int tid = threadIdx.x, lane = tid & 63, w = DS_WAVE_ID(tid);
  const int rpb = CLS_WAVES / wpr, rl = w / wpr, sw = w % wpr;
  const int64_t row = (int64_t)blockIdx.x * rpb + rl;
  const int64_t rc = row < n ? row : n - 1;      // (every wave reaches the barriers)
  double* wm = cls_lds + (size_t)w * 4 * CLS_CH * K;      // mu
  double* ws = wm + CLS_CH * K;                           // sqrt(2 max(v, 0.5e-10))
  double* wr = ws + CLS_CH * K;                           // rsqrt(2 max(v, 1e-10))
  double* wp = wr + CLS_CH * K;                           // p of (component, class)
  double* wsum = cls_lds + (size_t)CLS_WAVES * 4 * CLS_CH * K;
  if (tid < GH20_H) { gx[tid] = c_cls_x[tid]; gw[tid] = c_cls_w[tid]; }
  // wpr <= S (the launcher), so every wave has cmax or cmax - 1 components: cnt >= 1 and cnt - c0 >= 0 in every chunk; a wave
  // with cmax - 1 sits out a last chunk that holds wave 0's one left-over component (nc = 0, e.g. S = 33: 9 | 8 | 8 | 8)
  const int cnt = (S - sw + wpr - 1) / wpr;                   // components of this wave
  const int cmax = (S + wpr - 1) / wpr;                       // ... of wave 0: the trip count every wave shares
  const int U = CLS_HG * K;
  const double e1 = 1.0 - CLS_EPS, e0 = CLS_EPS / (K - 1.0);
  double acc = 0.0;      // lane k < K: the sum of p_k over this wave's components
  for (int c0 = 0; c0 < cmax; c0 += CLS_CH) {
    const int nc = cnt - c0 < CLS_CH ? cnt - c0 : CLS_CH;
    for (int t = lane; t < nc * K; t += 64) {
      const int c = t / K, j = t - c * K;
      const int64_t s = sw + (int64_t)(c0 + c) * wpr;
      const int64_t at = (s * n + rc) * K + j;
      const double v = var[at];
      wm[t] = mean[at];
      ws[t] = sqrt(2.0 * fmax(v, 0.5e-10));
      wr[t] = rsqrt(2.0 * fmax(v, 1e-10));
    }
    __syncthreads();
    for (int u0 = 0; u0 < nc * U; u0 += 64) {
      const int u = u0 + lane;
      const bool act = u < nc * U;
      const int uu = act ? u : 0;
      const int c = uu / U, r = uu - c * U, k = r / CLS_HG, g = r % CLS_HG;
      const double* cm = wm + c * K;
      const double* cr = wr + c * K;
      const double muk = cm[k], syk = ws[c * K + k];
      double X[CLS_HN], P[CLS_HN];
#pragma unroll
      for (int q = 0; q < CLS_HN; ++q) {
        X[q] = muk + gx[g * CLS_HN + q] * syk;
        P[q] = 1.0;
      }
      for (int jj = 0; jj < K - 1; ++jj) {
        const int j = jj + (jj >= k);      // the other classes in ascending order
        const double mj = cm[j], rj = cr[j];
#pragma unroll
        for (int q = 0; q < CLS_HN; ++q) P[q] *= 0.5 * (1.0 + erf((X[q] - mj) * rj)) * (1.0 - 2e-4) + 1e-4;
      }
      double p = 0.0;
#pragma unroll
      for (int q = 0; q < CLS_HN; ++q) p = fma(gw[g * CLS_HN + q], P[q], p);
      const int l0 = lane & ~(CLS_HG - 1);
      const double pt = ((__shfl(p, l0) + __shfl(p, l0 + 1)) + __shfl(p, l0 + 2)) + __shfl(p, l0 + 3);
      if (act && g == 0) wp[c * K + k] = pt * e1 + (1.0 - pt) * e0;
    }
    __syncthreads();
    if (lane < K)
      for (int c = 0; c < nc; ++c) acc += wp[c * K + lane];
  }
  if (lane < K) wsum[w * K + lane] = acc;
  __syncthreads();
  if (tid < rpb * K) {
    const int r = tid / K, k = tid - r * K;
    double t = 0.0;
    for (int q = 0; q < wpr; ++q) t += wsum[(r * wpr + q) * K + k];
    const int64_t ro = (int64_t)blockIdx.x * rpb + r;
    if (ro < n) pbar[ro * K + k] = t / (double)S;
  }
}

// Bernoulli: p (n x DY) from mean / var ((S n) x DY); memory-bound, the lanes of an item split its components
template <int SPLIT>
__global__ __launch_bounds__(MIX_T) void k_cls_bern(const double* __restrict__ mean, const double* __restrict__ var, int64_t total, int S,
                                                    double* __restrict__ p_out) {
  const MixItem<SPLIT> it(total);
  const double* mp = mean + it.jc;
  const double* vp = var + it.jc;
  double sp = 0.0;
#pragma unroll 4
  for (int s = it.sub; s < S; s += SPLIT) sp += bern_probit(mp[(int64_t)s * total] / sqrt(1.0 + vp[(int64_t)s * total]));
  sp = fold_sum<SPLIT>(sp, it.sub);
  if (it.live && it.sub == 0) p_out[it.jc] = sp / (double)S;
}

struct ClsArgs {
  const double* probs;      // MultiClass: n x C class probabilities; Bernoulli: n x ND, p(y = 1)
  const double* Y;          // MultiClass: n x 1 labels; Bernoulli: n x ND targets (1 selects class 1, anything else class 0)
  double* rows;             // total x 4 [predicted class, conf, l, brier] or NULL
  double* part;             // E ND x nblocks partial sums: [q ND + d][block]
  int64_t total;            // items: n (MultiClass), n ND (Bernoulli)
  int C, B, ND, bern, nblocks;
};

// One thread per item; then the workgroup's E x ND partial sums, every one over its items in ascending order.
__global__ __launch_bounds__(MIX_T) void k_cls_report(const ClsArgs a) {
  __shared__ double e_err[MIX_T], e_l[MIX_T], e_br[MIX_T], e_cf[MIX_T];
  __shared__ int e_bin[MIX_T], e_rank[MIX_T], e_y[MIX_T], e_pred[MIX_T];
  const MixItem<1> it(a.total);
  const int tid = threadIdx.x, C = a.C, B = a.B;
  const int64_t jc = it.jc;
  // class probabilities straight from memory (no per-thread array: its run-time index would live in scratch)
  const double pb = a.bern ? a.probs[jc] : 0.0;
  const double* pr = a.probs + (a.bern ? 0 : jc * C);
  auto pi = [&](int c) { return a.bern ? (c ? pb : 1.0 - pb) : pr[c]; };
  int y;
  if (a.bern) {
    y = a.Y[jc] == 1.0 ? 1 : 0;
  } else {
    const double yl = a.Y[jc];
    y = yl >= (double)(C - 1) ? C - 1 : yl > 0.0 ? (int)yl : 0;      // clamped into 0 .. C - 1 (NaN: 0)
  }
  int best = 0;
  double conf = pi(0);
  for (int c = 1; c < C; ++c) {
    const double x = pi(c);
    if (x > conf) { conf = x; best = c; }      // ties: the lowest index (numpy.argmax)
  }
  const double piy = pi(y);
  double brier = 0.0;
  int rank = 0;
  for (int c = 0; c < C; ++c) {
    const double x = pi(c), r = x - (c == y ? 1.0 : 0.0);
    brier += r * r;
    rank += (x > piy || (x == piy && c < y)) ? 1 : 0;
  }
  const double ell = log(piy);
  const double fb = floor(conf * (double)B);
  const int bin = fb >= (double)(B - 1) ? B - 1 : fb > 0.0 ? (int)fb : 0;
  if (a.rows && it.live) {
    double* r = a.rows + jc * 4;
    r[0] = (double)best; r[1] = conf; r[2] = ell; r[3] = brier;
  }
  // items past the end match no count and add 0 to every sum
  e_err[tid] = it.live && best != y ? 1.0 : 0.0;
  e_l[tid] = it.live ? ell : 0.0;
  e_br[tid] = it.live ? brier : 0.0;
  e_cf[tid] = it.live ? conf : 0.0;
  e_bin[tid] = it.live ? bin : -1;
  e_rank[tid] = it.live ? rank : -1;
  e_y[tid] = it.live ? y : -1;
  e_pred[tid] = it.live ? best : -1;
  __syncthreads();
  const int ND = a.ND, E = 4 + 3 * B + C + C * C;
  for (int p = tid; p < E * ND; p += MIX_T) {
    const int d = p % ND, q = p / ND;
    a.part[(int64_t)p * a.nblocks + blockIdx.x] = sum_output_items(d, ND, it.j0, 0, MIX_T, [&](int e) -> double {
      if (q == 0) return e_err[e];
      if (q == 1) return e_l[e];
      if (q == 2) return e_br[e];
      if (q == 3) return e_bin[e] >= 0 ? 1.0 : 0.0;
      int z = q - 4;
      if (z < B) return e_bin[e] == z ? 1.0 : 0.0;
      z -= B;
      if (z < B) return e_bin[e] == z ? e_cf[e] : 0.0;
      z -= B;
      if (z < B) return e_bin[e] == z && e_pred[e] == e_y[e] ? 1.0 : 0.0;
      z -= B;
      if (z < C) return e_rank[e] == z ? 1.0 : 0.0;
      z -= C;
      return e_y[e] == z / C && e_pred[e] == z % C ? 1.0 : 0.0;
    });
  }
}

int mixture_classification_launch(dsdgp_ctx* ctx, int kind, const double* mean, const double* var, const double* Y, int64_t n, int S,
                                  int DY, int bins, double* probs_out, double* rows_out, double* acc, int accumulate) {
  const char* who = "dsdgp_mixture_classification";
  DS_CHECK_ARG(ctx && mean && var && Y && acc && n > 0 && S > 0 && DY > 0);
  if (kind != DSDGP_LIK_MULTICLASS && kind != DSDGP_LIK_BERNOULLI) {
    dsdgp_set_error("%s: likelihood kind %d has no classes; MultiClass and Bernoulli are covered", who, kind);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const bool mc = kind == DSDGP_LIK_MULTICLASS;
  if (mc && (DY < 2 || DY > CLS_KMAX)) {
    dsdgp_set_error("%s: MultiClass: K=%d outside [2, %d]", who, DY, CLS_KMAX);
    return DSDGP_ERR_UNSUPPORTED;
  }
  if (bins < 1 || bins > CLS_BMAX) {
    dsdgp_set_error("%s: bad argument: bins = %d, 1 .. %d are taken", who, bins, CLS_BMAX);
    return DSDGP_ERR_BAD_ARG;
  }
  const int C = mc ? DY : 2, ND = mc ? 1 : DY;
  const int E = 4 + 3 * bins + C + C * C;
  DS_CHECK_ARG(n <= INT64_MAX / DY / S && (int64_t)E * ND <= 0x7fffffff);
  const int64_t total = n * ND;
  int nblocks;
  DS_TRY(mix_nblocks(total, 1, &nblocks));
  DS_CHECK_ARG((int64_t)E * ND <= INT64_MAX / 8 / nblocks);
  const int entries = E * ND;
  const size_t part_doubles = (size_t)round_up((int64_t)entries * nblocks, 32);
  void* scr;
  DS_TRY(ctx_scratch(ctx, (part_doubles + (probs_out ? 0 : (size_t)n * DY)) * sizeof(double), &scr));
  double* probs = probs_out ? probs_out : (double*)scr + part_doubles;
  ProfScope prof(ctx, "classification");
  if (mc) {
    DS_TRY(cls_ensure_gh(ctx->stream));
    const int wpr = S >= 4 ? 4 : S >= 2 ? 2 : 1;      // waves per row: by S alone, so a row's bits do not depend on n
    const int64_t nb = (n + CLS_WAVES / wpr - 1) / (CLS_WAVES / wpr);
    DS_CHECK_ARG(nb <= 0x7fffffff);
    DS_LAUNCH(k_cls_probs, dim3((unsigned)nb), dim3(MIX_T), cls_probs_lds(DY), ctx->stream, mean, var, n, S, DY, wpr, probs);
  } else {
    const int split = mix_split_clamp(mix_split_by_items(total), S);
    int nb;
    DS_TRY(mix_nblocks(total, split, &nb));
    mix_dispatch_split(split, [&](auto sp) { DS_LAUNCH((k_cls_bern<decltype(sp)::value>), dim3(nb), dim3(MIX_T), 0, ctx->stream, mean, var, total, S, probs); });
  }
  ClsArgs a{};
  a.probs = probs; a.Y = Y; a.rows = rows_out; a.part = (double*)scr; a.total = total;
  a.C = C; a.B = bins; a.ND = ND; a.bern = mc ? 0 : 1; a.nblocks = nblocks;
  DS_LAUNCH(k_cls_report, dim3(nblocks), dim3(MIX_T), 0, ctx->stream, a);
  mixture_finish_launch(ctx->stream, (const double*)scr, nblocks, entries, ND, ND, accumulate, acc);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_mixture_classification(dsdgp_ctx* ctx, int32_t kind, const double* mean, const double* var, const double* Y,
                                            int64_t n, int32_t S, int32_t DY, int32_t bins, double* probs_out, double* rows_out,
                                            double* acc, int accumulate) {
  return mixture_classification_launch(ctx, kind, mean, var, Y, n, S, DY, bins, probs_out, rows_out, acc, accumulate);
}

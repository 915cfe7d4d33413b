// Held-out evaluation on the device: the per-row reduction over the S mixture components that the reference's experiment script does
// on the host (demos/run_regression.py:108-123 on predict_y outputs; dgp.py:116-126 predict_y / predict_density), and its three sums.
//   per (i, d):  mhat = mean_s E_s ;  mixture variance = mean_s (V_s + E_s^2) - mhat^2 ;  l = logsumexp_s log p(y | mean_s, var_s) - log S
//   per output:  sum_i (y - mhat)^2 (MultiClass: sum_i [argmax_k mhat_k != y]),  sum_i l,  the row count
// (E_s, V_s) = predict_mean_and_var of component s.  The component formulas are lik_density / lik_moments of likelihood.hpp (the
// element-wise likelihoods) and multiclass_launch (MultiClass).
// Memory-bound: 2 S n DY doubles read once; nothing but the partial sums is written unless the per-row values are asked for.
// Every reduction runs in a fixed order: the same inputs and batch size give the same bits.
#include "likelihood.hpp"
#include "mixture_common.hpp"

#define EV_NSEG 8         // segments of the in-workgroup sums
#define EV_DFAST 32       // outputs up to which the in-workgroup sums run in two levels

struct EvalArgs {
  const double* mean;     // (S n) x DY, row s n + i      (MultiClass: unused)
  const double* var;
  const double* Y;        // n x DY                       (MultiClass: n x 1 labels)
  const double* T;        // MultiClass: (1 + K) x (S n): log density of the label, then log probability of class k, per (s, i)
  const double* p0_dev;   // the likelihood's positive parameter on the device (a model's lik_const), or NULL: p0
  double* rows;           // n x DY x 3 or NULL
  double* part;           // 3 DY x nblocks partial sums: [q DY + d][block], q = 0 squared error / misclassification, 1 l, 2 rows
  int64_t n, total;       // total = flat (i, d) items: n DY (MultiClass: n)
  int S, DY, kind, nblocks;
  double p0, p1;
};

// running (maximum, sum of exp(. - maximum)): one exp per component, a component far below the maximum adds exactly 0
__device__ __forceinline__ void lse_add(double& mx, double& sm, double lp) {
  if (lp > mx) {
    sm = sm * exp(mx - lp) + 1.0;      // first component: 0 * exp(-inf) + 1
    mx = lp;
  } else {
    sm += (lp == mx) ? 1.0 : exp(lp - mx);      // (-inf beside -inf: no NaN; the result stays -inf)
  }
}
// two such pairs, `a` from the lower lane: every lane of a group evaluates the same expression
__device__ __forceinline__ void lse_merge(double am, double as, double bm, double bs, double& mx, double& sm) {
  const double M = am > bm ? am : bm;
  const double ea = (am == M) ? 1.0 : exp(am - M), eb = (bm == M) ? 1.0 : exp(bm - M);
  mx = M;
  sm = as * ea + bs * eb;
}

// LIK: the family of an element-wise likelihood (LIKF_QUAD: runtime kind), LIKF_NONE = MultiClass
template <int LIK>
__device__ __forceinline__ void eval_component(int kind, double mu, double v, double y, double p0, double p1, double& lp, double& E,
                                               double& V) {
  lik_moments<LIK>(kind, mu, v, p0, p1, E, V);
  lp = lik_density<LIK>(kind, mu, v, y, p0, p1);
}

// fold_sum's butterfly for the (maximum, sum) pairs
template <int SPLIT>
__device__ __forceinline__ void fold_lse(double& mx, double& sm, int sub) {
#pragma unroll
  for (int off = 1; off < SPLIT; off <<= 1) {
    const double om = __shfl_xor(mx, off), os = __shfl_xor(sm, off);
    if (sub & off) lse_merge(om, os, mx, sm, mx, sm);
    else lse_merge(mx, sm, om, os, mx, sm);
  }
}

template <int LIK, int SPLIT>
__global__ __launch_bounds__(MIX_T) void k_eval_mix(const EvalArgs a) {
  constexpr int JPB = MixItem<SPLIT>::JPB;
  __shared__ double ent[3 * JPB];
  __shared__ double seg[3 * EV_DFAST * EV_NSEG];
  const MixItem<SPLIT> it(a.total);
  const int tid = threadIdx.x, sub = it.sub, jl = it.jl;
  const int64_t j0 = it.j0, jc = it.jc;
  const bool live = it.live;
  const int S = a.S;
  const double invS = 1.0 / (double)S, logS = log((double)S);
  double err, ell;
  if (LIK == LIKF_NONE) {
    // MultiClass: item = row i.  l from the label's log densities, then class by class the mixture probability and its argmax
    const int K = a.DY;
    const int64_t R = (int64_t)S * a.n;
    double mx = -1.0 / 0.0, sm = 0.0;
    for (int s = sub; s < S; s += SPLIT) lse_add(mx, sm, a.T[(int64_t)s * a.n + jc]);
    fold_lse<SPLIT>(mx, sm, sub);
    ell = mx + log(sm) - logS;
    int best = 0;
    double pbest = -1.0;
    for (int k = 0; k < K; ++k) {
      const double* Tk = a.T + (int64_t)(1 + k) * R + jc;
      double sp = 0.0, sv = 0.0, sq = 0.0;
      int s = sub;
      for (; s + 3 * SPLIT < S; s += 4 * SPLIT) {
        const double t0 = Tk[(int64_t)s * a.n], t1 = Tk[(int64_t)(s + SPLIT) * a.n], t2 = Tk[(int64_t)(s + 2 * SPLIT) * a.n],
                     t3 = Tk[(int64_t)(s + 3 * SPLIT) * a.n];
        const double p[4] = {exp(t0), exp(t1), exp(t2), exp(t3)};
#pragma unroll
        for (int u = 0; u < 4; ++u) { sp += p[u]; sv += p[u] - p[u] * p[u]; sq += p[u] * p[u]; }
      }
      for (; s < S; s += SPLIT) {
        const double p = exp(Tk[(int64_t)s * a.n]);
        sp += p; sv += p - p * p; sq += p * p;
      }
      sp = fold_sum<SPLIT>(sp, sub); sv = fold_sum<SPLIT>(sv, sub); sq = fold_sum<SPLIT>(sq, sub);
      const double mh = sp * invS;
      if (mh > pbest) { pbest = mh; best = k; }      // ties: the lowest index (numpy.argmax)
      if (a.rows && live && sub == 0) {
        double* r = a.rows + (jc * K + k) * 3;
        r[0] = mh;
        r[1] = (S == 1) ? sv : (sv + sq) * invS - mh * mh;
        r[2] = ell;
      }
    }
    err = (best != (int)a.Y[jc]) ? 1.0 : 0.0;
  } else {
    const double p0 = a.p0_dev ? a.p0_dev[0] : a.p0, p1 = a.p1;
    const double y = a.Y[jc];
    const double* mp = a.mean + jc;
    const double* vp = a.var + jc;
    const int64_t ts = a.total;      // stride between components
    double mx = -1.0 / 0.0, sm = 0.0, sE = 0.0, sV = 0.0, sQ = 0.0;
    int s = sub;
    for (; s + 3 * SPLIT < S; s += 4 * SPLIT) {      // four components' loads in flight
      double mu[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { mu[u] = mp[(int64_t)(s + u * SPLIT) * ts]; v[u] = vp[(int64_t)(s + u * SPLIT) * ts]; }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double lp, E, V;
        eval_component<LIK>(a.kind, mu[u], v[u], y, p0, p1, lp, E, V);
        lse_add(mx, sm, lp);
        sE += E; sV += V; sQ += E * E;
      }
    }
    for (; s < S; s += SPLIT) {
      double lp, E, V;
      eval_component<LIK>(a.kind, mp[(int64_t)s * ts], vp[(int64_t)s * ts], y, p0, p1, lp, E, V);
      lse_add(mx, sm, lp);
      sE += E; sV += V; sQ += E * E;
    }
    fold_lse<SPLIT>(mx, sm, sub);
    sE = fold_sum<SPLIT>(sE, sub); sV = fold_sum<SPLIT>(sV, sub); sQ = fold_sum<SPLIT>(sQ, sub);
    const double mh = sE * invS;
    ell = mx + log(sm) - logS;
    err = (y - mh) * (y - mh);
    if (a.rows && live && sub == 0) {
      double* r = a.rows + jc * 3;
      r[0] = mh;
      r[1] = (S == 1) ? sV : (sV + sQ) * invS - mh * mh;      // one component: its variance itself, not V + E^2 - E^2
      r[2] = ell;
    }
  }
  // ---- the workgroup's sums per output, items in ascending order
  if (sub == 0) {
    ent[jl] = live ? err : 0.0;
    ent[JPB + jl] = live ? ell : 0.0;
    ent[2 * JPB + jl] = live ? 1.0 : 0.0;
  }
  __syncthreads();
  const int ND = (LIK == LIKF_NONE) ? 1 : a.DY;      // outputs with sums of their own (MultiClass: one)
  if (ND <= EV_DFAST) {
    constexpr int SL = JPB / EV_NSEG;
    for (int p = tid; p < 3 * ND * EV_NSEG; p += MIX_T) {
      const int g = p % EV_NSEG, qd = p / EV_NSEG, d = qd % ND, q = qd / ND;
      seg[p] = sum_output_items(d, ND, j0, g * SL, (g + 1) * SL, [&](int e) { return ent[q * JPB + e]; });
    }
    __syncthreads();
    for (int p = tid; p < 3 * ND; p += MIX_T) {
      double t = 0.0;
#pragma unroll
      for (int g = 0; g < EV_NSEG; ++g) t += seg[p * EV_NSEG + g];
      a.part[(int64_t)((p / ND) * a.DY + p % ND) * a.nblocks + blockIdx.x] = t;
    }
  } else {
    for (int p = tid; p < 3 * ND; p += MIX_T) {
      const int d = p % ND, q = p / ND;
      a.part[(int64_t)(q * a.DY + d) * a.nblocks + blockIdx.x] = sum_output_items(d, ND, j0, 0, JPB, [&](int e) { return ent[q * JPB + e]; });
    }
  }
}

template <int LIK>
static void eval_launch(int split, int nblocks, hipStream_t st, const EvalArgs& a) {
  mix_dispatch_split(split, [&](auto sp) { DS_LAUNCH((k_eval_mix<LIK, decltype(sp)::value>), dim3(nblocks), dim3(MIX_T), 0, st, a); });
}

int eval_mixture_launch(dsdgp_ctx* ctx, int kind, double p0, double p1, const double* p0_dev, const double* mean, const double* var,
                        const double* Y, int64_t n, int S, int DY, double* rows_out, double* acc, int accumulate) {
  DS_CHECK_ARG(ctx && mean && var && Y && acc && n > 0 && S > 0 && DY > 0);
  const bool mc = kind == DSDGP_LIK_MULTICLASS;
  if (!mc && lik_family(kind) == LIKF_NONE) {
    dsdgp_set_error("dsdgp_eval_mixture: likelihood kind %d is not covered", kind);
    return DSDGP_ERR_UNSUPPORTED;
  }
  if (!mc) DS_CHECK_ARG(lik_params_ok(kind, p0_dev ? 1.0 : p0, p1));
  const int64_t total = mc ? n : n * DY;
  const int split = mix_split_clamp(mix_split_by_items(total), S);
  int nblocks;
  DS_TRY(mix_nblocks(total, split, &nblocks));
  const int64_t R = (int64_t)S * n;
  const size_t part_doubles = (size_t)round_up((int64_t)3 * DY * nblocks, 32);
  void* scr;
  DS_TRY(ctx_scratch(ctx, (part_doubles + (mc ? (size_t)(1 + DY) * R : 0)) * sizeof(double), &scr));
  ProfScope prof(ctx, "evaluate");
  EvalArgs a{};
  a.mean = mean; a.var = var; a.Y = Y; a.p0_dev = p0_dev; a.rows = rows_out; a.part = (double*)scr;
  a.n = n; a.total = total; a.S = S; a.DY = DY; a.kind = kind; a.nblocks = nblocks; a.p0 = p0; a.p1 = p1;
  if (mc) {
    // log densities by the arithmetic of dsdgp_multiclass_var_exp mode 1, class probabilities as dsdgp_multiclass_predict forms them
    double* T = (double*)scr + part_doubles;
    DS_TRY(multiclass_launch(ctx, mean, var, Y, n, R, DY, 1, 0.0, T, nullptr, nullptr, -1));
    for (int k = 0; k < DY; ++k) DS_TRY(multiclass_launch(ctx, mean, var, nullptr, R, R, DY, 1, 0.0, T + (int64_t)(1 + k) * R, nullptr, nullptr, k));
    a.T = T;
    eval_launch<LIKF_NONE>(split, nblocks, ctx->stream, a);
  } else {
    lik_dispatch(kind, [&](auto fam) { eval_launch<decltype(fam)::value>(split, nblocks, ctx->stream, a); });
  }
  // (MultiClass: one output has sums of its own)
  mixture_finish_launch(ctx->stream, (const double*)scr, nblocks, 3 * DY, DY, mc ? 1 : DY, accumulate, acc);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_eval_mixture(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var,
                                  const double* Y, int64_t n, int32_t S, int32_t DY, double* rows_out, double* acc, int accumulate) {
  return eval_mixture_launch(ctx, kind, p0, p1, nullptr, mean, var, Y, n, S, DY, rows_out, acc, accumulate);
}

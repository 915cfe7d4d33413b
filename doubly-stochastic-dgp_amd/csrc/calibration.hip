// Calibration of the predictive mixture on the device: quantiles (credible intervals), the probability integral transform of held-out
// targets, interval coverage counts and the continuous ranked probability score — what the reference's users compute on the host from
// predict_y / predict_f outputs (demos/using_natural_gradients.ipynb cell 9: np.percentile of 100 samples; demo_step_function.ipynb:83-85
// and priors.ipynb:1020: mean +- 1.96 sqrt(var); dgp.py:116-126 for the mixture itself).
//   component s of item (i, d):  N(mu_s, sig_s^2),  sig_s^2 = max(var_s + noise, DBL_MIN)
//   F(x) = (1/S) sum_s Phi((x - mu_s) / sig_s),  Phi(z) = erfc(-z / sqrt 2) / 2 ;  f = F'
//   quantile q_k:  F(q_k) = p_k  — safeguarded Newton inside a bracket that holds the root, at most CAL_MAXIT steps
//   PIT  u = F(y)
//   CRPS = (1/S) sum_s A(y - mu_s, sig_s^2) - (1/(2 S^2)) sum_s sum_t A(mu_s - mu_t, sig_s^2 + sig_t^2)      (Grimit et al. 2006)
//          A(m, s^2) = m (2 Phi(m/s) - 1) + 2 s phi(m/s) = m erf(m / (s sqrt 2)) + s sqrt(2/pi) exp(-m^2 / (2 s^2))
//   per output:  sum_i CRPS, the row count, and for every k the number of rows with u <= p_k
// No MFMA work: fp64 VALU and transcendentals.  Per item: S (erfc + exp) per Newton step and probability, S (erfc) + S (erf + exp) for u
// and the first CRPS sum, S (S - 1) / 2 (sqrt + divide + erf + exp) for the pair sum.  Every reduction runs in a fixed order: the same
// inputs and n give the same bits.
#include <float.h>
#include <math.h>

#include "mixture_common.hpp"

#define CAL_CAP 8         // components per lane staged in LDS as (mu, sig); later ones are read from global memory every time
#define CAL_MAXP 16       // probabilities per call
#define CAL_MAXIT 128     // root-finder steps per probability: bisection alone takes a bracket of 2^20 sig down to one ulp in ~75

struct CalArgs {
  const double* mean;       // (S n) x DY, row s n + i
  const double* var;
  const double* Y;          // n x DY (calibration only)
  const double* noise_dev;  // the noise variance on the device (a model's lik_const), or NULL: noise
  double* q_out;            // n x DY x P (quantiles only)
  double* rows;             // n x DY x 2 or NULL
  double* part;             // (2 + P) DY x nblocks partial sums: [q DY + d][block], q = 0 CRPS, 1 rows, 2 + k #(u <= p_k)
  int64_t total;            // flat (i, d) items: n DY
  int S, DY, P, nblocks;
  double noise;
  double probs[CAL_MAXP];
  double zlo[CAL_MAXP], zhi[CAL_MAXP];      // Phi(zlo_k) <= p_k <= Phi(zhi_k), with a margin for the rounding of either side
};

#define CAL_RSQRT2 0.70710678118654752440
#define CAL_RSQRT2PI 0.39894228040143267794      // 1 / sqrt(2 pi)
#define CAL_SQRT2_PI 0.79788456080286535588      // sqrt(2 / pi)
#define CAL_RSQRTPI 0.56418958354775628695       // 1 / sqrt(pi)

__device__ __forceinline__ double cal_A(double m, double s) {      // A(m, s^2), s > 0
  const double z = m / s;
  return m * erf(z * CAL_RSQRT2) + s * CAL_SQRT2_PI * exp(-0.5 * z * z);
}

// fold_sum's butterfly for the extrema
template <int SPLIT>
__device__ __forceinline__ double cal_fold_min(double x) {
#pragma unroll
  for (int off = 1; off < SPLIT; off <<= 1) x = fmin(x, __shfl_xor(x, off));
  return x;
}
template <int SPLIT>
__device__ __forceinline__ double cal_fold_max(double x) {
#pragma unroll
  for (int off = 1; off < SPLIT; off <<= 1) x = fmax(x, __shfl_xor(x, off));
  return x;
}

// MODE 0: quantiles.  MODE 1: PIT, CRPS and their sums.
// Lane `sub` of an item owns the components s = sub + c SPLIT, c = 0, 1, ...  The first CAL_CAP of them live in the lane's own LDS
// column as (mu, sig).
template <int MODE, int SPLIT>
__global__ __launch_bounds__(MIX_T) void k_calibration(const CalArgs a) {
  constexpr int JPB = MixItem<SPLIT>::JPB;
  __shared__ double lmu[CAL_CAP * MIX_T];
  __shared__ double lsg[CAL_CAP * MIX_T];
  __shared__ double ent[MODE == 1 ? 3 * JPB : 1];
  const MixItem<SPLIT> it(a.total);
  const int tid = threadIdx.x, sub = it.sub, jl = it.jl;
  const int64_t j0 = it.j0, jc = it.jc;
  const bool live = it.live;
  const int S = a.S;
  const int64_t ts = a.total;                     // stride between components
  const double noise = a.noise_dev ? a.noise_dev[0] : a.noise;
  const double* mp = a.mean + jc;
  const double* vp = a.var + jc;
  const int cnt = (S - sub + SPLIT - 1) / SPLIT;      // components of this lane
  const int nst = cnt < CAL_CAP ? cnt : CAL_CAP;      // ... of which staged

  for (int c = 0; c < nst; ++c) {
    const int64_t s = sub + (int64_t)c * SPLIT;
    lmu[c * MIX_T + tid] = mp[s * ts];
    lsg[c * MIX_T + tid] = sqrt(fmax(vp[s * ts] + noise, DBL_MIN));
  }
  __syncthreads();      // (the pair sum reads the other lanes' columns)

  // component c of this lane
  auto own = [&](int c, double& mu, double& sg) {
    if (c < CAL_CAP) {
      mu = lmu[c * MIX_T + tid];
      sg = lsg[c * MIX_T + tid];
    } else {
      const int64_t s = sub + (int64_t)c * SPLIT;
      mu = mp[s * ts];
      sg = sqrt(fmax(vp[s * ts] + noise, DBL_MIN));
    }
  };

  if (MODE == 0) {
    for (int k = 0; k < a.P; ++k) {
      const double p = a.probs[k], zl = a.zlo[k], zh = a.zhi[k];
      // bracket: at lo every (x - mu_s) / sig_s <= zlo, so F(lo) <= Phi(zlo) <= p; likewise F(hi) >= p
      double lo = 1.0 / 0.0, hi = -1.0 / 0.0;
      for (int c = 0; c < cnt; ++c) {
        double mu, sg;
        own(c, mu, sg);
        lo = fmin(lo, mu + zl * sg);
        hi = fmax(hi, mu + zh * sg);
      }
      lo = cal_fold_min<SPLIT>(lo);
      hi = cal_fold_max<SPLIT>(hi);
      double x = lo + 0.5 * (hi - lo), dxold = hi - lo, res = x;
      double glo = -1.0 / 0.0, ghi = 1.0 / 0.0;      // F - p at the ends, once known
      bool done = !(lo < hi);
      // Bounded: CAL_MAXIT steps at most.  All lanes of an item hold the same bits of (x, lo, hi) and take every branch together; the
      // wave goes on until each of its items is done, finished lanes only repeating the evaluation.
      for (int it = 0; it < CAL_MAXIT; ++it) {
        if (!__any(!done)) break;
        double F = 0.0, f = 0.0;
        for (int c = 0; c < cnt; ++c) {
          double mu, sg;
          own(c, mu, sg);
          const double z = (x - mu) / sg;
          F += 0.5 * erfc(-z * CAL_RSQRT2);
          f += CAL_RSQRT2PI * exp(-0.5 * z * z) / sg;
        }
        F = fold_sum<SPLIT>(F, sub) / (double)S;
        f = fold_sum<SPLIT>(f, sub) / (double)S;
        if (!done) {
          const double g = F - p;
          if (g == 0.0) {
            done = true;
            res = x;
          } else {
            if (g < 0.0) { lo = x; glo = g; } else { hi = x; ghi = g; }
            const double mid = lo + 0.5 * (hi - lo);
            const double dx = g / f;
            double xn = x - dx;
            // bisect when the Newton step leaves the bracket (or is not a number), or does not halve the previous step
            const bool bis = !(xn > lo && xn < hi) || fabs(2.0 * g) > fabs(dxold * f);
            if (bis) {
              xn = mid;
              dxold = 0.5 * (hi - lo);
            } else {
              dxold = fabs(dx);
            }
            if (bis && !(mid > lo && mid < hi)) {      // the bracket cannot shrink: the end with the smaller residual
              done = true;
              res = (-glo <= ghi) ? lo : hi;
            } else if (xn == x) {                      // a Newton step below the spacing of x
              done = true;
              res = x;
            } else {
              x = xn;
              res = mid;                               // (what is returned if the cap ends the iteration)
            }
          }
        }
      }
      if (live && sub == 0) a.q_out[jc * a.P + k] = res;
    }
    return;
  }

  // ---- MODE 1
  const double y = a.Y[jc];
  const double invS = 1.0 / (double)S;
  double u = 0.0, t1 = 0.0, diag = 0.0;
  for (int c = 0; c < cnt; ++c) {
    double mu, sg;
    own(c, mu, sg);
    const double m = y - mu, z = m / sg;
    u += 0.5 * erfc(-z * CAL_RSQRT2);
    t1 += cal_A(m, sg);
    diag += sg;
  }
  // pair sum over s < t: for every s the lanes of the item share t = s + 1, s + 2, ...
  double pr = 0.0;
  const int gbase = tid - sub;      // first lane of the item
  for (int s = 0; s + 1 < S; ++s) {
    double ms, ss;
    {
      const int c = s / SPLIT, o = s % SPLIT;
      if (c < CAL_CAP) {
        ms = lmu[c * MIX_T + gbase + o];
        ss = lsg[c * MIX_T + gbase + o];
      } else {
        ms = mp[(int64_t)s * ts];
        ss = sqrt(fmax(vp[(int64_t)s * ts] + noise, DBL_MIN));
      }
    }
    for (int t = s + 1 + sub; t < S; t += SPLIT) {
      double mt, st;
      const int c = t / SPLIT, o = t % SPLIT;
      if (c < CAL_CAP) {
        mt = lmu[c * MIX_T + gbase + o];
        st = lsg[c * MIX_T + gbase + o];
      } else {
        mt = mp[(int64_t)t * ts];
        st = sqrt(fmax(vp[(int64_t)t * ts] + noise, DBL_MIN));
      }
      pr += cal_A(ms - mt, sqrt(ss * ss + st * st));
    }
  }
  u = fold_sum<SPLIT>(u, sub) * invS;
  t1 = fold_sum<SPLIT>(t1, sub);
  diag = fold_sum<SPLIT>(diag, sub);
  pr = fold_sum<SPLIT>(pr, sub);
  // diagonal terms A(0, 2 sig^2) = 2 sig / sqrt(pi); off-diagonal pairs counted twice
  const double crps = t1 * invS - 0.5 * invS * invS * (2.0 * pr + 2.0 * CAL_RSQRTPI * diag);
  if (a.rows && live && sub == 0) {
    a.rows[jc * 2] = u;
    a.rows[jc * 2 + 1] = crps;
  }
  // ---- the workgroup's sums per output, items in ascending order
  if (sub == 0) {
    ent[jl] = live ? crps : 0.0;
    ent[JPB + jl] = live ? 1.0 : 0.0;
    ent[2 * JPB + jl] = u;
  }
  __syncthreads();
  const int ND = a.DY, Q = 2 + a.P;
  for (int p = tid; p < Q * ND; p += MIX_T) {
    const int d = p % ND, q = p / ND;
    const double pk = q >= 2 ? a.probs[q - 2] : 0.0;
    a.part[(int64_t)(q * ND + d) * a.nblocks + blockIdx.x] = sum_output_items(d, ND, j0, 0, JPB, [&](int e) {
      return q == 0 ? ent[e] : q == 1 ? ent[JPB + e] : (ent[JPB + e] != 0.0 && ent[2 * JPB + e] <= pk) ? 1.0 : 0.0;
    });
  }
}

template <int MODE>
static void cal_launch(int split, int nblocks, hipStream_t st, const CalArgs& a) {
  mix_dispatch_split(split, [&](auto sp) { DS_LAUNCH((k_calibration<MODE, decltype(sp)::value>), dim3(nblocks), dim3(MIX_T), 0, st, a); });
}

// Lanes per item: by the item count, raised until the lanes' LDS columns hold every component (S <= CAL_CAP x lanes) where 16 lanes
// can, and never more lanes than components.
static int cal_split(int64_t total, int S) {
  int split = mix_split_by_items(total);
  while (split < 16 && S > CAL_CAP * split) split = (split == 1) ? 4 : split * 2;
  return mix_split_clamp(split, S);
}

static double cal_Phi(double z) { return 0.5 * erfc(-z * CAL_RSQRT2); }

// z with Phi(z) = p by bisection on the host (64 halvings of [-40, 0]; p > 1/2 through 1 - p, which is exact there)
static double cal_probit(double p) {
  const bool upper = p > 0.5;
  const double q = upper ? 1.0 - p : p;
  double lo = -40.0, hi = 0.0;
  for (int it = 0; it < 64; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (cal_Phi(mid) < q) lo = mid; else hi = mid;
  }
  const double z = 0.5 * (lo + hi);
  return upper ? -z : z;
}

// the arguments both entries share, checked and filled in; P probabilities from the host array
static int cal_fill(const char* who, dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* noise_dev,
                    int64_t n, int S, int DY, const double* probs, int P, CalArgs& a) {
  DS_CHECK_ARG(ctx && mean && var && probs && n > 0 && S > 0 && DY > 0);
  DS_CHECK_ARG(n <= INT64_MAX / DY / (CAL_MAXP + 2));
  if (P < 1 || P > CAL_MAXP) {
    dsdgp_set_error("%s: bad argument: P = %d probabilities, 1 .. %d are taken", who, P, CAL_MAXP);
    return DSDGP_ERR_BAD_ARG;
  }
  if (!noise_dev && !(noise_var >= 0.0 && noise_var <= DBL_MAX)) {
    dsdgp_set_error("%s: bad argument: the noise variance %g must be finite and not negative", who, noise_var);
    return DSDGP_ERR_BAD_ARG;
  }
  a.mean = mean; a.var = var; a.noise_dev = noise_dev; a.noise = noise_dev ? 0.0 : noise_var;
  a.total = n * DY; a.S = S; a.DY = DY; a.P = P;
  for (int k = 0; k < P; ++k) {
    const double p = probs[k];
    if (!(p > 0.0 && p < 1.0)) {
      dsdgp_set_error("%s: bad argument: probs[%d] = %g is not inside (0, 1)", who, k, p);
      return DSDGP_ERR_BAD_ARG;
    }
    const double z = cal_probit(p), w = 1e-9 * (1.0 + fabs(z));
    a.probs[k] = p;
    a.zlo[k] = z - w;
    a.zhi[k] = z + w;
  }
  return DSDGP_OK;
}

int mixture_quantiles_launch(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* noise_dev,
                             int64_t n, int S, int DY, const double* probs, int P, double* q_out) {
  CalArgs a{};
  DS_TRY(cal_fill("dsdgp_mixture_quantiles", ctx, mean, var, noise_var, noise_dev, n, S, DY, probs, P, a));
  DS_CHECK_ARG(q_out != nullptr);
  const int split = cal_split(a.total, S);
  DS_TRY(mix_nblocks(a.total, split, &a.nblocks));
  a.q_out = q_out;
  ProfScope prof(ctx, "calibration");
  cal_launch<0>(split, a.nblocks, ctx->stream, a);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

int mixture_calibration_launch(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* noise_dev,
                               const double* Y, int64_t n, int S, int DY, const double* probs, int P, double* rows_out, double* acc,
                               int accumulate) {
  CalArgs a{};
  DS_TRY(cal_fill("dsdgp_mixture_calibration", ctx, mean, var, noise_var, noise_dev, n, S, DY, probs, P, a));
  DS_CHECK_ARG(Y && acc);
  const int split = cal_split(a.total, S);
  int nblocks;
  DS_TRY(mix_nblocks(a.total, split, &nblocks));
  const int entries = (2 + P) * DY;
  void* scr;
  DS_TRY(ctx_scratch(ctx, (size_t)round_up((int64_t)entries * nblocks, 32) * sizeof(double), &scr));
  a.Y = Y; a.rows = rows_out; a.part = (double*)scr; a.nblocks = nblocks;
  ProfScope prof(ctx, "calibration");
  cal_launch<1>(split, nblocks, ctx->stream, a);
  mixture_finish_launch(ctx->stream, (const double*)scr, nblocks, entries, DY, DY, accumulate, acc);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

extern "C" int dsdgp_mixture_quantiles(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, int64_t n, int32_t S,
                                       int32_t DY, const double* probs, int32_t P, double* q_out) {
  return mixture_quantiles_launch(ctx, mean, var, noise_var, nullptr, n, S, DY, probs, P, q_out);
}

extern "C" int dsdgp_mixture_calibration(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* Y,
                                         int64_t n, int32_t S, int32_t DY, const double* probs, int32_t P, double* rows_out,
                                         double* acc, int accumulate) {
  return mixture_calibration_launch(ctx, mean, var, noise_var, nullptr, Y, n, S, DY, probs, P, rows_out, acc, accumulate);
}

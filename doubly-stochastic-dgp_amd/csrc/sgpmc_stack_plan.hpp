// Host plan of a stack of sparse sampled layers (sgpmc_stack.hip): the carve-up of the caller's scratch block and the geometry of every
// launch and reduction, from (L, n, S, the layers' M, D, DO, p, the likelihood's width) alone — nothing else, so the summation order, and
// with it every bit of the results, depends neither on the device nor on which outputs the caller asks for.  No HIP:
// tests/host/sgpmc_stack_plan_check.cpp compiles it alone.
//
// Rows: r = s n + i, R = S n, the layout of dsdgp_model_propagate.  Layer l reads Xin[l] (R x D[l]; layer 0: X repeated S times) and
// leaves cm[l] (R x DO[l]) and var[l] (R); the hop writes [Xin[l][:, :p[l]] | sample] straight into Xin[l + 1], so D[l + 1] = p[l] + DO[l].
// The last layer is not sampled: p[L - 1] = 0 and DO[L - 1] = DY, the likelihood's width.
#pragma once
#include "sparse_cond_plan.hpp"

#define STK_MAX_L 16
#define STK_T 256            // threads per workgroup of every kernel of sgpmc_stack.hip

struct StackShape {
  int L;
  int64_t n;
  int S;
  int M[STK_MAX_L], D[STK_MAX_L], DO[STK_MAX_L], p[STK_MAX_L];
  int DY;
};

struct StackPlan {
  int L;
  int64_t n, R;
  int S, DY, maxM, maxD, maxDin, maxDO;
  bool ok;                                   // the shapes chain: D[l + 1] = p[l] + DO[l], p[L - 1] = 0, DO[L - 1] = DY, 0 <= p[l] <= D[l]
  // the factorisation check ahead of everything else: Z moved to its first row as origin, Ku -> Lu
  SCRegion Zc, Ku;
  // forward
  SCRegion Xin[STK_MAX_L], cm[STK_MAX_L], var[STK_MAX_L], z[STK_MAX_L];      // z[L - 1] is empty
  SCRegion lin;                              // Xin A of a Linear mean (R x maxDO), one layer at a time
  SCRegion fmean;                            // the last layer's mean with its mean function (R x DY)
  SCRegion sc;                               // the largest per-layer scratch of the sparse conditional, which the layers share
  size_t sc_bytes;
  // head: the variance column repeated DY times, the read-out's results, the priors
  SCRegion varb, part, ve, dmean, dvar, prior;
  int head_blocks;                           // ceil(R DY / 256): the read-out's block partials, added in ascending order
  size_t fwd_total;
  // reverse: the adjoints of a layer's mean and variance, of its input (two blocks, in turn: dX[l & 1] is layer l's)
  SCRegion gm, gv, dX[2];
  size_t total;
  // launches: one thread per entry / per row
  int64_t hop_blocks[STK_MAX_L], row_blocks;
};

static inline StackPlan sgpmc_stack_plan(const StackShape& s, bool reverse) {
  StackPlan P{};
  P.L = s.L, P.n = s.n, P.S = s.S, P.DY = s.DY, P.R = (int64_t)s.S * s.n;
  P.ok = s.L >= 1 && s.L <= STK_MAX_L && s.n >= 1 && s.S >= 1 && s.DY >= 1 && P.R < SC_MAX_ROWS;
  for (int l = 0; P.ok && l < s.L; ++l) {
    P.ok = s.M[l] >= 1 && s.M[l] <= SC_MAX_M && s.D[l] >= 1 && s.DO[l] >= 1 && s.p[l] >= 0 && s.p[l] <= s.D[l];
    if (P.ok && l + 1 < s.L) P.ok = s.D[l + 1] == s.p[l] + s.DO[l];
    if (P.ok && l + 1 == s.L) P.ok = s.p[l] == 0 && s.DO[l] == s.DY;
  }
  if (!P.ok) return P;
  const size_t R = (size_t)P.R;
  for (int l = 0; l < s.L; ++l) {
    P.maxM = std::max(P.maxM, s.M[l]), P.maxD = std::max(P.maxD, s.D[l]), P.maxDO = std::max(P.maxDO, s.DO[l]);
    if (l > 0) P.maxDin = std::max(P.maxDin, s.D[l]);
    const SCPlan c = sparse_cond_plan(P.R, s.M[l], s.D[l], s.DO[l]);
    P.sc_bytes = std::max(P.sc_bytes, reverse ? c.total : c.fwd_total);
    P.hop_blocks[l] = (int64_t)((R * (size_t)(s.p[l] + s.DO[l]) + STK_T - 1) / STK_T);
  }
  P.row_blocks = (int64_t)((R + STK_T - 1) / STK_T);
  P.head_blocks = (int)((R * (size_t)s.DY + 255) / 256);
  size_t t = 0;
  P.Zc = sc_take(t, (size_t)P.maxM * P.maxD * 8), P.Ku = sc_take(t, (size_t)P.maxM * P.maxM * 8);
  for (int l = 0; l < s.L; ++l) {
    P.Xin[l] = sc_take(t, R * s.D[l] * 8), P.cm[l] = sc_take(t, R * s.DO[l] * 8), P.var[l] = sc_take(t, R * 8);
    P.z[l] = sc_take(t, l + 1 < s.L ? R * s.DO[l] * 8 : 0);
  }
  P.lin = sc_take(t, R * P.maxDO * 8), P.fmean = sc_take(t, R * s.DY * 8), P.sc = sc_take(t, P.sc_bytes);
  P.varb = sc_take(t, R * s.DY * 8), P.part = sc_take(t, (size_t)2 * P.head_blocks * 8), P.ve = sc_take(t, R * 8);
  P.dmean = sc_take(t, R * s.DY * 8), P.dvar = sc_take(t, R * s.DY * 8), P.prior = sc_take(t, (size_t)s.L * 8);
  P.fwd_total = t;
  if (reverse) {
    P.gm = sc_take(t, R * P.maxDO * 8), P.gv = sc_take(t, R * 8);
    const size_t dx = R * (size_t)std::max(P.maxDin, 1) * 8;
    P.dX[0] = sc_take(t, dx), P.dX[1] = sc_take(t, dx);
  }
  P.total = t;
  return P;
}

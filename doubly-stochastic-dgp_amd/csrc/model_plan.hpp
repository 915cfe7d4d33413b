// Split-K plan of a layer's weight-gradient products and their reductions as pure host code (no HIP call, no dsdgp_model): layout() sizes
// with plan_caps(), ensure_plan() uploads what plan_layer() / plan_reductions() return, tests/host/plan_check.cpp walks a grid of shapes.
#pragma once
#include "plan_types.hpp"
#include <math.h>
#include <vector>

// G = E A^T is full; the D_out P_d are symmetric: off-diagonal tiles cost 1, diagonal tiles (NI+1)/(2 NI) and get that fraction
// of the K splits, so every task carries about the same number of MFMAs.  alg_g layers have no G job (k_asm_kbar
// assembles sum_r e a^T from the P_d).
static const double WG_DIAG_FRAC = (WG_NI + 1) / (2.0 * WG_NI);
static inline int wgrad_tiles_per_split(int alg_g, int D_out, int Mp) {
  const int ti = wgrad_ti(Mp);
  return (alg_g ? 0 : ti * ti) + D_out * (ti * (ti - 1) / 2) + (int)ceil(D_out * ti * WG_DIAG_FRAC);
}

// What layout() carves for a layer's plan (ld_max: most padded rows of a minibatch): split cap, WgradJob / ticket / RedJob slots, doubles
struct PlanCaps { int ns_max, jobs, ticks, reds; size_t part_big, part_thin, part_mean; };
static inline int plan_red_slots(int D_out) { return D_out + 5; }      // one per job + the chain's hyper-parameter partials
static inline PlanCaps plan_caps(int alg_g, int D_out, int Mp, int DP16, int DinP16, bool mean_grad, int64_t ld_max) {
  const int ti = wgrad_ti(Mp), tq = ceil_div(DP16 / 16, WG_NI), tz = ceil_div(DinP16 / 16, WG_NI);
  const size_t Mw = pad_Mw(Mp);
  PlanCaps c{};
  c.ns_max = choose_nsplit(wgrad_tiles_per_split(alg_g, D_out, Mp), ld_max / 16, 512);
  c.part_big = (size_t)c.ns_max * (1 + D_out) * Mw * Mw; c.part_thin = (size_t)c.ns_max * Mw * (DP16 + DinP16);
  c.part_mean = mean_grad ? (size_t)c.ns_max * 64 * ceil_div(DinP16, 64) * DP16 : 0;      // DinP16 rows on whole 64-row tiles
  c.jobs = D_out + 4;      // P_d | A mbar^T, mean function | E A^T, GW [X|1]^T
  c.ticks = (D_out + 1) * ti * ti + ti * (tq + tz) + tz * tq + 16;
  c.reds = plan_red_slots(D_out);
  return c;
}
// What the plan reads of a layer besides its LayerDev (LayerState derives from it); part_mean only with a trainable mean function
struct PlanBufs {
  double *A, *E, *GW, *VB, *MB, *XT1, *hyp_part, *part_big, *part_thin, *part_mean;
  int32_t* wtick;      // arrival counters of the in-launch split-K reduction, one per (job, tile) of this layer's products
  bool mean_grad;
  PlanCaps cap;
};
// ld: padded rows of this minibatch; hyp_parts: rows of hyp_part the backward chain writes for them; DSDGP_FORCE switches; two streams
struct PlanIn { const LayerDev* v; const PlanBufs* b; int64_t ld; int hyp_parts, wg_red, wg_group, overlap; };
struct PlanOut {
  std::vector<WgradJob> jobs;      // ONE list [A | B] with cumulative task numbers: one launch per layer
  std::vector<RedJob> red;
  int njobsA, totA, tot, ns, ticks;
};
// ---- the four shapes of reduction
static inline RedJob red_linear(const double* part, double* out, int64_t count, int64_t pstride, int ns) {      // `count` leading elements of every split
  RedJob r{}; r.part = part; r.out = out; r.count = count; r.nsplit = ns; r.pstride = pstride;
  return r;
}
static inline RedJob red_2d(const double* part, double* out, int Mp, int ns) {      // full Mp x Mp result on Mw-row partials
  RedJob r = red_linear(part, out, (int64_t)Mp * Mp, (int64_t)pad_Mw(Mp) * pad_Mw(Mp), ns);
  r.sym_tile = 16; r.in_ld = pad_Mw(Mp); r.out_ld = Mp;
  return r;
}
static inline RedJob red_sym_tiled(const double* part, double* out, int Mp, int ns) {      // ... symmetric: mirror at 16-block granularity
  RedJob r = red_2d(part, out, Mp, ns); r.sym_n = Mp;
  return r;
}
static inline RedJob red_wide(const double* part, double* out, int64_t count, int nparts) {      // few outputs, many partial rows
  RedJob r = red_linear(part, out, count, count, nparts); r.wide = 1;
  return r;
}
// ---- the three shapes of job (task_start, fin and tick are set where the job joins the list)
// unscaled P Q^T: the thin products (ti x tj tiles, leading dimension ldo = columns) and the full E A^T
static inline WgradJob job_product(const double* P, const double* Q, double* out, int ti, int tj, int ldo) {
  WgradJob J{}; J.P = P; J.Q = Q; J.out = out; J.ti = ti; J.tj = tj; J.ldo = ldo; J.qrows16 = ldo / 16;
  return J;
}
// P_d = sum_r vbar_d a a^T (symmetric), d = j - 1, partial slot j of part_big; ng > 0: the GROUPED job — ng of them from d on that
// share every load of A (32 x 32 tile tasks)
static inline WgradJob job_pd(const PlanIn& in, int j, int ng, int ns, int ns_diag) {
  const int64_t Mw = pad_Mw(in.v->Mp);
  WgradJob J = job_product(in.b->A, in.b->A, in.b->part_big + (int64_t)j * ns * Mw * Mw, (int)Mw / 64, (int)Mw / 64, (int)Mw);
  J.scale = in.b->VB + (int64_t)(j - 1) * in.ld; J.sym = 1; J.ns_diag = ns_diag; J.ng = ng;
  if (ng) { J.sstride = in.ld; J.ostride = (int64_t)ns * Mw * Mw; }
  return J;
}
// Jobs, task ranges, partial offsets, tickets and reductions of one layer for `in.ld` rows.
static inline void plan_layer(const PlanIn& in, PlanOut& out) {
  const LayerDev& v = *in.v; const PlanBufs& b = *in.b;
  const int NI = WG_NI, ti = wgrad_ti(v.Mp), Mp = v.Mp, Mw = pad_Mw(Mp), D_out = v.D_out, n_off = ti * (ti - 1) / 2;
  const int64_t MM = (int64_t)Mp * Mp;
  const int ns = std::min(choose_nsplit(wgrad_tiles_per_split(v.alg_g, D_out, Mp), in.ld / 16, 512), b.cap.ns_max);
  const int ns_diag = std::max(1, (int)ceil(ns * WG_DIAG_FRAC)), tjq = ceil_div(v.DP16 / 16, NI), tjz = ceil_div(v.DinP16 / 16, NI);
  double *const out_q = b.part_thin, *const out_z = b.part_thin + (int64_t)ns * Mw * v.DP16;
  // in-launch split-K reduction (WgradJob::fin): a job's tiles draw their tickets from wtick, the result goes where the reduction
  // launch used to put it and the job leaves k_reduce_grouped's list.  By default only where the plan has ONE split (large M: more
  // tiles than workgroup slots — the "reduction" was a copy-and-mirror pass over every P_d): the tile goes from registers to its
  // place(s) with no partial, no ticket.  With several splits every workgroup of the launch would wait for its partial's write
  // acknowledgement and draw a ticket before it can leave — measured at config 2 (23 splits of ~17 us tasks, wg_red = 2): the three
  // product launches 0.114 -> 0.294 ms per step, the step 0.510 -> 0.618 ms; config 3 +2 %.  (wg_red = 0: never; 2: always — parity tests.)
  const bool wfuse = in.wg_red >= 2 || (in.wg_red == 1 && ns == 1);
  // The D_out P_d share their operand A: grouped jobs (WgradJob::ng: up to four P_d per 32 x 32 tile task) load each A fragment once
  // for the whole group.  Same K splits (ns above fixes every element's order of summation: it must not depend on the grouping), same
  // partials.  Half the L2 requests but more L2 misses: at config 2 the launch is faster beside the next layer's backward chain and
  // slower alone; config 3 (Mw = 256) was slower.  So by default only on the two-stream schedule at Mw = 128 with
  // D_out >= 3 (groups of 3 or 4: a group of two moves as many bytes per MFMA as a 64 x 64 tile), and only for partials (wfuse jobs
  // keep the 64 x 64 tiles their in-launch reduction stages).  wg_group = 0: never; 2: every shape and schedule (parity tests).
  const bool wgroup = !wfuse && (in.wg_group >= 2 || (in.wg_group == 1 && D_out >= 3 && ti <= 2 && in.overlap));
  out.jobs.clear(); out.red.clear();
  int start = out.ticks = 0;
  // a job and what becomes of its result, together: reduced in the launch into R.out (wfuse) or by R in k_reduce_grouped
  auto add = [&](WgradJob J, int tasks, const RedJob& R, int fin_cols, int fin_rows) {
    J.task_start = start; start += tasks;
    if (wfuse) {
      J.fin = R.out; J.fin_ld = fin_cols; J.fin_rows = fin_rows; J.fin_cols = fin_cols;
      J.tick = b.wtick + out.ticks;
      out.ticks += J.sym ? J.ti * (J.ti + 1) / 2 : J.ti * J.tj;
    } else out.red.push_back(R);
    out.jobs.push_back(J);
  };
  // ---- A jobs: operands from the forward chain (A, [X^T;1]) and from the producer of this layer's upstream adjoints (VB, MB)
  const int ngroups = wgroup ? ceil_div(D_out, 4) : 0;
  for (int k = 0, j = 1; k < ngroups; ++k) {
    const int ng = D_out / ngroups + (k < D_out % ngroups ? 1 : 0);
    WgradJob J = job_pd(in, j, ng, ns, ns_diag);
    J.task_start = start; start += 4 * ns * n_off + 3 * ns_diag * ti;      // per split: 4 32-tiles of an off-diagonal 64-tile, 3 of a diagonal one
    out.jobs.push_back(J);
    for (int o = 0; o < ng; ++o, ++j) out.red.push_back(red_sym_tiled(J.out + o * J.ostride, v.bigred + (int64_t)j * MM, Mp, ns));
  }
  for (int j = 1; j <= (wgroup ? 0 : D_out); ++j) {
    const WgradJob J = job_pd(in, j, 0, ns, ns_diag);
    add(J, ns * n_off + ns_diag * ti, red_sym_tiled(J.out, v.bigred + (int64_t)j * MM, Mp, ns), Mp, Mp);
  }
  // thin product P Q^T on ti_ x tj_ tiles (whole 16*NI-row tiles, `cols` columns) -> the rows x cols result `res`
  auto add_thin = [&](const double* P, const double* Q, double* part, double* res, int ti_, int tj_, int cols, int rows) {
    add(job_product(P, Q, part, ti_, tj_, cols), ns * ti_ * tj_, red_linear(part, res, (int64_t)rows * cols, (int64_t)16 * NI * ti_ * cols, ns), cols, rows);
  };
  add_thin(b.A, b.MB, out_q, v.thinq, ti, tjq, v.DP16, Mp);      // A mbar^T -> q_mu
  // trainable Linear mean function: d loss / d [A ; b] = [X ; 1]^T MB^T  (XT1 is zero-padded to whole 16*NI-row tiles)
  if (b.mean_grad) add_thin(b.XT1, b.MB, b.part_mean, v.meanAB, tjz, tjq, v.DP16, 16 * NI * tjz);
  out.njobsA = (int)out.jobs.size(); out.totA = start;
  // ---- B jobs: operands from this layer's backward chain (E, GW)
  if (!v.alg_g) {
    WgradJob J = job_product(b.E, b.A, b.part_big, ti, ti, Mw); J.ns_diag = ns_diag;      // (read for sym jobs only; uploaded as it always was)
    add(J, ns * ti * ti, red_2d(J.out, v.bigred, Mp, ns), Mp, Mp);
  }
  add_thin(b.GW, b.XT1, out_z, v.thinz, ti, tjz, v.DinP16, Mp);      // GW [X|1]^T -> Z
  out.red.push_back(red_wide(b.hyp_part, v.hyp_red, (int64_t)v.D_in + 2, in.hyp_parts));
  out.ns = ns; out.tot = start;
}
// Form (ways) and block range of every reduction in list order -> block total; any64: some job needs k_reduce_grouped's 64 x 65 LDS tile
struct RedPlan { int blocks; bool any64; };
static inline RedPlan plan_reductions(std::vector<RedJob>& red) {
  RedPlan p{};
  for (auto& r : red) {
    r.ways = (!r.wide && r.nsplit >= 12) ? 4 : 0;
    const bool even = r.count % 2 == 0 && r.pstride % 2 == 0 && r.in_ld % 2 == 0 && r.out_ld % 2 == 0 && r.sym_tile % 2 == 0 &&
                      ((uintptr_t)r.part & 15) == 0;
    if (r.ways == 4 && even) r.ways = 8;
    const int64_t rows = r.out_ld > 0 ? r.count / r.out_ld : 0;
    const bool tiled = !r.wide && r.sym_n > 0 && r.sym_tile == 16 && r.out_ld > 0 && rows == r.out_ld && rows % 16 == 0 && even;
    if (tiled) r.ways = 16;
    // one or two splits of a symmetric result on whole 64-tiles: the copy-and-mirror form (one 64 x 64 tile per workgroup)
    const bool tiled64 = tiled && r.nsplit <= 2 && rows % 64 == 0 && r.sym_n % 64 == 0 && ((uintptr_t)r.out & 15) == 0;
    if (tiled64) { r.ways = 64; p.any64 = true; }
    r.blk_start = p.blocks;
    const int64_t t = rows / (tiled64 ? 64 : 16);      // tiles per side of a tiled form
    p.blocks += r.wide ? (int)r.count : (tiled ? (int)(t * (t + 1) / 2) : ceil_div(r.count, r.ways == 8 ? 128 : (r.ways == 4 ? 64 : 256)));
  }
  return p;
}

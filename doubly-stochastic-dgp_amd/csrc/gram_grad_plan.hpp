// Host plan of the reverse pass of the Gram matrix (gram_grad.hip): the row blocks and column splits of its passes and the carve-up of the
// call's scratch, from (n, n2, D, form) alone — nothing else, so the summation order, and with it every bit of the results, depends
// neither on the device nor on which outputs the caller asks for.  No HIP: tests/host/gram_grad_plan_check.cpp compiles it alone.
//
// A pass gives every row of its row side one thread (GG_T rows per workgroup) and cuts its column side into `nsplit` ranges of
// `cols_per_split` columns (whole tiles of GG_CT, the last range ragged); workgroup (b, s) walks the tiles of range s for the rows of
// block b and leaves one partial row per (s, row).  Pass a: rows = X, columns = X2 (or X in the symmetric form): d_X and the kernel's
// hyper-parameters.  Pass b (cross form only): the roles swapped, d_X2.
#pragma once
#include "plan_types.hpp"

#define GG_T 128            // rows per workgroup, one per thread
#define GG_CT 16            // columns per staged tile
#define GG_MAX_D 32         // widest input: a thread holds its row and two accumulators per dimension in registers
#define GG_TARGET_WG 512    // workgroups a pass aims for (two per CU)
#define GG_MIN_COLS 64      // fewest columns worth a split
#define GG_MAX_ROWS ((int64_t)1 << 31)
#define GG_SCRATCH_CAP ((size_t)8 << 30)

struct GGRegion { size_t off, bytes; };      // of the call's scratch; off is a multiple of 256, bytes == 0: not used by this form

struct GGPass {
  int64_t rows, cols, cols_per_split;
  int row_blocks, nsplit;
  GGRegion PX;                               // nsplit x rows x D: the partial sums over the columns of a split of t u_d (see gram_grad.hip)
};

struct GGPlan {
  bool symmetric;
  GGPass a, b;                               // b.rows == 0 in the symmetric form
  GGRegion PL, PV;                           // pass a: nsplit x rows x D partials of t u_d^2, nsplit x rows partials of w k / variance
  GGRegion Lrow, Vrow;                       // rows x D, rows: the same added over the splits
  size_t total;
};

static inline GGRegion gg_take(GGPlan& P, size_t bytes) {
  const GGRegion r{P.total, bytes};
  P.total += (size_t)round_up((int64_t)bytes, 256);
  return r;
}
// about GG_TARGET_WG workgroups, GG_MIN_COLS columns or more per split, whole tiles of GG_CT columns
static inline GGPass gg_pass(int64_t rows, int64_t cols) {
  GGPass p{};
  p.rows = rows, p.cols = cols, p.row_blocks = ceil_div(rows, GG_T);
  const int64_t want = std::min<int64_t>(ceil_div(GG_TARGET_WG, p.row_blocks), ceil_div(cols, GG_MIN_COLS));
  p.cols_per_split = round_up((cols + want - 1) / want, GG_CT);
  p.nsplit = ceil_div(cols, p.cols_per_split);
  return p;
}
// symmetric: X2 == NULL (n2 is ignored)
static inline GGPlan gram_grad_plan(int64_t n, int64_t n2, int D, bool symmetric) {
  GGPlan P{};
  P.symmetric = symmetric;
  P.a = gg_pass(n, symmetric ? n : n2);
  const size_t nd = (size_t)n * D * 8, ns = (size_t)P.a.nsplit;
  P.a.PX = gg_take(P, ns * nd), P.PL = gg_take(P, ns * nd), P.PV = gg_take(P, ns * n * 8);
  P.Lrow = gg_take(P, nd), P.Vrow = gg_take(P, (size_t)n * 8);
  if (!symmetric) {
    P.b = gg_pass(n2, n);
    P.b.PX = gg_take(P, (size_t)P.b.nsplit * n2 * D * 8);
  }
  return P;
}

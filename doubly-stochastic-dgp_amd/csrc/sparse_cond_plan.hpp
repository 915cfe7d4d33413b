// Host plan of the sparse conditional without q_sqrt and of its reverse pass (sparse_cond.hip): the column tiles of A = Lu^-1 K(Z, X), the
// row splits of the reverse pass and the carve-up of the caller's scratch block, from (n, M, D, DO) alone — nothing else, so the summation
// order, and with it every bit of the results, depends neither on the device nor on which outputs the caller asks for.  No HIP:
// tests/host/sparse_cond_plan_check.cpp compiles it alone.
//
// A is M x n, row-major: a COLUMN of A belongs to a ROW of X.  k_sc_fwd gives every tile of SC_CT columns one workgroup, which walks the
// rows of A in chunks of SC_KC.  k_sc_adj cuts the tiles into `nsplit` row splits (of X: `tiles_per_split` whole tiles each, the last
// ragged) and the rows of A into `row_chunks` chunks of SC_KC; workgroup (s, c) walks the tiles of split s for the rows of chunk c and
// leaves the split's partial of W_bar = A gm for those rows.  k_sc_wsum adds the partials in ascending split order.
#pragma once
#include "plan_types.hpp"

#define SC_T 256            // threads per workgroup: four waves, each 16 columns (forward) or 16 rows (reverse) of the staged block
#define SC_CT 64            // columns of A per tile
#define SC_KC 64            // rows of A per staged block
#define SC_LD 80            // doubles per row of the staged block in the LDS (two 16-lane groups land on disjoint banks)
#define SC_DOC 16           // outputs per MFMA chunk
#define SC_DOG 4            // chunks a wave holds in registers: 64 outputs per sweep over A
#define SC_MAX_M 2048
#define SC_MAX_D_GRAD 32    // dsdgp_gram_grad's input_dim limit: the reverse pass inherits it
#define SC_TARGET_SPLITS 256
#define SC_MAX_ROWS ((int64_t)1 << 31)
#define SC_SCRATCH_CAP ((size_t)8 << 30)

struct SCRegion { size_t off, bytes; };      // of the caller's scratch; off is a multiple of 256

struct SCPlan {
  int64_t n;
  int M, D, DO;
  int64_t tiles;                             // ceil(n / SC_CT): the forward's workgroups
  int row_chunks;                            // ceil(M / SC_KC)
  int out_groups;                            // ceil(DO / (SC_DOC SC_DOG)): sweeps over A (1 up to 64 outputs)
  int64_t tiles_per_split;
  int nsplit;
  // forward (and the reverse's repeat of it): Ku -> Lu (M x M), A (M x n), W (M x DO), Z and X moved to Z's first row as origin (M x D, n x D)
  SCRegion Ku, A, W, Zc, Xc;
  size_t fwd_total;
  // reverse: A_bar -> K1_bar (M x n), the splits' partials of W_bar (nsplit x M x DO), W_bar, V = Lu^-T W_bar (M x DO), T = K1_bar A^T ->
  // Lu_bar, Q = Lu^T Lu_bar, S = 1/2 (P + P^T), St = (Lu^-T S)^T -> Ku_bar^T (M x M each), the two Gram reverse passes' d_X (M x D each)
  // and d_kern (2 + D doubles each)
  SCRegion Abar, PW, Wbar, V, T, Q, S, St, dZ1, dZ2, dk1, dk2;
  size_t total;
};

static inline SCRegion sc_take(size_t& total, size_t bytes) {
  const SCRegion r{total, bytes};
  total += (size_t)round_up((int64_t)bytes, 256);
  return r;
}

static inline SCPlan sparse_cond_plan(int64_t n, int M, int D, int DO) {
  SCPlan P{};
  P.n = n, P.M = M, P.D = D, P.DO = DO;
  P.tiles = (n + SC_CT - 1) / SC_CT;
  P.row_chunks = ceil_div(M, SC_KC);
  P.out_groups = ceil_div(DO, SC_DOC * SC_DOG);
  const int64_t want = std::min<int64_t>(P.tiles, SC_TARGET_SPLITS);
  P.tiles_per_split = (P.tiles + want - 1) / want;
  P.nsplit = (int)((P.tiles + P.tiles_per_split - 1) / P.tiles_per_split);
  const size_t mm = (size_t)M * M * 8, mn = (size_t)M * (size_t)n * 8, mo = (size_t)M * DO * 8, md = (size_t)M * D * 8;
  size_t t = 0;
  P.Ku = sc_take(t, mm), P.A = sc_take(t, mn), P.W = sc_take(t, mo), P.Zc = sc_take(t, md), P.Xc = sc_take(t, (size_t)n * D * 8);
  P.fwd_total = t;
  P.Abar = sc_take(t, mn), P.PW = sc_take(t, (size_t)P.nsplit * mo), P.Wbar = sc_take(t, mo), P.V = sc_take(t, mo);
  P.T = sc_take(t, mm), P.Q = sc_take(t, mm), P.S = sc_take(t, mm), P.St = sc_take(t, mm);
  P.dZ1 = sc_take(t, md), P.dZ2 = sc_take(t, md);
  P.dk1 = sc_take(t, (size_t)(2 + D) * 8), P.dk2 = sc_take(t, (size_t)(2 + D) * 8);
  P.total = t;
  return P;
}

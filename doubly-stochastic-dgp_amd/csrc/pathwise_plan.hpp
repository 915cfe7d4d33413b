// Host plan of the pathwise (Matheron) function draws (pathwise.hip): the frequency chunks, k-groups, output sweeps and Z tiles of the
// evaluation kernel and its LDS bytes from (L, M, D, DO) alone, and the carve-up of the scratch block of dsdgp_pathwise_weights from
// (M, D, DO, S) alone.  Neither the row count n nor (for the kernel) the draw count S enters: the summation order of an entry, and with
// it every bit of it, depends neither on how many rows a call has nor on where in the call a row stands.  No HIP:
// tests/host/pathwise_plan_check.cpp compiles it alone.
//
// k_pw_eval: workgroup (tile, s) owns PW_RT rows of draw s, wave w the 16 rows 16 w .. 16 w + 15 of them.  Per sweep of PW_OG output
// chunks of PW_OC outputs it walks
//   the frequencies in chunks of PW_LC (the last ragged: +0.0 weights), each chunk's theta = (x - c) Omega over the input dimensions in
//   staged chunks of PW_DC, four dimensions (one k-group) per MFMA, the last group ragged (the loop ends at D);
//   the inducing rows in tiles of PW_ZT (the last ragged: +0.0 rows of V), their squared distances over the same chunks of PW_DC.
#pragma once
#include "plan_types.hpp"

#define PW_T 256              // threads per workgroup: four waves of 16 rows
#define PW_RT 64              // rows per workgroup
#define PW_LC 32              // frequencies per staged chunk: two MFMA tiles of 16
#define PW_DC 16              // input dimensions per staged chunk
#define PW_OC 16              // outputs per MFMA chunk
#define PW_OG 2               // chunks a wave holds in registers: 32 outputs per sweep over the frequencies and the inducing rows
#define PW_ZT 64              // inducing rows per staged tile
#define PW_XLD (PW_DC + 2)    // doubles per staged row of X and of Z (16 rows land on 16 disjoint bank pairs)
#define PW_OLD (PW_LC + 16)   // doubles per staged row of Omega (two 16-lane groups land on disjoint banks)
#define PW_WLD (PW_OC * PW_OG + 16)      // doubles per staged row of the weights Wc, Ws and of V
#define PW_MAX_M 2048
#define PW_MAX_L 65536
#define PW_MAX_S 65535        // the draws are the launch's second grid dimension
#define PW_MAX_ROWS ((int64_t)1 << 31)
#define PW_LDS_LIMIT 65536
#define PW_SCRATCH_CAP ((size_t)8 << 30)
#define PW_FAST_MAX 4096.0    // |theta| below it: two-constant reduction by pi/2; at or above it, or not finite: the library routine

struct PWPlan {
  int L, M, D, DO;
  int freq_chunks;            // ceil(L / PW_LC)
  int d_chunks;               // ceil(D / PW_DC)
  int k_groups;               // ceil(D / 4): MFMA k-steps of a theta tile
  int out_sweeps;             // ceil(DO / (PW_OC PW_OG))
  int z_tiles;                // ceil(M / PW_ZT); 0: the prior part alone
  size_t lds_x, lds_org, lds_omega, lds_w, lds_z, lds_ils, lds_bytes;      // the static LDS arrays of k_pw_eval
};

static inline PWPlan pathwise_plan(int L, int M, int D, int DO) {
  PWPlan P{};
  P.L = L, P.M = M, P.D = D, P.DO = DO;
  P.freq_chunks = ceil_div(L, PW_LC);
  P.d_chunks = ceil_div(D, PW_DC);
  P.k_groups = ceil_div(D, 4);
  P.out_sweeps = ceil_div(DO, PW_OC * PW_OG);
  P.z_tiles = ceil_div(M, PW_ZT);
  P.lds_x = (size_t)PW_RT * PW_XLD * 8, P.lds_org = (size_t)PW_DC * 8, P.lds_omega = (size_t)PW_DC * PW_OLD * 8;
  P.lds_w = (size_t)std::max(2 * PW_LC, PW_ZT) * PW_WLD * 8;      // [Wc; Ws] of a frequency chunk, then V of a Z tile
  P.lds_z = (size_t)PW_ZT * PW_XLD * 8, P.lds_ils = (size_t)PW_DC * 8;
  P.lds_bytes = P.lds_x + P.lds_org + P.lds_omega + P.lds_w + P.lds_z + P.lds_ils;
  return P;
}

struct PWRegion { size_t off, bytes; };      // of the caller's scratch; off is a multiple of 256

// dsdgp_pathwise_weights: Z moved to its first row as origin (M x D), Ku -> Lu (M x M), and three M x (S DO) matrices, column s DO + o
// for output o of draw s: U = q_mu + q_sqrt eps, LU = Lu U (white only), F0 = f0(Z) -> U - F0 -> v
struct PWScratch {
  int M, D, DO, S;
  PWRegion Zc, Ku, U, LU, F0;
  size_t total;
};

static inline PWRegion pw_take(size_t& total, size_t bytes) {
  const PWRegion r{total, bytes};
  total += (size_t)round_up((int64_t)bytes, 256);
  return r;
}

static inline PWScratch pathwise_scratch(int M, int D, int DO, int S) {
  PWScratch P{};
  P.M = M, P.D = D, P.DO = DO, P.S = S;
  const size_t wide = (size_t)M * (size_t)S * (size_t)DO * 8;
  size_t t = 0;
  P.Zc = pw_take(t, (size_t)M * D * 8), P.Ku = pw_take(t, (size_t)M * M * 8);
  P.U = pw_take(t, wide), P.LU = pw_take(t, wide), P.F0 = pw_take(t, wide);
  P.total = t;
  return P;
}

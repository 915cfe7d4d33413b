// Host plan of the RBF kernel expectations (psi.hip) and of their reverse pass (psi_grad.hip): the row splits of the hot kernels, the row
// chunks of k_psig_z and the carve-up of the call's scratch, from (n, M, D) and what the caller asks for — nothing else, so the summation
// order, and with it every bit of the results, does not depend on the device.  No HIP: tests/host/psi_plan_check.cpp compiles it alone.
#pragma once
#include "plan_types.hpp"

#define PS_MAX_M 2048
#define PS_MAX_D 1024
#define PS_T 256
#define PS_TILE 16          // tile edge of psi2
#define PS_KC 32            // input dimensions per chunk of the delta^2 operand (8 MFMA k-steps)
#define PS_TARGET_WG 4096
#define PS_MIN_ROWS 64      // fewest rows worth a split
#define PS_SCRATCH_CAP ((size_t)8 << 30)
#define PG_MAX_D PS_KC      // the reverse pass takes one chunk of the forward's delta^2 operand
#define PG_Z_ROWS 256       // fewest rows of a chunk of k_psig_z
#define PG_Z_CHUNKS 256     // most chunks

struct PsiRegion { size_t off, bytes; };      // of the call's scratch; off is a multiple of 256, bytes == 0: not asked for

struct PsiPlan {
  int Dq, nt1, ntiles;                        // D rounded up to 4; tiles of 16 inducing inputs; tiles of psi2's lower triangle
  int64_t rows_per_split, g_rows_per_split, rows_per_chunk;
  int nsplit, g_nsplit, nchunk;               // k_psi2 (by ntiles), k_psi2_grad (by nt1), k_psig_z
  PsiRegion ls, W1, W2, T, H1, H2, L;         // both calls: lengthscales (l^2; the reverse pass l as well), the row tables, the n x M table
  PsiRegion part;                             // forward: nsplit x ntiles partial tiles
  PsiRegion A, q, Gs, Ppart, Spart, Zpart, Crow, AV;      // reverse
  size_t total;
};

static inline PsiRegion psi_take(PsiPlan& P, size_t bytes) {
  const PsiRegion r{P.total, bytes};
  P.total += (size_t)round_up((int64_t)bytes, 256);
  return r;
}
// splits of whole blocks of 16 rows for a kernel with `wgs` workgroups per split: about PS_TARGET_WG workgroups, PS_MIN_ROWS rows or more
static inline void psi_splits(int64_t n, int wgs, int64_t& rows, int& nsplit) {
  const int64_t want = std::min(ceil_div(PS_TARGET_WG, wgs), ceil_div(n, PS_MIN_ROWS));
  rows = round_up(ceil_div(n, want), 16);
  nsplit = ceil_div(n, rows);
}
// what both calls need; ls_copies: 1 (l^2) or 2 (l^2, then l)
static inline PsiPlan psi_plan_tables(int64_t n, int M, int D, int ls_copies, bool want_L) {
  PsiPlan P{};
  P.Dq = (int)round_up(D, 4), P.nt1 = ceil_div(M, PS_TILE), P.ntiles = P.nt1 * (P.nt1 + 1) / 2;
  const size_t nd = (size_t)n * D * 8;
  P.ls = psi_take(P, (size_t)ls_copies * D * 8), P.W1 = psi_take(P, nd), P.W2 = psi_take(P, nd), P.T = psi_take(P, (size_t)n * P.Dq * 8);
  P.H1 = psi_take(P, (size_t)n * 8), P.H2 = psi_take(P, (size_t)n * 8), P.L = psi_take(P, want_L ? (size_t)n * M * 8 : 0);
  return P;
}
static inline PsiPlan psi_plan_forward(int64_t n, int M, int D, bool want_psi2) {
  PsiPlan P = psi_plan_tables(n, M, D, 1, want_psi2);
  psi_splits(n, P.ntiles, P.rows_per_split, P.nsplit);
  P.part = psi_take(P, want_psi2 ? (size_t)P.nsplit * P.ntiles * PS_TILE * PS_TILE * 8 : 0);
  return P;
}
static inline PsiPlan psi_plan_reverse(int64_t n, int M, int D, bool has_g1, bool has_g2, bool want_dZ) {
  PsiPlan P = psi_plan_tables(n, M, D, 2, has_g2);
  psi_splits(n, P.nt1, P.g_rows_per_split, P.g_nsplit);
  P.rows_per_chunk = ceil_div(n, std::min(ceil_div(n, PG_Z_ROWS), PG_Z_CHUNKS)), P.nchunk = ceil_div(n, P.rows_per_chunk);
  const size_t nd = (size_t)n * D * 8, nm = (size_t)n * M * 8, md = (size_t)M * D * 8;
  P.A = psi_take(P, has_g1 ? nm : 0), P.q = psi_take(P, has_g2 ? nm : 0), P.Gs = psi_take(P, has_g2 ? (size_t)M * M * 8 : 0);
  P.Ppart = psi_take(P, has_g2 ? P.nt1 * nd : 0), P.Spart = psi_take(P, has_g2 && want_dZ ? P.g_nsplit * md : 0);
  P.Zpart = psi_take(P, want_dZ ? P.nchunk * md : 0), P.Crow = psi_take(P, nd), P.AV = psi_take(P, (size_t)n * 8);
  return P;
}

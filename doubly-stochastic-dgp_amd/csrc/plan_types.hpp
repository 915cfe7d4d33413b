// Plain records and size policies that the library (through common.hpp) shares with the split-K planner (model_plan.hpp): integer helpers,
// paddings, the job and layer records the device reads.  No HIP, so the planner compiles for the host alone (tests/host/plan_check.cpp).
#pragma once
#include <stdint.h>
#include <algorithm>

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
// Padded inducing count used by every device-side M x M operand (identity pad on Ku, zero pad elsewhere).  The chain kernels
// exist for every multiple of 16 up to 128, of 32 up to 256, of 64 up to 512 and of 128 up to 1024: M = 100 (the reference
// demo size, demos/run_regression.py:57) runs as 112, not 128; M = 300 as 320, not 512.
static inline int pad_M(int M) { return M <= 32 ? 32 : (int)round_up(M, M <= 128 ? 16 : (M <= 256 ? 32 : (M <= 512 ? 64 : 128))); }
// Row count of the M-major per-row intermediates (A, E, GW) and of the weight-gradient results: whole 64 x 64 split-K tiles
static inline int pad_Mw(int Mp) { return (int)round_up(Mp, 64); }

// out[split][i][j] = sum_{r in split} P[i][r] * scale[r] * Q[j][r]
struct WgradJob {
  const double* P;
  const double* Q;
  const double* scale;  // or NULL
  double* out;          // [nsplit][rowsP][ldo]
  int32_t ti, tj;       // tiles in i / j (tile = 16*NI x 16*NJ; the last j tile may be partial, see qrows16)
  int32_t ldo;
  int32_t task_start;
  int32_t sym;          // P == Q (symmetric result): only tiles with tile_j <= tile_i are computed
  int32_t qrows16;      // rows of Q / 16 (= columns of the result / 16)
  int32_t ns_diag;      // sym: K splits of the (cheaper, 10/16) diagonal tiles; their tasks follow the off-diagonal ones
  int32_t ng;           // 0: one result per task.  1..4: a GROUP of ng symmetric, scaled results that share P = Q (the P_d of a layer)
                        // on 32 x 32 tiles, result o at out + o * ostride, scaled by scale + o * sstride (see k_wgrad_coop)
  // In-launch split-K reduction (round 6): with `fin` set the LAST of a tile's splits to arrive (ticket counter `tick[tile]`, zero between
  // launches) adds the tile's partials in split order and writes rows < fin_rows, columns < fin_cols of the result (leading dimension
  // fin_ld) — and, for sym, the mirror tile / the uncomputed upper blocks of a diagonal tile — so that no reduction launch follows the
  // products.  One split: the tile goes from registers to `fin`, `out` is not touched.  NULL: partials only (k_reduce_grouped adds them).
  double* fin;
  int32_t* tick;
  int32_t fin_ld, fin_rows, fin_cols, pad2;
  int64_t ostride, sstride;      // ng > 0: distance between the group's results / between their scale vectors (doubles)
};
struct RedJob {
  const double* part;
  double* out;
  int64_t count;
  int32_t nsplit, blk_start;
  int32_t wide;        // wide: few outputs, many splits -> one workgroup per output element (fixed-order tree)
  int32_t sym_n;       // > 0: symmetric result whose tiles above the diagonal were not computed (mirrored here)
  int32_t sym_tile;
  int64_t pstride;     // elements between consecutive splits of `part`
  int32_t in_ld, out_ld;   // > 0: 2-D result, `part` rows have leading dimension in_ld (the weight-gradient products run on
                           // whole 64-row tiles: Mw = round_up(Mp, 64)), `out` rows out_ld; 0: linear
  int32_t ways;            // 4: a workgroup owns 64 outputs, each of its four waves a quarter of the splits (many splits, few outputs:
                           // one thread per output walked 156 splits eight at a time — 20 dependent round trips); else one thread each
};

// K splits of a weight-gradient launch: about `target_tasks` workgroup tasks (512 = two workgroups of four waves per CU), every
// wave at least two 16-row chunks
static inline int choose_nsplit(int tiles_per_split, int64_t nchunks, int target_tasks) {
  const int64_t ns = target_tasks / (tiles_per_split > 0 ? tiles_per_split : 1), cap = nchunks / 8;
  return (int)std::max<int64_t>(1, std::min(ns, std::max<int64_t>(cap, 1)));
}
// 64 x 64 tiles (WG_NI = 4 blocks of 16) on Mw = round_up(Mp, 64) rows (zero rows beyond Mp)
enum { WG_NI = 4 };
static inline int wgrad_ti(int Mp) { return pad_Mw(Mp) / 64; }
// device-resident per-layer descriptor shared by all the small per-layer kernels
struct LayerDev {
  int32_t M, Mp, D_in, D_out, DP4, DP16, DinP16, kern_kind, ard, has_white, white, hyp_parts;   // rows of hyp2part per backward: > 0 written by k_asm_kbar (folded), < 0: -NPART rows by k_asm_hyp_part
  int32_t kl_parts, kvar_identity;   // partial sums k_kl_part leaves in klpart (the launch's block columns); dsdgp_layer_desc::kvar_identity
  int64_t off_Z, off_q_mu, off_q_sqrt, off_kvar, off_kls, off_wvar;
  double *Zp, *Zs, *hyp, *Tp, *TpT, *qmu, *qmu4;
  double *Kp, *Linv, *LinvT, *Kinv, *scal;
  double *V, *nL, *Sd, *klv;
  double *U, *n4, *PT, *UU, *Kbar, *wm, *wk;
  double *bigred, *thinq, *thinz, *hyp_red;
  double* meanAB;              // (64 ti x DP16) [X;1]^T MB^T: gradient of a trainable Linear mean function (rows: D_in of A, then b)
  int64_t off_mean_A, off_mean_b;   // -1: not a free parameter
  double *R2, *Zp1, *WZ;       // scaled squared distances of Z (Mp x Mp); [Z | 1] and wm [Z | 1] (Mp x DinP16, D_in > 32 only)
  double *klpart, *hyp2part;   // [NPART] KL partial sums ; [NPART][D_in + 2] Ku-side hyper-parameter partials
  // alg_g: sum_r e_r a_r^T is assembled from the (already needed) P_d and A mbar^T instead of a split-K product over the rows:
  //   sum_r e a^T = sum_d (2 Ku^-1 S_d - I) P_d + n (A mbar^T)^T   (e = Ku^-1 abar - g a, abar = sum_d 2 vbar_d S_d a + q_mu mbar)
  // KS_d = Ku^-1 S_d (parameter-only, side stream), GS_d = KS_d P_d (same launch as P_d T_d).  Chosen per layer when the row
  // count dwarfs D_out * M (2 D_out M^3 flops instead of 2 M^2 R, and the chain stops writing E).
  double *KS, *GS;
  int32_t alg_g, need_tpt;   // need_tpt: some chain kernel reads q_sqrt^T (Mp >= 512 row-oriented loads; the Csave backward chain)
  double *wLbar, *wH, *wY, *wX;  // white=True: Cholesky-adjoint temporaries (Mp x Mp each)
  // natural-gradient temporaries, (D_out x Mp x Mp) each unless noted
  double *ngTI, *ngTinv, *ngTbar, *ngH, *ngY, *ngX, *ngSinv, *ngA, *ngLAinv, *ngLAinvT, *ngV /* D_out x Mp */, *ngTheta1 /* D_out x Mp */, *ngScal /* 2 x D_out */;
};

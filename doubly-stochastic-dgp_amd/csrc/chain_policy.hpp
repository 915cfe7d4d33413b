// Size rules of the chain launches, as plain host functions of plain values (no HIP, no dsdgp_model): which instance a launch of a shape
// takes, what it leaves for the reverse pass, how many workgroups share a row block, and the scope of the fused last layer.  The launchers
// (layer_sm.hip, layer_last.hip, layer_gemm.hip) and the forward plan (forward_plan.hpp) read the same functions;
// tests/host/forward_check.cpp walks them on the CPU.
#pragma once
#include <stdlib.h>
#include "plan_types.hpp"
#include "../../include/dsdgp.h"

#define XCH 64             // columns of x/l the chain kernels stage per chunk; inputs wider than this take the WIDE instances
#define HEAD_THREADS 512   // threads of a block of the head launch (head_impl.hpp)
#define GL_EPI_ROWS 64     // rows per block of the GEMM-formulated forward pass's epilogue (layer_gemm.hip)

// waves per 16-row block.  Launches with few row blocks (the N-row first layer: 63 blocks at N = 1000) are latency-bound —
// one dependent MFMA chain per wave on a mostly idle chip — so they take twice the waves per block (half the chain each).
#define SM_SMALL_BLOCKS 160
#define SM_BWD_RESIDENT_8W 768
static inline bool sm_small(int Mp, int64_t nblk, int D_in, bool bwd) {
  // measured (tools/ab_kernels.py): M = 256 — the 8-wave form (two row blocks per wave instead of four) wins at every size
  // (-7 % on both chains); M = 128 — it wins for the backward chain while one round of it holds the launch (see below), for the
  // forward chain only on small launches (the 4-wave forward instance has the early-mean specialisation)
  // Mp = 160 .. 224 follow the M = 256 rule (tools/bench_padding.py: with 4 waves M = 224 ran no faster than M = 256 with 8)
  // round 5, backward chain at M = 128: the 8-wave instance holds 77 VGPRs = three workgroups per CU = 768 resident row blocks; a
  // launch with more runs in two rounds, the second one latency-bound on a third of the chip (config 2: 1250 blocks, 482 late
  // starters, 139 us).  The 4-wave instance with the paired d-loop (96 VGPRs, five workgroups per CU) keeps 1280 blocks resident with
  // the MFMA pipe saturated in the d-loop: 124 us.  (DSDGP_SM_BWD_LIM128: A/B aid.)
  // tests/test_gpu_large_launch_m128.py runs both sides of both M = 128 thresholds (161 / 769 row blocks) against the oracle;
  // tests/test_gpu_wide_input.py both sides of D_in <= XCH (64 | 65 at Mp = 128: the 8-wave and the 4-wave instance of the same launch)
  static const int64_t bwd_lim128 = getenv("DSDGP_SM_BWD_LIM128") ? atoll(getenv("DSDGP_SM_BWD_LIM128")) : SM_BWD_RESIDENT_8W;
  const int64_t lim = Mp > 128 ? ((int64_t)1 << 40) : (bwd ? bwd_lim128 : SM_SMALL_BLOCKS);
  return Mp >= 128 && Mp <= 256 && nblk <= lim && D_in <= XCH;
}
// waves per row block of the instance that a launch of this shape takes
static inline int sm_nw(int Mp, int64_t nblk, int D_in, bool bwd) {
  return (Mp > 512 || (Mp == 512 && D_in <= XCH && !bwd)) ? 16 : (Mp > 256 ? 8 : (sm_small(Mp, nblk, D_in, bwd) ? 8 : 4));
}
// rows of hyp_part the backward chain writes for ld padded rows (one per wave)
static inline int64_t sm_hyp_parts(int64_t ld, int Mp, int D_in) { return (int64_t)sm_nw(Mp, ceil_div(ld, 16), D_in, true) * ceil_div(ld, 16); }
// whether the backward chain of this shape can take the adjoint prologue (LayerBwdArgs::up_dF): it parks 2 x 16 x D_out partial sums
// in the chain's reduction scratch
static inline int sm_adj_fusable(int Mp, int64_t nblk, int D_in, int D_out) {
  if (D_in > XCH) return 0;
  const int NW = sm_nw(Mp, nblk, D_in, true);
  const int xch = D_in < XCH ? D_in : XCH;
  return NW * 16 * xch >= 2 * 16 * D_out;
}
// padded inducing counts whose backward chain has a Csave instance (layer_sm_impl.hpp: sm_cs_inst)
static inline int sm_cs_built(int Mp) { return Mp > 256 || Mp == 32 || Mp == 64 || Mp == 128 || Mp == 256; }

// Csave backward chain: the forward chain keeps c_d = q_sqrt_d^T a (D_out x Mp doubles per row) so that the backward chain's
// abar = sum_d 2 vbar_d S_d a becomes the triangular product sum_d q_sqrt_d (2 vbar_d c_d): half the MFMAs of that loop.  Measured
// (profiles/r02_fp64_mfma_notes.md): a clear win from Mp = 512 (cfg 4 +10 %, cfg 5 +14 %); at Mp = 128 / 256 the d-loop turns from
// MFMA-throughput-bound into latency-bound and the chain gets no faster, so those sizes keep the S_d form.
// (save_c: DSDGP_FORCE save_c — 0 never / 1 for Mp > 256 / 2 every size)
static inline bool save_c_enabled(int save_c, int Mp) { return save_c >= 2 || (save_c == 1 && Mp > 256); }
// workgroups per row block of a chain launch with few row blocks (the d-split).  < 256 row blocks (first layers, small shards): up to
// four, ~512 workgroups.  256..511 row blocks (the per-GPU shards of configs 4 / 5: two rounds on 256 CUs, the second a quarter to a
// half full): two or three pack better, but every workgroup repeats the prologue (Kuf tile and the two triangular chains), so only
// when each keeps at least five outputs (measured: config 4, D_out = 30, -6.6 % per step; config 5, D_out = 8, +6.7 % without the rule)
static inline int chain_d_split(int64_t nblk, int D_out) {
  int ds = 1;
  if (nblk < 256) ds = (int)std::min<int64_t>(4, std::max<int64_t>(1, 512 / nblk));
  else if (nblk < 512) ds = (int)std::min<int64_t>(1024 / nblk, D_out / 5);
  if (ds > D_out) ds = D_out;
  return ds < 1 ? 1 : ds;
}
// LayerBwdArgs::d_split of a backward chain over nblk row blocks. Few of them (the N-row first layer, small shards): up to four
// workgroups per row block share the d-loop. Only from Mp = 512 (bwd_split = 2 forces it everywhere, 0 disables): every workgroup of a
// split repeats the chain's prologue and epilogue phases. 63-row-block first layer of config 2 (M = 128): +57 us with the
// __threadfence() hand-over of round 2, still +6 us per step with the fence-free sc1 hand-over of round 3 (cutting the upper layer's
// weight-gradient task list over both streams to use the shortened chain: +10..+20 us); -0.9 ms on the 32-row-block, 30-output first
// layer of config 4 (M = 512).  (bwd_split: DSDGP_FORCE bwd_split; has_part: the layer has the partial-tile buffer)
static inline int bwd_d_split(int bwd_split, int Mp, bool has_part, int64_t nblk, int D_out) {
  const bool want = bwd_split >= 2 || (bwd_split == 1 && Mp > 256);
  return (want && has_part) ? chain_d_split(nblk, D_out) : 1;
}
// blocks of the GEMM-formulated forward pass's epilogue, each leaving one likelihood partial
static inline int layer_gemm_lik_blocks(int64_t Rin, int D_out) { return ceil_div(round_up(Rin, 16), GL_EPI_ROWS); }
// blocks of the head launch that draw `count` N(0,1) numbers (two per thread and pass, at most 64 blocks)
static inline int head_draw_blocks(int64_t count) { return (int)std::min<int64_t>(64, ceil_div((count + 1) / 2, 4 * HEAD_THREADS)); }

// The last layer of a training step as one launch (layer_last.hip): forward chain + Gaussian likelihood + reverse mode of the same row
// block.  Shapes the launch exists for:
static inline int layer_last_built(int Mp, int D_in, int D_out) { return (Mp == 128 || Mp == 256) && D_out == 1 && D_in <= 16; }
// THE decision whether a last layer is inside that launch's scope, on plain values: the forward plan (fwd_plan) takes it once, at
// forward time — and then launches no forward chain — and layer_last_launch only asserts it, fed from its two argument blocks.
struct LastScope {
  int Mp, D_in, D_out, kern_kind;
  int hyp_rows;      // rows of hyp_part per row block (sm_hyp_parts / row blocks): what the reduction plan counts
  // the forward side: likelihood in the epilogue, A kept, c_d kept, a sample F wanted, input rows repeated, whitened form, mean function
  bool lik, save_A, save_C, want_F;
  int rep;
  bool whitened;
  int mean_kind, d_split;
  // the backward side as it is known at forward time: its d_split (bwd_d_split), whether E is wanted (no algebraic dl/dKu assembly)
  int bwd_d_split;
  bool want_E;
};
static inline int layer_last_fusable(const LastScope& s) {
  const int waves = s.Mp == 128 ? 4 : 8;      // per row block of the instance: each writes one row of hyp_part, the surplus rows are zeroed
  return layer_last_built(s.Mp, s.D_in, s.D_out) && (s.kern_kind == DSDGP_KERN_RBF || s.kern_kind == DSDGP_KERN_MATERN52) &&
         s.hyp_rows >= waves && s.lik && s.save_A && !s.save_C && !s.want_F && s.rep == 1 && !s.whitened &&
         s.mean_kind == DSDGP_MEAN_ZERO && s.d_split <= 1 && s.bwd_d_split <= 1 && !s.want_E;
}

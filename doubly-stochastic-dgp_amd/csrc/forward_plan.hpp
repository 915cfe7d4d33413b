// What a forward pass launches and keeps, as pure host code (no HIP call, no dsdgp_model): fwd_plan() turns the call and the model, as
// plain values, into a FwdPlan — every decision of the forward pass (model_schedule.hpp: forward_pass places the draws and prepares,
// forward_layers fills the argument blocks and launches what the plan says).  FwdRecord is what the reverse pass may read of the last
// forward pass; it is written by its named transitions only.  tests/host/forward_check.cpp walks the plan over a grid of inputs.
#pragma once
#include "chain_policy.hpp"

static_assert(DSDGP_MAX_LAYERS <= 32, "FwdIn::caller_z is a 32-bit mask");
struct FwdIn {
  // the call.  prepare: it runs a prepare of its own (an evaluation, a saved forward pass), so the inner layers' draws may be placed ahead
  // of the factorisation; save: for a reverse pass; need_last_F: a sample of the last layer is wanted; lik_target: targets are given (an
  // evaluation); caller_z: bit l set = layer l's draws are the caller's; sample_w: quadrature sample weights are set
  int64_t n;
  int S;
  bool prepare, save, need_last_F, lik_target, sample_w, with_grad;
  uint32_t caller_z;
  // the model.  lik_elementwise / lik_gaussian: the likelihood's family (MultiClass is neither); overlap: two streams at this (n, S);
  // timing: the chains' phase clocks are on (debug aid)
  int L;
  bool white, lik_elementwise, lik_gaussian;
  int grad_first;
  bool grad_q_only, head_ok, overlap, timing;
  struct Layer {
    int Mp, M, D_in, D_out, kern_kind, mean_kind, prop;
    bool gemm, alg_g, need_tpt, has_C, has_bpart;      // has_C / has_bpart: the c_d buffer / the backward d-split's partial tiles exist
  } layer[DSDGP_MAX_LAYERS];
  struct { int white_fwd, cs_min_blocks, cs_min_dout, cs_max_dout, last_fuse, last_min_blocks, bwd_split, lik_fuse; } force;      // DSDGP_FORCE
};

enum DrawsAt : uint8_t { DRAWS_INLINE, DRAWS_HEAD, DRAWS_SIDE };      // the inner layers' draws that no caller covers: ahead of each chain / in spare
                                                                     // block columns of the head launch / on the side stream while Ku is factorised
enum DrawFrom : uint8_t { DRAW_NONE, DRAW_CALLER, DRAW_HERE, DRAW_READY };      // no F / the caller's zs / drawn ahead of the chain / made where DrawsAt says
enum FwdLaunch : uint8_t { LAUNCH_CHAIN, LAUNCH_GEMM, LAUNCH_WITH_REVERSE };     // WITH_REVERSE: no launch now, the reverse pass runs it (layer_last.hip)
enum LikRoute : uint8_t { LIK_NONE, LIK_IN_CHAIN, LIK_ELEMENTWISE, LIK_MULTICLASS };
struct FwdPlan {
  bool join_prep_first;      // the whitened form reads V, nL: the parameter products (side stream in the overlapped schedule)
  DrawsAt draws;
  bool draws_ahead;          //   ... some layer's draws are made there (DRAW_READY) ...
  int head_nblk;             //   ... in this many block columns of the head launch
  // the last layer of a deep model has one output row per input row: its transposed adjoints come straight from the likelihood kernel
  // (no k_adj_prep launch on the critical path) — or, Gaussian likelihood without quadrature weights, from the last forward chain's own
  // epilogue (no likelihood launch either)
  bool adjoints_from_lik, lik_in_chain;
  LikRoute lik;
  int lik_nblocks;           // partial sums the likelihood's route leaves in lik_part
  struct Layer {
    int64_t Rin, ld;
    int rep;
    bool whitened, want_F;
    DrawFrom draw;
    bool save_A, save_C, save_XT1;
    int d_split;
    bool lik_epilogue;
    FwdLaunch launch;
    bool concat;             // input propagation: [X_prop | F] is formed for the next layer
  } layer[DSDGP_MAX_LAYERS];
  int hyp_rows, bwd_d_split;      // last layer: rows of hyp_part per row block and the backward chain's d_split, as LAUNCH_WITH_REVERSE assumed them
};

// Whether the last layer's forward chain, the Gaussian likelihood and its reverse pass run as ONE launch in this step: the properties of
// the model and the step here, the launch's scope — backward side included — in layer_last_fusable (chain_policy.hpp)
static inline bool last_chain_fusable(const FwdIn& in, const FwdPlan& p) {
  const int l = in.L - 1;
  const FwdIn::Layer& v = in.layer[l];
  const FwdPlan::Layer& y = p.layer[l];
  // (bwd_split = 2 forces split chains everywhere: a D_out = 1 chain has nothing to split, d_split alone would not say so)
  if (in.force.last_fuse == 0 || in.force.bwd_split >= 2 || !v.need_tpt || in.white || v.gemm || in.L < 2) return false;
  if (in.grad_q_only && in.grad_first == in.L - 1) return false;     // that layer runs no backward chain at all
  if (in.timing || ceil_div(y.Rin, 16) < in.force.last_min_blocks) return false;      // the phase clocks are the two chains'
  return layer_last_fusable(LastScope{v.Mp, v.D_in, v.D_out, v.kern_kind, p.hyp_rows, y.lik_epilogue, y.save_A, y.save_C, y.want_F, y.rep,
                                      y.whitened, v.mean_kind, y.d_split, p.bwd_d_split, !v.alg_g});
}

static inline FwdPlan fwd_plan(const FwdIn& in) {
  FwdPlan p{};
  const int L = in.L;
  // Forward-only evaluations of a non-white model (predict_f, ELBO values) run in WHITENED coordinates: with V_d = Lu^-1 q_sqrt_d and
  // nL = Lu^-1 q_mu — both formed for the KL term anyway — mean = a1^T nL and var = kdiag - |a1|^2 + |V_d^T a1|^2 (V_d is
  // lower-triangular like q_sqrt_d), so the chain skips a = Lu^-T a1 (layers.py:188): one of 2 + D_out triangular products per row
  // block, a third of the MFMA work of a D_out = 1 layer.  The training pass keeps `a` (the reverse pass is written in terms of it).
  // Mp <= 256: the larger instances read the factor transposed, which exists for q_sqrt only.
  const bool wf_ok = !in.white && !in.save && in.force.white_fwd != 0;
  p.join_prep_first = wf_ok;
  p.draws = !in.prepare ? DRAWS_INLINE : (in.head_ok ? DRAWS_HEAD : (in.overlap ? DRAWS_SIDE : DRAWS_INLINE));
  p.adjoints_from_lik = in.lik_target && in.with_grad && L > 1 && in.lik_elementwise;
  p.lik_in_chain = p.adjoints_from_lik && in.lik_gaussian && !in.sample_w && in.force.lik_fuse != 0;
  for (int l = 0; l < L; ++l) {
    const FwdIn::Layer& v = in.layer[l];
    FwdPlan::Layer& y = p.layer[l];
    const bool last = (l == L - 1);
    y.Rin = (l == 0) ? in.n : (int64_t)in.S * in.n;
    y.rep = (l == 0) ? in.S : 1;
    y.ld = round_up(y.Rin, 16);
    const int64_t nblk = y.ld / 16;
    y.want_F = !last || in.need_last_F;
    y.whitened = wf_ok && v.Mp <= 256 && !v.gemm;
    if (!y.want_F) y.draw = DRAW_NONE;
    else if (in.caller_z >> l & 1) y.draw = DRAW_CALLER;
    else y.draw = (p.draws != DRAWS_INLINE && !last) ? DRAW_READY : DRAW_HERE;
    if (y.draw == DRAW_READY) {
      p.draws_ahead = true;
      if (p.draws == DRAWS_HEAD) p.head_nblk = std::max(p.head_nblk, head_draw_blocks((int64_t)in.S * in.n * v.D_out));
    }
    y.save_A = in.save && (in.white || l >= in.grad_first);    // layers below the pruned reverse pass keep nothing for it
    // c_d is kept for the backward chain where that pays: enough row blocks to hide the extra latency per output (the N-row first
    // layer is a latency-bound launch) and enough outputs for the halved d-loop to matter
    // (from Mp = 512 one output's product outlasts the staging latency even on a handful of row blocks: always)
    y.save_C = y.save_A && v.has_C && sm_cs_built(v.Mp) &&
               (v.Mp > 256 || (nblk > in.force.cs_min_blocks && v.D_out >= in.force.cs_min_dout && v.D_out <= in.force.cs_max_dout));
    if (v.gemm) y.save_C = y.save_A && v.has_C;      // the triangular abar product halves the largest GEMM of the reverse pass
    // (q, q_sqrt)-only gradients: the lowest layer of the reverse pass runs no backward chain (backward_layers), so it keeps neither
    const bool q_lowest = y.save_A && in.grad_q_only && !in.white && l == in.grad_first;
    if (q_lowest) y.save_C = false;
    y.save_XT1 = y.save_A && !q_lowest;
    y.d_split = chain_d_split(nblk, v.D_out);
    y.lik_epilogue = last && p.lik_in_chain;      // Gaussian variational expectations + adjoints in this chain's epilogue
    y.launch = v.gemm ? LAUNCH_GEMM : LAUNCH_CHAIN;
    y.concat = v.prop > 0 && !last;
  }
  const FwdIn::Layer& v = in.layer[L - 1];
  const FwdPlan::Layer& y = p.layer[L - 1];
  p.hyp_rows = (int)(sm_hyp_parts(y.ld, v.Mp, v.D_in) / (y.ld / 16));
  p.bwd_d_split = bwd_d_split(in.force.bwd_split, v.Mp, v.has_bpart, y.ld / 16, v.D_out);
  if (last_chain_fusable(in, p)) p.layer[L - 1].launch = LAUNCH_WITH_REVERSE;
  if (in.lik_target) {
    const int64_t R = (int64_t)in.S * in.n;
    p.lik = p.lik_in_chain ? LIK_IN_CHAIN : (in.lik_elementwise ? LIK_ELEMENTWISE : LIK_MULTICLASS);
    if (p.lik_in_chain) p.lik_nblocks = v.gemm ? layer_gemm_lik_blocks(y.Rin, v.D_out) : (int)(y.ld / 16) * y.d_split;
    else if (in.lik_elementwise) p.lik_nblocks = ceil_div((p.adjoints_from_lik ? round_up(R, 16) : R) * v.D_out, 256);      // (the padded rows as well)
    else p.lik_nblocks = ceil_div(R, 256);
  }
  return p;
}

// What the reverse pass may read of the last forward pass.  FwdArgs: the chains' forward argument block (LayerFwdArgs, layer.hpp).
struct FwdUsed { const double *X, *z; int64_t zs_s, zs_n, zs_d; };      // a layer's input and draws as its chain was handed them
template <class FwdArgs>
struct FwdRecord {
  struct Layer : FwdUsed { int64_t Rin, ld; int rep; bool c_saved; } layer[DSDGP_MAX_LAYERS];
  int64_t n = 0;
  int S = 0;
  bool adjoints_from_lik = false;      // the last layer's MB / VB were written by the likelihood (kernel or chain epilogue) of this step
  bool last_pending = false;           // the last layer's forward chain has not run: the reverse pass launches it fused with its own (layer_last.hip) ...
  FwdArgs last_fwd;                    //   ... with these arguments ...
  int hyp_rows = 0;                    //   ... and this many rows of hyp_part per row block

  // a forward pass ran as p says; `pending`: the argument block of a LAUNCH_WITH_REVERSE last layer, else null
  void forward_done(const FwdIn& in, const FwdPlan& p, const FwdUsed* used, const FwdArgs* pending) {
    n = in.n; S = in.S; adjoints_from_lik = p.adjoints_from_lik;
    for (int l = 0; l < in.L; ++l) {
      const FwdPlan::Layer& y = p.layer[l];
      Layer& r = layer[l];
      static_cast<FwdUsed&>(r) = used[l];
      r.Rin = y.Rin; r.ld = y.ld; r.rep = y.rep; r.c_saved = y.save_C;
    }
    last_pending = pending != nullptr;
    if (pending) { last_fwd = *pending; hyp_rows = p.hyp_rows; }
  }
  void adjoints_from_caller() { adjoints_from_lik = false; }      // dsdgp_model_backward_adjoints: they are read from lik_dmean / lik_dvar
  void last_launched() { last_pending = false; }
};

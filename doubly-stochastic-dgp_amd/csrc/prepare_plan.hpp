// What a prepare recomputes, as pure host code (no HIP call, no dsdgp_model): ParamState records what the device buffers were computed
// from and is written by its named transitions only; prep_plan() turns it and the call's plain inputs into a PrepPlan — every decision
// of prepare_async (model_schedule.hpp), which only launches what the plan says.  tests/host/prepare_check.cpp walks event sequences.
#pragma once
#include "plan_types.hpp"

// a reverse pass that leaves gradient entries stale: below grad_first, or everything but (q_mu, q_sqrt) (white = True: never restricted)
static inline bool pass_is_pruned(bool white, int grad_first, bool q_only) { return !white && (grad_first > 0 || q_only); }

struct PrepPlan;
// Validity of what the model keeps on the device between calls.  (side_pending / kinv_pending describe the streams: dsdgp_model.)
struct ParamState {
  enum QMoved : uint8_t { Q_NONE, Q_ONE, Q_UNKNOWN };      // since the last prepare: no (q_mu, q_sqrt) moved / layer q_layer's alone / several, unknown
  bool prepared = false;        // Ku's factor, the parameter transforms and the forward-side products belong to theta as it stands
  bool prepared_grad = false;   // the last prepare also produced U_d, n, U_d U_d^T of every layer
  bool track_theta = false;     // dsdgp_model_track_theta: the caller reports its writes to theta
  bool kuu_valid = false;       // Lu / Lu^-1 / Ku^-1 belong to the Z and kernel hyper-parameters currently in theta
  QMoved q = Q_UNKNOWN;         // (read together with kuu_valid)
  int q_layer = -1;
  bool grad_pruned = false;     // the gradient buffer holds a pruned reverse pass (stale entries: dsdgp_model_adam_step refuses it)
  // dsdgp_model_forward_saved was the last evaluation: the workspace holds what a reverse pass over saved_n rows x saved_S samples reads
  // (dsdgp_model_backward_adjoints).  Dropped by every writer of the workspace and every move of theta.
  bool saved = false;
  int64_t saved_n = 0;
  int saved_S = 0;

  // theta moved (an optimiser step, the caller's write: dsdgp_model_theta_changed): nothing prepared from it stands
  void theta_moved() { prepared = kuu_valid = saved = false; q = Q_UNKNOWN; }
  void set_track_theta(bool on) { track_theta = on; kuu_valid = false; q = Q_UNKNOWN; }      // (`prepared` stands: theta did not move)
  // a natural-gradient step wrote layer l's (q_mu, q_sqrt).  Z and the kernel hyper-parameters are untouched: kuu_valid stays
  void q_moved(int l) {
    prepared = saved = false;
    const bool alone = q == Q_NONE || (q == Q_ONE && q_layer == l);      // a second layer: unknown
    q = alone ? Q_ONE : Q_UNKNOWN;
    q_layer = alone ? l : -1;
  }
  void workspace_overwritten() { saved = false; }
  void saved_recorded(int64_t n, int S) { saved = true; saved_n = n; saved_S = S; }
  void saved_consumed() { saved = false; }      // also by a reverse pass that fails half-way
  void grad_evaluated(bool pruned) { grad_pruned = pruned; }
  inline void prepare_done(const PrepPlan& p);
};

// The call and the model, as plain values.  blocked: bit l set = layer l takes the multi-workgroup blocked factorisation
struct PrepIn {
  bool with_grad, side;      // the gradient-side products are wanted; the parameter-only part goes to the side stream
  int L;
  bool white;
  int grad_first;
  bool head_ok, uniform_big;
  uint32_t blocked;
  int mp_max, big_mp;
  bool ext_ev;      // DSDGP_FORCE ext_ev: the head launch may carry the fork event
};

enum PrepFactor : uint8_t {
  FACTOR_NONE,            // Z and the kernel hyper-parameters are those of the previous evaluation: Lu, Lu^-1, log det stay
  FACTOR_IN_HEAD,         // inside the head launch (which skips it itself under keep_kuu)
  FACTOR_BATCHED_BLOCKED, // all layers share M: ONE batched multi-workgroup Cholesky
  FACTOR_PER_LAYER,       // layer by layer: blocked where PrepPlan::blocked says so, else the one-workgroup kernel
  FACTOR_ONE_WG_BATCH     // one launch of the one-workgroup kernel for all layers
};
enum PrepRedo : uint8_t { REDO_NONE, REDO_LAYER, REDO_FROM, REDO_ALL };      // nothing / layer `*_layer` alone / layers `*_layer`..L-1 / all
struct PrepPlan {
  bool head;             // the head launch runs — also when nothing changed: it carries the draws and the gather
  bool keep_kuu;         //   ... its / k_prep_kuu's keep_kuu argument
  bool prep_kuu;         // k_prep_kuu runs (parameter transforms) ...
  bool kuu_blocks;       //   ... with the Ku blocks in its grid
  PrepFactor factor;
  uint32_t blocked;
  bool early;            // nothing changed: the call returns right after the factor
  bool fork;             // the side stream waits for ev_fork and takes the rest ...
  bool fork_on_head;     //   ... which the head launch carries (no record of its own)
  PrepRedo fwd; int fwd_layer;       // forward side: Ku^-1, Lu^-1 q_sqrt, Lu^-1 q_mu, S_d, KL partials (REDO_NONE / _LAYER / _ALL)
  PrepRedo grad; int grad_layer;     // gradient side: U_d, n, U_d U_d^T
  bool rec_kinv, rec_prep_side;      // ev_kinv behind the forward side, ev_prep_side behind everything, both on the side stream
  bool grad_all;         // prepared_grad afterwards
};

// Forward and gradient side are decided separately: after a natural-gradient step on layer lf the forward side of every other layer is
// still that of the previous evaluation, whatever that evaluation did on the gradient side (a pruned natural-gradient evaluation leaves
// the lower layers' U_d undone: the Adam evaluation that follows redoes the gradient side of ALL layers, but the forward side of layer lf
// only — it used to redo all 17 Lu^-1 q_sqrt_d of a config-5 model as well)
static inline PrepPlan prep_plan(const ParamState& s, const PrepIn& in) {
  PrepPlan p{};
  const bool keep = s.track_theta && s.kuu_valid;
  const bool grad_ok = s.prepared_grad || !in.with_grad;      // the previous evaluation produced every gradient-side product this one needs
  // no change since an evaluation that produced everything this one needs: the factor AND the parameter-side products (Ku^-1,
  // Lu^-1 q_sqrt, KL, ...) stay — a forward-only evaluation at fixed parameters is the chains alone
  p.early = keep && s.q == ParamState::Q_NONE && grad_ok;
  p.keep_kuu = keep;
  p.head = in.head_ok;
  p.prep_kuu = !in.head_ok && !p.early;
  p.kuu_blocks = p.prep_kuu && !keep;
  p.factor = in.head_ok ? FACTOR_IN_HEAD
           : keep ? FACTOR_NONE
           : in.uniform_big ? FACTOR_BATCHED_BLOCKED
           : in.mp_max >= in.big_mp ? FACTOR_PER_LAYER : FACTOR_ONE_WG_BATCH;
  p.blocked = in.blocked;
  p.fork_on_head = in.head_ok && in.side && in.ext_ev;
  if (p.early) return p;
  p.fork = in.side;
  // only layer lf's (q_mu, q_sqrt) moved since an evaluation that left everything else current: its products alone
  const int lf = (keep && s.q == ParamState::Q_ONE) ? s.q_layer : -1;
  if (keep && s.q == ParamState::Q_NONE) p.fwd = REDO_NONE;      // (the last evaluation lacked the gradient side only)
  else if (lf >= 0) { p.fwd = REDO_LAYER; p.fwd_layer = lf; }
  else p.fwd = REDO_ALL;
  const bool grad = in.with_grad && !in.white;      // white = True has no gradient-side products
  const int gfirst = grad ? in.grad_first : 0;
  if (!grad) p.grad = REDO_NONE;
  else if (lf >= 0 && grad_ok) { p.grad = REDO_LAYER; p.grad_layer = lf; }
  else if (gfirst > 0) { p.grad = REDO_FROM; p.grad_layer = gfirst; }
  else p.grad = REDO_ALL;
  p.rec_kinv = in.side && grad;
  p.rec_prep_side = in.side;
  p.grad_all = in.with_grad && gfirst == 0;      // (a partial prepare with_grad required the previous one to have had it)
  return p;
}

inline void ParamState::prepare_done(const PrepPlan& p) {
  prepared = true;
  if (p.early) return;      // everything else stands as it was
  prepared_grad = p.grad_all;
  kuu_valid = true;
  q = Q_NONE; q_layer = -1;
}
